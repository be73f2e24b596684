"""idfcodec -- MI355X-native (gfx950) integer-discrete-flow + rANS lossless image codec.

Native core: libidfcodec.so (HIP, C ABI in include/idf_codec.h).  This package
holds the host side: ctypes binding (_lib), weight packing (packing), the flow
engine (engine), the batched coder and bitstream container (codec), the
synthetic-weight recipe (synthetic), the multi-GPU shard/gather (dist), the
residual configs' codec (residual, vq), the TwoLevelFlows codec (twolevel) and the
codec of images of any size as tiles of a flow's input (tiled: TiledCodec,
TiledBitstream, exported here) with its raw-tile escape (safe: SafeTiledCodec,
SafeTiledBitstream, exported here), the predictive coder of the escaped tiles (predict:
PredictiveTileCodec, PredictiveTiledBitstream, exported here) and the seal of all three
(integrity: SealedCodec, SealedBitstream, exported here: a CRC-32 per tile and the model's
fingerprint), and the codec of images of another channel count than the model's -- grey, grey +
alpha, RGBA -- around any of the first three (planes: PlaneSetCodec, PlaneSetBitstream, exported
here), and the model-free codec of 16-bit images (deep: DeepTiledCodec, DeepTiledBitstream,
deep_section_bound, exported here).
"""
import os
import sys

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG_ROOT not in sys.path:
    # the reference-API mirror modules (flows, coder, rans, ...) live next to this package
    sys.path.insert(0, _PKG_ROOT)

__version__ = "0.1.0"

__all__ = ["DeepTiledBitstream", "DeepTiledCodec", "deep_section_bound", "PlaneSetBitstream",
           "PlaneSetCodec", "PredictiveTileCodec", "PredictiveTiledBitstream", "SafeTiledBitstream", "SafeTiledCodec", "SealedBitstream",
           "SealedCodec", "TiledBitstream", "TiledCodec"]


def __getattr__(name):
    # resolved on first use: importing the package alone stays free of torch
    if name in __all__:
        if name.startswith(("Deep", "deep_")):
            from . import deep
            return getattr(deep, name)
        if name.startswith("PlaneSet"):
            from . import planes
            return getattr(planes, name)
        if name.startswith("Predictive"):
            from . import predict
            return getattr(predict, name)
        if name.startswith("Safe"):
            from . import safe
            return getattr(safe, name)
        if name.startswith("Sealed"):
            from . import integrity
            return getattr(integrity, name)
        from . import tiled
        return getattr(tiled, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
