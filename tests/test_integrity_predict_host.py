"""The seal around the predictive containers on the host (no device): IDFC around hand-made IDFP
and IDFQ bitstreams -- plain, colour and interleaved -- byte for byte, the refusals that concern
the inner file, the pairing rule of SealedCodec, and the file tool's reader."""
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import REPO
from test_integrity_host import CRCS, FP, _safe, _sealed, _tiled
from test_predict_colour_host import _col
from test_predict_host import MIXED, PACKED, _pred
from test_predict_ways_host import _ways

INNERS = {"idfp": (lambda: _pred(MIXED, PACKED), b"IDFP", 0),
          "idfq": (lambda: _col(), b"IDFQ", 0),
          "idfp_8_ways": (lambda: _ways(_pred(MIXED, PACKED), 8), b"IDFP", 8),
          "idfq_8_ways": (lambda: _ways(_col(), 8), b"IDFQ", 8),
          "idfp_nothing_kept": (lambda: _pred([True] * 6, [True, False] * 3), b"IDFP", 0),
          "idfp_nothing_escaped": (lambda: _pred([False] * 6, [False] * 6), b"IDFP", 0)}


@pytest.mark.parametrize("name", INNERS)
def test_idfc_around_a_predictive_file_round_trips_byte_for_byte(name):
    from idfcodec.integrity import SealedBitstream
    from idfcodec.predict import PredictiveTiledBitstream
    make, magic, flags = INNERS[name]
    inner = make()
    body = inner.to_bytes()
    assert body[:4] == magic and struct.unpack_from("<H", body, 6)[0] == flags
    buf = _sealed(inner).to_bytes()
    # the header is the one IDFT and IDFS files get: version 1, flags 0, nothing added
    head = (struct.pack("<4sHHII", b"IDFC", 1, 0, FP, 6) + struct.pack("<6I", *CRCS)
            + struct.pack("<Q", len(body)))
    assert buf == head + struct.pack("<I", zlib.crc32(head)) + body
    assert len(buf) == len(body) + 28 + 4 * 6
    back = SealedBitstream.from_bytes(buf)
    assert type(back.inner) is PredictiveTiledBitstream and back.inner.to_bytes() == body
    assert back.inner.predict_ways == (flags or 1)
    assert (back.inner.colour is not None) == (magic == b"IDFQ")
    assert back.crc.dtype == np.uint32 and back.crc.tolist() == CRCS and back.fingerprint == FP
    assert back.to_bytes() == buf and back.layout.n_tiles == 6


@pytest.mark.parametrize("name", ["idfp", "idfq_8_ways"])
def test_refusals_that_concern_the_inner_file(name):
    from idfcodec.integrity import SealedBitstream
    inner = INNERS[name][0]()
    raw = _sealed(inner).to_bytes()
    o_inner = 16 + 24 + 12
    n_inner = len(raw) - o_inner
    # five CRCs before an inner file of six tiles
    head = (struct.pack("<4sHHII", b"IDFC", 1, 0, FP, 5) + struct.pack("<5I", *CRCS[:5])
            + struct.pack("<Q", n_inner))
    with pytest.raises(ValueError, match="5 tile CRCs, its inner file 6"):
        SealedBitstream.from_bytes(head + struct.pack("<I", zlib.crc32(head)) + raw[o_inner:])
    with pytest.raises(ValueError, match="5 tile CRCs for 6"):
        SealedBitstream(inner, np.array(CRCS[:5], dtype=np.uint32), FP).to_bytes()
    # an IDFB stream is no tiled file, as before
    with pytest.raises(ValueError, match="unknown magic"):
        SealedBitstream.from_bytes(raw[:o_inner] + b"IDFB" + raw[o_inner + 4:])
    # inner damage is the inner reader's to report: flags that name no number of ways
    b = bytearray(raw)
    struct.pack_into("<H", b, o_inner + 6, 5)
    with pytest.raises(ValueError, match="flags"):
        SealedBitstream.from_bytes(bytes(b))


def test_existing_sealed_files_keep_their_bytes():
    """test_integrity_host.test_idfc_bytes_are_frozen pins the digests; here the reader still
    returns the same kinds."""
    from idfcodec.integrity import SealedBitstream
    from idfcodec.safe import SafeTiledBitstream
    from idfcodec.tiled import TiledBitstream
    for make, kind in ((_tiled, TiledBitstream), (_safe, SafeTiledBitstream)):
        buf = _sealed(make()).to_bytes()
        back = SealedBitstream.from_bytes(buf)
        assert type(back.inner) is kind and back.to_bytes() == buf


def _tiny_model():
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    return synthetic.build_model(_flows("IDFlows", 2, 2, 16, 16, 3, _dense(24, 3), _dense(16, 2),
                                        2))


def test_codec_and_inner_file_pair_by_exact_kind():
    """_open's first check runs on the host: each of the three codecs takes its own bitstream
    and refuses the other two with a ValueError that names both."""
    from idfcodec.integrity import SealedCodec
    from idfcodec.predict import PredictiveTileCodec
    from idfcodec.safe import SafeTiledCodec
    from idfcodec.tiled import TiledCodec
    model = _tiny_model()
    files = {"TiledBitstream": _sealed(_tiled()), "SafeTiledBitstream": _sealed(_safe()),
             "PredictiveTiledBitstream": _sealed(_pred(MIXED, PACKED)),
             "PredictiveTiledBitstream (IDFQ)": _sealed(_col())}
    codecs = {"TiledBitstream": TiledCodec(model), "SafeTiledBitstream": SafeTiledCodec(model),
              "PredictiveTiledBitstream": PredictiveTileCodec(model)}
    for want, codec in codecs.items():
        zc = SealedCodec(codec)
        for kind, zbs in files.items():
            if kind.split(" ")[0] == want:
                continue
            with pytest.raises(ValueError) as err:
                zc._open(zbs, check_model=False)
            assert type(zbs.inner).__name__ in str(err.value)
            assert type(codec).__name__ in str(err.value)
    # its own kind passes the pairing: IDFP and IDFQ alike, at the file's own ways
    zc = SealedCodec(codecs["PredictiveTiledBitstream"])
    for inner in (_pred(MIXED, PACKED), _col(), _ways(_col(), 8)):
        assert zc._open(_sealed(inner), check_model=False) is None


def test_tiled_safe_takes_seal_and_tiled_sealed_keeps_its_signature():
    import inspect
    from flows import IDFlows
    assert list(inspect.signature(IDFlows.tiled_safe).parameters) == [
        "self", "max_batch", "ways", "predict", "predict_ways", "seal"]
    assert inspect.signature(IDFlows.tiled_safe).parameters["seal"].default is False
    assert list(inspect.signature(IDFlows.tiled_sealed).parameters) == [
        "self", "max_batch", "ways", "safe"]


def test_file_tool_reads_sealed_predictive_files_by_their_inner_magic():
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from idfcodec.integrity import SealedBitstream
    from idfcodec.predict import PredictiveTiledBitstream
    for name, (make, _, _) in INNERS.items():
        inner = make()
        buf = _sealed(inner).to_bytes()
        got, escape, sealed = tool.read_file(buf, None)
        assert (type(got), escape, sealed) == (SealedBitstream, True, True), name
        assert type(got.inner) is PredictiveTiledBitstream and got.to_bytes() == buf
        got, escape, sealed = tool.read_file(inner.to_bytes(), None)
        assert type(got) is PredictiveTiledBitstream and escape and not sealed
    # the other kinds as before
    assert tool.read_file(_sealed(_tiled()).to_bytes(), None)[1:] == (False, True)
    assert tool.read_file(_sealed(_safe()).to_bytes(), None)[1:] == (True, True)
