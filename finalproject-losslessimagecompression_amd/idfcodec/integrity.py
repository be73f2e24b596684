"""Sealed tiled files: a CRC-32 of every tile's source bytes and a fingerprint of the model,
around an IDFT (idfcodec.tiled), IDFS (idfcodec.safe) or IDFP / IDFQ (idfcodec.predict) file that
stays byte for byte what its own codec writes.

The checksum is zlib's crc32.  It is computed on the device, from the bytes where they already
lie (csrc/crc_kernels.hip; csrc/idf_crc.h states the identity that lets a GPU sum a run in
parts):

encode: SealedCodec.encode is the wrapped codec's encode plus one idf_tile_crc32_u8 launch over
        the sources' tile table: crc[e] is the CRC-32 of entry e's in-image rectangle as bytes
        [C][hin][win], what idf_tile_gather_raw_u8 would store for it.
decode: a tile the flow decodes is summed by idf_tile_crc32_pm on each chunk's pixel-major rows,
        right where the scatter reads them; a tile stored raw by idf_crc32_segments_u8 over its
        stored run; a tile the predictor decodes by idf_crc32_segments_u8 over its run of the
        dense buffer the predictive decoders fill, after the launch that leaves the source bytes
        there (a colour entry's inverse transform included).  The sums are compared with the
        recorded ones on the device.  Only the tiles a call decodes are checked; info['crc_bad']
        lists the entries among them that did not come back, in entry order, and the outputs are
        returned in full, so a caller can keep the sound tiles.
model:  model_fingerprint is one idf_crc32_segments_u8 launch over every state_dict() tensor,
        folded on the host with each tensor's key, dtype, shape and byte count and with the
        model's idf_precision.  It is cached on the engine, which IDFlows.engine() rebuilds when
        a parameter changes.  decode refuses a file another fingerprint wrote before it decodes
        anything (check_model=False: decode anyway).

Container IDFC (little-endian): magic "IDFC", u16 version 1, u16 flags 0, u32 fingerprint, u32
n_tiles, n_tiles x u32 CRC-32 (entry order), u64 inner length, u32 CRC-32 (zlib) of every byte
before it, the inner IDFT, IDFS, IDFP or IDFQ file, told apart by its magic: 28 + 4 * n_tiles
bytes above the inner file.  The colour mode and predict_ways of an IDFP / IDFQ file do not touch
the CRCs: they are taken over the source bytes.  This is a check against damage and mix-ups, not
against forgery.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, predict, safe, tiled
from ._lib import check, lib, ptr
from .codec import RANS_L, streams_ok
from .dist import _to_device
from .tiled import _check_table, _entry

MAGIC = b"IDFC"
VERSION = 1
NAME = "sealed bitstream"
_HDR = "<4sHHII"
OVERHEAD = struct.calcsize(_HDR) + 8 + 4        # 28, + 4 per tile


# ------------------------------------------------------------------ device calls
def _check_crc(out: torch.Tensor, n: int):
    _lib.require_device(out, "CRC output")
    if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < n:
        raise ValueError("the CRC output is contiguous int32 [n] (the bits of uint32 values)")


def device_crc32_segments(table: torch.Tensor, n: int, out: torch.Tensor):
    """table: device int64 [>= n, 2] rows (address, n_bytes) -> out[k], int32 holding the bits
    of the CRC-32 of that byte run (idf_crc32_segments_u8)."""
    _lib.require_device(table, "segment table")
    if table.dtype != torch.int64 or not table.is_contiguous() or table.numel() < n * 2:
        raise ValueError("segment table must be contiguous int64 [n, 2]")
    _check_crc(out, n)
    check(lib().idf_crc32_segments_u8(_lib.stream_ptr(out.device), n, ptr(table), ptr(out)),
          "crc32 segments")


def device_tile_crc32(table: torch.Tensor, n: int, C: int, th: int, tw: int, out: torch.Tensor):
    """out[t]: the CRC-32 of the in-image bytes [C][hin][win] of the tile the table row
    (addr, H, W, y0, x0) names (idf_tile_crc32_u8), or the row of eight fields with its byte
    strides (idf_tile_crc32_strided_u8)."""
    fields = _check_table(table, n)
    _check_crc(out, n)
    check(_entry("idf_tile_crc32_u8", fields)(_lib.stream_ptr(out.device), n, C, th, tw,
                                              ptr(table), ptr(out)), "tile crc32")


def device_tile_crc32_pm(src: torch.Tensor, n: int, C: int, th: int, tw: int, rect: torch.Tensor,
                         out: torch.Tensor, ld: int = 4):
    """out[t]: the CRC-32 of the bytes idf_tile_scatter_u8 writes for the in-image part rect[t] =
    (hin, win) of tile t of the pixel-major float32 rows src (idf_tile_crc32_pm)."""
    _lib.require_device(src, "tile buffer")
    _lib.require_device(rect, "tile rectangles")
    if src.dtype != torch.float32 or src.numel() < n * th * tw * ld:
        raise ValueError("crc input must be float32 and hold n * th * tw * ld values")
    if rect.dtype != torch.int32 or not rect.is_contiguous() or rect.numel() < 2 * n:
        raise ValueError("tile rectangles must be contiguous int32 [n_tiles, 2]")
    _check_crc(out, n)
    check(lib().idf_tile_crc32_pm(_lib.stream_ptr(out.device), n, C, th, tw, ptr(src), ld,
                                  ptr(rect), ptr(out)), "tile crc32 pm")


def _u32(t: torch.Tensor) -> np.ndarray:
    """A device int32 CRC tensor as host uint32 (a stream sync)."""
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ the model's fingerprint
def model_fingerprint(model) -> int:
    """A CRC-32 over every state_dict() tensor's bytes (one device launch), key, dtype, shape
    and byte count, in order, and over idf_precision: what a sealed file records of the weights
    that wrote it.  Cached on model.engine(), so computed once per set of weights."""
    return _engine_fingerprint(model, model.engine())


def _engine_fingerprint(model, eng) -> int:
    """model_fingerprint for a caller that holds model.engine() already: the lookup walks every
    parameter, so a call makes it once."""
    fp = getattr(eng, "_fingerprint", None)
    if fp is None:
        fp = eng._fingerprint = _fingerprint(model, torch.device(eng.device))
    return fp


def _fingerprint(model, dev) -> int:
    state = [(k, v.detach()) for k, v in model.state_dict().items()]
    held = []
    for k, v in state:
        _lib.require_device(v, f"state tensor {k}")
        held.append(v if v.is_contiguous() else v.contiguous())
    rows = [(v.data_ptr() if v.numel() else 0, v.numel() * v.element_size()) for v in held]
    crcs = np.zeros(0, dtype=np.uint32)
    if rows:
        table = _to_device(torch.tensor(rows, dtype=torch.int64).reshape(-1, 2), dev)
        out = torch.empty(len(rows), dtype=torch.int32, device=dev)
        device_crc32_segments(table, len(rows), out)
        crcs = _u32(out)                # the sync: `held` outlives the launch
    h = zlib.crc32(b"IDFM\x01")
    for (k, v), (_, nbytes), crc in zip(state, rows, crcs):
        h = zlib.crc32(k.encode() + b"\0" + str(v.dtype).encode() + b"\0"
                       + struct.pack(f"<I{v.dim()}q", v.dim(), *v.shape)
                       + struct.pack("<qI", nbytes, int(crc)), h)
    return zlib.crc32(str(getattr(model, "idf_precision", "f32")).encode(), h)


# ------------------------------------------------------------------ container
@dataclass
class SealedBitstream:
    inner: object               # a Tiled-, SafeTiled- or PredictiveTiledBitstream, untouched
    crc: np.ndarray             # uint32 [N], entry order: CRC-32 of every tile's source bytes
    fingerprint: int            # model_fingerprint of the weights that wrote it

    @property
    def layout(self):
        return self.inner.layout

    def to_bytes(self) -> bytes:
        crc = np.ascontiguousarray(self.crc, dtype="<u4")
        N = self.inner.layout.n_tiles
        if crc.shape != (N,):
            raise ValueError(f"{crc.size} tile CRCs for {N} tiles")
        inner = self.inner.to_bytes()
        head = (struct.pack(_HDR, MAGIC, VERSION, 0, int(self.fingerprint) & 0xFFFFFFFF, N)
                + crc.tobytes() + struct.pack("<Q", len(inner)))
        return head + struct.pack("<I", zlib.crc32(head)) + inner

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "SealedBitstream":
        buf = bytes(buf)
        n_hdr = struct.calcsize(_HDR)
        if len(buf) < n_hdr:
            raise ValueError(f"truncated {NAME} (header)")
        magic, ver, flags, fp, N = struct.unpack_from(_HDR, buf, 0)
        if magic != MAGIC:
            raise ValueError(f"not an IDF {NAME}")
        if ver != VERSION:
            raise ValueError(f"unknown {NAME} version {ver}")
        if flags:
            raise ValueError(f"unknown {NAME} flags {flags:#x}")
        o = n_hdr + 4 * N
        if len(buf) < o + 12:
            raise ValueError(f"truncated {NAME} (tile CRCs)")
        (length,) = struct.unpack_from("<Q", buf, o)
        (want,) = struct.unpack_from("<I", buf, o + 8)
        if zlib.crc32(buf[:o + 8]) != want:
            raise ValueError(f"{NAME}: the header's CRC does not match (a damaged header)")
        crc = np.frombuffer(buf, "<u4", N, n_hdr).astype(np.uint32)
        o += 12
        if len(buf) != o + length:
            raise ValueError(f"{NAME} holds {len(buf) - o} inner bytes, its header names "
                             f"{length}")
        body = buf[o:]
        if body[:4] == tiled.MAGIC:
            inner = tiled.TiledBitstream.from_bytes(body, device=device)
        elif body[:4] == safe.MAGIC:
            inner = safe.SafeTiledBitstream.from_bytes(body, device=device)
        elif body[:4] in (predict.MAGIC, predict.MAGIC_COLOUR):
            inner = predict.PredictiveTiledBitstream.from_bytes(body, device=device)
        else:
            raise ValueError(f"{NAME} holds an inner file of unknown magic {body[:4]!r}")
        if inner.layout.n_tiles != N:
            raise ValueError(f"{NAME} holds {N} tile CRCs, its inner file {inner.layout.n_tiles} "
                             "tiles")
        return cls(inner, crc, fp)


# ------------------------------------------------------------------ one decode call's check
class _Check:
    """The CRC check of one decode call: handed down TiledCodec._decode_entries /
    SafeTiledCodec._decode_entries / PredictiveTileCodec._decode_entries /
    TiledCodec._decode_tiles as `seal`, which call back where the decoded bytes lie.  Slot s of
    `got` is the tile at position order[s] of the call's entries: the flow-decoded ones first,
    in the order their chunks run, then the raw ones, then the ones the predictor decodes."""

    def __init__(self, C, tile_hw, rects, entries, want: np.ndarray, dev, ic=None):
        self.C, (self.th, self.tw) = C, tile_hw
        self.entries = list(entries)
        self.rects = [rects[e] for e in self.entries]
        self.want = np.asarray(want, dtype=np.uint32)[self.entries] if self.entries else \
            np.zeros(0, dtype=np.uint32)
        self.dev = dev
        self.ic = ic                # the ImageCodec already looked up for the model check
        self.got = torch.empty(len(self.entries), dtype=torch.int32, device=dev)
        self.packed, self._within = [], None
        self.split(list(range(len(self.entries))), [])

    def within(self, positions):
        """The entries handed further down are these positions of the call's entries: split then
        receives positions among them (PredictiveTileCodec hands SafeTiledCodec only the entries
        that are not packed)."""
        self._within = list(positions)

    def split(self, kept, raw):
        """kept, raw: the positions of the call's entries the flow decodes / that are stored."""
        if self._within is not None:
            kept, raw = ([self._within[k] for k in kept], [self._within[k] for k in raw])
        self.kept, self.raw = list(kept), list(raw)
        self._rect = None

    def kept_chunk(self, k: int, m: int, buf: torch.Tensor):
        """buf holds the pixel-major rows of kept tiles k .. k + m."""
        if self._rect is None:
            self._rect = _to_device(torch.tensor([self.rects[p] for p in self.kept],
                                                 dtype=torch.int32).reshape(-1, 2), self.dev)
        device_tile_crc32_pm(buf, m, self.C, self.th, self.tw, self._rect[k:k + m],
                             self.got[k:k + m])

    def raw_runs(self, raw: torch.Tensor, offs):
        """offs[j]: the byte offset in raw of the stored bytes of raw tile j."""
        base = raw.data_ptr()
        rows = [(base + o, self.C * self.rects[p][0] * self.rects[p][1])
                for o, p in zip(offs, self.raw)]
        table = _to_device(torch.tensor(rows, dtype=torch.int64).reshape(-1, 2), self.dev)
        device_crc32_segments(table, len(rows), self.got[len(self.kept):])

    def packed_rows(self, packed, base: int, offs) -> np.ndarray:
        """packed: the positions of the call's entries the predictor decodes, whose bytes will
        lie at base + offs[j] -> the rows (address, n_bytes) of their runs, int64 [2 n], for the
        caller to copy to the device with its own tables."""
        self.packed = list(packed)
        rows = [(base + int(o), self.C * self.rects[p][0] * self.rects[p][1])
                for o, p in zip(offs, self.packed)]
        return np.asarray(rows, dtype=np.int64).reshape(-1)

    def packed_runs(self, table: torch.Tensor):
        """table: packed_rows on the device; the predictive decode that fills the runs is
        queued."""
        device_crc32_segments(table, len(self.packed),
                              self.got[len(self.kept) + len(self.raw):])

    def finish(self, info: dict, verify: bool) -> dict:
        order = self.kept + self.raw + self.packed
        n = len(order)
        if verify:
            want = _to_device(torch.from_numpy(self.want[order].view(np.int32).copy()), self.dev)
            differs = (self.got != want).cpu().numpy() if n else np.zeros(0, dtype=bool)
            # the one wait of the call; the reads below find the stream drained
            info["crc_bad"] = sorted(self.entries[order[s]] for s in np.flatnonzero(differs))
            info["ok"] = (not info["crc_bad"] and int(info["off_grid"].item()) == 0
                          and streams_ok(info["final_states"], info["status"]))
            if self.packed:     # one final state per packed entry and way, as the unsealed decode
                info["ok"] = (info["ok"] and not bool(info["packed_status"].any().item()) and
                              bool((info["packed_final_states"] == RANS_L).all().item()))
        else:
            info["crc"] = self.got
            if order != list(range(n)):     # tiles of several kinds: back into the call's order
                inv = np.empty(n, dtype=np.int64)
                inv[order] = np.arange(n)
                info["crc"] = self.got[_to_device(torch.from_numpy(inv), self.dev)]
            info["crc_entries"] = list(self.entries)
        return info


# ------------------------------------------------------------------ codec
# the bitstream each codec reads, the most derived codec first
_PAIRS = ((predict.PredictiveTileCodec, predict.PredictiveTiledBitstream),
          (safe.SafeTiledCodec, safe.SafeTiledBitstream),
          (tiled.TiledCodec, tiled.TiledBitstream))


class SealedCodec:
    """A TiledCodec, SafeTiledCodec or PredictiveTileCodec whose files carry a CRC-32 per tile
    and the model's fingerprint (the module's doc has the flow).  encode's keywords are the
    wrapped codec's, layout included (a PredictiveTileCodec's choose and shortlist too);
    decode's layout and out are TiledCodec.decode's."""

    def __init__(self, codec):
        if not isinstance(codec, tiled.TiledCodec):
            raise TypeError(f"SealedCodec wraps a TiledCodec, a SafeTiledCodec or a "
                            f"PredictiveTileCodec, not {type(codec).__name__}")
        self.codec = codec
        self.model = codec.model
        self.C, self.tile_hw = codec.C, codec.tile_hw

    @property
    def max_batch(self) -> int:
        return self.codec.max_batch

    @property
    def ways(self) -> int:
        return self.codec.ways

    @torch.no_grad()
    def encode(self, images, layout=None, **kw) -> SealedBitstream:
        inner = self.codec.encode(images, layout=layout, **kw)
        # the wrapped encode has just looked the engine up (IDFlows.codec() walks every
        # parameter: 1.7 ms for imagenet64), so it is current; not a second walk
        eng = self.model._engine or self.model.engine()
        dev = torch.device(eng.device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        images, lay, rows = self.codec._sources(images, dev, layout)
        crc = torch.empty(lay.n_tiles, dtype=torch.int32, device=dev)
        device_tile_crc32(self.codec._device_table(rows, dev), lay.n_tiles, self.C,
                          *self.tile_hw, crc)
        return SealedBitstream(inner, _u32(crc), _engine_fingerprint(self.model, eng))

    # -------------------------------------------------------------- decode
    def _open(self, sbs: SealedBitstream, check_model: bool):
        """The checks that precede every decode -> the ImageCodec looked up for them, or None."""
        if not isinstance(sbs, SealedBitstream):
            raise TypeError(f"SealedCodec decodes a SealedBitstream, not {type(sbs).__name__}")
        # codec and inner file pair by exact kind; an IDFP and an IDFQ file go alike
        want = next(b for c, b in _PAIRS if isinstance(self.codec, c))
        if type(sbs.inner) is not want:
            raise ValueError(f"{NAME} holds a {type(sbs.inner).__name__}, the codec is a "
                             f"{type(self.codec).__name__}")
        self.codec.check_bitstream(sbs.inner)
        if len(sbs.crc) != sbs.inner.layout.n_tiles:
            raise ValueError(f"{NAME} holds {len(sbs.crc)} tile CRCs for "
                             f"{sbs.inner.layout.n_tiles} tiles")
        if not check_model:
            return None
        ic = self.model.codec()
        fp = _engine_fingerprint(self.model, ic.engine)
        if fp != sbs.fingerprint:
            raise ValueError(f"{NAME} was written by a model of fingerprint "
                             f"{sbs.fingerprint:#010x}, this model's is {fp:#010x} (other "
                             "weights or precision; check_model=False decodes anyway)")
        return ic

    def _run(self, sbs, ic, entries, rows, verify, dev):
        lay = sbs.inner.layout
        seal = _Check(self.C, self.tile_hw, lay.rects, entries, sbs.crc, dev, ic)
        info = self.codec._decode_entries(sbs.inner, entries, rows, False, seal=seal)
        return seal.finish(info, verify)

    @torch.no_grad()
    def decode(self, sbs, images=None, verify: bool = True, check_model: bool = True,
               layout: str = "chw", out=None):
        """-> (list of uint8 [C, H_i, W_i], info) as TiledCodec.decode; info['crc_bad']: the
        entries decoded whose bytes are not the ones encoded (verify=False: info['crc'], the
        sums of info['crc_entries'] on the device, no wait)."""
        ic = self._open(sbs, check_model)
        lay = sbs.inner.layout
        want, entries, rows = lay.image_rows(images)
        outs, addrs, strides = self.codec._outputs([(self.C, *lay.sizes[i]) for i in want],
                                                   layout, out)
        rows = lay.place(rows, addrs, strides)
        return outs, self._run(sbs, ic, entries, rows, verify, self.codec._device())

    @torch.no_grad()
    def decode_region(self, sbs, image: int, y0: int, x0: int, h: int, w: int,
                      verify: bool = True, check_model: bool = True, layout: str = "chw",
                      out=None):
        """-> (uint8 [C, h, w], info) as TiledCodec.decode_region; the tiles the region touches
        are checked whole."""
        ic = self._open(sbs, check_model)
        lay = sbs.inner.layout
        entries, rows = lay.region_rows(image, y0, x0, h, w)
        outs, addrs, strides = self.codec._outputs([(self.C, int(h), int(w))], layout,
                                                   None if out is None else [out])
        return outs[0], self._run(sbs, ic, entries, lay.place(rows, addrs, strides), verify,
                                  self.codec._device())


def bad_tiles(sbs: SealedBitstream, crc_bad) -> list:
    """info['crc_bad'] as [(image, tile row, tile column)]."""
    ent = sbs.inner.layout.entries
    return [ent[e] for e in crc_bad]


__all__ = ["MAGIC", "VERSION", "OVERHEAD", "SealedBitstream", "SealedCodec", "bad_tiles",
           "device_crc32_segments", "device_tile_crc32", "device_tile_crc32_pm",
           "model_fingerprint"]
