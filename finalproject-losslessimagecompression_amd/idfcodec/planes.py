"""Plane sets: images whose channel count is not the model's -- grey, grey + alpha, RGBA, more.

A source of Cs channels is split against a model of C channels.  With Cs >= C its first C
channels are the *base planes* (Cb = C): they go to a tiled codec of the model (TiledCodec,
SafeTiledCodec or PredictiveTileCodec, the *base*) as [:Cb] views of the source, so interleaved
RGBA is read where it lies, with pixel stride 4.  The other Ce = Cs - Cb channels are *extra
planes*.  With Cs < C no flow runs: Cb = 0 and every channel is an extra plane.

The extra planes are tiled as the base tiles its planes: TileLayout(sizes, ., the model's tile),
the same entries in the same order.  A *unit* is one extra plane of one entry's in-image
rectangle, uint8 [hin][win]; unit u = entry * Ce + plane.  A unit is coded on its own, from its
own bytes alone, in the first class that holds (unit_class):

  constant  min == max over its bytes; one byte is stored;
  packed    its predictive stream -- idfcodec.predict's coder at C = 1, plain mode -- has status 0
            and entry_overhead(ways) + 4 * nwords < hin * win (predict.is_packed; a tie stores
            raw): sel, the state or states, the word count and the words are stored;
  raw       its bytes are stored.

The constant class is what makes alpha affordable: the predictor's sharpest scale gives a
perfectly predicted symbol sigma(1) - sigma(-1) = 0.462 of the range, 1.11 bits, so an opaque
64 x 64 alpha tile would cost about 570 bytes as a packed unit and costs one byte here.

encode: one idf_tile_gather_raw(_strided)_u8 launch at C = 1 over a table of one row a unit
copies the units into a dense staging buffer (it is also where the raw class's bytes come from);
idf_segment_range_u8 gives every unit's smallest and largest byte; device_predict_encode codes the
units that are not constant, at most SYMBOLS_PER_PASS symbols a pass, from five-field rows naming
the staging buffer.  decode: idf_segment_fill_u8 writes the wanted constants and
idf_predict_decode_u8 (idf_predict_decode_ways_u8 for N-way files) the wanted packed units into
one dense buffer, the wanted raw units are copied next to them, and one
idf_tile_scatter_raw(_strided)_u8 launch at C = 1 over a table of one row a unit writes them into
channel Cb + plane of the outputs, through the outputs' own strides.  The base decodes into the
[:Cb] views of the same outputs.

Container IDFM (little-endian):

  magic "IDFM", u16 version 1, u16 flags (predict_ways where it is > 1, else 0)
  u32 n_images, u32 Cs, u32 Cb, u32 tile_h, u32 tile_w, n_images x (u32 H, u32 W)
  u64 base length, the base codec's file untouched (IDFT, IDFS, IDFP or IDFQ over Cb channels;
      length 0 and absent when Cb == 0)
  the constant bitmap: U = N * Ce bits in unit order, LSB first, ceil(U / 8) bytes
  the packed bitmap: U - K bits over the units that are not constant, ceil((U - K) / 8) bytes
  the K constants, one byte each, in unit order
  u64 raw length, the raw units' bytes in unit order
  u64 packed-section length, the packed section: u32 P, u32 sel[P], u64 state[P] (N-way files:
      [P][N], unit-major and way-minor), u32 nwords[P], the words as u32 in unit order and push
      order

so the plane section (everything behind the base file) is at most plane_section_bound: a constant
unit's byte, a packed unit's fields and words and a raw unit's bytes are each at most the unit's
bytes.  idfcodec.units reads and writes the section up to its packed section, whose tables and
words predict.read_tables and read_section_words read, as they read IDFP's.  Sealing plane sets (a SealedCodec base would not cover the extra planes) is not built.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .codec import RANS_L
from .dist import _to_device
from .predict import (PREDICT_WAYS, PredictiveTileCodec, PredictiveTiledBitstream, _pick_words,
                      check_predict_ways, device_predict_decode, device_predict_decode_ways,
                      device_predict_encode, entry_overhead, is_packed, pack_tables, passes,
                      read_section_words, read_tables, ways_supported)
from . import predict as _predict
from . import safe as _safe
from . import tiled as _tiled
from .safe import SafeTiledBitstream, SafeTiledCodec, device_gather_raw, device_scatter_raw
from .tiled import (VERSION, Reader, TiledBitstream, TiledCodec, TileLayout, _ceil_div,
                    output_views, pack_lengthed, pack_words, source_views)
from .units import (CLASS_CONSTANT, CLASS_PACKED, CLASS_RAW, UnitSection, _runs, class_counts,
                    copy_raw_units, read_units, select_units)
from .units import unit_counts as unit_bytes

MAGIC = b"IDFM"
NAME = "plane set bitstream"
_HDR = "<4sHHIIIII"

# the base codecs and the file each writes, by its magic
_BASE_STREAMS = ((TiledCodec, TiledBitstream, (_tiled.MAGIC,)),
                 (SafeTiledCodec, SafeTiledBitstream, (_safe.MAGIC,)),
                 (PredictiveTileCodec, PredictiveTiledBitstream,
                  (_predict.MAGIC, _predict.MAGIC_COLOUR)))


# ------------------------------------------------------------------ host arithmetic
def split_channels(Cs, C: int) -> tuple:
    """(Cb, Ce) of sources of Cs channels against a model of C: the first C are the base planes
    where there are that many, else none is."""
    if isinstance(Cs, bool) or not isinstance(Cs, (int, np.integer)) or int(Cs) < 1:
        raise ValueError(f"channels {Cs!r} must be an integer of at least 1")
    Cs = int(Cs)
    return (int(C), Cs - int(C)) if Cs >= int(C) else (0, Cs)


def unit_class(mn, mx, status, nwords, n_bytes, ways: int = 1) -> np.ndarray:
    """uint8 per unit of CLASS_*, decided in this order: constant iff min == max; packed iff its
    stream's status is 0 and entry_overhead(ways) + 4 * nwords < its bytes (predict.is_packed: a
    tie stores raw); else raw.  status and nwords of a constant unit are not looked at."""
    const = np.asarray(mn) == np.asarray(mx)
    packs = is_packed(status, nwords, n_bytes, ways)
    return np.where(const, CLASS_CONSTANT,
                    np.where(packs, CLASS_PACKED, CLASS_RAW)).astype(np.uint8)


def plane_section_bytes(n_units: int, n_const: int, n_raw_bytes: int, nwords,
                        ways: int = 1) -> int:
    """The plane section of a file from its counts: the two bitmaps, the constants, the raw
    bytes and the packed section with their u64 lengths (the module's doc has the layout)."""
    nw = np.asarray(nwords, dtype=np.int64)
    return (_ceil_div(n_units, 8) + _ceil_div(n_units - n_const, 8) + n_const + 8
            + int(n_raw_bytes) + 8 + 4 + entry_overhead(ways) * len(nw) + 4 * int(nw.sum()))


def plane_section_bound(sizes, Ce: int, th: int, tw: int) -> int:
    """The bytes no plane section exceeds: every unit costs at most its bytes (a constant one
    byte of at least one, a packed unit less than its bytes by the class rule), plus the two
    bitmaps (at most ceil(U / 8) each), the two u64 lengths and the u32 count."""
    lay = TileLayout(sizes, max(int(Ce), 1), (th, tw))
    U = lay.n_tiles * int(Ce)
    return int(Ce) * sum(H * W for H, W in lay.sizes) + 2 * _ceil_div(U, 8) + 8 + 8 + 4


# ------------------------------------------------------------------ device calls
def device_segment_range(off: torch.Tensor, n: int, src: torch.Tensor) -> torch.Tensor:
    """off: device int64 [n + 1], rising -> device uint8 [n, 2]: the smallest and the largest
    byte of src[off[k]:off[k + 1]], (255, 0) for an empty run (idf_segment_range_u8;
    asynchronous)."""
    _lib.require_device(off, "run offsets")
    _lib.require_device(src, "run bytes")
    if off.dtype != torch.int64 or not off.is_contiguous() or off.numel() < n + 1:
        raise ValueError("run offsets must be contiguous int64 [n + 1]")
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError("the run bytes are a contiguous uint8 buffer")
    out = torch.empty((n, 2), dtype=torch.uint8, device=src.device)
    check(lib().idf_segment_range_u8(_lib.stream_ptr(src.device), n, ptr(off), ptr(src),
                                     ptr(out)), "segment range")
    return out


def device_segment_fill(off: torch.Tensor, length: torch.Tensor, value: torch.Tensor, n: int,
                        dst: torch.Tensor):
    """length[k] copies of value[k] at dst[off[k]:] (idf_segment_fill_u8; asynchronous).  The
    caller keeps the runs inside dst and apart."""
    for name, t, dt in (("run offsets", off, torch.int64), ("run lengths", length, torch.int64),
                        ("run values", value, torch.uint8)):
        _lib.require_device(t, name)
        if t.dtype != dt or not t.is_contiguous() or t.numel() < n:
            raise ValueError(f"{name} must be contiguous {dt} [n]")
    _lib.require_device(dst, "run bytes")
    if dst.dtype != torch.uint8 or not dst.is_contiguous():
        raise ValueError("the run bytes are a contiguous uint8 buffer")
    check(lib().idf_segment_fill_u8(_lib.stream_ptr(dst.device), n, ptr(off), ptr(length),
                                    ptr(value), ptr(dst)), "segment fill")


# ------------------------------------------------------------------ container
def _parse_base(buf: bytes, device):
    magic = bytes(buf[:4])
    for _, stream, magics in _BASE_STREAMS:
        if magic in magics:
            return stream.from_bytes(buf, device)
    raise ValueError(f"{NAME} holds a base file of unknown magic {magic!r}")


@dataclass
class PlaneSetBitstream(UnitSection):
    NAME, SAMPLE = NAME, np.uint8   # of the unit section behind the base file
    base: object                # the base codec's bitstream over the Cb base planes; None: Cb == 0
    sizes: list                 # [(H, W)] per image
    Cs: int                     # channels of the sources
    Cb: int                     # of them the base codes: 0 or the model's C
    tile_hw: tuple              # (th, tw)
    constant: np.ndarray        # bool [U], unit order: entry-major, plane-minor
    packed: np.ndarray          # bool [U]: not constant and coded by the predictor
    values: np.ndarray          # uint8 [K]: the constant units' bytes, unit order
    raw: torch.Tensor           # uint8: the raw units' bytes, unit order
    sel: np.ndarray             # uint32 [P], the packed units in unit order
    states: np.ndarray          # uint64 [P] ([P, ways] with predict_ways > 1)
    nwords: np.ndarray          # int64 [P]
    words: torch.Tensor         # int32 [sum nwords]: unit order, push order
    predict_ways: int = 1

    @property
    def Ce(self) -> int:
        return int(self.Cs) - int(self.Cb)

    @property
    def layout(self) -> TileLayout:
        """of the whole sources: Cs channels"""
        return TileLayout(self.sizes, self.Cs, self.tile_hw)

    @property
    def n_images(self) -> int:
        return len(self.sizes)

    @property
    def n_constant(self) -> int:
        return int(np.count_nonzero(self.constant))

    @property
    def n_packed(self) -> int:
        return int(np.count_nonzero(self.packed))

    def unit_bytes(self) -> np.ndarray:
        return unit_bytes(self.layout.rects, self.Ce)

    def n_subpixels(self) -> int:
        """of the unpadded images, all Cs channels"""
        return self.layout.n_subpixels

    def plane_bits(self) -> int:
        """What the extra planes add: 8 a constant, 8 a raw byte, 64 + 64 * predict_ways + 32 a
        word of every packed unit."""
        return (8 * self.n_constant + 8 * int(self.raw.numel())
                + 8 * entry_overhead(self.predict_ways) * self.n_packed
                + 32 * int(np.sum(self.nwords)))

    def bits(self) -> int:
        return (self.base.bits() if self.base is not None else 0) + self.plane_bits()

    def bpd(self) -> float:
        """bits per sub-pixel of the unpadded images"""
        n = self.n_subpixels()
        return self.bits() / n if n else float("nan")

    def check(self):
        """Raises unless the parts fit each other."""
        lay = self.layout
        if not (0 <= self.Cb <= self.Cs) or self.Cs < 1:
            raise ValueError(f"{NAME} of {self.Cs} channels names {self.Cb} base planes")
        if (self.base is None) != (self.Cb == 0):
            raise ValueError(f"{NAME} of {self.Cb} base planes "
                             + ("holds a base file" if self.Cb == 0 else "holds no base file"))
        if self.base is not None:
            b = self.base
            if (list(map(tuple, b.sizes)), tuple(b.tile_hw), b.C) != (
                    list(lay.sizes), lay.tile_hw, self.Cb):
                raise ValueError(f"{NAME} of {self.Cb} base planes, tiles {lay.tile_hw} holds a "
                                 f"base file of C {b.C}, tiles {tuple(b.tile_hw)} whose layout "
                                 "disagrees with its own")
        P, W = self.check_units(self.unit_bytes()), check_predict_ways(self.predict_ways)
        if not (len(self.sel) == len(self.states) == len(self.nwords) == P):
            raise ValueError(f"{NAME} packs {P} units, its tables hold {len(self.sel)}, "
                             f"{len(self.states)} and {len(self.nwords)} rows")
        if int(np.asarray(self.states).size) != P * W:
            raise ValueError(f"{NAME} packs {P} units of {W} ways, its states number "
                             f"{int(np.asarray(self.states).size)}")
        self.check_words()

    def plane_section(self) -> bytes:
        """Everything behind the base file: the unit section (idfcodec.units)."""
        return self.pack_units() + pack_lengthed(
            pack_tables(self.n_packed, self.sel, self.states, self.nwords)
            + pack_words(self.words))

    def to_bytes(self) -> bytes:
        self.check()
        flags = self.predict_ways if self.predict_ways > 1 else 0
        hdr = struct.pack(_HDR, MAGIC, VERSION, flags, len(self.sizes), self.Cs, self.Cb,
                          *self.tile_hw)
        hdr += b"".join(struct.pack("<II", H, W) for H, W in self.sizes)
        base = self.base.to_bytes() if self.base is not None else b""
        return hdr + struct.pack("<Q", len(base)) + base + self.plane_section()

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "PlaneSetBitstream":
        r = Reader(buf, NAME)
        got, ver, flags, n, Cs, Cb, th, tw = struct.unpack_from(
            _HDR, buf, r.take(struct.calcsize(_HDR), "header"))
        if got != MAGIC:
            raise ValueError(f"not an IDF {NAME}")
        if ver != VERSION:
            raise ValueError(f"unknown {NAME} version {ver}")
        if flags not in (0,) + PREDICT_WAYS[1:]:
            raise ValueError(f"unknown {NAME} flags {flags:#x}")
        if min(n, Cs, th, tw) < 1:
            raise ValueError(f"{NAME} header holds a zero size")
        if Cb > Cs:
            raise ValueError(f"{NAME} of {Cs} channels names {Cb} base planes")
        W = flags or 1
        sizes = r.array("<u4", 2 * n, "image sizes", then=8).reshape(n, 2).tolist()
        if any(min(s) < 1 for s in sizes):
            raise ValueError(f"{NAME} holds an image with a zero size")
        lay = TileLayout(sizes, Cs, (th, tw))
        n_base = r.u64()
        o = r.take(n_base, "base file")
        if (n_base == 0) != (Cb == 0):
            raise ValueError(f"{NAME} of {Cb} base planes holds a base file of {n_base} bytes")
        base = None
        if Cb:
            try:
                base = _parse_base(bytes(buf[o:o + n_base]), device)
            except struct.error as e:
                raise ValueError(f"truncated {NAME} (base file: {e})") from None
            if (list(map(tuple, base.sizes)), tuple(base.tile_hw), base.C) != (
                    list(lay.sizes), lay.tile_hw, Cb):
                raise ValueError(f"{NAME} of {Cb} base planes, tiles {lay.tile_hw} holds a base "
                                 f"file of C {base.C}, tiles {tuple(base.tile_hw)} whose layout "
                                 "disagrees with the header")
        constant, packed, values, raw = read_units(r, lay, Cs - Cb, np.uint8)
        n_sect = r.u64()
        s = r.end(n_sect)
        sel, states, nwords, n_tab = read_tables(s, n_sect, int(packed.sum()), W, "units")
        words = read_section_words(s, n_sect, n_tab, nwords, W)
        if device:
            raw, words = raw.to(device), words.to(device)
        return cls(base, [tuple(s) for s in sizes], Cs, Cb, (th, tw), constant, packed, values,
                   raw, sel, states, nwords, words, W)


# ------------------------------------------------------------------ codec
class PlaneSetCodec:
    """Lists of uint8 images of `channels` channels, [Cs, H_i, W_i] or [H_i, W_i, Cs], of any
    sizes and strides <-> PlaneSetBitstream (the module's doc has the split, the unit classes
    and the file).  base: the tiled codec of this model that codes the first C channels --
    model.tiled(), model.tiled_safe() or model.tiled_safe(predict=...); default
    model.tiled_safe(predict=True).  predict_ways: the interleaved states of the extra planes'
    predictive streams."""

    def __init__(self, model, channels: int, base=None, predict_ways: int = 1, max_batch=None):
        from .integrity import SealedCodec
        self.Cb, self.Ce = split_channels(channels, model.C)
        self.Cs = int(channels)
        self.C, self.tile_hw = model.C, (model.H, model.W)
        self.predict_ways = check_predict_ways(predict_ways)
        if self.predict_ways > 1 and not ways_supported(1, *self.tile_hw, self.predict_ways):
            raise ValueError(f"predict_ways {self.predict_ways} does not decode planes of tiles "
                             f"{self.tile_hw}: a unit does not fit the decoder's LDS")
        if base is None:
            base = model.tiled_safe(max_batch, predict=True)
        if isinstance(base, SealedCodec):
            raise ValueError("a sealed base would seal the base planes only: the extra planes "
                             "would look checked and not be; sealing plane sets is not built")
        if not isinstance(base, TiledCodec):
            raise TypeError(f"base is a tiled codec of the model, not {type(base).__name__}")
        if base.model is not model:
            raise ValueError("base is a codec of another model")
        self.model, self.base = model, base
        self._base_stream = next(s for c, s, _ in _BASE_STREAMS if type(base) is c)

    def _device(self) -> torch.device:
        return next(self.model.parameters()).device

    # -------------------------------------------------------------- the units' tables
    def _unit_rows(self, rows, views):
        """rows: planned rows (j, H, W, y0, x0) of some entries, views[j] the [Cs, H, W] view row
        j lies in -> the table rows of their units, entry-major and plane-minor: channel Cb + p
        of the view as an image of one channel.  Five fields where every view is dense planar,
        else eight."""
        Cb, Ce = self.Cb, self.Ce
        dense = all(_tiled.is_dense_planar(v) for v in views)
        out = []
        for j, H, W, y, x in rows:
            v = views[j]
            sc = v.stride(0) if v.shape[0] > 1 else 0
            for p in range(Ce):
                addr = v.data_ptr() + (Cb + p) * sc
                out.append((addr, H, W, y, x) if dense else
                           (addr, H, W, y, x, sc, v.stride(1), v.stride(2)))
        return out

    # -------------------------------------------------------------- encode
    def _code_units(self, staging, off_h, idx, rects_u, dev):
        """The predictive streams of units idx of the staging buffer, at most SYMBOLS_PER_PASS
        symbols a pass -> device_predict_encode's values, the passes joined."""
        th, tw = self.tile_hw
        base = staging.data_ptr()
        rows = [(base + int(off_h[u]), *rects_u[u], 0, 0) for u in idx]
        counts = (off_h[1:] - off_h[:-1])[idx]
        parts = [device_predict_encode(TiledCodec._device_table(rows[k:k + m], dev),
                                       counts[k:k + m], 1, th, tw, self.predict_ways)
                 for k, m in passes(counts)]
        sel, states, nw, status = (np.concatenate([p[i] for p in parts]) for i in range(4))
        return sel, states, nw, status, torch.cat([p[4] for p in parts])

    @torch.no_grad()
    def encode(self, images, layout=None, **base_kwargs) -> PlaneSetBitstream:
        """images, layout: as TiledCodec.encode, with `channels` channels in place of the
        model's.  base_kwargs (max_ratio, check, choose, ...) go to the base codec's encode,
        which is given the [:Cb] views of the sources with layout="chw" named."""
        dev = self._device()
        Cs, Cb, Ce, (th, tw), W = self.Cs, self.Cb, self.Ce, self.tile_hw, self.predict_ways
        views = source_views(images, Cs, dev, layout)   # held to the end
        lay = TileLayout([v.shape[1:] for v in views], Cs, (th, tw))
        base = None
        if Cb:
            base = self.base.encode([v[:Cb] for v in views], layout="chw", **base_kwargs)
        elif base_kwargs:
            raise ValueError(f"no base codes sources of {Cs} channels: {sorted(base_kwargs)} "
                             "have no taker")
        U = lay.n_tiles * Ce
        constant, packed = np.zeros(U, dtype=bool), np.zeros(U, dtype=bool)
        values = np.zeros(0, dtype=np.uint8)
        raw = torch.zeros(0, dtype=torch.uint8, device=dev)
        sel, nwords = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64)
        states = np.zeros((0, W) if W > 1 else 0, dtype=np.uint64)
        words = torch.zeros(0, dtype=torch.int32, device=dev)
        if U:
            rects_u = [r for r in lay.rects for _ in range(Ce)]
            off_h = np.zeros(U + 1, dtype=np.int64)
            np.cumsum(unit_bytes(lay.rects, Ce), out=off_h[1:])
            off = _to_device(torch.from_numpy(off_h), dev)
            staging = torch.empty(int(off_h[-1]), dtype=torch.uint8, device=dev)
            table = TiledCodec._device_table(self._unit_rows(lay.image_rows()[2], views), dev)
            device_gather_raw(table, U, 1, th, tw, off, staging)
            mm = device_segment_range(off, U, staging).cpu().numpy()
            constant = mm[:, 0] == mm[:, 1]
            values = mm[constant, 0].copy()
            idx = np.flatnonzero(~constant)
            if len(idx):
                sel, states, nwords, status, words = self._code_units(staging, off_h, idx,
                                                                      rects_u, dev)
                # what the model guarantees (every byte inside the window, every frequency >= 1)
                assert not status.any(), f"predictive encode status {status[status != 0][:8]}"
                cls = unit_class(np.zeros(len(idx)), np.ones(len(idx)), status, nwords,
                                 (off_h[1:] - off_h[:-1])[idx], W)
                use = cls == CLASS_PACKED
                packed[idx[use]] = True
                words = _pick_words(words, nwords, np.ones(len(idx), dtype=bool), use, dev)
                sel, states, nwords = sel[use], states[use], nwords[use]
                # neighbouring raw units are neighbours in the staging buffer: one slice a run
                r_idx = idx[~use]
                r_nb = (off_h[1:] - off_h[:-1])[r_idx]
                runs = _runs(off_h[r_idx], np.cumsum(r_nb) - r_nb, r_nb)
                if runs:
                    raw = torch.cat([staging[s:s + n] for s, _, n in runs])
            if W > 1:
                states = np.asarray(states, dtype=np.uint64).reshape(-1, W)
        return PlaneSetBitstream(base, [tuple(s) for s in lay.sizes], Cs, Cb, (th, tw), constant,
                                 packed, values, raw, sel, states, nwords, words, W)

    # -------------------------------------------------------------- decode
    def check_bitstream(self, bs: PlaneSetBitstream):
        if tuple(bs.tile_hw) != self.tile_hw:
            raise ValueError(f"{NAME} of tiles {tuple(bs.tile_hw)} does not match the model's "
                             f"input {self.tile_hw}")
        if bs.Cb not in (0, self.C) or (bs.Cb, bs.Ce) != split_channels(bs.Cs, self.C):
            raise ValueError(f"{NAME} of {bs.Cs} channels, {bs.Cb} of them base planes, does not "
                             f"fit the model's C {self.C}")
        if bs.Cs != self.Cs:
            raise ValueError(f"{NAME} of {bs.Cs} channels, the codec codes {self.Cs}")
        bs.check()
        if bs.base is not None:
            if type(bs.base) is not self._base_stream:
                raise ValueError(f"{NAME} holds a {type(bs.base).__name__} base, the codec's "
                                 f"base reads {self._base_stream.__name__}")
            self.base.check_bitstream(bs.base)

    def _decode_units(self, bs: PlaneSetBitstream, entries, rows, views, verify: bool, info):
        """The extra planes of entries `entries` into channel Cb + p of views[j], rows[k] =
        (j, H, W, y0, x0) saying where entry k goes; info gains the counts and the verdict."""
        dev, (th, tw), Ce, W = self._device(), self.tile_hw, self.Ce, bs.predict_ways
        cls = bs.classes
        units, ucls, u_rects, nb, out_h = select_units(cls, bs.layout.rects, entries, Ce)
        info.update(class_counts(ucls))
        info["damaged_planes"] = []
        n = len(units)
        if not n:
            return
        buf = torch.empty(int(out_h[-1]), dtype=torch.uint8, device=dev)
        ck = np.flatnonzero(ucls == CLASS_CONSTANT)
        if len(ck):
            cidx = np.cumsum(cls == CLASS_CONSTANT) - 1
            d64 = _to_device(torch.from_numpy(np.concatenate([out_h[ck], nb[ck]])), dev)
            d_val = _to_device(torch.from_numpy(
                np.asarray(bs.values, dtype=np.uint8)[cidx[units[ck]]].copy()), dev)
            device_segment_fill(d64[:len(ck)], d64[len(ck):], d_val, len(ck), buf)
        copy_raw_units(buf, bs.raw, cls, bs.unit_bytes(), units, ucls, nb, out_h)
        pk = np.flatnonzero(ucls == CLASS_PACKED)
        if len(pk):
            pidx = np.cumsum(cls == CLASS_PACKED) - 1
            which = pidx[units[pk]]
            w_off = np.zeros(len(bs.nwords) + 1, dtype=np.int64)
            np.cumsum(bs.nwords, out=w_off[1:])
            m = len(pk)
            words = bs.words if bs.words.device == dev else bs.words.to(dev)
            words = words.contiguous()
            if not words.numel():  # streams of no word still name a buffer
                words = torch.zeros(1, dtype=torch.int32, device=dev)
            d64 = _to_device(torch.from_numpy(np.concatenate([
                w_off[which], np.asarray(bs.nwords, dtype=np.int64)[which], out_h[pk],
                np.ascontiguousarray(np.asarray(bs.states, dtype=np.uint64)[which])
                .view(np.int64).reshape(-1)])), dev)
            d_states = d64[3 * m:]
            d64 = d64[:3 * m].view(3, m)
            d_sel = _to_device(torch.from_numpy(
                np.asarray(bs.sel, dtype=np.uint32)[which].view(np.int32).copy()), dev)
            d_rect = _to_device(torch.from_numpy(u_rects[pk]), dev)
            final = torch.empty(m * W, dtype=torch.int64, device=dev)
            status = torch.empty(m, dtype=torch.int32, device=dev)
            if W > 1:
                device_predict_decode_ways(m, W, 1, th, tw, words, d64[0], d64[1], d_states,
                                           d_sel, None, None, 0, d_rect, d64[2], buf, final,
                                           status)
            else:
                device_predict_decode(m, 1, th, tw, words, d64[0], d64[1], d_states, d_sel,
                                      d_rect, d64[2], buf, final, status)
            info["plane_units"] = units[pk]
            info["plane_final_states"], info["plane_status"] = final, status
        d_off = _to_device(torch.from_numpy(out_h[:n].copy()), dev)
        d_rect = _to_device(torch.from_numpy(u_rects), dev)
        table = TiledCodec._device_table(self._unit_rows(rows, views), dev)
        device_scatter_raw(table, n, 1, th, tw, buf, d_off, d_rect)
        if verify and len(pk):
            bad = ((final.view(len(pk), W) != RANS_L).any(1) | (status != 0)).cpu().numpy()
            info["damaged_planes"] = [int(u) for u in units[pk][bad]]
            info["ok"] = bool(info.get("ok", True)) and not bad.any()

    def _finish(self, bs, entries, rows, views, verify, info):
        if info is None:    # no base: no flow runs
            dev = self._device()
            info = {"final_states": torch.zeros(0, dtype=torch.int64, device=dev),
                    "status": torch.zeros(0, dtype=torch.int32, device=dev),
                    "tiles": len(entries), "raw_tiles": 0, "packed_tiles": 0}
            if verify:
                info["ok"] = True
            info["flow_tiles"] = 0
        else:
            info["flow_tiles"] = (info["tiles"] - info.get("raw_tiles", 0)
                                  - info.get("packed_tiles", 0))
        self._decode_units(bs, entries, rows, views, verify, info)
        return info

    @torch.no_grad()
    def decode(self, bs, images=None, verify: bool = True, layout: str = "chw", out=None):
        """As the base codec's decode, the outputs of `channels` channels: -> (list of uint8
        [Cs, H_i, W_i] (layout="hwc": [H_i, W_i, Cs]) or the caller's `out`, info).  info is the
        base's, with flow_tiles and the extra-plane units decoded per class: constant_planes,
        packed_planes, raw_planes; with verify, damaged_planes lists the packed units (entry *
        Ce + plane) whose stream did not end as it was written, and they clear info['ok']."""
        self.check_bitstream(bs)
        lay = bs.layout
        want, entries, rows = lay.image_rows(images)
        outs, views = output_views([(self.Cs, *lay.sizes[i]) for i in want], self._device(),
                                   layout, out)
        info = None
        if self.Cb:
            _, info = self.base.decode(bs.base, images=images, verify=verify, layout="chw",
                                       out=[v[:self.Cb] for v in views])
        return outs, self._finish(bs, entries, rows, views, verify, info)

    @torch.no_grad()
    def decode_region(self, bs, image: int, y0: int, x0: int, h: int, w: int,
                      verify: bool = True, layout: str = "chw", out=None):
        """-> (uint8 [Cs, h, w], info): rows [y0, y0 + h) x columns [x0, x0 + w) of one image,
        from exactly the tiles that intersect them, in both parts."""
        self.check_bitstream(bs)
        lay = bs.layout
        entries, rows = lay.region_rows(image, y0, x0, h, w)
        outs, views = output_views([(self.Cs, int(h), int(w))], self._device(), layout,
                                   None if out is None else [out])
        info = None
        if self.Cb:
            _, info = self.base.decode_region(bs.base, image, y0, x0, h, w, verify=verify,
                                              layout="chw", out=views[0][:self.Cb])
        return outs[0], self._finish(bs, entries, rows, views, verify, info)


__all__ = ["MAGIC", "NAME", "CLASS_CONSTANT", "CLASS_PACKED", "CLASS_RAW", "PlaneSetBitstream",
           "PlaneSetCodec", "device_segment_fill", "device_segment_range",
           "plane_section_bound", "plane_section_bytes", "split_channels", "unit_bytes",
           "unit_class"]
