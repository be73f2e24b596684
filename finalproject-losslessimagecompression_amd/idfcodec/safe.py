"""The tiled codec with a raw-tile escape: a file that always decodes to the source and is never
larger than the source plus a fixed header.

SafeTiledCodec codes a ragged list of images as TiledCodec does (idfcodec.tiled: one batch entry
per tile), then decides per entry, on the host, whether the entry is *kept* (its rANS streams go
into the file) or *escaped* (the bytes of its in-image rectangle go into the file as they are).
An entry is kept iff

  * no level's encode status holds a flag other than WORDS_LEFT (a latent outside the rANS window,
    a zero / NaN scale, a non-monotone CDF: streams that do not decode to the source), and
  * bits_e <= max_ratio * 8 * raw_e, with bits_e = sum over levels of (64 * ways + 32 * nwords +
    32) -- the states, the words and the entry's fields of the word-count table, what the entry
    adds to the file -- and raw_e = C * hin * win, the bytes of its in-image rectangle.

check="decode" also decodes the kept entries and escapes every entry whose decoded tile differs
from the source (idf_tile_verify_u8), whose final states are not L or whose decode raised a status
flag.  An entry's streams depend on no other entry's, so one pass decides.  The decision is
recorded in the file (a bitmap); the decoder never derives it again.  The reason an entry was
escaped (REASON_*) is kept on the returned object only.

With max_ratio <= 1 every kept entry costs at most its raw bytes, so bits() <= 8 * (source bytes)
and the file is at most the source plus its headers (file_size_bound).

Container IDFS (little-endian): magic "IDFS", u16 version 1, u16 flags 0, u32 n_images, u32 C,
u32 tile_h, u32 tile_w, n_images x (u32 H, u32 W), the escape bitmap (N bits in entry order, LSB
first, ceil(N / 8) bytes), u64 raw length, the raw bytes (the escaped entries in entry order, each
uint8 [C][hin][win]), u64 inner length, the inner IDFB container over the K kept entries in entry
order (length 0 and absent when K == 0).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .codec import RANS_L, STATUS_FAILED, Bitstream
from .dist import _to_device
from .tiled import (VERSION, Reader, TileLayout, TiledBitstream, TiledCodec, _ceil_div,
                    _check_table, _entry, _TiledSizes, as_chw, pack_bitmap, pack_lengthed)

MAGIC = b"IDFS"
NAME = "safe tiled bitstream"

REASON_STATUS, REASON_SIZE, REASON_VERIFY = 1, 2, 4
REASON_SMALLER = 8  # the keep rule kept it; another coding is smaller (idfcodec.predict)


# ------------------------------------------------------------------ host arithmetic
def entry_rects(sizes, th: int, tw: int) -> list:
    """[(hin, win)] per entry, in entry order: the in-image part of every tile."""
    return TileLayout(sizes, 1, (th, tw)).rects


def entry_bits(nwords, n_entries: int, ways: int = 1) -> np.ndarray:
    """nwords: the level-major, entry-minor word counts of a Bitstream of n_entries entries ->
    int64 [n_entries], sum over levels of 64 * ways + 32 * nwords + 32."""
    nw = np.asarray(nwords, dtype=np.int64).reshape(-1, n_entries)
    return (64 * int(ways) + 32 * nw + 32).sum(0)


def keep_rule(nwords, status, rects, C: int, ways: int = 1, max_ratio: float = 1.0) -> np.ndarray:
    """-> uint8 [N] of REASON_* bits, 0 = kept.  nwords, status: level-major, entry-minor, one
    value per (level, entry); rects: entry_rects.  A tie bits_e == max_ratio * 8 * raw_e keeps."""
    N = len(rects)
    if not (max_ratio > 0):  # NaN included
        raise ValueError(f"max_ratio {max_ratio!r} must be positive")
    bits = entry_bits(nwords, N, ways)
    st = np.asarray(status, dtype=np.int64).reshape(-1, N)
    raw_bits = 8 * int(C) * np.array([h * w for h, w in rects], dtype=np.int64).reshape(N)
    reasons = np.zeros(N, dtype=np.uint8)
    reasons[((st & STATUS_FAILED) != 0).any(0)] |= REASON_STATUS
    # exact integers against one float product each: a tie keeps
    over = [int(b) > float(max_ratio) * int(r) for b, r in zip(bits, raw_bits)]
    reasons[np.array(over, dtype=bool)] |= REASON_SIZE
    return reasons


def inner_index(escaped) -> list:
    """entry -> its index among the kept entries (the inner stream's entry), -1 if escaped"""
    out, k = [], 0
    for e in escaped:
        out.append(-1 if e else k)
        k += 0 if e else 1
    return out


def raw_offsets(escaped, rects, C: int):
    """-> ([byte offset of entry e in the raw bytes, -1 if kept], the raw length)"""
    out, o = [], 0
    for e, (h, w) in zip(escaped, rects):
        out.append(o if e else -1)
        o += int(C) * h * w if e else 0
    return out, o


def file_size_bound(sizes, C: int, th: int, tw: int, levels: int, kept: bool = True) -> int:
    """The bytes a file coded with max_ratio <= 1 cannot exceed: the source, the IDFS fields and,
    where an entry is kept, the inner container's own header."""
    lay = TileLayout(sizes, C, (th, tw))
    N, src = lay.n_tiles, lay.n_subpixels
    return src + 24 + 8 * len(sizes) + _ceil_div(N, 8) + 16 + (36 + 12 * levels if kept else 0)


# ------------------------------------------------------------------ device calls
def _check_off(off: torch.Tensor, n: int):
    _lib.require_device(off, "raw offsets")
    if off.dtype != torch.int64 or not off.is_contiguous() or off.numel() < n:
        raise ValueError("raw offsets must be contiguous int64 [n_tiles]")


def device_gather_raw(table: torch.Tensor, n: int, C: int, th: int, tw: int, off: torch.Tensor,
                      out: torch.Tensor):
    """The in-image bytes of the n tiles the table names -> out[off[t]:] as uint8 [C][hin][win]
    (idf_tile_gather_raw_u8; idf_tile_gather_raw_strided_u8 for rows of eight fields).  The
    caller sizes out from the same table."""
    fields = _check_table(table, n)
    _check_off(off, n)
    _lib.require_device(out, "raw bytes")
    if out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("the raw bytes are a contiguous uint8 buffer")
    check(_entry("idf_tile_gather_raw_u8", fields)(_lib.stream_ptr(out.device), n, C, th, tw,
                                                   ptr(table), ptr(off), ptr(out)),
          "tile gather raw")


def device_scatter_raw(table: torch.Tensor, n: int, C: int, th: int, tw: int, src: torch.Tensor,
                       off: torch.Tensor, rect: torch.Tensor):
    """The stored rectangles (rect: int32 [n, 2] of (hin, win), at src[off[t]:]) -> the uint8
    buffers the table names, inside their bounds only (idf_tile_scatter_raw_u8;
    idf_tile_scatter_raw_strided_u8 for rows of eight fields)."""
    fields = _check_table(table, n)
    _check_off(off, n)
    _lib.require_device(src, "raw bytes")
    _lib.require_device(rect, "raw rectangles")
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError("the raw bytes are a contiguous uint8 buffer")
    if rect.dtype != torch.int32 or not rect.is_contiguous() or rect.numel() < 2 * n:
        raise ValueError("raw rectangles must be contiguous int32 [n_tiles, 2]")
    check(_entry("idf_tile_scatter_raw_u8", fields)(_lib.stream_ptr(src.device), n, C, th, tw,
                                                    ptr(src), ptr(off), ptr(rect), ptr(table)),
          "tile scatter raw")


def device_verify(table: torch.Tensor, n: int, C: int, th: int, tw: int, src: torch.Tensor,
                  mismatch: torch.Tensor, ld: int = 4):
    """mismatch[t] += the in-image (pixel, channel) pairs of tile t whose value in the
    pixel-major rows src is not the source byte the table names (idf_tile_verify_u8;
    idf_tile_verify_strided_u8 for rows of eight fields)."""
    fields = _check_table(table, n)
    _lib.require_device(src, "tile buffer")
    _lib.require_device(mismatch, "mismatch counters")
    if src.dtype != torch.float32 or src.numel() < n * th * tw * ld:
        raise ValueError("verify input must be float32 and hold n * th * tw * ld values")
    if mismatch.dtype != torch.int32 or not mismatch.is_contiguous() or mismatch.numel() < n:
        raise ValueError("the mismatch counters are contiguous int32 [n_tiles]")
    check(_entry("idf_tile_verify_u8", fields)(_lib.stream_ptr(src.device), n, C, th, tw,
                                               ptr(src), ld, ptr(table), ptr(mismatch)),
          "tile verify")


# ------------------------------------------------------------------ container
def _check_kept(K: int, stream, one_per_entry: bool = False):
    """Raises unless the inner stream holds the K kept entries (one_per_entry: and codes each in
    streams of its own, as the decode needs it)."""
    have = stream.n_images if stream is not None else 0
    if have != K or (one_per_entry and K and stream.group != 1):
        raise ValueError(f"{NAME} keeps {K} tiles, its inner stream holds {have} entries")


def _read_inner(r: Reader, K: int, device):
    """What IDFS, IDFP and IDFQ end with: a u64 length and the inner IDFB container over the K
    kept entries, absent when K == 0 -> the Bitstream, or None."""
    length = r.u64()
    if len(r.buf) != r.o + length:
        raise ValueError(f"{r.name} holds {len(r.buf) - r.o} inner bytes, its header names "
                         f"{length}")
    if K == 0:
        if length:
            raise ValueError(f"{r.name} keeps no tile but holds an inner stream")
        return None
    try:
        stream = Bitstream.from_bytes(r.buf[r.o:], device)
    except struct.error as e:
        raise ValueError(f"truncated {r.name} ({e})") from None
    _check_kept(K, stream)
    return stream


@dataclass
class SafeTiledBitstream(_TiledSizes):
    stream: Bitstream | None    # the K kept entries in entry order; None when K == 0
    sizes: list                 # [(H, W)] per image
    C: int
    tile_hw: tuple              # (th, tw)
    escaped: np.ndarray         # bool [N], entry order
    raw: torch.Tensor           # uint8: the escaped entries' in-image bytes, entry order
    reasons: np.ndarray | None = None   # uint8 [N] of REASON_* from encode; not serialised

    @property
    def n_entries(self) -> int:
        return len(self.escaped)

    @property
    def n_kept(self) -> int:
        return int(self.n_entries - int(np.count_nonzero(self.escaped)))

    def rects(self) -> list:
        return self.layout.rects

    def bits(self) -> int:
        """The inner stream's bits (Bitstream.bits) + 8 per raw byte."""
        return (self.stream.bits() if self.stream is not None else 0) + 8 * int(self.raw.numel())

    def escaped_share(self) -> float:
        """The share of the unpadded sub-pixels that is stored raw."""
        n = self.n_subpixels()
        return int(self.raw.numel()) / n if n else 0.0

    def to_bytes(self) -> bytes:
        lay, N = self.layout, self.n_entries
        if N != lay.n_tiles:
            raise ValueError(f"{N} escape flags for {lay.n_tiles} tiles")
        _, n_raw = raw_offsets(self.escaped, lay.rects, self.C)
        if int(self.raw.numel()) != n_raw:
            raise ValueError(f"{self.raw.numel()} raw bytes, the escaped tiles hold {n_raw}")
        _check_kept(self.n_kept, self.stream)
        inner = self.stream.to_bytes() if self.n_kept else b""
        return (lay.pack(MAGIC) + pack_bitmap(self.escaped) + pack_lengthed(self.raw)
                + pack_lengthed(inner))

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "SafeTiledBitstream":
        lay, o = TileLayout.unpack(buf, MAGIC, NAME)
        r = Reader(buf, NAME, o)
        escaped = r.bitmap(lay.n_tiles, "escape", "tiles", then=8)
        _, want = raw_offsets(escaped, lay.rects, lay.C)
        raw = torch.from_numpy(r.lengthed(want, "raw bytes", "escaped tiles", then=8).copy())
        stream = _read_inner(r, lay.n_tiles - int(escaped.sum()), device)
        if device:
            raw = raw.to(device)
        return cls(stream, list(lay.sizes), lay.C, lay.tile_hw, escaped, raw)


# ------------------------------------------------------------------ codec
@dataclass
class Decided:
    """What SafeTiledCodec._decide hands to _assemble."""
    sizes: list                 # [(H, W)] per image
    layout: TileLayout
    stream: Bitstream           # every entry's flow streams, status included
    dev: torch.device
    images: list                # the source views, held until the bytes are gathered
    rows: list                  # their tile table rows
    reasons: np.ndarray         # uint8 [N] of REASON_*, 0 = the keep rule keeps the entry
    flow_bits: np.ndarray       # int64 [N]: entry_bits


class SafeTiledCodec(TiledCodec):
    """A list of uint8 images [C, H_i, W_i] of any sizes <-> SafeTiledBitstream: TiledCodec with
    every tile either kept or stored raw (the module's doc has the rule), over the same memory
    layouts (encode's layout, decode's layout and out: idfcodec.tiled).  decode and
    decode_region are TiledCodec's; their info['raw_tiles'] of the info['tiles'] tiles were
    stored raw, and where all are no flow runs."""

    # -------------------------------------------------------------- encode
    def _coded(self, images) -> TiledBitstream:
        """The flow-coded streams of every tile, status included: TiledCodec.encode unchanged."""
        return TiledCodec.encode(self, images, layout="chw")  # encode has applied the layout

    def _decoded_wrong(self, ic, stream: Bitstream, kept, rows) -> np.ndarray:
        """bool [len(kept)]: entry kept[k] of stream does not decode to the tile rows[k] names
        (a byte differs, a final state is not L, or a decode status flag)."""
        dev = ic.engine.device
        C, (th, tw) = self.C, self.tile_hw
        n_lvl, W = len(stream.level_shapes), stream.ways
        table = self._device_table(rows, dev)
        wrong = np.zeros(len(kept), dtype=bool)
        for k, m, part in self._chunks(ic, stream, kept):
            mism = torch.zeros(m, dtype=torch.int32, device=dev)
            device_verify(table[k:k + m], m, C, th, tw, self._buf, mism)
            bad = (mism != 0) | (part["final_states"].view(n_lvl, m, W) != RANS_L).any(2).any(0)
            bad |= ((part["status"].view(n_lvl, m) & STATUS_FAILED) != 0).any(0)
            wrong[k:k + m] = bad.cpu().numpy()
        return wrong

    def _decide(self, images, max_ratio: float, check: str, layout, launch=None) -> "Decided":
        """The first half of encode: every tile coded by the flow and the keep rule applied (the
        module's doc has it; check="decode" included).  launch(rows, layout, device), if given,
        is called once the flow's work is queued and before its status is read, so that what it
        queues is complete where the status is and its results cost no host wait of their own."""
        if check not in ("status", "decode"):
            raise ValueError(f"check {check!r} is not 'status' or 'decode'")
        images = as_chw(images, layout)  # [C, H, W] views from here on; None: contiguous ones
        tbs = self._coded(images)  # it checks the images and lays out their tiles
        stream, lay = tbs.stream, tbs.layout
        dev = stream.states.device
        rects, N = lay.rects, lay.n_tiles
        if stream.n_images != N or stream.status is None:
            raise ValueError(f"the coded stream holds {stream.n_images} entries"
                             + ("" if stream.status is not None else " and no status")
                             + f"; the images have {N} tiles")
        images, _, rows = self._sources(images, dev, "chw")  # checked above; held to the end
        if launch is not None:
            launch(rows, lay, dev)
        nw_h = stream.nwords_host().numpy()
        reasons = keep_rule(nw_h, stream.status.cpu().numpy(), rects, self.C, stream.ways,
                            max_ratio)
        if check == "decode":
            kept = [e for e in range(N) if not reasons[e]]
            if kept:
                wrong = self._decoded_wrong(self.model.codec(), stream, kept,
                                            [rows[e] for e in kept])
                reasons[np.asarray(kept)[wrong]] |= REASON_VERIFY
        return Decided(tbs.sizes, lay, stream, dev, images, rows, reasons,
                       entry_bits(nw_h, N, stream.ways))

    def _assemble(self, d: "Decided", escaped, stored=None):
        """The second half: -> (the inner stream over the entries not escaped, the bytes of the
        entries `stored` flags -- default: the escaped ones -- in entry order)."""
        C, (th, tw) = self.C, self.tile_hw
        rects, N = d.layout.rects, d.layout.n_tiles
        stored = escaped if stored is None else stored
        kept = [e for e in range(N) if not escaped[e]]
        inner = None if not kept else d.stream if len(kept) == N else d.stream.select(kept)
        offs, n_raw = raw_offsets(stored, rects, C)
        raw = torch.empty(n_raw, dtype=torch.uint8, device=d.dev)
        esc = [e for e in range(N) if stored[e]]
        if esc:
            d_off = _to_device(torch.tensor([offs[e] for e in esc], dtype=torch.int64), d.dev)
            device_gather_raw(self._device_table([d.rows[e] for e in esc], d.dev), len(esc), C,
                              th, tw, d_off, raw)
        return inner, raw

    @torch.no_grad()
    def encode(self, images, max_ratio: float = 1.0, check: str = "status",
               layout=None) -> SafeTiledBitstream:
        """images, layout: as TiledCodec.encode.  max_ratio: a tile is kept only if it costs at most
        max_ratio times its in-image bytes (inf: the size never escapes).  check: "status" (the
        encoder's flags) or "decode" (also decode every kept tile and compare with the source)."""
        d = self._decide(images, max_ratio, check, layout)
        escaped = d.reasons != 0
        inner, raw = self._assemble(d, escaped)
        return SafeTiledBitstream(inner, d.sizes, self.C, self.tile_hw, escaped, raw, d.reasons)

    # -------------------------------------------------------------- decode
    def check_bitstream(self, sbs: SafeTiledBitstream):
        if (sbs.C, tuple(sbs.tile_hw)) != (self.C, self.tile_hw):
            raise ValueError(f"{NAME} of C {sbs.C}, tiles {tuple(sbs.tile_hw)} does not match "
                             f"the model's C {self.C}, input {self.tile_hw}")
        lay = sbs.layout
        if len(sbs.escaped) != lay.n_tiles:
            raise ValueError(f"{NAME} of {lay.n_tiles} tiles holds {len(sbs.escaped)} escape "
                             "flags")
        _check_kept(sbs.n_kept, sbs.stream, one_per_entry=True)
        _, n_raw = raw_offsets(sbs.escaped, lay.rects, self.C)
        if sbs.raw.dtype != torch.uint8 or int(sbs.raw.numel()) != n_raw:
            raise ValueError(f"{NAME} holds {sbs.raw.numel()} raw bytes, its escaped tiles "
                             f"{n_raw}")

    def _decode_entries(self, sbs: SafeTiledBitstream, entries, rows, verify: bool, seal=None,
                        raw_offs=None):
        """Entries `entries` of sbs into the buffers rows[k] names: the kept ones through the
        flow (TiledCodec._decode_tiles over the inner stream), the raw ones by one byte scatter.
        seal: a sealed file's check (idfcodec.integrity), told which entries are which and shown
        the stored bytes.  raw_offs: where each escaped entry asked for lies in sbs.raw, for a
        caller whose raw bytes hold only some of the escaped entries (idfcodec.predict)."""
        dev = self._device()
        C, (th, tw) = self.C, self.tile_hw
        inner = inner_index(sbs.escaped)
        k_ent = [k for k, e in enumerate(entries) if not sbs.escaped[e]]
        r_ent = [k for k, e in enumerate(entries) if sbs.escaped[e]]
        if seal is not None:
            seal.split(k_ent, r_ent)
        if k_ent:
            info = self._decode_tiles(self._codec_for(seal), sbs.stream,
                                      [inner[entries[k]] for k in k_ent],
                                      [rows[k] for k in k_ent], verify, seal)
        else:  # no flow runs
            info = {"final_states": torch.zeros(0, dtype=torch.int64, device=dev),
                    "status": torch.zeros(0, dtype=torch.int32, device=dev),
                    "off_grid": torch.zeros(1, dtype=torch.int32, device=dev), "tiles": 0}
            if verify:
                info["ok"] = True
        if r_ent:
            rects = sbs.rects()
            offs = raw_offs if raw_offs is not None else raw_offsets(sbs.escaped, rects, C)[0]
            raw = sbs.raw if sbs.raw.device == dev else sbs.raw.to(dev)
            raw = raw.contiguous()
            r_off = [offs[entries[k]] for k in r_ent]
            d_off = _to_device(torch.tensor(r_off, dtype=torch.int64), dev)
            d_rect = _to_device(torch.tensor([rects[entries[k]] for k in r_ent],
                                             dtype=torch.int32).reshape(-1, 2), dev)
            device_scatter_raw(self._device_table([rows[k] for k in r_ent], dev), len(r_ent), C,
                               th, tw, raw, d_off, d_rect)
            if seal is not None:
                seal.raw_runs(raw, r_off)
        info["tiles"] = len(entries)
        info["raw_tiles"] = len(r_ent)
        return info


__all__ = ["MAGIC", "VERSION", "REASON_STATUS", "REASON_SIZE", "REASON_VERIFY", "REASON_SMALLER",
           "SafeTiledBitstream", "SafeTiledCodec", "device_gather_raw", "device_scatter_raw",
           "device_verify", "entry_bits", "entry_rects", "file_size_bound", "inner_index",
           "keep_rule", "raw_offsets"]
