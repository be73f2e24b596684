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
from .codec import RANS_L, Bitstream
from .tiled import (TiledBitstream, TiledCodec, _ceil_div, _check_table, region_tiles,
                    tile_table)

MAGIC = b"IDFS"
VERSION = 1
_HDR = "<4sHHIIII"

REASON_STATUS, REASON_SIZE, REASON_VERIFY = 1, 2, 4


# ------------------------------------------------------------------ host arithmetic
def entry_rects(sizes, th: int, tw: int) -> list:
    """[(hin, win)] per entry, in entry order: the in-image part of every tile."""
    _, entries = tile_table(sizes, th, tw)
    return [(min(th, int(sizes[i][0]) - ty * th), min(tw, int(sizes[i][1]) - tx * tw))
            for i, ty, tx in entries]


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
    reasons[((st & ~_lib.STREAM_WORDS_LEFT) != 0).any(0)] |= REASON_STATUS
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
    N = sum(tile_table(sizes, th, tw)[0])
    src = sum(int(C) * int(H) * int(W) for H, W in sizes)
    return src + 24 + 8 * len(sizes) + _ceil_div(N, 8) + 16 + (36 + 12 * levels if kept else 0)


# ------------------------------------------------------------------ device calls
def _check_off(off: torch.Tensor, n: int):
    _lib.require_device(off, "raw offsets")
    if off.dtype != torch.int64 or not off.is_contiguous() or off.numel() < n:
        raise ValueError("raw offsets must be contiguous int64 [n_tiles]")


def device_gather_raw(table: torch.Tensor, n: int, C: int, th: int, tw: int, off: torch.Tensor,
                      out: torch.Tensor):
    """The in-image bytes of the n tiles the table names -> out[off[t]:] as uint8 [C][hin][win]
    (idf_tile_gather_raw_u8).  The caller sizes out from the same table."""
    _check_table(table, n)
    _check_off(off, n)
    _lib.require_device(out, "raw bytes")
    if out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("the raw bytes are a contiguous uint8 buffer")
    check(lib().idf_tile_gather_raw_u8(_lib.stream_ptr(out.device), n, C, th, tw, ptr(table),
                                       ptr(off), ptr(out)), "tile gather raw")


def device_scatter_raw(table: torch.Tensor, n: int, C: int, th: int, tw: int, src: torch.Tensor,
                       off: torch.Tensor, rect: torch.Tensor):
    """The stored rectangles (rect: int32 [n, 2] of (hin, win), at src[off[t]:]) -> the uint8
    buffers the table names, inside their bounds only (idf_tile_scatter_raw_u8)."""
    _check_table(table, n)
    _check_off(off, n)
    _lib.require_device(src, "raw bytes")
    _lib.require_device(rect, "raw rectangles")
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError("the raw bytes are a contiguous uint8 buffer")
    if rect.dtype != torch.int32 or not rect.is_contiguous() or rect.numel() < 2 * n:
        raise ValueError("raw rectangles must be contiguous int32 [n_tiles, 2]")
    check(lib().idf_tile_scatter_raw_u8(_lib.stream_ptr(src.device), n, C, th, tw, ptr(src),
                                        ptr(off), ptr(rect), ptr(table)), "tile scatter raw")


def device_verify(table: torch.Tensor, n: int, C: int, th: int, tw: int, src: torch.Tensor,
                  mismatch: torch.Tensor, ld: int = 4):
    """mismatch[t] += the in-image (pixel, channel) pairs of tile t whose value in the
    pixel-major rows src is not the source byte the table names (idf_tile_verify_u8)."""
    _check_table(table, n)
    _lib.require_device(src, "tile buffer")
    _lib.require_device(mismatch, "mismatch counters")
    if src.dtype != torch.float32 or src.numel() < n * th * tw * ld:
        raise ValueError("verify input must be float32 and hold n * th * tw * ld values")
    if mismatch.dtype != torch.int32 or not mismatch.is_contiguous() or mismatch.numel() < n:
        raise ValueError("the mismatch counters are contiguous int32 [n_tiles]")
    check(lib().idf_tile_verify_u8(_lib.stream_ptr(src.device), n, C, th, tw, ptr(src), ld,
                                   ptr(table), ptr(mismatch)), "tile verify")


# ------------------------------------------------------------------ container
@dataclass
class SafeTiledBitstream:
    stream: Bitstream | None    # the K kept entries in entry order; None when K == 0
    sizes: list                 # [(H, W)] per image
    C: int
    tile_hw: tuple              # (th, tw)
    escaped: np.ndarray         # bool [N], entry order
    raw: torch.Tensor           # uint8: the escaped entries' in-image bytes, entry order
    reasons: np.ndarray | None = None   # uint8 [N] of REASON_* from encode; not serialised

    @property
    def n_images(self) -> int:
        return len(self.sizes)

    def tile_counts(self) -> list:
        return tile_table(self.sizes, *self.tile_hw)[0]

    @property
    def n_entries(self) -> int:
        return len(self.escaped)

    @property
    def n_kept(self) -> int:
        return int(self.n_entries - int(np.count_nonzero(self.escaped)))

    def rects(self) -> list:
        return entry_rects(self.sizes, *self.tile_hw)

    def n_subpixels(self) -> int:
        """of the unpadded images"""
        return sum(self.C * int(H) * int(W) for H, W in self.sizes)

    def bits(self) -> int:
        """The inner stream's bits (Bitstream.bits) + 8 per raw byte."""
        return (self.stream.bits() if self.stream is not None else 0) + 8 * int(self.raw.numel())

    def bpd(self) -> float:
        """bits per sub-pixel of the unpadded images"""
        n = self.n_subpixels()
        return self.bits() / n if n else float("nan")

    def escaped_share(self) -> float:
        """The share of the unpadded sub-pixels that is stored raw."""
        n = self.n_subpixels()
        return int(self.raw.numel()) / n if n else 0.0

    def to_bytes(self) -> bytes:
        N = self.n_entries
        if N != sum(self.tile_counts()):
            raise ValueError(f"{N} escape flags for {sum(self.tile_counts())} tiles")
        _, n_raw = raw_offsets(self.escaped, self.rects(), self.C)
        if int(self.raw.numel()) != n_raw:
            raise ValueError(f"{self.raw.numel()} raw bytes, the escaped tiles hold {n_raw}")
        K = self.n_kept
        if (self.stream.n_images if self.stream is not None else 0) != K:
            raise ValueError(f"safe tiled bitstream keeps {K} tiles, its inner stream holds "
                             f"{self.stream.n_images if self.stream is not None else 0} entries")
        inner = self.stream.to_bytes() if K else b""
        hdr = struct.pack(_HDR, MAGIC, VERSION, 0, len(self.sizes), self.C, *self.tile_hw)
        sizes = b"".join(struct.pack("<II", int(H), int(W)) for H, W in self.sizes)
        bitmap = np.packbits(np.asarray(self.escaped, dtype=bool), bitorder="little").tobytes()
        raw = self.raw.detach().cpu().numpy().tobytes()
        return (hdr + sizes + bitmap + struct.pack("<Q", len(raw)) + raw
                + struct.pack("<Q", len(inner)) + inner)

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "SafeTiledBitstream":
        n_hdr = struct.calcsize(_HDR)
        if len(buf) < n_hdr:
            raise ValueError("truncated safe tiled bitstream (header)")
        magic, ver, flags, n, C, th, tw = struct.unpack_from(_HDR, buf, 0)
        if magic != MAGIC:
            raise ValueError("not an IDF safe tiled bitstream")
        if ver != VERSION:
            raise ValueError(f"unknown safe tiled bitstream version {ver}")
        if flags:
            raise ValueError(f"unknown safe tiled bitstream flags {flags:#x}")
        if min(n, C, th, tw) < 1:
            raise ValueError("safe tiled bitstream header holds a zero size")
        o = n_hdr + 8 * n
        if len(buf) < o:
            raise ValueError("truncated safe tiled bitstream (image sizes)")
        sizes = [struct.unpack_from("<II", buf, n_hdr + 8 * i) for i in range(n)]
        if any(min(s) < 1 for s in sizes):
            raise ValueError("safe tiled bitstream holds an image with a zero size")
        sizes = [tuple(s) for s in sizes]
        N = sum(tile_table(sizes, th, tw)[0])
        n_map = _ceil_div(N, 8)
        if len(buf) < o + n_map + 8:
            raise ValueError("truncated safe tiled bitstream (escape bitmap)")
        bits = np.unpackbits(np.frombuffer(buf, np.uint8, n_map, o), bitorder="little")
        if bits[N:].any():
            raise ValueError(f"safe tiled bitstream of {N} tiles sets escape bits past them")
        escaped = bits[:N].astype(bool)
        o += n_map
        (n_raw,) = struct.unpack_from("<Q", buf, o)
        o += 8
        _, want = raw_offsets(escaped, entry_rects(sizes, th, tw), C)
        if n_raw != want:
            raise ValueError(f"safe tiled bitstream names {n_raw} raw bytes, its escaped tiles "
                             f"hold {want}")
        if len(buf) < o + n_raw + 8:
            raise ValueError("truncated safe tiled bitstream (raw bytes)")
        raw = torch.from_numpy(np.frombuffer(buf, np.uint8, n_raw, o).copy())
        if device:
            raw = raw.to(device)
        o += n_raw
        (length,) = struct.unpack_from("<Q", buf, o)
        o += 8
        if len(buf) != o + length:
            raise ValueError(f"safe tiled bitstream holds {len(buf) - o} inner bytes, its header "
                             f"names {length}")
        K = N - int(escaped.sum())
        stream = None
        if K == 0:
            if length:
                raise ValueError("safe tiled bitstream keeps no tile but holds an inner stream")
        else:
            try:
                stream = Bitstream.from_bytes(buf[o:], device)
            except struct.error as e:
                raise ValueError(f"truncated safe tiled bitstream ({e})") from None
            if stream.n_images != K:
                raise ValueError(f"safe tiled bitstream keeps {K} tiles, its inner stream holds "
                                 f"{stream.n_images} entries")
        return cls(stream, sizes, C, (th, tw), escaped, raw)


# ------------------------------------------------------------------ codec
class SafeTiledCodec(TiledCodec):
    """A list of uint8 images [C, H_i, W_i] of any sizes <-> SafeTiledBitstream: TiledCodec with
    every tile either kept or stored raw (the module's doc has the rule)."""

    # -------------------------------------------------------------- encode
    def _coded(self, images) -> TiledBitstream:
        """The flow-coded streams of every tile, status included: TiledCodec.encode unchanged."""
        return TiledCodec.encode(self, images)

    def _source_rows(self, images, sizes):
        th, tw = self.tile_hw
        _, entries = tile_table(sizes, th, tw)
        return [(images[i].data_ptr(), *sizes[i], ty * th, tx * tw) for i, ty, tx in entries]

    def _decoded_wrong(self, ic, stream: Bitstream, kept, rows) -> np.ndarray:
        """bool [len(kept)]: entry kept[k] of stream does not decode to the tile rows[k] names
        (a byte differs, a final state is not L, or a decode status flag)."""
        dev = ic.engine.device
        C, (th, tw) = self.C, self.tile_hw
        n, px4, n_lvl, W = len(kept), th * tw * 4, len(stream.level_shapes), stream.ways
        m_max = min(n, self.max_batch)
        if self._buf is None or self._buf.numel() < m_max * px4:
            self._buf = torch.empty(m_max * px4, dtype=torch.float32, device=dev)
        buf = self._buf
        whole = kept == list(range(stream.n_images)) and n <= self.max_batch
        nothing = lambda i, b0, m, ws: None  # noqa: E731  (the lanes write into buf)
        table = self._device_table(rows, dev)
        wrong = np.zeros(n, dtype=bool)
        for k in range(0, n, self.max_batch):
            m = min(self.max_batch, n - k)
            sub = stream if whole else stream.select(kept[k:k + m])
            part = ic._decode_lanes(sub, None, nothing, img_out=buf[:m * px4])
            mism = torch.zeros(m, dtype=torch.int32, device=dev)
            device_verify(table[k:k + m], m, C, th, tw, buf, mism)
            bad = (mism != 0) | (part["final_states"].view(n_lvl, m, W) != RANS_L).any(2).any(0)
            bad |= ((part["status"].view(n_lvl, m) & ~_lib.STREAM_WORDS_LEFT) != 0).any(0)
            wrong[k:k + m] = bad.cpu().numpy()
        return wrong

    @torch.no_grad()
    def encode(self, images, max_ratio: float = 1.0, check: str = "status") -> SafeTiledBitstream:
        """images: as TiledCodec.encode.  max_ratio: a tile is kept only if it costs at most
        max_ratio times its in-image bytes (inf: the size never escapes).  check: "status" (the
        encoder's flags) or "decode" (also decode every kept tile and compare with the source)."""
        if check not in ("status", "decode"):
            raise ValueError(f"check {check!r} is not 'status' or 'decode'")
        tbs = self._coded(images)  # it checks the images
        stream = tbs.stream
        dev = stream.states.device
        images = self._image_list(images, dev)
        C, (th, tw) = self.C, self.tile_hw
        sizes = [(int(t.shape[1]), int(t.shape[2])) for t in images]
        rects = entry_rects(sizes, th, tw)
        N = len(rects)
        if stream.n_images != N or stream.status is None:
            raise ValueError(f"the coded stream holds {stream.n_images} entries"
                             + ("" if stream.status is not None else " and no status")
                             + f"; the images have {N} tiles")
        reasons = keep_rule(stream.nwords_host().numpy(), stream.status.cpu().numpy(), rects, C,
                            stream.ways, max_ratio)
        rows = self._source_rows(images, sizes)
        if check == "decode":
            kept = [e for e in range(N) if not reasons[e]]
            if kept:
                wrong = self._decoded_wrong(self.model.codec(), stream, kept,
                                            [rows[e] for e in kept])
                reasons[np.asarray(kept)[wrong]] |= REASON_VERIFY
        escaped = reasons != 0
        kept = [e for e in range(N) if not escaped[e]]
        inner = None if not kept else stream if len(kept) == N else stream.select(kept)
        offs, n_raw = raw_offsets(escaped, rects, C)
        raw = torch.empty(n_raw, dtype=torch.uint8, device=dev)
        esc = [e for e in range(N) if escaped[e]]
        if esc:
            from .dist import _to_device
            d_off = _to_device(torch.tensor([offs[e] for e in esc], dtype=torch.int64), dev)
            device_gather_raw(self._device_table([rows[e] for e in esc], dev), len(esc), C, th,
                              tw, d_off, raw)
        return SafeTiledBitstream(inner, sizes, C, (th, tw), escaped, raw, reasons)

    # -------------------------------------------------------------- decode
    def check_bitstream(self, sbs: SafeTiledBitstream):
        if (sbs.C, tuple(sbs.tile_hw)) != (self.C, self.tile_hw):
            raise ValueError(f"safe tiled bitstream of C {sbs.C}, tiles {tuple(sbs.tile_hw)} does "
                             f"not match the model's C {self.C}, input {self.tile_hw}")
        N = sum(sbs.tile_counts())
        if len(sbs.escaped) != N:
            raise ValueError(f"safe tiled bitstream of {N} tiles holds {len(sbs.escaped)} escape "
                             "flags")
        K = sbs.n_kept
        have = sbs.stream.n_images if sbs.stream is not None else 0
        if have != K or (K and sbs.stream.group != 1):
            raise ValueError(f"safe tiled bitstream keeps {K} tiles, its inner stream holds "
                             f"{have} entries")
        _, n_raw = raw_offsets(sbs.escaped, sbs.rects(), self.C)
        if sbs.raw.dtype != torch.uint8 or int(sbs.raw.numel()) != n_raw:
            raise ValueError(f"safe tiled bitstream holds {sbs.raw.numel()} raw bytes, its "
                             f"escaped tiles {n_raw}")

    def _device(self) -> torch.device:
        """The engine's device, without the engine: IDFlows.codec() walks every parameter, and a
        decode of raw tiles only needs none of it."""
        return next(self.model.parameters()).device

    def _decode_entries(self, sbs: SafeTiledBitstream, entries, rows, verify: bool):
        """Entries `entries` of sbs into the buffers rows[k] names: the kept ones through the
        flow (TiledCodec._decode_tiles over the inner stream), the raw ones by one byte scatter."""
        dev = self._device()
        C, (th, tw) = self.C, self.tile_hw
        inner = inner_index(sbs.escaped)
        k_ent = [k for k, e in enumerate(entries) if not sbs.escaped[e]]
        r_ent = [k for k, e in enumerate(entries) if sbs.escaped[e]]
        if k_ent:
            info = self._decode_tiles(self.model.codec(),
                                      TiledBitstream(sbs.stream, sbs.sizes, C, (th, tw)),
                                      [inner[entries[k]] for k in k_ent],
                                      [rows[k] for k in k_ent], verify)
        else:  # no flow runs
            info = {"final_states": torch.zeros(0, dtype=torch.int64, device=dev),
                    "status": torch.zeros(0, dtype=torch.int32, device=dev),
                    "off_grid": torch.zeros(1, dtype=torch.int32, device=dev), "tiles": 0}
            if verify:
                info["ok"] = True
        if r_ent:
            from .dist import _to_device
            offs, _ = raw_offsets(sbs.escaped, sbs.rects(), C)
            rects = sbs.rects()
            raw = sbs.raw if sbs.raw.device == dev else sbs.raw.to(dev)
            d_off = _to_device(torch.tensor([offs[entries[k]] for k in r_ent],
                                            dtype=torch.int64), dev)
            d_rect = _to_device(torch.tensor([rects[entries[k]] for k in r_ent],
                                             dtype=torch.int32).reshape(-1, 2), dev)
            device_scatter_raw(self._device_table([rows[k] for k in r_ent], dev), len(r_ent), C,
                               th, tw, raw.contiguous(), d_off, d_rect)
        info["tiles"] = len(entries)
        info["raw_tiles"] = len(r_ent)
        return info

    @torch.no_grad()
    def decode(self, sbs: SafeTiledBitstream, images=None, verify: bool = True):
        """-> (list of uint8 [C, H_i, W_i], info): as TiledCodec.decode; info['raw_tiles'] of the
        info['tiles'] tiles were stored raw."""
        self.check_bitstream(sbs)
        th, tw = self.tile_hw
        counts = sbs.tile_counts()
        first = [0]
        for c in counts:
            first.append(first[-1] + c)
        want = list(range(len(counts))) if images is None else [int(i) for i in images]
        for i in want:
            if not 0 <= i < len(counts):
                raise ValueError(f"image {i} is outside the bitstream's {len(counts)} images")
        dev = self._device()
        outs, entries, rows = [], [], []
        for i in want:
            H, W = sbs.sizes[i]
            out = torch.empty((self.C, H, W), dtype=torch.uint8, device=dev)
            outs.append(out)
            nw = _ceil_div(W, tw)
            for j in range(counts[i]):
                entries.append(first[i] + j)
                rows.append((out.data_ptr(), H, W, (j // nw) * th, (j % nw) * tw))
        return outs, self._decode_entries(sbs, entries, rows, verify)

    @torch.no_grad()
    def decode_region(self, sbs: SafeTiledBitstream, image: int, y0: int, x0: int, h: int, w: int,
                      verify: bool = True):
        """-> (uint8 [C, h, w], info): as TiledCodec.decode_region; a region of raw tiles only
        runs no flow."""
        self.check_bitstream(sbs)
        image = int(image)
        if not 0 <= image < sbs.n_images:
            raise ValueError(f"image {image} is outside the bitstream's {sbs.n_images} images")
        th, tw = self.tile_hw
        H, W = sbs.sizes[image]
        tiles = region_tiles((H, W), y0, x0, h, w, th, tw)
        first = sum(sbs.tile_counts()[:image])
        nw = _ceil_div(W, tw)
        out = torch.empty((self.C, int(h), int(w)), dtype=torch.uint8, device=self._device())
        entries = [first + ty * nw + tx for ty, tx in tiles]
        rows = [(out.data_ptr(), int(h), int(w), ty * th - int(y0), tx * tw - int(x0))
                for ty, tx in tiles]
        return out, self._decode_entries(sbs, entries, rows, verify)


__all__ = ["MAGIC", "VERSION", "REASON_STATUS", "REASON_SIZE", "REASON_VERIFY",
           "SafeTiledBitstream", "SafeTiledCodec", "device_gather_raw", "device_scatter_raw",
           "device_verify", "entry_bits", "entry_rects", "file_size_bound", "inner_index",
           "keep_rule", "raw_offsets"]
