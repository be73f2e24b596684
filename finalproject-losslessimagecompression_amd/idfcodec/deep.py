"""16-bit images: a tiled predictive rANS coder for uint16 samples, no model needed.

DeepTiledCodec tiles its sources as the other tiled codecs do (TileLayout) and codes every *unit*
-- one plane of one tile's in-image rectangle, uint16 [hin][win]; unit u = entry * C + plane --
on its own, from its own samples alone (include/idf_codec.h "the 16-bit predictive coder" states
the model, csrc/idf_deep.h holds its literals and the window argument): the MED predictor of the
8-bit predictive coder on the samples' high part v >> s, the unit's shift s in 0..8 chosen so that
at most an eighth of its residuals reach 16 << s, an escape list for the samples the 2048-bin
window cannot hold (|q - pq| >= 1000), and the low s bits stored as they are.  A unit is kept in
the first class that holds (unit_class):

  constant  min == max; its value is stored, two bytes;
  packed    21 + 4 * nwords + 4 * ceil(n * s / 32) + 2 * n_esc < 2 * n (shift 1, sel 4, state 8,
            nwords 4, n_esc 4 bytes; a tie stores raw);
  raw       its 2 * n bytes, little-endian.

Interleaved states (DeepTiledCodec(channels, ways=N), N in 8, 16, 32, 64; csrc/idf_deep.h has the
format): a packed unit is coded by N rANS states that share one word sequence, its samples
ordered along a pixel wavefront -- pixel (y, x) has step (y // N) * max(win, N) + y % N + x and
slot y % N, its a, b and c lie in earlier steps -- so that idf_deep_decode_ways_u16 decodes a
step of up to N samples at a time: 519 steps for a 64 x 64 unit at N = 8 and 127 at N = 64,
against 4096 serial symbols.  The model is untouched; the escapes are listed in wavefront order,
the low bits stay where they are, and a packed unit costs 13 + 8 N + 4 * nwords + ... bytes
(unit_overhead), so small units fall to raw as N grows.  The file names its N; any codec of
matching C and tile decodes any file whose N its tile supports (ways_supported: the decoder keeps
the whole unit in LDS).  ways=1, the default, writes the files it always wrote, byte for byte.

encode: idf_deep_prep_u16 reads the samples where they lie (a table row a unit: interleaved HWC,
row pitches and windows of larger images are never copied) and writes the symbols, the low-bit
words and the escapes; idf_rans_encode_streams codes the symbols; idf_gather_words compacts the
words, the low-bit words and the escapes of the packed units; idf_tile_gather_raw_strided_u16
fetches the raw units.  At most SYMBOLS_PER_PASS symbols are in flight.  decode:
idf_deep_decode_u16 fills the constant units and decodes the packed ones (one wave a unit) into a
dense buffer, the raw units are copied next to them and idf_tile_scatter_raw_strided_u16 writes
them into the outputs through the outputs' own strides.  decode(images=...) and decode_region
decode exactly the units they touch.

Container IDFD (little-endian), laid out as IDFM's plane section is (idfcodec.units reads and
writes both up to the packed section, whose tables are parsed here):

  magic "IDFD", u16 version 1, u16 flags: 0, or the N of a file of interleaved states
  u32 n_images, u32 C, u32 tile_h, u32 tile_w, n_images x (u32 H, u32 W)
  the constant bitmap: U = N * C bits in unit order, LSB first, ceil(U / 8) bytes
  the packed bitmap: U - K bits over the units that are not constant
  the K constants as u16, in unit order
  u64 raw length, the raw units' samples as u16 in unit order
  u64 packed-section length, the packed section: u32 P, u8 shift[P] padded to 4 bytes,
      u32 sel[P], u64 state[P] ([P][N]), u32 nwords[P], u32 nesc[P], the rANS words of all units
      (unit order, push order), the low-bit words of all units, the escapes of all units as u16
      (unit order; raster order in a unit, wavefront order at N states) padded to 4 bytes

Not built: ways chosen per unit, several waves a unit, a colour transform between 16-bit planes,
sealing IDFD files, 16-bit sources in plane sets or in any flow path.
"""
from __future__ import annotations

import ctypes
import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .codec import RANS_L
from .dist import _to_device
from .predict import SYMBOLS_PER_PASS, _code_streams, passes, read_count
from .tiled import (_HDR, Reader, TileLayout, _ceil_div, output_views, pack_lengthed, pack_words,
                    read_words, source_views)
from .units import (CLASS_CONSTANT, CLASS_PACKED, CLASS_RAW, UnitSection, class_counts,
                    copy_raw_units, read_units, select_units)
from .units import unit_counts as unit_samples

MAGIC = b"IDFD"
NAME = "16-bit tiled bitstream"
UNIT_BYTES = 21             # a packed unit besides its words: shift 1, sel 4, state 8, counts 4 + 4
SHIFT_MAX = 8
WAYS = (1, 8, 16, 32, 64)   # the states of a packed unit a file may name
_FIELDS = 8                 # addr, H, W, y0, x0, unused, sy, sx (strides in bytes)


# ------------------------------------------------------------------ host arithmetic
def tw_max() -> int:
    """The widest tile idf_deep_decode_u16 decodes (a row of the unit is kept in LDS)."""
    return int(lib().idf_deep_tw_max())


def low_words(n, shift) -> np.ndarray:
    """int64: the u32 words of the low bits of units of n samples at shift s, ceil(n s / 32)"""
    return (np.asarray(n, dtype=np.int64) * np.asarray(shift, dtype=np.int64) + 31) // 32


def check_ways(ways) -> int:
    """ways as an int, or ValueError unless the kernels code it (WAYS)."""
    if isinstance(ways, bool) or not isinstance(ways, (int, np.integer)) or int(ways) not in WAYS:
        raise ValueError(f"ways {ways!r} is not one of {WAYS}")
    return int(ways)


def unit_overhead(ways: int = 1) -> int:
    """A packed unit besides its words, low bits and escapes: shift 1, sel 4, counts 4 + 4 and
    8 a state; UNIT_BYTES at one way."""
    return 13 + 8 * int(ways)


def ways_supported(th: int, tw: int, ways: int) -> bool:
    """Whether idf_deep_decode_ways_u16 decodes tiles of th x tw at `ways` > 1
    (idf_deep_ways_supported; host only): False where a unit does not fit its LDS."""
    rc = lib().idf_deep_ways_supported(int(th), int(tw), int(ways))
    if rc == _lib.IDF_ERR_UNSUPPORTED:
        return False
    check(rc, "idf_deep_ways_supported")
    return True


def packed_bytes(n, shift, nwords, nesc, ways: int = 1) -> np.ndarray:
    """int64: what a packed unit of `ways` states takes in a file"""
    return (unit_overhead(ways) + 4 * np.asarray(nwords, dtype=np.int64) + 4 * low_words(n, shift)
            + 2 * np.asarray(nesc, dtype=np.int64))


def unit_class(mn, mx, n, shift, nwords, nesc, ways: int = 1) -> np.ndarray:
    """uint8 per unit of CLASS_*, decided in this order: constant iff min == max; packed iff
    packed_bytes < 2 n (a tie stores raw); else raw."""
    const = np.asarray(mn) == np.asarray(mx)
    packs = packed_bytes(n, shift, nwords, nesc, ways) < 2 * np.asarray(n, dtype=np.int64)
    return np.where(const, CLASS_CONSTANT,
                    np.where(packs, CLASS_PACKED, CLASS_RAW)).astype(np.uint8)


def deep_section_bound(sizes, C: int, tile) -> int:
    """The bytes no IDFD file of these images exceeds: the header and the size table, two bytes a
    sample (a constant unit's two bytes, a packed unit's fields, words, low bits and escapes and
    a raw unit's samples are each at most the unit's 2 n bytes), the two bitmaps (at most
    ceil(U / 8) each), the two u64 lengths, the u32 count and the two pads of the packed section
    (at most 3 + 2 bytes, of which a packed unit's one byte below 2 n pays one)."""
    lay = TileLayout(sizes, int(C), tuple(tile))
    U = lay.n_tiles * int(C)
    return (struct.calcsize(_HDR) + 8 * len(lay.sizes) + 2 * lay.n_subpixels + 2 * _ceil_div(U, 8)
            + 8 + 8 + 4 + 4)


# ------------------------------------------------------------------ memory layouts
def source_views16(images, C: int, dev, layout=None) -> list:
    """tiled.source_views for uint16 sources; a host tensor is copied to dev."""
    return source_views(images, C, dev, layout, torch.uint16, host_ok=True, owner="codec")


def output_views16(shapes, dev, layout: str = "chw", out=None):
    """tiled.output_views for uint16 outputs."""
    return output_views(shapes, dev, layout, out, torch.uint16, owner="codec")


def unit_rows(rows, views, C: int) -> np.ndarray:
    """rows: planned rows (j, H, W, y0, x0) of some entries, views[j] the uint16 [C, H, W] view
    row j lies in -> int64 [n * C, 8], the table rows of their units, entry-major and
    plane-minor, strides in bytes."""
    out = np.zeros((len(rows) * C, _FIELDS), dtype=np.int64)
    k = 0
    for j, H, W, y, x in rows:
        v = views[j]
        sc = v.stride(0) if v.shape[0] > 1 else 0
        for p in range(C):
            out[k] = (v.data_ptr() + 2 * p * sc, H, W, y, x, 0, 2 * v.stride(1), 2 * v.stride(2))
            k += 1
    return out


def _host_ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------ the model on the host
def host_prep(unit, ways: int = 1) -> dict:
    """One dense unit uint16 [hin, win] in host memory through csrc/idf_deep.h's model
    (idf_deep_prep_host; no device) -> shift, sel, min, max, esc uint16 [n_esc], low uint32
    [ceil(n s / 32)] and x, mean, scale float32 [n] in stream order.  ways > 1: the symbols and
    the escapes in the wavefront order of that many states (idf_deep_prep_ways_host)."""
    u = np.ascontiguousarray(unit, dtype=np.uint16)
    if u.ndim != 2 or not u.size:
        raise ValueError("a unit is a uint16 array [hin, win] of at least one sample")
    n = u.size
    shift, sel, n_esc = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_int64()
    mm, esc = np.zeros(2, dtype=np.uint16), np.zeros(n, dtype=np.uint16)
    low = np.zeros(int(low_words(n, SHIFT_MAX)), dtype=np.uint32)
    x, mean, scale = (np.zeros(n, dtype=np.float32) for _ in range(3))
    outs = (ctypes.byref(shift), ctypes.byref(sel), _host_ptr(mm), ctypes.byref(n_esc),
            _host_ptr(esc), _host_ptr(low), _host_ptr(x), _host_ptr(mean), _host_ptr(scale))
    if ways != 1:
        check(lib().idf_deep_prep_ways_host(_host_ptr(u), u.shape[0], u.shape[1], int(ways),
                                            *outs), "idf_deep_prep_ways_host")
    else:
        check(lib().idf_deep_prep_host(_host_ptr(u), u.shape[0], u.shape[1], *outs),
              "idf_deep_prep_host")
    return {"shift": shift.value, "sel": sel.value, "min": int(mm[0]), "max": int(mm[1]),
            "esc": esc[:n_esc.value].copy(),
            "low": low[:int(low_words(n, shift.value))].copy(), "x": x, "mean": mean,
            "scale": scale}


def host_decode(hin: int, win: int, shift: int, sel: int, state: int, words, low, esc):
    """The serial decoder of csrc/idf_deep.h on the host (idf_deep_decode_host; no device) ->
    (uint16 [hin, win], final state, status)."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    esc = np.ascontiguousarray(esc, dtype=np.uint16)
    low = np.ascontiguousarray(low, dtype=np.uint32)
    low = np.concatenate([low, np.zeros(1, dtype=np.uint32)])   # a buffer even at shift 0
    out = np.zeros((int(hin), int(win)), dtype=np.uint16)
    final, status = ctypes.c_uint64(), ctypes.c_int32()
    check(lib().idf_deep_decode_host(int(hin), int(win), int(shift), int(sel), int(state),
                                     _host_ptr(words) if len(words) else None, len(words),
                                     _host_ptr(low), _host_ptr(esc) if len(esc) else None,
                                     len(esc), _host_ptr(out), ctypes.byref(final),
                                     ctypes.byref(status)), "idf_deep_decode_host")
    return out, final.value, status.value


def host_decode_ways(hin: int, win: int, ways: int, shift: int, sel: int, states, words, low,
                     esc):
    """The step-wise decoder of csrc/idf_deep.h at `ways` states on the host
    (idf_deep_decode_ways_host; no device): states holds `ways` values, esc is in wavefront
    order -> (uint16 [hin, win], final states uint64 [ways], status)."""
    states = np.ascontiguousarray(states, dtype=np.uint64)
    if states.shape != (int(ways),):
        raise ValueError(f"{len(states)} states for {ways} ways")
    words = np.ascontiguousarray(words, dtype=np.uint32)
    esc = np.ascontiguousarray(esc, dtype=np.uint16)
    low = np.ascontiguousarray(low, dtype=np.uint32)
    pad = max(int(low_words(int(hin) * int(win), SHIFT_MAX)) - len(low), 0) + 1
    low = np.concatenate([low, np.zeros(pad, dtype=np.uint32)])  # a run for any shift read as 8
    out = np.zeros((int(hin), int(win)), dtype=np.uint16)
    final, status = np.zeros(int(ways), dtype=np.uint64), ctypes.c_int32()
    check(lib().idf_deep_decode_ways_host(int(hin), int(win), int(ways), int(shift), int(sel),
                                          _host_ptr(states),
                                          _host_ptr(words) if len(words) else None, len(words),
                                          _host_ptr(low), _host_ptr(esc) if len(esc) else None,
                                          len(esc), _host_ptr(out), _host_ptr(final),
                                          ctypes.byref(status)), "idf_deep_decode_ways_host")
    return out, final, status.value


# ------------------------------------------------------------------ device calls
def device_deep_prep(rows: np.ndarray, counts: np.ndarray, th: int, tw: int, dev,
                     ways: int = 1):
    """The units the rows name, counts[t] = hin * win samples each -> a dict: the host tables
    off, low_off, esc_off (int64), the device tensors off, x, mean, scale, low, esc and, as
    numpy, minmax uint16 [n, 2], shift uint8, sel uint32, nesc int64 (idf_deep_prep_u16).
    ways > 1: the symbols and the escapes in the wavefront order of that many states
    (idf_deep_prep_ways_u16)."""
    n = len(rows)
    counts = np.asarray(counts, dtype=np.int64)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off_h[1:])
    low_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(low_words(counts, SHIFT_MAX), out=low_h[1:])
    nsym = int(off_h[-1])
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    d64 = _to_device(torch.from_numpy(np.concatenate([rows.reshape(-1), off_h, low_h[:n]])), dev)
    table, off, low_off = d64[:n * _FIELDS], d64[n * _FIELDS:n * _FIELDS + n + 1], \
        d64[n * _FIELDS + n + 1:]
    x, mean, scale = (torch.empty(max(nsym, 1), dtype=torch.float32, device=dev)
                      for _ in range(3))
    low = torch.empty(max(int(low_h[-1]), 1), dtype=torch.int32, device=dev)
    esc = torch.empty(max(nsym, 1), dtype=torch.int32, device=dev)
    minmax = torch.empty((n, 2), dtype=torch.int16, device=dev)
    shift = torch.empty(n, dtype=torch.uint8, device=dev)
    sel = torch.empty(n, dtype=torch.int32, device=dev)
    nesc = torch.empty(n, dtype=torch.int64, device=dev)
    args = (_lib.stream_ptr(dev), n, th, tw, ptr(table), _host_ptr(rows), ptr(off), ptr(low_off),
            ptr(off), ptr(x), ptr(mean), ptr(scale), ptr(low), ptr(esc), ptr(minmax), ptr(shift),
            ptr(sel), ptr(nesc))
    if ways != 1:
        check(lib().idf_deep_prep_ways_u16(*args, int(ways)), "deep prep")
    else:
        check(lib().idf_deep_prep_u16(*args), "deep prep")
    return {"off_h": off_h, "low_h": low_h, "off": off, "x": x, "mean": mean, "scale": scale,
            "low": low, "esc": esc, "minmax": minmax.cpu().numpy().view(np.uint16),
            "shift": shift.cpu().numpy(), "sel": sel.cpu().numpy().view(np.uint32),
            "nesc": nesc.cpu().numpy()}


def _gather(src: torch.Tensor, src_off: np.ndarray, counts: np.ndarray, dev) -> torch.Tensor:
    """src[src_off[k]:src_off[k] + counts[k]] of every k, joined (idf_gather_words)."""
    m = len(counts)
    dst_h = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(counts, out=dst_h[1:])
    total = int(dst_h[-1])
    out = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    if m and total:
        d64 = _to_device(torch.from_numpy(np.concatenate(
            [np.asarray(src_off, dtype=np.int64), np.asarray(counts, dtype=np.int64),
             dst_h[:m]])), dev)
        check(lib().idf_gather_words(_lib.stream_ptr(dev), m, ptr(d64[:m]), ptr(d64[m:2 * m]),
                                     ptr(d64[2 * m:]), ptr(src), ptr(out)), "deep gather")
    return out[:total]


def device_gather_raw16(rows: np.ndarray, counts: np.ndarray, th: int, tw: int,
                        dev) -> torch.Tensor:
    """The units the rows name as dense uint16 runs, joined -> device int16 [sum counts]
    (idf_tile_gather_raw_strided_u16)."""
    n = len(rows)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=off_h[1:])
    out = torch.empty(max(int(off_h[-1]), 1), dtype=torch.int16, device=dev)
    if n:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        d64 = _to_device(torch.from_numpy(np.concatenate([rows.reshape(-1), off_h[:n]])), dev)
        check(lib().idf_tile_gather_raw_strided_u16(
            _lib.stream_ptr(dev), n, th, tw, ptr(d64[:n * _FIELDS]), _host_ptr(rows),
            ptr(d64[n * _FIELDS:]), ptr(out)), "deep raw gather")
    return out[:int(off_h[-1])]


# ------------------------------------------------------------------ container
@dataclass
class DeepTiledBitstream(UnitSection):
    NAME, SAMPLE = NAME, np.uint16  # of the unit section behind the header
    sizes: list                 # [(H, W)] per image
    C: int
    tile_hw: tuple              # (th, tw)
    constant: np.ndarray        # bool [U], unit order: entry-major, plane-minor
    packed: np.ndarray          # bool [U]: not constant and coded
    values: np.ndarray          # uint16 [K]: the constant units' values, unit order
    raw: torch.Tensor           # uint8: the raw units' samples as little-endian bytes, unit order
    shift: np.ndarray           # uint8 [P], the packed units in unit order
    sel: np.ndarray             # uint32 [P]
    states: np.ndarray          # uint64 [P]; [P, ways] with ways > 1
    nwords: np.ndarray          # int64 [P]
    nesc: np.ndarray            # int64 [P]
    words: torch.Tensor         # int32 [sum nwords]: unit order, push order
    low: torch.Tensor           # int32 [sum ceil(n s / 32)]: the low-bit words, unit order
    escapes: np.ndarray         # uint16 [sum nesc]: unit order; raster order in a unit at one
                                # way, wavefront order with ways > 1
    ways: int = 1               # states per packed unit

    @property
    def layout(self) -> TileLayout:
        return TileLayout(self.sizes, self.C, self.tile_hw)

    @property
    def n_images(self) -> int:
        return len(self.sizes)

    def unit_samples(self) -> np.ndarray:
        return unit_samples(self.layout.rects, self.C)

    def n_samples(self) -> int:
        return self.layout.n_subpixels

    def bits(self) -> int:
        """of the units: 16 a constant, 16 a raw sample, the packed units' fields and runs"""
        n = self.unit_samples()[np.asarray(self.packed, dtype=bool)]
        return 8 * (2 * len(self.values) + int(self.raw.numel())
                    + int(packed_bytes(n, self.shift, self.nwords, self.nesc, self.ways).sum()))

    def bps(self) -> float:
        """bits per sample"""
        n = self.n_samples()
        return self.bits() / n if n else float("nan")

    def check(self):
        """Raises unless the parts fit each other."""
        ns = self.unit_samples()
        P, pk = self.check_units(ns), np.asarray(self.packed, dtype=bool)
        W = check_ways(self.ways)
        if np.asarray(self.states).shape != ((P, W) if W > 1 else (P,)):
            raise ValueError(f"{NAME} packs {P} units of {W} ways, its states number "
                             f"{np.asarray(self.states).shape}")
        if not (len(self.shift) == len(self.sel) == len(self.states) == len(self.nwords)
                == len(self.nesc) == P):
            raise ValueError(f"{NAME} packs {P} units, its tables hold {len(self.shift)}, "
                             f"{len(self.sel)}, {len(self.states)}, {len(self.nwords)} and "
                             f"{len(self.nesc)} rows")
        sh = np.asarray(self.shift, dtype=np.int64)
        if (sh > SHIFT_MAX).any():
            raise ValueError(f"{NAME} holds a shift of {int(sh.max())}, above {SHIFT_MAX}")
        self.check_words()
        n_low = int(low_words(ns[pk], sh).sum())
        if int(self.low.numel()) != n_low:
            raise ValueError(f"{NAME} holds {self.low.numel()} low-bit words, its shifts name "
                             f"{n_low}")
        ne = np.asarray(self.nesc, dtype=np.int64)
        if (ne < 0).any() or (ne > ns[pk]).any() or int(ne.sum()) != len(self.escapes):
            raise ValueError(f"{NAME} holds {len(self.escapes)} escapes, its escape counts name "
                             f"{int(ne.sum())}")

    def to_bytes(self) -> bytes:
        self.check()
        P = int(np.count_nonzero(self.packed))
        esc = np.asarray(self.escapes, dtype="<u2").tobytes()
        sect = (struct.pack("<I", P)
                + np.asarray(self.shift, dtype=np.uint8).tobytes() + b"\0" * (-P % 4)
                + np.asarray(self.sel, dtype="<u4").tobytes()
                + np.asarray(self.states, dtype="<u8").tobytes()
                + np.asarray(self.nwords, dtype=np.int64).astype("<u4").tobytes()
                + np.asarray(self.nesc, dtype=np.int64).astype("<u4").tobytes()
                + pack_words(self.words) + pack_words(self.low) + esc + b"\0" * (-len(esc) % 4))
        flags = self.ways if self.ways > 1 else 0
        return self.layout.pack(MAGIC, flags) + self.pack_units() + pack_lengthed(sect)

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "DeepTiledBitstream":
        lay, o = TileLayout.unpack(buf, MAGIC, NAME, flags_ok=(0,) + WAYS[1:])
        W = struct.unpack_from("<H", buf, 6)[0] or 1    # the header's flags: ways > 1
        at = f" at the {W} ways its flags name" if W > 1 else ""
        C = lay.C
        r = Reader(buf, NAME, o)
        constant, packed, values, raw = read_units(r, lay, C, np.uint16)
        ns = unit_samples(lay.rects, C)
        n_sect = r.u64()
        s = r.end(n_sect)
        P = read_count(s, n_sect, int(packed.sum()), "units")
        n_shift = P + (-P % 4)
        n_tab = 4 + n_shift + (unit_overhead(W) - 1) * P
        if n_sect < n_tab:
            raise ValueError(f"{NAME} holds a packed section of {n_sect} bytes, too short for "
                             f"the tables of {P} units" + at)
        shift = s.array(np.uint8, P).copy()
        if s.array(np.uint8, n_shift - P).any():
            raise ValueError(f"{NAME} holds a non-zero pad behind its shifts")
        if (shift > SHIFT_MAX).any():
            raise ValueError(f"{NAME} holds a shift of {int(shift.max())}, above {SHIFT_MAX}")
        sel = s.array("<u4", P).astype(np.uint32)
        states = s.array("<u8", P * W).astype(np.uint64)
        states = states.reshape(P, W) if W > 1 else states
        nwords = s.array("<u4", P).astype(np.int64)
        nesc = s.array("<u4", P).astype(np.int64)
        if (nesc > ns[packed]).any():
            raise ValueError(f"{NAME} names more escapes than a unit has samples" + at)
        total, n_low, n_esc = int(nwords.sum()), int(low_words(ns[packed], shift).sum()), \
            int(nesc.sum())
        n_escb = 2 * n_esc + (-2 * n_esc % 4)
        if n_sect != n_tab + 4 * total + 4 * n_low + n_escb:
            raise ValueError(f"{NAME} holds a packed section of {n_sect} bytes, its counts name "
                             f"{total} words, {n_low} low-bit words and {n_esc} escapes: "
                             f"{n_tab + 4 * total + 4 * n_low + n_escb} bytes" + at)
        words, low = read_words(s, total), read_words(s, n_low)
        escapes = s.array("<u2", n_esc).astype(np.uint16)
        if s.array(np.uint8, n_escb - 2 * n_esc).any():
            raise ValueError(f"{NAME} holds a non-zero pad behind its escapes")
        if device:
            raw, words, low = raw.to(device), words.to(device), low.to(device)
        return cls([tuple(s) for s in lay.sizes], C, lay.tile_hw, constant, packed, values, raw,
                   shift, sel, states, nwords, nesc, words, low, escapes, ways=W)


# ------------------------------------------------------------------ codec
class DeepTiledCodec:
    """Lists of uint16 images of `channels` channels, [C, H_i, W_i] or [H_i, W_i, C], of any sizes
    and strides, on the host or the device <-> DeepTiledBitstream (the module's doc has the
    model, the unit classes and the file).  tile: (th, tw), tw at most tw_max().  ways: the
    interleaved states of every packed unit encode writes (the module's doc has the order); decode
    and decode_region take a file's own."""

    def __init__(self, channels: int, tile=(64, 64), device=None, ways: int = 1):
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or \
                int(channels) < 1:
            raise ValueError(f"channels {channels!r} must be an integer of at least 1")
        self.C = int(channels)
        lay = TileLayout([(1, 1)], self.C, tuple(tile))     # checks the tile
        self.tile_hw = lay.tile_hw
        if self.tile_hw[1] > tw_max():
            raise ValueError(f"tiles of width {self.tile_hw[1]} exceed the decoder's row of "
                             f"{tw_max()} samples")
        self.ways = check_ways(ways)
        if self.ways > 1 and not ways_supported(*self.tile_hw, self.ways):
            raise ValueError(f"ways {self.ways} does not decode tiles of {self.tile_hw}: a unit "
                             "does not fit the decoder's LDS")
        self.device = None if device is None else torch.device(device)

    def _device(self) -> torch.device:
        dev = self.device if self.device is not None else torch.device("cuda")
        if dev.type != "cuda":
            raise _lib.IdfError("idfcodec: the 16-bit coder runs on a HIP device (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return dev

    # -------------------------------------------------------------- encode
    @torch.no_grad()
    def encode(self, images, layout=None) -> DeepTiledBitstream:
        """images: a list of uint16 tensors [C, H_i, W_i], or one [B, C, H, W] tensor;
        layout="hwc": [H_i, W_i, C].  With a layout named any strides are taken and the samples
        read where they lie; without one the tensors must be contiguous."""
        dev = self._device()
        C, (th, tw) = self.C, self.tile_hw
        views = source_views16(images, C, dev, layout)       # held to the end
        lay = TileLayout([v.shape[1:] for v in views], C, (th, tw))
        rows = unit_rows(lay.image_rows()[2], views, C)
        ns = unit_samples(lay.rects, C)
        U = len(ns)
        cls = np.zeros(U, dtype=np.uint8)
        mn = np.zeros(U, dtype=np.uint16)
        parts = []
        with torch.cuda.device(dev):
            for k, m in passes(ns, SYMBOLS_PER_PASS):
                part = self._code_pass(rows[k:k + m], ns[k:k + m], dev)
                cls[k:k + m], mn[k:k + m] = part.pop("cls"), part.pop("min")
                parts.append(part)
            r_idx = np.flatnonzero(cls == CLASS_RAW)
            raw = device_gather_raw16(rows[r_idx], ns[r_idx], th, tw, dev)
            torch.cuda.current_stream(dev).synchronize()     # the sources may go now

        def cat(key, dtype):
            empty = np.zeros((0, self.ways) if key == "states" and self.ways > 1 else 0, dtype)
            return np.concatenate([p[key] for p in parts] or [empty]).astype(dtype)

        def tcat(key):
            ts = [p[key] for p in parts if p[key].numel()]
            return torch.cat(ts) if ts else torch.zeros(0, dtype=torch.int32, device=dev)

        return DeepTiledBitstream(
            [tuple(s) for s in lay.sizes], C, (th, tw), cls == CLASS_CONSTANT,
            cls == CLASS_PACKED, mn[cls == CLASS_CONSTANT].copy(),
            raw.contiguous().view(torch.uint8), cat("shift", np.uint8), cat("sel", np.uint32),
            cat("states", np.uint64), cat("nwords", np.int64), cat("nesc", np.int64),
            tcat("words"), tcat("low"), cat("escapes", np.uint16), ways=self.ways)

    def _code_pass(self, rows, counts, dev) -> dict:
        """One pass of encode over the units the rows name -> their classes and minima and the
        packed ones' fields, words, low-bit words and escapes."""
        (th, tw), W = self.tile_hw, self.ways
        p = device_deep_prep(rows, counts, th, tw, dev, W)
        mm, shift, nesc = p["minmax"], p["shift"], p["nesc"]
        got = {}

        def keep(nw, status):
            # what the model guarantees (every symbol inside the window, every frequency >= 1)
            assert not status.any(), f"16-bit encode status {status[status != 0][:8]}"
            got["cls"] = unit_class(mm[:, 0], mm[:, 1], counts, shift, nw, nesc, W)
            return np.flatnonzero(got["cls"] == CLASS_PACKED)

        states, nw_h, _, words = _code_streams(p["off"], p["off_h"], p["x"], p["mean"],
                                               p["scale"], keep=keep, ways=W)
        pk = np.flatnonzero(got["cls"] == CLASS_PACKED)
        low = _gather(p["low"], p["low_h"][pk], low_words(counts[pk], shift[pk]), dev)
        esc = _gather(p["esc"], p["off_h"][pk], nesc[pk], dev)
        return {"cls": got["cls"], "min": mm[:, 0], "shift": shift[pk], "sel": p["sel"][pk],
                "states": states[pk], "nwords": nw_h[pk], "nesc": nesc[pk], "words": words,
                "low": low, "escapes": esc.cpu().numpy().astype(np.uint16)}

    # -------------------------------------------------------------- decode
    def check_bitstream(self, bs: DeepTiledBitstream):
        if (bs.C, tuple(bs.tile_hw)) != (self.C, self.tile_hw):
            raise ValueError(f"{NAME} of C {bs.C}, tiles {tuple(bs.tile_hw)} does not match the "
                             f"codec's C {self.C}, tiles {self.tile_hw}")
        bs.check()
        if bs.ways > 1 and not ways_supported(*self.tile_hw, bs.ways):
            raise ValueError(f"{NAME} of {bs.ways} ways does not decode at tiles {self.tile_hw}: "
                             "a unit does not fit the decoder's LDS")

    def _decode_units(self, bs: DeepTiledBitstream, entries, rows, views, verify: bool) -> dict:
        """The units of entries `entries` into views[j], rows[k] = (j, H, W, y0, x0) saying where
        entry k goes -> the decode info."""
        dev, (th, tw), C, W = self._device(), self.tile_hw, self.C, bs.ways
        cls = bs.classes
        units, ucls, u_rects, nb, out_h = select_units(cls, bs.layout.rects, entries, C)
        n = len(units)
        pk = np.flatnonzero(ucls == CLASS_PACKED)
        pidx = np.cumsum(cls == CLASS_PACKED) - 1
        which = pidx[units[pk]]
        info = {"tiles": len(entries), **class_counts(ucls),
                "escapes": int(np.asarray(bs.nesc, dtype=np.int64)[which].sum()),
                "damaged_planes": [], "plane_units": units[pk]}
        if verify:
            info["ok"] = True
        if not n:
            return info
        all_ns = bs.unit_samples()
        with torch.cuda.device(dev):
            buf = torch.empty(int(out_h[-1]), dtype=torch.int16, device=dev)
            copy_raw_units(buf, bs.raw, cls, all_ns, units, ucls, nb, out_h)    # as int16
            # the per-unit tables: zeros for the units that are not packed
            value = np.zeros(n, dtype=np.uint16)
            ck = np.flatnonzero(ucls == CLASS_CONSTANT)
            cidx = np.cumsum(cls == CLASS_CONSTANT) - 1
            value[ck] = np.asarray(bs.values, dtype=np.uint16)[cidx[units[ck]]]
            shift, sel = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
            t64 = np.zeros((6, n), dtype=np.int64)  # word_off, nwords, low_off, esc_off, nesc, out
            st = np.full((n, W), RANS_L, dtype=np.uint64)   # L where a unit is not packed
            nw_all = np.asarray(bs.nwords, dtype=np.int64)
            ne_all = np.asarray(bs.nesc, dtype=np.int64)
            lw_all = low_words(all_ns[cls == CLASS_PACKED], bs.shift)
            for row, counts in ((0, nw_all), (2, lw_all), (3, ne_all)):
                o = np.zeros(len(counts) + 1, dtype=np.int64)
                np.cumsum(counts, out=o[1:])
                t64[row, pk] = o[which]
            t64[1, pk], t64[4, pk] = nw_all[which], ne_all[which]
            t64[5] = out_h[:n]
            st[pk] = np.asarray(bs.states, dtype=np.uint64).reshape(-1, W)[which]
            shift[pk] = np.asarray(bs.shift, dtype=np.uint8)[which]
            sel[pk] = np.asarray(bs.sel, dtype=np.uint32)[which]
            d64 = _to_device(torch.from_numpy(np.concatenate(
                [t64.reshape(-1), st.reshape(-1).view(np.int64)])), dev)
            d64, d_state = d64[:6 * n].view(6, n), d64[6 * n:]
            small = _to_device(torch.from_numpy(np.concatenate(
                [u_rects.reshape(-1).view(np.uint8), sel.view(np.uint8), value.view(np.uint8),
                 ucls.astype(np.uint8), shift])), dev)
            d_rect, d_sel = small[:8 * n].view(torch.int32), small[8 * n:12 * n].view(torch.int32)
            d_value = small[12 * n:14 * n].view(torch.int16)
            d_cls, d_shift = small[14 * n:15 * n], small[15 * n:16 * n]

            def on_dev(t):   # streams of no word still name a buffer
                t = t if t.device == dev else t.to(dev)
                return t.contiguous() if t.numel() else torch.zeros(1, dtype=torch.int32,
                                                                    device=dev)
            words, low = on_dev(bs.words), on_dev(bs.low)
            esc = on_dev(_to_device(torch.from_numpy(
                np.asarray(bs.escapes, dtype=np.uint16).astype(np.int32)), dev))
            final = torch.empty(n * W, dtype=torch.int64, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            s = _lib.stream_ptr(dev)
            args = (ptr(d_cls), ptr(d_value), ptr(d_shift), ptr(d_sel), ptr(d_state), ptr(words),
                    ptr(d64[0]), ptr(d64[1]), ptr(low), ptr(d64[2]), ptr(esc), ptr(d64[3]),
                    ptr(d64[4]), ptr(d_rect), ptr(d64[5]), ptr(buf), ptr(final), ptr(status))
            if W > 1:   # a step of up to W samples at a time
                check(lib().idf_deep_decode_ways_u16(s, n, W, th, tw, *args), "deep decode")
                final = final.view(n, W)
            else:
                check(lib().idf_deep_decode_u16(s, n, th, tw, *args), "deep decode")
            out_rows = unit_rows(rows, views, C)
            table = _to_device(torch.from_numpy(out_rows.reshape(-1)), dev)
            check(lib().idf_tile_scatter_raw_strided_u16(
                s, n, th, tw, ptr(buf), ptr(d64[5]), ptr(d_rect), ptr(table),
                _host_ptr(out_rows)), "deep raw scatter")
            info["final_states"], info["status"] = final, status
            if verify:
                bad = ((final.view(n, W) != RANS_L).any(dim=1) | (status != 0)).cpu().numpy()
                info["damaged_planes"] = [int(u) for u in units[bad]]
                info["ok"] = not bad.any()
            else:
                torch.cuda.current_stream(dev).synchronize()  # the tables may go now
        return info

    @torch.no_grad()
    def decode(self, bs, images=None, verify: bool = True, layout: str = "chw", out=None):
        """-> (list of uint16 [C, H_i, W_i] (layout="hwc": [H_i, W_i, C]) or the caller's `out`,
        info).  images: the indices of the images to decode (default: all); only their units are
        decoded.  info counts them per class (constant_planes, packed_planes, raw_planes) and
        their escapes; with verify, damaged_planes lists the units (entry * C + plane) whose
        stream did not end as it was written, and they clear info['ok'].  info['final_states']
        is [n] of a one-way file and [n, ways] of a file of interleaved states."""
        self.check_bitstream(bs)
        lay = bs.layout
        want, entries, rows = lay.image_rows(images)
        outs, views = output_views16([(self.C, *lay.sizes[i]) for i in want], self._device(),
                                     layout, out)
        return outs, self._decode_units(bs, entries, rows, views, verify)

    @torch.no_grad()
    def decode_region(self, bs, image: int, y0: int, x0: int, h: int, w: int,
                      verify: bool = True, layout: str = "chw", out=None):
        """-> (uint16 [C, h, w], info): rows [y0, y0 + h) x columns [x0, x0 + w) of one image,
        from exactly the units of the tiles that intersect them."""
        self.check_bitstream(bs)
        entries, rows = bs.layout.region_rows(image, y0, x0, h, w)
        outs, views = output_views16([(self.C, int(h), int(w))], self._device(), layout,
                                     None if out is None else [out])
        return outs[0], self._decode_units(bs, entries, rows, views, verify)


__all__ = ["MAGIC", "NAME", "SHIFT_MAX", "UNIT_BYTES", "WAYS", "DeepTiledBitstream",
           "DeepTiledCodec", "check_ways", "deep_section_bound", "device_deep_prep",
           "device_gather_raw16", "host_decode", "host_decode_ways", "host_prep", "low_words",
           "output_views16", "packed_bytes", "source_views16", "tw_max", "unit_class",
           "unit_overhead", "unit_rows", "ways_supported"]
