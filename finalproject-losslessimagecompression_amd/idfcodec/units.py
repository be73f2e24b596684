"""The unit section: what an IDFM file's plane section (idfcodec.planes: uint8 units) and an IDFD
file (idfcodec.deep: uint16 units) hold behind their headers, and what both codecs do with it on
the host.

A *unit* is one plane of one tile's in-image rectangle, [hin][win] samples; units are ordered
entry-major and plane-minor.  Every unit is in one class: constant (one sample is stored), packed
(coded; the codec's own packed section holds it) or raw (its samples are stored).  The section:

  the constant bitmap: U bits in unit order, LSB first, ceil(U / 8) bytes
  the packed bitmap: U - K bits over the units that are not constant
  the K constants, one sample each, in unit order
  u64 raw length in bytes, the raw units' samples in unit order
  u64 packed-section length, the packed section (the codec's: its tables, words and runs)

Samples of two bytes are little-endian.  read_units and pack_units stop in front of the packed
section's length; UnitSection is what both bitstreams derive from these parts; select_units,
class_counts and copy_raw_units open both codecs' decode.
"""
from __future__ import annotations

import numpy as np
import torch

from .tiled import Reader, TileLayout, check_words, pack_bitmap, pack_lengthed

CLASS_CONSTANT, CLASS_PACKED, CLASS_RAW = 0, 1, 2


# ------------------------------------------------------------------ host arithmetic
def classes_of(constant, packed) -> np.ndarray:
    """uint8 [U] of CLASS_*"""
    return np.where(np.asarray(constant, dtype=bool), CLASS_CONSTANT,
                    np.where(np.asarray(packed, dtype=bool), CLASS_PACKED,
                             CLASS_RAW)).astype(np.uint8)


def unit_counts(rects, C: int) -> np.ndarray:
    """int64 [N * C]: hin * win of every unit, entry-major and plane-minor"""
    return np.repeat(np.array([h * w for h, w in rects], dtype=np.int64).reshape(len(rects)),
                     int(C))


def _runs(src_off, dst_off, n_bytes):
    """Byte copies (src, dst, n), in order -> the fewest copies that do the same: neighbours
    that continue each other on both sides are joined."""
    out = []
    for s, d, n in zip(src_off, dst_off, n_bytes):
        s, d, n = int(s), int(d), int(n)
        if out and out[-1][0] + out[-1][2] == s and out[-1][1] + out[-1][2] == d:
            out[-1][2] += n
        else:
            out.append([s, d, n])
    return out


# ------------------------------------------------------------------ container
def read_units(r: Reader, lay: TileLayout, C: int, sample):
    """r: at the constant bitmap of the unit section of C planes of lay's entries, samples of
    dtype `sample` -> (constant bool [U], packed bool [U], values [K] of sample, raw uint8); r
    is left at the packed section's length."""
    sample = np.dtype(sample)
    constant = r.bitmap(lay.n_tiles * C, "constant", "units")
    packed = r.sub_bitmap(~constant, "packed", "coded units")
    values = r.array(sample.newbyteorder("<"), int(constant.sum()), "constants",
                     then=8).astype(sample)
    # the file holds a bit a unit: only now is a table of the units known to be affordable
    want = sample.itemsize * int(unit_counts(lay.rects, C)[~constant & ~packed].sum())
    raw = r.lengthed(want, "raw bytes" if sample.itemsize == 1 else "raw samples", "raw units",
                     then=8)
    return constant, packed, values, torch.from_numpy(raw.copy())


class UnitSection:
    """What the two bitstreams of units derive from their constant, packed, values, raw, nwords
    and words; NAME is the container's, SAMPLE its units' dtype."""
    NAME = None
    SAMPLE = None

    @property
    def n_units(self) -> int:
        return len(self.constant)

    @property
    def stored_raw(self) -> np.ndarray:
        """bool [U]: neither constant nor packed"""
        return ~np.asarray(self.constant, dtype=bool) & ~np.asarray(self.packed, dtype=bool)

    @property
    def classes(self) -> np.ndarray:
        """uint8 [U] of CLASS_*"""
        return classes_of(self.constant, self.packed)

    def check_units(self, counts) -> int:
        """Raises unless the flags, the constants and the raw bytes fit the units of counts[u]
        samples; -> the number of packed units."""
        name, U = self.NAME, len(counts)
        if len(self.constant) != U or len(self.packed) != U:
            raise ValueError(f"{len(self.constant)} constant and {len(self.packed)} packed flags "
                             f"for {U} units")
        const, pk = np.asarray(self.constant, dtype=bool), np.asarray(self.packed, dtype=bool)
        if (const & pk).any():
            raise ValueError(f"{name} packs a unit it holds as a constant")
        if len(self.values) != int(const.sum()):
            raise ValueError(f"{name} flags {int(const.sum())} constant units, holds "
                             f"{len(self.values)} constants")
        n_raw = np.dtype(self.SAMPLE).itemsize * int(counts[self.stored_raw].sum())
        if self.raw.dtype != torch.uint8 or int(self.raw.numel()) != n_raw:
            raise ValueError(f"{name} holds {self.raw.numel()} raw bytes, its raw units {n_raw}")
        return int(pk.sum())

    def check_words(self):
        check_words(self.NAME, self.nwords, self.words)

    def pack_units(self) -> bytes:
        """What read_units reads."""
        const = np.asarray(self.constant, dtype=bool)
        return (pack_bitmap(const) + pack_bitmap(self.packed, over=~const)
                + np.asarray(self.values, dtype=np.dtype(self.SAMPLE).newbyteorder("<")).tobytes()
                + pack_lengthed(self.raw))


# ------------------------------------------------------------------ decode
def select_units(cls, rects, entries, C: int):
    """The C units of each of `entries`, which go into one dense buffer in that order -> (units
    int64 [n], their classes uint8 [n], their rectangles int32 [n, 2], their samples int64 [n],
    their offsets in the buffer int64 [n + 1])."""
    units = np.array([e * C + p for e in entries for p in range(C)], dtype=np.int64)
    ucls = cls[units] if len(units) else np.zeros(0, dtype=np.uint8)
    u_rects = np.array([rects[e] for e in entries for _ in range(C)],
                       dtype=np.int32).reshape(-1, 2)
    nb = u_rects[:, 0].astype(np.int64) * u_rects[:, 1]
    out_h = np.zeros(len(units) + 1, dtype=np.int64)
    np.cumsum(nb, out=out_h[1:])
    return units, ucls, u_rects, nb, out_h


def class_counts(ucls) -> dict:
    """The decode info's counts of the units asked, per class."""
    return {"constant_planes": int((ucls == CLASS_CONSTANT).sum()),
            "packed_planes": int((ucls == CLASS_PACKED).sum()),
            "raw_planes": int((ucls == CLASS_RAW).sum())}


def copy_raw_units(buf: torch.Tensor, raw: torch.Tensor, cls, counts, units, ucls, nb, out_h):
    """The raw ones of the units select_units chose, from the file's raw bytes (all raw units in
    unit order; cls and counts are all units') into the dense buffer buf, whose dtype is the
    samples': one copy a run of units that are neighbours on both sides."""
    rk = np.flatnonzero(ucls == CLASS_RAW)
    if not len(rk):
        return
    r_off = np.zeros(len(cls) + 1, dtype=np.int64)
    np.cumsum(np.where(cls == CLASS_RAW, counts, 0), out=r_off[1:])
    raw = raw if raw.device == buf.device else raw.to(buf.device)
    raw = raw.contiguous().view(buf.dtype)
    for s, d, m in _runs(r_off[units[rk]], out_h[rk], nb[rk]):
        buf[d:d + m].copy_(raw[s:s + m])


__all__ = ["CLASS_CONSTANT", "CLASS_PACKED", "CLASS_RAW", "UnitSection", "class_counts",
           "classes_of", "copy_raw_units", "read_units", "select_units", "unit_counts"]
