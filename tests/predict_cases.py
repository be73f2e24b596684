"""The shared case set of the 8-bit predictive decoders' tests: small coded units and every way
of damaging one (damage_kinds, damaged), the references' verdict on each (damage_set), and
big_units(), the geometries at the kernels' limits.  No test lives here.

tests/test_predict_cases_host.py checks through the references alone that the damage set yields
every outcome its users rely on and that the big geometries reach the regimes they are there for,
so that tests/test_gpu_predict_damage.py and tests/test_gpu_predict_big.py cannot pass on a set
that has stopped covering anything.

An entry is (sel, sel2 or None, states, words): states a tuple of N ints (one at one way), words
np.uint32 in push order, so the decoder reads words[-1] first and words[0] last."""
import functools
from collections import namedtuple

import numpy as np

import colour_ref as cref
import predict_ref as ref
import predict_ways_ref as wref
from test_predict_host import contents

Entry = namedtuple("Entry", "sel sel2 states words")

L = ref.L
CONTENTS = ("zeros", "ramp", "vstep", "noise")
UNIT_SHAPES = ((3, 16, 16), (1, 12, 8))
WORD_OPS = {"^0x00010000": lambda v: v ^ 0x00010000, "^0x80000000": lambda v: v ^ 0x80000000,
            "=0": lambda v: 0, "=0xFFFFFFFF": lambda v: 0xFFFFFFFF}
WORD_PLACES = ("first read", "middle", "last read")
EXTRA_WORD = 0x9E3779B9


def units(shape):
    """-> [(content name, uint8 [C, h, w])]"""
    c = contents(shape)
    return [(name, c[name]) for name in CONTENTS]


def encode(planes, N=1, colour=False) -> Entry:
    """The references' intact coding of one unit."""
    if N == 1:
        if colour:
            sel, sel2, state, words = cref.encode(planes)
        else:
            (sel, state, words), sel2 = ref.encode(planes), None
        return Entry(int(sel), sel2, (int(state),), np.asarray(words, dtype=np.uint32))
    sel, sel2, S, words = wref.encode(planes, N, colour)
    return Entry(int(sel), sel2, tuple(int(s) for s in S), np.asarray(words, dtype=np.uint32))


# ------------------------------------------------------------------ damage
def damage_kinds():
    """The names damaged() takes: 12 word changes (4 values at 3 places), 4 changes of the word
    count, 2 initial states, 2 values of sel and of sel2, and the colour flag flipped."""
    return ([f"word {op} at the {place}" for op in WORD_OPS for place in WORD_PLACES] +
            ["first pushed word dropped", "last pushed word dropped", "an extra word in front",
             "no words", "state below L", "state bit 63", "sel = 0", "sel = 0xFFFFFFFF",
             "sel2 = 0", "sel2 = 0xFFFFFFFF", "colour flag flipped"])


def damaged(entry: Entry, kind: str, C: int = 3):
    """-> the damaged Entry, or None where the entry has no room for the change (a word of an
    entry without words, sel2 of a plain entry, a colour flag with fewer than three planes).
    Values change and the word count moves; nothing points outside the entry's own arrays."""
    sel, sel2, states, words = entry
    if kind.startswith("word "):
        if not len(words):
            return None
        _, op, _, _, place = kind.split(" ", 4)
        i = {"first read": len(words) - 1, "middle": len(words) // 2, "last read": 0}[place]
        w = words.copy()
        w[i] = WORD_OPS[op](int(w[i]))
        return entry._replace(words=w)
    if kind == "first pushed word dropped":
        return entry._replace(words=words[1:].copy()) if len(words) else None
    if kind == "last pushed word dropped":
        return entry._replace(words=words[:-1].copy()) if len(words) else None
    if kind == "an extra word in front":
        return entry._replace(words=np.concatenate([np.array([EXTRA_WORD], np.uint32), words]))
    if kind == "no words":
        return entry._replace(words=words[:0].copy()) if len(words) else None
    if kind == "state below L":
        return entry._replace(states=(states[0] >> 8,) + states[1:])
    if kind == "state bit 63":
        return entry._replace(states=states[:-1] + (states[-1] | 1 << 63,))
    if kind in ("sel = 0", "sel = 0xFFFFFFFF"):
        return entry._replace(sel=int(kind[6:], 0))
    if kind in ("sel2 = 0", "sel2 = 0xFFFFFFFF"):
        return None if sel2 is None else entry._replace(sel2=int(kind[7:], 0))
    if kind == "colour flag flipped":
        if C < 3:
            return None
        return entry._replace(sel2=0 if sel2 is None else None)   # a plain entry gains table 0
    raise ValueError(kind)


def reference(entry: Entry, C, h, w, N=1, stop="step"):
    """What the header promises of the entry decoded as a C x h x w rectangle -> (bytes uint8
    [C, h, w] -- v for a colour entry --, the final states as a list, status, trace): by
    predict_ref / colour_ref at one way, by predict_ways_ref with the device's step rule at N."""
    trace = {}
    if N == 1:
        if entry.sel2 is None:
            out, S, st = ref.decode(entry.sel, entry.states[0], entry.words, C, h, w, trace)
        else:
            out, S, st = cref.decode(entry.sel, entry.sel2, entry.states[0], entry.words, C, h, w,
                                     trace)
        return out, [S], st, trace
    out, S, st = wref.decode(entry.sel, entry.states, entry.words, C, h, w, N, entry.sel2, stop,
                             trace)
    return out, S, st, trace


Case = namedtuple("Case", "name entry rect planes want")
# name: what it is; rect: the (hin, win) handed to the decoder; planes: the intact bytes or None
# for a damaged entry; want: reference() of the entry at the rectangle held to the tile


@functools.lru_cache(maxsize=None)
def damage_set(shape, N=1):
    """Every damaged form of every unit of `shape` = (C, th, tw), each behind an intact entry,
    and the rectangle cases, as one launch holds them -> [Case].  With C >= 3 the units are coded
    as colour entries too; plain_only() keeps what a decoder without colour flags can be given.
    Computed once per argument set and shared, never modified."""
    C, th, tw = shape
    us = units(shape)
    modes = (False, True) if C >= 3 else (False,)
    coded = {(name, col): encode(p, N, col) for name, p in us for col in modes}
    intact = [Case(f"intact {name} {'colour' if col else 'plain'}", coded[name, col], (th, tw), p,
                   reference(coded[name, col], C, th, tw, N))
              for col in modes for name, p in us]
    out, k = [], 0
    for col in modes:
        for name, p in us:
            for kind in damage_kinds():
                bad = damaged(coded[name, col], kind, C)
                if bad is None:
                    continue
                out.append(intact[k % len(intact)])
                k += 1
                out.append(Case(f"{name} {'colour' if col else 'plain'}: {kind}", bad, (th, tw),
                                None, reference(bad, C, th, tw, N)))
    # rectangles: above the tile (decoded as the tile), and negative (no symbol)
    ramp = next(c for c in intact if c.name.startswith("intact ramp"))
    out.append(ramp._replace(name="rect above the tile", rect=(th + 3, tw + 70)))
    for rect in ((-1, tw), (th, -5), (-2, -2)):
        e = ramp.entry
        out.append(Case(f"rect {rect}", e, rect, None, reference(e, C, 0, 0, N)))
    none = ramp.entry._replace(words=ramp.entry.words[:0].copy())
    out.append(Case("rect (-1, -1) without words", none, (-1, -1), None,
                    reference(none, C, 0, 0, N)))
    out.append(intact[0])
    return out


def plain_only(cases):
    """The cases whose entry carries no colour flag (a colour coding whose flag was cleared is
    one of them)."""
    return [c for c in cases if c.entry.sel2 is None]


def reverse_layout(sizes, gap=5):
    """Output offsets handed out in reverse entry order with `gap` unused bytes behind each:
    -> (offsets, total)."""
    offs, o = [0] * len(sizes), 0
    for e in reversed(range(len(sizes))):
        offs[e] = o
        o += int(sizes[e]) + gap
    return offs, o


def launch_arrays(cases, N=1):
    """The decoder's per-entry arguments for a list of Case: words concatenated in entry order."""
    nw = np.array([len(c.entry.words) for c in cases], dtype=np.int64)
    w_off = np.zeros(len(cases), dtype=np.int64)
    np.cumsum(nw[:-1], out=w_off[1:])
    words = np.concatenate([c.entry.words for c in cases] + [np.zeros(1, np.uint32)])
    return {"words": words.astype(np.uint32), "w_off": w_off, "nw": nw,
            "states": np.array([c.entry.states for c in cases], dtype=np.uint64).reshape(-1, N),
            "sel": np.array([c.entry.sel for c in cases], dtype=np.uint32),
            "sel2": np.array([c.entry.sel2 or 0 for c in cases], dtype=np.uint32),
            "col": np.array([c.entry.sel2 is not None for c in cases], dtype=np.uint8),
            "rects": np.array([c.rect for c in cases], dtype=np.int32)}


# ------------------------------------------------------------------ the big geometries
TILE64 = (64, 64)
SIZES64 = ((64, 64), (65, 64), (64, 65), (69, 69))     # rects: full, 1x64, 64x1, 5x5, 64x5, 5x64


def smooth(C, h, w, seed):
    """A ramp plus noise 0..3 (packs at every geometry below): uint8 [C, h, w]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = np.arange(C).reshape(C, 1, 1)
    return ((3 * yy + 2 * xx + 40 * ch + rng.integers(0, 4, (C, h, w))) % 256).astype(np.uint8)


def big_units():
    """-> [(kind, C, th, tw, the N to run, [uint8 [C, hin, win]])]: kernel-level tiles that are no
    model's.  What each is for; test_predict_cases_host.py asserts the figures.

    ways (2, 70, 130)   win > N at every N, N = 64 included: P = win, a band's rows end P - win
                        = 0 steps before the next band's begin; 140 rows are 3 bands at N = 64
                        (the last of 12 rows), 18 at N = 8; a 70 x 65 rectangle inside it
                        (win > 64 by one, rows of the tile's LDS stride unused).
    ways (1, 3, 200)    R = 3 < N = 64 with win > N: one partly filled band.
    ways (4, 120, 126)  the largest LDS the N-way decoder accepts, 61280 of 61440 bytes.
    one  (1, 1, 32768)  the one-way decoder's LDS row at its limit (PRED_TW_MAX), 512 stores.
    one  (4, 1, 15000)  four one-row planes: toff and the plane change at a row end."""
    return [("ways", 2, 70, 130, (8, 16, 32, 64), [smooth(2, 70, 130, 1), smooth(2, 70, 65, 2)]),
            ("ways", 1, 3, 200, (64,), [smooth(1, 3, 200, 3)]),
            ("ways", 4, 120, 126, (64, 8), [smooth(4, 120, 126, 4)]),
            ("one", 1, 1, 32768, (1,), [smooth(1, 1, 32768, 5)]),
            ("one", 4, 1, 15000, (1,), [smooth(4, 1, 15000, 6)])]


def ways_lds_bytes(C, th, tw):
    """The header's formula: 320 + pad16(C th) + pad16(C th tw)"""
    pad16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    return 320 + pad16(C * th) + pad16(C * th * tw)


@functools.lru_cache(maxsize=None)
def case64(C):
    """Every content of CONTENTS at every size of SIZES64 cut into 64 x 64 tiles: the images, the
    entries' bytes in entry order and their counts.  Shared, never modified."""
    from idfcodec.safe import entry_rects
    from idfcodec.tiled import tile_table
    th, tw = TILE64
    sizes, imgs = [], []
    for i, (H, W) in enumerate(SIZES64):
        c = contents((C, H, W), seed=17 * i)
        for name in CONTENTS:
            sizes.append((H, W))
            imgs.append(c[name])
    rects = entry_rects(sizes, th, tw)
    _, entries = tile_table(sizes, th, tw)
    planes = [np.ascontiguousarray(imgs[i][:, ty * th:ty * th + h, tx * tw:tx * tw + w])
              for (i, ty, tx), (h, w) in zip(entries, rects)]
    names = [CONTENTS[i % len(CONTENTS)] for i, _, _ in entries]
    counts = np.array([p.size for p in planes], dtype=np.int64)
    return {"sizes": sizes, "imgs": imgs, "rects": [tuple(r) for r in rects], "planes": planes,
            "names": names, "counts": counts}


@functools.lru_cache(maxsize=None)
def coded64(C, N=1, colour=False):
    """The reference's coding of case64(C): plain candidates alone, or (colour) stream 2e the
    plain and 2e + 1 the colour candidate of entry e.  -> sel uint32 [n] or [n, 3], symbols, off,
    states [streams, N], nw, the words compact in stream order and their offsets."""
    import rans_oracle
    import rans_ways_ref
    case = case64(C)
    planes = case["planes"]
    if colour:
        sel = np.array([(ref.choose_sel(p),) + cref.choose_sels(p) for p in planes], np.uint32)
        arrs = []
        for p, s in zip(planes, sel):
            if N == 1:
                arrs += [ref.arrays(p, int(s[0])), cref.arrays(p, int(s[1]), int(s[2]))]
            else:
                arrs += [wref.arrays(p, N, int(s[0])),
                         wref.colour_arrays(p, N, int(s[1]), int(s[2]))]
        counts = np.repeat(case["counts"], 2)
    else:
        sel = np.array([ref.choose_sel(p) for p in planes], dtype=np.uint32)
        arrs = [ref.arrays(p, int(s)) if N == 1 else wref.arrays(p, N, int(s))
                for p, s in zip(planes, sel)]
        counts = case["counts"]
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    x, mean, scale = (np.concatenate([a[i] for a in arrs]) for i in range(3))
    if N == 1:
        fs, words, nw, status = rans_oracle.encode_streams(off, x, mean, scale)
        assert not status.any()
    else:
        fs, words, nw = rans_ways_ref.encode_streams(off, x, mean, scale, N)
    w_off = np.zeros(len(nw) + 1, dtype=np.int64)
    np.cumsum(nw, out=w_off[1:])
    compact = np.concatenate([words[a:a + n] for a, n in zip(off[:-1], nw)] +
                             [np.zeros(0, np.uint32)]).astype(np.uint32)
    return {"sel": sel, "x": x, "mean": mean, "scale": scale, "off": off,
            "states": np.asarray(fs, dtype=np.uint64).reshape(-1, N), "nw": np.asarray(nw),
            "words": compact, "w_off": w_off}
