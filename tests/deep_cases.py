"""The shared case set of the 16-bit coder's tests: the small random and hand-made units of
tests/test_deep_host.py, and mechanics_units(), units made for named lines of
csrc/deep_kernels.hip.

tests/test_deep_cases_host.py checks through deep_ref alone that the mechanics set covers what its
comments claim (every shift among the packed units, every scale nibble, refills of both windows,
escapes of both signs and at both ends, long one-row and one-column units), so that
tests/test_gpu_deep_units.py cannot pass on a set that has stopped covering anything."""
import numpy as np

KINDS = ("uniform", "salt", "gauss", "outliers", "depth")


def random_unit(rng, kind, h, w):
    if kind == "uniform":
        u = rng.integers(0, 65536, (h, w))
    elif kind == "salt":
        u = rng.choice([0, 65535], (h, w))
    elif kind == "gauss":
        u = rng.integers(0, 65536) + rng.normal(0, 10 ** rng.uniform(0, 4), (h, w))
    elif kind == "outliers":
        u = rng.integers(0, 65536) + rng.normal(0, 3, (h, w))
        m = rng.random((h, w)) < 0.05
        u[m] = rng.integers(0, 65536, int(m.sum()))
    else:
        u = rng.integers(0, 1 << int(rng.integers(1, 17)), (h, w))
    return np.clip(np.rint(u), 0, 65535).astype(np.uint16)


def hand_units():
    esc00 = np.full((4, 5), 100, dtype=np.uint16)           # (0, 0) is 32668 from its prediction
    esc00[1:, 2:] += np.arange(12, dtype=np.uint16).reshape(3, 4)[:, :3]
    return [np.array([[12345]], dtype=np.uint16),
            np.arange(7, dtype=np.uint16)[None] * 300 + 5,
            np.arange(7, dtype=np.uint16)[:, None] * 300 + 5,
            np.full((6, 9), 777, dtype=np.uint16),
            (np.indices((8, 8)).sum(0) % 2 * 65535).astype(np.uint16),
            esc00]


def small_units():
    """The 306 units of test_deep_host.py's unit_set: 300 random ones of at most 16 x 16 and the
    hand units."""
    rng = np.random.default_rng(16)
    units = [random_unit(rng, KINDS[i % 5], int(rng.integers(1, 17)), int(rng.integers(1, 17)))
             for i in range(300)]
    return units + hand_units()


# ------------------------------------------------------------------ the mechanics set
SHAPES = ((1, 16384), (2, 16384), (3, 1000), (1000, 3), (4096, 1), (5, 257), (1, 1), (1, 63),
          (1, 65), (255, 1))
SIGMAS = (0.15, 0.3, 0.6, 1.2, 2.5)
TAILS = ((0.1, 300), (0.1, 3000), (0.1, 30000), (0.05, 60000), (0.12, 1000))  # (p, A)


def _u16(a):
    return np.clip(np.rint(a), 0, 65535).astype(np.uint16)


def _ramp(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return 30000 + 7 * yy + 5 * xx


def mechanics_units():
    """-> [(name, uint16 [h, w])].  What each group is for (deep_decode_kernel unless prep is
    named); test_deep_cases_host.py asserts the figures.

    shift s      48 x 48 at every shift 0..8: 370 and more rANS words, so the 128-word window
                 (wA, wB) refills five times, and 72 s low-bit words, so the 64-word low window
                 (wi - lbase >= 63) refills for every s >= 1; prep's word gather (rf..rl) at every
                 field width.
    sigma, tail  packed units whose buckets take the scale nibbles 0..13: the guess and its one
                 exact round at narrow scales, the fallback rounds (!found) deep in a tail.
    noise, salt, checker   nibbles 14 and 15 in most or all buckets; raw in a file, so only a
                 direct call decodes them.
    low, high    samples clipped at 0 and at 65535.
    esc+, esc-, esc last, esc pair   escapes above and below the prediction, at the last sample
                 and side by side (the hand units hold one at (0, 0)).
    h x w        the LDS row at idf_deep_tw_max() samples, one-row units (up never true) and
                 one-column units (win == 1: b is the sample just decoded) of more than 64 samples,
                 prep's chunks of 256 inside one row and across rows of 3 and 257, units of 1, 63
                 and 65 samples around the 64-sample store."""
    out = []
    for s in range(9):
        rng = np.random.default_rng(100 + s)
        out.append((f"shift {s}", _u16(_ramp(48, 48) + rng.normal(0, 6 * 2 ** s, (48, 48)))))
    for i, sigma in enumerate(SIGMAS):
        rng = np.random.default_rng(200 + i)
        out.append((f"sigma {sigma}", _u16(_ramp(32, 32) + rng.normal(0, sigma, (32, 32)))))
    for i, (p, A) in enumerate(TAILS):
        rng = np.random.default_rng(300 + i)
        u = _ramp(32, 32) + rng.normal(0, 1.5, (32, 32))
        hit = rng.random((32, 32)) < p
        out.append((f"tail {p} {A}", _u16(u + hit * rng.uniform(-A, A, (32, 32)))))
    rng = np.random.default_rng(400)
    out.append(("noise", _u16(rng.integers(0, 65536, (32, 32)))))
    out.append(("salt", _u16(rng.choice([0, 65535], (32, 32)))))
    out.append(("checker", (np.indices((32, 32)).sum(0) % 2 * 65535).astype(np.uint16)))
    # the ends of the range
    rng = np.random.default_rng(500)
    out.append(("low", _u16(rng.normal(0, 40, (32, 32)))))
    out.append(("high", _u16(65535 + rng.normal(0, 40, (32, 32)))))
    yy, xx = np.mgrid[0:32, 0:32]
    u = 1000 + 3 * yy + 2 * xx + rng.normal(0, 1, (32, 32))
    hit = rng.random((32, 32)) < 0.02
    u[hit] = rng.integers(20000, 65536, int(hit.sum()))
    out.append(("esc+", _u16(u)))
    u = 64000 + rng.normal(0, 1, (32, 32))
    hit = rng.random((32, 32)) < 0.02
    u[hit] = rng.integers(0, 3000, int(hit.sum()))
    out.append(("esc-", _u16(u)))
    u = 40000 + 2 * yy + rng.normal(0, 1, (32, 32))
    u[31, 31] = 900
    out.append(("esc last", _u16(u)))
    u = 40000 + 2 * yy + rng.normal(0, 1, (32, 32))
    u[9, 13], u[9, 14] = 65000, 200
    out.append(("esc pair", _u16(u)))
    # shapes
    for h, w in SHAPES:
        rng = np.random.default_rng(9)
        yy, xx = np.mgrid[0:h, 0:w]
        out.append((f"{h} x {w}", _u16(12000 + 3 * yy + 2 * xx % 5000 + rng.normal(0, 20, (h, w)))))
    return out


# ------------------------------------------------------------------ damaged units
SHIFT_MAX = 8


def low_slot(low, n: int) -> np.ndarray:
    """A unit's low-bit words in a run sized for SHIFT_MAX, ceil(8 n / 32) words, zero-padded: what
    the direct decode calls are given at every shift, a damaged one included."""
    slot = np.zeros((n * SHIFT_MAX + 31) // 32, dtype=np.uint32)
    slot[:len(low)] = low
    return slot


def damage_units():
    """About 40 units of 16 x 16 and fewer samples: every eighth of the small set, and 16 x 16
    corners of the range-ends group (the last one keeps its escape at the last sample)."""
    ends = dict(mechanics_units())
    cut = [ends[k][:16, :16] for k in ("low", "high", "esc+", "esc-", "esc pair")]
    cut.append(ends["esc last"][16:, 16:])
    return small_units()[::8] + [np.ascontiguousarray(c) for c in cut]


def damaged(unit, m, state, words, bucket_of):
    """The damaged forms of one coded unit: m, state, words from deep_ref.encode(unit), bucket_of =
    deep_ref.buckets -> [(change, dict(shift, sel, state, words, low, esc))], low a low_slot.
    Contents change and counts move by one; a change the unit has no room for is left out."""
    words = np.asarray(words, dtype=np.uint32)
    base = {"shift": m["shift"], "sel": m["sel"], "state": int(state), "words": words,
            "low": low_slot(m["low"], unit.size), "esc": np.asarray(m["esc"], dtype=np.uint16)}
    out = []

    def add(change, **kw):
        out.append((change, {**base, **kw}))

    if len(words):
        add("last word dropped", words=words[:-1])
        mid = words.copy()
        mid[len(mid) // 2] ^= 1 << 9
        add("bit 9 of a middle word", words=mid)
    add("a word appended", words=np.concatenate([words, np.array([0x9E3779B9], np.uint32)]))
    if len(m["low"]):
        low = base["low"].copy()
        low[len(m["low"]) // 2] ^= 1 << 3
        add("bit 3 of a low-bit word", low=low)
    if len(base["esc"]):
        add("last escape dropped", esc=base["esc"][:-1])
    add("a spare escape", esc=np.concatenate([base["esc"], np.array([0x1234], np.uint16)]))
    ks, counts = np.unique(bucket_of(unit, m["shift"]), return_counts=True)
    kb = int(ks[np.argmax(counts)])                         # the fullest bucket's nibble
    add("a nibble of sel", sel=m["sel"] ^ (0b0110 << (4 * kb)))
    add("state ^ 1", state=int(state) ^ 1)
    add("shift 9", shift=9)
    return out
