"""The 16-bit coder's interleaved states (ways = N), restated in numpy and pure Python (a test
helper).

The model is deep_ref's; only the order in which the samples meet the N states changes, and with
it the order of the escape list.  A unit is one plane, so the order is predict_ways_ref's at C = 1:
pixel (y, x) has step t = (y // N) * max(w, N) + y % N + x and slot y % N, the rank q is ascending
(t, slot) -- a sort, not the closed form of csrc/idf_predict.h -- and pixel q is symbol n - 1 - q
of a stream that rans_ways_ref codes with N states.  The low bits stay at bit r * s of pixel
r = y * w + x.  The CDF is the oracle's (through deep_ref and rans_ways_ref): nothing here
restates it.
"""
import struct

import numpy as np

import deep_ref as R
import predict_ways_ref as pw
import rans_oracle as oracle
import rans_ways_ref as wref
from predict_ref import SCALE

L, U64 = R.L, R.U64
UNDERFLOW, OUT_OF_WINDOW, WORDS_LEFT = R.UNDERFLOW, R.OUT_OF_WINDOW, R.WORDS_LEFT
WAYS = (8, 16, 32, 64)


def unit_overhead(N: int) -> int:
    """shift 1, sel 4, nwords 4, n_esc 4 and N states"""
    return 13 + 8 * N


def packed_bytes(n: int, s: int, nwords: int, n_esc: int, N: int) -> int:
    return unit_overhead(N) + 4 * nwords + 4 * ((n * s + 31) // 32) + 2 * n_esc


def perm_steps(h: int, w: int, N: int):
    """-> (perm, step): perm[q] the raster index of pixel q, step[q] its step, ascending"""
    t, j = pw.steps_slots(1, h, w, N)
    perm = np.lexsort((j.reshape(-1), t.reshape(-1)))
    return perm, t.reshape(-1)[perm]


def model(unit, N: int):
    """deep_ref.model with x, mean, scale in the wavefront stream order (pixel q at n - 1 - q)
    and the escapes in wavefront order."""
    unit = np.asarray(unit, dtype=np.uint16)
    m = dict(R.model(unit))
    q = pw.order(1, *unit.shape, N).reshape(-1)
    n = q.size
    for k in ("x", "mean", "scale"):
        raster = m[k][::-1]
        o = np.empty_like(raster)
        o[n - 1 - q] = raster
        m[k] = o
    perm, _ = perm_steps(*unit.shape, N)
    m["esc_raster"] = m["esc"]
    m["esc"] = unit.reshape(-1)[perm][m["esc_mask"].reshape(-1)[perm]].copy()
    return m


def encode(unit, N: int):
    """-> (model dict, the N final states as ints, words np.uint32 in push order)"""
    m = model(unit, N)
    S, words, _ = wref.encode(m["x"], m["mean"], m["scale"], N)
    return m, S, words


def unit_class(unit, N: int):
    """-> (class, model, states, words): deep_ref.unit_class with N states' overhead"""
    unit = np.asarray(unit, dtype=np.uint16)
    if int(unit.min()) == int(unit.max()):
        return R.CONSTANT, None, None, None
    m, S, words = encode(unit, N)
    if packed_bytes(unit.size, m["shift"], len(words), len(m["esc"]), N) < 2 * unit.size:
        return R.PACKED, m, S, words
    return R.RAW, m, S, words


def decode(s, sel, states, words, low, esc, h, w, N):
    """The decoder by step: -> (uint16 [h, w], final states, status).  The pixels of one step are
    taken together.  If more of the step's states are below L than words are left, or the step's
    decoded high parts name more escapes than are left, the step decodes nothing -- states, both
    cursors and flags stay as before it -- and the unit stops with UNDERFLOW; pixels never
    reached are 0.  WORDS_LEFT where words or escapes remain."""
    out = np.zeros((h, w), dtype=np.uint16)
    status = 0
    if s > 8:
        s, status = 8, OUT_OF_WINDOW
    n = h * w
    perm, step_of = perm_steps(h, w, N)
    S = [int(v) for v in states]
    pos, ei = len(words), 0
    big = sum(int(wd) << (32 * j) for j, wd in enumerate(low))
    k = 0
    while k < n:
        end = k
        while end < n and step_of[end] == step_of[k]:
            end += 1
        need = sum(1 for i in range(k, end) if S[(n - 1 - i) % N] < L)
        if need > pos:
            status |= UNDERFLOW
            break
        S2, pos2, st2, vals = list(S), pos, 0, []
        for i in range(k, end):
            r = int(perm[i])
            y, x = divmod(r, w)
            lane = (n - 1 - i) % N
            if S2[lane] < L:
                pos2 -= 1
                S2[lane] = (S2[lane] << 32) | int(words[pos2])
            if y == 0 and x == 0:
                a = b = c = 32768
            elif y == 0:
                a = b = c = int(out[0, x - 1])
            elif x == 0:
                a = b = c = int(out[y - 1, 0])
            else:
                a, b, c = int(out[y, x - 1]), int(out[y - 1, x]), int(out[y - 1, x - 1])
            pred = min(a, b) if c >= max(a, b) else max(a, b) if c <= min(a, b) else a + b - c
            kb = 0 if (y == 0 or x == 0) else 1 + min(6, (((abs(a - c) + abs(b - c)) >> s) + 1)
                                                      .bit_length() - 1)
            mean = np.float32(2 * pred + 1 - (1 << s)) / np.float32((1 << (s + 1)) * 256)
            scale = float(SCALE[(sel >> (4 * kb)) & 15])
            pq = pred >> s
            lower_f = (pq - 1024) / 256.0

            def cdf(q):
                return oracle.cdf(q / 256.0, float(mean), scale, lower_f)
            mod = S2[lane] & 0xffffff
            lo, hi = pq - R.ESCAPE, pq + R.ESCAPE + 1
            while lo < hi:
                mid = (lo + hi) >> 1
                if cdf(mid) > mod:
                    hi = mid
                else:
                    lo = mid + 1
            q = min(lo, pq + R.ESCAPE)
            c0, c1 = cdf(q - 1), cdf(q)
            if lo > pq + R.ESCAPE or c0 > mod:
                st2 |= OUT_OF_WINDOW
            S2[lane] = ((S2[lane] >> 24) * (c1 - c0) + mod - c0) & U64
            if abs(q - pq) == R.ESCAPE:
                vals.append((y, x, None))
            else:
                v = (q << s) + ((big >> (r * s)) & ((1 << s) - 1))
                if v < 0 or v > 65535:
                    v, st2 = min(max(v, 0), 65535), st2 | OUT_OF_WINDOW
                vals.append((y, x, v))
        if ei + sum(1 for v in vals if v[2] is None) > len(esc):
            status |= UNDERFLOW
            break
        S, pos, status = S2, pos2, status | st2
        for y, x, v in vals:
            if v is None:
                v = int(esc[ei])
                ei += 1
            out[y, x] = v
        k = end
    return out, S, status | (WORDS_LEFT if pos or ei < len(esc) else 0)


def write_file(images, th: int, tw: int, N: int) -> bytes:
    """The IDFD file of a list of uint16 [C, H, W] images at N states, by this module alone."""
    images = [np.asarray(i, dtype=np.uint16) for i in images]
    C = images[0].shape[0]
    units = R.units_of(images, th, tw)
    coded = [unit_class(u, N) for u in units]
    cls = np.array([c[0] for c in coded])
    buf = struct.pack("<4sHHIIII", R.MAGIC, 1, N, len(images), C, th, tw)
    buf += b"".join(struct.pack("<II", *i.shape[1:]) for i in images)
    const = cls == R.CONSTANT
    buf += np.packbits(const, bitorder="little").tobytes()
    buf += np.packbits(cls[~const] == R.PACKED, bitorder="little").tobytes()
    buf += np.array([u.flat[0] for u, k in zip(units, cls) if k == R.CONSTANT],
                    dtype="<u2").tobytes()
    raw = b"".join(u.astype("<u2").tobytes() for u, k in zip(units, cls) if k == R.RAW)
    buf += struct.pack("<Q", len(raw)) + raw
    pk = [c for c in coded if c[0] == R.PACKED]
    P = len(pk)
    sect = struct.pack("<I", P)
    sect += bytes(c[1]["shift"] for c in pk) + b"\0" * (-P % 4)
    sect += np.array([c[1]["sel"] for c in pk], dtype="<u4").tobytes()
    sect += b"".join(np.array(c[2], dtype="<u8").tobytes() for c in pk)
    sect += np.array([len(c[3]) for c in pk], dtype="<u4").tobytes()
    sect += np.array([len(c[1]["esc"]) for c in pk], dtype="<u4").tobytes()
    sect += b"".join(np.asarray(c[3], dtype="<u4").tobytes() for c in pk)
    sect += b"".join(c[1]["low"].astype("<u4").tobytes() for c in pk)
    esc = b"".join(c[1]["esc"].astype("<u2").tobytes() for c in pk)
    sect += esc + b"\0" * (-len(esc) % 4)
    return buf + struct.pack("<Q", len(sect)) + sect


# ------------------------------------------------------------------ the shared test units
SHAPES = ((1, 1), (7, 1), (1, 70), (19, 9), (9, 40), (33, 5), (24, 70), (40, 40), (64, 64))


def ramp_unit(h: int, w: int, noise: int, diagonals: bool, seed: int = 7):
    """20000 + 30 y - 11 x with noise of +-`noise`; diagonals: the anti-diagonals x + y == 10 and
    x + y == h + w - 12 set to 64000."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    u = 20000 + 30 * yy - 11 * xx + rng.integers(-noise, noise + 1, (h, w))
    if diagonals:
        u[(xx + yy == 10) | (xx + yy == h + w - 12)] = 64000
    return np.clip(u, 0, 65535).astype(np.uint16)


def noisy_unit(h: int, w: int):
    """the ramp with noise of +-40 and no diagonals (the seed gives shift 3 at 9 x 40)"""
    return ramp_unit(h, w, 40, False, seed=2)


def mixed_unit(h: int = 24, w: int = 70):
    """escapes and s > 0 in one unit: the ramp with noise +-40 and a sparse anti-diagonal of
    samples far off it"""
    u = ramp_unit(h, w, 40, False).astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    u[(xx + yy == 10) | ((xx + yy == h + w - 12) & (yy % 2 == 0))] = 64000
    return u.astype(np.uint16)


def damaged(m, S, words):
    """The damaged streams of one coded unit: [(name, dict of shift, sel, states, words, low,
    esc)]: one word removed, one escape removed, one extra word, one flipped word, shift 9."""
    base = {"shift": m["shift"], "sel": m["sel"], "states": list(S), "words": words,
            "low": m["low"], "esc": m["esc"]}
    out = []
    if len(words):
        out.append(("word removed", {**base, "words": words[1:]}))
        flipped = words.copy()
        flipped[len(words) // 2] ^= np.uint32(0x00010000)
        out.append(("word flipped", {**base, "words": flipped}))
    if len(m["esc"]):
        out.append(("escape removed", {**base, "esc": m["esc"][:-1]}))
    out.append(("extra word", {**base, "words": np.concatenate(
        [np.array([0x12345678], dtype=np.uint32), words])}))
    out.append(("shift 9", {**base, "shift": 9}))
    return out
