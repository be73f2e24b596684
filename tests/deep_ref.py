"""The 16-bit predictive coder, restated in numpy (a test helper).

The model is include/idf_codec.h's "the 16-bit predictive coder" (csrc/idf_deep.h): per unit
uint16 [h][w], neighbours a = left, b = up, c = up-left with 32768 at (0, 0), the MED prediction,
a shift s chosen by a count, the high part v >> s coded with an escape at |q - pq| >= 1000, the
low s bits stored.  Scales, thresholds and the choice of a scale are predict_ref's; the rANS
arithmetic is the oracle's (rans_oracle.encode / cdf): nothing here restates the CDF.
"""
import struct

import numpy as np
import rans_oracle as oracle
from predict_ref import SCALE, choose_j

L = 1 << 32
U64 = (1 << 64) - 1
UNDERFLOW, OUT_OF_WINDOW, WORDS_LEFT = 8, 16, 32  # IDF_STREAM_*
UNIT_BYTES = 21     # shift 1, sel 4, state 8, nwords 4, n_esc 4
ESCAPE = 1000
CONSTANT, PACKED, RAW = 0, 1, 2
MAGIC = b"IDFD"


def predict(unit):
    """unit: uint16 [h, w] -> (pred, delta = |a - c| + |b - c|), int64 [h, w] each."""
    v = np.asarray(unit).astype(np.int64)
    a, b, c = np.empty_like(v), np.empty_like(v), np.empty_like(v)
    a[:, 1:] = v[:, :-1]
    b[1:, :] = v[:-1, :]
    c[1:, 1:] = v[:-1, :-1]
    a[1:, 0] = b[1:, 0]
    c[1:, 0] = b[1:, 0]
    b[0, 1:] = a[0, 1:]
    c[0, 1:] = a[0, 1:]
    a[0, 0] = b[0, 0] = c[0, 0] = 32768
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    pred = np.where(c >= hi, lo, np.where(c <= lo, hi, a + b - c))
    return pred, np.abs(a - c) + np.abs(b - c)


def choose_shift(unit) -> int:
    """The smallest s in 0..7 with 8 * #{e >= (16 << s)} <= n, else 8."""
    v = np.asarray(unit).astype(np.int64)
    e = np.abs(v - predict(unit)[0])
    for s in range(8):
        if 8 * int((e >= (16 << s)).sum()) <= v.size:
            return s
    return 8


def buckets(unit, s: int):
    delta = predict(unit)[1]
    k = 1 + np.minimum(6, np.floor(np.log2((delta >> s) + 1)).astype(np.int64))
    k[0, :] = 0
    k[:, 0] = 0
    return k


def model(unit):
    """-> dict of everything the encoder derives from a unit: s, sel, q' (int64 [h, w]), the
    escape mask and list, the low-bit words, and x, mean, scale float32 [n] in stream order."""
    unit = np.asarray(unit, dtype=np.uint16)
    v = unit.astype(np.int64)
    n = v.size
    pred, _ = predict(unit)
    s = choose_shift(unit)
    k = buckets(unit, s)
    e = np.abs(v - pred)
    cost = np.minimum(e >> s, ESCAPE)
    sel = 0
    for kb in range(8):
        m = k == kb
        sel |= choose_j(int(cost[m].sum()), int(m.sum())) << (4 * kb)
    q, pq = v >> s, pred >> s
    esc = np.abs(q - pq) >= ESCAPE
    qc = np.where(esc, pq + ESCAPE * np.sign(q - pq), q)
    x = (qc.astype(np.float32) / np.float32(256)).reshape(-1)
    mean = ((2 * pred + 1 - (1 << s)).astype(np.float32)
            / np.float32((1 << (s + 1)) * 256)).reshape(-1)
    scale = SCALE[(sel >> (4 * k.reshape(-1))) & 15]
    return {"shift": s, "sel": sel, "q": qc, "esc_mask": esc,
            "esc": unit.reshape(-1)[esc.reshape(-1)].copy(), "low": pack_low(unit, s),
            "x": x[::-1].copy(), "mean": mean[::-1].copy(), "scale": scale[::-1].copy(),
            "min": int(v.min()), "max": int(v.max()), "n": n}


def pack_low(unit, s: int) -> np.ndarray:
    """uint32 [ceil(n s / 32)]: v & (2^s - 1) of pixel r in bits [r s, (r + 1) s)."""
    v = np.asarray(unit).astype(np.int64).reshape(-1)
    nl = (v.size * s + 31) // 32
    big = 0
    for r, val in enumerate(v):
        big |= (int(val) & ((1 << s) - 1)) << (r * s)
    return np.array([(big >> (32 * j)) & 0xffffffff for j in range(nl)], dtype=np.uint32)


def encode(unit):
    """-> (model dict, final state, words np.uint32 in push order); the encode status is 0."""
    m = model(unit)
    state, words = oracle.encode(L, m["x"], m["mean"], m["scale"])
    return m, state, words


def packed_bytes(n: int, s: int, nwords: int, n_esc: int) -> int:
    return UNIT_BYTES + 4 * nwords + 4 * ((n * s + 31) // 32) + 2 * n_esc


def unit_class(unit):
    """-> (class, model, state, words): constant iff min == max; packed iff its bytes are fewer
    than 2 n (a tie stores raw); else raw."""
    unit = np.asarray(unit, dtype=np.uint16)
    if int(unit.min()) == int(unit.max()):
        return CONSTANT, None, None, None
    m, state, words = encode(unit)
    if packed_bytes(unit.size, m["shift"], len(words), len(m["esc"])) < 2 * unit.size:
        return PACKED, m, state, words
    return RAW, m, state, words


def decode(s, sel, state, words, low, esc, h, w):
    """The serial decoder: -> (uint16 [h, w], final state, status).  Words or escapes left
    unread are flagged however the unit ends."""
    left = [len(words), 0]      # the words not yet popped, the escapes taken
    out, S, status = _decode(s, sel, state, words, low, esc, h, w, left)
    return out, S, status | (WORDS_LEFT if left[0] or left[1] < len(esc) else 0)


def _decode(s, sel, state, words, low, esc, h, w, left):
    out = np.zeros((h, w), dtype=np.uint16)
    status = 0
    if s > 8:
        s, status = 8, OUT_OF_WINDOW
    S, pos, ei, n = int(state), len(words), 0, h * w
    big = sum(int(wd) << (32 * j) for j, wd in enumerate(low))
    for r in range(n):
        y, x = divmod(r, w)
        if S < L:
            if pos <= 0:
                return out, S, status | UNDERFLOW
            pos -= 1
            left[0] = pos
            S = (S << 32) | int(words[pos])
        if y == 0 and x == 0:
            a = b = c = 32768
        elif y == 0:
            a = b = c = int(out[0, x - 1])
        elif x == 0:
            a = b = c = int(out[y - 1, 0])
        else:
            a, b, c = int(out[y, x - 1]), int(out[y - 1, x]), int(out[y - 1, x - 1])
        pred = min(a, b) if c >= max(a, b) else max(a, b) if c <= min(a, b) else a + b - c
        k = 0 if (y == 0 or x == 0) else 1 + min(6, (((abs(a - c) + abs(b - c)) >> s) + 1)
                                                 .bit_length() - 1)
        mean = np.float32(2 * pred + 1 - (1 << s)) / np.float32((1 << (s + 1)) * 256)
        scale = float(SCALE[(sel >> (4 * k)) & 15])
        pq = pred >> s
        lower_f = (pq - 1024) / 256.0

        def cdf(q):
            return oracle.cdf(q / 256.0, float(mean), scale, lower_f)
        mod = S & 0xffffff
        lo, hi = pq - ESCAPE, pq + ESCAPE + 1
        while lo < hi:
            m = (lo + hi) >> 1
            if cdf(m) > mod:
                hi = m
            else:
                lo = m + 1
        q = min(lo, pq + ESCAPE)
        c0, c1 = cdf(q - 1), cdf(q)
        if lo > pq + ESCAPE or c0 > mod:
            status |= OUT_OF_WINDOW
        S = ((S >> 24) * (c1 - c0) + mod - c0) & U64
        if abs(q - pq) == ESCAPE:
            if ei >= len(esc):
                return out, S, status | UNDERFLOW
            v = int(esc[ei])
            ei += 1
            left[1] = ei
        else:
            v = (q << s) + ((big >> (r * s)) & ((1 << s) - 1))
            if v < 0 or v > 65535:
                v, status = min(max(v, 0), 65535), status | OUT_OF_WINDOW
        out[y, x] = v
    return out, S, status


# ------------------------------------------------------------------ the container
def units_of(images, th: int, tw: int):
    """images: list of uint16 [C, H, W] -> their units in unit order (image, tile row, tile
    column; plane-minor)."""
    out = []
    for img in images:
        C, H, W = img.shape
        for y in range(0, H, th):
            for x in range(0, W, tw):
                out += [np.ascontiguousarray(img[p, y:y + th, x:x + tw]) for p in range(C)]
    return out


def write_file(images, th: int, tw: int) -> bytes:
    """The IDFD file of a list of uint16 [C, H, W] images, by this module alone."""
    images = [np.asarray(i, dtype=np.uint16) for i in images]
    C = images[0].shape[0]
    units = units_of(images, th, tw)
    coded = [unit_class(u) for u in units]
    cls = np.array([c[0] for c in coded])
    buf = struct.pack("<4sHHIIII", MAGIC, 1, 0, len(images), C, th, tw)
    buf += b"".join(struct.pack("<II", *i.shape[1:]) for i in images)
    const = cls == CONSTANT
    buf += np.packbits(const, bitorder="little").tobytes()
    buf += np.packbits(cls[~const] == PACKED, bitorder="little").tobytes()
    buf += np.array([u.flat[0] for u, k in zip(units, cls) if k == CONSTANT],
                    dtype="<u2").tobytes()
    raw = b"".join(u.astype("<u2").tobytes() for u, k in zip(units, cls) if k == RAW)
    buf += struct.pack("<Q", len(raw)) + raw
    pk = [c for c in coded if c[0] == PACKED]
    P = len(pk)
    sect = struct.pack("<I", P)
    sect += bytes(c[1]["shift"] for c in pk) + b"\0" * (-P % 4)
    sect += np.array([c[1]["sel"] for c in pk], dtype="<u4").tobytes()
    sect += np.array([c[2] for c in pk], dtype="<u8").tobytes()
    sect += np.array([len(c[3]) for c in pk], dtype="<u4").tobytes()
    sect += np.array([len(c[1]["esc"]) for c in pk], dtype="<u4").tobytes()
    sect += b"".join(np.asarray(c[3], dtype="<u4").tobytes() for c in pk)
    sect += b"".join(c[1]["low"].astype("<u4").tobytes() for c in pk)
    esc = b"".join(c[1]["esc"].astype("<u2").tobytes() for c in pk)
    sect += esc + b"\0" * (-len(esc) % 4)
    return buf + struct.pack("<Q", len(sect)) + sect


# ------------------------------------------------------------------ the shared test images
def hand_images():
    """The three images of the pinned file (tests/golden/idfd_hand.sha256), tile 8 x 8: grey
    13 x 11, 3-channel 9 x 20 and grey 8 x 8.  Between them: constant, packed and raw units,
    shifts 0, 3 and 8, an escape, one-sample-wide and one-sample-high units, partial tiles and a
    whole tile (test_gpu_deep asserts each)."""
    rng = np.random.default_rng(20260)
    yy, xx = np.mgrid[0:13, 0:11]
    a = (1000 + 7 * yy + 3 * xx).astype(np.int64)            # a smooth ramp: shift 0
    a[0:8, 8:11] = 4242                                       # a constant unit
    a[8:13, 0:8] += rng.integers(-40, 41, (5, 8))             # noise of ~6 bits: shift 3
    a[3, 4] = 60000                                           # an escape inside a packed unit
    b = np.empty((3, 9, 20), dtype=np.int64)
    yy, xx = np.mgrid[0:9, 0:20]
    b[0] = 30000 + 50 * yy - 20 * xx + rng.integers(-3, 4, (9, 20))
    b[1] = rng.integers(0, 65536, (9, 20))                    # uniform noise: raw
    b[2] = 500 + rng.integers(-2500, 2501, (9, 20))           # wide noise: shift 8
    b[2] = np.clip(b[2] + 20000, 0, 65535)
    c = (20000 + 16 * np.mgrid[0:8, 0:8][0] + rng.integers(-70, 71, (8, 8))).astype(np.int64)  # shift 3
    return [np.clip(a, 0, 65535).astype(np.uint16)[None], np.clip(b, 0, 65535).astype(np.uint16),
            c.astype(np.uint16)[None]]
