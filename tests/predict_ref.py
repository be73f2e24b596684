"""The predictive coder of escaped tiles, restated in numpy (a test helper).

The model is include/idf_codec.h's "the predictive coder of escaped tiles": per plane of a
rectangle uint8 [C][hin][win], neighbours a = left, b = up, c = up-left, the MED prediction, 8
context buckets, 16 scale candidates and an integer rule that picks one per bucket.  The rANS
arithmetic is the oracle's (rans_oracle.encode / cdf): nothing here restates the CDF.
"""
import math

import numpy as np
import rans_oracle as oracle

L = 1 << 32
U64 = (1 << 64) - 1
UNDERFLOW, OUT_OF_WINDOW, WORDS_LEFT = 8, 16, 32  # IDF_STREAM_*
ENTRY_BYTES = 16  # sel 4, state 8, count 4

# SCALE[j], e = j - 2: 2^(e/2 - 8) for even e, 0x1.6a09e6p+0f * 2^((e-1)/2 - 8) for odd e
SCALE = np.array([np.float32(2.0 ** ((j - 2) // 2 - 8)) if (j - 2) % 2 == 0 else
                  np.float32(float.fromhex("0x1.6a09e6p+0")) * np.float32(2.0 ** ((j - 3) // 2 - 8))
                  for j in range(16)], dtype=np.float32)
# T[j] = floor(1024 * 2 ln 2 * 2^((j - 2)/2 + 1/4) + 0.5) in float64
T = np.array([math.floor(1024.0 * 2.0 * math.log(2.0) * 2.0 ** ((j - 2) / 2 + 0.25) + 0.5)
              for j in range(15)], dtype=np.int64)


def predict(planes):
    """planes: uint8 [C, h, w] -> (pred, bucket), int64 [C, h, w] each."""
    v = np.asarray(planes).astype(np.int64)
    C, h, w = v.shape
    a = np.empty_like(v)
    b = np.empty_like(v)
    c = np.empty_like(v)
    a[:, :, 1:] = v[:, :, :-1]
    b[:, 1:, :] = v[:, :-1, :]
    c[:, 1:, 1:] = v[:, :-1, :-1]
    # x = 0, y > 0: a = c = b;  y = 0, x > 0: b = c = a;  (0, 0): 128
    a[:, 1:, 0] = b[:, 1:, 0]
    c[:, 1:, 0] = b[:, 1:, 0]
    b[:, 0, 1:] = a[:, 0, 1:]
    c[:, 0, 1:] = a[:, 0, 1:]
    a[:, 0, 0] = b[:, 0, 0] = c[:, 0, 0] = 128
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    pred = np.where(c >= hi, lo, np.where(c <= lo, hi, a + b - c))
    delta = np.abs(a - c) + np.abs(b - c)
    k = 1 + np.minimum(6, np.floor(np.log2(delta + 1)).astype(np.int64))
    k[:, 0, :] = 0
    k[:, :, 0] = 0
    return pred, k


def choose_j(S: int, n: int) -> int:
    """One bucket's scale index from its sum of |v - pred| and its pixel count."""
    if n == 0:
        return 0
    for j in range(15):
        if 1024 * int(S) <= int(n) * int(T[j]):
            return j
    return 15


def choose_sel(planes) -> int:
    pred, k = predict(planes)
    ad = np.abs(np.asarray(planes).astype(np.int64) - pred)
    sel = 0
    for kb in range(8):
        m = k == kb
        sel |= choose_j(int(ad[m].sum()), int(m.sum())) << (4 * kb)
    return sel


def arrays(planes, sel=None):
    """-> (x, mean, scale) float32 [n] in stream order: pixel r at index n - 1 - r."""
    planes = np.asarray(planes)
    sel = choose_sel(planes) if sel is None else sel
    pred, k = predict(planes)
    x = (planes.astype(np.float32) / np.float32(256)).reshape(-1)
    mean = (pred.astype(np.float32) / np.float32(256)).reshape(-1)
    scale = SCALE[(sel >> (4 * k.reshape(-1))) & 15]
    return x[::-1].copy(), mean[::-1].copy(), scale[::-1].copy()


def encode(planes):
    """-> (sel, final state, words np.uint32 in push order)"""
    sel = choose_sel(planes)
    x, mean, scale = arrays(planes, sel)
    state, words = oracle.encode(L, x, mean, scale)
    return sel, state, words


def packed_cost(planes):
    """The bytes the entry takes in a file: 16 + 4 * nwords if that is fewer than its bytes,
    else its bytes."""
    n = int(np.asarray(planes).size)
    cost = ENTRY_BYTES + 4 * len(encode(planes)[2])
    return cost if cost < n else n


def decode(sel, state, words, C, h, w, trace=None):
    """The serial decoder: -> (bytes uint8 [C, h, w], final state, status).  A byte the slot does
    not name (a damaged stream) is clamped and flagged; running out of words stops the entry.
    trace: a dict that receives "reached" (the pixels decoded, in raster order), "low" and "high"
    (the slots clamped to 0, below CDF(-1), and to 255, at or above CDF(255))."""
    out = np.zeros((C, h, w), dtype=np.uint8)
    S, pos, status = int(state), len(words), 0
    trace = {} if trace is None else trace
    trace.update(reached=0, low=0, high=0)
    for ch in range(C):
        for y in range(h):
            for x in range(w):
                if S < L:
                    if pos <= 0:
                        return out, S, status | UNDERFLOW
                    pos -= 1
                    S = (S << 32) | int(words[pos])
                if y == 0 and x == 0:
                    a = b = c = 128
                elif y == 0:
                    a = b = c = int(out[ch, 0, x - 1])
                elif x == 0:
                    a = b = c = int(out[ch, y - 1, 0])
                else:
                    a, b, c = int(out[ch, y, x - 1]), int(out[ch, y - 1, x]), int(out[ch, y - 1,
                                                                                      x - 1])
                pred = min(a, b) if c >= max(a, b) else max(a, b) if c <= min(a, b) else a + b - c
                k = 0 if (y == 0 or x == 0) else 1 + min(6, (abs(a - c) + abs(b - c) + 1)
                                                         .bit_length() - 1)
                mean, scale = pred / 256.0, float(SCALE[(sel >> (4 * k)) & 15])
                lower_f = (pred - 1024) / 256.0

                def cdf(q):
                    return oracle.cdf(q / 256.0, mean, scale, lower_f)
                mod = S & 0xffffff
                lo, hi = 0, 256  # the smallest v in 0..255 with CDF(v) > mod, 256 if none
                while lo < hi:
                    m = (lo + hi) >> 1
                    if cdf(m) > mod:
                        hi = m
                    else:
                        lo = m + 1
                v = min(lo, 255)
                c0, c1 = cdf(v - 1), cdf(v)
                if lo == 256 or c0 > mod:
                    status |= OUT_OF_WINDOW
                    trace["high" if lo == 256 else "low"] += 1
                out[ch, y, x] = v
                trace["reached"] += 1
                S = ((S >> 24) * (c1 - c0) + mod - c0) & U64
    return out, S, status | (WORDS_LEFT if pos else 0)
