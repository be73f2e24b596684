"""The N-way interleaved rANS format as two serial loops in pure Python (a test helper).

A stream of n symbols is coded by N states ("ways"), all starting at L = 2^32, that share one
word sequence; symbol i meets state i % N with the reference's per-symbol arithmetic
(rans.pyx:58-66 encode, :86-109 decode).  States are Python ints; (start, freq) come from
oracle.cdf_freq and the decoder's probes from oracle.cdf, so nothing here restates the CDF.
"""
import math

import numpy as np
import rans_oracle as oracle

L = 1 << 32
U64 = (1 << 64) - 1
WORDS_LEFT = 32  # IDF_STREAM_WORDS_LEFT


def inputs(g, n):
    """(x, mean, scale) of n symbols: the generator of tests/test_gpu_rans.py's
    test_many_ragged_streams_match_oracle."""
    mean = (g.integers(-256, 257, n) / 256).astype(np.float32)
    scale = (np.exp(10 * g.random(n) - 5) / 256).astype(np.float32)
    x = (np.round((mean + scale * (10 * g.random(n) - 5)) * 256) / 256).astype(np.float32)
    return x, mean, scale


def c_round(v: float) -> float:
    """C round(): half away from zero (np.round and Python's round go to even)."""
    return math.copysign(math.floor(abs(v) + 0.5), v)


def encode(x, mean, scale, ways: int):
    """-> (final states [ways] as ints, words np.uint32 in push order, words pushed per way)."""
    start, freq = oracle.cdf_freq(x, mean, scale)  # rans.pyx:50-56
    S = [L] * ways
    words, pushed = [], [0] * ways
    for i in range(len(start)):
        j = i % ways
        f, c = int(freq[i]) & U64, int(start[i]) & U64  # vector<ull>.push_back(int)
        if S[j] >= (f << 40) & U64:
            words.append(S[j] & 0xffffffff)
            pushed[j] += 1
            S[j] >>= 32
        if f == 0:
            raise ZeroDivisionError("integer division or modulo by zero")
        S[j] = (((S[j] // f) << 24) + S[j] % f + c) & U64
    return S, np.asarray(words, dtype=np.uint32), pushed


def decode(states, words, n: int, mean, scale, ways: int):
    """-> (final states [ways], symbols np.float32 [n], unread words).  Raises what the
    reference raises: ZeroDivisionError (scale 0), OverflowError (a negative CDF), IndexError
    (the buffer ran out)."""
    S = [int(s) for s in states]
    pos = len(words)
    out = np.empty(n, np.float32)
    for i in range(n - 1, -1, -1):
        j = i % ways
        m, sc = float(mean[i]), float(scale[i])
        if S[j] < L:
            if pos <= 0:
                raise IndexError("rANS word buffer exhausted")
            pos -= 1
            S[j] = (S[j] << 32) | int(words[pos])
        mod = S[j] & 0xffffff
        lower = int(c_round(m * 256.0 - 1024.0))  # rans.pyx:91
        upper = lower + 0x7FF
        lower_f = float(np.float32(lower / 256.0))
        while lower <= upper:  # rans.pyx:96-104
            s = (lower + upper) >> 1
            c = oracle.cdf(s / 256.0, m, sc, lower_f)
            if c < 0:
                raise OverflowError("can't convert negative value to unsigned int")
            if c > mod:
                upper = s - 1
            else:
                lower = s + 1
        s = lower
        out[i] = np.float32(s / 256.0)
        c0 = oracle.cdf((s - 1) / 256.0, m, sc, lower_f)
        c1 = oracle.cdf(s / 256.0, m, sc, lower_f)
        if c0 < 0 or c1 - c0 < 0:
            raise OverflowError("can't convert negative value to unsigned int")
        S[j] = ((S[j] >> 24) * (c1 - c0) + mod - c0) & U64  # rans.pyx:108
    return S, out, pos


def encode_streams(off, x, mean, scale, ways: int):
    """Independent streams k = symbols [off[k], off[k + 1]), laid out as the device call's:
    (final states u64 [n * ways] stream-major, words u32 with stream k at off[k], counts)."""
    ns = len(off) - 1
    fs = np.empty(ns * ways, np.uint64)
    words = np.zeros(max(int(off[-1]), 1), np.uint32)
    nw = np.zeros(ns, np.int64)
    for k in range(ns):
        a, e = int(off[k]), int(off[k + 1])
        S, w, _ = encode(x[a:e], mean[a:e], scale[a:e], ways)
        fs[k * ways:(k + 1) * ways] = np.asarray(S, dtype=np.uint64)
        words[a:a + w.size] = w
        nw[k] = w.size
    return fs, words, nw


def decode_streams(off, woff, nw, words, mean, scale, states, ways: int):
    """-> (final states u64 [n * ways], symbols, status i32 [n], ok bool [n]): ok[k] is False
    where the reference raises (that stream's outputs are then not filled in); status is
    WORDS_LEFT where words stay unread, else 0."""
    ns = len(off) - 1
    fs = np.zeros(ns * ways, np.uint64)
    out = np.zeros(max(int(off[-1]), 1), np.float32)
    status = np.zeros(ns, np.int32)
    ok = np.zeros(ns, bool)
    for k in range(ns):
        a, e, w0 = int(off[k]), int(off[k + 1]), int(woff[k])
        try:
            S, o, left = decode(states[k * ways:(k + 1) * ways], words[w0:w0 + int(nw[k])],
                                e - a, mean[a:e], scale[a:e], ways)
        except (ZeroDivisionError, OverflowError, IndexError):
            continue
        fs[k * ways:(k + 1) * ways] = np.asarray(S, dtype=np.uint64)
        out[a:e] = o
        status[k] = WORDS_LEFT if left else 0
        ok[k] = True
    return fs, out[: int(off[-1])], status, ok
