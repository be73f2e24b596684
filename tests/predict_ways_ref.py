"""The predictive coder's interleaved streams (predict_ways = N), restated in numpy and pure Python
(a test helper).

The model is predict_ref's (colour_ref's for colour entries); only the order in which the symbols
meet the N states changes.  Stack the planes of a rectangle uint8 [C][h][w] into R = C * h rows of
w pixels, row rho = ch * h + y, and let P = max(w, N): pixel (rho, x) has step t = (rho // N) * P
+ rho % N + x and slot j = rho % N; the wavefront order q is ascending (t, j) and pixel q is
symbol n - 1 - q of the stream, which rans_ways_ref codes with N states.  The order here is a sort,
not the closed form of csrc/idf_predict.h.
"""
import numpy as np

import colour_ref
import predict_ref as ref
import rans_oracle as oracle
import rans_ways_ref as wref

L = ref.L
WAYS = (8, 16, 32, 64)


def steps_slots(C, h, w, N):
    """-> (t, j), int64 [C * h, w] each"""
    rho = np.arange(C * h, dtype=np.int64)[:, None]
    x = np.arange(w, dtype=np.int64)[None, :]
    P = max(w, N)
    t = (rho // N) * P + rho % N + x
    return t, np.broadcast_to(rho % N, t.shape).copy()


def order(C, h, w, N):
    """int64 [C, h, w]: the rank q of every pixel, ascending (t, j)."""
    t, j = steps_slots(C, h, w, N)
    perm = np.lexsort((j.reshape(-1), t.reshape(-1)))     # perm[q]: the raster index of pixel q
    q = np.empty(perm.size, dtype=np.int64)
    q[perm] = np.arange(perm.size)
    return q.reshape(C, h, w)


def _reorder(arrs, shape, N):
    """predict_ref's stream arrays (pixel r at n - 1 - r) -> pixel q at n - 1 - q"""
    q = order(*shape, N).reshape(-1)
    n = q.size
    out = []
    for a in arrs:
        raster = a[::-1]
        o = np.empty_like(raster)
        o[n - 1 - q] = raster
        out.append(o)
    return tuple(out)


def arrays(planes, N, sel=None):
    """-> (x, mean, scale) float32 [n] of the plain stream in wavefront order"""
    planes = np.asarray(planes)
    return _reorder(ref.arrays(planes, sel), planes.shape, N)


def colour_arrays(planes, N, sel=None, sel2=None):
    planes = np.asarray(planes)
    return _reorder(colour_ref.arrays(planes, sel, sel2), planes.shape, N)


def encode(planes, N, colour=False):
    """-> (sel, sel2 or None, the N final states as ints, words np.uint32 in push order)"""
    planes = np.asarray(planes)
    if colour:
        sel, sel2 = colour_ref.choose_sels(planes)
        x, mean, scale = colour_arrays(planes, N, sel, sel2)
    else:
        sel, sel2 = ref.choose_sel(planes), None
        x, mean, scale = arrays(planes, N, sel)
    S, words, _ = wref.encode(x, mean, scale, N)
    return sel, sel2, S, words


def entry_cost(nwords, N, colour=False):
    """The bytes of a packed entry: sel 4, count 4, N states, its words; sel2 4 more."""
    return 8 + 8 * N + 4 * int(nwords) + (4 if colour else 0)


def choice(planes, N, colour=False):
    """-> (kind, bytes): "raw", "plain" or "colour" and the entry's cost in a file."""
    planes = np.asarray(planes)
    n = int(planes.size)
    kind, cost = "plain", entry_cost(len(encode(planes, N)[3]), N)
    if colour and planes.shape[0] >= 3:
        col = entry_cost(len(encode(planes, N, True)[3]), N, True)
        if col < cost:
            kind, cost = "colour", col
    return (kind, cost) if cost < n else ("raw", n)


def decode(sel, states, words, C, h, w, N, sel2=None, stop="serial", trace=None):
    """The serial causal decoder: pixels in wavefront order, pixel q on state (n - 1 - q) % N,
    every mean formed from the bytes decoded so far.  -> (bytes uint8 [C, h, w], final states,
    status) with predict_ref.decode's status rules; sel2: a colour entry (the bytes returned are
    then v, the transform undone).

    stop: where a missing word ends the entry.  "serial": at the pixel whose state needs it, the
    step's earlier pixels decoded.  "step", the device's rule: the pixels of one wavefront step are
    taken together; if more of their states are below L than words are left, none of them is
    decoded, the states stay as they were and the words that are left (too few) are reported as
    WORDS_LEFT beside UNDERFLOW.  Either way the pixels not reached are 0 (before the inverse
    transform of a colour entry, which runs over them too).
    trace: as predict_ref.decode fills it; "reached" counts pixels in wavefront order."""
    assert stop in ("serial", "step")
    n = C * h * w
    t, j = steps_slots(C, h, w, N)
    perm = np.lexsort((j.reshape(-1), t.reshape(-1)))       # perm[q]: the raster index of pixel q
    step_of = t.reshape(-1)[perm]                           # ascending
    out = np.zeros((C, h, w), dtype=np.uint8)
    S = [int(s) for s in states]
    pos, status = len(words), 0
    g2 = colour_ref.second_table(C)
    trace = {} if trace is None else trace
    trace.update(reached=0, low=0, high=0)
    k = 0
    while k < n and not status & ref.UNDERFLOW:
        end = k
        while end < n and step_of[end] == step_of[k]:
            end += 1
        if stop == "step":
            need = sum(1 for i in range(k, end) if S[(n - 1 - i) % N] < L)
            if need > pos:
                status |= ref.UNDERFLOW
                break
        for i in range(k, end):
            r = int(perm[i])
            ch, y, x = r // (h * w), (r // w) % h, r % w
            lane = (n - 1 - i) % N
            if S[lane] < L:
                if pos <= 0:
                    status |= ref.UNDERFLOW
                    break
                pos -= 1
                S[lane] = (S[lane] << 32) | int(words[pos])
            if y == 0 and x == 0:
                a = b = c = 128
            elif y == 0:
                a = b = c = int(out[ch, 0, x - 1])
            elif x == 0:
                a = b = c = int(out[ch, y - 1, 0])
            else:
                a, b, c = int(out[ch, y, x - 1]), int(out[ch, y - 1, x]), int(out[ch, y - 1, x - 1])
            pred = min(a, b) if c >= max(a, b) else max(a, b) if c <= min(a, b) else a + b - c
            kb = 0 if (y == 0 or x == 0) else 1 + min(6, (abs(a - c) + abs(b - c) + 1)
                                                      .bit_length() - 1)
            table = sel2 if (sel2 is not None and g2[ch]) else sel
            mean, scale = pred / 256.0, float(ref.SCALE[(table >> (4 * kb)) & 15])
            lower_f = (pred - 1024) / 256.0
            mod = S[lane] & 0xffffff
            lo, hi = 0, 256  # the smallest v in 0..255 with CDF(v) > mod, 256 if none
            while lo < hi:
                m = (lo + hi) >> 1
                if oracle.cdf(m / 256.0, mean, scale, lower_f) > mod:
                    hi = m
                else:
                    lo = m + 1
            v = min(lo, 255)
            c0 = oracle.cdf((v - 1) / 256.0, mean, scale, lower_f)
            c1 = oracle.cdf(v / 256.0, mean, scale, lower_f)
            if lo == 256 or c0 > mod:
                status |= ref.OUT_OF_WINDOW
                trace["high" if lo == 256 else "low"] += 1
            out[ch, y, x] = v
            trace["reached"] += 1
            S[lane] = ((S[lane] >> 24) * (c1 - c0) + mod - c0) & ref.U64
        k = end
    status |= ref.WORDS_LEFT if pos else 0
    if sel2 is not None:
        out = colour_ref.inverse(out)
    return out, S, status

