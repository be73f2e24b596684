"""The colour mode of the predictive coder of escaped tiles, restated in numpy (a test helper).

The model is include/idf_codec.h's "colour entries": the planes of a rectangle uint8 [C][hin][win],
C >= 3, are transformed -- t[1] = v[1], t[p] = (v[p] - v[1] + 128) mod 256 for p in {0, 2}, planes
>= 3 unchanged -- and t is coded exactly as predict_ref codes v, but with two scale tables: sel from
the planes other than 0 and 2, sel2 from planes 0 and 2 together.  An entry is a colour entry iff
20 + 4 * nw_c < 16 + 4 * nw_p, and packed iff the smaller cost is below its bytes.  Built on
predict_ref and rans_oracle: nothing here restates the CDF.
"""
import numpy as np
import predict_ref as ref
import rans_oracle as oracle

L = ref.L
ENTRY_BYTES_COLOUR = 20  # sel 4, sel2 4, state 8, count 4


# ------------------------------------------------------------------ content
def correlated(H, W, seed, C=3):
    """Shared luminance, small chroma: uint8 [C, H, W].  A fourth plane (no part of the transform)
    follows the luminance too."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lum = (yy * 3 + xx * 2) // 2 + r.integers(0, 24, (H, W)).cumsum(1) % 64 + 30
    planes = [lum + 20 + r.integers(0, 3, (H, W)), lum + r.integers(0, 3, (H, W)),
              lum - 15 + r.integers(0, 3, (H, W))]
    if C > 3:
        planes.append(lum + 5 + r.integers(0, 3, (H, W)))
    return np.clip(planes[:C], 0, 255).astype(np.uint8)


def independent(H, W, seed, C=3):
    """Planes with ramps and noise of their own: uint8 [C, H, W]."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([((yy * (1 + c) + xx * (2 + c % 2)) // 4 + 40 * c + r.integers(0, 4, (H, W)))
                     % 256 for c in range(C)]).astype(np.uint8)


def noise(H, W, seed, C=3):
    return np.random.default_rng(seed).integers(0, 256, (C, H, W), dtype=np.uint8)


KINDS = (correlated, independent, noise)


def patchwork(H, W, seed, th, tw, first=0, C=3):
    """An image whose tile (ty, tx) of th x tw holds KINDS[(first + ty * ntx + tx) % 3]."""
    full = [g(H, W, seed, C) for g in KINDS]
    out = np.empty((C, H, W), dtype=np.uint8)
    ntx = -(-W // tw)
    for ty in range(-(-H // th)):
        for tx in range(ntx):
            k = (first + ty * ntx + tx) % 3
            ys, xs = slice(ty * th, (ty + 1) * th), slice(tx * tw, (tx + 1) * tw)
            out[:, ys, xs] = full[k][:, ys, xs]
    return out


def end_to_end_input(sizes, th=16, tw=16, seed=300):
    """The end-to-end set: image i of `sizes` is a patchwork that starts at kind i % 3."""
    return [patchwork(H, W, seed + i, th, tw, first=i) for i, (H, W) in enumerate(sizes)]


# ------------------------------------------------------------------ the model
def transform(planes):
    """v uint8 [C, h, w], C >= 3 -> t uint8 [C, h, w]"""
    v = np.asarray(planes).astype(np.int64)
    assert v.shape[0] >= 3
    t = v.copy()
    t[0] = (v[0] - v[1] + 128) % 256
    t[2] = (v[2] - v[1] + 128) % 256
    return t.astype(np.uint8)


def inverse(t):
    t = np.asarray(t).astype(np.int64)
    v = t.copy()
    v[0] = (t[0] + t[1] - 128) % 256
    v[2] = (t[2] + t[1] - 128) % 256
    return v.astype(np.uint8)


def second_table(C):
    """bool [C]: the planes whose symbols take their scale from sel2"""
    return np.array([p in (0, 2) for p in range(C)])


def choose_sels(planes):
    """-> (sel, sel2) of the colour candidate"""
    t = transform(planes)
    pred, k = ref.predict(t)
    ad = np.abs(t.astype(np.int64) - pred)
    g2 = second_table(t.shape[0])
    sels = []
    for grp in (~g2, g2):
        sel = 0
        for kb in range(8):
            m = k[grp] == kb
            sel |= ref.choose_j(int(ad[grp][m].sum()), int(m.sum())) << (4 * kb)
        sels.append(sel)
    return sels[0], sels[1]


def arrays(planes, sel=None, sel2=None):
    """The colour candidate's (x, mean, scale) float32 [n] in stream order."""
    t = transform(planes)
    if sel is None:
        sel, sel2 = choose_sels(planes)
    pred, k = ref.predict(t)
    g2 = second_table(t.shape[0])
    x = (t.astype(np.float32) / np.float32(256)).reshape(-1)
    mean = (pred.astype(np.float32) / np.float32(256)).reshape(-1)
    per_plane = np.where(g2, sel2, sel).astype(np.int64).reshape(-1, 1, 1)
    scale = ref.SCALE[((per_plane >> (4 * k)) & 15).reshape(-1)]
    return x[::-1].copy(), mean[::-1].copy(), scale[::-1].copy()


def encode(planes):
    """-> (sel, sel2, final state, words np.uint32 in push order) of the colour candidate"""
    sel, sel2 = choose_sels(planes)
    x, mean, scale = arrays(planes, sel, sel2)
    state, words = oracle.encode(L, x, mean, scale)
    return sel, sel2, state, words


def decode_t(sel, sel2, state, words, C, h, w, trace=None):
    """predict_ref.decode with a table per plane: -> (t uint8 [C, h, w], final state, status);
    trace as predict_ref.decode fills it."""
    out = np.zeros((C, h, w), dtype=np.uint8)
    S, pos, status = int(state), len(words), 0
    trace = {} if trace is None else trace
    trace.update(reached=0, low=0, high=0)
    g2 = second_table(C)
    for ch in range(C):
        table = sel2 if g2[ch] else sel
        for y in range(h):
            for x in range(w):
                if S < L:
                    if pos <= 0:
                        return out, S, status | ref.UNDERFLOW
                    pos -= 1
                    S = (S << 32) | int(words[pos])
                if y == 0 and x == 0:
                    a = b = c = 128
                elif y == 0:
                    a = b = c = int(out[ch, 0, x - 1])
                elif x == 0:
                    a = b = c = int(out[ch, y - 1, 0])
                else:
                    a, b, c = (int(out[ch, y, x - 1]), int(out[ch, y - 1, x]),
                               int(out[ch, y - 1, x - 1]))
                pred = (min(a, b) if c >= max(a, b) else max(a, b) if c <= min(a, b)
                        else a + b - c)
                k = 0 if (y == 0 or x == 0) else 1 + min(6, (abs(a - c) + abs(b - c) + 1)
                                                         .bit_length() - 1)
                mean, scale = pred / 256.0, float(ref.SCALE[(table >> (4 * k)) & 15])
                lower_f = (pred - 1024) / 256.0
                mod = S & 0xffffff
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
                S = ((S >> 24) * (c1 - c0) + mod - c0) & ref.U64
    return out, S, status | (ref.WORDS_LEFT if pos else 0)


def decode(sel, sel2, state, words, C, h, w, trace=None):
    """-> (bytes uint8 [C, h, w], final state, status)"""
    t, S, status = decode_t(sel, sel2, state, words, C, h, w, trace)
    return inverse(t), S, status


# ------------------------------------------------------------------ the choice
def choice(planes, colour=True):
    """-> (kind, bytes): what the entry is stored as -- "raw", "plain" or "colour" -- and what it
    costs in a file.  colour=False: the IDFP rule."""
    planes = np.asarray(planes)
    n = int(planes.size)
    plain = ref.ENTRY_BYTES + 4 * len(ref.encode(planes)[2])
    kind, cost = "plain", plain
    if colour and planes.shape[0] >= 3:
        col = ENTRY_BYTES_COLOUR + 4 * len(encode(planes)[3])
        if col < plain:
            kind, cost = "colour", col
    return (kind, cost) if cost < n else ("raw", n)
