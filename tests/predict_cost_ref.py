"""The predictor's cost of an entry, restated in numpy (a test helper).

include/idf_codec.h "the predictor's cost of an entry" states it: per symbol 24 * 256 -
log2_q8(freq) in 1/256 bit, freq the encoder's own frequency of the symbol, summed.  The symbols are
predict_ref's (colour_ref's for the colour candidate) and the frequencies the oracle's (cdf_freq):
nothing here restates the model or the CDF.  log2_q8 restates csrc/idf_predict.h predict_log2_q8.
"""
import colour_ref
import numpy as np
import predict_ref as ref
import rans_oracle as oracle

COST_ONE = 24 * 256     # a symbol of frequency 1 of 2^24
COST_WORD = 32 * 256    # a word of the stream


def log2_q8(freq) -> np.ndarray:
    """int64 per value: the leading bit, then eight squarings of the Q31 mantissa, each product
    cut to 33 bits; 0 for 0."""
    f = np.asarray(freq, dtype=np.uint64).reshape(-1)
    e = np.zeros(f.shape, dtype=np.uint64)
    for s in (16, 8, 4, 2, 1):      # floor(log2 f) of f < 2^32, by halving
        hit = (f >> (e + np.uint64(s))) != 0
        e = np.where(hit, e + np.uint64(s), e)
    m = f << (np.uint64(31) - e)
    q = e.astype(np.int64)
    for _ in range(8):
        m = (m * m) >> np.uint64(31)            # m < 2^32: the product fits 64 bits
        bit = m >> np.uint64(32)
        m = m >> bit
        q = 2 * q + bit.astype(np.int64)
    return np.where(f == 0, 0, q)


def symbol_costs(x, mean, scale) -> np.ndarray:
    """int64 per symbol of (x, mean, scale): 24 * 256 - log2_q8 of the frequency it is coded with"""
    _, freq = oracle.cdf_freq(x, mean, scale)
    assert (freq >= 1).all()
    return COST_ONE - log2_q8(freq)


def cost_q8(planes, colour: bool = False) -> int:
    """The cost of a rectangle uint8 [C, h, w] in 1/256 bit: its plain candidate's, or its colour
    candidate's (C >= 3)."""
    arrays = colour_ref.arrays if colour else ref.arrays
    return int(symbol_costs(*arrays(np.asarray(planes))).sum())


def costs(planes, colour: bool = False):
    """-> [plain, colour or 0]: a row of idf_predict_cost_u8's output"""
    return [cost_q8(planes), cost_q8(planes, True) if colour else 0]
