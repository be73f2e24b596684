// idf_deep.h -- the model of the 16-bit predictive coder (idfcodec/deep.py, container IDFD),
// usable from host and device code (gfx950).  Everything here is integer arithmetic or an exact
// f32 value; the literals are the file format.  predict_med, predict_scale, predict_choose and
// predict_threshold are idf_predict.h's, unchanged.
//
// A unit is one plane of one tile's in-image rectangle, uint16 [hin][win], n = hin * win, coded
// from its own samples alone.  The neighbours of the sample v at (y, x) are a = left, b = up,
// c = up-left, with
//   (0, 0): a = b = c = 32768;   y = 0, x > 0: b = c = a;   x = 0, y > 0: a = c = b.
// pred = MED(a, b, c), e = |v - pred|.
//
// The shift s of a unit, 0..8: the smallest s in 0..7 with 8 * #{e >= (16 << s)} <= n, else 8.
// A count, so it depends on no order of summation.  The high part q = v >> s is modelled, the low
// s bits are stored as they are.  With pq = pred >> s a sample is *escaped* iff |q - pq| >= 1000:
// its coded high part is q' = pq + 1000 sign(q - pq) and its 16 bits go to the unit's escape list
// in raster order; every other sample has q' = q, |q' - pq| <= 999, so |q' - pq| == 1000 marks an
// escape for the decoder.
//
// Bucket k = 0 on the first row and column, else 1 + min(6, floor(log2(((|a-c| + |b-c|) >> s)
// + 1))).  Nibble k of the unit's sel is predict_choose(S_k, n_k), S_k the sum of min(e >> s, 1000)
// and n_k the count of bucket k.
//
// The symbol: x = q' / 256, mean = (2 pred + 1 - 2^s) / (2^(s+1) * 256) -- the centre of pred's
// bin of width 2^s, in bins; pred / 256 at s = 0 -- and scale = SCALE[nibble k], under
// idf::rans_cdf and its 2048-bin window.  x and mean are exact in f32: their numerators are below
// 2^18 in magnitude and their denominators powers of two.  mean * 256 = (2 pred + 1 - 2^s) /
// 2^(s+1) is an integer at s = 0 and has an odd numerator over 2^(s+1) >= 4 for s >= 1, so it is
// never a half-integer and the window origin lower = round(mean * 256 - 1024) is the same on
// every machine.
//
// The window argument.  pq <= pred / 2^s < pq + 1, and mean * 256 = pred / 2^s + (1 - 2^s) /
// 2^(s+1) lies in (pred / 2^s - 1/2, pred / 2^s], so |pq - mean * 256| < 3/2 and
// |q' - mean * 256| < 1000 + 3/2 < 1002.  The window spans lower .. lower + 2047 with
// |lower + 1024 - mean * 256| <= 1/2: every q' and q' - 1 is at least 21 bins inside it, the CDF's
// linear term gives every bin a frequency >= 1, and a unit's encode status is always 0.
//
// Stream order: pixel r = y * win + x is symbol n - 1 - r; one way, initial state L.
// Low bits: v & (2^s - 1) of pixel r lies in bits [r s, (r + 1) s) of the unit's little-endian
// u32 run of ceil(n s / 32) words (idf_pack_bits' field layout); an escaped pixel's field is
// written and not read back; s = 0 has no run.
// Classes: constant iff min == max (two bytes stored); packed iff 21 + 4 nwords + 4 ceil(n s /
// 32) + 2 n_esc < 2 n (shift 1, sel 4, state 8, nwords 4, n_esc 4; a tie stores raw); else raw.
//
// Interleaved states (ways = N in {8, 16, 32, 64}; a file's header names its N, 0 for one way).
// The model above is untouched; only the order in which the samples meet N states changes.  A
// unit is one plane, so the order is idf_predict.h's wavefront at C = 1: row rho = y, R = hin,
// P = max(win, N); pixel (y, x) has step t = (y / N) * P + y % N + x and slot y % N, its a, b and
// c lie in earlier steps, and its rank q = predict_rank(hin, win, N, y, x) is ascending (step,
// slot).  Pixel q is symbol n - 1 - q of a stream coded by N states that all start at L
// (idf_rans_encode_streams_ways' format): pixel q meets state (n - 1 - q) % N.
// Escapes are listed in wavefront order (ascending q), not raster order: the escaped pixels of one
// step find theirs by a count over the step's earlier slots.
// Low bits stay where they are: pixel r = y * win + x keeps its field at bit r s, whatever N.
// A packed unit holds N states: 13 + 8 N + 4 nwords + 4 ceil(n s / 32) + 2 n_esc bytes, packed iff
// that is below 2 n.
// A damaged unit, by step: the pixels of one step are taken together.  If more of the step's
// states are below L than words are left, or the step's decoded high parts name more escapes than
// are left, the step decodes nothing -- states, word cursor, escape cursor and flags stay as they
// were before it -- and the unit stops with UNDERFLOW; the pixels never reached are 0.
#pragma once
#include <stdint.h>

#include "idf_predict.h"

namespace idf {

constexpr int kDeepOrigin = 32768;     // a = b = c at (0, 0)
constexpr int kDeepEscape = 1000;      // |q' - pq| of an escaped sample
constexpr int kDeepShiftMax = 8;
constexpr int kDeepShiftFloor = 16;    // s counts the samples with e >= (16 << s)
constexpr int kDeepUnitBytes = 21;     // a packed unit besides its words, low bits and escapes
constexpr int kDeepUnitFixed = 13;     // of which shift 1, sel 4, nwords 4, n_esc 4; 8 a state

IDF_PHD void deep_borders(bool left, bool up, int& a, int& b, int& c) {
  if (!left && !up) a = b = c = kDeepOrigin;
  else if (!up) b = c = a;
  else if (!left) a = c = b;
}

// the bucket of an interior sample (y > 0 and x > 0)
IDF_PHD int deep_bucket(int a, int b, int c, int s) {
  const int ac = a - c, bc = b - c;
  const uint32_t d = ((uint32_t)((ac < 0 ? -ac : ac) + (bc < 0 ? -bc : bc)) >> s) + 1u;
  const int lg = 31 - __builtin_clz(d);
  return 1 + (lg < 6 ? lg : 6);
}

// the shift from over[s] = #{e >= (16 << s)}, s = 0..7, and n
IDF_PHD int deep_shift(const uint64_t over[kDeepShiftMax], uint64_t n) {
  for (int s = 0; s < kDeepShiftMax; ++s)
    if (8ull * over[s] <= n) return s;
  return kDeepShiftMax;
}

// what sample v adds to its bucket's S: min(e >> s, 1000)
IDF_PHD uint32_t deep_cost(int v, int pred, int s) {
  const int d = v - pred;
  const uint32_t e = (uint32_t)(d < 0 ? -d : d) >> s;
  return e < (uint32_t)kDeepEscape ? e : (uint32_t)kDeepEscape;
}

// the coded high part q' of sample v; esc: the sample is escaped
IDF_PHD int deep_high(int v, int pred, int s, bool& esc) {
  const int q = v >> s, pq = pred >> s, d = q - pq;
  esc = d >= kDeepEscape || d <= -kDeepEscape;
  return esc ? pq + (d > 0 ? kDeepEscape : -kDeepEscape) : q;
}

// 2^-e, e in 0..126
IDF_PHD float deep_exp2_neg(int e) {
  const uint32_t u = (uint32_t)(127 - e) << 23;
#if defined(__HIPCC__)
  return __builtin_bit_cast(float, u);
#else
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
#endif
}

IDF_PHD float deep_x(int qc) { return (float)qc * 0.00390625f; }
IDF_PHD float deep_mean(int pred, int s) {
  return (float)(2 * pred + 1 - (1 << s)) * deep_exp2_neg(s + 9);
}

// the u32 words of a unit's low bits
IDF_PHD int64_t deep_low_words(int64_t n, int s) { return (n * s + 31) >> 5; }

// a packed unit besides its words, low bits and escapes, at `ways` states (1: kDeepUnitBytes)
IDF_PHD int64_t deep_unit_overhead(int ways) { return kDeepUnitFixed + 8 * (int64_t)ways; }

// the bytes a packed unit takes in a file
IDF_PHD int64_t deep_packed_bytes(int64_t n, int s, int64_t nwords, int64_t n_esc, int ways = 1) {
  return deep_unit_overhead(ways) + 4 * nwords + 4 * deep_low_words(n, s) + 2 * n_esc;
}

}  // namespace idf
