// idf_predict.h -- the model of the predictive coder of escaped tiles (idfcodec/predict.py), usable
// from host and device code (gfx950).  Everything here is integer arithmetic or an exact f32
// literal; the literals are the file format of the IDFP container.
//
// The model sees one escaped entry's in-image rectangle uint8 [C][hin][win], each plane on its
// own.  The neighbours of the pixel at (y, x) are a = left, b = up, c = up-left, with
//   (0, 0): a = b = c = 128;   y = 0, x > 0: b = c = a;   x = 0, y > 0: a = c = b.
// pred is the MED (LOCO-I) predictor; the context bucket k is 0 on the first row and column,
// else 1 + min(6, floor(log2(|a - c| + |b - c| + 1))).  The byte v is coded with idf::rans_cdf
// at x = v / 256, mean = pred / 256, scale = kScale[nibble k of the entry's sel].
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IDF_PHD __host__ __device__ __forceinline__
#else
#define IDF_PHD static inline
#endif

namespace idf {

constexpr int kPredictBuckets = 8;
constexpr int kPredictScales = 16;

// SCALE[j], j = 0..15, e = j - 2: 2^(e/2 - 8) for even e, 0x1.6a09e6p+0f * 2^((e-1)/2 - 8) for
// odd e: 0.5 to ~90.5 bins.
IDF_PHD float predict_scale(int j) {
  constexpr float kScale[kPredictScales] = {
      0x1p-9f, 0x1.6a09e6p-9f, 0x1p-8f, 0x1.6a09e6p-8f, 0x1p-7f, 0x1.6a09e6p-7f,
      0x1p-6f, 0x1.6a09e6p-6f, 0x1p-5f, 0x1.6a09e6p-5f, 0x1p-4f, 0x1.6a09e6p-4f,
      0x1p-3f, 0x1.6a09e6p-3f, 0x1p-2f, 0x1.6a09e6p-2f};
  return kScale[j & (kPredictScales - 1)];
}

// T[j] = floor(1024 * 2 ln 2 * 2^((j - 2)/2 + 1/4) + 0.5), j = 0..14: bucket k takes the smallest
// j with 1024 * S <= n * T[j] (S = sum |v - pred|, n = its pixels), else 15.
IDF_PHD int64_t predict_threshold(int j) {
  constexpr int64_t kT[kPredictScales - 1] = {844,  1194,  1688,  2387,  3376,  4775,  6753, 9550,
                                              13505, 19099, 27011, 38199, 54021, 76397, 108042};
  return kT[j < 0 ? 0 : (j > 14 ? 14 : j)];
}

IDF_PHD int predict_med(int a, int b, int c) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return c >= hi ? lo : (c <= lo ? hi : a + b - c);
}

// the bucket of an interior pixel (y > 0 and x > 0); the first row and column are bucket 0
IDF_PHD int predict_bucket(int a, int b, int c) {
  const int ac = a - c, bc = b - c;
  const uint32_t d = (uint32_t)((ac < 0 ? -ac : ac) + (bc < 0 ? -bc : bc)) + 1u;  // 1..511
  const int lg = 31 - __builtin_clz(d);                                          // floor(log2)
  return 1 + (lg < 6 ? lg : 6);
}

// The neighbours' rule at the borders: `left` and `up` say whether the pixel has them; a, b, c
// come in as the stored neighbours (any value where absent) and leave as the model's.
IDF_PHD void predict_borders(bool left, bool up, int& a, int& b, int& c) {
  if (!left && !up) a = b = c = 128;
  else if (!up) b = c = a;
  else if (!left) a = c = b;
}

// The colour mode (C >= 3; IDFQ files): the model above applied to the transformed planes t,
//   t[1] = v[1],  t[p] = (v[p] - v[1] + 128) mod 256 for p in {0, 2},  t[p] = v[p] for p >= 3,
// with two scale tables: a symbol of plane 0 or 2 takes its scale from the entry's sel2, every
// other plane from its sel.
constexpr int kPredictColourMinC = 3;
constexpr int kPredictColourBias = 128;

// plane p's symbols read the second table
IDF_PHD bool predict_colour_second(int p) { return p == 0 || p == 2; }
// t[p] of a pixel of plane 0 or 2 from its byte v and the same pixel's byte g of plane 1
IDF_PHD int predict_colour_fwd(int v, int g) { return (v - g + kPredictColourBias) & 255; }
// and back: v from t[p] and t[1] (= g)
IDF_PHD int predict_colour_inv(int t, int g) { return (t + g - kPredictColourBias) & 255; }

// the j of one bucket from its (S, n), 64-bit
IDF_PHD int predict_choose(uint64_t S, uint64_t n) {
  if (n == 0) return 0;
  for (int j = 0; j < kPredictScales - 1; ++j)
    if (1024ull * S <= n * (uint64_t)predict_threshold(j)) return j;
  return kPredictScales - 1;
}

// What a symbol of frequency f (of 2^24) costs, in 1/256 bit: kPredictCostOne - predict_log2_q8(f).
// predict_log2_q8 is log2(f) in 1/256 bit by integers alone, so a sum of costs depends on neither
// the order of summation nor the machine: the leading bit gives the integer part, eight squarings
// of the Q31 mantissa m in [2^31, 2^32) the eight fraction bits (m^2 >= 2 names a 1 and halves).
// Every squaring drops the product's low 31 bits, so m only ever falls short of the exact power:
// by a relative 2^-31 a step, doubled by each later squaring, less than 2^-22 at the last bit.
// The result is therefore floor(256 log2(f (1 - e))) for some 0 <= e < 2^-22:
//   0 <= 256 log2(f) - predict_log2_q8(f) < 1 + 256 * 2^-22 / ln 2 < 1 + 2^-13,
// the floor itself except where 256 log2(f) lies within 2^-13 above an integer, and exact at the
// powers of two (their mantissa 2^31 squares to itself).  f = 0 gives 0.
constexpr int kPredictCostOne = 24 * 256;

IDF_PHD int predict_log2_q8(uint32_t f) {
  if (f == 0) return 0;
  const int e = 31 - __builtin_clz(f);
  uint64_t m = (uint64_t)f << (31 - e);
  int q = e;
  for (int i = 0; i < 8; ++i) {
    m = (m * m) >> 31;  // [2^31, 2^33)
    const int bit = (int)(m >> 32);
    m >>= bit;
    q = 2 * q + bit;
  }
  return q;
}

// The wavefront order (predict_ways = N > 1): the planes stacked into R = C * hin rows of win
// pixels, row rho = ch * hin + y; bands of N rows; P = max(win, N).  Pixel (rho, x) has step
// t = (rho / N) * P + rho % N + x and slot j = rho % N; its a, b and c lie in earlier steps and the
// pixels of one step have distinct slots.  The order q is ascending (t, j); pixel q is symbol
// n - 1 - q of the entry's stream.  N = 1 is the raster order.
IDF_PHD void predict_step_slot(int64_t rho, int64_t x, int64_t win, int ways, int64_t& t, int& j) {
  const int64_t P = win > ways ? win : (int64_t)ways;
  j = (int)(rho % ways);
  t = (rho / ways) * P + j + x;
}

// sum over k = 1..m of min(win, k)
IDF_PHD int64_t predict_tri(int64_t m, int64_t win) {
  if (m <= 0) return 0;
  return m <= win ? m * (m + 1) / 2 : win * (win + 1) / 2 + (m - win) * win;
}

// the rows of band `band` (0 for a band outside the entry)
IDF_PHD int64_t predict_band_rows(int64_t R, int ways, int64_t band) {
  if (band < 0) return 0;
  const int64_t left = R - band * ways;
  return left < 0 ? 0 : (left > ways ? (int64_t)ways : left);
}

// The rank q of pixel (rho, x) in closed form: the pixels of earlier steps -- every band before
// rho's neighbours whole, the three bands that can share a step with it by predict_tri: a band of
// nr rows holds tri(T) - tri(T - nr) pixels of local step j + x < T -- plus the active slots
// below j in its own step (an interval of slots per band).
IDF_PHD int64_t predict_rank(int64_t R, int64_t win, int ways, int64_t rho, int64_t x) {
  const int64_t P = win > ways ? win : (int64_t)ways;
  const int64_t band = rho / ways;
  int64_t t;
  int j;
  predict_step_slot(rho, x, win, ways, t, j);
  int64_t q = band > 1 ? (band - 1) * ways * win : 0;
  for (int64_t bb = band - 1; bb <= band + 1; ++bb) {
    const int64_t nr = predict_band_rows(R, ways, bb);
    if (nr == 0) continue;
    const int64_t T = t - bb * P;  // the band's local step
    q += predict_tri(T, win) - predict_tri(T - nr, win);
    const int64_t lo = T - win + 1 > 0 ? T - win + 1 : 0;
    int64_t hi = nr - 1 < T ? nr - 1 : T;
    hi = hi < j - 1 ? hi : (int64_t)j - 1;
    q += hi >= lo ? hi - lo + 1 : 0;
  }
  return q;
}

}  // namespace idf
