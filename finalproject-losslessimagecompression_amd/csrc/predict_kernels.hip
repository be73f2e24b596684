// predict_kernels.hip -- the predictive rANS coder of escaped tiles (idfcodec/predict.py): the
// bytes of a tile the flow does not code, coded with a causal MED predictor and a per-context
// logistic scale (csrc/idf_predict.h has the model) through the same CDF, window and state
// arithmetic as the flow's symbols (idf_cdf.h, rans.pyx:37-110).
//
// Kernels
//   predict_prep   : one block per entry, element-wise.  Pass 1 reads the entry's in-image bytes
//                    where the tile table says they lie (as tile_gather_raw_u8 does), sums |v - pred|
//                    and the pixel count of each of the 8 context buckets in LDS and chooses the
//                    entry's sel; pass 2 writes x = v/256, mean = pred/256 and scale in stream order
//                    (pixel r of n at index n - 1 - r: rANS pops the last symbol first and the
//                    decoder must see pixels in raster order).  idf_rans_encode_streams and
//                    idf_gather_words do the rest unchanged.
//   predict_decode : ONE WAVE per entry, the serial chain.  Per symbol: renormalise (the state and
//                    the words stay wave-uniform), form a, b, c from the bytes already decoded (the
//                    row above in LDS, never this kernel's own global stores), then find the byte v
//                    with CDF(v - 1) <= slot < CDF(v) by exact CDF probes (cdf_bin, bit-identical
//                    to rans_cdf): the inverse logistic of the slot guesses a bin and 64 lanes
//                    probe the 64 bins around it in ONE round; where that window misses, two
//                    rounds: lane l probes bin 4 l + 3, one ballot names the block of four, five
//                    lanes probe that block and its left neighbour.  Only the 256 byte bins of
//                    the 2048-bin window can occur.
//   predict_prep2  : predict_prep for both candidates of an entry of C >= 3 planes in one launch:
//                    the plain one and the colour one (idf_predict.h: planes 0 and 2 minus plane
//                    1, two scale tables), whose transformed neighbours are formed from two
//                    source bytes each.  One encoder launch then codes twice as many streams.
//   predict_cost   : one block per entry, the preps' pass 1 (shared device functions) and then the
//                    cost the predictor would have on the entry, sum of -log2(freq / 2^24) in
//                    integers (idf_predict.h predict_log2_q8) -- no symbol is written or coded.
//   predict_decode2: predict_decode's body with a per-entry colour flag: a colour entry decodes
//                    the transformed planes, its second table on lanes 8..15.
//   predict_colour_inverse : element-wise, the colour entries' bytes from t back to v in place.
//   predict_prep<true>, predict_prep2<true> : the preps with the symbols in the wavefront order
//                    of N interleaved states (idf_predict.h predict_rank, closed form per pixel).
//   predict_decode_ways<N> : ONE WAVE per entry, N lanes owning one state each, a wavefront step
//                    of up to N pixels at once; the entry lives in LDS (described at the kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "idf_cdf.h"
#include "idf_cdf_fast.h"
#include "idf_codec_internal.h"
#include "idf_predict.h"

#pragma clang fp contract(off)

namespace idf {

constexpr int PRED_FIELDS = 5;       // addr, H, W, y0, x0 (the tile table's rows)
constexpr int PRED_CMAX = 4;
constexpr int PRED_TW_MAX = 32768;   // the decoder keeps one row of the plane in LDS

// the model's (pred, bucket) of pixel (y, x) of a plane p of rows of `pitch` bytes
__device__ __forceinline__ void predict_at(const uint8_t* p, int64_t pitch, int64_t y, int64_t x,
                                           int& pred, int& k) {
  const bool left = x > 0, up = y > 0;
  int a = left ? (int)p[y * pitch + x - 1] : 0;
  int b = up ? (int)p[(y - 1) * pitch + x] : 0;
  int c = left && up ? (int)p[(y - 1) * pitch + x - 1] : 0;
  predict_borders(left, up, a, b, c);
  pred = predict_med(a, b, c);
  k = left && up ? predict_bucket(a, b, c) : 0;
}

// The entry a block works on: where its planes lie (tile table row t: addr, H, W, y0, x0) and its
// in-image rectangle hin x win; npl = hin * win, n = C * npl.  A tile outside the image is empty.
struct PredEntry {
  const uint8_t* src;
  int64_t H, W, y0, x0, hin, win, npl, n;
  int C;
};

__device__ __forceinline__ PredEntry predict_entry(const int64_t* __restrict__ table, int64_t t,
                                                   int C, int th, int tw) {
  const int64_t* row = table + t * PRED_FIELDS;
  PredEntry e;
  e.src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(row[0]));
  e.H = row[1], e.W = row[2], e.y0 = row[3], e.x0 = row[4];
  const bool inside = e.y0 >= 0 && e.x0 >= 0 && e.y0 < e.H && e.x0 < e.W;
  e.hin = inside ? (e.H - e.y0 < th ? e.H - e.y0 : th) : 0;
  e.win = inside ? (e.W - e.x0 < tw ? e.W - e.x0 : tw) : 0;
  e.npl = e.hin * e.win;
  e.n = (int64_t)C * e.npl;
  e.C = C;
  return e;
}

// Pass 1 of the plain coding, by the whole block: |v - pred| and the pixel count of each bucket
// summed in acc (LDS: S[8], n[8]) and the entry's sel chosen into *sel_s.  Every thread of the
// block calls it; *sel_s is readable when it returns.
__device__ __forceinline__ void predict_pass1(const PredEntry& e, unsigned long long* acc,
                                              uint32_t* sel_s) {
  const int64_t H = e.H, W = e.W, y0 = e.y0, x0 = e.x0, win = e.win, npl = e.npl, n = e.n;
  if (threadIdx.x < 2 * kPredictBuckets) acc[threadIdx.x] = 0;
  __syncthreads();
  uint32_t S[kPredictBuckets], cnt[kPredictBuckets];  // a thread sees < 2^24 pixels of <= 255 each
#pragma unroll
  for (int k = 0; k < kPredictBuckets; ++k) S[k] = cnt[k] = 0;
  for (int64_t r = threadIdx.x; r < n; r += blockDim.x) {
    const int64_t c = r / npl, q = r - c * npl, y = q / win, x = q - y * win;
    const uint8_t* p = e.src + (c * H + y0) * W + x0;
    int pred, kb;
    predict_at(p, W, y, x, pred, kb);
    const int d = (int)p[y * W + x] - pred;
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
#pragma unroll
    for (int k = 0; k < kPredictBuckets; ++k) {
      S[k] += k == kb ? ad : 0u;
      cnt[k] += k == kb ? 1u : 0u;
    }
  }
#pragma unroll
  for (int k = 0; k < kPredictBuckets; ++k) {
    if (cnt[k]) {
      atomicAdd(&acc[k], (unsigned long long)S[k]);
      atomicAdd(&acc[kPredictBuckets + k], (unsigned long long)cnt[k]);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int k = 0; k < kPredictBuckets; ++k)
      s |= (uint32_t)predict_choose(acc[k], acc[kPredictBuckets + k]) << (4 * k);
    *sel_s = s;
  }
  __syncthreads();
}

// WAYS: the symbols in the wavefront order of `ways` states (idf_predict.h: pixel q at index
// n - 1 - q, q = predict_rank in closed form); else the raster order, `ways` unread.
template <bool WAYS>
__global__ void __launch_bounds__(256)
predict_prep_kernel(int C, int th, int tw, const int64_t* __restrict__ table,
                    const int64_t* __restrict__ sym_off, uint32_t* __restrict__ sel_out,
                    float* __restrict__ xo, float* __restrict__ mo, float* __restrict__ so,
                    int ways) {
  __shared__ unsigned long long acc[2 * kPredictBuckets];  // S[8], n[8]
  __shared__ uint32_t sel_s;
  const int64_t t = blockIdx.x;
  const PredEntry e = predict_entry(table, t, C, th, tw);
  const uint8_t* src = e.src;
  const int64_t H = e.H, W = e.W, y0 = e.y0, x0 = e.x0, hin = e.hin, win = e.win;
  const int64_t npl = e.npl, n = e.n;
  const int64_t o = sym_off[t];
  if (sym_off[t + 1] - o != n) {  // the caller's offsets do not fit this entry: nothing is written
    if (threadIdx.x == 0) sel_out[t] = 0;
    return;
  }
  predict_pass1(e, acc, &sel_s);
  if (threadIdx.x == 0) sel_out[t] = sel_s;
  const uint32_t sel = sel_s;
  for (int64_t r = threadIdx.x; r < n; r += blockDim.x) {
    const int64_t c = r / npl, q = r - c * npl, y = q / win, x = q - y * win;
    const uint8_t* p = src + (c * H + y0) * W + x0;
    int pred, kb;
    predict_at(p, W, y, x, pred, kb);
    const int64_t i = o + n - 1 - (WAYS ? predict_rank(C * hin, win, ways, c * hin + y, x) : r);
    xo[i] = (float)p[y * W + x] * 0.00390625f;
    mo[i] = (float)pred * 0.00390625f;
    so[i] = predict_scale((int)(sel >> (4 * kb)) & 15);
  }
}

// predict_at on the transformed plane t[c] of a colour entry: p is plane c of the source and g
// plane 1 at the same origin; xf says whether c is 0 or 2.  Two source bytes a neighbour, t is
// never stored.
__device__ __forceinline__ int colour_byte(const uint8_t* p, const uint8_t* g, bool xf,
                                           int64_t i) {
  return xf ? predict_colour_fwd((int)p[i], (int)g[i]) : (int)p[i];
}

__device__ __forceinline__ void predict_at_colour(const uint8_t* p, const uint8_t* g, bool xf,
                                                  int64_t pitch, int64_t y, int64_t x, int& pred,
                                                  int& k) {
  const bool left = x > 0, up = y > 0;
  int a = left ? colour_byte(p, g, xf, y * pitch + x - 1) : 0;
  int b = up ? colour_byte(p, g, xf, (y - 1) * pitch + x) : 0;
  int c = left && up ? colour_byte(p, g, xf, (y - 1) * pitch + x - 1) : 0;
  predict_borders(left, up, a, b, c);
  pred = predict_med(a, b, c);
  k = left && up ? predict_bucket(a, b, c) : 0;
}

// Pass 1 of both candidates of an entry of C >= 3 planes, by the whole block.  Three plane groups
// are summed in acc (LDS, per group: S[8], n[8]): 0, every plane as it is (the plain sel); 1, the
// transformed planes other than 0 and 2 (the colour sel); 2, the transformed planes 0 and 2
// (sel2).  sel_s[0..2] = (plain sel, colour sel, sel2), readable when it returns.
__device__ __forceinline__ void predict_pass1_colour(const PredEntry& e,
                                                     unsigned long long (*acc)[2 * kPredictBuckets],
                                                     uint32_t* sel_s) {
  const int64_t H = e.H, W = e.W, y0 = e.y0, x0 = e.x0, win = e.win, npl = e.npl;
  if (threadIdx.x < 3 * 2 * kPredictBuckets) (&acc[0][0])[threadIdx.x] = 0;
  __syncthreads();
  const uint8_t* green = e.src + (H + y0) * W + x0;  // plane 1 at the entry's origin
  for (int c = 0; c < e.C; ++c) {
    const uint8_t* p = e.src + (c * H + y0) * W + x0;
    const bool xf = predict_colour_second(c);
    // [0]: the plain candidate; [1]: the colour candidate; < 2^24 pixels of <= 255 a thread
    uint32_t S[2][kPredictBuckets], cnt[2][kPredictBuckets];
#pragma unroll
    for (int k = 0; k < kPredictBuckets; ++k) S[0][k] = S[1][k] = cnt[0][k] = cnt[1][k] = 0;
    for (int64_t q = threadIdx.x; q < npl; q += blockDim.x) {
      const int64_t y = q / win, x = q - y * win;
      int pred, kb, predc, kbc;
      predict_at(p, W, y, x, pred, kb);
      predict_at_colour(p, green, xf, W, y, x, predc, kbc);
      const int d = (int)p[y * W + x] - pred;
      const int dc = colour_byte(p, green, xf, y * W + x) - predc;
      const uint32_t ad = (uint32_t)(d < 0 ? -d : d), adc = (uint32_t)(dc < 0 ? -dc : dc);
#pragma unroll
      for (int k = 0; k < kPredictBuckets; ++k) {
        S[0][k] += k == kb ? ad : 0u;
        cnt[0][k] += k == kb ? 1u : 0u;
        S[1][k] += k == kbc ? adc : 0u;
        cnt[1][k] += k == kbc ? 1u : 0u;
      }
    }
    const int grp = xf ? 2 : 1;
#pragma unroll
    for (int k = 0; k < kPredictBuckets; ++k) {
      if (cnt[0][k]) {
        atomicAdd(&acc[0][k], (unsigned long long)S[0][k]);
        atomicAdd(&acc[0][kPredictBuckets + k], (unsigned long long)cnt[0][k]);
      }
      if (cnt[1][k]) {
        atomicAdd(&acc[grp][k], (unsigned long long)S[1][k]);
        atomicAdd(&acc[grp][kPredictBuckets + k], (unsigned long long)cnt[1][k]);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int g = threadIdx.x;
    uint32_t s = 0;
    for (int k = 0; k < kPredictBuckets; ++k)
      s |= (uint32_t)predict_choose(acc[g][k], acc[g][kPredictBuckets + k]) << (4 * k);
    sel_s[g] = s;
  }
  __syncthreads();
}

// Both candidates of an entry in one launch (C >= 3): stream 2 t is entry t's plain candidate,
// exactly predict_prep_kernel's symbols, stream 2 t + 1 its colour candidate.  Pass 1 is
// predict_pass1_colour's three plane groups; sel_out[3 t ..] = (plain sel, colour sel, sel2).
template <bool WAYS>
__global__ void __launch_bounds__(256)
predict_prep2_kernel(int C, int th, int tw, const int64_t* __restrict__ table,
                     const int64_t* __restrict__ sym_off, uint32_t* __restrict__ sel_out,
                     float* __restrict__ xo, float* __restrict__ mo, float* __restrict__ so,
                     int ways) {
  __shared__ unsigned long long acc[3][2 * kPredictBuckets];  // per group: S[8], n[8]
  __shared__ uint32_t sel_s[3];
  const int64_t t = blockIdx.x;
  const PredEntry e = predict_entry(table, t, C, th, tw);
  const uint8_t* src = e.src;
  const int64_t H = e.H, W = e.W, y0 = e.y0, x0 = e.x0, hin = e.hin, win = e.win;
  const int64_t npl = e.npl, n = e.n;
  const int64_t o0 = sym_off[2 * t], o1 = sym_off[2 * t + 1];
  if (o1 - o0 != n || sym_off[2 * t + 2] - o1 != n) {  // the offsets do not fit: nothing is written
    if (threadIdx.x < 3) sel_out[3 * t + threadIdx.x] = 0;
    return;
  }
  predict_pass1_colour(e, acc, sel_s);
  if (threadIdx.x < 3) sel_out[3 * t + threadIdx.x] = sel_s[threadIdx.x];
  const uint8_t* green = src + (H + y0) * W + x0;  // plane 1 at the entry's origin
  const uint32_t sel_p = sel_s[0], sel_c = sel_s[1], sel_c2 = sel_s[2];
  for (int64_t r = threadIdx.x; r < n; r += blockDim.x) {
    const int64_t c = r / npl, q = r - c * npl, y = q / win, x = q - y * win;
    const uint8_t* p = src + (c * H + y0) * W + x0;
    const bool xf = predict_colour_second((int)c);
    int pred, kb, predc, kbc;
    predict_at(p, W, y, x, pred, kb);
    predict_at_colour(p, green, xf, W, y, x, predc, kbc);
    const int64_t rk = WAYS ? predict_rank(C * hin, win, ways, c * hin + y, x) : r;
    const int64_t i = o0 + n - 1 - rk, ic = o1 + n - 1 - rk;
    xo[i] = (float)p[y * W + x] * 0.00390625f;
    mo[i] = (float)pred * 0.00390625f;
    so[i] = predict_scale((int)(sel_p >> (4 * kb)) & 15);
    xo[ic] = (float)colour_byte(p, green, xf, y * W + x) * 0.00390625f;
    mo[ic] = (float)predc * 0.00390625f;
    so[ic] = predict_scale((int)((xf ? sel_c2 : sel_c) >> (4 * kbc)) & 15);
  }
}

// The frequency the encoder codes byte v with: rans_start_freq (the encoder's own pass 1) at the
// x, mean and scale the preps write for it.
__device__ __forceinline__ int predict_freq(int v, int pred, uint32_t sel, int kb,
                                            const uint64_t* tab) {
  const float x = (float)v * 0.00390625f, mean = (float)pred * 0.00390625f;
  const float scale = predict_scale((int)(sel >> (4 * kb)) & 15);
  int start, freq;
  rans_start_freq(x, mean, scale, rans_lower_int(mean), tab, start, freq);
  return freq;
}

// What the predictor would cost on an entry, without coding it: one block per entry as the preps,
// their pass 1 (the same functions), then per symbol kPredictCostOne - predict_log2_q8(freq) in
// 1/256 bit, summed in integers -- per thread, per wave by shuffles, per block through LDS -- so
// the sum depends on no order.  cost_out[2 t] is the plain candidate's, cost_out[2 t + 1] the
// colour candidate's (COLOUR, C >= 3) or 0.  Two exact CDFs in f64 a symbol and candidate bound
// it, not its loads.
template <bool COLOUR>
__global__ void __launch_bounds__(256)
predict_cost_kernel(int C, int th, int tw, const int64_t* __restrict__ table,
                    int64_t* __restrict__ cost_out) {
  __shared__ unsigned long long acc[COLOUR ? 3 : 1][2 * kPredictBuckets];
  __shared__ uint32_t sel_s[3];
  __shared__ uint64_t tab[32];
  __shared__ unsigned long long part[2][4];  // per candidate, per wave
  const int64_t t = blockIdx.x;
  const PredEntry e = predict_entry(table, t, C, th, tw);
  const int64_t H = e.H, W = e.W, y0 = e.y0, x0 = e.x0, win = e.win, npl = e.npl, n = e.n;
  if (threadIdx.x < 32) tab[threadIdx.x] = kExp2fTab[threadIdx.x];  // pass 1's barriers cover it
  if constexpr (COLOUR) predict_pass1_colour(e, acc, sel_s);
  else predict_pass1(e, acc[0], sel_s);
  const uint32_t sel_p = sel_s[0];
  const uint32_t sel_c = COLOUR ? sel_s[1] : 0u, sel_c2 = COLOUR ? sel_s[2] : 0u;
  const uint8_t* green = e.src + (H + y0) * W + x0;  // plane 1 at the entry's origin (COLOUR)
  unsigned long long sp = 0, sc = 0;
  for (int64_t r = threadIdx.x; r < n; r += blockDim.x) {
    const int64_t c = r / npl, q = r - c * npl, y = q / win, x = q - y * win;
    const uint8_t* p = e.src + (c * H + y0) * W + x0;
    int pred, kb;
    predict_at(p, W, y, x, pred, kb);
    const int f = predict_freq((int)p[y * W + x], pred, sel_p, kb, tab);
    sp += (unsigned long long)(kPredictCostOne - predict_log2_q8((uint32_t)(f < 1 ? 1 : f)));
    if constexpr (COLOUR) {
      const bool xf = predict_colour_second((int)c);
      int predc, kbc;
      predict_at_colour(p, green, xf, W, y, x, predc, kbc);
      const int fc = predict_freq(colour_byte(p, green, xf, y * W + x), predc,
                                  xf ? sel_c2 : sel_c, kbc, tab);
      sc += (unsigned long long)(kPredictCostOne - predict_log2_q8((uint32_t)(fc < 1 ? 1 : fc)));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sp += __shfl_down(sp, off);
    if constexpr (COLOUR) sc += __shfl_down(sc, off);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = sp;
    part[1][threadIdx.x >> 6] = sc;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    cost_out[2 * t + threadIdx.x] = (int64_t)(part[threadIdx.x][0] + part[threadIdx.x][1] +
                                              part[threadIdx.x][2] + part[threadIdx.x][3]);
}

// a wave-uniform double held by lane `src` of a VGPR pair
__device__ __forceinline__ double readlane_d(double v, int src) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
  return __builtin_bit_cast(double, (uint64_t)hi << 32 | lo);
}

// SHAPE: how the byte is searched.  0, the default: a guess and one exact round, the two exact
// rounds where the guess misses.  The others are kept for measurement (IDF_PREDICT_SEARCH): 2,
// the two exact rounds on every symbol; 1, one round of five probes a lane -- lane l probes bins
// 4 l - 1 .. 4 l + 3 itself, one ballot names the lane that holds the answer and five readlanes
// fetch its probes: one dependent CDF chain a step for 5 / 2 of the vector instructions.  Every
// shape decodes the same bytes, states and flags from any words.
//
// TWO: the entry may be a colour entry (`colour`, wave-uniform).  It then decodes the transformed
// planes t by the same loop -- the LDS row and the a / b / c carry hold t values -- with a second
// table, sel2's eight scales and reciprocals on lanes 8..15 beside sel's on lanes 0..7: toff, 8
// while the pixel r being decoded lies in plane 0 or 2 and else 0, is added to the bucket's lane.
// toff follows r (it changes where y wraps), never the 64-byte store batch.  An entry that is not
// a colour entry keeps toff = 0 and runs the instructions of TWO = false.
template <int SHAPE, bool TWO>
__device__ __forceinline__ void
predict_decode_entry(const int64_t k, int C, int th, int tw, const uint32_t* __restrict__ words,
                     const int64_t* __restrict__ word_off, const int64_t* __restrict__ nwords,
                     const uint64_t* __restrict__ init_state, const uint32_t* __restrict__ sel_in,
                     const uint32_t sel2, const bool colour, const int32_t* __restrict__ rect,
                     const int64_t* __restrict__ out_off, uint8_t* __restrict__ out,
                     uint64_t* __restrict__ final_state, int32_t* __restrict__ status,
                     uint64_t* tab, uint8_t* prow) {
  const int lane = threadIdx.x;
  if (lane < 32) tab[lane] = kExp2fTab[lane];
  __syncthreads();
  // the stored rectangle, held to the tile (the LDS row holds tw bytes)
  int hin = rect[2 * k], win = rect[2 * k + 1];
  hin = hin < 0 ? 0 : (hin > th ? th : hin);
  win = win < 0 ? 0 : (win > tw ? tw : win);
  const int64_t n = (int64_t)C * hin * win;
  const uint32_t* w = words + word_off[k];
  uint8_t* dst = out + out_off[k];
  int64_t pos = nwords[k];
  pos = pos < 0 ? 0 : pos;
  uint64_t state = init_state[k];
  // lane j < 8: bucket j's scale, widened, and its refined reciprocal (every scale of the model
  // lies inside fast_scale_ok)
  const uint32_t sel_l = TWO && colour && (lane & 8) ? sel2 : sel_in[k];
  const double sd_l = (double)predict_scale((int)(sel_l >> (4 * (lane & 7))) & 15);
  const double rs_l = rcp_refined(sd_l);
  const float sb_l = (float)(sd_l * 256.0 * 0.6931471805599453);  // bins per unit of log2 odds
  // the words: lane l of wA holds w[wb - 1 - l], of wB w[wb - 65 - l]; wB is loaded a whole
  // window before it is read
  auto ld_words = [&](int64_t base) -> uint32_t {
    const int64_t i = base - 1 - lane;
    return i >= 0 ? w[i] : 0u;
  };
  int64_t wb = pos;
  uint32_t wA = ld_words(wb), wB = ld_words(wb - 64);
  int32_t flag = 0;
  int x = 0, y = 0;           // the pixel being decoded, within its plane
  int a = 128, c = 128;       // the byte to the left; the byte up-left (the previous b)
  int b = 0;                  // prow[x], read one symbol ahead
  uint32_t outv = 0;          // lane t: byte r0 + t
  int toff = TWO && colour ? 8 : 0;  // plane 0 reads the second table
  int pl = 0;
  int64_t r = 0;
  for (; r < n; ++r) {
    // rans.pyx:86-89: one word when the state is below L
    if ((uint32_t)(state >> 32) == 0) {
      if (pos <= 0) {
        flag |= IDF_STREAM_UNDERFLOW;
        break;
      }
      int idx = (int)(wb - pos);
      if (idx == 64) {
        wA = wB;
        wb -= 64;
        wB = ld_words(wb - 64);
        idx = 0;
      }
      state = (state << 32) | (uint32_t)__builtin_amdgcn_readlane((int)wA, idx);
      --pos;
    }
    const int mod = (int)(state & 0xffffffull);
    // the model: neighbours, prediction, bucket, scale
    const bool left = x > 0, up = y > 0;
    int na = a, nb = __builtin_amdgcn_readfirstlane(b), nc = c;
    const int b_raw = nb;
    predict_borders(left, up, na, nb, nc);
    const int pred = predict_med(na, nb, nc);
    const int kb = (left && up ? predict_bucket(na, nb, nc) : 0) + (TWO ? toff : 0);
    const double sd = readlane_d(sd_l, kb), rs = readlane_d(rs_l, kb);
    const double mean_d = (double)pred * 0.00390625;
    const int lower = pred - 1024;  // rans.pyx:91 at mean = pred / 256
    // the next symbol's b (the row above is complete; this symbol's own slot is written below)
    const int xn = x + 1 < win ? x + 1 : 0;
    const int b_next = prow[xn];
    uint64_t mb = 1;
    int blk = 0, kk = 0, c_lo = 0, c_hi = 0, v = -1;
    if constexpr (SHAPE == 0) {
      // A guess, then ONE exact round.  Without part2's small linear term the CDF is the logistic
      // itself, so its inverse at the slot names a bin near the answer: 64 lanes probe the 64
      // bins around it and, the CDF being strictly increasing, a lane at or below the slot
      // followed by one above it IS the answer.  Nothing rests on the guess: where the window
      // misses (far tails, where part2 carries the CDF; a damaged stream) the two exact rounds
      // below run.
      float pf = (float)(mod - 1025) * 0x1p-24f;
      pf = __builtin_amdgcn_fmed3f(pf, 0x1p-23f, 1.0f - 0x1p-23f);
      const float u = __builtin_amdgcn_logf(pf * __builtin_amdgcn_rcpf(1.0f - pf));  // log2
      const float sb = __builtin_bit_cast(
          float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sb_l), kb));
      int q0 = pred - 32 + (int)(sb * u);
      q0 = q0 < -1 ? -1 : (q0 > 192 ? 192 : q0);
      const int c1 = cdf_bin(q0 + lane, lower, mean_d, sd, rs, tab);
      const uint64_t m1 = __ballot(c1 > mod);
      if (m1 != 0 && (m1 & 1) == 0) {
        const int k1 = (int)__builtin_ctzll(m1);  // 1..63
        v = q0 + k1;                              // 0..255
        c_lo = __builtin_amdgcn_readlane(c1, k1 - 1);
        c_hi = __builtin_amdgcn_readlane(c1, k1);
      }
    }
    if constexpr (SHAPE == 1) {
      int cj[5], sj[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) cj[j] = cdf_bin(4 * lane - 1 + j, lower, mean_d, sd, rs, tab);
      mb = __ballot(cj[4] > mod);
      blk = mb ? (int)__builtin_ctzll(mb) : 63;
#pragma unroll
      for (int j = 0; j < 5; ++j) sj[j] = __builtin_amdgcn_readlane(cj[j], blk);
      kk = sj[1] > mod ? 1 : (sj[2] > mod ? 2 : (sj[3] > mod ? 3 : 4));
      c_lo = kk == 1 ? sj[0] : (kk == 2 ? sj[1] : (kk == 3 ? sj[2] : sj[3]));
      c_hi = kk == 1 ? sj[1] : (kk == 2 ? sj[2] : (kk == 3 ? sj[3] : sj[4]));
      v = 4 * blk - 1 + kk;
    } else if (v < 0) {
      // round 1: the last bin of each block of four byte values
      const int c1 = cdf_bin(4 * lane + 3, lower, mean_d, sd, rs, tab);
      mb = __ballot(c1 > mod);
      blk = mb ? (int)__builtin_ctzll(mb) : 63;
      // round 2: bins 4 blk - 1 .. 4 blk + 3 on lanes 0..4
      const int c2 = cdf_bin(4 * blk - 1 + (lane < 4 ? lane : 4), lower, mean_d, sd, rs, tab);
      const uint64_t m2 = __ballot(c2 > mod) & 0x1eull;
      kk = m2 ? (int)__builtin_ctzll(m2) : 4;  // 1..4
      c_lo = __builtin_amdgcn_readlane(c2, kk - 1);
      c_hi = __builtin_amdgcn_readlane(c2, kk);
      v = 4 * blk - 1 + kk;  // 0..255 whatever the slot
    }
    // a slot below CDF(-1) or at or above CDF(255): only a damaged file; v is the clamped byte
    flag |= (mb == 0 || c_lo > mod) ? IDF_STREAM_OUT_OF_WINDOW : 0;
    // rans.pyx:108; freq >= 1 (part2 steps by one, part1 is monotone)
    state = (state >> 24) * (uint64_t)(uint32_t)(c_hi - c_lo) + (uint64_t)(int64_t)(mod - c_lo);
    // the byte: lane r % 64 keeps it for one coalesced store, the LDS row takes it
    const int t = (int)(r & 63);
    outv = lane == t ? (uint32_t)v : outv;
    if (lane == 0) prow[x] = (uint8_t)v;
    if (t == 63) dst[r - 63 + lane] = (uint8_t)outv;
    // advance: c is the b just used, a the byte just decoded
    a = v;
    c = b_raw;
    b = win == 1 ? v : b_next;  // a one-column plane reads the slot written in this step
    x = xn;
    if (xn == 0) {
      y = y + 1 < hin ? y + 1 : 0;
      if (TWO && y == 0) {  // pixel r + 1 opens plane pl + 1
        ++pl;
        toff = colour && predict_colour_second(pl) ? 8 : 0;
      }
    }
  }
  {  // the bytes decoded since the last full store (r of them in all)
    const int64_t r0 = r & ~(int64_t)63;
    if (r0 + lane < r) dst[r0 + lane] = (uint8_t)outv;
  }
  if (lane == 0) {
    final_state[k] = state;
    status[k] = flag | (pos > 0 ? IDF_STREAM_WORDS_LEFT : 0);
  }
}

template <int SHAPE>
__global__ void __launch_bounds__(64)
predict_decode_kernel(int64_t n_entries, int C, int th, int tw, const uint32_t* __restrict__ words,
                      const int64_t* __restrict__ word_off, const int64_t* __restrict__ nwords,
                      const uint64_t* __restrict__ init_state, const uint32_t* __restrict__ sel_in,
                      const int32_t* __restrict__ rect, const int64_t* __restrict__ out_off,
                      uint8_t* __restrict__ out, uint64_t* __restrict__ final_state,
                      int32_t* __restrict__ status) {
  __shared__ uint64_t tab[32];
  extern __shared__ __attribute__((aligned(16))) uint8_t prow[];  // [tw]: the row above, in place
  const int64_t k = blockIdx.x;
  if (k >= n_entries) return;
  predict_decode_entry<SHAPE, false>(k, C, th, tw, words, word_off, nwords, init_state, sel_in, 0u,
                                     false, rect, out_off, out, final_state, status, tab, prow);
}

// The decoder of IDFQ files: entry k is a colour entry iff colour[k] != 0 (C >= 3; the launcher
// checks), and then sel2[k] is its second table.  The bytes a colour entry stores are t; the
// inverse kernel below turns them into v.
template <int SHAPE>
__global__ void __launch_bounds__(64)
predict_decode2_kernel(int64_t n_entries, int C, int th, int tw, const uint32_t* __restrict__ words,
                       const int64_t* __restrict__ word_off, const int64_t* __restrict__ nwords,
                       const uint64_t* __restrict__ init_state, const uint32_t* __restrict__ sel_in,
                       const uint32_t* __restrict__ sel2_in, const uint8_t* __restrict__ colour,
                       const int32_t* __restrict__ rect, const int64_t* __restrict__ out_off,
                       uint8_t* __restrict__ out, uint64_t* __restrict__ final_state,
                       int32_t* __restrict__ status) {
  __shared__ uint64_t tab[32];
  extern __shared__ __attribute__((aligned(16))) uint8_t prow[];  // [tw]: the row above, in place
  const int64_t k = blockIdx.x;
  if (k >= n_entries) return;
  const bool col = colour[k] != 0;
  predict_decode_entry<SHAPE, true>(k, C, th, tw, words, word_off, nwords, init_state, sel_in,
                                    col ? sel2_in[k] : 0u, col, rect, out_off, out, final_state,
                                    status, tab, prow);
}

// The inverse transform of the colour entries, in place in the raw-layout buffer the decoder
// wrote: one block per entry, a thread per pixel (strided where the plane holds more than the
// block), t[0..2] of the pixel read and v[0], v[2] written.  A launch of its own after the
// decoder: the serial kernel never reads its own global stores.
__global__ void __launch_bounds__(256)
predict_colour_inverse_kernel(int th, int tw, const uint8_t* __restrict__ colour,
                              const int32_t* __restrict__ rect,
                              const int64_t* __restrict__ out_off, uint8_t* __restrict__ out) {
  const int64_t k = blockIdx.x;
  if (!colour[k]) return;
  int hin = rect[2 * k], win = rect[2 * k + 1];
  hin = hin < 0 ? 0 : (hin > th ? th : hin);
  win = win < 0 ? 0 : (win > tw ? tw : win);
  const int64_t npl = (int64_t)hin * win;
  uint8_t* dst = out + out_off[k];
  for (int64_t q = threadIdx.x; q < npl; q += blockDim.x) {
    const int t0 = dst[q], g = dst[npl + q], t2 = dst[2 * npl + q];
    dst[q] = (uint8_t)predict_colour_inv(t0, g);
    dst[2 * npl + q] = (uint8_t)predict_colour_inv(t2, g);
  }
}

// ---- the N-way decoder (predict_ways = N in {8, 16, 32, 64}; idf_predict.h has the order).
// ONE WAVE per entry, lane l < N owning state l.  The loop runs over the wavefront steps; the
// step's bookkeeping is wave-uniform: band b = t / P and local step T = t - b P give the active
// slots as two intervals, [lo0, lo0 + c0) of band b below [lo1, lo1 + c1) of band b - 1 (its
// rows' tails), cnt = c0 + c1 pixels q0 .. q0 + cnt - 1 in slot order.  Pixel q0 + k belongs to
// state (n - 1 - q0 - k) % N: lane l decodes k = (base - l) % N where base = (n - 1 - q0) % N, if
// k < cnt.  The lanes below L take their words by one ballot and a prefix count in k order (the
// serial loop's order) from a window of 128 words held across the lanes of two registers, read
// by two ds_bpermute.  The whole entry lives in LDS ([C hin][win] bytes beside the scale tables
// and a byte of row facts -- has a row above, reads the second table): a, b, c are three LDS
// reads, the decoded byte one LDS write, and the entry leaves by coalesced stores at the end.
// Each lane searches its byte alone: the inverse logistic of the slot guesses it, four exact
// probes around the guess (independent, so they overlap) name it where they bracket the slot,
// else an exact bisection of 0..255 inside what the probes left.  The answer is the bisection's
// whatever the guess.  The 64 - N spare lanes idle.
constexpr size_t PRED_WAYS_TAB_BYTES = 16 * 8 + 16 * 8 + 16 * 4;  // sd, rs: f64 [16]; sb: f32 [16]
constexpr size_t PRED_WAYS_LDS_MAX = 60 * 1024;

__host__ __device__ constexpr size_t pred_pad16(size_t v) { return (v + 15) & ~(size_t)15; }

// the dynamic LDS of one entry of a C x th x tw tile; 0 where it cannot fit
static size_t predict_ways_lds_bytes(int32_t C, int32_t th, int32_t tw) {
  if ((size_t)th > PRED_WAYS_LDS_MAX || (size_t)tw > PRED_WAYS_LDS_MAX) return 0;
  const size_t b = PRED_WAYS_TAB_BYTES + pred_pad16((size_t)C * th) +
                   pred_pad16((size_t)C * th * (size_t)tw);
  return b <= PRED_WAYS_LDS_MAX ? b : 0;
}

template <int N>
__global__ void __launch_bounds__(64)
predict_decode_ways_kernel(int64_t n_entries, int C, int th, int tw,
                           const uint32_t* __restrict__ words,
                           const int64_t* __restrict__ word_off,
                           const int64_t* __restrict__ nwords,
                           const uint64_t* __restrict__ init_state,
                           const uint32_t* __restrict__ sel_in,
                           const uint32_t* __restrict__ sel2_in,
                           const uint8_t* __restrict__ colour, const int32_t* __restrict__ rect,
                           const int64_t* __restrict__ out_off, uint8_t* __restrict__ out,
                           uint64_t* __restrict__ final_state, int32_t* __restrict__ status) {
  __shared__ uint64_t tab[32];
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int64_t k = blockIdx.x;
  if (k >= n_entries) return;
  const int lane = threadIdx.x;
  double* sd_t = reinterpret_cast<double*>(lds);
  double* rs_t = sd_t + 16;
  float* sb_t = reinterpret_cast<float*>(rs_t + 16);
  uint8_t* rinfo = lds + PRED_WAYS_TAB_BYTES;                 // [C th]: bit 0 up, bit 1 table 2
  uint8_t* pix = rinfo + pred_pad16((size_t)C * th);          // [C hin][win]
  int hin = rect[2 * k], win = rect[2 * k + 1];
  hin = hin < 0 ? 0 : (hin > th ? th : hin);
  win = win < 0 ? 0 : (win > tw ? tw : win);
  const int R = C * hin, n = R * win;
  const bool col = colour != nullptr && colour[k] != 0;
  if (lane < 32) tab[lane] = kExp2fTab[lane];
  if (lane < 16) {  // lanes 0..7: sel's buckets; 8..15: sel2's (every scale is fast_scale_ok)
    const uint32_t s = (lane & 8) ? (col ? sel2_in[k] : 0u) : sel_in[k];
    const double sd = (double)predict_scale((int)(s >> (4 * (lane & 7))) & 15);
    sd_t[lane] = sd;
    rs_t[lane] = rcp_refined(sd);
    sb_t[lane] = (float)(sd * 256.0 * 0.6931471805599453);  // bins per unit of log2 odds
  }
  for (int r = lane; r < R; r += 64) {
    const int ch = r / hin, y = r - ch * hin;
    rinfo[r] = (uint8_t)((y > 0 ? 1 : 0) | (col && predict_colour_second(ch) ? 2 : 0));
  }
  // what an entry stopped by UNDERFLOW stores for the pixels it never reached
  for (int i = 4 * lane; i < n; i += 256) *reinterpret_cast<uint32_t*>(pix + i) = 0u;
  __syncthreads();
  const uint32_t* w = words + word_off[k];
  uint8_t* dst = out + out_off[k];
  int64_t pos = nwords[k];
  pos = pos < 0 ? 0 : pos;
  uint64_t state = lane < N ? init_state[k * N + lane] : 0ull;
  // the words: lane l of wA holds w[wb - 1 - l], of wB w[wb - 65 - l]
  auto ld_words = [&](int64_t base) -> uint32_t {
    const int64_t i = base - 1 - lane;
    return i >= 0 ? w[i] : 0u;
  };
  int64_t wb = pos;
  uint32_t wA = ld_words(wb), wB = ld_words(wb - 64);
  const int P = win > N ? win : N;
  const int nb = (R + N - 1) / N;
  const int nsteps = n > 0 ? (nb - 1) * P + (R - (nb - 1) * N - 1) + win : 0;
  int b = 0, T = 0;                            // the step's band and local step
  int base = n > 0 ? (n - 1) & (N - 1) : 0;    // the state of the step's first pixel
  int32_t flag = 0;
  for (int t = 0; t < nsteps; ++t) {
    // the active slots: band b's [lo0, lo0 + c0), band b - 1's [lo1, lo1 + c1)
    int nr0 = R - b * N;
    nr0 = nr0 < 0 ? 0 : (nr0 > N ? N : nr0);
    const int lo0 = T - win + 1 > 0 ? T - win + 1 : 0;
    const int hi0 = nr0 - 1 < T ? nr0 - 1 : T;
    const int c0 = hi0 >= lo0 ? hi0 - lo0 + 1 : 0;
    const int T1 = T + P;
    int lo1 = 0, c1 = 0;
    if (b > 0) {
      int nr1 = R - (b - 1) * N;
      nr1 = nr1 < 0 ? 0 : (nr1 > N ? N : nr1);
      lo1 = T1 - win + 1 > 0 ? T1 - win + 1 : 0;
      const int hi1 = nr1 - 1 < T1 ? nr1 - 1 : T1;
      c1 = hi1 >= lo1 ? hi1 - lo1 + 1 : 0;
    }
    const int cnt = c0 + c1;
    const int kk = (base - lane) & (N - 1);
    const bool active = lane < N && kk < cnt;
    const bool head = kk < c0;
    const int j = head ? lo0 + kk : lo1 + kk - c0;
    const int rho = active ? (head ? b : b - 1) * N + j : 0;
    const int xx = active ? (head ? T : T1) - j : 0;
    // rans.pyx:86-89 for the step's states at once: the ways below L, in pixel order
    const bool need = active && (uint32_t)(state >> 32) == 0;
    const uint64_t mask = __ballot(need);
    const int total = (int)__popcll(mask);
    if ((int64_t)total > pos) {  // wave-uniform: the entry stops at the step that lacks a word
      flag |= IDF_STREAM_UNDERFLOW;
      break;
    }
    // the needing lanes ahead of this one in pixel order: those in (lane, base], cyclically
    const uint64_t le = mask & ((2ull << base) - 1ull);
    const int m = lane <= base ? (int)__popcll((le >> lane) >> 1)
                               : (int)__popcll((mask >> lane) >> 1) + (int)__popcll(le);
    const int idx = (int)(wb - pos) + m;  // 0..127 where needed
    const uint32_t g0 = (uint32_t)__shfl((int)wA, idx & 63);
    const uint32_t g1 = (uint32_t)__shfl((int)wB, idx & 63);
    if (need) state = (state << 32) | (idx < 64 ? g0 : g1);
    pos -= total;
    if (wb - pos >= 64) {
      wA = wB;
      wb -= 64;
      wB = ld_words(wb - 64);
    }
    const int mod = (int)(state & 0xffffffull);
    // the model: neighbours, prediction, bucket, scale
    const int at = rho * win + xx;
    const int info = rinfo[rho];
    const bool left = xx > 0, up = (info & 1) != 0;
    int a = pix[left ? at - 1 : at];
    int bv = pix[up ? at - win : at];
    int c = pix[left && up ? at - win - 1 : at];
    predict_borders(left, up, a, bv, c);
    const int pred = predict_med(a, bv, c);
    const int kb = (left && up ? predict_bucket(a, bv, c) : 0) + ((info & 2) ? 8 : 0);
    const double sd = sd_t[kb], rs = rs_t[kb];
    const double mean_d = (double)pred * 0.00390625;
    const int lower = pred - 1024;  // rans.pyx:91 at mean = pred / 256
    // the guess: without part2's small linear term the CDF is the logistic itself
    float pf = (float)(mod - 1025) * 0x1p-24f;
    pf = __builtin_amdgcn_fmed3f(pf, 0x1p-23f, 1.0f - 0x1p-23f);
    const float u = __builtin_amdgcn_logf(pf * __builtin_amdgcn_rcpf(1.0f - pf));  // log2
    int g = pred + (int)__builtin_floorf(sb_t[kb] * u + 0.5f);
    g = g < 1 ? 1 : (g > 254 ? 254 : g);  // the probes: bins g - 2 .. g + 1, inside -1 .. 255
    int cq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cq[i] = cdf_bin(g - 2 + i, lower, mean_d, sd, rs, tab);
    // lo: the smallest v in 0..255 with CDF(v) > mod, 256 if none (the CDF is strictly increasing)
    int lo = 0, hi = 256;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int bin = g - 2 + i;
      if (cq[i] <= mod) lo = lo > bin + 1 ? lo : bin + 1;
      else hi = hi < (bin > 0 ? bin : 0) ? hi : (bin > 0 ? bin : 0);
    }
    while (active && lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf_bin(mid, lower, mean_d, sd, rs, tab) > mod) hi = mid;
      else lo = mid + 1;
    }
    const int v = lo < 255 ? lo : 255;
    const int iv = v - (g - 2);  // bin v among the probes
    int c_lo, c_hi;
    if (iv >= 1 && iv <= 3) {
      c_lo = iv == 1 ? cq[0] : (iv == 2 ? cq[1] : cq[2]);
      c_hi = iv == 1 ? cq[1] : (iv == 2 ? cq[2] : cq[3]);
    } else {
      c_lo = cdf_bin(v - 1, lower, mean_d, sd, rs, tab);
      c_hi = cdf_bin(v, lower, mean_d, sd, rs, tab);
    }
    if (active) {
      // a slot below CDF(-1) or at or above CDF(255): only a damaged file; v is the clamped byte
      flag |= (lo == 256 || c_lo > mod) ? IDF_STREAM_OUT_OF_WINDOW : 0;
      // rans.pyx:108; freq >= 1
      state = (state >> 24) * (uint64_t)(uint32_t)(c_hi - c_lo) + (uint64_t)(int64_t)(mod - c_lo);
      pix[at] = (uint8_t)v;
    }
    __syncthreads();  // one wave: orders the step's LDS writes before the next step's reads
    base = (base - cnt) & (N - 1);
    if (++T == P) {
      T = 0;
      ++b;
    }
  }
  __syncthreads();
  for (int i = lane; i < n; i += 64) dst[i] = pix[i];
  const int32_t f = (__ballot(flag & IDF_STREAM_UNDERFLOW) ? IDF_STREAM_UNDERFLOW : 0) |
                    (__ballot(flag & IDF_STREAM_OUT_OF_WINDOW) ? IDF_STREAM_OUT_OF_WINDOW : 0);
  if (lane < N) final_state[k * N + lane] = state;
  if (lane == 0) status[k] = f | (pos > 0 ? IDF_STREAM_WORDS_LEFT : 0);
}

static bool predict_ways_ok(int32_t ways) {
  return ways == 8 || ways == 16 || ways == 32 || ways == 64;
}

// The search shape (IDF_PREDICT_SEARCH = 1 or 2; timing only, the bytes never change).
static int predict_search_shape() {
  const char* e = getenv("IDF_PREDICT_SEARCH");
  const int v = e ? atoi(e) : 0;
  return (v == 1 || v == 2) ? v : 0;
}

static int predict_launch_shape(int64_t n, int32_t C, int32_t th, int32_t tw) {
  if (n < 0 || C < 1 || C > PRED_CMAX || th < 1 || tw < 1) return IDF_ERR_ARG;
  if (n > 0x7fffffff) return IDF_ERR_ARG;
  return IDF_OK;
}

}  // namespace idf

using namespace idf;

extern "C" {

int idf_predict_tables(float scale[16], int64_t t[15]) {
  if (!scale || !t) return IDF_ERR_ARG;
  for (int j = 0; j < kPredictScales; ++j) scale[j] = predict_scale(j);
  for (int j = 0; j < kPredictScales - 1; ++j) t[j] = predict_threshold(j);
  return IDF_OK;
}

int idf_predict_prep_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                        const int64_t* d_table, const int64_t* d_sym_off, uint32_t* d_sel,
                        float* d_x, float* d_mean, float* d_scale) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_sym_off || !d_sel || !d_x || !d_mean || !d_scale) return IDF_ERR_ARG;
  hipLaunchKernelGGL(predict_prep_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0,
                     (hipStream_t)stream, C, th, tw, d_table, d_sym_off, d_sel, d_x, d_mean,
                     d_scale, 1);
  return idf_last_error();
}

int idf_predict_log2_q8(const uint32_t* freq, int64_t n, int32_t* out) {
  if (n < 0 || (n > 0 && (!freq || !out))) return IDF_ERR_ARG;
  for (int64_t i = 0; i < n; ++i) out[i] = predict_log2_q8(freq[i]);
  return IDF_OK;
}

int idf_predict_cost_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                        const int64_t* d_table, int32_t colour, int64_t* d_cost) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (colour && C < kPredictColourMinC) return IDF_ERR_ARG;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_cost) return IDF_ERR_ARG;
  if (colour)
    hipLaunchKernelGGL(predict_cost_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0,
                       (hipStream_t)stream, C, th, tw, d_table, d_cost);
  else
    hipLaunchKernelGGL(predict_cost_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0,
                       (hipStream_t)stream, C, th, tw, d_table, d_cost);
  return idf_last_error();
}

int idf_predict_decode_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                          const uint32_t* d_words, const int64_t* d_word_off,
                          const int64_t* d_nwords, const uint64_t* d_state, const uint32_t* d_sel,
                          const int32_t* d_rect, const int64_t* d_out_off, uint8_t* d_out,
                          uint64_t* d_final_state, int32_t* d_status) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_words || !d_word_off || !d_nwords || !d_state || !d_sel || !d_rect || !d_out_off ||
      !d_out || !d_final_state || !d_status)
    return IDF_ERR_ARG;
  if (tw > PRED_TW_MAX) return IDF_ERR_UNSUPPORTED;
  const size_t row_bytes = ((size_t)tw + 15) & ~(size_t)15;
#define IDF_PREDICT_DECODE(SHAPE)                                                              \
  hipLaunchKernelGGL(predict_decode_kernel<SHAPE>, dim3((unsigned)n_tiles), dim3(64), row_bytes,  \
                     (hipStream_t)stream, n_tiles, C, th, tw, d_words, d_word_off, d_nwords,      \
                     d_state, d_sel, d_rect, d_out_off, d_out, d_final_state, d_status)
  switch (predict_search_shape()) {
    case 1: IDF_PREDICT_DECODE(1); break;
    case 2: IDF_PREDICT_DECODE(2); break;
    default: IDF_PREDICT_DECODE(0); break;
  }
#undef IDF_PREDICT_DECODE
  return idf_last_error();
}

int idf_predict_prep2_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                         const int64_t* d_table, const int64_t* d_sym_off, uint32_t* d_sel,
                         float* d_x, float* d_mean, float* d_scale) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (C < kPredictColourMinC) return IDF_ERR_ARG;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_sym_off || !d_sel || !d_x || !d_mean || !d_scale) return IDF_ERR_ARG;
  hipLaunchKernelGGL(predict_prep2_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0,
                     (hipStream_t)stream, C, th, tw, d_table, d_sym_off, d_sel, d_x, d_mean,
                     d_scale, 1);
  return idf_last_error();
}

int idf_predict_decode2_u8(void* stream, int64_t n_tiles, int64_t n_colour, int32_t C, int32_t th,
                           int32_t tw, const uint32_t* d_words, const int64_t* d_word_off,
                           const int64_t* d_nwords, const uint64_t* d_state, const uint32_t* d_sel,
                           const uint32_t* d_sel2, const uint8_t* d_colour, const int32_t* d_rect,
                           const int64_t* d_out_off, uint8_t* d_out, uint64_t* d_final_state,
                           int32_t* d_status) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (n_colour < 0 || n_colour > n_tiles) return IDF_ERR_ARG;
  if (n_colour > 0 && C < kPredictColourMinC) return IDF_ERR_ARG;
  if (n_tiles == 0) return IDF_OK;
  if (!d_words || !d_word_off || !d_nwords || !d_state || !d_sel || !d_rect || !d_out_off ||
      !d_out || !d_final_state || !d_status)
    return IDF_ERR_ARG;
  if (n_colour > 0 && (!d_sel2 || !d_colour)) return IDF_ERR_ARG;
  if (tw > PRED_TW_MAX) return IDF_ERR_UNSUPPORTED;
  const size_t row_bytes = ((size_t)tw + 15) & ~(size_t)15;
  if (n_colour == 0) {  // no flag is read: idf_predict_decode_u8's launch
    return idf_predict_decode_u8(stream, n_tiles, C, th, tw, d_words, d_word_off, d_nwords,
                                 d_state, d_sel, d_rect, d_out_off, d_out, d_final_state,
                                 d_status);
  }
#define IDF_PREDICT_DECODE2(SHAPE)                                                              \
  hipLaunchKernelGGL(predict_decode2_kernel<SHAPE>, dim3((unsigned)n_tiles), dim3(64), row_bytes, \
                     (hipStream_t)stream, n_tiles, C, th, tw, d_words, d_word_off, d_nwords,      \
                     d_state, d_sel, d_sel2, d_colour, d_rect, d_out_off, d_out, d_final_state,   \
                     d_status)
  switch (predict_search_shape()) {
    case 1: IDF_PREDICT_DECODE2(1); break;
    case 2: IDF_PREDICT_DECODE2(2); break;
    default: IDF_PREDICT_DECODE2(0); break;
  }
#undef IDF_PREDICT_DECODE2
  const int rc2 = idf_last_error();
  if (rc2 != IDF_OK) return rc2;
  return idf_predict_colour_inverse_u8(stream, n_tiles, C, th, tw, d_colour, d_rect, d_out_off,
                                       d_out);
}

int idf_predict_colour_inverse_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                                  const uint8_t* d_colour, const int32_t* d_rect,
                                  const int64_t* d_out_off, uint8_t* d_out) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (C < kPredictColourMinC) return IDF_ERR_ARG;
  if (n_tiles == 0) return IDF_OK;
  if (!d_colour || !d_rect || !d_out_off || !d_out) return IDF_ERR_ARG;
  hipLaunchKernelGGL(predict_colour_inverse_kernel, dim3((unsigned)n_tiles), dim3(256), 0,
                     (hipStream_t)stream, th, tw, d_colour, d_rect, d_out_off, d_out);
  return idf_last_error();
}

// ---- predict_ways: the wavefront order and its calls

int idf_predict_order(int32_t C, int32_t hin, int32_t win, int32_t ways, int64_t* q_of_pixel) {
  if (C < 1 || C > PRED_CMAX || hin < 1 || win < 1 || !q_of_pixel) return IDF_ERR_ARG;
  if (ways != 1 && !predict_ways_ok(ways)) return IDF_ERR_ARG;
  const int64_t R = (int64_t)C * hin;
  for (int64_t rho = 0; rho < R; ++rho)
    for (int64_t x = 0; x < win; ++x) q_of_pixel[rho * win + x] = predict_rank(R, win, ways, rho, x);
  return IDF_OK;
}

int idf_predict_ways_supported(int32_t C, int32_t th, int32_t tw, int32_t ways) {
  if (C < 1 || C > PRED_CMAX || th < 1 || tw < 1 || !predict_ways_ok(ways)) return IDF_ERR_ARG;
  return predict_ways_lds_bytes(C, th, tw) ? IDF_OK : IDF_ERR_UNSUPPORTED;
}

int idf_predict_prep_ways_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                             const int64_t* d_table, const int64_t* d_sym_off, uint32_t* d_sel,
                             float* d_x, float* d_mean, float* d_scale, int32_t ways) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (!predict_ways_ok(ways)) return IDF_ERR_ARG;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_sym_off || !d_sel || !d_x || !d_mean || !d_scale) return IDF_ERR_ARG;
  hipLaunchKernelGGL(predict_prep_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0,
                     (hipStream_t)stream, C, th, tw, d_table, d_sym_off, d_sel, d_x, d_mean,
                     d_scale, ways);
  return idf_last_error();
}

int idf_predict_prep2_ways_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                              const int64_t* d_table, const int64_t* d_sym_off, uint32_t* d_sel,
                              float* d_x, float* d_mean, float* d_scale, int32_t ways) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (C < kPredictColourMinC || !predict_ways_ok(ways)) return IDF_ERR_ARG;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_sym_off || !d_sel || !d_x || !d_mean || !d_scale) return IDF_ERR_ARG;
  hipLaunchKernelGGL(predict_prep2_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0,
                     (hipStream_t)stream, C, th, tw, d_table, d_sym_off, d_sel, d_x, d_mean,
                     d_scale, ways);
  return idf_last_error();
}

int idf_predict_decode_ways_u8(void* stream, int64_t n_tiles, int64_t n_colour, int32_t ways,
                               int32_t C, int32_t th, int32_t tw, const uint32_t* d_words,
                               const int64_t* d_word_off, const int64_t* d_nwords,
                               const uint64_t* d_state, const uint32_t* d_sel,
                               const uint32_t* d_sel2, const uint8_t* d_colour,
                               const int32_t* d_rect, const int64_t* d_out_off, uint8_t* d_out,
                               uint64_t* d_final_state, int32_t* d_status) {
  const int rc = predict_launch_shape(n_tiles, C, th, tw);
  if (rc != IDF_OK) return rc;
  if (!predict_ways_ok(ways)) return IDF_ERR_ARG;
  if (n_colour < 0 || n_colour > n_tiles) return IDF_ERR_ARG;
  if (n_colour > 0 && C < kPredictColourMinC) return IDF_ERR_ARG;
  if (n_tiles == 0) return IDF_OK;
  if (!d_words || !d_word_off || !d_nwords || !d_state || !d_sel || !d_rect || !d_out_off ||
      !d_out || !d_final_state || !d_status)
    return IDF_ERR_ARG;
  if (n_colour > 0 && (!d_sel2 || !d_colour)) return IDF_ERR_ARG;
  const size_t lds_bytes = predict_ways_lds_bytes(C, th, tw);
  if (!lds_bytes) return IDF_ERR_UNSUPPORTED;
  const uint8_t* flags = n_colour > 0 ? d_colour : nullptr;  // no flag is read without one set
#define IDF_PREDICT_DECODE_WAYS(N)                                                              \
  hipLaunchKernelGGL(predict_decode_ways_kernel<N>, dim3((unsigned)n_tiles), dim3(64), lds_bytes, \
                     (hipStream_t)stream, n_tiles, C, th, tw, d_words, d_word_off, d_nwords,      \
                     d_state, d_sel, d_sel2, flags, d_rect, d_out_off, d_out, d_final_state,      \
                     d_status)
  switch (ways) {
    case 8: IDF_PREDICT_DECODE_WAYS(8); break;
    case 16: IDF_PREDICT_DECODE_WAYS(16); break;
    case 32: IDF_PREDICT_DECODE_WAYS(32); break;
    default: IDF_PREDICT_DECODE_WAYS(64); break;
  }
#undef IDF_PREDICT_DECODE_WAYS
  const int rc2 = idf_last_error();
  if (rc2 != IDF_OK || n_colour == 0) return rc2;
  return idf_predict_colour_inverse_u8(stream, n_tiles, C, th, tw, d_colour, d_rect, d_out_off,
                                       d_out);
}

}  // extern "C"
