// deep_kernels.hip -- the 16-bit predictive rANS coder (idfcodec/deep.py, container IDFD): units
// of uint16 samples coded with a causal MED predictor on their high part, an escape for what the
// 2048-bin window cannot hold and the low bits stored as they are (csrc/idf_deep.h has the model),
// through the same CDF, window and state arithmetic as every other stream (idf_cdf.h).
//
// Kernels
//   deep_prep     : one block per unit, element-wise, three passes over the unit's samples where
//                   the table says they lie.  Pass 1: min, max and, through LDS, the counts of
//                   e >= (16 << s), s = 0..7 (the histogram of bit_length(e) from 5 up, summed
//                   from above), giving the shift.  Pass 2: S_k and n_k of the 8 buckets and the
//                   escape count, giving sel.  Pass 3: x, mean, scale in stream order, the escapes
//                   in raster order -- placed by a block-wide prefix sum over chunks of 256
//                   samples, never by an atomic cursor: their order is the format -- and the low-
//                   bit words, a thread per word (a word gathers the fields that overlap it, so no
//                   word is written twice).  idf_rans_encode_streams and idf_gather_words do the
//                   rest unchanged.
//   deep_decode   : ONE WAVE per unit, by class: a constant unit is filled, a raw unit is left to
//                   the caller's copy, a packed unit runs predict_decode_entry's serial loop at 16
//                   bits: the row above as uint16 in LDS, the high part q' searched among the 2001
//                   bins pq - 1000 .. pq + 1000 -- the inverse logistic of the slot guesses a bin
//                   and 64 lanes probe the 64 bins around it in ONE exact round; where that misses,
//                   two exact rounds: lane l probes the last bin of block l of 32, one ballot names
//                   the block, 33 lanes probe it and its left neighbour -- then the escape value or
//                   (q << s) | low bits, the low words read from a 64-word window held across the
//                   lanes.
//   deep_gather_raw / deep_scatter_raw : the strided raw-tile copies at one plane and two bytes
//                   a sample.
//   deep_prep<true> : deep_prep with the symbols and the escapes in the wavefront order of N
//                   states (idf_deep.h): symbol n - 1 - q by predict_rank in closed form, the
//                   escapes marked in the unit's own n escape slots at q and compacted in place.
//   deep_decode_ways<N> : ONE WAVE per unit, lane l < N owning state l, a wavefront step of up to
//                   N samples at a time (its own comment has the loop).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "idf_cdf.h"
#include "idf_cdf_fast.h"
#include "idf_codec_internal.h"
#include "idf_deep.h"

#pragma clang fp contract(off)

namespace idf {

constexpr int DEEP_FIELDS = 8;        // addr, H, W, y0, x0, unused, sy, sx (strides in bytes)
constexpr int DEEP_TW_MAX = 16384;    // the decoder keeps one row of uint16 in LDS: 32 KiB
constexpr int DEEP_CONSTANT = 0, DEEP_PACKED = 1;  // every other class is left to the caller
constexpr uint64_t DEEP_L = 1ull << 32;

// The unit a block works on: its first in-image sample and its rectangle.  A tile outside the
// image, or a row whose address or strides are odd or negative, is empty.
struct DeepUnit {
  const uint8_t* src;
  int64_t sy, sx, hin, win, n;
  __device__ __forceinline__ int at(int64_t y, int64_t x) const {
    return (int)*reinterpret_cast<const uint16_t*>(src + y * sy + x * sx);
  }
};

__device__ __forceinline__ bool deep_row_ok(const int64_t* row) {
  return ((row[0] | row[6] | row[7]) & 1) == 0 && row[6] >= 0 && row[7] >= 0;
}

__device__ __forceinline__ DeepUnit deep_unit(const int64_t* __restrict__ table, int64_t t, int th,
                                              int tw) {
  const int64_t* row = table + t * DEEP_FIELDS;
  const int64_t H = row[1], W = row[2], y0 = row[3], x0 = row[4];
  DeepUnit u;
  u.sy = row[6], u.sx = row[7];
  const bool inside = y0 >= 0 && x0 >= 0 && y0 < H && x0 < W && deep_row_ok(row);
  u.hin = inside ? (H - y0 < th ? H - y0 : th) : 0;
  u.win = inside ? (W - x0 < tw ? W - x0 : tw) : 0;
  u.n = u.hin * u.win;
  u.src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(row[0])) +
          (inside ? y0 * u.sy + x0 * u.sx : 0);
  return u;
}

// the model at sample (y, x): its value, prediction and, for interior samples, a, b, c
__device__ __forceinline__ void deep_at(const DeepUnit& u, int64_t y, int64_t x, int& v, int& pred,
                                        int& a, int& b, int& c) {
  const bool left = x > 0, up = y > 0;
  v = u.at(y, x);
  a = left ? u.at(y, x - 1) : 0;
  b = up ? u.at(y - 1, x) : 0;
  c = left && up ? u.at(y - 1, x - 1) : 0;
  deep_borders(left, up, a, b, c);
  pred = predict_med(a, b, c);
}

// WAYS: the symbols and the escapes in the wavefront order of `ways` states (idf_deep.h: pixel q
// at index n - 1 - q, q = predict_rank at C = 1); else the raster order, `ways` unread.
template <bool WAYS>
__global__ void __launch_bounds__(256)
deep_prep_kernel(int th, int tw, const int64_t* __restrict__ table,
                 const int64_t* __restrict__ sym_off, const int64_t* __restrict__ low_off,
                 const int64_t* __restrict__ esc_off, float* __restrict__ xo,
                 float* __restrict__ mo, float* __restrict__ so, uint32_t* __restrict__ low,
                 uint32_t* __restrict__ esc, uint16_t* __restrict__ minmax,
                 uint8_t* __restrict__ shift_out, uint32_t* __restrict__ sel_out,
                 int64_t* __restrict__ nesc_out, int ways) {
  __shared__ unsigned long long acc[2 * kPredictBuckets];  // S[8], n[8]
  __shared__ unsigned int over_s[kDeepShiftMax], mn_s, mx_s, nesc_s, sel_s, wave_tot[4];
  __shared__ int shift_s;
  const int64_t t = blockIdx.x;
  const int tid = threadIdx.x;
  const DeepUnit u = deep_unit(table, t, th, tw);
  const int64_t n = u.n, win = u.win;
  const int64_t o = sym_off[t];
  if (n == 0 || sym_off[t + 1] - o != n) {  // nothing to code, or offsets that do not fit
    if (tid == 0) {
      minmax[2 * t] = 0xffff, minmax[2 * t + 1] = 0;
      shift_out[t] = 0, sel_out[t] = 0, nesc_out[t] = 0;
    }
    return;
  }
  if (tid < 2 * kPredictBuckets) acc[tid] = 0;
  if (tid < kDeepShiftMax) over_s[tid] = 0;
  if (tid == 0) mn_s = 0xffffu, mx_s = 0u, nesc_s = 0u;
  __syncthreads();
  {  // pass 1
    unsigned int over[kDeepShiftMax], mn = 0xffffu, mx = 0u;
#pragma unroll
    for (int s = 0; s < kDeepShiftMax; ++s) over[s] = 0;
    for (int64_t r = tid; r < n; r += blockDim.x) {
      const int64_t y = r / win, x = r - y * win;
      int v, pred, a, b, c;
      deep_at(u, y, x, v, pred, a, b, c);
      const int d = v - pred;
      const unsigned int e = (unsigned int)(d < 0 ? -d : d);
#pragma unroll
      for (int s = 0; s < kDeepShiftMax; ++s) over[s] += e >= ((unsigned int)kDeepShiftFloor << s);
      mn = mn < (unsigned int)v ? mn : (unsigned int)v;
      mx = mx > (unsigned int)v ? mx : (unsigned int)v;
    }
#pragma unroll
    for (int s = 0; s < kDeepShiftMax; ++s)
      if (over[s]) atomicAdd(&over_s[s], over[s]);
    atomicMin(&mn_s, mn);
    atomicMax(&mx_s, mx);
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t ov[kDeepShiftMax];
    for (int s = 0; s < kDeepShiftMax; ++s) ov[s] = over_s[s];
    shift_s = deep_shift(ov, (uint64_t)n);
    minmax[2 * t] = (uint16_t)mn_s, minmax[2 * t + 1] = (uint16_t)mx_s;
    shift_out[t] = (uint8_t)shift_s;
  }
  __syncthreads();
  const int s = shift_s;
  {  // pass 2
    uint32_t S[kPredictBuckets], cnt[kPredictBuckets], ne = 0;  // <= 1000 a sample
#pragma unroll
    for (int k = 0; k < kPredictBuckets; ++k) S[k] = cnt[k] = 0;
    for (int64_t r = tid; r < n; r += blockDim.x) {
      const int64_t y = r / win, x = r - y * win;
      int v, pred, a, b, c;
      deep_at(u, y, x, v, pred, a, b, c);
      const int kb = x > 0 && y > 0 ? deep_bucket(a, b, c, s) : 0;
      const uint32_t cost = deep_cost(v, pred, s);
      bool is_esc;
      deep_high(v, pred, s, is_esc);
      ne += is_esc ? 1u : 0u;
#pragma unroll
      for (int k = 0; k < kPredictBuckets; ++k) {
        S[k] += k == kb ? cost : 0u;
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
    if (ne) atomicAdd(&nesc_s, ne);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t sl = 0;
    for (int k = 0; k < kPredictBuckets; ++k)
      sl |= (uint32_t)predict_choose(acc[k], acc[kPredictBuckets + k]) << (4 * k);
    sel_s = sl;
    sel_out[t] = sl;
    nesc_out[t] = (int64_t)nesc_s;
  }
  __syncthreads();
  const uint32_t sel = sel_s;
  const bool any_esc = nesc_s != 0;
  // pass 3: the symbols, and the escapes in raster order.  Chunks of 256 samples, every thread in
  // every chunk (the barriers are block-wide).
  uint32_t* eo = esc + esc_off[t];
  const int lane = tid & 63, wave = tid >> 6;
  int64_t ebase = 0;
  for (int64_t r0 = 0; r0 < n; r0 += blockDim.x) {
    const int64_t r = r0 + tid;
    bool is_esc = false;
    int v = 0;
    if (r < n) {
      const int64_t y = r / win, x = r - y * win;
      int pred, a, b, c;
      deep_at(u, y, x, v, pred, a, b, c);
      const int kb = x > 0 && y > 0 ? deep_bucket(a, b, c, s) : 0;
      const int qc = deep_high(v, pred, s, is_esc);
      const int64_t q = WAYS ? predict_rank(u.hin, win, ways, y, x) : r;
      const int64_t i = o + n - 1 - q;
      xo[i] = deep_x(qc);
      mo[i] = deep_mean(pred, s);
      so[i] = predict_scale((int)(sel >> (4 * kb)) & 15);
      // WAYS: slot q of the unit's own n escape slots takes the pixel, marked, to be compacted
      if (WAYS && any_esc) eo[q] = is_esc ? (uint32_t)v | 0x10000u : 0u;
    }
    if (!WAYS && any_esc) {
      const uint64_t m = __ballot(is_esc);
      if (lane == 0) wave_tot[wave] = (unsigned int)__popcll(m);
      __syncthreads();
      int64_t before = 0, total = 0;
      for (int w = 0; w < 4; ++w) {
        before += w < wave ? wave_tot[w] : 0u;
        total += wave_tot[w];
      }
      if (is_esc) eo[ebase + before + (int64_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)v;
      ebase += total;
      __syncthreads();
    }
  }
  if (WAYS && any_esc) {
    // The marked slots, compacted in place in wavefront order: a chunk's destinations never pass
    // the chunk (ebase <= q0), every thread reads its slot before the first barrier and the next
    // chunk is read behind the second.
    __syncthreads();
    for (int64_t q0 = 0; q0 < n; q0 += blockDim.x) {
      const int64_t q = q0 + tid;
      const uint32_t val = q < n ? eo[q] : 0u;
      const bool is_esc = val != 0u;
      const uint64_t m = __ballot(is_esc);
      if (lane == 0) wave_tot[wave] = (unsigned int)__popcll(m);
      __syncthreads();
      int64_t before = 0, total = 0;
      for (int w = 0; w < 4; ++w) {
        before += w < wave ? wave_tot[w] : 0u;
        total += wave_tot[w];
      }
      if (is_esc)
        eo[ebase + before + (int64_t)__popcll(m & ((1ull << lane) - 1ull))] = val & 0xffffu;
      ebase += total;
      __syncthreads();
    }
  }
  // the low bits: word j holds bits [32 j, 32 j + 32) of the fields, field r at bit r s
  if (s > 0) {
    const int64_t nl = deep_low_words(n, s);
    uint32_t* lo = low + low_off[t];
    const uint32_t mask = (1u << s) - 1u;
    for (int64_t j = tid; j < nl; j += blockDim.x) {
      const int64_t bit0 = 32 * j;
      const int64_t rf = bit0 / s;
      int64_t rl = (bit0 + 31) / s;
      rl = rl < n - 1 ? rl : n - 1;
      uint32_t word = 0;
      for (int64_t r = rf; r <= rl; ++r) {
        const int64_t y = r / win, x = r - y * win;
        const uint32_t f = (uint32_t)u.at(y, x) & mask;
        const int sh = (int)(r * s - bit0);  // -7 .. 31
        word |= sh >= 0 ? f << sh : f >> (-sh);
      }
      lo[j] = word;
    }
  }
}

// a wave-uniform double held by lane `src` of a VGPR pair
__device__ __forceinline__ double deep_readlane_d(double v, int src) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
  return __builtin_bit_cast(double, (uint64_t)hi << 32 | lo);
}

__global__ void __launch_bounds__(64)
deep_decode_kernel(int64_t n_units, int th, int tw, const uint8_t* __restrict__ cls,
                   const uint16_t* __restrict__ value, const uint8_t* __restrict__ shift_in,
                   const uint32_t* __restrict__ sel_in, const uint64_t* __restrict__ init_state,
                   const uint32_t* __restrict__ words, const int64_t* __restrict__ word_off,
                   const int64_t* __restrict__ nwords, const uint32_t* __restrict__ low,
                   const int64_t* __restrict__ low_off, const uint32_t* __restrict__ esc,
                   const int64_t* __restrict__ esc_off, const int64_t* __restrict__ nesc,
                   const int32_t* __restrict__ rect, const int64_t* __restrict__ out_off,
                   uint16_t* __restrict__ out, uint64_t* __restrict__ final_state,
                   int32_t* __restrict__ status) {
  __shared__ uint64_t tab[32];
  extern __shared__ __attribute__((aligned(16))) uint16_t deep_prow[];  // [tw]: the row above
  uint16_t* prow = deep_prow;
  const int64_t k = blockIdx.x;
  if (k >= n_units) return;
  const int lane = threadIdx.x;
  // the stored rectangle, held to the tile (the LDS row holds tw samples)
  int hin = rect[2 * k], win = rect[2 * k + 1];
  hin = hin < 0 ? 0 : (hin > th ? th : hin);
  win = win < 0 ? 0 : (win > tw ? tw : win);
  const int64_t n = (int64_t)hin * win;
  uint16_t* dst = out + out_off[k];
  const int kind = cls[k];
  if (kind != DEEP_PACKED) {
    if (kind == DEEP_CONSTANT) {
      const uint16_t cv = value[k];
      for (int64_t i = lane; i < n; i += 64) dst[i] = cv;
    }
    if (lane == 0) final_state[k] = DEEP_L, status[k] = 0;
    return;
  }
  if (lane < 32) tab[lane] = kExp2fTab[lane];
  __syncthreads();
  int32_t flag = 0;
  int s = shift_in[k];
  if (s > kDeepShiftMax) {  // only a damaged file
    s = kDeepShiftMax;
    flag |= IDF_STREAM_OUT_OF_WINDOW;
  }
  const uint32_t* w = words + word_off[k];
  int64_t pos = nwords[k];
  pos = pos < 0 ? 0 : pos;
  uint64_t state = init_state[k];
  // lane j < 8: bucket j's scale, widened, and its refined reciprocal (every scale of the model
  // lies inside fast_scale_ok)
  const double sd_l = (double)predict_scale((int)(sel_in[k] >> (4 * (lane & 7))) & 15);
  const double rs_l = rcp_refined(sd_l);
  const float sb_l = (float)(sd_l * 256.0 * 0.6931471805599453);  // bins per unit of log2 odds
  // the words: lane l of wA holds w[wb - 1 - l], of wB w[wb - 65 - l]
  auto ld_words = [&](int64_t base) -> uint32_t {
    const int64_t i = base - 1 - lane;
    return i >= 0 ? w[i] : 0u;
  };
  int64_t wb = pos;
  uint32_t wA = ld_words(wb), wB = ld_words(wb - 64);
  // the low bits: lane l of lwin holds lw[lbase + l]
  const int64_t nl = deep_low_words(n, s);
  const uint32_t* lw = low + low_off[k];
  auto ld_low = [&](int64_t base) -> uint32_t { return base + lane < nl ? lw[base + lane] : 0u; };
  int64_t lbase = 0;
  uint32_t lwin = s > 0 ? ld_low(0) : 0u;
  const uint32_t lmask = (1u << s) - 1u;
  // the escapes
  const uint32_t* ep = esc + esc_off[k];
  int64_t ne = nesc[k], ei = 0;
  ne = ne < 0 ? 0 : ne;
  int x = 0, y = 0;                           // the sample being decoded
  int a = kDeepOrigin, c = kDeepOrigin;       // the sample to the left; up-left (the previous b)
  int b = 0;                                  // prow[x], read one symbol ahead
  uint32_t outv = 0;                          // lane t: sample r0 + t
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
    deep_borders(left, up, na, nb, nc);
    const int pred = predict_med(na, nb, nc);
    const int kb = left && up ? deep_bucket(na, nb, nc, s) : 0;
    const double sd = deep_readlane_d(sd_l, kb), rs = deep_readlane_d(rs_l, kb);
    const double mean_d = (double)deep_mean(pred, s);
    const int pq = pred >> s;
    const int lower = pq - 1024;  // rans.pyx:91: round(mean * 256 - 1024), never at a half
    // the next symbol's b (the row above is complete; this symbol's own slot is written below)
    const int xn = x + 1 < win ? x + 1 : 0;
    const int b_next = prow[xn];
    int qv = 0, c_lo = 0, c_hi = 0;
    bool found = false;
    {
      // A guess, then ONE exact round.  Without part2's small linear term the CDF is the logistic
      // itself, so its inverse at the slot names a bin near the answer: 64 lanes probe the 64
      // bins around it and, the CDF being strictly increasing, a lane at or below the slot
      // followed by one above it IS the answer.  Nothing rests on the guess.
      float pf = (float)(mod - 1025) * 0x1p-24f;
      pf = __builtin_amdgcn_fmed3f(pf, 0x1p-23f, 1.0f - 0x1p-23f);
      const float uu = __builtin_amdgcn_logf(pf * __builtin_amdgcn_rcpf(1.0f - pf));  // log2
      const float sb = __builtin_bit_cast(
          float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sb_l), kb));
      int q0 = pq - 32 + (int)(sb * uu);
      q0 = q0 < pq - kDeepEscape - 1 ? pq - kDeepEscape - 1
                                     : (q0 > pq + kDeepEscape - 63 ? pq + kDeepEscape - 63 : q0);
      const int c1 = cdf_bin(q0 + lane, lower, mean_d, sd, rs, tab);
      const uint64_t m1 = __ballot(c1 > mod);
      if (m1 != 0 && (m1 & 1) == 0) {
        const int k1 = (int)__builtin_ctzll(m1);  // 1..63
        qv = q0 + k1;                             // pq - 1000 .. pq + 1000
        c_lo = __builtin_amdgcn_readlane(c1, k1 - 1);
        c_hi = __builtin_amdgcn_readlane(c1, k1);
        found = true;
      }
    }
    if (!found) {
      // bin j is q = base0 + j, j = 0 .. 2048; the answer is the smallest j >= 1 with CDF > slot
      const int base0 = pq - kDeepEscape - 1;
      // round 1: the last bin of each block of 32 (block l: j = 32 l + 1 .. 32 l + 32)
      const int c1 = cdf_bin(base0 + 32 * lane + 32, lower, mean_d, sd, rs, tab);
      const uint64_t mb = __ballot(c1 > mod);
      const int blk = mb ? (int)__builtin_ctzll(mb) : 63;
      // round 2: j = 32 blk .. 32 blk + 32 on lanes 0..32
      const int c2 = cdf_bin(base0 + 32 * blk + (lane < 32 ? lane : 32), lower, mean_d, sd, rs, tab);
      const uint64_t m2 = __ballot(c2 > mod) & 0x1fffffffeull;
      const int kk = m2 ? (int)__builtin_ctzll(m2) : 32;  // 1..32
      c_lo = __builtin_amdgcn_readlane(c2, kk - 1);
      c_hi = __builtin_amdgcn_readlane(c2, kk);
      qv = base0 + 32 * blk + kk;
      // a slot below CDF(pq - 1001) or at or above CDF(pq + 1000): only a damaged file; the
      // high part is clamped
      bool bad = mb == 0 || c_lo > mod;
      if (qv > pq + kDeepEscape) {
        qv = pq + kDeepEscape;
        c_lo = cdf_bin(qv - 1, lower, mean_d, sd, rs, tab);
        c_hi = cdf_bin(qv, lower, mean_d, sd, rs, tab);
        bad = true;
      }
      flag |= bad ? IDF_STREAM_OUT_OF_WINDOW : 0;
    }
    // rans.pyx:108; freq >= 1 (part2 steps by one, part1 is monotone)
    state = (state >> 24) * (uint64_t)(uint32_t)(c_hi - c_lo) + (uint64_t)(int64_t)(mod - c_lo);
    // the sample: the next escape, or the high part above the stored low bits
    int v;
    const int dq = qv - pq;
    if (dq == kDeepEscape || dq == -kDeepEscape) {
      if (ei >= ne) {
        flag |= IDF_STREAM_UNDERFLOW;
        break;
      }
      v = (int)(ep[ei] & 0xffffu);
      ++ei;
    } else {
      uint32_t f = 0;
      if (s > 0) {
        const int64_t bit = r * s, wi = bit >> 5;
        if (wi - lbase >= 63) {
          lbase = wi;
          lwin = ld_low(lbase);
        }
        const int i0 = (int)(wi - lbase);  // 0..62
        const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)lwin, i0);
        const uint32_t w1 = (uint32_t)__builtin_amdgcn_readlane((int)lwin, i0 + 1);
        f = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (int)(bit & 31)) & lmask;
      }
      v = qv * (1 << s) + (int)f;
      if (v < 0 || v > 0xffff) {  // only a damaged file
        v = v < 0 ? 0 : 0xffff;
        flag |= IDF_STREAM_OUT_OF_WINDOW;
      }
    }
    // lane r % 64 keeps it for one coalesced store, the LDS row takes it
    const int t = (int)(r & 63);
    outv = lane == t ? (uint32_t)v : outv;
    if (lane == 0) prow[x] = (uint16_t)v;
    if (t == 63) dst[r - 63 + lane] = (uint16_t)outv;
    // advance: c is the b just used, a the sample just decoded
    a = v;
    c = b_raw;
    b = win == 1 ? v : b_next;  // a one-column unit reads the slot written in this step
    x = xn;
    if (xn == 0) y = y + 1 < hin ? y + 1 : 0;
  }
  {  // the samples decoded since the last full store (r of them in all)
    const int64_t r0 = r & ~(int64_t)63;
    if (r0 + lane < r) dst[r0 + lane] = (uint16_t)outv;
  }
  if (lane == 0) {
    final_state[k] = state;
    status[k] = flag | (pos > 0 || ei < ne ? IDF_STREAM_WORDS_LEFT : 0);
  }
}

// ---- the N-way decoder (ways = N in {8, 16, 32, 64}; idf_deep.h has the order and the step rule).
// ONE WAVE per unit, lane l < N owning state l, the step loop of predict_decode_ways_kernel at
// C = 1: wave-uniform band b and local step T give the active slots as two intervals, pixel
// q0 + k of the step belongs to state (n - 1 - q0 - k) % N, so lane l decodes k = (base - l) % N
// where base = (n - 1 - q0) % N, if k < cnt.  The words of the lanes below L come by one ballot
// and a prefix count in k order from a window of 128 words across two registers.  The unit lives
// in LDS as uint16 [hin][win], zeroed first, beside the 8 scales, reciprocals and guess slopes;
// a, b, c are three LDS reads and the unit leaves by coalesced stores at the end.  Each lane
// searches its high part alone among pq - 1000 .. pq + 1000: the inverse logistic of the slot
// guesses a bin, four exact probes around it (independent, so they overlap) name it where they
// bracket the slot, else an exact bisection inside what the probes left, at most 11 rounds; the
// answer is the bisection's whatever the guess.  The escaped lanes of a step find their values by
// one ballot of |q' - pq| == 1000 and the same prefix count.  A lane's low-bit field lies where
// the geometry says, so its two words are loaded at the top of the step, off the dependent chain.
// A step's new states, cursors and flags are committed only once its words and escapes are known
// to suffice.  Every index is bounded: words by nwords, low words by nl, escapes by nesc, pixels
// by the rectangle held to the tile.
constexpr size_t DEEP_WAYS_TAB_BYTES = 8 * 8 + 8 * 8 + 8 * 4;  // sd, rs: f64 [8]; sb: f32 [8]
constexpr size_t DEEP_WAYS_LDS_MAX = 60 * 1024;

// the dynamic LDS of one unit of a th x tw tile; 0 where it cannot fit
static size_t deep_ways_lds_bytes(int32_t th, int32_t tw) {
  if ((size_t)th > DEEP_WAYS_LDS_MAX || (size_t)tw > DEEP_WAYS_LDS_MAX) return 0;
  const size_t b = DEEP_WAYS_TAB_BYTES + ((2 * (size_t)th * (size_t)tw + 15) & ~(size_t)15);
  return b <= DEEP_WAYS_LDS_MAX ? b : 0;
}

template <int N>
__global__ void __launch_bounds__(64)
deep_decode_ways_kernel(int64_t n_units, int th, int tw, const uint8_t* __restrict__ cls,
                        const uint16_t* __restrict__ value, const uint8_t* __restrict__ shift_in,
                        const uint32_t* __restrict__ sel_in,
                        const uint64_t* __restrict__ init_state,
                        const uint32_t* __restrict__ words, const int64_t* __restrict__ word_off,
                        const int64_t* __restrict__ nwords, const uint32_t* __restrict__ low,
                        const int64_t* __restrict__ low_off, const uint32_t* __restrict__ esc,
                        const int64_t* __restrict__ esc_off, const int64_t* __restrict__ nesc,
                        const int32_t* __restrict__ rect, const int64_t* __restrict__ out_off,
                        uint16_t* __restrict__ out, uint64_t* __restrict__ final_state,
                        int32_t* __restrict__ status) {
  __shared__ uint64_t tab[32];
  extern __shared__ __attribute__((aligned(16))) uint8_t deep_lds[];
  const int64_t k = blockIdx.x;
  if (k >= n_units) return;
  const int lane = threadIdx.x;
  double* sd_t = reinterpret_cast<double*>(deep_lds);
  double* rs_t = sd_t + 8;
  float* sb_t = reinterpret_cast<float*>(rs_t + 8);
  uint16_t* pix = reinterpret_cast<uint16_t*>(deep_lds + DEEP_WAYS_TAB_BYTES);  // [hin][win]
  int hin = rect[2 * k], win = rect[2 * k + 1];
  hin = hin < 0 ? 0 : (hin > th ? th : hin);
  win = win < 0 ? 0 : (win > tw ? tw : win);
  const int n = hin * win;
  uint16_t* dst = out + out_off[k];
  const int kind = cls[k];
  if (kind != DEEP_PACKED) {
    if (kind == DEEP_CONSTANT) {
      const uint16_t cv = value[k];
      for (int i = lane; i < n; i += 64) dst[i] = cv;
    }
    if (lane < N) final_state[k * N + lane] = DEEP_L;
    if (lane == 0) status[k] = 0;
    return;
  }
  if (lane < 32) tab[lane] = kExp2fTab[lane];
  if (lane < 8) {  // bucket `lane`'s scale, widened (every scale of the model is fast_scale_ok)
    const double sd = (double)predict_scale((int)(sel_in[k] >> (4 * lane)) & 15);
    sd_t[lane] = sd;
    rs_t[lane] = rcp_refined(sd);
    sb_t[lane] = (float)(sd * 256.0 * 0.6931471805599453);  // bins per unit of log2 odds
  }
  // what a unit stopped by UNDERFLOW stores for the pixels it never reached (the area is padded
  // to 16 bytes, so the last pair of an odd n stays inside it)
  for (int i = 2 * lane; i < n; i += 128) *reinterpret_cast<uint32_t*>(pix + i) = 0u;
  __syncthreads();
  int32_t flag = 0;
  int s = shift_in[k];
  if (s > kDeepShiftMax) {  // only a damaged file
    s = kDeepShiftMax;
    flag |= IDF_STREAM_OUT_OF_WINDOW;
  }
  const uint32_t* w = words + word_off[k];
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
  const int64_t nl = deep_low_words(n, s);
  const uint32_t* lw = low + low_off[k];
  const uint32_t lmask = (1u << s) - 1u;
  const uint32_t* ep = esc + esc_off[k];
  int64_t ne = nesc[k], ei = 0;
  ne = ne < 0 ? 0 : ne;
  const int R = hin;
  const int P = win > N ? win : N;
  const int nb = (R + N - 1) / N;
  const int nsteps = n > 0 ? (nb - 1) * P + (R - (nb - 1) * N - 1) + win : 0;
  int b = 0, T = 0;                            // the step's band and local step
  int base = n > 0 ? (n - 1) & (N - 1) : 0;    // the state of the step's first pixel
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
    const int yy = active ? (head ? b : b - 1) * N + j : 0;
    const int xx = active ? (head ? T : T1) - j : 0;
    const int at = yy * win + xx;
    // the low bits: the field of pixel `at` lies at bit at * s, in two words of the run
    uint32_t l0 = 0, l1 = 0;
    if (s > 0 && active) {
      const int64_t wi = ((int64_t)at * s) >> 5;
      l0 = wi < nl ? lw[wi] : 0u;
      l1 = wi + 1 < nl ? lw[wi + 1] : 0u;
    }
    // the lanes of `mask` ahead of this one in pixel order: those in (lane, base], cyclically
    auto ahead = [&](uint64_t mask) -> int {
      const uint64_t le = mask & ((2ull << base) - 1ull);
      return lane <= base ? (int)__popcll((le >> lane) >> 1)
                          : (int)__popcll((mask >> lane) >> 1) + (int)__popcll(le);
    };
    // rans.pyx:86-89 for the step's states at once: the ways below L, in pixel order
    const bool need = active && (uint32_t)(state >> 32) == 0;
    const uint64_t wmask = __ballot(need);
    const int total = (int)__popcll(wmask);
    if ((int64_t)total > pos) {  // wave-uniform: the unit stops at the step that lacks a word
      flag |= IDF_STREAM_UNDERFLOW;
      break;
    }
    const int idx = (int)(wb - pos) + ahead(wmask);  // 0..127 where needed
    const uint32_t g0 = (uint32_t)__shfl((int)wA, idx & 63);
    const uint32_t g1 = (uint32_t)__shfl((int)wB, idx & 63);
    const uint64_t st = need ? (state << 32) | (idx < 64 ? g0 : g1) : state;
    const int mod = (int)(st & 0xffffffull);
    // the model: neighbours, prediction, bucket, scale
    const bool left = xx > 0, up = yy > 0;
    int a = pix[left ? at - 1 : at];
    int bv = pix[up ? at - win : at];
    int c = pix[left && up ? at - win - 1 : at];
    deep_borders(left, up, a, bv, c);
    const int pred = predict_med(a, bv, c);
    const int kb = left && up ? deep_bucket(a, bv, c, s) : 0;
    const double sd = sd_t[kb], rs = rs_t[kb];
    const double mean_d = (double)deep_mean(pred, s);
    const int pq = pred >> s;
    const int lower = pq - 1024;  // rans.pyx:91: round(mean * 256 - 1024), never at a half
    // the guess: without part2's small linear term the CDF is the logistic itself
    float pf = (float)(mod - 1025) * 0x1p-24f;
    pf = __builtin_amdgcn_fmed3f(pf, 0x1p-23f, 1.0f - 0x1p-23f);
    const float uu = __builtin_amdgcn_logf(pf * __builtin_amdgcn_rcpf(1.0f - pf));  // log2
    float gf = __builtin_floorf(sb_t[kb] * uu + 0.5f);
    gf = __builtin_amdgcn_fmed3f(gf, -(float)(kDeepEscape - 2), (float)(kDeepEscape - 1));
    const int g = pq + (int)gf;  // the probes: bins g - 2 .. g + 1, inside pq - 1000 .. pq + 1000
    int cq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cq[i] = cdf_bin(g - 2 + i, lower, mean_d, sd, rs, tab);
    // lo: the smallest q in pq - 1000 .. pq + 1000 with CDF(q) > mod, pq + 1001 if none
    int lo = pq - kDeepEscape, hi = pq + kDeepEscape + 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int bin = g - 2 + i;
      if (cq[i] <= mod) lo = lo > bin + 1 ? lo : bin + 1;
      else hi = hi < bin ? hi : bin;
    }
    while (active && lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (cdf_bin(mid, lower, mean_d, sd, rs, tab) > mod) hi = mid;
      else lo = mid + 1;
    }
    const int qv = lo < pq + kDeepEscape ? lo : pq + kDeepEscape;
    const int iv = qv - (g - 2);  // bin qv among the probes
    int c_lo, c_hi;
    if (iv >= 1 && iv <= 3) {
      c_lo = iv == 1 ? cq[0] : (iv == 2 ? cq[1] : cq[2]);
      c_hi = iv == 1 ? cq[1] : (iv == 2 ? cq[2] : cq[3]);
    } else {
      c_lo = cdf_bin(qv - 1, lower, mean_d, sd, rs, tab);
      c_hi = cdf_bin(qv, lower, mean_d, sd, rs, tab);
    }
    // the step's escapes, in pixel order
    const int dq = qv - pq;
    const bool is_esc = active && (dq == kDeepEscape || dq == -kDeepEscape);
    const uint64_t emask = __ballot(is_esc);
    const int etotal = (int)__popcll(emask);
    if (ei + etotal > ne) {  // wave-uniform: nothing of the step is kept
      flag |= IDF_STREAM_UNDERFLOW;
      break;
    }
    if (active) {
      // a slot below CDF(pq - 1001) or at or above CDF(pq + 1000): only a damaged file; the high
      // part is clamped
      flag |= (lo > pq + kDeepEscape || c_lo > mod) ? IDF_STREAM_OUT_OF_WINDOW : 0;
      // rans.pyx:108; freq >= 1
      state = (st >> 24) * (uint64_t)(uint32_t)(c_hi - c_lo) + (uint64_t)(int64_t)(mod - c_lo);
      int v;
      if (is_esc) {
        v = (int)(ep[ei + ahead(emask)] & 0xffffu);
      } else {
        const uint32_t f =
            (uint32_t)((((uint64_t)l1 << 32) | l0) >> (int)(((int64_t)at * s) & 31)) & lmask;
        v = qv * (1 << s) + (int)f;
        if (v < 0 || v > 0xffff) {  // only a damaged file
          v = v < 0 ? 0 : 0xffff;
          flag |= IDF_STREAM_OUT_OF_WINDOW;
        }
      }
      pix[at] = (uint16_t)v;
    }
    pos -= total;
    ei += etotal;
    if (wb - pos >= 64) {
      wA = wB;
      wb -= 64;
      wB = ld_words(wb - 64);
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
  if (lane == 0) status[k] = f | (pos > 0 || ei < ne ? IDF_STREAM_WORDS_LEFT : 0);
}

// The in-image rectangle of unit t as dense uint16 [hin][win] at out + off[t] (in samples).
__global__ void __launch_bounds__(256)
deep_gather_raw_kernel(int th, int tw, const int64_t* __restrict__ table,
                       const int64_t* __restrict__ off, uint16_t* __restrict__ out) {
  const int64_t t = blockIdx.x;
  const DeepUnit u = deep_unit(table, t, th, tw);
  uint16_t* dst = out + off[t];
  for (int64_t r = threadIdx.x; r < u.n; r += blockDim.x) {
    const int64_t y = r / u.win, x = r - y * u.win;
    dst[r] = (uint16_t)u.at(y, x);
  }
}

// The inverse: sample (y, x) of the stored [hin][win] rectangle of unit t (rect[t] = (hin, win),
// held to the tile) to image sample (y0 + y, x0 + x), only inside [0,H) x [0,W).
__global__ void __launch_bounds__(256)
deep_scatter_raw_kernel(int th, int tw, const uint16_t* __restrict__ in,
                        const int64_t* __restrict__ off, const int32_t* __restrict__ rect,
                        const int64_t* __restrict__ table) {
  const int64_t t = blockIdx.x;
  const int64_t* row = table + t * DEEP_FIELDS;
  if (!deep_row_ok(row)) return;
  uint8_t* base = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(row[0]));
  const int64_t H = row[1], W = row[2], y0 = row[3], x0 = row[4], sy = row[6], sx = row[7];
  int64_t hin = rect[2 * t], win = rect[2 * t + 1];
  hin = hin < 0 ? 0 : (hin > th ? th : hin);
  win = win < 0 ? 0 : (win > tw ? tw : win);
  const uint16_t* src = in + off[t];
  for (int64_t r = threadIdx.x; r < hin * win; r += blockDim.x) {
    const int64_t yy = r / win, xx = r - yy * win;
    const int64_t y = y0 + yy, x = x0 + xx;
    if (y < 0 || y >= H || x < 0 || x >= W) continue;  // outside a crop
    *reinterpret_cast<uint16_t*>(base + y * sy + x * sx) = src[r];
  }
}

static int deep_launch_shape(int64_t n, int32_t th, int32_t tw) {
  if (n < 0 || n > 0x7fffffff || th < 1 || tw < 1) return IDF_ERR_ARG;
  return IDF_OK;
}

// the rows of a host copy of the table: an odd or negative address or stride is refused
static int deep_check_rows(const int64_t* h_table, int64_t n) {
  if (!h_table) return IDF_OK;
  for (int64_t t = 0; t < n; ++t) {
    const int64_t* row = h_table + t * DEEP_FIELDS;
    if (((row[0] | row[6] | row[7]) & 1) != 0 || row[6] < 0 || row[7] < 0) return IDF_ERR_ARG;
  }
  return IDF_OK;
}

// ---- the model on the host: one dense unit, the header's functions and nothing else
struct DeepHostUnit {
  const uint16_t* p;
  int64_t hin, win;
  void at(int64_t y, int64_t x, int& v, int& pred, int& a, int& b, int& c) const {
    const bool left = x > 0, up = y > 0;
    v = p[y * win + x];
    a = left ? p[y * win + x - 1] : 0;
    b = up ? p[(y - 1) * win + x] : 0;
    c = left && up ? p[(y - 1) * win + x - 1] : 0;
    deep_borders(left, up, a, b, c);
    pred = predict_med(a, b, c);
  }
};

static bool deep_ways_ok(int32_t ways) {
  return ways == 8 || ways == 16 || ways == 32 || ways == 64;
}

// perm[q]: the raster index of the pixel of rank q at `ways` states (1: the raster order itself)
static std::vector<int64_t> deep_order(int64_t hin, int64_t win, int ways) {
  std::vector<int64_t> perm((size_t)(hin * win));
  for (int64_t y = 0; y < hin; ++y)
    for (int64_t x = 0; x < win; ++x)
      perm[(size_t)(ways > 1 ? predict_rank(hin, win, ways, y, x) : y * win + x)] = y * win + x;
  return perm;
}

// One sample of the host decoders: the model at (y, x) of the unit decoded so far and the search,
// by bisection over the exact CDF.  state: word taken; -> the high part, clamped, the new state
// and the flags.
static int deep_host_symbol(const DeepHostUnit& u, int64_t y, int64_t xx, int s, uint32_t sel,
                            uint64_t& state, int& pq, int32_t& flag) {
  int v, pred, a, b, c;
  u.at(y, xx, v, pred, a, b, c);
  const int kb = xx > 0 && y > 0 ? deep_bucket(a, b, c, s) : 0;
  const float mean = deep_mean(pred, s), scale = predict_scale((int)(sel >> (4 * kb)) & 15);
  const float lower = rans_lower_f(rans_lower_int(mean));
  const int mod = (int)(state & 0xffffffull);
  pq = pred >> s;
  // the smallest q in pq - 1000 .. pq + 1000 with CDF(q) > mod, pq + 1001 if none
  int lo = pq - kDeepEscape, hi = pq + kDeepEscape + 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rans_cdf(deep_x(mid), mean, scale, lower, kExp2fTabHost) > mod) hi = mid;
    else lo = mid + 1;
  }
  const int qv = lo > pq + kDeepEscape ? pq + kDeepEscape : lo;
  const int c_lo = rans_cdf(deep_x(qv - 1), mean, scale, lower, kExp2fTabHost);
  const int c_hi = rans_cdf(deep_x(qv), mean, scale, lower, kExp2fTabHost);
  if (lo > pq + kDeepEscape || c_lo > mod) flag |= IDF_STREAM_OUT_OF_WINDOW;
  state = (state >> 24) * (uint64_t)(uint32_t)(c_hi - c_lo) + (uint64_t)(int64_t)(mod - c_lo);
  return qv;
}

// the sample of high part qv that is not escaped: above its stored low bits, clamped
static int deep_host_sample(int qv, int64_t r, int64_t n, int s, const uint32_t* low,
                            int32_t& flag) {
  uint32_t f = 0;
  if (s > 0) {
    const int64_t bit = r * s, wi = bit >> 5, nl = deep_low_words(n, s);
    const uint64_t two = (uint64_t)low[wi] | (wi + 1 < nl ? (uint64_t)low[wi + 1] << 32 : 0);
    f = (uint32_t)(two >> (bit & 31)) & ((1u << s) - 1u);
  }
  int v = qv * (1 << s) + (int)f;
  if (v < 0 || v > 0xffff) {
    v = v < 0 ? 0 : 0xffff;
    flag |= IDF_STREAM_OUT_OF_WINDOW;
  }
  return v;
}

}  // namespace idf

using namespace idf;

extern "C" {

int idf_deep_tw_max(void) { return DEEP_TW_MAX; }

int idf_deep_prep_u16(void* stream, int64_t n_units, int32_t th, int32_t tw,
                      const int64_t* d_table, const int64_t* h_table, const int64_t* d_sym_off,
                      const int64_t* d_low_off, const int64_t* d_esc_off, float* d_x,
                      float* d_mean, float* d_scale, uint32_t* d_low, uint32_t* d_esc,
                      uint16_t* d_minmax, uint8_t* d_shift, uint32_t* d_sel, int64_t* d_nesc) {
  const int rc = deep_launch_shape(n_units, th, tw);
  if (rc != IDF_OK) return rc;
  if (n_units == 0) return IDF_OK;
  if (!d_table || !d_sym_off || !d_low_off || !d_esc_off || !d_x || !d_mean || !d_scale ||
      !d_low || !d_esc || !d_minmax || !d_shift || !d_sel || !d_nesc)
    return IDF_ERR_ARG;
  if (deep_check_rows(h_table, n_units) != IDF_OK) return IDF_ERR_ARG;
  hipLaunchKernelGGL(deep_prep_kernel<false>, dim3((unsigned)n_units), dim3(256), 0,
                     (hipStream_t)stream, th, tw, d_table, d_sym_off, d_low_off, d_esc_off, d_x,
                     d_mean, d_scale, d_low, d_esc, d_minmax, d_shift, d_sel, d_nesc, 1);
  return idf_last_error();
}

int idf_deep_decode_u16(void* stream, int64_t n_units, int32_t th, int32_t tw,
                        const uint8_t* d_class, const uint16_t* d_value, const uint8_t* d_shift,
                        const uint32_t* d_sel, const uint64_t* d_state, const uint32_t* d_words,
                        const int64_t* d_word_off, const int64_t* d_nwords, const uint32_t* d_low,
                        const int64_t* d_low_off, const uint32_t* d_esc, const int64_t* d_esc_off,
                        const int64_t* d_nesc, const int32_t* d_rect, const int64_t* d_out_off,
                        uint16_t* d_out, uint64_t* d_final_state, int32_t* d_status) {
  const int rc = deep_launch_shape(n_units, th, tw);
  if (rc != IDF_OK) return rc;
  if (n_units == 0) return IDF_OK;
  if (!d_class || !d_value || !d_shift || !d_sel || !d_state || !d_words || !d_word_off ||
      !d_nwords || !d_low || !d_low_off || !d_esc || !d_esc_off || !d_nesc || !d_rect ||
      !d_out_off || !d_out || !d_final_state || !d_status)
    return IDF_ERR_ARG;
  if (tw > DEEP_TW_MAX) return IDF_ERR_UNSUPPORTED;
  const size_t row_bytes = (2 * (size_t)tw + 15) & ~(size_t)15;
  hipLaunchKernelGGL(deep_decode_kernel, dim3((unsigned)n_units), dim3(64), row_bytes,
                     (hipStream_t)stream, n_units, th, tw, d_class, d_value, d_shift, d_sel,
                     d_state, d_words, d_word_off, d_nwords, d_low, d_low_off, d_esc, d_esc_off,
                     d_nesc, d_rect, d_out_off, d_out, d_final_state, d_status);
  return idf_last_error();
}

int idf_tile_gather_raw_strided_u16(void* stream, int64_t n_units, int32_t th, int32_t tw,
                                    const int64_t* d_table, const int64_t* h_table,
                                    const int64_t* d_off, uint16_t* d_out) {
  const int rc = deep_launch_shape(n_units, th, tw);
  if (rc != IDF_OK) return rc;
  if (n_units == 0) return IDF_OK;
  if (!d_table || !d_off || !d_out) return IDF_ERR_ARG;
  if (deep_check_rows(h_table, n_units) != IDF_OK) return IDF_ERR_ARG;
  hipLaunchKernelGGL(deep_gather_raw_kernel, dim3((unsigned)n_units), dim3(256), 0,
                     (hipStream_t)stream, th, tw, d_table, d_off, d_out);
  return idf_last_error();
}

int idf_tile_scatter_raw_strided_u16(void* stream, int64_t n_units, int32_t th, int32_t tw,
                                     const uint16_t* d_in, const int64_t* d_off,
                                     const int32_t* d_rect, const int64_t* d_table,
                                     const int64_t* h_table) {
  const int rc = deep_launch_shape(n_units, th, tw);
  if (rc != IDF_OK) return rc;
  if (n_units == 0) return IDF_OK;
  if (!d_in || !d_off || !d_rect || !d_table) return IDF_ERR_ARG;
  if (deep_check_rows(h_table, n_units) != IDF_OK) return IDF_ERR_ARG;
  hipLaunchKernelGGL(deep_scatter_raw_kernel, dim3((unsigned)n_units), dim3(256), 0,
                     (hipStream_t)stream, th, tw, d_in, d_off, d_rect, d_table);
  return idf_last_error();
}

// idf_deep_prep_host at `ways` states: 1 is the raster order, else the wavefront order
static int deep_prep_host(const uint16_t* unit, int32_t hin, int32_t win, int32_t ways,
                          int32_t* shift, uint32_t* sel, uint16_t minmax[2], int64_t* n_esc,
                          uint16_t* esc, uint32_t* low, float* x, float* mean, float* scale) {
  if (!unit || hin < 1 || win < 1 || !shift || !sel || !minmax || !n_esc || !esc || !low || !x ||
      !mean || !scale)
    return IDF_ERR_ARG;
  const DeepHostUnit u{unit, hin, win};
  const int64_t n = (int64_t)hin * win;
  uint64_t over[kDeepShiftMax] = {0};
  int mn = 0xffff, mx = 0;
  for (int64_t r = 0; r < n; ++r) {
    int v, pred, a, b, c;
    u.at(r / win, r % win, v, pred, a, b, c);
    const int d = v - pred;
    const uint32_t e = (uint32_t)(d < 0 ? -d : d);
    for (int s = 0; s < kDeepShiftMax; ++s) over[s] += e >= ((uint32_t)kDeepShiftFloor << s);
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  const int s = deep_shift(over, (uint64_t)n);
  uint64_t S[kPredictBuckets] = {0}, cnt[kPredictBuckets] = {0};
  for (int64_t r = 0; r < n; ++r) {
    const int64_t y = r / win, xx = r % win;
    int v, pred, a, b, c;
    u.at(y, xx, v, pred, a, b, c);
    const int kb = xx > 0 && y > 0 ? deep_bucket(a, b, c, s) : 0;
    S[kb] += deep_cost(v, pred, s);
    cnt[kb] += 1;
  }
  uint32_t sl = 0;
  for (int k = 0; k < kPredictBuckets; ++k) sl |= (uint32_t)predict_choose(S[k], cnt[k]) << (4 * k);
  const int64_t nl = deep_low_words(n, s);
  for (int64_t j = 0; j < nl; ++j) low[j] = 0;
  int64_t ne = 0;
  const std::vector<int64_t> perm = deep_order(hin, win, ways);  // perm[q]: the pixel of rank q
  for (int64_t q = 0; q < n; ++q) {
    const int64_t r = perm[q];
    const int64_t y = r / win, xx = r % win;
    int v, pred, a, b, c;
    u.at(y, xx, v, pred, a, b, c);
    const int kb = xx > 0 && y > 0 ? deep_bucket(a, b, c, s) : 0;
    bool is_esc;
    const int qc = deep_high(v, pred, s, is_esc);
    if (is_esc) esc[ne++] = (uint16_t)v;
    const int64_t i = n - 1 - q;
    x[i] = deep_x(qc);
    mean[i] = deep_mean(pred, s);
    scale[i] = predict_scale((int)(sl >> (4 * kb)) & 15);
    if (s > 0) {
      const uint64_t f = (uint64_t)((uint32_t)v & ((1u << s) - 1u)) << ((r * s) & 31);
      const int64_t wi = (r * s) >> 5;
      low[wi] |= (uint32_t)f;
      if (f >> 32) low[wi + 1] |= (uint32_t)(f >> 32);
    }
  }
  *shift = s, *sel = sl, *n_esc = ne;
  minmax[0] = (uint16_t)mn, minmax[1] = (uint16_t)mx;
  return IDF_OK;
}

int idf_deep_prep_host(const uint16_t* unit, int32_t hin, int32_t win, int32_t* shift,
                       uint32_t* sel, uint16_t minmax[2], int64_t* n_esc, uint16_t* esc,
                       uint32_t* low, float* x, float* mean, float* scale) {
  return deep_prep_host(unit, hin, win, 1, shift, sel, minmax, n_esc, esc, low, x, mean, scale);
}

int idf_deep_decode_host(int32_t hin, int32_t win, int32_t shift, uint32_t sel, uint64_t state,
                         const uint32_t* words, int64_t nwords, const uint32_t* low,
                         const uint16_t* esc, int64_t n_esc, uint16_t* out, uint64_t* final_state,
                         int32_t* status) {
  if (hin < 1 || win < 1 || nwords < 0 || n_esc < 0 || !out || !final_state || !status ||
      (nwords > 0 && !words) || (n_esc > 0 && !esc))
    return IDF_ERR_ARG;
  const int64_t n = (int64_t)hin * win;
  int32_t flag = 0;
  int s = shift;
  if (s < 0 || s > kDeepShiftMax) {
    s = kDeepShiftMax;
    flag |= IDF_STREAM_OUT_OF_WINDOW;
  }
  if (s > 0 && !low) return IDF_ERR_ARG;
  for (int64_t r = 0; r < n; ++r) out[r] = 0;
  const DeepHostUnit u{out, hin, win};
  int64_t pos = nwords, ei = 0;
  for (int64_t r = 0; r < n; ++r) {
    if ((state >> 32) == 0) {
      if (pos <= 0) {
        flag |= IDF_STREAM_UNDERFLOW;
        break;
      }
      state = (state << 32) | words[--pos];
    }
    const int64_t y = r / win, xx = r % win;
    int pq, v;
    const int qv = deep_host_symbol(u, y, xx, s, sel, state, pq, flag);
    const int dq = qv - pq;
    if (dq == kDeepEscape || dq == -kDeepEscape) {
      if (ei >= n_esc) {
        flag |= IDF_STREAM_UNDERFLOW;
        break;
      }
      v = esc[ei++];
    } else {
      v = deep_host_sample(qv, r, n, s, low, flag);
    }
    out[r] = (uint16_t)v;
  }
  *final_state = state;
  *status = flag | (pos > 0 || ei < n_esc ? IDF_STREAM_WORDS_LEFT : 0);
  return IDF_OK;
}

// ---- interleaved states: the wavefront order and its calls

int idf_deep_ways_supported(int32_t th, int32_t tw, int32_t ways) {
  if (th < 1 || tw < 1 || !deep_ways_ok(ways)) return IDF_ERR_ARG;
  return deep_ways_lds_bytes(th, tw) ? IDF_OK : IDF_ERR_UNSUPPORTED;
}

int idf_deep_prep_ways_u16(void* stream, int64_t n_units, int32_t th, int32_t tw,
                           const int64_t* d_table, const int64_t* h_table,
                           const int64_t* d_sym_off, const int64_t* d_low_off,
                           const int64_t* d_esc_off, float* d_x, float* d_mean, float* d_scale,
                           uint32_t* d_low, uint32_t* d_esc, uint16_t* d_minmax, uint8_t* d_shift,
                           uint32_t* d_sel, int64_t* d_nesc, int32_t ways) {
  const int rc = deep_launch_shape(n_units, th, tw);
  if (rc != IDF_OK) return rc;
  if (!deep_ways_ok(ways)) return IDF_ERR_ARG;
  if (n_units == 0) return IDF_OK;
  if (!d_table || !d_sym_off || !d_low_off || !d_esc_off || !d_x || !d_mean || !d_scale ||
      !d_low || !d_esc || !d_minmax || !d_shift || !d_sel || !d_nesc)
    return IDF_ERR_ARG;
  if (deep_check_rows(h_table, n_units) != IDF_OK) return IDF_ERR_ARG;
  hipLaunchKernelGGL(deep_prep_kernel<true>, dim3((unsigned)n_units), dim3(256), 0,
                     (hipStream_t)stream, th, tw, d_table, d_sym_off, d_low_off, d_esc_off, d_x,
                     d_mean, d_scale, d_low, d_esc, d_minmax, d_shift, d_sel, d_nesc, ways);
  return idf_last_error();
}

int idf_deep_decode_ways_u16(void* stream, int64_t n_units, int32_t ways, int32_t th, int32_t tw,
                             const uint8_t* d_class, const uint16_t* d_value,
                             const uint8_t* d_shift, const uint32_t* d_sel,
                             const uint64_t* d_state, const uint32_t* d_words,
                             const int64_t* d_word_off, const int64_t* d_nwords,
                             const uint32_t* d_low, const int64_t* d_low_off,
                             const uint32_t* d_esc, const int64_t* d_esc_off,
                             const int64_t* d_nesc, const int32_t* d_rect,
                             const int64_t* d_out_off, uint16_t* d_out, uint64_t* d_final_state,
                             int32_t* d_status) {
  const int rc = deep_launch_shape(n_units, th, tw);
  if (rc != IDF_OK) return rc;
  if (!deep_ways_ok(ways)) return IDF_ERR_ARG;
  if (n_units == 0) return IDF_OK;
  if (!d_class || !d_value || !d_shift || !d_sel || !d_state || !d_words || !d_word_off ||
      !d_nwords || !d_low || !d_low_off || !d_esc || !d_esc_off || !d_nesc || !d_rect ||
      !d_out_off || !d_out || !d_final_state || !d_status)
    return IDF_ERR_ARG;
  const size_t lds_bytes = deep_ways_lds_bytes(th, tw);
  if (!lds_bytes) return IDF_ERR_UNSUPPORTED;
#define IDF_DEEP_DECODE_WAYS(N)                                                                  \
  hipLaunchKernelGGL(deep_decode_ways_kernel<N>, dim3((unsigned)n_units), dim3(64), lds_bytes,   \
                     (hipStream_t)stream, n_units, th, tw, d_class, d_value, d_shift, d_sel,     \
                     d_state, d_words, d_word_off, d_nwords, d_low, d_low_off, d_esc, d_esc_off, \
                     d_nesc, d_rect, d_out_off, d_out, d_final_state, d_status)
  switch (ways) {
    case 8: IDF_DEEP_DECODE_WAYS(8); break;
    case 16: IDF_DEEP_DECODE_WAYS(16); break;
    case 32: IDF_DEEP_DECODE_WAYS(32); break;
    default: IDF_DEEP_DECODE_WAYS(64); break;
  }
#undef IDF_DEEP_DECODE_WAYS
  return idf_last_error();
}

int idf_deep_prep_ways_host(const uint16_t* unit, int32_t hin, int32_t win, int32_t ways,
                            int32_t* shift, uint32_t* sel, uint16_t minmax[2], int64_t* n_esc,
                            uint16_t* esc, uint32_t* low, float* x, float* mean, float* scale) {
  if (!deep_ways_ok(ways)) return IDF_ERR_ARG;
  return deep_prep_host(unit, hin, win, ways, shift, sel, minmax, n_esc, esc, low, x, mean, scale);
}

int idf_deep_decode_ways_host(int32_t hin, int32_t win, int32_t ways, int32_t shift, uint32_t sel,
                              const uint64_t* states, const uint32_t* words, int64_t nwords,
                              const uint32_t* low, const uint16_t* esc, int64_t n_esc,
                              uint16_t* out, uint64_t* final_states, int32_t* status) {
  if (hin < 1 || win < 1 || !deep_ways_ok(ways) || nwords < 0 || n_esc < 0 || !states || !out ||
      !final_states || !status || (nwords > 0 && !words) || (n_esc > 0 && !esc))
    return IDF_ERR_ARG;
  const int64_t n = (int64_t)hin * win;
  int32_t flag = 0;
  int s = shift;
  if (s < 0 || s > kDeepShiftMax) {
    s = kDeepShiftMax;
    flag |= IDF_STREAM_OUT_OF_WINDOW;
  }
  if (s > 0 && !low) return IDF_ERR_ARG;
  for (int64_t r = 0; r < n; ++r) out[r] = 0;
  const DeepHostUnit u{out, hin, win};
  const std::vector<int64_t> perm = deep_order(hin, win, ways);
  std::vector<uint64_t> S(states, states + ways), S2(ways);
  std::vector<int> vals(ways);  // the step's samples; -1: escaped
  int64_t pos = nwords, ei = 0;
  for (int64_t q0 = 0; q0 < n;) {
    // the step: pixels q0 .. q1 - 1
    auto step_of = [&](int64_t q) {
      int64_t t;
      int j;
      predict_step_slot(perm[q] / win, perm[q] % win, win, ways, t, j);
      return t;
    };
    const int64_t t0 = step_of(q0);
    int64_t q1 = q0 + 1;
    while (q1 < n && step_of(q1) == t0) ++q1;
    int64_t need = 0;
    for (int64_t q = q0; q < q1; ++q) need += (S[(n - 1 - q) % ways] >> 32) == 0;
    if (need > pos) {
      flag |= IDF_STREAM_UNDERFLOW;
      break;
    }
    S2 = S;
    int64_t pos2 = pos, n_step_esc = 0;
    int32_t flag2 = 0;
    for (int64_t q = q0; q < q1; ++q) {
      uint64_t& st = S2[(n - 1 - q) % ways];
      if ((st >> 32) == 0) st = (st << 32) | words[--pos2];  // rans.pyx:86-89, in pixel order
      const int64_t r = perm[q];
      int pq;
      const int qv = deep_host_symbol(u, r / win, r % win, s, sel, st, pq, flag2);
      const int dq = qv - pq;
      if (dq == kDeepEscape || dq == -kDeepEscape) {
        vals[q - q0] = -1;
        ++n_step_esc;
      } else {
        vals[q - q0] = deep_host_sample(qv, r, n, s, low, flag2);
      }
    }
    if (ei + n_step_esc > n_esc) {  // nothing of the step is kept
      flag |= IDF_STREAM_UNDERFLOW;
      break;
    }
    S = S2, pos = pos2, flag |= flag2;
    for (int64_t q = q0; q < q1; ++q)
      out[perm[q]] = (uint16_t)(vals[q - q0] < 0 ? (int)esc[ei++] : vals[q - q0]);
    q0 = q1;
  }
  for (int j = 0; j < ways; ++j) final_states[j] = S[j];
  *status = flag | (pos > 0 || ei < n_esc ? IDF_STREAM_WORDS_LEFT : 0);
  return IDF_OK;
}

}  // extern "C"
