// TwoLevelFlows plumbing (flows.py:209-216, 267-269 of the reference): replication pad,
// average pool to the rough image, residual against the replicated rough image, Patching
// of the residual -- and the inverse -- as two index kernels between an NCHW image and the
// pixel-major (ld 4) input buffers of the rough and the fine FlowEngine.
//
// All arithmetic is in integers on the 1/256 grid: k' = k + [k >= 128] is the dequantised
// byte times 256 (idf_dequant_u8), a window of n = wh * ww padded pixels sums to S (int32, so
// the sum does not depend on its order or on the launch shape), and the rough value is
// q = round_half_even(S / n).  rough = q / 256 and residual = (k' - q) / 256 are exact floats.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idf_codec_internal.h"

namespace idf {

// floor division and round-half-even of s / n (n > 0), s of either sign
__device__ __forceinline__ int round_half_even_div(int s, int n) {
  int q = s / n;
  int r = s - q * n;
  if (r < 0) {
    r += n;
    q -= 1;
  }
  if (2 * r > n || (2 * r == n && (q & 1))) q += 1;
  return q;
}

// |k'| limit for f32 input: keeps every window sum (n <= 2^10 here) inside int32 and the value
// exactly representable on the grid
constexpr int TL_KMAX = 1 << 20;

// One block per (image, rough row): the wh padded rows of that band, all channels.
//   pass 1: every padded element of the band is read once (coalesced along x, the pad by
//           clamped indices) into LDS as k';
//   pass 2: one thread per (channel, rough pixel) sums its window from LDS, rounds, writes the
//           rough value once;
//   pass 3: every element writes its residual at its place in Patching order
//           (image, patch row, patch column), channel fastest.
template <bool F32>
__global__ void __launch_bounds__(256)
twolevel_split_kernel(int C, int Hs, int Ws, int Hp, int Wp, int rh, int rw, int fh, int fw,
                      const void* __restrict__ src_, float* __restrict__ rough, int64_t ldr,
                      float* __restrict__ fine, int64_t ldf, int32_t* __restrict__ bad) {
  extern __shared__ int tl_lds[];
  const int wh = Hp / rh, ww = Wp / rw;
  const int band = wh * Wp;           // elements per channel in this block's band
  int* kv = tl_lds;                   // [C][wh][Wp]
  int* qv = tl_lds + C * band;        // [C][rw]
  const int64_t b = blockIdx.x / rh;
  const int ry = blockIdx.x % rh;
  const int n_el = C * band;
  int n_bad = 0;
  for (int e = threadIdx.x; e < n_el; e += blockDim.x) {
    const int c = e / band, r = e % band;
    const int y = ry * wh + r / Wp, x = r % Wp;
    const int ys = y < Hs ? y : Hs - 1, xs = x < Ws ? x : Ws - 1;
    const int64_t si = ((b * C + c) * Hs + ys) * (int64_t)Ws + xs;
    int k;
    if (F32) {
      const float v = static_cast<const float*>(src_)[si] * 256.0f;
      const float m = __builtin_rintf(v);
      const bool ok = (m == v) && m >= -(float)TL_KMAX && m <= (float)TL_KMAX;
      k = ok ? (int)m : 0;
      // a pad position repeats a source pixel: count each source pixel once
      if (!ok && y < Hs && x < Ws) ++n_bad;
    } else {
      k = static_cast<const uint8_t*>(src_)[si];
      k += k >= 128 ? 1 : 0;
    }
    kv[e] = k;
  }
  if (F32 && n_bad) atomicAdd(bad, n_bad);
  __syncthreads();
  const int n = wh * ww;
  for (int t = threadIdx.x; t < C * rw; t += blockDim.x) {
    const int c = t / rw, rx = t % rw;
    const int* w0 = kv + c * band + rx * ww;
    int s = 0;
    for (int i = 0; i < wh; ++i)
      for (int j = 0; j < ww; ++j) s += w0[i * Wp + j];
    const int q = round_half_even_div(s, n);
    qv[t] = q;
    rough[((b * rh + ry) * (int64_t)rw + rx) * ldr + c] = (float)q * (1.0f / 256.0f);
  }
  __syncthreads();
  const int npw = Wp / fw, nph = Hp / fh;
  for (int e = threadIdx.x; e < n_el; e += blockDim.x) {
    // channel fastest: neighbouring threads write neighbouring floats of a pixel row
    const int c = e % C, r = e / C;
    const int wy = r / Wp, x = r % Wp;
    const int y = ry * wh + wy;
    const int d = kv[c * band + wy * Wp + x] - qv[c * rw + x / ww];
    const int64_t patch = (b * nph + y / fh) * (int64_t)npw + x / fw;
    const int64_t pix = (patch * fh + y % fh) * (int64_t)fw + x % fw;
    fine[pix * ldf + c] = (float)d * (1.0f / 256.0f);
  }
}

// One thread per element of the source-size NCHW output: x = rough[y / wh, x / ww] + fine patch
// value; the pad is never written.  U8: quantised as quant_u8_kernel does (same off-grid rule).
template <bool U8>
__global__ void __launch_bounds__(256)
twolevel_merge_kernel(int64_t total, int C, int Hs, int Ws, int Hp, int Wp, int rh, int rw, int fh,
                      int fw, const float* __restrict__ rough, int64_t ldr,
                      const float* __restrict__ fine, int64_t ldf, void* __restrict__ out_,
                      int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int wh = Hp / rh, ww = Wp / rw;
  const int npw = Wp / fw, nph = Hp / fh;
  const int x = (int)(i % Ws);
  int64_t t = i / Ws;
  const int y = (int)(t % Hs);
  t /= Hs;
  const int c = (int)(t % C);
  const int64_t b = t / C;
  const float r = rough[((b * rh + y / wh) * (int64_t)rw + x / ww) * ldr + c];
  const int64_t patch = (b * nph + y / fh) * (int64_t)npw + x / fw;
  const int64_t pix = (patch * fh + y % fh) * (int64_t)fw + x % fw;
  const float v = r + fine[pix * ldf + c];
  if (!U8) {
    static_cast<float*>(out_)[i] = v;
    return;
  }
  const float s = v * 256.0f;
  const float m = __builtin_rintf(s);
  const bool in = m >= 0.0f && m <= 256.0f;
  int mi = in ? (int)m : (m < 0.0f ? -1 : 257);
  int k = mi >= 129 ? mi - 1 : mi;
  const bool ok = (m == s) && in && mi != 128;
  if (!ok) {
    atomicAdd(bad, 1);
    k = k < 0 ? 0 : (k > 255 ? 255 : k);
  }
  static_cast<uint8_t*>(out_)[i] = (uint8_t)k;
}

static bool twolevel_geometry_ok(int32_t B, int32_t C, int32_t Hs, int32_t Ws, int32_t Hp,
                                 int32_t Wp, int32_t rh, int32_t rw, int32_t fh, int32_t fw,
                                 int64_t ldr, int64_t ldf) {
  if (B < 0 || C <= 0 || Hs <= 0 || Ws <= 0 || Hp < Hs || Wp < Ws) return false;
  if (rh <= 0 || rw <= 0 || fh <= 0 || fw <= 0) return false;
  if (Hp % rh || Wp % rw || Hp % fh || Wp % fw) return false;
  if (ldr < C || ldf < C) return false;
  return true;
}

}  // namespace idf

using namespace idf;

extern "C" {

int idf_twolevel_split(void* stream, int32_t B, int32_t C, int32_t Hs, int32_t Ws, int32_t Hp,
                       int32_t Wp, int32_t rh, int32_t rw, int32_t fh, int32_t fw,
                       const uint8_t* d_src_u8, const float* d_src_f32, float* d_rough,
                       int64_t ld_rough, float* d_fine, int64_t ld_fine, int32_t* d_bad) {
  if (!twolevel_geometry_ok(B, C, Hs, Ws, Hp, Wp, rh, rw, fh, fw, ld_rough, ld_fine))
    return IDF_ERR_ARG;
  if ((d_src_u8 == nullptr) == (d_src_f32 == nullptr)) return IDF_ERR_ARG;  // exactly one
  if (B == 0) return IDF_OK;
  if (!d_rough || !d_fine || (d_src_f32 && !d_bad)) return IDF_ERR_ARG;
  const int64_t wh = Hp / rh, ww = Wp / rw;
  if (wh * ww > 1024) return IDF_ERR_UNSUPPORTED;  // int32 window sums (TL_KMAX * n < 2^31)
  const int64_t lds = ((int64_t)C * wh * Wp + (int64_t)C * rw) * (int64_t)sizeof(int);
  if (lds > 64 * 1024) return IDF_ERR_UNSUPPORTED;
  const int64_t blocks = (int64_t)B * rh;
  if (blocks > 0x7fffffff) return IDF_ERR_ARG;
  if (d_src_f32)
    hipLaunchKernelGGL(twolevel_split_kernel<true>, dim3((unsigned)blocks), dim3(256), (size_t)lds,
                       (hipStream_t)stream, C, Hs, Ws, Hp, Wp, rh, rw, fh, fw,
                       (const void*)d_src_f32, d_rough, ld_rough, d_fine, ld_fine, d_bad);
  else
    hipLaunchKernelGGL(twolevel_split_kernel<false>, dim3((unsigned)blocks), dim3(256),
                       (size_t)lds, (hipStream_t)stream, C, Hs, Ws, Hp, Wp, rh, rw, fh, fw,
                       (const void*)d_src_u8, d_rough, ld_rough, d_fine, ld_fine, d_bad);
  return idf_last_error();
}

int idf_twolevel_merge(void* stream, int32_t B, int32_t C, int32_t Hs, int32_t Ws, int32_t Hp,
                       int32_t Wp, int32_t rh, int32_t rw, int32_t fh, int32_t fw,
                       const float* d_rough, int64_t ld_rough, const float* d_fine,
                       int64_t ld_fine, uint8_t* d_out_u8, float* d_out_f32, int32_t* d_bad) {
  if (!twolevel_geometry_ok(B, C, Hs, Ws, Hp, Wp, rh, rw, fh, fw, ld_rough, ld_fine))
    return IDF_ERR_ARG;
  if ((d_out_u8 == nullptr) == (d_out_f32 == nullptr)) return IDF_ERR_ARG;  // exactly one
  if (B == 0) return IDF_OK;
  if (!d_rough || !d_fine || (d_out_u8 && !d_bad)) return IDF_ERR_ARG;
  const int64_t total = (int64_t)B * C * Hs * Ws;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return IDF_ERR_ARG;
  if (d_out_u8)
    hipLaunchKernelGGL(twolevel_merge_kernel<true>, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, total, C, Hs, Ws, Hp, Wp, rh, rw, fh, fw, d_rough,
                       ld_rough, d_fine, ld_fine, (void*)d_out_u8, d_bad);
  else
    hipLaunchKernelGGL(twolevel_merge_kernel<false>, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, total, C, Hs, Ws, Hp, Wp, rh, rw, fh, fw, d_rough,
                       ld_rough, d_fine, ld_fine, (void*)d_out_f32, d_bad);
  return idf_last_error();
}

}  // extern "C"
