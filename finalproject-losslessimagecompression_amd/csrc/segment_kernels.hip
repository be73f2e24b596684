// Byte runs of one buffer, a run per wave (idfcodec/planes.py): the smallest and largest byte of
// each run, which tells a constant plane of a tile from one worth coding, and the fill that
// writes such a plane back.
//
// A run [begin, end) of any alignment is cut in three: the head, the bytes in front of the first
// 16-byte boundary (at most 15, one a lane); the middle, whole aligned 16-byte vectors, lane l
// taking vectors l, l + 64, ...; the tail, the bytes behind the last whole vector (at most 15,
// one a lane).  A run shorter than its head is all head.  No lane touches a byte outside the
// run, so a run may end at the last byte of an allocation.  The range is folded across the wave
// by shuffles alone: no LDS, no barrier, and the waves of a block share nothing.
//
// Both kernels are memory-bound single passes: plain vector loads and stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idf_codec_internal.h"

namespace idf {

constexpr int SEG_WAVE = 64;
constexpr int SEG_WAVES = 4;                        // runs per block
constexpr int SEG_THREADS = SEG_WAVE * SEG_WAVES;
constexpr int SEG_VEC = 16;                         // bytes per vector access

// the three parts of a run of len > 0 bytes at address a
struct SegParts {
  int64_t head, nvec, tail;
};

__device__ __forceinline__ SegParts seg_parts(uintptr_t a, int64_t len) {
  int64_t head = (int64_t)((SEG_VEC - (a & (SEG_VEC - 1))) & (SEG_VEC - 1));
  head = head < len ? head : len;
  const int64_t nvec = (len - head) / SEG_VEC;
  return {head, nvec, len - head - nvec * SEG_VEC};
}

__device__ __forceinline__ void seg_fold_byte(uint32_t b, uint32_t* mn, uint32_t* mx) {
  *mn = b < *mn ? b : *mn;
  *mx = b > *mx ? b : *mx;
}

__device__ __forceinline__ void seg_fold_word(uint32_t w, uint32_t* mn, uint32_t* mx) {
#pragma unroll
  for (int i = 0; i < 4; ++i) seg_fold_byte((w >> (8 * i)) & 0xffu, mn, mx);
}

// wave w of block b: run k = b * SEG_WAVES + w of src, (min, max) to minmax[k]
__global__ void __launch_bounds__(SEG_THREADS)
segment_range_u8_kernel(int64_t n, const int64_t* __restrict__ off,
                        const uint8_t* __restrict__ src, uint8_t* __restrict__ minmax) {
  const int lane = threadIdx.x & (SEG_WAVE - 1);
  const int64_t k = (int64_t)blockIdx.x * SEG_WAVES + (threadIdx.x / SEG_WAVE);
  if (k >= n) return;  // the whole wave
  const int64_t begin = off[k], end = off[k + 1];
  uint32_t mn = 255u, mx = 0u;  // an empty run's
  if (end > begin) {
    const uint8_t* p = src + begin;
    const SegParts s = seg_parts(reinterpret_cast<uintptr_t>(p), end - begin);
    if (lane < s.head) seg_fold_byte(p[lane], &mn, &mx);
    const uint4* v = reinterpret_cast<const uint4*>(p + s.head);
    for (int64_t i = lane; i < s.nvec; i += SEG_WAVE) {
      const uint4 q = v[i];
      seg_fold_word(q.x, &mn, &mx);
      seg_fold_word(q.y, &mn, &mx);
      seg_fold_word(q.z, &mn, &mx);
      seg_fold_word(q.w, &mn, &mx);
    }
    const uint8_t* t = p + s.head + s.nvec * SEG_VEC;
    if (lane < s.tail) seg_fold_byte(t[lane], &mn, &mx);
  }
#pragma unroll
  for (int d = SEG_WAVE / 2; d > 0; d >>= 1) {
    const uint32_t a = (uint32_t)__shfl_xor((int)mn, d, SEG_WAVE);
    const uint32_t b = (uint32_t)__shfl_xor((int)mx, d, SEG_WAVE);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if (lane == 0) {
    minmax[2 * k] = (uint8_t)mn;
    minmax[2 * k + 1] = (uint8_t)mx;
  }
}

// wave w of block b: len[k] copies of value[k] at dst + off[k], k = b * SEG_WAVES + w
__global__ void __launch_bounds__(SEG_THREADS)
segment_fill_u8_kernel(int64_t n, const int64_t* __restrict__ off,
                       const int64_t* __restrict__ len, const uint8_t* __restrict__ value,
                       uint8_t* __restrict__ dst) {
  const int lane = threadIdx.x & (SEG_WAVE - 1);
  const int64_t k = (int64_t)blockIdx.x * SEG_WAVES + (threadIdx.x / SEG_WAVE);
  if (k >= n) return;
  const int64_t nb = len[k];
  if (nb <= 0) return;
  uint8_t* p = dst + off[k];
  const uint8_t b = value[k];
  const uint32_t w = 0x01010101u * b;
  const SegParts s = seg_parts(reinterpret_cast<uintptr_t>(p), nb);
  if (lane < s.head) p[lane] = b;
  uint4* v = reinterpret_cast<uint4*>(p + s.head);
  for (int64_t i = lane; i < s.nvec; i += SEG_WAVE) v[i] = make_uint4(w, w, w, w);
  uint8_t* t = p + s.head + s.nvec * SEG_VEC;
  if (lane < s.tail) t[lane] = b;
}

static unsigned seg_blocks(int64_t n) { return (unsigned)((n + SEG_WAVES - 1) / SEG_WAVES); }

}  // namespace idf

using namespace idf;

extern "C" {

int idf_segment_range_u8(void* stream, int64_t n, const int64_t* d_off, const uint8_t* d_src,
                         uint8_t* d_minmax) {
  if (n < 0 || n > 0x7fffffff) return IDF_ERR_ARG;
  if (n == 0) return IDF_OK;
  if (!d_off || !d_src || !d_minmax) return IDF_ERR_ARG;
  hipLaunchKernelGGL(segment_range_u8_kernel, dim3(seg_blocks(n)), dim3(SEG_THREADS), 0,
                     (hipStream_t)stream, n, d_off, d_src, d_minmax);
  return idf_last_error();
}

int idf_segment_fill_u8(void* stream, int64_t n, const int64_t* d_off, const int64_t* d_len,
                        const uint8_t* d_value, uint8_t* d_dst) {
  if (n < 0 || n > 0x7fffffff) return IDF_ERR_ARG;
  if (n == 0) return IDF_OK;
  if (!d_off || !d_len || !d_value || !d_dst) return IDF_ERR_ARG;
  hipLaunchKernelGGL(segment_fill_u8_kernel, dim3(seg_blocks(n)), dim3(SEG_THREADS), 0,
                     (hipStream_t)stream, n, d_off, d_len, d_value, d_dst);
  return idf_last_error();
}

}  // extern "C"
