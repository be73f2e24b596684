// CRC-32 (zlib's) of byte runs and of tiles on the device (idfcodec/integrity.py): the seal of
// the tiled containers.  The arithmetic is idf_crc.h's; its header states the identity.
//
// One block step covers a chunk of CRC_CHUNK = 4096 message bytes: thread q takes the 16-byte
// slice that ends (255 - q) slices before the chunk's end (the first slice of a short chunk is
// the short one, so every slice's distance to the chunk's end is a multiple of 16), runs the
// byte loop over an LDS copy of the byte table, and the 256 raw values are folded by a tree
// whose level l multiplies the left half by the constant x^(8 * 16 * 2^l).  One thread then
// multiplies the chunk's value by x^(8 * (bytes behind the chunk)) and XORs it into the output
// with one vector atomic.  An init launch first sets every output to the frame term
// 0xFFFFFFFF (x) x^(8 n) ^ 0xFFFFFFFF (0 for n = 0), so a call overwrites its outputs; XOR
// commutes, so the value does not depend on the grid or on the order the blocks run in.
//
// These are byte-stream kernels at launch-latency scale: plain byte loads, no vector path.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idf_codec_internal.h"
#include "idf_crc.h"
#include "idf_tile_row.h"

namespace idf {

constexpr int CRC_THREADS = 256;
constexpr int CRC_SLICE = 16;                        // bytes per thread and chunk
constexpr int CRC_CHUNK = CRC_THREADS * CRC_SLICE;   // bytes per block step
constexpr int CRC_CMAX = 4;
constexpr int CRC_TILE_PX = 1024;                    // tile_kernels.hip's band, for its limits

template <int L>
struct CrcStep {  // x^(8 * CRC_SLICE * 2^L)
  static constexpr uint32_t v = crc32_xpow8((uint64_t)CRC_SLICE << L);
};

template <int L>
__device__ __forceinline__ uint32_t crc_fold_levels(uint32_t* v) {
  constexpr int s = 1 << L;
  const int i = threadIdx.x;
  uint32_t node = 0;
  if (i < (CRC_THREADS >> (L + 1))) {  // node i of this level ends at position (i + 1) * 2s - 1
    const int t = (i + 1) * 2 * s - 1;
    node = crc32_mul(v[t - s], CrcStep<L>::v) ^ v[t];
    v[t] = node;
  }
  __syncthreads();
  if constexpr (L + 1 < 8) return crc_fold_levels<L + 1>(v);
  return node;  // thread 0 holds the chunk's value
}

// r: raw0 of thread q's slice, the slices right-aligned (slice 255 ends the chunk, absent slices
// are 0).  -> in thread 0, raw0 of the chunk.  v: 256 words of LDS, free again on return.
__device__ __forceinline__ uint32_t crc_fold(uint32_t r, uint32_t* v) {
  v[threadIdx.x] = r;
  __syncthreads();
  return crc_fold_levels<0>(v);
}

// the slice of thread q in a chunk [begin, end): bytes [lo, hi), empty when hi <= begin
__device__ __forceinline__ void crc_slice(int64_t begin, int64_t end, int64_t* lo, int64_t* hi) {
  *hi = end - (int64_t)(CRC_THREADS - 1 - (int)threadIdx.x) * CRC_SLICE;
  *lo = *hi - CRC_SLICE < begin ? begin : *hi - CRC_SLICE;
}

__device__ __forceinline__ void crc_stage_table(uint32_t* tab) {
  tab[threadIdx.x] = crc32_table_entry(threadIdx.x);
  __syncthreads();
}

// ---- byte runs: table int64 [n][2] of (address, n_bytes)
__global__ void __launch_bounds__(256)
crc_segments_init_kernel(int64_t n, const int64_t* __restrict__ table, uint32_t* __restrict__ crc) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t nb = table[2 * k + 1];
  crc[k] = crc32_frame(nb > 0 ? (uint64_t)nb : 0);
}

// block (k, y): chunks y, y + gridDim.y, ... of run k
__global__ void __launch_bounds__(CRC_THREADS)
crc_segments_kernel(const int64_t* __restrict__ table, uint32_t* __restrict__ crc) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t v[CRC_THREADS];
  const int64_t k = blockIdx.x;
  const uint8_t* p = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(table[2 * k]));
  const int64_t nb = table[2 * k + 1];
  const int64_t nchunks = nb > 0 ? (nb + CRC_CHUNK - 1) / CRC_CHUNK : 0;
  if ((int64_t)blockIdx.y >= nchunks) return;
  crc_stage_table(tab);
  uint32_t acc = 0;
  for (int64_t c = blockIdx.y; c < nchunks; c += gridDim.y) {
    const int64_t begin = c * CRC_CHUNK;
    const int64_t end = begin + CRC_CHUNK < nb ? begin + CRC_CHUNK : nb;
    int64_t lo, hi;
    crc_slice(begin, end, &lo, &hi);
    uint32_t r = 0;
    for (int64_t i = lo; i < hi; ++i) r = crc32_byte(tab, r, p[i]);
    r = crc_fold(r, v);
    if (threadIdx.x == 0) acc ^= crc32_mul(r, crc32_xpow8((uint64_t)(nb - end)));
  }
  if (threadIdx.x == 0) atomicXor(crc + k, acc);
}

// ---- tiles: the in-image rectangle as bytes [C][hin][win]
struct CrcRect {
  int64_t hin, win;
  __device__ int64_t bytes(int C) const { return (int64_t)C * hin * win; }
};

// the in-image part of the tile a table row names; empty when its origin lies outside the image
template <int F>
__device__ __forceinline__ CrcRect crc_row_rect(const TileRow<F>& r, int th, int tw) {
  if (!r.inside(r.y0, r.x0)) return {0, 0};
  return {r.H - r.y0 < th ? r.H - r.y0 : th, r.W - r.x0 < tw ? r.W - r.x0 : tw};
}

// the stored rectangle of tile t, held inside the tile
__device__ __forceinline__ CrcRect crc_given_rect(const int32_t* rect, int64_t t, int th, int tw) {
  const int64_t h = rect[2 * t], w = rect[2 * t + 1];
  if (h < 1 || w < 1) return {0, 0};
  return {h < th ? h : th, w < tw ? w : tw};
}

// F: the tile table's format (idf_tile_row.h); it is read only where rect is null
template <int F>
__global__ void __launch_bounds__(256)
crc_tile_init_kernel(int64_t n, int C, int th, int tw, const int64_t* __restrict__ table,
                     const int32_t* __restrict__ rect, uint32_t* __restrict__ crc) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const CrcRect rc = rect ? crc_given_rect(rect, t, th, tw)
                          : crc_row_rect(tile_row<F>(table, t), th, tw);
  crc[t] = crc32_frame((uint64_t)rc.bytes(C));
}

// idf_tile_scatter_u8's byte for a value of the pixel-major tile rows: idf_quant_u8's rule, a
// value off the grid or outside 0..256 clamped as the scatter clamps it (NaN gives 255)
__device__ __forceinline__ uint8_t crc_quant_u8(float val) {
  const float s = val * 256.0f;
  const float m = __builtin_rintf(s);
  const bool in_range = m >= 0.0f && m <= 256.0f;
  const int mi = in_range ? (int)m : (m < 0.0f ? -1 : 257);
  const int k = mi >= 129 ? mi - 1 : mi;
  return (uint8_t)(k < 0 ? 0 : (k > 255 ? 255 : k));
}

// block (t, c): chunk c of tile t's byte stream.  PM: the bytes are quantised from the
// pixel-major f32 rows `in` (ld floats per pixel); else read from the uint8 image the row of a
// table of format F names.
template <bool PM, int F>
__global__ void __launch_bounds__(CRC_THREADS)
crc_tile_kernel(int C, int th, int tw, const int64_t* __restrict__ table,
                const float* __restrict__ in, int64_t ld, const int32_t* __restrict__ rect,
                uint32_t* __restrict__ crc) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t v[CRC_THREADS];
  const int64_t t = blockIdx.x;
  TileRow<F> row = {};
  if (!PM) row = tile_row<F>(table, t);
  const CrcRect rc = PM ? crc_given_rect(rect, t, th, tw) : crc_row_rect(row, th, tw);
  const int64_t nb = rc.bytes(C);
  const int64_t begin = (int64_t)blockIdx.y * CRC_CHUNK;
  if (begin >= nb) return;
  crc_stage_table(tab);
  const int64_t end = begin + CRC_CHUNK < nb ? begin + CRC_CHUNK : nb;
  int64_t lo, hi;
  crc_slice(begin, end, &lo, &hi);
  uint32_t r = 0;
  if (lo < hi) {
    const int64_t plane = rc.hin * rc.win;
    int64_t ch = lo / plane, y = (lo % plane) / rc.win, x = lo % rc.win;
    const float* px = PM ? in + t * ((int64_t)th * tw) * ld : nullptr;
    for (int64_t i = lo; i < hi; ++i) {
      const uint8_t b = PM ? crc_quant_u8(px[(y * tw + x) * ld + ch])
                           : row.base[row.at(ch, row.y0 + y, row.x0 + x)];
      r = crc32_byte(tab, r, b);
      if (++x == rc.win) {
        x = 0;
        if (++y == rc.hin) y = 0, ++ch;
      }
    }
  }
  r = crc_fold(r, v);
  if (threadIdx.x == 0) atomicXor(crc + t, crc32_mul(r, crc32_xpow8((uint64_t)(nb - end))));
}

// the tile kernels' argument rules (tile_kernels.hip tile_launch_shape), and the chunks a tile's
// byte stream can have
static int crc_tile_shape(int64_t n_tiles, int32_t C, int32_t th, int32_t tw, int64_t ld,
                          int64_t* chunks) {
  if (n_tiles < 0 || C < 1 || C > CRC_CMAX || th < 1 || tw < 1 || ld < C) return IDF_ERR_ARG;
  if (n_tiles > 0x7fffffff) return IDF_ERR_ARG;
  if (((int64_t)th * tw + CRC_TILE_PX - 1) / CRC_TILE_PX > 65535) return IDF_ERR_UNSUPPORTED;
  *chunks = ((int64_t)C * th * tw + CRC_CHUNK - 1) / CRC_CHUNK;  // <= 65535 for C <= 4
  return IDF_OK;
}

static unsigned crc_init_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// idf_tile_crc32_u8 over a table of format F
template <int F>
static int crc_tile_source(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                           const int64_t* d_table, uint32_t* d_crc) {
  int64_t chunks = 0;
  const int rc = crc_tile_shape(n_tiles, C, th, tw, C, &chunks);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_crc) return IDF_ERR_ARG;
  hipLaunchKernelGGL(crc_tile_init_kernel<F>, dim3(crc_init_blocks(n_tiles)), dim3(256), 0,
                     (hipStream_t)stream, n_tiles, C, th, tw, d_table, (const int32_t*)nullptr,
                     d_crc);
  hipLaunchKernelGGL((crc_tile_kernel<false, F>), dim3((unsigned)n_tiles, (unsigned)chunks),
                     dim3(CRC_THREADS), 0, (hipStream_t)stream, C, th, tw, d_table,
                     (const float*)nullptr, (int64_t)0, (const int32_t*)nullptr, d_crc);
  return idf_last_error();
}

}  // namespace idf

using namespace idf;

extern "C" {

uint32_t idf_crc32_host(const void* p, int64_t n) { return crc32_bytes(p, n); }

uint32_t idf_crc32_combine(uint32_t crc_a, uint32_t crc_b, int64_t len_b) {
  return crc32_combine(crc_a, crc_b, len_b > 0 ? (uint64_t)len_b : 0);
}

int idf_crc32_segments_u8(void* stream, int64_t n, const int64_t* d_table, uint32_t* d_crc) {
  if (n < 0 || n > 0x7fffffff) return IDF_ERR_ARG;
  if (n == 0) return IDF_OK;
  if (!d_table || !d_crc) return IDF_ERR_ARG;
  // about 16384 blocks in all: one long run is spread over 4096 of them, many runs take a few
  // lanes each; a block with no chunk of its own returns at once
  int64_t lanes = 16384 / n;
  lanes = lanes < 1 ? 1 : (lanes > 4096 ? 4096 : lanes);
  hipLaunchKernelGGL(crc_segments_init_kernel, dim3(crc_init_blocks(n)), dim3(256), 0,
                     (hipStream_t)stream, n, d_table, d_crc);
  hipLaunchKernelGGL(crc_segments_kernel, dim3((unsigned)n, (unsigned)lanes), dim3(CRC_THREADS),
                     0, (hipStream_t)stream, d_table, d_crc);
  return idf_last_error();
}

int idf_tile_crc32_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                      const int64_t* d_table, uint32_t* d_crc) {
  return crc_tile_source<TILE_FIELDS>(stream, n_tiles, C, th, tw, d_table, d_crc);
}

int idf_tile_crc32_strided_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                              const int64_t* d_table, uint32_t* d_crc) {
  return crc_tile_source<TILE_FIELDS_STRIDED>(stream, n_tiles, C, th, tw, d_table, d_crc);
}

int idf_tile_crc32_pm(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                      const float* d_in, int64_t ld_in, const int32_t* d_rect, uint32_t* d_crc) {
  int64_t chunks = 0;
  const int rc = crc_tile_shape(n_tiles, C, th, tw, ld_in, &chunks);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_in || !d_rect || !d_crc) return IDF_ERR_ARG;
  hipLaunchKernelGGL(crc_tile_init_kernel<TILE_FIELDS>, dim3(crc_init_blocks(n_tiles)),
                     dim3(256), 0, (hipStream_t)stream, n_tiles, C, th, tw, (const int64_t*)nullptr, d_rect,
                     d_crc);
  hipLaunchKernelGGL((crc_tile_kernel<true, TILE_FIELDS>),
                     dim3((unsigned)n_tiles, (unsigned)chunks), dim3(CRC_THREADS), 0, (hipStream_t)stream, C, th, tw,
                     (const int64_t*)nullptr, d_in, ld_in, d_rect, d_crc);
  return idf_last_error();
}

}  // extern "C"
