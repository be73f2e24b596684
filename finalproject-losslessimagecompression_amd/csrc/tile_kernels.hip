// Images of any size as tiles of the flow's input (idfcodec/tiled.py): the gather from a ragged
// set of uint8 NCHW images to the pixel-major (ld 4) input of a FlowEngine, one batch entry per
// th x tw tile, and the scatter back.  The pad is the reference's ReplicationPad2d((0, pw, 0,
// ph)) (trainer.py:62) by clamped indexing, the tiles are Patching.forward's
// (extenddim.py:51-57); neither is materialised.
//
// Every kernel here reads a device table int64 [n_tiles][5] of rows (addr, H, W, y0, x0): addr is the
// device address of a contiguous uint8 [C, H, W] buffer, (y0, x0) the tile's origin in that
// buffer's coordinates.  Every index is 64-bit: a set of images may exceed 2^31 bytes.
//
// One block per (tile, run of TILE_PX consecutive tile pixels).  A run is staged through LDS so
// that the NCHW side is accessed along x by neighbouring threads of a channel and the
// pixel-major side channel-fastest, neighbouring threads on neighbouring floats of a pixel row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idf_codec_internal.h"

namespace idf {

constexpr int TILE_PX = 1024;    // tile pixels per block
constexpr int TILE_CMAX = 4;     // channels (the pixel rows of ws['img'] are 4 wide)
constexpr int TILE_FIELDS = 5;   // addr, H, W, y0, x0

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

__global__ void __launch_bounds__(256)
tile_gather_u8_kernel(int C, int th, int tw, const int64_t* __restrict__ table,
                      float* __restrict__ out, int64_t ld) {
  __shared__ float kv[TILE_CMAX * TILE_PX];  // [C][TILE_PX]
  const int64_t t = blockIdx.x;
  const int64_t* row = table + t * TILE_FIELDS;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(row[0]));
  const int64_t H = row[1], W = row[2], y0 = row[3], x0 = row[4];
  const int64_t npx = (int64_t)th * tw;
  const int64_t p0 = (int64_t)blockIdx.y * TILE_PX;
  const int n = (int)(npx - p0 < TILE_PX ? npx - p0 : TILE_PX);
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e / n, j = e % n;
    const int64_t p = p0 + j;
    const int64_t y = clamp_i64(y0 + p / tw, 0, H - 1), x = clamp_i64(x0 + p % tw, 0, W - 1);
    const int k = src[(c * H + y) * W + x];
    kv[c * TILE_PX + j] = (float)(k + (k >= 128 ? 1 : 0)) * (1.0f / 256.0f);
  }
  __syncthreads();
  float* dst = out + (t * npx + p0) * ld;
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e % C, j = e / C;
    dst[(int64_t)j * ld + c] = kv[c * TILE_PX + j];
  }
}

__global__ void __launch_bounds__(256)
tile_scatter_u8_kernel(int C, int th, int tw, const float* __restrict__ in, int64_t ld,
                       const int64_t* __restrict__ table, int32_t* __restrict__ bad) {
  __shared__ uint8_t kv[TILE_CMAX * TILE_PX];  // [C][TILE_PX]
  __shared__ int block_bad;
  const int64_t t = blockIdx.x;
  const int64_t* row = table + t * TILE_FIELDS;
  uint8_t* dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(row[0]));
  const int64_t H = row[1], W = row[2], y0 = row[3], x0 = row[4];
  const int64_t npx = (int64_t)th * tw;
  const int64_t p0 = (int64_t)blockIdx.y * TILE_PX;
  const int n = (int)(npx - p0 < TILE_PX ? npx - p0 : TILE_PX);
  if (threadIdx.x == 0) block_bad = 0;
  __syncthreads();
  const float* src = in + (t * npx + p0) * ld;
  int n_bad = 0;
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e % C, j = e / C;
    const int64_t p = p0 + j;
    const int64_t y = y0 + p / tw, x = x0 + p % tw;
    if (y < 0 || y >= H || x < 0 || x >= W) continue;  // the pad, or outside a crop
    // idf_quant_u8's rule
    const float s = src[(int64_t)j * ld + c] * 256.0f;
    const float m = __builtin_rintf(s);
    const bool in_range = m >= 0.0f && m <= 256.0f;
    const int mi = in_range ? (int)m : (m < 0.0f ? -1 : 257);
    int k = mi >= 129 ? mi - 1 : mi;
    if (!((m == s) && in_range && mi != 128)) {
      ++n_bad;
      k = k < 0 ? 0 : (k > 255 ? 255 : k);
    }
    kv[c * TILE_PX + j] = (uint8_t)k;
  }
  if (n_bad) atomicAdd(&block_bad, n_bad);
  __syncthreads();
  if (threadIdx.x == 0 && block_bad) atomicAdd(bad, block_bad);
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e / n, j = e % n;
    const int64_t p = p0 + j;
    const int64_t y = y0 + p / tw, x = x0 + p % tw;
    if (y < 0 || y >= H || x < 0 || x >= W) continue;
    dst[(c * H + y) * W + x] = kv[c * TILE_PX + j];
  }
}

// ---- the raw-tile escape (idfcodec/safe.py): a tile's in-image bytes stored as they are, and the
// decoded tiles compared with the source.  Same table, same grid; these are plain byte copies,
// one pass, neighbouring threads along x within a channel.

// The in-image rectangle of the tile, rows [y0, min(y0+th, H)) x columns [x0, min(x0+tw, W)), as
// contiguous uint8 [C][hin][win] at out + off[t].
__global__ void __launch_bounds__(256)
tile_gather_raw_u8_kernel(int C, int th, int tw, const int64_t* __restrict__ table,
                          const int64_t* __restrict__ off, uint8_t* __restrict__ out) {
  const int64_t t = blockIdx.x;
  const int64_t* row = table + t * TILE_FIELDS;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(row[0]));
  const int64_t H = row[1], W = row[2], y0 = row[3], x0 = row[4];
  if (y0 < 0 || x0 < 0 || y0 >= H || x0 >= W) return;  // no in-image part
  const int64_t hin = H - y0 < th ? H - y0 : th, win = W - x0 < tw ? W - x0 : tw;
  const int64_t npx = (int64_t)th * tw;
  const int64_t p0 = (int64_t)blockIdx.y * TILE_PX;
  const int n = (int)(npx - p0 < TILE_PX ? npx - p0 : TILE_PX);
  uint8_t* dst = out + off[t];
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e / n, j = e % n;
    const int64_t p = p0 + j;
    const int64_t r = p / tw, x = p % tw;
    if (r >= hin || x >= win) continue;  // the pad is not stored
    dst[(c * hin + r) * win + x] = src[(c * H + y0 + r) * W + x0 + x];
  }
}

// The inverse: byte (ch, r, c) of the stored [C][hin][win] rectangle of tile t (rect[t] = (hin,
// win)) to dst[ch*H*W + (y0+r)*W + (x0+c)], only inside [0,H) x [0,W).
__global__ void __launch_bounds__(256)
tile_scatter_raw_u8_kernel(int C, int th, int tw, const uint8_t* __restrict__ in,
                           const int64_t* __restrict__ off, const int32_t* __restrict__ rect,
                           const int64_t* __restrict__ table) {
  const int64_t t = blockIdx.x;
  const int64_t* row = table + t * TILE_FIELDS;
  uint8_t* dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(row[0]));
  const int64_t H = row[1], W = row[2], y0 = row[3], x0 = row[4];
  const int64_t hin = rect[2 * t], win = rect[2 * t + 1];
  const int64_t npx = (int64_t)th * tw;
  const int64_t p0 = (int64_t)blockIdx.y * TILE_PX;
  const int n = (int)(npx - p0 < TILE_PX ? npx - p0 : TILE_PX);
  const uint8_t* src = in + off[t];
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e / n, j = e % n;
    const int64_t p = p0 + j;
    const int64_t r = p / tw, xx = p % tw;
    if (r >= hin || xx >= win) continue;  // not stored
    const int64_t y = y0 + r, x = x0 + xx;
    if (y < 0 || y >= H || x < 0 || x >= W) continue;  // outside a crop
    dst[(c * H + y) * W + x] = src[(c * hin + r) * win + xx];
  }
}

// mismatch[t] += the (pixel, channel) pairs of tile t, over the tile pixels whose source position
// lies inside the image, whose value in the pixel-major tile buffer is not the dequantised source
// byte (idf_quant_u8's rule; a value off the grid is a mismatch).
__global__ void __launch_bounds__(256)
tile_verify_u8_kernel(int C, int th, int tw, const float* __restrict__ in, int64_t ld,
                      const int64_t* __restrict__ table, int32_t* __restrict__ mismatch) {
  __shared__ int part[256];
  const int64_t t = blockIdx.x;
  const int64_t* row = table + t * TILE_FIELDS;
  const uint8_t* ref = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(row[0]));
  const int64_t H = row[1], W = row[2], y0 = row[3], x0 = row[4];
  const int64_t npx = (int64_t)th * tw;
  const int64_t p0 = (int64_t)blockIdx.y * TILE_PX;
  const int n = (int)(npx - p0 < TILE_PX ? npx - p0 : TILE_PX);
  const float* src = in + (t * npx + p0) * ld;
  int n_bad = 0;
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e % C, j = e / C;
    const int64_t p = p0 + j;
    const int64_t y = y0 + p / tw, x = x0 + p % tw;
    if (y < 0 || y >= H || x < 0 || x >= W) continue;  // the pad is not compared
    // idf_quant_u8's rule
    const float s = src[(int64_t)j * ld + c] * 256.0f;
    const float m = __builtin_rintf(s);
    const bool in_range = m >= 0.0f && m <= 256.0f;
    const int mi = in_range ? (int)m : -1;
    const int k = mi >= 129 ? mi - 1 : mi;
    const bool on_grid = (m == s) && in_range && mi != 128;
    if (!on_grid || k != (int)ref[(c * H + y) * W + x]) ++n_bad;
  }
  part[threadIdx.x] = n_bad;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0 && part[0]) atomicAdd(mismatch + t, part[0]);
}

// IDF_OK with *bands set, or the error code of a bad launch shape
static int tile_launch_shape(int64_t n_tiles, int32_t C, int32_t th, int32_t tw, int64_t ld,
                             int64_t* bands) {
  if (n_tiles < 0 || C < 1 || C > TILE_CMAX || th < 1 || tw < 1 || ld < C) return IDF_ERR_ARG;
  if (n_tiles > 0x7fffffff) return IDF_ERR_ARG;
  *bands = ((int64_t)th * tw + TILE_PX - 1) / TILE_PX;
  if (*bands > 65535) return IDF_ERR_UNSUPPORTED;
  return IDF_OK;
}

}  // namespace idf

using namespace idf;

extern "C" {

int idf_tile_gather_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                       const int64_t* d_table, float* d_out, int64_t ld_out) {
  int64_t bands = 0;
  const int rc = tile_launch_shape(n_tiles, C, th, tw, ld_out, &bands);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_out) return IDF_ERR_ARG;
  hipLaunchKernelGGL(tile_gather_u8_kernel, dim3((unsigned)n_tiles, (unsigned)bands), dim3(256),
                     0, (hipStream_t)stream, C, th, tw, d_table, d_out, ld_out);
  return idf_last_error();
}

int idf_tile_scatter_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                        const float* d_in, int64_t ld_in, const int64_t* d_table,
                        int32_t* d_bad) {
  int64_t bands = 0;
  const int rc = tile_launch_shape(n_tiles, C, th, tw, ld_in, &bands);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_in || !d_bad) return IDF_ERR_ARG;
  hipLaunchKernelGGL(tile_scatter_u8_kernel, dim3((unsigned)n_tiles, (unsigned)bands), dim3(256),
                     0, (hipStream_t)stream, C, th, tw, d_in, ld_in, d_table, d_bad);
  return idf_last_error();
}

int idf_tile_gather_raw_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                           const int64_t* d_table, const int64_t* d_off, uint8_t* d_out) {
  int64_t bands = 0;
  const int rc = tile_launch_shape(n_tiles, C, th, tw, C, &bands);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_off || !d_out) return IDF_ERR_ARG;
  hipLaunchKernelGGL(tile_gather_raw_u8_kernel, dim3((unsigned)n_tiles, (unsigned)bands),
                     dim3(256), 0, (hipStream_t)stream, C, th, tw, d_table, d_off, d_out);
  return idf_last_error();
}

int idf_tile_scatter_raw_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                            const uint8_t* d_in, const int64_t* d_off, const int32_t* d_rect,
                            const int64_t* d_table) {
  int64_t bands = 0;
  const int rc = tile_launch_shape(n_tiles, C, th, tw, C, &bands);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_in || !d_off || !d_rect) return IDF_ERR_ARG;
  hipLaunchKernelGGL(tile_scatter_raw_u8_kernel, dim3((unsigned)n_tiles, (unsigned)bands),
                     dim3(256), 0, (hipStream_t)stream, C, th, tw, d_in, d_off, d_rect, d_table);
  return idf_last_error();
}

int idf_tile_verify_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                       const float* d_in, int64_t ld_in, const int64_t* d_table,
                       int32_t* d_mismatch) {
  int64_t bands = 0;
  const int rc = tile_launch_shape(n_tiles, C, th, tw, ld_in, &bands);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!d_table || !d_in || !d_mismatch) return IDF_ERR_ARG;
  hipLaunchKernelGGL(tile_verify_u8_kernel, dim3((unsigned)n_tiles, (unsigned)bands), dim3(256),
                     0, (hipStream_t)stream, C, th, tw, d_in, ld_in, d_table, d_mismatch);
  return idf_last_error();
}

}  // extern "C"
