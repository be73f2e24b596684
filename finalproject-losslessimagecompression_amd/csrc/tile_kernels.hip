// Images of any size as tiles of the flow's input (idfcodec/tiled.py): the gather from a ragged
// set of uint8 images to the pixel-major (ld 4) input of a FlowEngine, one batch entry per
// th x tw tile, and the scatter back.  The pad is the reference's ReplicationPad2d((0, pw, 0,
// ph)) (trainer.py:62) by clamped indexing, the tiles are Patching.forward's
// (extenddim.py:51-57); neither is materialised.
//
// Every kernel here reads a device tile table, one row per tile, in one of idf_tile_row.h's two
// formats: (addr, H, W, y0, x0) names a dense planar uint8 [C, H, W] buffer, (addr, H, W, y0,
// x0, sc, sy, sx) an image whose byte (c, y, x) lies at addr + c*sc + y*sy + x*sx; (y0, x0) is
// the tile's origin in the image's coordinates.  Each kernel is a template over the format and
// states its rule once.
//
// One block per (tile, run of TILE_PX consecutive tile pixels).  Neighbouring lanes walk the
// image's smallest stride.  Where that is x within a plane (sx < sc: planar, pitched or not) a
// run is staged through LDS, so that the image side is accessed along x by neighbouring threads
// of a channel and the pixel-major side channel-fastest, neighbouring threads on neighbouring
// floats of a pixel row.  Where the image is channel-fastest itself (sc < sx: HWC, dense or with
// a row pitch, RGBX) both sides are, and the run is one straight pass without LDS: a lane moves
// (pixel j, channel c) between the image byte and float j*ld + c.  The choice depends on the
// tile's row alone, so it is uniform over a block.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idf_codec_internal.h"
#include "idf_tile_row.h"

namespace idf {

constexpr int TILE_PX = 1024;    // tile pixels per block
constexpr int TILE_CMAX = 4;     // channels (the pixel rows of ws['img'] are 4 wide)

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// the block's run of a tile of npx pixels: its first pixel and how many it holds
__device__ __forceinline__ int tile_run(int64_t npx, int64_t* p0) {
  *p0 = (int64_t)blockIdx.y * TILE_PX;
  return (int)(npx - *p0 < TILE_PX ? npx - *p0 : TILE_PX);
}

// whether the image a row names is channel-fastest: the straight pass (planar tables: never)
template <int F>
__device__ __forceinline__ bool tile_interleaved(const TileRow<F>& r) {
  return F == TILE_FIELDS_STRIDED && r.sc < r.sx;
}

// idf_dequant_u8's rule
__device__ __forceinline__ float tile_dequant(int k) {
  return (float)(k + (k >= 128 ? 1 : 0)) * (1.0f / 256.0f);
}

// idf_quant_u8's rule: -> the byte of a pixel-major value; *on_grid is false for a value off
// the grid, equal to 128/256 or outside 0..256, and the return then lies in -1..256, below or
// above every byte as the value is
__device__ __forceinline__ int tile_quant(float v, bool* on_grid) {
  const float s = v * 256.0f;
  const float m = __builtin_rintf(s);
  const bool in_range = m >= 0.0f && m <= 256.0f;
  const int mi = in_range ? (int)m : (m < 0.0f ? -1 : 257);
  *on_grid = (m == s) && in_range && mi != 128;
  return mi >= 129 ? mi - 1 : mi;
}

template <int F>
__global__ void __launch_bounds__(256)
tile_gather_u8_kernel(int C, int th, int tw, const int64_t* __restrict__ table,
                      float* __restrict__ out, int64_t ld) {
  __shared__ float kv[TILE_CMAX * TILE_PX];  // [C][TILE_PX]
  const int64_t t = blockIdx.x;
  const TileRow<F> r = tile_row<F>(table, t);
  const int64_t npx = (int64_t)th * tw;
  int64_t p0;
  const int n = tile_run(npx, &p0);
  const bool straight = tile_interleaved<F>(r);
  auto value = [&](int c, int j) {  // channel c of the run's pixel j, the pad by clamping
    const int64_t p = p0 + j;
    const int64_t y = clamp_i64(r.y0 + p / tw, 0, r.H - 1);
    const int64_t x = clamp_i64(r.x0 + p % tw, 0, r.W - 1);
    return tile_dequant(r.base[r.at(c, y, x)]);
  };
  if (!straight) {
    for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
      const int c = e / n, j = e % n;
      kv[c * TILE_PX + j] = value(c, j);
    }
    __syncthreads();
  }
  float* dst = out + (t * npx + p0) * ld;
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e % C, j = e / C;
    dst[(int64_t)j * ld + c] = straight ? value(c, j) : kv[c * TILE_PX + j];
  }
}

template <int F>
__global__ void __launch_bounds__(256)
tile_scatter_u8_kernel(int C, int th, int tw, const float* __restrict__ in, int64_t ld,
                       const int64_t* __restrict__ table, int32_t* __restrict__ bad) {
  __shared__ uint8_t kv[TILE_CMAX * TILE_PX];  // [C][TILE_PX]
  __shared__ int block_bad;
  const int64_t t = blockIdx.x;
  const TileRow<F> r = tile_row<F>(table, t);
  const int64_t npx = (int64_t)th * tw;
  int64_t p0;
  const int n = tile_run(npx, &p0);
  const bool straight = tile_interleaved<F>(r);
  if (threadIdx.x == 0) block_bad = 0;
  __syncthreads();
  const float* src = in + (t * npx + p0) * ld;
  int n_bad = 0;
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e % C, j = e / C;
    const int64_t p = p0 + j;
    const int64_t y = r.y0 + p / tw, x = r.x0 + p % tw;
    if (!r.inside(y, x)) continue;  // the pad, or outside a crop
    bool on_grid;
    int k = tile_quant(src[(int64_t)j * ld + c], &on_grid);
    if (!on_grid) {
      ++n_bad;
      k = k < 0 ? 0 : (k > 255 ? 255 : k);
    }
    if (straight) r.base[r.at(c, y, x)] = (uint8_t)k;
    else kv[c * TILE_PX + j] = (uint8_t)k;
  }
  if (n_bad) atomicAdd(&block_bad, n_bad);
  __syncthreads();
  if (threadIdx.x == 0 && block_bad) atomicAdd(bad, block_bad);
  if (straight) return;
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e / n, j = e % n;
    const int64_t p = p0 + j;
    const int64_t y = r.y0 + p / tw, x = r.x0 + p % tw;
    if (!r.inside(y, x)) continue;
    r.base[r.at(c, y, x)] = kv[c * TILE_PX + j];
  }
}

// ---- the raw-tile escape (idfcodec/safe.py): a tile's in-image bytes stored as they are, and the
// decoded tiles compared with the source.  Same tables, same grid; these are plain byte copies,
// one pass, neighbouring threads along x within a channel: the stored side is planar.

// The in-image rectangle of the tile, rows [y0, min(y0+th, H)) x columns [x0, min(x0+tw, W)), as
// contiguous uint8 [C][hin][win] at out + off[t].
template <int F>
__global__ void __launch_bounds__(256)
tile_gather_raw_u8_kernel(int C, int th, int tw, const int64_t* __restrict__ table,
                          const int64_t* __restrict__ off, uint8_t* __restrict__ out) {
  const int64_t t = blockIdx.x;
  const TileRow<F> r = tile_row<F>(table, t);
  if (!r.inside(r.y0, r.x0)) return;  // no in-image part
  const int64_t hin = r.H - r.y0 < th ? r.H - r.y0 : th, win = r.W - r.x0 < tw ? r.W - r.x0 : tw;
  int64_t p0;
  const int n = tile_run((int64_t)th * tw, &p0);
  uint8_t* dst = out + off[t];
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e / n, j = e % n;
    const int64_t p = p0 + j;
    const int64_t y = p / tw, x = p % tw;
    if (y >= hin || x >= win) continue;  // the pad is not stored
    dst[(c * hin + y) * win + x] = r.base[r.at(c, r.y0 + y, r.x0 + x)];
  }
}

// The inverse: byte (ch, y, x) of the stored [C][hin][win] rectangle of tile t (rect[t] = (hin,
// win)) to image byte (ch, y0 + y, x0 + x), only inside [0,H) x [0,W).
template <int F>
__global__ void __launch_bounds__(256)
tile_scatter_raw_u8_kernel(int C, int th, int tw, const uint8_t* __restrict__ in,
                           const int64_t* __restrict__ off, const int32_t* __restrict__ rect,
                           const int64_t* __restrict__ table) {
  const int64_t t = blockIdx.x;
  const TileRow<F> r = tile_row<F>(table, t);
  const int64_t hin = rect[2 * t], win = rect[2 * t + 1];
  int64_t p0;
  const int n = tile_run((int64_t)th * tw, &p0);
  const uint8_t* src = in + off[t];
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e / n, j = e % n;
    const int64_t p = p0 + j;
    const int64_t yy = p / tw, xx = p % tw;
    if (yy >= hin || xx >= win) continue;  // not stored
    const int64_t y = r.y0 + yy, x = r.x0 + xx;
    if (!r.inside(y, x)) continue;  // outside a crop
    r.base[r.at(c, y, x)] = src[(c * hin + yy) * win + xx];
  }
}

// mismatch[t] += the (pixel, channel) pairs of tile t, over the tile pixels whose source position
// lies inside the image, whose value in the pixel-major tile buffer is not the dequantised source
// byte (idf_quant_u8's rule; a value off the grid is a mismatch).
template <int F>
__global__ void __launch_bounds__(256)
tile_verify_u8_kernel(int C, int th, int tw, const float* __restrict__ in, int64_t ld,
                      const int64_t* __restrict__ table, int32_t* __restrict__ mismatch) {
  __shared__ int part[256];
  const int64_t t = blockIdx.x;
  const TileRow<F> r = tile_row<F>(table, t);
  const int64_t npx = (int64_t)th * tw;
  int64_t p0;
  const int n = tile_run(npx, &p0);
  const float* src = in + (t * npx + p0) * ld;
  int n_bad = 0;
  for (int e = threadIdx.x; e < C * n; e += blockDim.x) {
    const int c = e % C, j = e / C;
    const int64_t p = p0 + j;
    const int64_t y = r.y0 + p / tw, x = r.x0 + p % tw;
    if (!r.inside(y, x)) continue;  // the pad is not compared
    bool on_grid;
    const int k = tile_quant(src[(int64_t)j * ld + c], &on_grid);
    if (!on_grid || k != (int)r.base[r.at(c, y, x)]) ++n_bad;
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

// The calls, once for both table formats: the argument checks, then kernel<F> over the grid of
// (tile, run) blocks.  `needed` are the pointers a launch reads or writes.
template <typename Kernel, typename... Args>
static int tile_launch(Kernel kernel, void* stream, int64_t n_tiles, int32_t C, int32_t th,
                       int32_t tw, int64_t ld, bool needed, Args... args) {
  int64_t bands = 0;
  const int rc = tile_launch_shape(n_tiles, C, th, tw, ld, &bands);
  if (rc != IDF_OK) return rc;
  if (n_tiles == 0) return IDF_OK;
  if (!needed) return IDF_ERR_ARG;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_tiles, (unsigned)bands), dim3(256), 0,
                     (hipStream_t)stream, C, th, tw, args...);
  return idf_last_error();
}

template <int F>
static int tile_gather(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                       const int64_t* d_table, float* d_out, int64_t ld_out) {
  return tile_launch(tile_gather_u8_kernel<F>, stream, n_tiles, C, th, tw, ld_out,
                     d_table && d_out, d_table, d_out, ld_out);
}

template <int F>
static int tile_scatter(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                        const float* d_in, int64_t ld_in, const int64_t* d_table,
                        int32_t* d_bad) {
  return tile_launch(tile_scatter_u8_kernel<F>, stream, n_tiles, C, th, tw, ld_in,
                     d_table && d_in && d_bad, d_in, ld_in, d_table, d_bad);
}

template <int F>
static int tile_gather_raw(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                           const int64_t* d_table, const int64_t* d_off, uint8_t* d_out) {
  return tile_launch(tile_gather_raw_u8_kernel<F>, stream, n_tiles, C, th, tw, (int64_t)C,
                     d_table && d_off && d_out, d_table, d_off, d_out);
}

template <int F>
static int tile_scatter_raw(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                            const uint8_t* d_in, const int64_t* d_off, const int32_t* d_rect,
                            const int64_t* d_table) {
  return tile_launch(tile_scatter_raw_u8_kernel<F>, stream, n_tiles, C, th, tw, (int64_t)C,
                     d_table && d_in && d_off && d_rect, d_in, d_off, d_rect, d_table);
}

template <int F>
static int tile_verify(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                       const float* d_in, int64_t ld_in, const int64_t* d_table,
                       int32_t* d_mismatch) {
  return tile_launch(tile_verify_u8_kernel<F>, stream, n_tiles, C, th, tw, ld_in,
                     d_table && d_in && d_mismatch, d_in, ld_in, d_table, d_mismatch);
}

}  // namespace idf

using namespace idf;

extern "C" {

int idf_tile_gather_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                       const int64_t* d_table, float* d_out, int64_t ld_out) {
  return tile_gather<TILE_FIELDS>(stream, n_tiles, C, th, tw, d_table, d_out, ld_out);
}

int idf_tile_gather_strided_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                               const int64_t* d_table, float* d_out, int64_t ld_out) {
  return tile_gather<TILE_FIELDS_STRIDED>(stream, n_tiles, C, th, tw, d_table, d_out, ld_out);
}

int idf_tile_scatter_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                        const float* d_in, int64_t ld_in, const int64_t* d_table,
                        int32_t* d_bad) {
  return tile_scatter<TILE_FIELDS>(stream, n_tiles, C, th, tw, d_in, ld_in, d_table, d_bad);
}

int idf_tile_scatter_strided_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                                const float* d_in, int64_t ld_in, const int64_t* d_table,
                                int32_t* d_bad) {
  return tile_scatter<TILE_FIELDS_STRIDED>(stream, n_tiles, C, th, tw, d_in, ld_in, d_table,
                                           d_bad);
}

int idf_tile_gather_raw_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                           const int64_t* d_table, const int64_t* d_off, uint8_t* d_out) {
  return tile_gather_raw<TILE_FIELDS>(stream, n_tiles, C, th, tw, d_table, d_off, d_out);
}

int idf_tile_gather_raw_strided_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th,
                                   int32_t tw, const int64_t* d_table, const int64_t* d_off,
                                   uint8_t* d_out) {
  return tile_gather_raw<TILE_FIELDS_STRIDED>(stream, n_tiles, C, th, tw, d_table, d_off, d_out);
}

int idf_tile_scatter_raw_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                            const uint8_t* d_in, const int64_t* d_off, const int32_t* d_rect,
                            const int64_t* d_table) {
  return tile_scatter_raw<TILE_FIELDS>(stream, n_tiles, C, th, tw, d_in, d_off, d_rect, d_table);
}

int idf_tile_scatter_raw_strided_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th,
                                    int32_t tw, const uint8_t* d_in, const int64_t* d_off,
                                    const int32_t* d_rect, const int64_t* d_table) {
  return tile_scatter_raw<TILE_FIELDS_STRIDED>(stream, n_tiles, C, th, tw, d_in, d_off, d_rect,
                                               d_table);
}

int idf_tile_verify_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                       const float* d_in, int64_t ld_in, const int64_t* d_table,
                       int32_t* d_mismatch) {
  return tile_verify<TILE_FIELDS>(stream, n_tiles, C, th, tw, d_in, ld_in, d_table, d_mismatch);
}

int idf_tile_verify_strided_u8(void* stream, int64_t n_tiles, int32_t C, int32_t th, int32_t tw,
                               const float* d_in, int64_t ld_in, const int64_t* d_table,
                               int32_t* d_mismatch) {
  return tile_verify<TILE_FIELDS_STRIDED>(stream, n_tiles, C, th, tw, d_in, ld_in, d_table,
                                          d_mismatch);
}

}  // extern "C"
