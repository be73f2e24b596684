// idf_tile_row.h -- a row of the tile tables (tile_kernels.hip, crc_kernels.hip; not part of the
// ABI).  Two formats name the image a tile lies in:
//   int64 [n_tiles][5]  (addr, H, W, y0, x0)              a dense planar uint8 [C, H, W] buffer
//   int64 [n_tiles][8]  (addr, H, W, y0, x0, sc, sy, sx)  byte (c, y, x) at
//                                                        addr + c*sc + y*sy + x*sx
// The first is the second with sc = H*W, sy = W, sx = 1.  Strides are in bytes and not negative;
// every index is 64-bit: a set of images may exceed 2^31 bytes.  A kernel is instantiated per
// format (TileRow<F>), so the planar one keeps its own address arithmetic.
#pragma once
#include <stdint.h>

namespace idf {

constexpr int TILE_FIELDS = 5;          // addr, H, W, y0, x0
constexpr int TILE_FIELDS_STRIDED = 8;  // ... sc, sy, sx

template <int F>
struct TileRow {
  static_assert(F == TILE_FIELDS || F == TILE_FIELDS_STRIDED, "a tile table has 5 or 8 fields");
  uint8_t* base;
  int64_t H, W, y0, x0;  // the image's size, the tile's origin in its coordinates
  int64_t sc, sy, sx;    // read from a strided row only
  __device__ __forceinline__ int64_t at(int64_t c, int64_t y, int64_t x) const {
    return F == TILE_FIELDS ? (c * H + y) * W + x : c * sc + y * sy + x * sx;
  }
  __device__ __forceinline__ bool inside(int64_t y, int64_t x) const {
    return y >= 0 && y < H && x >= 0 && x < W;
  }
};

template <int F>
__device__ __forceinline__ TileRow<F> tile_row(const int64_t* __restrict__ table, int64_t t) {
  const int64_t* row = table + t * F;
  TileRow<F> r;
  r.base = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(row[0]));
  r.H = row[1], r.W = row[2], r.y0 = row[3], r.x0 = row[4];
  r.sc = r.sy = r.sx = 0;
  if (F == TILE_FIELDS_STRIDED) r.sc = row[5], r.sy = row[6], r.sx = row[7];
  return r;
}

}  // namespace idf
