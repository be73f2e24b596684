// idf_crc.h -- CRC-32 as zlib computes it (IEEE 802.3, reflected polynomial 0xEDB88320, init
// and final XOR 0xFFFFFFFF), in parts that combine in any order, usable from host and device
// code (gfx950) the way idf_cdf.h is.
//
// A value is a polynomial over GF(2) modulo P in the reflected representation: bit 31 is the
// coefficient of x^0, bit 0 that of x^31; 1 = 0x80000000, x^8 = 0x00800000.
//   raw0(M)      the table / bitwise CRC with init 0 and no final XOR: M(x) * x^32 mod P
//   a (x) b      crc32_mul: the product mod P, 32 shift / XOR steps
//   x^(8k)       crc32_xpow8(k): square-and-multiply
// With n = |M| and M cut into parts, part i ending at offset end_i:
//   crc32(M) = XOR_i raw0(part_i) (x) x^(8 (n - end_i))  ^  0xFFFFFFFF (x) x^(8 n)  ^  0xFFFFFFFF
// XOR is commutative, so the parts may be accumulated in any order (one atomicXor per block).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IDF_CRC_HD __host__ __device__ inline
#else
#define IDF_CRC_HD inline
#endif

namespace idf {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;   // x^0
constexpr uint32_t kCrcX8 = 0x00800000u;    // x^8

// a * b mod P
IDF_CRC_HD constexpr uint32_t crc32_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= (a & (kCrcOne >> i)) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);  // b * x
  }
  return p;
}

// x^(8 k) mod P, k >= 0 bytes
IDF_CRC_HD constexpr uint32_t crc32_xpow8(uint64_t k) {
  uint32_t r = kCrcOne, b = kCrcX8;
  for (; k; k >>= 1) {
    if (k & 1u) r = crc32_mul(r, b);
    b = crc32_mul(b, b);
  }
  return r;
}

// entry i of the byte table: raw0 of the one byte i
IDF_CRC_HD constexpr uint32_t crc32_table_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i >> 1) ^ ((i & 1u) ? kCrcPoly : 0u);
  return i;
}

// one byte into a running raw CRC, over a table of crc32_table_entry values
IDF_CRC_HD uint32_t crc32_byte(const uint32_t* tab, uint32_t crc, uint8_t b) {
  return tab[(crc ^ b) & 0xffu] ^ (crc >> 8);
}

// the byte loop: raw0 of p[0, n) continued from crc (0 for a part of its own)
IDF_CRC_HD uint32_t crc32_raw0(const uint32_t* tab, const uint8_t* p, int64_t n,
                               uint32_t crc = 0) {
  for (int64_t i = 0; i < n; ++i) crc = crc32_byte(tab, crc, p[i]);
  return crc;
}

// what init and final XOR add to raw0 of a message of n bytes: the CRC-32 of n zero bytes
IDF_CRC_HD constexpr uint32_t crc32_frame(uint64_t n) {
  return crc32_mul(0xFFFFFFFFu, crc32_xpow8(n)) ^ 0xFFFFFFFFu;
}

// CRC-32 of a || b from the CRC-32 of a, of b and the length of b (zlib's crc32_combine):
// frame(|a|) (x) x^(8 |b|) ^ frame(|b|) = frame(|a| + |b|), so the frames need no correction.
IDF_CRC_HD constexpr uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return crc32_mul(crc_a, crc32_xpow8(len_b)) ^ crc_b;
}

struct Crc32Table {
  uint32_t t[256];
  constexpr Crc32Table() : t() {
    for (uint32_t i = 0; i < 256; ++i) t[i] = crc32_table_entry(i);
  }
};

// host: the CRC-32 of p[0, n)
inline uint32_t crc32_bytes(const void* p, int64_t n) {
  static const Crc32Table tab;
  if (n <= 0) return 0;
  return crc32_raw0(tab.t, static_cast<const uint8_t*>(p), n) ^ crc32_frame((uint64_t)n);
}

}  // namespace idf
