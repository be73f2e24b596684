// Stand-alone check of csrc/idf_crc.h's host side (no device, no library): prints
// "<offset> <length> <crc32 hex>" for runs of a buffer whose byte i is (i * 131 + 89) % 251, and
// checks the combine on the way.  test_integrity_host.py compiles it with the host compiler,
// runs it and compares every line with zlib; built with -fsanitize=address,undefined it is the
// sanitizer run of the header.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "idf_crc.h"

int main() {
  std::vector<int64_t> lens;
  for (int64_t n = 0; n <= 70; ++n) lens.push_back(n);
  for (int64_t n : {255, 256, 257, 4095, 4096, 4097, (1 << 20) + 3}) lens.push_back(n);
  const int64_t total = (1 << 20) + 3 + 8;
  std::vector<uint8_t> buf(total);
  for (int64_t i = 0; i < total; ++i) buf[i] = (uint8_t)((i * 131 + 89) % 251);
  if (idf::crc32_bytes("123456789", 9) != 0xCBF43926u) return 2;  // the standard check value
  for (int off = 0; off < 8; ++off) {
    for (int64_t n : lens) {
      const uint32_t c = idf::crc32_bytes(buf.data() + off, n);
      // the same run in two parts, cut at a third of it
      const int64_t a = n / 3;
      const uint32_t ca = idf::crc32_bytes(buf.data() + off, a);
      const uint32_t cb = idf::crc32_bytes(buf.data() + off + a, n - a);
      if (idf::crc32_combine(ca, cb, (uint64_t)(n - a)) != c) return 3;
      std::printf("%d %lld %08x\n", off, (long long)n, c);
    }
  }
  return 0;
}
