// Host-side probe of the host threads of the host matrix seam (harmony_amd/csrc/hmx_xfer_pool.h, HIP-free): built by tests/test_xfer_cpu.py
// with the host compiler and called through ctypes; with its main() it is also a program of its own (the form a sanitizer build runs).
// XferPool::copy must reproduce memcpy whatever the helper count and the size, one copy after the other on the same pool.
#include "../../harmony_amd/csrc/hmx_xfer_pool.h"
#include <cstdint>
#include <cstdio>
namespace {
// `copies` copies of `bytes` bytes on one pool of `threads` helpers: 0 when every destination equals its source and the guard bytes behind it are intact
int run(int threads, size_t bytes, int copies) {
  hmx::XferPool pool;
  pool.start(threads);
  std::vector<unsigned char> src(bytes), dst(bytes + 64);
  for (int c = 0; c < copies; c++) {
    uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(c + 1) + bytes;      // another pattern for every copy: a stale chunk of the last one shows
    for (size_t i = 0; i < bytes; i++) { x = x * 6364136223846793005ull + 1442695040888963407ull; src[i] = (unsigned char)(x >> 56); }
    std::fill(dst.begin(), dst.end(), (unsigned char)0xA5);
    pool.copy(dst.data(), src.data(), bytes);
    if (bytes && std::memcmp(dst.data(), src.data(), bytes) != 0) return 1;
    for (size_t i = bytes; i < dst.size(); i++) if (dst[i] != 0xA5) return 2;
  }
  return 0;
}
}  // namespace
extern "C" {
long long probe_xfer_chunk(void) { return (long long)hmx::XferPool::CHUNK; }
int probe_xfer_copy(int threads, long long bytes, int copies) { return run(threads, (size_t)bytes, copies); }
}
int main() {
  const size_t C4 = 4 * hmx::XferPool::CHUNK;
  const size_t sizes[] = {0, 1, 4097, C4 - 1, C4, (C4 + 1) | 1, 7 * hmx::XferPool::CHUNK + 12345};
  int bad = 0;
  for (int threads : {0, 3})
    for (size_t n : sizes) {
      const int r = run(threads, n, n >= C4 ? 20 : 2);
      if (r) { std::printf("FAIL threads=%d bytes=%zu code=%d\n", threads, n, r); bad++; }
    }
  std::printf(bad ? "xfer_pool_probe: %d failures\n" : "xfer_pool_probe: ok\n", bad);
  return bad ? 1 : 0;
}
