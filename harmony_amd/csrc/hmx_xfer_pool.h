// hmx_xfer_pool.h -- the host threads of a transfer through the page-locked ring (hmx_api_xfer.inc): one memcpy split over a few spinning
// helpers.  Host code only, no HIP: tests/cpp/xfer_pool_probe.cpp builds it alone.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

namespace hmx {

struct XferPool {
  // (the workers SPIN between the slots of one transfer -- a transfer lasts ~10-20 ms and hands out a slot every ~0.5 ms; waking sleeping
  //  threads through a condition variable for every slot cost more than the copies)
  std::vector<std::thread> th;
  const char* src = nullptr; char* dst = nullptr; size_t bytes = 0;
  std::atomic<size_t> next{0};
  std::atomic<int> gen{0}, running{0};
  std::atomic<bool> stop{false};
  static constexpr size_t CHUNK = 1 << 20;
  void work() {
    for (;;) {
      const size_t off = next.fetch_add(CHUNK);
      if (off >= bytes) break;
      memcpy(dst + off, src + off, std::min(CHUNK, bytes - off));
    }
  }
  void loop() {
    int seen = 0;
    for (;;) {
      int g;
      while ((g = gen.load(std::memory_order_acquire)) == seen) {
        if (stop.load(std::memory_order_relaxed)) return;
        __builtin_ia32_pause();
      }
      seen = g;
      work();
      running.fetch_sub(1, std::memory_order_release);
    }
  }
  void start(int T) {      // (a thread that cannot be created is simply missing: the caller works too, copy() falls back to a plain memcpy without helpers)
    for (int i = 0; i < T; i++) {
      try { th.emplace_back([this] { loop(); }); } catch (...) { break; }
    }
  }
  void copy(void* d, const void* s_, size_t n) {           // blocking; the caller works too
    if (th.empty() || n < 4 * CHUNK) { if (n) memcpy(d, s_, n); return; }      // (n == 0: the pointers may be null)
    src = (const char*)s_; dst = (char*)d; bytes = n; next.store(0);
    running.store((int)th.size(), std::memory_order_relaxed);
    gen.fetch_add(1, std::memory_order_release);
    work();
    while (running.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
  }
  ~XferPool() {
    stop.store(true);
    for (auto& t : th) t.join();
  }
};

}  // namespace hmx
