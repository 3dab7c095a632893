// hmx_api_xfer.inc -- part of hmx_api.cpp (included there, ONE translation unit, ahead of its users): the host matrix seam -- page-locked ring, host threads (hmx_xfer_pool.h), the pipe of one transfer and the slab pipeline of either direction (hmx_setup / hmx_map_query / hmx_get_matrix with host buffers)
// ---- host side of the R seam (R/ui.R:178-183, 292-295: a pageable fp64 matrix in, a fresh pageable fp64 matrix out) ---------------------
// Page-locking the caller's 400 MB matrix for one transfer costs more than the transfer (every page is faulted in and pinned by ONE thread
// before the first byte moves).  Default path instead: a small ring of page-locked buffers, allocated once per process, and a few host
// threads that move the bytes between the caller's matrix and the ring slot by slot while the DMA engine moves the previous slots --
// on egress the threads are also the ones that first touch the fresh destination pages, in parallel.  HMX_XFER=pin: register the caller's
// buffer (the earlier path); HMX_PIN=0: plain pageable copies; HMX_XFER_THREADS: threads (default 8).
bool host_pin_enabled() { const char* e = getenv("HMX_PIN"); return !(e && atoi(e) == 0); }
int xfer_mode() {     // 0 pageable copies, 1 register the caller's buffer, 2 ring of page-locked slots + host threads (default)
  if (!host_pin_enabled()) return 0;
  const char* e = getenv("HMX_XFER");
  if (e && std::string(e) == "pin") return 1;
  return 2;
}
int xfer_threads() {      // (the workers spin while a transfer runs: never more of them than spare cores)
  const char* e = getenv("HMX_XFER_THREADS");
  const int t = e ? atoi(e) : 8, spare = (int)std::thread::hardware_concurrency() - 1;
  return std::max(0, std::min(std::min(t, 64), std::max(spare, 0)));
}
struct XferRing {     // page-locked staging slots + the copy stream, HBM staging slabs and events of a transfer: one set per device and
                      // process, built (and run through once) on first use, shared by all handles (guarded: one transfer at a time)
  static constexpr int NB = 4;
  static constexpr size_t SLOT = (size_t)16 << 20;
  std::mutex mu, init_mu;
  void* slot[NB] = {nullptr, nullptr, nullptr, nullptr};
  void* stage[2] = {nullptr, nullptr};                       // HBM staging slabs (SLOT bytes each)
  hipStream_t cs = nullptr;
  hipEvent_t ev_a[2] = {nullptr, nullptr}, ev_b[2] = {nullptr, nullptr}, ev_slot[NB] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = false, tried = false;
  bool ensure() {
    std::lock_guard<std::mutex> lk(init_mu);
    if (tried) return ok;
    tried = true;
    bool good = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < NB && good; i++) good = hipHostMalloc(&slot[i], SLOT, hipHostMallocDefault) == hipSuccess && hipEventCreateWithFlags(&ev_slot[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && good; i++) good = hipMalloc(&stage[i], SLOT) == hipSuccess && hipEventCreateWithFlags(&ev_a[i], hipEventDisableTiming) == hipSuccess &&
                                               hipEventCreateWithFlags(&ev_b[i], hipEventDisableTiming) == hipSuccess;
    // first touch from both sides and one pass through exactly the calls a transfer makes (the CPU faults the slots' pages in on its
    // first write, the device maps them and sets up its copy queues on the first asynchronous copy): once per process instead of inside
    // the first matrix's transfer
    for (int i = 0; i < NB && good; i++) {
      memset(slot[i], 0, SLOT);
      good = hipMemcpyAsync(stage[i & 1], slot[i], SLOT, hipMemcpyHostToDevice, cs) == hipSuccess && hipEventRecord(ev_slot[i], cs) == hipSuccess &&
             hipMemcpyAsync(slot[i], stage[i & 1], SLOT, hipMemcpyDeviceToHost, cs) == hipSuccess && hipEventRecord(ev_a[i & 1], cs) == hipSuccess &&
             hipEventSynchronize(ev_slot[i]) == hipSuccess;
    }
    if (good) good = hipStreamSynchronize(cs) == hipSuccess;
    if (good) {
      // ... and once through the helper threads (round 3 measured +16 ms on a process' FIRST threaded transfer and left it unexplained:
      // thread stacks, first scheduling of eight spinning threads, the cores' clocks): a pool of the size a transfer uses moves 4 slots'
      // worth of bytes between the slots here, once per process, instead of inside the first matrix's transfer
      XferPool warm; warm.start(xfer_threads());
      for (int r = 0; r < 2; r++) for (int i = 0; i + 1 < NB; i += 2) warm.copy(slot[i + 1], slot[i], SLOT);
    }
    if (!good) (void)hipGetLastError();
    return ok = good;
  }
};
XferRing& xfer_ring(int device) { static std::mutex m; static std::map<int, XferRing> rings; std::lock_guard<std::mutex> lk(m); return rings[device]; }
#define XFCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

// What one transfer of a host matrix needs: a copy stream, two HBM staging slabs, two event pairs and -- through the ring only -- the
// page-locked slots with an event each.  Borrowed from the process' ring (whose mutex it then holds) or its own, released either way when
// it goes out of scope, the copy stream drained first.
struct XferPipe {
  static constexpr size_t OWN_SLAB = (size_t)128 << 20;      // bytes of a staging slab of its own
  hipStream_t cs = nullptr; void* stage[2] = {nullptr, nullptr};
  hipEvent_t ev_a[2] = {nullptr, nullptr}, ev_b[2] = {nullptr, nullptr};
  void* const* slot = nullptr; hipEvent_t* ev_slot = nullptr;      // the ring's, or none
  int64_t slab = 0;            // whole cells per slab
  int pinned = 0;              // hmx_get "timer:ingest_pinned": 2 the ring, 1 the caller's buffer registered, 0 pageable
  std::unique_lock<std::mutex> ring_lock; void* registered = nullptr;      // what is held for the transfer: the ring's mutex, or the caller's buffer page-locked
  // the pipe of a transfer of `cells` cells of cell_bytes each between HBM and `host`: the ring's where that is the mode and the ring came up,
  // else its own.  A slab holds min(the path's default, cap_bytes) bytes (cap_bytes 0: the default) of whole cells, at least one.
  hipError_t open(int device, void* host, int64_t cells, size_t cell_bytes, int64_t cap_bytes) {
    const auto cells_in = [&](size_t bytes) { return std::max<int64_t>(1, (int64_t)(cap_bytes > 0 ? std::min(bytes, (size_t)cap_bytes) : bytes) / (int64_t)cell_bytes); };
    if (xfer_mode() == 2 && xfer_ring(device).ensure()) {
      XferRing& ring = xfer_ring(device);
      ring_lock = std::unique_lock<std::mutex>(ring.mu);
      cs = ring.cs; slot = ring.slot; ev_slot = ring.ev_slot; pinned = 2; slab = cells_in(XferRing::SLOT);
      for (int i = 0; i < 2; i++) { stage[i] = ring.stage[i]; ev_a[i] = ring.ev_a[i]; ev_b[i] = ring.ev_b[i]; }
      return hipSuccess;
    }
    // The caller's matrix is pageable (R's heap): page-lock it for the duration of the transfer, so that the slab copies are real DMA
    // at PCIe speed instead of the runtime's staged pageable path (HMX_PIN=0 leaves it pageable; a failed registration is not an error).
    slab = cells_in(OWN_SLAB);
    if (xfer_mode() >= 1 && hipHostRegister(host, (size_t)cells * cell_bytes, hipHostRegisterDefault) == hipSuccess) registered = host;
    else (void)hipGetLastError();
    pinned = registered ? 1 : 0;
    XFCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
      XFCHK(hipMalloc(&stage[i], (size_t)std::min(slab, cells) * cell_bytes));
      XFCHK(hipEventCreateWithFlags(&ev_a[i], hipEventDisableTiming));
      XFCHK(hipEventCreateWithFlags(&ev_b[i], hipEventDisableTiming));
    }
    return hipSuccess;
  }
  ~XferPipe() {
    if (cs) (void)hipStreamSynchronize(cs);
    if (slot) return;      // (the ring keeps what it lent; its mutex goes with ring_lock)
    for (int i = 0; i < 2; i++) { if (stage[i]) (void)hipFree(stage[i]); if (ev_a[i]) (void)hipEventDestroy(ev_a[i]); if (ev_b[i]) (void)hipEventDestroy(ev_b[i]); }
    if (cs) (void)hipStreamDestroy(cs);
    if (registered) (void)hipHostUnregister(registered);
  }
};

// Ingest: host cells [0, N) -> convert(stage, s0, cnt) on `st`, slab by slab through the two staging slabs: the copy of slab s+1 (copy stream)
// overlaps the conversion of slab s.  Through the ring, host threads fill slot s % NB first while the DMA engine drains the earlier ones.
// convert launches the conversion of cells [s0, s0 + cnt) out of the slab and returns the launch's error.
template <class Convert>
hipError_t xfer_ingest(XferPipe& P, hipStream_t st, const void* host, int64_t N, size_t cell_bytes, Convert convert) {
  constexpr int NB = XferRing::NB;
  XferPool pool; if (P.slot) pool.start(xfer_threads());
  hipEvent_t* copied = P.ev_a; hipEvent_t* used = P.ev_b; hipEvent_t* left = P.ev_slot;   // left[r]: slot r's bytes have left for the device
  int it = 0;
  for (int64_t s0 = 0; s0 < N; s0 += P.slab, it++) {
    const int64_t cnt = std::min<int64_t>(P.slab, N - s0);
    const size_t nbytes = (size_t)cnt * cell_bytes; const int b = it & 1, r = it % NB;
    const void* from = (const char*)host + (size_t)s0 * cell_bytes;
    if (P.slot) {
      if (it >= NB) XFCHK(hipEventSynchronize(left[r]));
      pool.copy(P.slot[r], from, nbytes);
      from = P.slot[r];
    }
    if (it >= 2) XFCHK(hipStreamWaitEvent(P.cs, used[b], 0));           // the slab's previous conversion has read it
    XFCHK(hipMemcpyAsync(P.stage[b], from, nbytes, hipMemcpyHostToDevice, P.cs));
    if (P.slot) XFCHK(hipEventRecord(left[r], P.cs));
    XFCHK(hipEventRecord(copied[b], P.cs));
    XFCHK(hipStreamWaitEvent(st, copied[b], 0));
    XFCHK(convert(P.stage[b], s0, cnt));
    XFCHK(hipEventRecord(used[b], st));
  }
  return hipStreamSynchronize(st);
}

// Egress: convert(stage, s0, cnt) on `st` -> host cells [0, N), slab by slab (the conversion of slab s+1 overlaps the copy of slab s).  Through
// the ring a slab lands in slot s % NB, and the host threads copy it into the caller's (fresh, pageable) matrix, touching its pages in
// parallel, NB - 1 slabs behind the conversions -- the next slots are on their way meanwhile.
template <class Convert>
hipError_t xfer_egress(XferPipe& P, hipStream_t st, void* host, int64_t N, size_t cell_bytes, Convert convert) {
  constexpr int NB = XferRing::NB;
  XferPool pool; if (P.slot) pool.start(xfer_threads());
  hipEvent_t* conv = P.ev_a; hipEvent_t* copied = P.ev_b; hipEvent_t* arrived = P.ev_slot;
  const int nslabs = (int)((N + P.slab - 1) / P.slab), lag = P.slot ? NB - 1 : 0;
  for (int it = 0; it < nslabs + lag; it++) {
    if (it < nslabs) {
      const int64_t s0 = (int64_t)it * P.slab, c = std::min<int64_t>(P.slab, N - s0); const int b = it & 1;
      if (it >= 2) XFCHK(hipStreamWaitEvent(st, copied[b], 0));   // the slab's previous contents have left for the host
      XFCHK(convert(P.stage[b], s0, c));
      XFCHK(hipEventRecord(conv[b], st));
      XFCHK(hipStreamWaitEvent(P.cs, conv[b], 0));
      // (ring slot it % NB was drained by the host in iteration it - NB + lag, i.e. before this point)
      XFCHK(hipMemcpyAsync(P.slot ? P.slot[it % NB] : (char*)host + (size_t)s0 * cell_bytes, P.stage[b], (size_t)c * cell_bytes, hipMemcpyDeviceToHost, P.cs));
      XFCHK(hipEventRecord(copied[b], P.cs));
      if (P.slot) XFCHK(hipEventRecord(arrived[it % NB], P.cs));
    }
    if (P.slot && it >= lag) {          // slab j has arrived in its ring slot: out of the ring, into the caller's matrix
      const int j = it - lag; const int64_t s0 = (int64_t)j * P.slab, c = std::min<int64_t>(P.slab, N - s0);
      XFCHK(hipEventSynchronize(arrived[j % NB]));
      pool.copy((char*)host + (size_t)s0 * cell_bytes, P.slot[j % NB], (size_t)c * cell_bytes);
    }
  }
  XFCHK(hipStreamSynchronize(P.cs));
  return hipStreamSynchronize(st);
}
#undef XFCHK
