// hmx_api_project.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_project_counts
// (include/harmony_mi355x_project.h; DESIGN "Projecting query counts").  Kernel: hmx_project.hip.
// The call keeps no state on the handle but the timer: every device buffer lives for one call (hmx_api_call.inc).

namespace {

constexpr int64_t PROJ_SLAB_BYTES = (int64_t)256 << 20;      // index + value bytes of a staging slab (the "project_slab_bytes" lab field overrides it)

struct ProjSlab { int64_t row0, row1; };      // cells [row0, row1)

// Slabs of whole cells whose stored entries fit `cap` entries; a cell longer than that gets a slab of its own.
std::vector<ProjSlab> proj_slabs(const int64_t* indptr, int64_t Nq, int64_t cap) {
  std::vector<ProjSlab> S;
  for (int64_t r = 0; r < Nq;) {
    int64_t e = r + 1;
    while (e < Nq && indptr[e + 1] - indptr[r] <= cap) e++;
    S.push_back({r, e});
    r = e;
  }
  return S;
}

// host CSR: indptr monotone from 0, every column in [0, G_all).  0, or 1 / 2 with the offending position in *where
int proj_validate(const int64_t* indptr, const int32_t* indices, int64_t Nq, int32_t G_all, int64_t* where) {
  if (indptr[0] != 0) { *where = 0; return 1; }
  for (int64_t i = 0; i < Nq; i++) if (indptr[i + 1] < indptr[i]) { *where = i; return 1; }
  const int64_t nnz = indptr[Nq];
  unsigned nt = std::thread::hardware_concurrency(); if (nt < 1) nt = 1; if (nt > 16) nt = 16;
  if (nnz < (int64_t)1 << 22) nt = 1;
  std::vector<int64_t> first((size_t)nt, -1);
  auto run = [&](unsigned t) {
    const int64_t a = nnz * t / nt, b = nnz * (t + 1) / nt;
    for (int64_t e = a; e < b; e++) if ((uint32_t)indices[e] >= (uint32_t)G_all) { first[t] = e; return; }
  };
  if (nt == 1) run(0);
  else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back(run, t);
    for (auto& x : th) x.join();
  }
  for (unsigned t = 0; t < nt; t++) if (first[t] >= 0) { *where = first[t]; return 2; }
  return 0;
}

const char* proj_violation(unsigned flag) {
  if (flag & PROJ_BAD_INDPTR) return "indptr is not monotone within [0, nnz]";
  if (flag & PROJ_BAD_COLUMN) return "a column index is outside [0, G_all)";
  if (flag & PROJ_BAD_NEGATIVE) return "a stored value is negative";
  return "a stored value is not finite";
}

// One pass over a CSR matrix of `N` rows: launch(indptr, base, nnz, indices, data, nrows, row0) once for a device-resident matrix, once per slab
// of whole cells for a host-resident one -- two sets of staging buffers (owned by `B`), the copy of slab t + 1 (upload stream) beside the kernel
// of slab t.  Returns with both streams drained.  (hmx_project_counts; hmx_gene_stats and hmx_pca_prepare in hmx_api_pca.inc)
template <class F>
int csr_sweep(hmx_ctx* ctx, CallBufs& B, int64_t N, const int64_t* indptr, const int32_t* indices, const void* data, int esz, int32_t csr_location,
              const char* what, F launch) {
  hipStream_t st = ctx->L.stream;
  if (csr_location == HMX_DEVICE) {
    long long nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, indptr + N, sizeof(nnz), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nnz < 0) return fail(ctx, HMX_ERR_ARG, "indptr[Nq] is negative");
    launch((const long long*)indptr, (long long)0, nnz, indices, data, (long long)N, (long long)0); KCHK();
    return 0;
  }
  // ---- slabs of whole cells through two sets of staging buffers
  const int64_t cap_bytes = ctx->project_slab_bytes > 0 ? ctx->project_slab_bytes : PROJ_SLAB_BYTES;
  const std::vector<ProjSlab> S = proj_slabs(indptr, N, std::max<int64_t>(1, cap_bytes / (4 + esz)));
  int64_t max_nnz = 1, max_rows = 1;
  for (const ProjSlab& s : S) { max_nnz = std::max(max_nnz, indptr[s.row1] - indptr[s.row0]); max_rows = std::max(max_rows, s.row1 - s.row0); }
  ctx->project_slabs = (int64_t)S.size();
  const int nset = S.size() > 1 ? 2 : 1;
  long long* sptr[2]; int* sidx[2]; char* sval[2];
  for (int s = 0; s < nset; s++) {
    HIPCHK(B.get(&sptr[s], (size_t)max_rows + 1)); HIPCHK(B.get(&sidx[s], (size_t)max_nnz)); HIPCHK(B.get(&sval[s], (size_t)max_nnz * esz));
  }
  struct Side {      // the upload stream and the events of one pass
    hipStream_t up = nullptr; hipEvent_t uploaded[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
    ~Side() {
      for (int s = 0; s < 2; s++) { if (uploaded[s]) (void)hipEventDestroy(uploaded[s]); if (consumed[s]) (void)hipEventDestroy(consumed[s]); }
      if (up) (void)hipStreamDestroy(up);
    }
  } Y;
  HIPCHK(hipStreamCreateWithFlags(&Y.up, hipStreamNonBlocking));
  for (int s = 0; s < nset; s++) {
    HIPCHK(hipEventCreateWithFlags(&Y.uploaded[s], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&Y.consumed[s], hipEventDisableTiming));
  }
  HIPCHK(hipEventRecord(Y.uploaded[0], st));      // the tables are in place before the first kernel: same stream; and the upload stream
  HIPCHK(hipStreamWaitEvent(Y.up, Y.uploaded[0], 0));      // starts behind them only to keep the order of the copies simple
  hipError_t e = hipSuccess;
  for (size_t t = 0; t < S.size() && e == hipSuccess; t++) {
    const int s = (int)(t & 1);
    const int64_t r0 = S[t].row0, nr = S[t].row1 - r0, base = indptr[r0], cnt = indptr[S[t].row1] - base;
    if (t >= 2) e = hipStreamWaitEvent(Y.up, Y.consumed[s], 0);      // the kernel of slab t - 2 has read this set
    if (e == hipSuccess) e = hipMemcpyAsync(sptr[s], indptr + r0, (size_t)(nr + 1) * sizeof(int64_t), hipMemcpyHostToDevice, Y.up);
    if (e == hipSuccess && cnt) e = hipMemcpyAsync(sidx[s], indices + base, (size_t)cnt * sizeof(int32_t), hipMemcpyHostToDevice, Y.up);
    if (e == hipSuccess && cnt) e = hipMemcpyAsync(sval[s], (const char*)data + (size_t)base * esz, (size_t)cnt * esz, hipMemcpyHostToDevice, Y.up);
    if (e == hipSuccess) e = hipEventRecord(Y.uploaded[s], Y.up);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, Y.uploaded[s], 0);
    if (e != hipSuccess) break;
    launch((const long long*)sptr[s], (long long)base, (long long)cnt, (const int*)sidx[s], (const void*)sval[s], (long long)nr, (long long)r0);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(Y.consumed[s], st);
  }
  const hipError_t e1 = hipStreamSynchronize(Y.up), e2 = hipStreamSynchronize(st);      // (the buffers are released by the caller: nothing may still use them)
  if (e != hipSuccess || e1 != hipSuccess || e2 != hipSuccess)
    return fail(ctx, HMX_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e != hipSuccess ? e : e1 != hipSuccess ? e1 : e2));
  return 0;
}

// the checks of a count matrix's description that need no device, and the host's pass over a host-resident matrix
int csr_args(hmx_ctx* ctx, int64_t N, int32_t G_all, const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype,
             int32_t csr_location, double scale, const double* totals) {
  if (!indptr || !indices || !data) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (N <= 0 || G_all <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (data_dtype != HMX_F32 && data_dtype != HMX_F64) return fail(ctx, HMX_ERR_ARG, "data_dtype must be HMX_F32 or HMX_F64");
  if (csr_location != HMX_HOST && csr_location != HMX_DEVICE) return fail(ctx, HMX_ERR_ARG, "a location must be HMX_HOST or HMX_DEVICE");
  if (G_all > (1 << 24)) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: G, G_all <= 2^24");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 cells");
  if (!(scale > 0) || !std::isfinite(scale)) return fail(ctx, HMX_ERR_ARG, "scale must be positive and finite");
  if (totals)
    for (int64_t i = 0; i < N; i++)
      if (!(totals[i] >= 0) || !std::isfinite(totals[i])) return fail(ctx, HMX_ERR_ARG, "totals must be non-negative and finite (cell " + std::to_string(i) + ")");
  return 0;
}
int csr_host_pass(hmx_ctx* ctx, int64_t N, int32_t G_all, const int64_t* indptr, const int32_t* indices) {
  int64_t where = 0;
  const int v = proj_validate(indptr, indices, N, G_all, &where);
  if (v == 1) return fail(ctx, HMX_ERR_ARG, "indptr is not monotone from 0 (row " + std::to_string(where) + ")");
  if (v == 2) return fail(ctx, HMX_ERR_ARG, "a column index is outside [0, G_all) (entry " + std::to_string(where) + ")");
  return 0;
}

}  // namespace

extern "C" {

int hmx_project_counts(hmx_ctx* ctx, int64_t Nq, int32_t G_all, const int64_t* indptr, const int32_t* indices, const void* data,
                       int32_t data_dtype, int32_t csr_location, const int32_t* slot, const double* U, const double* mean, const double* sd,
                       int32_t G, int32_t d, double scale, double clip, const double* totals, void* out, int32_t out_location) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!indptr || !indices || !data || !slot || !U || !mean || !sd || !out) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (Nq <= 0 || G_all <= 0 || G <= 0 || d <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (data_dtype != HMX_F32 && data_dtype != HMX_F64) return fail(ctx, HMX_ERR_ARG, "data_dtype must be HMX_F32 or HMX_F64");
  if ((csr_location != HMX_HOST && csr_location != HMX_DEVICE) || (out_location != HMX_HOST && out_location != HMX_DEVICE))
    return fail(ctx, HMX_ERR_ARG, "a location must be HMX_HOST or HMX_DEVICE");
  if (d > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= 128");
  if (G > (1 << 24) || G_all > (1 << 24)) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: G, G_all <= 2^24");
  if (Nq > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 cells");
  if (!(scale > 0) || !std::isfinite(scale)) return fail(ctx, HMX_ERR_ARG, "scale must be positive and finite");
  if (std::isnan(clip) || std::isinf(clip)) return fail(ctx, HMX_ERR_ARG, "clip must be finite (<= 0: none)");
  for (int32_t j = 0; j < G; j++) {
    if (!(sd[j] > 0) || !std::isfinite(sd[j])) return fail(ctx, HMX_ERR_ARG, "sd must be positive and finite (reference gene " + std::to_string(j) + ")");
    if (!(mean[j] >= 0) || !std::isfinite(mean[j])) return fail(ctx, HMX_ERR_ARG, "mean must be non-negative and finite (reference gene " + std::to_string(j) + ")");
  }
  for (int64_t i = 0; i < (int64_t)G * d; i++) if (!std::isfinite(U[i])) return fail(ctx, HMX_ERR_ARG, "the loadings must be finite");
  std::vector<char> present((size_t)G, 0);
  for (int32_t g = 0; g < G_all; g++) {
    const int32_t j = slot[g];
    if (j < -1 || j >= G) return fail(ctx, HMX_ERR_ARG, "slot[" + std::to_string(g) + "] = " + std::to_string(j) + " is outside -1 .. G - 1");
    if (j >= 0) {
      if (present[(size_t)j]) return fail(ctx, HMX_ERR_ARG, "slot maps two query genes to reference gene " + std::to_string(j));
      present[(size_t)j] = 1;
    }
  }
  if (totals)
    for (int64_t i = 0; i < Nq; i++)
      if (!(totals[i] >= 0) || !std::isfinite(totals[i])) return fail(ctx, HMX_ERR_ARG, "totals must be non-negative and finite (cell " + std::to_string(i) + ")");
  const int esz = data_dtype == HMX_F32 ? 4 : 8;
  const double t0 = now_ms();      // (the timer covers the host's pass over a host-resident matrix)
  if (csr_location == HMX_HOST) {
    int64_t where = 0;
    const int v = proj_validate(indptr, indices, Nq, G_all, &where);
    if (v == 1) return fail(ctx, HMX_ERR_ARG, "indptr is not monotone from 0 (row " + std::to_string(where) + ")");
    if (v == 2) return fail(ctx, HMX_ERR_ARG, "a column index is outside [0, G_all) (entry " + std::to_string(where) + ")");
  }
  CHK(call_device(ctx));

  // ---- the tables: b in fp64, the rest as the kernel's fp32
  const int zs = (d + 63) / 64 * 64;
  std::vector<float> U32((size_t)G * zs, 0.f), inv_sd((size_t)G), cap((size_t)G);
  std::vector<double> b((size_t)d, 0.0);
  for (int32_t j = 0; j < G; j++) {
    inv_sd[(size_t)j] = (float)(1.0 / sd[j]);
    cap[(size_t)j] = clip > 0 ? (float)(mean[j] + clip * sd[j]) : std::numeric_limits<float>::infinity();
    const double c = -mean[j] / sd[j];
    for (int32_t q = 0; q < d; q++) {
      U32[(size_t)j * zs + q] = (float)U[(size_t)j * d + q];
      if (present[(size_t)j]) b[(size_t)q] += c * U[(size_t)j * d + q];
    }
  }

  CallBufs B;
  ProjDev P{};
  int* dslot; float* dU; float* dinv; float* dcap; double* db; double* dtot = nullptr; unsigned* dflag; float* dout;
  HIPCHK(B.get(&dslot, (size_t)G_all)); HIPCHK(B.get(&dU, U32.size())); HIPCHK(B.get(&dinv, (size_t)G)); HIPCHK(B.get(&dcap, (size_t)G));
  HIPCHK(B.get(&db, (size_t)d)); HIPCHK(B.get(&dflag, 1));
  if (totals) HIPCHK(B.get(&dtot, (size_t)Nq));
  if (out_location == HMX_DEVICE) dout = (float*)out; else HIPCHK(B.get(&dout, (size_t)Nq * d));
  hipStream_t st = ctx->L.stream;
  HIPCHK(hipMemcpyAsync(dslot, slot, (size_t)G_all * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dU, U32.data(), U32.size() * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dinv, inv_sd.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dcap, cap.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(db, b.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  if (totals) HIPCHK(hipMemcpyAsync(dtot, totals, (size_t)Nq * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(dflag, 0, sizeof(unsigned), st));
  P.f64 = data_dtype == HMX_F64; P.slot = dslot; P.U = dU; P.inv_sd = dinv; P.cap = dcap; P.b = db; P.totals = dtot; P.scale = scale;
  P.G_all = G_all; P.G = G; P.d = d; P.out = dout; P.flag = dflag;

  CHK(csr_sweep(ctx, B, Nq, indptr, indices, data, esz, csr_location, "project",
                [&](const long long* ptr, long long base, long long nnz, const int* idx, const void* val, long long nrows, long long row0) {
                  P.indptr = ptr; P.base = base; P.nnz = nnz; P.indices = idx; P.data = val; P.nrows = nrows; P.row0 = row0;
                  l_project(ctx->L, P, st);
                }));
  unsigned flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, dflag, sizeof(flag), hipMemcpyDeviceToHost, st));
  if (out_location == HMX_HOST) HIPCHK(hipMemcpyAsync(out, dout, (size_t)Nq * d * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (flag) return fail(ctx, HMX_ERR_ARG, std::string("the count matrix is out of contract: ") + proj_violation(flag));
  ctx->timers["project"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
