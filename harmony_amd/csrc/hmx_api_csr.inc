// hmx_api_csr.inc -- part of hmx_api.cpp (included there, ONE translation unit, behind hmx_api_call.inc and ahead of the four sections that read
// a count matrix: project, pca, groups, ranksum): the count-matrix seam.  The checks of a CSR matrix's description, the host's pass over a
// host-resident one, the sweep that shows a kernel its rows (at once, or slab by slab through two staging sets), the uploads and the flag word
// every sweep needs, and the tables the calls must build alike: a gene map, 1 / sd and the clip, the fixed-point steps of the gene sums.

namespace {

constexpr int64_t CSR_SLAB_BYTES = (int64_t)256 << 20;      // index + value bytes of a staging slab (the "project_slab_bytes" lab field overrides it)

struct CsrSlab { int64_t row0, row1; };      // cells [row0, row1)

// Slabs of whole cells whose stored entries fit `cap` entries; a cell longer than that gets a slab of its own.
std::vector<CsrSlab> csr_slabs(const int64_t* indptr, int64_t N, int64_t cap) {
  std::vector<CsrSlab> S;
  for (int64_t r = 0; r < N;) {
    int64_t e = r + 1;
    while (e < N && indptr[e + 1] - indptr[r] <= cap) e++;
    S.push_back({r, e});
    r = e;
  }
  return S;
}
// the entries of a slab of the handle's sweeps, for elements of esz bytes
int64_t csr_slab_cap(const hmx_ctx* ctx, int esz) {
  return std::max<int64_t>(1, (ctx->project_slab_bytes > 0 ? ctx->project_slab_bytes : CSR_SLAB_BYTES) / (4 + esz));
}

// host CSR: indptr monotone from 0, every column in [0, G_all).  0, or 1 / 2 with the offending position in *where
int csr_validate(const int64_t* indptr, const int32_t* indices, int64_t N, int32_t G_all, int64_t* where) {
  if (indptr[0] != 0) { *where = 0; return 1; }
  for (int64_t i = 0; i < N; i++) if (indptr[i + 1] < indptr[i]) { *where = i; return 1; }
  const int64_t nnz = indptr[N];
  unsigned nt = std::thread::hardware_concurrency(); if (nt < 1) nt = 1; if (nt > 16) nt = 16;
  if (nnz < (int64_t)1 << 22) nt = 1;
  std::vector<int64_t> first((size_t)nt, -1);
  auto run = [&first, indices, G_all, nnz, nt](unsigned t) {      // (the scan's operands by value: the loop keeps them in registers)
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

const char* csr_violation(unsigned flag) {
  if (flag & PROJ_BAD_INDPTR) return "indptr is not monotone within [0, nnz]";
  if (flag & PROJ_BAD_COLUMN) return "a column index is outside [0, G_all)";
  if (flag & PROJ_BAD_NEGATIVE) return "a stored value is negative";
  return "a stored value is not finite";
}

// the rows one launch of a sweep reads, as ProjDev names them
struct CsrRows {
  const long long* ptr; long long base, nnz; const int* idx; const void* val; long long nrows, row0;
  void into(ProjDev& P) const { P.indptr = ptr; P.base = base; P.nnz = nnz; P.indices = idx; P.data = val; P.nrows = nrows; P.row0 = row0; }
};

// One pass over a CSR matrix of `N` rows: launch(CsrRows) once for a device-resident matrix, once per slab of whole cells for a host-resident
// one -- two sets of staging buffers (owned by `B`; bytes, the element size is a run-time value), the copy of slab t + 1 (upload stream) beside
// the kernel of slab t.  Returns with both streams drained.
template <class F>
int csr_sweep(hmx_ctx* ctx, CallBufs& B, int64_t N, const int64_t* indptr, const int32_t* indices, const void* data, int esz, int32_t csr_location,
              const char* what, F launch) {
  hipStream_t st = ctx->L.stream;
  if (csr_location == HMX_DEVICE) {
    long long nnz = 0;
    HIPCHK(download(&nnz, indptr + N, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nnz < 0) return fail(ctx, HMX_ERR_ARG, "indptr[Nq] is negative");
    launch(CsrRows{(const long long*)indptr, 0, nnz, indices, data, (long long)N, 0}); KCHK();
    return 0;
  }
  // ---- slabs of whole cells through two sets of staging buffers
  const std::vector<CsrSlab> S = csr_slabs(indptr, N, csr_slab_cap(ctx, esz));
  int64_t max_nnz = 1, max_rows = 1;
  for (const CsrSlab& s : S) { max_nnz = std::max(max_nnz, indptr[s.row1] - indptr[s.row0]); max_rows = std::max(max_rows, s.row1 - s.row0); }
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
    if (e == hipSuccess) e = upload(sptr[s], indptr + r0, (size_t)(nr + 1), Y.up);
    if (e == hipSuccess) e = upload(sidx[s], indices + base, (size_t)cnt, Y.up);
    if (e == hipSuccess) e = upload(sval[s], (const char*)data + (size_t)base * esz, (size_t)cnt * esz, Y.up);
    if (e == hipSuccess) e = hipEventRecord(Y.uploaded[s], Y.up);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, Y.uploaded[s], 0);
    if (e != hipSuccess) break;
    launch(CsrRows{sptr[s], base, cnt, sidx[s], sval[s], nr, r0});
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
  const int v = csr_validate(indptr, indices, N, G_all, &where);
  if (v == 1) return fail(ctx, HMX_ERR_ARG, "indptr is not monotone from 0 (row " + std::to_string(where) + ")");
  if (v == 2) return fail(ctx, HMX_ERR_ARG, "a column index is outside [0, G_all) (entry " + std::to_string(where) + ")");
  return 0;
}

// the uploads every sweep of a count matrix needs: totals and the flag word; and the flag word read back (it synchronises)
int csr_uploads(hmx_ctx* ctx, CallBufs& B, ProjDev& P, int64_t N, int32_t G_all, int32_t data_dtype, double scale, const double* totals) {
  double* dtot = nullptr; unsigned* dflag;
  HIPCHK(B.get(&dflag, 1));
  if (totals) HIPCHK(B.put(&dtot, totals, (size_t)N, ctx->L.stream));
  HIPCHK(zero_fill(dflag, 1, ctx->L.stream));
  P.f64 = data_dtype == HMX_F64; P.totals = dtot; P.scale = scale; P.G_all = G_all; P.flag = dflag;
  return 0;
}
int csr_flag(hmx_ctx* ctx, const ProjDev& P) {
  unsigned flag = 0;
  HIPCHK(download(&flag, P.flag, 1, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  if (flag) return fail(ctx, HMX_ERR_ARG, std::string("the count matrix is out of contract: ") + csr_violation(flag));
  return 0;
}

// a gene map slot [G_all] -> -1 .. G - 1, one to one where it is not -1.  `name`: the argument, `pairs`: what two genes on one target are
// called ("genes to column").  present [G]: 1 where a gene maps to the target
int gene_slot_check(hmx_ctx* ctx, const int32_t* slot, int32_t G_all, int32_t G, const char* name, const char* pairs, std::vector<char>& present) {
  present.assign((size_t)G, 0);
  for (int32_t g = 0; g < G_all; g++) {
    const int32_t j = slot[g];
    if (j < -1 || j >= G) return fail(ctx, HMX_ERR_ARG, std::string(name) + "[" + std::to_string(g) + "] = " + std::to_string(j) + " is outside -1 .. G - 1");
    if (j >= 0) {
      if (present[(size_t)j]) return fail(ctx, HMX_ERR_ARG, std::string(name) + " maps two " + pairs + " " + std::to_string(j));
      present[(size_t)j] = 1;
    }
  }
  return 0;
}

// the standardisation's tables: the checks of mean and sd [G] (`gene`: what an entry is called in the error), clip, and the kernels' fp32
// 1 / sd and mean + clip sd (+inf: no clip) -- ONE function, so that projection and PCA standardise alike
int gene_moments_check(hmx_ctx* ctx, const double* mean, const double* sd, int32_t G, const char* gene) {
  for (int32_t j = 0; j < G; j++) {
    if (!(sd[j] > 0) || !std::isfinite(sd[j])) return fail(ctx, HMX_ERR_ARG, std::string("sd must be positive and finite (") + gene + " " + std::to_string(j) + ")");
    if (!(mean[j] >= 0) || !std::isfinite(mean[j])) return fail(ctx, HMX_ERR_ARG, std::string("mean must be non-negative and finite (") + gene + " " + std::to_string(j) + ")");
  }
  return 0;
}
void gene_tables(const double* mean, const double* sd, int32_t G, double clip, std::vector<float>& inv_sd, std::vector<float>& cap) {
  inv_sd.resize((size_t)G); cap.resize((size_t)G);
  for (int32_t j = 0; j < G; j++) {
    inv_sd[(size_t)j] = (float)(1.0 / sd[j]);
    cap[(size_t)j] = clip > 0 ? (float)(mean[j] + clip * sd[j]) : std::numeric_limits<float>::infinity();
  }
}

// the fixed-point steps of the gene sums: N values of at most ymax (ymax^2) must add up below 2^62.  From the WHOLE N, grouped or not: group
// sums and ungrouped sums are multiples of the same step
struct GeneSteps { float ymax; int F1, F2; };
GeneSteps gene_steps(int64_t N, double scale, bool has_totals) {
  GeneSteps T;
  T.ymax = has_totals ? 89.0f : (float)(1.001 * std::log1p(scale));
  T.F1 = std::min(40, (int)std::floor(62.0 - std::log2((double)N * T.ymax)));
  T.F2 = std::min(40, (int)std::floor(62.0 - std::log2((double)N * T.ymax * T.ymax)));
  return T;
}

}  // namespace
