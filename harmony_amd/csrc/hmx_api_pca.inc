// hmx_api_pca.inc -- part of hmx_api.cpp (included there, ONE translation unit, behind hmx_api_project.inc whose count-matrix checks and slab
// sweep it uses): hmx_gene_stats, hmx_pca_prepare / apply / release (include/harmony_mi355x_pca.h; DESIGN "Fitting the loadings").
// Kernels: hmx_pca.hip.  The prepared state (ctx->pca) is the only thing these calls leave on the handle.

namespace {

struct PcaState {      // what hmx_pca_prepare leaves: the two lists in HBM and the host's tables
  std::vector<void*> dev;
  int64_t N = 0, entries = 0, nchunks = 0; int32_t G = 0;
  long long* cptr = nullptr; int* cj = nullptr; float* cw = nullptr;          // cell-major
  int* tcell = nullptr; float* tw = nullptr; PcaChunk* chunk = nullptr; int* cstart = nullptr; double* ratio = nullptr;      // gene-major
  std::vector<double> c;      // [G] -mean / sd of the columns a gene maps to, 0 elsewhere
  ~PcaState() { for (void* p : dev) (void)hipFree(p); }
  template <class T> hipError_t get(T** p, size_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) dev.push_back(q);
    *p = (T*)q;
    return e;
  }
};

// the uploads every sweep of a count matrix needs: totals and the flag word
int pca_common(hmx_ctx* ctx, CallBufs& B, ProjDev& P, int64_t N, int32_t G_all, int32_t data_dtype, double scale, const double* totals) {
  double* dtot = nullptr; unsigned* dflag;
  HIPCHK(B.get(&dflag, 1));
  if (totals) {
    HIPCHK(B.get(&dtot, (size_t)N));
    HIPCHK(hipMemcpyAsync(dtot, totals, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->L.stream));
  }
  HIPCHK(hipMemsetAsync(dflag, 0, sizeof(unsigned), ctx->L.stream));
  P.f64 = data_dtype == HMX_F64; P.totals = dtot; P.scale = scale; P.G_all = G_all; P.flag = dflag;
  return 0;
}
int pca_flag(hmx_ctx* ctx, const ProjDev& P) {
  unsigned flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, P.flag, sizeof(flag), hipMemcpyDeviceToHost, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  if (flag) return fail(ctx, HMX_ERR_ARG, std::string("the count matrix is out of contract: ") + proj_violation(flag));
  return 0;
}

}  // namespace

extern "C" {

int hmx_gene_stats(hmx_ctx* ctx, int64_t N, int32_t G_all, const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype,
                   int32_t csr_location, double scale, const double* totals, int64_t* n, double* s1, double* s2, double* step) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(csr_args(ctx, N, G_all, indptr, indices, data, data_dtype, csr_location, scale, totals));
  if (!n || !s1 || !s2) return fail(ctx, HMX_ERR_ARG, "null output");
  if (N < 2) return fail(ctx, HMX_ERR_ARG, "a variance needs at least two cells");
  const double t0 = now_ms();
  if (csr_location == HMX_HOST) CHK(csr_host_pass(ctx, N, G_all, indptr, indices));
  CHK(call_device(ctx));
  // the steps: N values of at most ymax (ymax^2) must add up below 2^62
  const float ymax = totals ? 89.0f : (float)(1.001 * std::log1p(scale));
  const int F1 = std::min(40, (int)std::floor(62.0 - std::log2((double)N * ymax)));
  const int F2 = std::min(40, (int)std::floor(62.0 - std::log2((double)N * ymax * ymax)));
  CallBufs B;
  PcaStatDev S{};
  CHK(pca_common(ctx, B, S.C, N, G_all, data_dtype, scale, totals));
  unsigned long long* acc;
  HIPCHK(B.get(&acc, (size_t)3 * G_all));
  HIPCHK(hipMemsetAsync(acc, 0, (size_t)3 * G_all * sizeof(unsigned long long), ctx->L.stream));
  S.ymax = ymax; S.q1 = std::ldexp(1.0, F1); S.q2 = std::ldexp(1.0, F2); S.s1 = acc; S.s2 = acc + G_all; S.n = acc + 2 * (size_t)G_all;
  hipStream_t st = ctx->L.stream;
  CHK(csr_sweep(ctx, B, N, indptr, indices, data, data_dtype == HMX_F32 ? 4 : 8, csr_location, "gene_stats",
                [&](const long long* ptr, long long base, long long nnz, const int* idx, const void* val, long long nrows, long long row0) {
                  S.C.indptr = ptr; S.C.base = base; S.C.nnz = nnz; S.C.indices = idx; S.C.data = val; S.C.nrows = nrows; S.C.row0 = row0;
                  l_gene_stats(S, st);
                }));
  std::vector<unsigned long long> h((size_t)3 * G_all);
  HIPCHK(hipMemcpyAsync(h.data(), acc, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  CHK(pca_flag(ctx, S.C));
  for (int32_t g = 0; g < G_all; g++) {
    s1[g] = std::ldexp((double)h[(size_t)g], -F1);
    s2[g] = std::ldexp((double)h[(size_t)G_all + g], -F2);
    n[g] = (int64_t)h[2 * (size_t)G_all + g];
  }
  if (step) { step[0] = std::ldexp(1.0, -F1); step[1] = std::ldexp(1.0, -F2); }
  ctx->timers["gene_stats"] = now_ms() - t0;
  return 0;
}

int hmx_pca_release(hmx_ctx* ctx) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (ctx->pca && ctx->device >= 0) (void)hipSetDevice(ctx->device);
  ctx->pca.reset();
  ctx->pca_entries = 0;
  return 0;
}

int hmx_pca_prepare(hmx_ctx* ctx, int64_t N, int32_t G_all, const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype,
                    int32_t csr_location, const int32_t* slot, const double* mean, const double* sd, int32_t G, double scale, double clip,
                    const double* totals) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(csr_args(ctx, N, G_all, indptr, indices, data, data_dtype, csr_location, scale, totals));
  if (!slot || !mean || !sd) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (G <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (G > 16384) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: G <= 16384 chosen genes");
  if (std::isnan(clip) || std::isinf(clip)) return fail(ctx, HMX_ERR_ARG, "clip must be finite (<= 0: none)");
  for (int32_t j = 0; j < G; j++) {
    if (!(sd[j] > 0) || !std::isfinite(sd[j])) return fail(ctx, HMX_ERR_ARG, "sd must be positive and finite (gene " + std::to_string(j) + ")");
    if (!(mean[j] >= 0) || !std::isfinite(mean[j])) return fail(ctx, HMX_ERR_ARG, "mean must be non-negative and finite (gene " + std::to_string(j) + ")");
  }
  std::vector<char> present((size_t)G, 0);
  for (int32_t g = 0; g < G_all; g++) {
    const int32_t j = slot[g];
    if (j < -1 || j >= G) return fail(ctx, HMX_ERR_ARG, "slot[" + std::to_string(g) + "] = " + std::to_string(j) + " is outside -1 .. G - 1");
    if (j >= 0) {
      if (present[(size_t)j]) return fail(ctx, HMX_ERR_ARG, "slot maps two genes to column " + std::to_string(j));
      present[(size_t)j] = 1;
    }
  }
  const double t0 = now_ms();
  if (csr_location == HMX_HOST) CHK(csr_host_pass(ctx, N, G_all, indptr, indices));
  CHK(call_device(ctx));
  hmx_pca_release(ctx);
  hipStream_t st = ctx->L.stream;
  const int esz = data_dtype == HMX_F32 ? 4 : 8;

  std::shared_ptr<PcaState> Sp = std::make_shared<PcaState>();
  PcaState& S = *Sp;
  S.N = N; S.G = G; S.c.assign((size_t)G, 0.0);
  std::vector<float> inv_sd((size_t)G), cap((size_t)G);
  std::vector<double> ratio((size_t)G, 0.0);
  for (int32_t j = 0; j < G; j++) {      // (the fp32 tables exactly as hmx_project_counts builds them)
    inv_sd[(size_t)j] = (float)(1.0 / sd[j]);
    cap[(size_t)j] = clip > 0 ? (float)(mean[j] + clip * sd[j]) : std::numeric_limits<float>::infinity();
    if (present[(size_t)j]) { S.c[(size_t)j] = -mean[j] / sd[j]; ratio[(size_t)j] = mean[j] / sd[j]; }
  }
  {
    CallBufs B;
    PcaCompactDev Cd{};
    CHK(pca_common(ctx, B, Cd.C, N, G_all, data_dtype, scale, totals));
    int* dslot; float* dinv; float* dcap; long long* dcnt;
    HIPCHK(B.get(&dslot, (size_t)G_all)); HIPCHK(B.get(&dinv, (size_t)G)); HIPCHK(B.get(&dcap, (size_t)G)); HIPCHK(B.get(&dcnt, (size_t)N));
    HIPCHK(hipMemcpyAsync(dslot, slot, (size_t)G_all * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dinv, inv_sd.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dcap, cap.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice, st));
    Cd.C.slot = dslot; Cd.C.inv_sd = dinv; Cd.C.cap = dcap; Cd.C.G = G; Cd.cnt = dcnt;
    auto sweep = [&](bool fill) {
      CallBufs staging;      // (a pass returns with its streams drained: the staging sets of the count pass are gone before the fill pass allocates its own)
      return csr_sweep(ctx, staging, N, indptr, indices, data, esz, csr_location, "pca_prepare",
                       [&](const long long* ptr, long long base, long long nnz, const int* idx, const void* val, long long nrows, long long row0) {
                         Cd.C.indptr = ptr; Cd.C.base = base; Cd.C.nnz = nnz; Cd.C.indices = idx; Cd.C.data = val; Cd.C.nrows = nrows; Cd.C.row0 = row0;
                         l_pca_compact(Cd, fill, st);
                       });
    };
    // ---- count, scan (host), fill
    CHK(sweep(false));
    std::vector<long long> cptr((size_t)N + 1);
    HIPCHK(hipMemcpyAsync(cptr.data() + 1, dcnt, (size_t)N * sizeof(long long), hipMemcpyDeviceToHost, st));
    CHK(pca_flag(ctx, Cd.C));
    cptr[0] = 0;
    for (int64_t i = 0; i < N; i++) cptr[(size_t)i + 1] += cptr[(size_t)i];
    S.entries = cptr[(size_t)N];
    HIPCHK(S.get(&S.cptr, (size_t)N + 1)); HIPCHK(S.get(&S.cj, (size_t)S.entries)); HIPCHK(S.get(&S.cw, (size_t)S.entries));
    HIPCHK(hipMemcpyAsync(S.cptr, cptr.data(), ((size_t)N + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(S.cj, 0, (size_t)S.entries * sizeof(int), st));      // (a host matrix that changes between the two passes leaves defined entries: column 0, w = 0)
    HIPCHK(hipMemsetAsync(S.cw, 0, (size_t)S.entries * sizeof(float), st));
    Cd.cptr = S.cptr; Cd.entries = S.entries; Cd.cj = S.cj; Cd.cw = S.cw;
    CHK(sweep(true));
    CHK(pca_flag(ctx, Cd.C));
  }
  {
    // ---- the same entries gene-major: histogram per tile, scan per gene, the genes' segments (host), one wave per tile places its cells in order
    CallBufs B;
    PcaListDev T{};
    T.cptr = S.cptr; T.cj = S.cj; T.cw = S.cw; T.N = N; T.G = G; T.ntiles = (N + PCA_TILE - 1) / PCA_TILE;
    long long* dglen; long long* dgptr;
    HIPCHK(B.get(&T.hist, (size_t)T.ntiles * G)); HIPCHK(B.get(&dglen, (size_t)G)); HIPCHK(B.get(&dgptr, (size_t)G + 1));
    T.glen = dglen;
    l_pca_transpose_count(T, st); KCHK();
    std::vector<long long> gptr((size_t)G + 1);
    HIPCHK(hipMemcpyAsync(gptr.data() + 1, dglen, (size_t)G * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    gptr[0] = 0;
    std::vector<PcaChunk> chunk; std::vector<int> cstart((size_t)G + 1, 0);
    for (int32_t j = 0; j < G; j++) {
      const long long len = gptr[(size_t)j + 1];
      gptr[(size_t)j + 1] += gptr[(size_t)j];
      for (long long o = 0; o < len; o += PCA_CHUNK) chunk.push_back({j, (int)std::min<long long>(PCA_CHUNK, len - o), gptr[(size_t)j] + o});
      cstart[(size_t)j + 1] = (int)chunk.size();
    }
    if (gptr[(size_t)G] != S.entries) return fail(ctx, HMX_ERR_DEVICE, "pca_prepare: the two lists disagree");
    S.nchunks = (int64_t)chunk.size();
    HIPCHK(S.get(&S.tcell, (size_t)S.entries)); HIPCHK(S.get(&S.tw, (size_t)S.entries)); HIPCHK(S.get(&S.chunk, chunk.size()));
    HIPCHK(S.get(&S.cstart, (size_t)G + 1)); HIPCHK(S.get(&S.ratio, (size_t)G));
    HIPCHK(hipMemsetAsync(S.tcell, 0, (size_t)S.entries * sizeof(int), st));      // (a row that names a gene twice leaves slots unplaced: they read cell 0, w = 0)
    HIPCHK(hipMemsetAsync(S.tw, 0, (size_t)S.entries * sizeof(float), st));
    HIPCHK(hipMemcpyAsync(dgptr, gptr.data(), ((size_t)G + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    if (!chunk.empty()) HIPCHK(hipMemcpyAsync(S.chunk, chunk.data(), chunk.size() * sizeof(PcaChunk), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S.cstart, cstart.data(), cstart.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S.ratio, ratio.data(), (size_t)G * sizeof(double), hipMemcpyHostToDevice, st));
    T.gptr = dgptr; T.tcell = S.tcell; T.tw = S.tw;
    l_pca_transpose_place(T, st); KCHK();
    HIPCHK(hipStreamSynchronize(st));
  }
  ctx->pca = Sp;
  ctx->pca_entries = S.entries;
  ctx->timers["pca_prepare"] = now_ms() - t0;
  return 0;
}

int hmx_pca_apply(hmx_ctx* ctx, const double* V, int32_t k, double* W, void* P, int32_t P_location) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!ctx->pca) return fail(ctx, HMX_ERR_STATE, "no prepared matrix on this handle: hmx_pca_prepare first");
  if (!V || !W) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (k <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (k > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: k <= 128");
  if (P && P_location != HMX_HOST && P_location != HMX_DEVICE) return fail(ctx, HMX_ERR_ARG, "a location must be HMX_HOST or HMX_DEVICE");
  const PcaState& S = *std::static_pointer_cast<PcaState>(ctx->pca);
  const int32_t G = S.G; const int64_t N = S.N;
  for (int64_t i = 0; i < (int64_t)G * k; i++) if (!std::isfinite(V[i])) return fail(ctx, HMX_ERR_ARG, "V must be finite");
  const double t0 = now_ms();
  CHK(call_device(ctx));
  hipStream_t st = ctx->L.stream;
  const int zs = (k + 63) / 64 * 64;
  std::vector<float> V32((size_t)G * zs, 0.f);
  std::vector<double> b((size_t)k, 0.0);
  for (int32_t j = 0; j < G; j++) {      // (b in the order hmx_project_counts adds it)
    const double c = S.c[(size_t)j];
    for (int32_t q = 0; q < k; q++) {
      V32[(size_t)j * zs + q] = (float)V[(size_t)j * k + q];
      if (c != 0.0) b[(size_t)q] += c * V[(size_t)j * k + q];
    }
  }
  CallBufs B;
  PcaApplyDev A{};
  float* dV; double* db; double* dW; float* dout = nullptr;
  A.N = N; A.G = G; A.k = k; A.zs = zs; A.nranges = (N + PCA_COLSUM_ROWS - 1) / PCA_COLSUM_ROWS; A.nchunks = S.nchunks;
  HIPCHK(B.get(&dV, V32.size())); HIPCHK(B.get(&db, (size_t)k)); HIPCHK(B.get(&dW, (size_t)G * k));
  HIPCHK(B.get(&A.Ppad, (size_t)N * zs)); HIPCHK(B.get(&A.colpart, (size_t)A.nranges * zs)); HIPCHK(B.get(&A.colsum, (size_t)zs));
  HIPCHK(B.get(&A.part, (size_t)S.nchunks * zs));
  if (P) { if (P_location == HMX_DEVICE) dout = (float*)P; else HIPCHK(B.get(&dout, (size_t)N * k)); }
  HIPCHK(hipMemcpyAsync(dV, V32.data(), V32.size() * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(db, b.data(), (size_t)k * sizeof(double), hipMemcpyHostToDevice, st));
  A.cptr = S.cptr; A.cj = S.cj; A.cw = S.cw; A.V = dV; A.b = db; A.out = dout; A.tcell = S.tcell; A.tw = S.tw; A.chunk = S.chunk; A.cstart = S.cstart;
  A.ratio = S.ratio; A.W = dW;
  l_pca_apply(A, st); KCHK();
  HIPCHK(hipMemcpyAsync(W, dW, (size_t)G * k * sizeof(double), hipMemcpyDeviceToHost, st));
  if (P && P_location == HMX_HOST) HIPCHK(hipMemcpyAsync(P, dout, (size_t)N * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  ctx->timers["pca_apply"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
