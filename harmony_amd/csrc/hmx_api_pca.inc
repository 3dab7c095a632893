// hmx_api_pca.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_gene_stats, hmx_pca_prepare / apply / release
// (include/harmony_mi355x_pca.h; DESIGN "Fitting the loadings").  Kernels: hmx_pca.hip.  The count matrix's checks, sweep and tables are the
// count-matrix seam's (hmx_api_csr.inc).  The prepared state (ctx->pca) is the only thing these calls leave on the handle.

namespace {

struct PcaState {      // what hmx_pca_prepare leaves: the two lists in HBM and the host's tables
  CallBufs dev;      // (they live until hmx_pca_release)
  int64_t N = 0, entries = 0, nchunks = 0; int32_t G = 0;
  long long* cptr = nullptr; int* cj = nullptr; float* cw = nullptr;          // cell-major
  int* tcell = nullptr; float* tw = nullptr; PcaChunk* chunk = nullptr; int* cstart = nullptr; double* ratio = nullptr;      // gene-major
  std::vector<double> c;      // [G] -mean / sd of the columns a gene maps to, 0 elsewhere
};

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
  const GeneSteps T = gene_steps(N, scale, totals != nullptr);
  const int F1 = T.F1, F2 = T.F2;
  CallBufs B;
  PcaStatDev S{};
  CHK(csr_uploads(ctx, B, S.C, N, G_all, data_dtype, scale, totals));
  hipStream_t st = ctx->L.stream;
  unsigned long long* acc;
  HIPCHK(B.get(&acc, (size_t)3 * G_all));
  HIPCHK(zero_fill(acc, (size_t)3 * G_all, st));
  S.ymax = T.ymax; S.q1 = std::ldexp(1.0, F1); S.q2 = std::ldexp(1.0, F2); S.s1 = acc; S.s2 = acc + G_all; S.n = acc + 2 * (size_t)G_all;
  CHK(csr_sweep(ctx, B, N, indptr, indices, data, data_dtype == HMX_F32 ? 4 : 8, csr_location, "gene_stats",
                [&](const CsrRows& R) { R.into(S.C); l_gene_stats(S, st); }));
  std::vector<unsigned long long> h((size_t)3 * G_all);
  HIPCHK(download(h.data(), acc, h.size(), st));
  CHK(csr_flag(ctx, S.C));
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
  CHK(gene_moments_check(ctx, mean, sd, G, "gene"));
  std::vector<char> present;
  CHK(gene_slot_check(ctx, slot, G_all, G, "slot", "genes to column", present));
  const double t0 = now_ms();
  if (csr_location == HMX_HOST) CHK(csr_host_pass(ctx, N, G_all, indptr, indices));
  CHK(call_device(ctx));
  hmx_pca_release(ctx);
  hipStream_t st = ctx->L.stream;
  const int esz = data_dtype == HMX_F32 ? 4 : 8;

  std::shared_ptr<PcaState> Sp = std::make_shared<PcaState>();
  PcaState& S = *Sp;
  S.N = N; S.G = G; S.c.assign((size_t)G, 0.0);
  std::vector<float> inv_sd, cap;
  std::vector<double> ratio((size_t)G, 0.0);
  gene_tables(mean, sd, G, clip, inv_sd, cap);      // (the fp32 tables of hmx_project_counts)
  for (int32_t j = 0; j < G; j++)
    if (present[(size_t)j]) { S.c[(size_t)j] = -mean[j] / sd[j]; ratio[(size_t)j] = mean[j] / sd[j]; }
  {
    CallBufs B;
    PcaCompactDev Cd{};
    CHK(csr_uploads(ctx, B, Cd.C, N, G_all, data_dtype, scale, totals));
    int* dslot; float* dinv; float* dcap; long long* dcnt;
    HIPCHK(B.put(&dslot, slot, (size_t)G_all, st)); HIPCHK(B.put(&dinv, inv_sd.data(), (size_t)G, st)); HIPCHK(B.put(&dcap, cap.data(), (size_t)G, st));
    HIPCHK(B.get(&dcnt, (size_t)N));
    Cd.C.slot = dslot; Cd.C.inv_sd = dinv; Cd.C.cap = dcap; Cd.C.G = G; Cd.cnt = dcnt;
    auto sweep = [&](bool fill) {
      CallBufs staging;      // (a pass returns with its streams drained: the staging sets of the count pass are gone before the fill pass allocates its own)
      return csr_sweep(ctx, staging, N, indptr, indices, data, esz, csr_location, "pca_prepare",
                       [&](const CsrRows& R) { R.into(Cd.C); l_pca_compact(Cd, fill, st); });
    };
    // ---- count, scan (host), fill
    CHK(sweep(false));
    std::vector<long long> cptr((size_t)N + 1);
    HIPCHK(download(cptr.data() + 1, dcnt, (size_t)N, st));
    CHK(csr_flag(ctx, Cd.C));
    cptr[0] = 0;
    for (int64_t i = 0; i < N; i++) cptr[(size_t)i + 1] += cptr[(size_t)i];
    S.entries = cptr[(size_t)N];
    HIPCHK(S.dev.put(&S.cptr, cptr.data(), (size_t)N + 1, st)); HIPCHK(S.dev.get(&S.cj, (size_t)S.entries)); HIPCHK(S.dev.get(&S.cw, (size_t)S.entries));
    HIPCHK(zero_fill(S.cj, (size_t)S.entries, st));      // (a host matrix that changes between the two passes leaves defined entries: column 0, w = 0)
    HIPCHK(zero_fill(S.cw, (size_t)S.entries, st));
    Cd.cptr = S.cptr; Cd.entries = S.entries; Cd.cj = S.cj; Cd.cw = S.cw;
    CHK(sweep(true));
    CHK(csr_flag(ctx, Cd.C));
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
    HIPCHK(download(gptr.data() + 1, dglen, (size_t)G, st));
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
    HIPCHK(S.dev.get(&S.tcell, (size_t)S.entries)); HIPCHK(S.dev.get(&S.tw, (size_t)S.entries));
    HIPCHK(zero_fill(S.tcell, (size_t)S.entries, st));      // (a row that names a gene twice leaves slots unplaced: they read cell 0, w = 0)
    HIPCHK(zero_fill(S.tw, (size_t)S.entries, st));
    HIPCHK(upload(dgptr, gptr.data(), (size_t)G + 1, st));
    HIPCHK(S.dev.put(&S.chunk, chunk.data(), chunk.size(), st));
    HIPCHK(S.dev.put(&S.cstart, cstart.data(), cstart.size(), st)); HIPCHK(S.dev.put(&S.ratio, ratio.data(), (size_t)G, st));
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
  HIPCHK(B.put(&dV, V32.data(), V32.size(), st)); HIPCHK(B.put(&db, b.data(), (size_t)k, st)); HIPCHK(B.get(&dW, (size_t)G * k));
  HIPCHK(B.get(&A.Ppad, (size_t)N * zs)); HIPCHK(B.get(&A.colpart, (size_t)A.nranges * zs)); HIPCHK(B.get(&A.colsum, (size_t)zs));
  HIPCHK(B.get(&A.part, (size_t)S.nchunks * zs));
  if (P) { if (P_location == HMX_DEVICE) dout = (float*)P; else HIPCHK(B.get(&dout, (size_t)N * k)); }
  A.cptr = S.cptr; A.cj = S.cj; A.cw = S.cw; A.V = dV; A.b = db; A.out = dout; A.tcell = S.tcell; A.tw = S.tw; A.chunk = S.chunk; A.cstart = S.cstart;
  A.ratio = S.ratio; A.W = dW;
  l_pca_apply(A, st); KCHK();
  HIPCHK(download(W, dW, (size_t)G * k, st));
  if (P && P_location == HMX_HOST) HIPCHK(download((float*)P, dout, (size_t)N * k, st));
  HIPCHK(hipStreamSynchronize(st));
  ctx->timers["pca_apply"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
