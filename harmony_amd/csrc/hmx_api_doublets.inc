// hmx_api_doublets.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_simulate_doublets and hmx_doublet_neighbors
// (include/harmony_mi355x_doublets.h; DESIGN "Doublet detection").  Kernels: hmx_doublets.hip; launch plan: hmx_doublet_plan.h.  The count
// matrix's checks and tables are the count-matrix seam's (hmx_api_csr.inc), the search is the call seam's (knn_front, hmx_api_call.inc).
// Both calls keep no state on the handle but the timers: every device buffer lives for one call.

extern "C" {

int hmx_simulate_doublets(hmx_ctx* ctx, int64_t N, int32_t G_all, const int64_t* indptr, const int32_t* indices, const void* data,
                          int32_t data_dtype, int32_t csr_location, const int32_t* slot, const double* U, const double* mean, const double* sd,
                          int32_t G, int32_t d, double scale, double clip, const double* totals, int64_t n_sim, const int64_t* pairs,
                          void* out, int32_t out_location) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(csr_args(ctx, N, G_all, indptr, indices, data, data_dtype, csr_location, scale, totals));
  if (!slot || !U || !mean || !sd || !pairs || !out) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (G <= 0 || d <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (n_sim < 1) return fail(ctx, HMX_ERR_ARG, "n_sim must be at least 1");
  if (out_location != HMX_HOST && out_location != HMX_DEVICE) return fail(ctx, HMX_ERR_ARG, "a location must be HMX_HOST or HMX_DEVICE");
  if (n_sim > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 synthetic cells");
  DoubletPlan plan;
  const int ps = doublet_plan(G, d, n_sim, plan);
  if (ps == DBL_PLAN_PCS) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= " + std::to_string(DBL_MAX_D));
  if (ps == DBL_PLAN_GENES)
    return fail(ctx, HMX_ERR_LIMIT, "supported envelope: G <= " + std::to_string(DBL_MAX_GENES) + " reference genes (a wave's slot table lives in " +
                                        std::to_string(DBL_LDS_BYTES / 1024) + " KB of LDS)");
  if (ps != DBL_PLAN_OK) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (std::isnan(clip) || std::isinf(clip)) return fail(ctx, HMX_ERR_ARG, "clip must be finite (<= 0: none)");
  CHK(gene_moments_check(ctx, mean, sd, G, "reference gene"));
  for (int64_t i = 0; i < (int64_t)G * d; i++) if (!std::isfinite(U[i])) return fail(ctx, HMX_ERR_ARG, "the loadings must be finite");
  std::vector<char> present;
  CHK(gene_slot_check(ctx, slot, G_all, G, "slot", "query genes to reference gene", present));
  for (int64_t s = 0; s < 2 * n_sim; s++)
    if (pairs[s] < 0 || pairs[s] >= N)
      return fail(ctx, HMX_ERR_ARG, "pairs[" + std::to_string(s / 2) + "][" + std::to_string(s % 2) + "] = " + std::to_string(pairs[s]) + " is outside [0, N)");
  const int esz = data_dtype == HMX_F32 ? 4 : 8;
  const double t0 = now_ms();      // (the timer covers the host's pass over a host-resident matrix)
  if (csr_location == HMX_HOST) CHK(csr_host_pass(ctx, N, G_all, indptr, indices));
  CHK(call_device(ctx));

  // ---- the tables, as hmx_project_counts builds them: b in fp64, the rest as the kernel's fp32
  const int zs = (d + 63) / 64 * 64;
  std::vector<float> U32((size_t)G * zs, 0.f), inv_sd, cap;
  std::vector<double> b((size_t)d, 0.0);
  gene_tables(mean, sd, G, clip, inv_sd, cap);
  for (int32_t j = 0; j < G; j++) {
    const double c = -mean[j] / sd[j];
    for (int32_t q = 0; q < d; q++) {
      U32[(size_t)j * zs + q] = (float)U[(size_t)j * d + q];
      if (present[(size_t)j]) b[(size_t)q] += c * U[(size_t)j * d + q];
    }
  }

  CallBufs B;
  DoubletDev D{};
  ProjDev& P = D.C;
  hipStream_t st = ctx->L.stream;
  int* dslot; float* dU; float* dinv; float* dcap; double* db; float* dout; long long* dpairs;
  HIPCHK(B.put(&dslot, slot, (size_t)G_all, st)); HIPCHK(B.put(&dU, U32.data(), U32.size(), st)); HIPCHK(B.put(&dinv, inv_sd.data(), (size_t)G, st));
  HIPCHK(B.put(&dcap, cap.data(), (size_t)G, st)); HIPCHK(B.put(&db, b.data(), (size_t)d, st));
  HIPCHK(B.put(&dpairs, pairs, (size_t)n_sim * 2, st));
  CHK(csr_uploads(ctx, B, P, N, G_all, data_dtype, scale, totals));
  if (out_location == HMX_DEVICE) dout = (float*)out; else HIPCHK(B.get(&dout, (size_t)n_sim * d));

  // ---- the matrix: where it lives, or the WHOLE of it in call-scoped buffers (a pair's parents are arbitrary rows: no slabs of whole cells)
  long long nnz = 0;
  if (csr_location == HMX_DEVICE) {
    HIPCHK(download(&nnz, indptr + N, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nnz < 0) return fail(ctx, HMX_ERR_ARG, "indptr[N] is negative");
    P.indptr = (const long long*)indptr; P.indices = indices; P.data = data;
  } else {
    nnz = indptr[N];
    const double bytes = (double)nnz * (4 + esz) + ((double)N + 1) * 8;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (bytes > (double)free_b)
      return fail(ctx, HMX_ERR_LIMIT, "the count matrix (" + std::to_string((long long)(bytes / 1048576.0) + 1) + " MB) does not fit the " +
                                          std::to_string((long long)(free_b >> 20)) + " MB of free device memory: the simulation reads arbitrary rows and needs it whole");
    long long* dptr; int* didx; char* dval;
    HIPCHK(B.get(&dptr, (size_t)N + 1)); HIPCHK(B.get(&didx, (size_t)nnz)); HIPCHK(B.get(&dval, (size_t)nnz * esz));
    const size_t chunk = (size_t)csr_slab_cap(ctx, esz);      // entries of a copy
    HIPCHK(upload(dptr, indptr, (size_t)N + 1, st));
    for (size_t e = 0; e < (size_t)nnz; e += chunk) {
      const size_t n = std::min(chunk, (size_t)nnz - e);
      HIPCHK(upload(didx + e, indices + e, n, st));
      HIPCHK(upload(dval + e * esz, (const char*)data + e * esz, n * esz, st));
    }
    P.indptr = dptr; P.indices = didx; P.data = dval;
  }
  P.base = 0; P.nnz = nnz; P.nrows = N; P.row0 = 0;
  P.slot = dslot; P.U = dU; P.inv_sd = dinv; P.cap = dcap; P.b = db; P.G = G; P.d = d; P.out = dout;
  D.pairs = dpairs; D.n_sim = n_sim; D.gp = plan.gp;

  l_doublet_project(ctx->L, D, plan, st); KCHK();
  if (out_location == HMX_HOST) HIPCHK(download((float*)out, dout, (size_t)n_sim * d, st));
  CHK(csr_flag(ctx, P));
  ctx->timers["simulate_doublets"] = now_ms() - t0;
  return 0;
}

int hmx_doublet_neighbors(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t n_obs, int64_t n_sim, int32_t d, int32_t k_adj,
                          int32_t* n_sim_neighbors_out, int32_t* knn_idx_out, float* knn_dist_out) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(check_rows(ctx, X, x_dtype, x_location, "X"));
  if (!n_sim_neighbors_out) return fail(ctx, HMX_ERR_ARG, "null output");
  if (n_obs <= 0 || n_sim <= 0 || d <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (n_obs > 2000000000ll || n_sim > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  const int64_t N = n_obs + n_sim;
  CHK(score_limits(ctx, N, d));
  // knn_front's envelope with self excluded (check_neighbor_count's counts the cell itself: this is it shifted by one)
  if (k_adj < 1 || k_adj > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: 1 <= k_adj <= 128");
  if (k_adj >= N) return fail(ctx, HMX_ERR_LIMIT, "k_adj excludes the cell itself: at most n_obs + n_sim - 1");
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  KnnLists K;
  CHK(knn_front(ctx, B, t0, X, x_dtype, x_location, N, d, k_adj, knn_idx_out, knn_dist_out, K));
  int* dcnt;
  HIPCHK(B.get(&dcnt, (size_t)N));
  l_doublet_count(ctx->L, K.idx, N, k_adj, n_obs, dcnt, ctx->L.stream); KCHK();
  HIPCHK(download(n_sim_neighbors_out, dcnt, (size_t)N, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  ctx->timers["doublet_neighbors"] = now_ms() - K.t1;
  return 0;
}

}  // extern "C"
