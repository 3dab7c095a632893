// hmx_api_snn.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_snn_from_knn and hmx_snn_graph
// (include/harmony_mi355x_snn.h; DESIGN "Seurat's SNN graph").  Kernels: hmx_graph.hip.  The search, the check of the lists, the transposed
// lists and the CSR emit are the call seam's (hmx_api_call.inc).  The calls keep no state on the handle but the timers and the counters of
// the last call.

namespace {

// the smallest s in 1 .. k + 1 whose weight s / (2k - s) is not below `prune` (k >= 2: every denominator is positive)
int snn_s_min(int k, double prune) {
  for (int s = 1; s <= k; s++)
    if ((double)s / (double)(2 * k - s) >= prune) return s;
  return k + 1;
}
// the weight of every shared count s = 0 .. k: formed in fp64, rounded once
std::vector<float> snn_weights(int k) {
  std::vector<float> t((size_t)k + 1);
  for (int s = 0; s <= k; s++) t[(size_t)s] = (float)((double)s / (double)(2 * k - s));
  return t;
}

// the SNN stage on device lists didx [N][m]: indptr always, indices / weights when they fit `capacity`
int snn_device(hmx_ctx* ctx, CallBufs& B, const int* didx, int64_t N, int32_t m, double prune,
               int64_t* indptr, int32_t* indices, float* weights, int64_t capacity) {
  hipStream_t st = ctx->L.stream;
  const int k = m + 1;
  const std::vector<float> jtab = snn_weights(k);
  ctx->snn_s_min = snn_s_min(k, prune);
  ctx->snn_long_rows = 0;
  GraphDev G{};                                          // the transposed lists, by the graph stage's own launchers
  G.idx = didx; G.N = N; G.m = m;
  SnnDev S{};
  S.idx = didx; S.N = N; S.m = m; S.s_min = (int)ctx->snn_s_min;
  long long* bsum; long long* dindptr; float* djtab;
  HIPCHK(B.get(&S.cand, (size_t)N)); HIPCHK(B.get(&S.longrows, (size_t)N)); HIPCHK(B.get(&S.nlong, 1));
  HIPCHK(B.get(&S.len, (size_t)N));
  HIPCHK(zero_fill(S.nlong, 1, st));
  HIPCHK(zero_fill(S.len, (size_t)N, st));
  HIPCHK(B.put(&djtab, jtab.data(), jtab.size(), st));
  CHK(transposed_lists(ctx, B, G, &bsum, [&]() -> int { l_snn_indegree(ctx->L, G); KCHK(); return 0; }));
  S.toff = G.toff; S.tkey = G.tkey; S.jtab = djtab;
  l_snn_rowweight(ctx->L, S); KCHK();
  l_snn_short(ctx->L, S, false); KCHK();
  l_snn_long(ctx->L, S, false); KCHK();
  CHK(csr_offsets(ctx, B, S.len, N, bsum, indptr, &dindptr));
  unsigned nlong = 0;
  HIPCHK(download(&nlong, S.nlong, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  ctx->snn_long_rows = (int64_t)nlong;
  const int64_t nnz = indptr[N];
  CHK(csr_entries(ctx, B, "snn", nnz, (double)N * (double)N, capacity, &S.indices, &S.weights));
  if (!nnz) return 0;
  S.indptr = dindptr;
  l_snn_short(ctx->L, S, true); KCHK();
  l_snn_long(ctx->L, S, true); KCHK();
  HIPCHK(download(indices, S.indices, (size_t)nnz, st));
  HIPCHK(download(weights, S.weights, (size_t)nnz, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

int snn_prune(hmx_ctx* ctx, double prune) {
  if (!(prune >= 0.0 && prune <= 1.0)) return fail(ctx, HMX_ERR_ARG, "prune must lie in [0, 1]");
  return 0;
}

}  // namespace

extern "C" {

int hmx_snn_from_knn(hmx_ctx* ctx, const int32_t* idx, int64_t N, int32_t m, double prune,
                     int64_t* indptr, int32_t* indices, float* weights, int64_t capacity) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!idx) return fail(ctx, HMX_ERR_ARG, "null neighbour lists");
  CHK(graph_outputs(ctx, indptr, indices, weights, capacity));
  CHK(snn_prune(ctx, prune));
  CHK(check_lists(ctx, idx, nullptr, true, N, m));
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  int* didx;
  HIPCHK(B.put(&didx, idx, (size_t)N * m, ctx->L.stream));
  const int s = snn_device(ctx, B, didx, N, m, prune, indptr, indices, weights, capacity);
  ctx->timers["snn"] = now_ms() - t0;
  return s;
}

int hmx_snn_graph(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d, int32_t k, double prune,
                  int32_t* knn_idx, float* knn_dist, int64_t* indptr, int32_t* indices, float* weights, int64_t capacity) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(score_args(ctx, X, x_dtype, x_location, N, d, indptr));      // (X == nullptr: the handle's current Z_corr)
  CHK(graph_outputs(ctx, indptr, indices, weights, capacity));
  CHK(snn_prune(ctx, prune));
  CHK(score_limits(ctx, N, d));
  CHK(check_neighbor_count(ctx, "k", k, N));
  const int m = k - 1;
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  KnnLists K;
  CHK(knn_front(ctx, B, t0, X, x_dtype, x_location, N, d, m, knn_idx, knn_dist, K));
  const int s = snn_device(ctx, B, K.idx, N, m, prune, indptr, indices, weights, capacity);
  ctx->timers["snn"] = now_ms() - K.t1;
  return s;
}

}  // extern "C"
