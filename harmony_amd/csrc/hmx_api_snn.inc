// hmx_api_snn.inc -- part of hmx_api.cpp (included there, ONE translation unit, behind hmx_api_graph.inc, whose graph_outputs it shares, and
// hmx_api_metrics.inc, whose knn_device it runs): hmx_snn_from_knn and hmx_snn_graph (include/harmony_mi355x_snn.h; DESIGN "Seurat's SNN graph").
// Kernels: hmx_graph.hip.  The calls keep no state on the handle but the timers and the counters of the last call.

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
  const size_t cnt = (size_t)N * m;
  const int k = m + 1;
  const std::vector<float> jtab = snn_weights(k);
  ctx->snn_s_min = snn_s_min(k, prune);
  ctx->snn_long_rows = 0;
  GraphDev G{};                                          // the transposed lists, by the graph stage's own launchers
  G.idx = didx; G.N = N; G.m = m;
  SnnDev S{};
  S.idx = didx; S.N = N; S.m = m; S.s_min = (int)ctx->snn_s_min;
  long long* bsum; long long* dindptr; float* djtab;
  HIPCHK(B.get(&G.deg, (size_t)N)); HIPCHK(B.get(&G.toff, (size_t)N + 1));
  HIPCHK(B.get(&G.tkey, cnt)); HIPCHK(B.get(&G.tother, cnt));
  HIPCHK(B.get(&G.longrows, cnt / GR_WAVE_KEYS + 1)); HIPCHK(B.get(&G.nlong, 1));
  HIPCHK(B.get(&S.cand, (size_t)N)); HIPCHK(B.get(&S.longrows, (size_t)N)); HIPCHK(B.get(&S.nlong, 1));
  HIPCHK(B.get(&S.len, (size_t)N)); HIPCHK(B.get(&dindptr, (size_t)N + 1)); HIPCHK(B.get(&djtab, jtab.size()));
  HIPCHK(B.get(&bsum, (size_t)(N + GR_SCAN_CHUNK - 1) / GR_SCAN_CHUNK + 1));
  HIPCHK(hipMemsetAsync(G.deg, 0, (size_t)N * sizeof(unsigned), st));
  HIPCHK(hipMemsetAsync(G.nlong, 0, sizeof(unsigned), st));
  HIPCHK(hipMemsetAsync(S.nlong, 0, sizeof(unsigned), st));
  HIPCHK(hipMemsetAsync(S.len, 0, (size_t)N * sizeof(unsigned), st));
  HIPCHK(hipMemcpyAsync(djtab, jtab.data(), jtab.size() * sizeof(float), hipMemcpyHostToDevice, st));
  S.toff = G.toff; S.tkey = G.tkey; S.jtab = djtab;
  l_snn_indegree(ctx->L, G); KCHK();
  l_graph_scan(ctx->L, G.deg, N, G.toff, bsum); KCHK();
  l_graph_place(ctx->L, G); KCHK();
  l_graph_sort(ctx->L, G); KCHK();
  l_snn_rowweight(ctx->L, S); KCHK();
  l_snn_short(ctx->L, S, false); KCHK();
  l_snn_long(ctx->L, S, false); KCHK();
  l_graph_scan(ctx->L, S.len, N, dindptr, bsum); KCHK();
  unsigned nlong = 0;
  HIPCHK(hipMemcpyAsync(indptr, dindptr, ((size_t)N + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&nlong, S.nlong, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  ctx->snn_long_rows = (int64_t)nlong;
  const int64_t nnz = indptr[N];
  if (nnz < 0 || (double)nnz > (double)N * (double)N) return fail(ctx, HMX_ERR_DEVICE, "snn: the row lengths do not add up");
  if (capacity < nnz) return fail(ctx, HMX_ERR_LIMIT, "capacity " + std::to_string(capacity) + " is below the graph's " + std::to_string(nnz) + " entries (indptr is written)");
  if (!nnz) return 0;
  S.indptr = dindptr;
  HIPCHK(B.get(&S.indices, (size_t)nnz)); HIPCHK(B.get(&S.weights, (size_t)nnz));
  l_snn_short(ctx->L, S, true); KCHK();
  l_snn_long(ctx->L, S, true); KCHK();
  HIPCHK(hipMemcpyAsync(indices, S.indices, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(weights, S.weights, (size_t)nnz * sizeof(float), hipMemcpyDeviceToHost, st));
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
  if (N <= 0 || m <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (m > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: at most 128 neighbours");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  std::vector<int32_t> row((size_t)m);
  for (int64_t i = 0; i < N; i++) {
    for (int32_t j = 0; j < m; j++) {
      const int32_t v = idx[(size_t)i * m + j];
      if (v < -1 || v >= N) return fail(ctx, HMX_ERR_ARG, "neighbour index outside [-1, N) (row " + std::to_string(i) + ")");
      if (v == i) return fail(ctx, HMX_ERR_ARG, "row " + std::to_string(i) + " lists its own cell: the lists exclude self");
      row[(size_t)j] = v;
    }
    std::sort(row.begin(), row.end());
    for (int32_t j = 1; j < m; j++)
      if (row[(size_t)j] >= 0 && row[(size_t)j] == row[(size_t)j - 1]) return fail(ctx, HMX_ERR_ARG, "row " + std::to_string(i) + " lists a cell twice");
  }
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  int* didx;
  const size_t cnt = (size_t)N * m;
  HIPCHK(B.get(&didx, cnt));
  HIPCHK(hipMemcpyAsync(didx, idx, cnt * sizeof(int32_t), hipMemcpyHostToDevice, ctx->L.stream));
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
  if (k < 2 || k > SNN_MAX_K) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: 2 <= k <= 129");
  if (k > N) return fail(ctx, HMX_ERR_LIMIT, "k counts the cell itself: at most N");
  const int m = k - 1;
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  KnnDev P{};
  P.zs = (d + 3) / 4 * 4; P.k = m; P.excl = 1; P.N = P.Nq = N;
  float* xr; float* xn;
  CHK(score_rows(ctx, B, X, x_dtype, x_location, N, d, P.zs, &xr, &xn));
  P.X = P.Q = xr; P.xn = P.qn = xn;
  const size_t cnt = (size_t)N * m;
  HIPCHK(B.get(&P.idx, cnt)); HIPCHK(B.get(&P.dist, cnt));
  CHK(knn_device(ctx, B, P));
  if (knn_idx) HIPCHK(hipMemcpyAsync(knn_idx, P.idx, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->L.stream));
  if (knn_dist) HIPCHK(hipMemcpyAsync(knn_dist, P.dist, cnt * sizeof(float), hipMemcpyDeviceToHost, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  const double t1 = now_ms();
  ctx->timers["knn"] = t1 - t0;
  const int s = snn_device(ctx, B, P.idx, N, m, prune, indptr, indices, weights, capacity);
  ctx->timers["snn"] = now_ms() - t1;
  return s;
}

}  // extern "C"
