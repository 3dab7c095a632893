// hmx_api_graph.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_graph_from_knn, hmx_neighbor_graph and
// hmx_graph_components (include/harmony_mi355x_graph.h; DESIGN "The neighbour graph").  Kernels: hmx_graph.hip.  The search, the check of the
// lists, the transposed lists and the CSR emit are the call seam's (hmx_api_call.inc).  The calls keep no state on the handle but the timers
// and the rounds of the last components call.

namespace {

// the graph stage on device lists didx / ddist [N][m]: indptr always, indices / weights when they fit `capacity`, rho / sigma when asked for
int graph_device(hmx_ctx* ctx, CallBufs& B, const int* didx, const float* ddist, int64_t N, int32_t m,
                 int64_t* indptr, int32_t* indices, float* weights, int64_t capacity, double* rho, double* sigma) {
  hipStream_t st = ctx->L.stream;
  const size_t cnt = (size_t)N * m;
  GraphDev G{};
  G.idx = didx; G.dist = ddist; G.N = N; G.m = m;
  G.nparts = (int)graph_sum_parts((long long)cnt);
  long long* bsum; long long* dindptr;
  HIPCHK(B.get(&G.part, (size_t)G.nparts)); HIPCHK(B.get(&G.total, 1));
  HIPCHK(B.get(&G.rho, (size_t)N)); HIPCHK(B.get(&G.sigma, (size_t)N)); HIPCHK(B.get(&G.w, cnt));
  HIPCHK(B.get(&G.len, (size_t)N)); HIPCHK(B.get(&G.flag, 1));
  HIPCHK(zero_fill(G.flag, 1, st));
  CHK(transposed_lists(ctx, B, G, &bsum, [&]() -> int {      // (the smoothing counts the in-degrees beside its search)
    l_graph_distsum(ctx->L, G); KCHK();
    l_graph_smooth(ctx->L, G); KCHK();
    return 0;
  }));
  l_graph_union(ctx->L, G, false); KCHK();
  CHK(csr_offsets(ctx, B, G.len, N, bsum, indptr, &dindptr));
  int flag = 0;
  HIPCHK(download(&flag, G.flag, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  if (flag & GR_FLAG_DUP) return fail(ctx, HMX_ERR_ARG, "a row of the neighbour lists holds a cell twice");
  const int64_t nnz = indptr[N];
  CHK(csr_entries(ctx, B, "graph", nnz, 2.0 * (double)cnt, capacity, &G.indices, &G.weights));
  G.indptr = dindptr;
  l_graph_union(ctx->L, G, true); KCHK();
  HIPCHK(download(indices, G.indices, (size_t)nnz, st));
  HIPCHK(download(weights, G.weights, (size_t)nnz, st));
  if (rho) HIPCHK(download(rho, G.rho, (size_t)N, st));
  if (sigma) HIPCHK(download(sigma, G.sigma, (size_t)N, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

}  // namespace

extern "C" {

int hmx_graph_from_knn(hmx_ctx* ctx, const int32_t* idx, const float* dist, int64_t N, int32_t m,
                       int64_t* indptr, int32_t* indices, float* weights, int64_t capacity, double* rho, double* sigma) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!idx || !dist) return fail(ctx, HMX_ERR_ARG, "null neighbour lists");
  CHK(graph_outputs(ctx, indptr, indices, weights, capacity));
  CHK(check_lists(ctx, idx, dist, false, N, m));
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  int* didx; float* ddist;
  HIPCHK(B.put(&didx, idx, (size_t)N * m, ctx->L.stream)); HIPCHK(B.put(&ddist, dist, (size_t)N * m, ctx->L.stream));
  const int s = graph_device(ctx, B, didx, ddist, N, m, indptr, indices, weights, capacity, rho, sigma);
  ctx->timers["graph"] = now_ms() - t0;
  return s;
}

int hmx_neighbor_graph(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d, int32_t n_neighbors,
                       int32_t* knn_idx, float* knn_dist, int64_t* indptr, int32_t* indices, float* weights, int64_t capacity,
                       double* rho, double* sigma) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(score_args(ctx, X, x_dtype, x_location, N, d, indptr));      // (X == nullptr: the handle's current Z_corr)
  CHK(graph_outputs(ctx, indptr, indices, weights, capacity));
  CHK(score_limits(ctx, N, d));
  CHK(check_neighbor_count(ctx, "n_neighbors", n_neighbors, N));
  const int m = n_neighbors - 1;
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  KnnLists K;
  CHK(knn_front(ctx, B, t0, X, x_dtype, x_location, N, d, m, knn_idx, knn_dist, K));
  const int s = graph_device(ctx, B, K.idx, K.dist, N, m, indptr, indices, weights, capacity, rho, sigma);
  ctx->timers["graph"] = now_ms() - K.t1;
  return s;
}

int hmx_graph_components(hmx_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const int32_t* labels,
                         int32_t* comp, int64_t* n_components) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!indptr || !comp) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (N <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  if (indptr[0] != 0) return fail(ctx, HMX_ERR_ARG, "indptr must start at 0");
  for (int64_t i = 0; i < N; i++)
    if (indptr[i + 1] < indptr[i] || indptr[i + 1] - indptr[i] > N) return fail(ctx, HMX_ERR_ARG, "indptr must ascend by at most N per row (row " + std::to_string(i) + ")");
  const int64_t nnz = indptr[N];
  if (nnz > 0 && !indices) return fail(ctx, HMX_ERR_ARG, "null indices");
  if (labels)
    for (int64_t i = 0; i < N; i++) if (labels[i] < -1) return fail(ctx, HMX_ERR_ARG, "a label is below -1 (cell " + std::to_string(i) + ")");
  CHK(call_device(ctx));
  const double t0 = now_ms();
  hipStream_t st = ctx->L.stream;
  CallBufs B;
  long long* dptr; int* dind; int* dlab = nullptr;
  CcDev C{};
  HIPCHK(B.put(&dptr, indptr, (size_t)N + 1, st)); HIPCHK(B.get(&dind, (size_t)nnz)); HIPCHK(B.get(&C.comp, (size_t)N)); HIPCHK(B.get(&C.flag, 1));
  if (nnz) HIPCHK(upload(dind, indices, (size_t)nnz, st));
  if (labels) HIPCHK(B.put(&dlab, labels, (size_t)N, st));
  C.N = N; C.indptr = dptr; C.indices = dind; C.labels = dlab;
  int flag = 0;
  auto read_flag = [&]() -> int {
    HIPCHK(download(&flag, C.flag, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  };
  HIPCHK(zero_fill(C.flag, 1, st));
  l_cc_check(ctx->L, C); KCHK();
  CHK(read_flag());
  if (flag & GR_FLAG_RANGE) return fail(ctx, HMX_ERR_ARG, "an index of the pattern is outside [0, N)");
  if (flag & GR_FLAG_ORDER) return fail(ctx, HMX_ERR_ARG, "a row of the pattern is not strictly ascending");
  if (flag & GR_FLAG_ASYM) return fail(ctx, HMX_ERR_ARG, "the pattern is not symmetric: an edge has no mirror");
  int jumps = 1;                                         // GR_CC_HOPS^jumps >= N: a tree as deep as N is flat after that many launches
  for (int64_t reach = GR_CC_HOPS; reach < N; reach *= GR_CC_HOPS) jumps++;
  l_cc_init(ctx->L, C); KCHK();
  ctx->graph_cc_rounds = 0;
  bool settled = false;
  for (int round = 0; round < GR_CC_ROUNDS && !settled; round++) {
    HIPCHK(zero_fill(C.flag, 1, st));
    l_cc_hook(ctx->L, C); KCHK();
    for (int j = 0; j < jumps; j++) { l_cc_jump(ctx->L, C, false); KCHK(); }
    l_cc_jump(ctx->L, C, true); KCHK();
    CHK(read_flag());
    ctx->graph_cc_rounds = round + 1;
    if (flag & GR_FLAG_DEEP) return fail(ctx, HMX_ERR_INTERNAL, "components: a tree was not flat after the round's pointer jumps");
    settled = !(flag & GR_FLAG_CHANGED);
  }
  if (!settled) return fail(ctx, HMX_ERR_INTERNAL, "components: no fixed point within " + std::to_string(GR_CC_ROUNDS) + " rounds");
  HIPCHK(download(comp, C.comp, (size_t)N, st));
  HIPCHK(hipStreamSynchronize(st));
  if (n_components) {
    int64_t n = 0;
    for (int64_t i = 0; i < N; i++) n += comp[i] == i ? 1 : 0;
    *n_components = n;
  }
  ctx->timers["components"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
