// hmx_api_graph.inc -- part of hmx_api.cpp (included there, ONE translation unit, behind hmx_api_metrics.inc, whose knn_device it runs):
// hmx_graph_from_knn, hmx_neighbor_graph and hmx_graph_components (include/harmony_mi355x_graph.h; DESIGN "The neighbour graph").
// Kernels: hmx_graph.hip.  The calls keep no state on the handle but the timers and the rounds of the last components call.

namespace {

static_assert(sizeof(long long) == sizeof(int64_t), "offsets are copied as they are");

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
  HIPCHK(B.get(&G.deg, (size_t)N)); HIPCHK(B.get(&G.toff, (size_t)N + 1));
  HIPCHK(B.get(&G.tkey, cnt)); HIPCHK(B.get(&G.tother, cnt));
  HIPCHK(B.get(&G.longrows, cnt / GR_WAVE_KEYS + 1)); HIPCHK(B.get(&G.nlong, 1));
  HIPCHK(B.get(&G.len, (size_t)N)); HIPCHK(B.get(&dindptr, (size_t)N + 1)); HIPCHK(B.get(&G.flag, 1));
  HIPCHK(B.get(&bsum, (size_t)(N + GR_SCAN_CHUNK - 1) / GR_SCAN_CHUNK + 1));
  HIPCHK(hipMemsetAsync(G.deg, 0, (size_t)N * sizeof(unsigned), st));
  HIPCHK(hipMemsetAsync(G.nlong, 0, sizeof(unsigned), st));
  HIPCHK(hipMemsetAsync(G.flag, 0, sizeof(int), st));
  l_graph_distsum(ctx->L, G); KCHK();
  l_graph_smooth(ctx->L, G); KCHK();
  l_graph_scan(ctx->L, G.deg, N, G.toff, bsum); KCHK();
  l_graph_place(ctx->L, G); KCHK();
  l_graph_sort(ctx->L, G); KCHK();
  l_graph_union(ctx->L, G, false); KCHK();
  l_graph_scan(ctx->L, G.len, N, dindptr, bsum); KCHK();
  int flag = 0;
  HIPCHK(hipMemcpyAsync(indptr, dindptr, ((size_t)N + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&flag, G.flag, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (flag & GR_FLAG_DUP) return fail(ctx, HMX_ERR_ARG, "a row of the neighbour lists holds a cell twice");
  const int64_t nnz = indptr[N];
  if (nnz < 0 || nnz > 2 * (int64_t)cnt) return fail(ctx, HMX_ERR_DEVICE, "graph: the row lengths do not add up");
  if (capacity < nnz) return fail(ctx, HMX_ERR_LIMIT, "capacity " + std::to_string(capacity) + " is below the graph's " + std::to_string(nnz) + " entries (indptr is written)");
  G.indptr = dindptr;
  HIPCHK(B.get(&G.indices, (size_t)nnz)); HIPCHK(B.get(&G.weights, (size_t)nnz));
  l_graph_union(ctx->L, G, true); KCHK();
  if (nnz) {
    HIPCHK(hipMemcpyAsync(indices, G.indices, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(weights, G.weights, (size_t)nnz * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  if (rho) HIPCHK(hipMemcpyAsync(rho, G.rho, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (sigma) HIPCHK(hipMemcpyAsync(sigma, G.sigma, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

int graph_outputs(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t capacity) {
  if (!indptr) return fail(ctx, HMX_ERR_ARG, "null indptr");
  if (capacity < 0) return fail(ctx, HMX_ERR_ARG, "negative capacity");
  if (capacity > 0 && (!indices || !weights)) return fail(ctx, HMX_ERR_ARG, "null indices / weights with a positive capacity");
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
  if (N <= 0 || m <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (m > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: at most 128 neighbours");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  for (int64_t i = 0; i < N; i++)
    for (int32_t j = 0; j < m; j++) {
      const int32_t v = idx[(size_t)i * m + j];
      if (v < -1 || v >= N) return fail(ctx, HMX_ERR_ARG, "neighbour index outside [-1, N) (row " + std::to_string(i) + ")");
      if (v == i) return fail(ctx, HMX_ERR_ARG, "row " + std::to_string(i) + " lists its own cell: the lists exclude self");
      if (v >= 0 && std::isnan(dist[(size_t)i * m + j])) return fail(ctx, HMX_ERR_ARG, "NaN distance (row " + std::to_string(i) + ")");
    }
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  int* didx; float* ddist;
  const size_t cnt = (size_t)N * m;
  HIPCHK(B.get(&didx, cnt)); HIPCHK(B.get(&ddist, cnt));
  HIPCHK(hipMemcpyAsync(didx, idx, cnt * sizeof(int32_t), hipMemcpyHostToDevice, ctx->L.stream));
  HIPCHK(hipMemcpyAsync(ddist, dist, cnt * sizeof(float), hipMemcpyHostToDevice, ctx->L.stream));
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
  if (n_neighbors < 2 || n_neighbors > 129) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: 2 <= n_neighbors <= 129");
  if (n_neighbors > N) return fail(ctx, HMX_ERR_LIMIT, "n_neighbors counts the cell itself: at most N");
  const int m = n_neighbors - 1;
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
  const int s = graph_device(ctx, B, P.idx, P.dist, N, m, indptr, indices, weights, capacity, rho, sigma);
  ctx->timers["graph"] = now_ms() - t1;
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
  HIPCHK(B.get(&dptr, (size_t)N + 1)); HIPCHK(B.get(&dind, (size_t)nnz)); HIPCHK(B.get(&C.comp, (size_t)N)); HIPCHK(B.get(&C.flag, 1));
  HIPCHK(hipMemcpyAsync(dptr, indptr, ((size_t)N + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  if (nnz) HIPCHK(hipMemcpyAsync(dind, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (labels) {
    HIPCHK(B.get(&dlab, (size_t)N));
    HIPCHK(hipMemcpyAsync(dlab, labels, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  C.N = N; C.indptr = dptr; C.indices = dind; C.labels = dlab;
  int flag = 0;
  auto read_flag = [&]() -> int {
    HIPCHK(hipMemcpyAsync(&flag, C.flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  };
  HIPCHK(hipMemsetAsync(C.flag, 0, sizeof(int), st));
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
    HIPCHK(hipMemsetAsync(C.flag, 0, sizeof(int), st));
    l_cc_hook(ctx->L, C); KCHK();
    for (int j = 0; j < jumps; j++) { l_cc_jump(ctx->L, C, false); KCHK(); }
    l_cc_jump(ctx->L, C, true); KCHK();
    CHK(read_flag());
    ctx->graph_cc_rounds = round + 1;
    if (flag & GR_FLAG_DEEP) return fail(ctx, HMX_ERR_INTERNAL, "components: a tree was not flat after the round's pointer jumps");
    settled = !(flag & GR_FLAG_CHANGED);
  }
  if (!settled) return fail(ctx, HMX_ERR_INTERNAL, "components: no fixed point within " + std::to_string(GR_CC_ROUNDS) + " rounds");
  HIPCHK(hipMemcpyAsync(comp, C.comp, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
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
