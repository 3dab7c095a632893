// hmx_api_metrics.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_knn, hmx_lisi and hmx_compute_lisi
// (include/harmony_mi355x_metrics.h; DESIGN "Scoring an integration").  Kernels: hmx_knn.hip.  The calls keep no state on the handle
// but the timers: every device buffer lives for one call.

namespace {

struct MetricBufs {        // device buffers of one call
  std::vector<void*> v;
  ~MetricBufs() { for (void* p : v) (void)hipFree(p); }
  template <class T> hipError_t get(T** p, size_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) v.push_back(q);
    *p = (T*)q;
    return e;
  }
};

int metrics_device(hmx_ctx* ctx) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ctx, HMX_ERR_DEVICE, "no HIP device available: libharmony_mi355x has no CPU fallback");
  if (ctx->device < 0) { int cur = 0; (void)hipGetDevice(&cur); ctx->device = cur; }
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->L.stream) { HIPCHK(hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking)); ctx->own_stream = true; }
  return 0;
}

// rows of either element type, host or HBM -> fp32 rows of stride zs and squared norms, both owned by `B`
int metrics_rows(hmx_ctx* ctx, MetricBufs& B, const void* X, int32_t dtype, int32_t location, int64_t N, int32_t d, int zs, float** rows, float** nrm) {
  const size_t bytes = (size_t)N * d * (dtype == HMX_F32 ? 4 : 8);
  const void* src = X;
  if (location == HMX_HOST) {
    char* raw = nullptr;
    HIPCHK(B.get(&raw, bytes));
    HIPCHK(hipMemcpyAsync(raw, X, bytes, hipMemcpyHostToDevice, ctx->L.stream));
    src = raw;
  }
  HIPCHK(B.get(rows, (size_t)N * zs));
  HIPCHK(B.get(nrm, (size_t)N));
  l_knn_ingest(ctx->L, src, dtype == HMX_F32, N, d, zs, *rows, *nrm); KCHK();
  return 0;
}

// how the data rows are split over grid.y: one chunk when the query tiles alone fill the device, else enough chunks for ~512 workgroups,
// each a multiple of the slab and at least 2 k rows long
void knn_plan(KnnDev& P) {
  const int64_t tiles = (P.Nq + KNN_QROWS - 1) / KNN_QROWS;
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(512 / tiles, 512));
  int64_t chunk = (P.N + want - 1) / want;
  chunk = std::max<int64_t>(chunk, 2 * P.k);
  chunk = (chunk + KNN_SLAB - 1) / KNN_SLAB * KNN_SLAB;
  P.chunk = chunk;
  P.nchunks = (int)((P.N + chunk - 1) / chunk);
}

// the search itself on device rows; idx / dist: device buffers [Nq][k]
int knn_device(hmx_ctx* ctx, MetricBufs& B, KnnDev P) {
  P.NG = (P.zs + 15) / 16;
  knn_plan(P);
  P.part = nullptr;
  if (P.nchunks > 1) HIPCHK(B.get(&P.part, (size_t)P.Nq * P.nchunks * P.k));
  l_knn(ctx->L, P); KCHK();
  return 0;
}

int check_rows(hmx_ctx* ctx, const void* X, int32_t dtype, int32_t location, const char* what) {
  if (!X) return fail(ctx, HMX_ERR_ARG, std::string("null ") + what);
  if ((dtype != HMX_F64 && dtype != HMX_F32) || (location != HMX_HOST && location != HMX_DEVICE))
    return fail(ctx, HMX_ERR_ARG, std::string("bad dtype / location of ") + what);
  return 0;
}

int check_labels(hmx_ctx* ctx, const int32_t* labels, int64_t N, int32_t n_cols, const int32_t* n_levels) {
  if (!labels || !n_levels) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (n_cols <= 0) return fail(ctx, HMX_ERR_ARG, "at least one label column");
  for (int c = 0; c < n_cols; c++) {
    if (n_levels[c] <= 0) return fail(ctx, HMX_ERR_ARG, "n_levels must be positive");
    for (int64_t i = 0; i < N; i++)
      if (labels[(size_t)c * N + i] < 0 || labels[(size_t)c * N + i] >= n_levels[c])
        return fail(ctx, HMX_ERR_ARG, "label code outside [0, n_levels) in column " + std::to_string(c));
  }
  return 0;
}

}  // namespace

extern "C" {

int hmx_knn(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N,
            const void* Q, int32_t q_dtype, int32_t q_location, int64_t Nq,
            int32_t d, int32_t k, int32_t* idx, float* dist, int32_t out_location) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(check_rows(ctx, X, x_dtype, x_location, "X"));
  if (Q) CHK(check_rows(ctx, Q, q_dtype, q_location, "Q"));
  if (!idx || !dist) return fail(ctx, HMX_ERR_ARG, "null output");
  if (out_location != HMX_HOST && out_location != HMX_DEVICE) return fail(ctx, HMX_ERR_ARG, "bad location of the output");
  const bool self = Q == nullptr;
  if (self) Nq = N;
  if (N <= 0 || Nq <= 0 || d <= 0 || k <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (d > 128 || k > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= 128, k <= 128");
  if (N > 2000000000ll || Nq > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  if (k > N - (self ? 1 : 0)) return fail(ctx, HMX_ERR_LIMIT, self ? "k must not exceed N - 1 when self is excluded" : "k must not exceed N");
  CHK(metrics_device(ctx));
  const double t0 = now_ms();
  MetricBufs B;
  KnnDev P{};
  P.zs = (d + 3) / 4 * 4; P.k = k; P.excl = self ? 1 : 0; P.N = N; P.Nq = Nq;
  float* xr; float* xn;
  CHK(metrics_rows(ctx, B, X, x_dtype, x_location, N, d, P.zs, &xr, &xn));
  P.X = xr; P.xn = xn; P.Q = xr; P.qn = xn;
  if (!self) {
    float* qr; float* qn;
    CHK(metrics_rows(ctx, B, Q, q_dtype, q_location, Nq, d, P.zs, &qr, &qn));
    P.Q = qr; P.qn = qn;
  }
  const size_t cnt = (size_t)Nq * k;
  P.idx = idx; P.dist = dist;
  if (out_location == HMX_HOST) { HIPCHK(B.get(&P.idx, cnt)); HIPCHK(B.get(&P.dist, cnt)); }
  CHK(knn_device(ctx, B, P));
  if (out_location == HMX_HOST) {
    HIPCHK(hipMemcpyAsync(idx, P.idx, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->L.stream));
    HIPCHK(hipMemcpyAsync(dist, P.dist, cnt * sizeof(float), hipMemcpyDeviceToHost, ctx->L.stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  ctx->timers["knn"] = now_ms() - t0;
  return 0;
}

int hmx_lisi(hmx_ctx* ctx, const int32_t* idx, const float* dist, int64_t Nq, int32_t m,
             const int32_t* labels, int64_t N, int32_t n_cols, const int32_t* n_levels, double perplexity, double* out) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!idx || !dist || !out) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (Nq <= 0 || N <= 0 || m <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (m > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: at most 128 neighbours");
  if (N > 2000000000ll || Nq > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  if (!(perplexity > 0) || !std::isfinite(perplexity)) return fail(ctx, HMX_ERR_ARG, "perplexity must be positive");
  CHK(check_labels(ctx, labels, N, n_cols, n_levels));
  for (size_t i = 0; i < (size_t)Nq * m; i++) if (idx[i] < 0 || idx[i] >= N) return fail(ctx, HMX_ERR_ARG, "neighbour index outside [0, N)");
  CHK(metrics_device(ctx));
  const double t0 = now_ms();
  MetricBufs B;
  int* didx; float* ddist; int* dlab; double* dout;
  const size_t cnt = (size_t)Nq * m;
  HIPCHK(B.get(&didx, cnt)); HIPCHK(B.get(&ddist, cnt)); HIPCHK(B.get(&dlab, (size_t)n_cols * N)); HIPCHK(B.get(&dout, (size_t)Nq * n_cols));
  HIPCHK(hipMemcpyAsync(didx, idx, cnt * sizeof(int32_t), hipMemcpyHostToDevice, ctx->L.stream));
  HIPCHK(hipMemcpyAsync(ddist, dist, cnt * sizeof(float), hipMemcpyHostToDevice, ctx->L.stream));
  HIPCHK(hipMemcpyAsync(dlab, labels, (size_t)n_cols * N * sizeof(int32_t), hipMemcpyHostToDevice, ctx->L.stream));
  l_lisi(ctx->L, didx, ddist, Nq, m, dlab, N, n_cols, perplexity, dout); KCHK();
  HIPCHK(hipMemcpyAsync(out, dout, (size_t)Nq * n_cols * sizeof(double), hipMemcpyDeviceToHost, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  ctx->timers["lisi"] = now_ms() - t0;
  return 0;
}

int hmx_compute_lisi(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d,
                     const int32_t* labels, int32_t n_cols, const int32_t* n_levels, double perplexity, double* out) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  const bool own = X == nullptr;            // the handle's current Z_corr
  if (own) {
    if (!(ctx->ran_setup || ctx->query_done)) return fail(ctx, HMX_ERR_STATE, "no embedding on this handle: setup or map_query first, or pass X");
    if (N != ctx->N) return fail(ctx, HMX_ERR_ARG, "N is not the handle's cell count");
    d = ctx->d;
  } else {
    CHK(check_rows(ctx, X, x_dtype, x_location, "X"));
  }
  if (!out) return fail(ctx, HMX_ERR_ARG, "null output");
  if (N <= 0 || d <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (!(perplexity > 0) || !std::isfinite(perplexity)) return fail(ctx, HMX_ERR_ARG, "perplexity must be positive");
  if (d > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= 128");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  const double m3 = std::floor(3.0 * perplexity) - 1.0;
  if (m3 < 1) return fail(ctx, HMX_ERR_ARG, "perplexity too small: 3 perplexity - 1 neighbours are needed");
  if (m3 > 128 || m3 > (double)(N - 1)) return fail(ctx, HMX_ERR_LIMIT, "3 perplexity - 1 neighbours: at most 128 and at most N - 1");
  const int m = (int)m3;
  CHK(check_labels(ctx, labels, N, n_cols, n_levels));
  CHK(metrics_device(ctx));
  const double t0 = now_ms();
  MetricBufs B;
  KnnDev P{};
  P.zs = (d + 3) / 4 * 4; P.k = m; P.excl = 1; P.N = P.Nq = N;
  float* xr; float* xn;
  if (own) {
    CHK(sync_solve_results(ctx));      // (a singular system of the last correction surfaces here, as in hmx_get_matrix)
    float* dense;                                           // Z_corr in the order the cells were given in
    HIPCHK(B.get(&dense, (size_t)N * d));
    l_convert_out(ctx->L, ctx->D.Zc, dense, 1, ctx->D.invperm, ctx->D.n, d, ctx->D.zs); KCHK();
    CHK(metrics_rows(ctx, B, dense, HMX_F32, HMX_DEVICE, N, d, P.zs, &xr, &xn));
  } else {
    CHK(metrics_rows(ctx, B, X, x_dtype, x_location, N, d, P.zs, &xr, &xn));
  }
  P.X = P.Q = xr; P.xn = P.qn = xn;
  int* dlab; double* dout;
  HIPCHK(B.get(&P.idx, (size_t)N * m)); HIPCHK(B.get(&P.dist, (size_t)N * m));
  HIPCHK(B.get(&dlab, (size_t)n_cols * N)); HIPCHK(B.get(&dout, (size_t)N * n_cols));
  HIPCHK(hipMemcpyAsync(dlab, labels, (size_t)n_cols * N * sizeof(int32_t), hipMemcpyHostToDevice, ctx->L.stream));
  CHK(knn_device(ctx, B, P));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  const double t1 = now_ms();
  l_lisi(ctx->L, P.idx, P.dist, N, m, dlab, N, n_cols, perplexity, dout); KCHK();
  HIPCHK(hipMemcpyAsync(out, dout, (size_t)N * n_cols * sizeof(double), hipMemcpyDeviceToHost, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  ctx->timers["knn"] = t1 - t0;
  ctx->timers["lisi"] = now_ms() - t1;
  return 0;
}

}  // extern "C"
