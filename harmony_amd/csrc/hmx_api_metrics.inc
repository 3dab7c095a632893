// hmx_api_metrics.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_knn, hmx_lisi and hmx_compute_lisi
// (include/harmony_mi355x_metrics.h; DESIGN "Scoring an integration").  Kernels: hmx_knn.hip.  The calls keep no state on the handle
// but the timers: every device buffer lives for one call, and the search is the call seam's (hmx_api_call.inc).

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
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  KnnDev P{};
  P.zs = (d + 3) / 4 * 4; P.k = k; P.excl = self ? 1 : 0; P.N = N; P.Nq = Nq;
  float* xr; float* xn;
  CHK(call_rows(ctx, B, X, x_dtype, x_location, N, d, P.zs, &xr, &xn));
  P.X = xr; P.xn = xn; P.Q = xr; P.qn = xn;
  if (!self) {
    float* qr; float* qn;
    CHK(call_rows(ctx, B, Q, q_dtype, q_location, Nq, d, P.zs, &qr, &qn));
    P.Q = qr; P.qn = qn;
  }
  const size_t cnt = (size_t)Nq * k;
  P.idx = idx; P.dist = dist;
  if (out_location == HMX_HOST) { HIPCHK(B.get(&P.idx, cnt)); HIPCHK(B.get(&P.dist, cnt)); }
  CHK(knn_device(ctx, B, P));
  if (out_location == HMX_HOST) {
    HIPCHK(download(idx, P.idx, cnt, ctx->L.stream));
    HIPCHK(download(dist, P.dist, cnt, ctx->L.stream));
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
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  int* didx; float* ddist; int* dlab; double* dout;
  const size_t cnt = (size_t)Nq * m;
  HIPCHK(B.put(&didx, idx, cnt, ctx->L.stream)); HIPCHK(B.put(&ddist, dist, cnt, ctx->L.stream));
  HIPCHK(B.put(&dlab, labels, (size_t)n_cols * N, ctx->L.stream)); HIPCHK(B.get(&dout, (size_t)Nq * n_cols));
  l_lisi(ctx->L, didx, ddist, Nq, m, dlab, N, n_cols, perplexity, dout); KCHK();
  HIPCHK(download(out, dout, (size_t)Nq * n_cols, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  ctx->timers["lisi"] = now_ms() - t0;
  return 0;
}

int hmx_compute_lisi(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d,
                     const int32_t* labels, int32_t n_cols, const int32_t* n_levels, double perplexity, double* out) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(score_args(ctx, X, x_dtype, x_location, N, d, out));      // (X == nullptr: the handle's current Z_corr)
  if (!(perplexity > 0) || !std::isfinite(perplexity)) return fail(ctx, HMX_ERR_ARG, "perplexity must be positive");
  CHK(score_limits(ctx, N, d));
  const double m3 = std::floor(3.0 * perplexity) - 1.0;
  if (m3 < 1) return fail(ctx, HMX_ERR_ARG, "perplexity too small: 3 perplexity - 1 neighbours are needed");
  if (m3 > 128 || m3 > (double)(N - 1)) return fail(ctx, HMX_ERR_LIMIT, "3 perplexity - 1 neighbours: at most 128 and at most N - 1");
  const int m = (int)m3;
  CHK(check_labels(ctx, labels, N, n_cols, n_levels));
  CHK(call_device(ctx));
  const double t0 = now_ms();
  CallBufs B;
  int* dlab; double* dout;
  HIPCHK(B.put(&dlab, labels, (size_t)n_cols * N, ctx->L.stream)); HIPCHK(B.get(&dout, (size_t)N * n_cols));
  KnnLists K;
  CHK(knn_front(ctx, B, t0, X, x_dtype, x_location, N, d, m, nullptr, nullptr, K));
  l_lisi(ctx->L, K.idx, K.dist, N, m, dlab, N, n_cols, perplexity, dout); KCHK();
  HIPCHK(download(out, dout, (size_t)N * n_cols, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  ctx->timers["lisi"] = now_ms() - K.t1;
  return 0;
}

}  // extern "C"
