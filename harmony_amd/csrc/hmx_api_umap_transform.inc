// hmx_api_umap_transform.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_umap_query_weights and hmx_umap_transform
// (include/harmony_mi355x_umap_transform.h; DESIGN "Query cells in a fitted layout").  Kernels: hmx_umap_transform.hip; the distance sum:
// hmx_graph.hip; the sum of the firing counters: hmx_umap.hip.  Device, stream and buffers are the call seam's (hmx_api_call.inc, CallBufs).
// Every argument is checked on the host, where the lists live, before a device is touched.  The calls keep no state on the handle but the
// timers and the counters of the last transform.

namespace {

// what the two calls check alike: the shape of the lists and the range of their indices
int ut_check_lists(hmx_ctx* ctx, const int32_t* idx, int64_t Nq, int32_t k, int64_t Nr) {
  if (Nq < 1) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (k < 1 || k > UT_MAX_K) return fail(ctx, HMX_ERR_ARG, "k must lie in 1 .. 128");
  if (k > Nr) return fail(ctx, HMX_ERR_ARG, "k exceeds the Nr reference cells");
  if (Nr > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 reference cells");
  if (Nq > ((1ll << 31) - 1) / k) return fail(ctx, HMX_ERR_LIMIT, "at most 2^31 - 1 list entries");
  for (int64_t t = 0; t < Nq * k; t++)
    if (idx[t] < 0 || idx[t] >= Nr) return fail(ctx, HMX_ERR_ARG, "an index of the lists is outside [0, Nr) (row " + std::to_string(t / k) + ")");
  return 0;
}

struct UtEvent {                                          // an event that lives for one call
  hipEvent_t e = nullptr;
  ~UtEvent() { if (e) (void)hipEventDestroy(e); }
};

struct UtArgs {
  int32_t dim, n_epochs, epoch_begin, epoch_end, negative_sample_rate;
  double a, b, gamma, alpha0;
  uint32_t seed;
};

int ut_device(hmx_ctx* ctx, const int32_t* idx, const float* weights, int64_t Nq, int32_t k, const float* Yref, int64_t Nr, const float* Yq0,
              float wmax, const UtArgs& A, float* Yinit, float* Y) {
  hipStream_t st = ctx->L.stream;
  CallBufs B;
  const size_t cnt = (size_t)Nq * k, pos = (size_t)Nq * A.dim;
  const int epochs = wmax > 0.0f ? A.epoch_end - A.epoch_begin : 0;      // (no weight above 0: the start is the result)
  int* didx; float* dw; float* dref;
  UtDev D{};
  HIPCHK(B.put(&didx, idx, cnt, st)); HIPCHK(B.put(&dw, weights, cnt, st)); HIPCHK(B.put(&dref, Yref, (size_t)Nr * A.dim, st));
  D.Nq = Nq; D.k = k; D.Nr = Nr; D.idx = didx; D.w = dw; D.yref = dref;
  if (Yq0) HIPCHK(B.put(&D.y0, Yq0, pos, st));
  else {
    HIPCHK(B.get(&D.y0, pos));
    l_ut_init(ctx->L, D, A.dim); KCHK();
  }
  if (epochs == 0) {
    HIPCHK(download(Y, D.y0, pos, st));
    if (Yinit) HIPCHK(download(Yinit, D.y0, pos, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  // alpha_n = (float)(alpha0 (1 - n / n_epochs)), the layout's host expression, as a table of the epochs run
  std::vector<float> alpha((size_t)epochs);
  for (int n = A.epoch_begin; n < A.epoch_end; n++) alpha[(size_t)(n - A.epoch_begin)] = (float)(A.alpha0 * (1.0 - (double)n / (double)A.n_epochs));
  float* dalpha;
  HIPCHK(B.put(&dalpha, alpha.data(), alpha.size(), st));
  UmDev F{};                                             // (the layout's sum of the firing counters reads N, fired and total)
  F.N = Nq;
  HIPCHK(B.get(&D.y, pos)); HIPCHK(B.get(&D.fired, (size_t)Nq)); HIPCHK(B.get(&F.total, 1));
  HIPCHK(zero_fill(F.total, 1, st));
  F.fired = D.fired;
  D.alpha = dalpha; D.wmax = (double)wmax; D.n0 = A.epoch_begin; D.n1 = A.epoch_end;
  D.a = (float)A.a; D.b = (float)A.b; D.m2ab = (float)(-2.0 * A.a * A.b); D.g2b = (float)(2.0 * A.gamma * A.b);
  D.kbase0 = um_h_fmix32(A.seed) + 1u; D.nneg = A.negative_sample_rate;
  UtEvent e0, e1;                                        // the epochs' kernel alone, in GPU time: "timer:umap_transform_epochs"
  HIPCHK(hipEventCreate(&e0.e)); HIPCHK(hipEventCreate(&e1.e));
  HIPCHK(hipEventRecord(e0.e, st));
  l_ut_transform(ctx->L, D, A.dim); KCHK();
  HIPCHK(hipEventRecord(e1.e, st));
  l_um_fired(ctx->L, F); KCHK();
  unsigned long long fired = 0;
  HIPCHK(download(&fired, F.total, 1, st));
  HIPCHK(download(Y, D.y, pos, st));
  if (Yinit) HIPCHK(download(Yinit, D.y0, pos, st));
  HIPCHK(hipStreamSynchronize(st));
  float kernel_ms = 0.0f;
  HIPCHK(hipEventElapsedTime(&kernel_ms, e0.e, e1.e));
  ctx->timers["umap_transform_epochs"] = (double)kernel_ms;
  ctx->umap_transform_fired = (int64_t)fired;
  ctx->umap_transform_epochs = epochs;
  return 0;
}

}  // namespace

extern "C" {

int hmx_umap_query_weights(hmx_ctx* ctx, const int32_t* idx, const float* dist, int64_t Nq, int32_t k, int64_t Nr, float* weights, double* sigma) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!idx || !dist || !weights) return fail(ctx, HMX_ERR_ARG, "null argument");
  CHK(ut_check_lists(ctx, idx, Nq, k, Nr));
  for (int64_t t = 0; t < Nq * k; t++)
    if (!(dist[t] >= 0.0f) || std::isinf(dist[t])) return fail(ctx, HMX_ERR_ARG, "a distance is NaN, negative or infinite (row " + std::to_string(t / k) + ")");
  CHK(call_device(ctx));
  const double t0 = now_ms();
  hipStream_t st = ctx->L.stream;
  CallBufs B;
  const size_t cnt = (size_t)Nq * k;
  int* didx; float* ddist;
  HIPCHK(B.put(&didx, idx, cnt, st)); HIPCHK(B.put(&ddist, dist, cnt, st));
  GraphDev G{};                                          // (the graph stage's distance sum: every slot of these lists is filled)
  G.idx = didx; G.dist = ddist; G.N = Nq; G.m = k;
  G.nparts = (int)graph_sum_parts((long long)cnt);
  HIPCHK(B.get(&G.part, (size_t)G.nparts)); HIPCHK(B.get(&G.total, 1));
  UqDev Q{};
  Q.idx = didx; Q.dist = ddist; Q.Nq = Nq; Q.k = k; Q.total = G.total;
  HIPCHK(B.get(&Q.w, cnt)); HIPCHK(B.get(&Q.sigma, (size_t)Nq));
  l_graph_distsum(ctx->L, G); KCHK();
  l_ut_weights(ctx->L, Q); KCHK();
  HIPCHK(download(weights, Q.w, cnt, st));
  if (sigma) HIPCHK(download(sigma, Q.sigma, (size_t)Nq, st));
  HIPCHK(hipStreamSynchronize(st));
  ctx->timers["umap_query_weights"] = now_ms() - t0;
  return 0;
}

int hmx_umap_transform(hmx_ctx* ctx, const int32_t* idx, const float* weights, int64_t Nq, int32_t k, const float* Yref, int64_t Nr, int32_t dim,
                       const float* Yq0, int32_t n_epochs, int32_t epoch_begin, int32_t epoch_end, double a, double b, double gamma, double alpha0,
                       int32_t negative_sample_rate, uint32_t seed, float* Yinit, float* Y) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  ctx->umap_transform_fired = ctx->umap_transform_epochs = 0;
  ctx->timers["umap_transform_epochs"] = 0.0;
  if (!idx || !weights || !Yref || !Y) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (dim != 2 && dim != 3) return fail(ctx, HMX_ERR_ARG, "dim must be 2 or 3");
  if (n_epochs < 1 || n_epochs > UM_MAX_EPOCHS) return fail(ctx, HMX_ERR_ARG, "n_epochs must lie in 1 .. 1048576");
  if (epoch_begin < 0 || epoch_end < epoch_begin || epoch_end > n_epochs) return fail(ctx, HMX_ERR_ARG, "the epochs [epoch_begin, epoch_end) must lie in [0, n_epochs)");
  if (!(a > 0.0 && std::isfinite(a)) || !(b > 0.0 && std::isfinite(b))) return fail(ctx, HMX_ERR_ARG, "a and b must be positive and finite");
  if (!(gamma >= 0.0 && std::isfinite(gamma))) return fail(ctx, HMX_ERR_ARG, "gamma must be non-negative and finite");
  if (!(alpha0 > 0.0 && std::isfinite(alpha0))) return fail(ctx, HMX_ERR_ARG, "alpha0 must be positive and finite");
  if (negative_sample_rate < 0 || negative_sample_rate > UM_MAX_NEG) return fail(ctx, HMX_ERR_ARG, "negative_sample_rate must lie in 0 .. 31");
  CHK(ut_check_lists(ctx, idx, Nq, k, Nr));
  float wmax = 0.0f;
  for (int64_t t = 0; t < Nq * k; t++) {
    if (!(weights[t] >= 0.0f && weights[t] <= 1.0f)) return fail(ctx, HMX_ERR_ARG, "a weight is outside [0, 1] or not finite (row " + std::to_string(t / k) + ")");
    wmax = std::max(wmax, weights[t]);
  }
  for (int64_t t = 0; t < Nr * dim; t++)
    if (!std::isfinite(Yref[t])) return fail(ctx, HMX_ERR_ARG, "Yref holds a value that is not finite (cell " + std::to_string(t / dim) + ")");
  if (Yq0)
    for (int64_t t = 0; t < Nq * dim; t++)
      if (!std::isfinite(Yq0[t])) return fail(ctx, HMX_ERR_ARG, "Yq0 holds a value that is not finite (cell " + std::to_string(t / dim) + ")");
  CHK(call_device(ctx));
  const double t0 = now_ms();
  const UtArgs A{dim, n_epochs, epoch_begin, epoch_end, negative_sample_rate, a, b, gamma, alpha0, seed};
  const int s = ut_device(ctx, idx, weights, Nq, k, Yref, Nr, Yq0, wmax, A, Yinit, Y);
  ctx->timers["umap_transform"] = now_ms() - t0;
  return s;
}

}  // extern "C"
