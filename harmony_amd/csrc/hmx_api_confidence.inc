// hmx_api_confidence.inc -- part of hmx_api.cpp (included there, ONE translation unit, behind hmx_api_query.inc whose query_chunks /
// query_sums run pass A): hmx_reference_moments and hmx_mapping_confidence
// (include/harmony_mi355x_confidence.h; DESIGN "Mapping confidence").  Kernels: hmx_confidence.hip, k_query_stats<2> of hmx_query.hip.
// The calls keep no state on the handle but the timers: every device buffer lives for one call (hmx_api_call.inc).

namespace {

constexpr size_t CONF_PART_BYTES = (size_t)256 << 20;      // the moments' partial slots stay within this much HBM
constexpr int CONF_MAX_CHUNKS = 256;

// chunks of pass B: contiguous cells, a multiple of the flush unit (CONF_FLUSH tiles) each, as many as the slot budget allows (at most CONF_MAX_CHUNKS)
void conf_chunks(int64_t n, size_t slot_bytes, std::vector<Item>& chunks) {
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(CONF_MAX_CHUNKS, (int64_t)(CONF_PART_BYTES / slot_bytes)));
  const int64_t unit = 16 * CONF_FLUSH;
  int64_t per = (n + want - 1) / want;
  per = std::max<int64_t>(unit, (per + unit - 1) / unit * unit);
  chunks.clear();
  for (int64_t s = 0; s < n; s += per) chunks.push_back({0, (int)s, (int)std::min<int64_t>(per, n - s)});
}

// cov_k + ridge I = L L^T in fp64, then U = L^-1 (lower triangular) and the mean as the fp32 tables of k_conf_score; false: not positive definite
bool conf_whiten(const double* mean, const double* cov, int K, int d, int zs, int k, double ridge, float* U, float* mu) {
  std::vector<double> Lm((size_t)d * d, 0.0), Um((size_t)d * d, 0.0);
  const double* S = cov + (size_t)k * d * d;
  for (int j = 0; j < d; j++) {
    double s = S[(size_t)j * d + j] + ridge;
    for (int p = 0; p < j; p++) s -= Lm[(size_t)j * d + p] * Lm[(size_t)j * d + p];
    if (!(s > 0) || !std::isfinite(s)) return false;
    const double ljj = std::sqrt(s);
    Lm[(size_t)j * d + j] = ljj;
    for (int i = j + 1; i < d; i++) {
      double t = S[(size_t)i * d + j];
      for (int p = 0; p < j; p++) t -= Lm[(size_t)i * d + p] * Lm[(size_t)j * d + p];
      Lm[(size_t)i * d + j] = t / ljj;
    }
  }
  for (int c = 0; c < d; c++) {
    Um[(size_t)c * d + c] = 1.0 / Lm[(size_t)c * d + c];
    for (int i = c + 1; i < d; i++) {
      double t = 0.0;
      for (int p = c; p < i; p++) t += Lm[(size_t)i * d + p] * Um[(size_t)p * d + c];
      Um[(size_t)i * d + c] = -t / Lm[(size_t)i * d + i];
    }
  }
  for (int i = 0; i < d; i++) {
    for (int c = 0; c <= i; c++) {
      if (!std::isfinite(Um[(size_t)i * d + c])) return false;
      U[((size_t)k * zs + i) * zs + c] = (float)Um[(size_t)i * d + c];
    }
    mu[(size_t)k * zs + i] = (float)mean[k + (size_t)K * i];
  }
  return true;
}

}  // namespace

extern "C" {

int hmx_reference_moments(hmx_ctx* ctx, int32_t space, double* mean, double* cov) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (space != HMX_SPACE_ORIG && space != HMX_SPACE_CORR) return fail(ctx, HMX_ERR_ARG, "space must be HMX_SPACE_ORIG or HMX_SPACE_CORR");
  if (!mean || !cov) return fail(ctx, HMX_ERR_ARG, "null output");
  if (ctx->query_done) return fail(ctx, HMX_ERR_STATE, "a query handle has no reference moments: call this on the fitted handle");
  if (!ctx->ran_setup || !ctx->ran_init) return fail(ctx, HMX_ERR_STATE, "no fitted state on this handle: setup and init_cluster first");
  if (!ctx->R_valid) return fail(ctx, HMX_ERR_STATE, "R is not available: the clustering call that would have stored it did not complete");
  HIPCHK(hipSetDevice(ctx->device));
  CHK(sync_solve_results(ctx));      // (a singular system of the last correction surfaces here, as in hmx_get_matrix)
  const double t0 = now_ms();
  const Dev& D = ctx->D;
  const int K = ctx->K, d = ctx->d, zs = D.zs;
  const float* rows = space == HMX_SPACE_CORR ? D.Zc : D.Zo;

  // ---- pass A: S0 = sum R, sum R^2, sum R z per cluster (sharded: the global sums on every rank)
  const int W = query_stats_width(d, 2);
  std::vector<double> A;
  {
    QueryDev Q{};
    Q.n = (int)ctx->N; Q.d = d; Q.K = K; Q.zs = zs; Q.KP16 = (K + 15) / 16 * 16;
    Q.Zsum = rows; Q.Rsum = D.R;
    std::vector<int> start = {0, (int)ctx->N};
    std::vector<Item> chunks; std::vector<int> qchunk;
    query_chunks(start, ctx->N, 512, chunks, qchunk);
    CHK(query_sums(ctx, Q, 2, chunks, qchunk, A));
  }
  std::vector<float> c((size_t)K * zs, 0.f);
  for (int k = 0; k < K; k++) {
    const double S0 = A[(size_t)k * W + d];
    if (!(S0 > 0) || !std::isfinite(S0)) return fail(ctx, HMX_ERR_SOLVE, "reference moments: cluster " + std::to_string(k) + " holds no mass (sum R = 0)");
    for (int j = 0; j < d; j++) c[(size_t)k * zs + j] = (float)(A[(size_t)k * W + j] / S0);
  }

  // ---- pass B: the second and first moments about c_k = fl32(mu_k), upper triangle of 16 x 16 tiles
  ConfMomDev P{};
  P.Z = rows; P.R = D.R; P.K = K; P.zs = zs; P.NG = (zs + 15) / 16; P.npairs = P.NG * (P.NG + 1) / 2; P.E = 256 * P.npairs + 16 * P.NG;
  const size_t total = (size_t)K * P.E;
  std::vector<Item> chunks;
  conf_chunks(ctx->N, total * sizeof(double), chunks);
  P.nchunks = (int)chunks.size();
  const int fold[2] = {0, P.nchunks};
  std::vector<double> M(total);
  {
    CallBufs B;
    float* dc; Item* dch; int* dfold; double* dres;
    HIPCHK(B.put(&dc, c.data(), c.size(), ctx->L.stream)); HIPCHK(B.put(&dch, chunks.data(), chunks.size(), ctx->L.stream));
    HIPCHK(B.put(&dfold, fold, 2, ctx->L.stream));
    HIPCHK(B.get(&P.part, (size_t)P.nchunks * total)); HIPCHK(B.get(&dres, total));
    P.c = dc; P.chunks = dch;
    hipError_t e = hipSuccess;
    if (P.nchunks) { l_conf_moments(ctx->L, P); e = hipGetLastError(); }
    if (e == hipSuccess) { l_query_fold(ctx->L, P.part, dfold, 1, (int)total, dres); e = hipGetLastError(); }
    int st = 0;
    if (e == hipSuccess) st = allreduce(ctx, dres, (int64_t)total, 1);      // sharded handle: the global sums on every rank
    if (e == hipSuccess && !st) e = download(M.data(), dres, total, ctx->L.stream);
    const hipError_t es = hipStreamSynchronize(ctx->L.stream);      // (the buffers are released below: nothing may still use them)
    if (st) return st;
    if (e != hipSuccess || es != hipSuccess) return fail(ctx, HMX_ERR_DEVICE, std::string("reference moments: ") + hipGetErrorString(e != hipSuccess ? e : es));
  }

  // ---- the moments in fp64: mu = c + delta with delta = sum R (z - c) / S0, and sum R (z - mu)(z - mu)^T = sum R y y^T - S0 delta delta^T exactly
  std::vector<double> delta((size_t)d);
  for (int k = 0; k < K; k++) {
    const double S0 = A[(size_t)k * W + d], S2 = A[(size_t)k * W + d + 1];
    const double den = 1.0 - S2 / (S0 * S0);
    if (!(den > 0)) return fail(ctx, HMX_ERR_SOLVE, "reference moments: cluster " + std::to_string(k) + " has no unbiased covariance (1 - sum w^2 <= 0)");
    const double* slot = &M[(size_t)k * P.E];
    for (int j = 0; j < d; j++) {
      delta[j] = slot[(size_t)256 * P.npairs + j] / S0;
      mean[k + (size_t)K * j] = (double)c[(size_t)k * zs + j] + delta[j];
    }
    double* Sk = cov + (size_t)k * d * d;
    int p = 0;
    for (int a = 0; a < P.NG; a++)
      for (int b = a; b < P.NG; b++, p++) {
        const double* T = slot + (size_t)256 * p;
        for (int i = 0; i < 16; i++)
          for (int r = 0; r < 16; r++) {
            const int j = 16 * a + i, j2 = 16 * b + r;
            if (j > j2 || j2 >= d) continue;       // (a diagonal tile holds both halves: the upper one is kept and mirrored)
            const double v = (T[4 * (16 * (i >> 2) + r) + (i & 3)] / S0 - delta[j] * delta[j2]) / den;
            Sk[(size_t)j * d + j2] = v; Sk[(size_t)j2 * d + j] = v;
          }
      }
  }
  ctx->timers["reference_moments"] = now_ms() - t0;
  return 0;
}

int hmx_mapping_confidence(hmx_ctx* ctx, int32_t space, const double* mean, const double* cov, int32_t K, int32_t d,
                           double ridge, double* score, float* dist) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (space != HMX_SPACE_ORIG && space != HMX_SPACE_CORR) return fail(ctx, HMX_ERR_ARG, "space must be HMX_SPACE_ORIG or HMX_SPACE_CORR");
  if (!mean || !cov || !score) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (!(ridge >= 0) || !std::isfinite(ridge)) return fail(ctx, HMX_ERR_ARG, "ridge must be finite and non-negative");
  if (K <= 0 || d <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (K > 256 || d > 128) return fail(ctx, HMX_ERR_ARG, "K and d must equal the handle's (K <= 256, d <= 128)");
  for (int64_t i = 0; i < (int64_t)K * d; i++) if (!std::isfinite(mean[i])) return fail(ctx, HMX_ERR_ARG, "mean must be finite");
  for (int64_t i = 0; i < (int64_t)K * d * d; i++) if (!std::isfinite(cov[i])) return fail(ctx, HMX_ERR_ARG, "cov must be finite");
  if (!ctx->query_done) return fail(ctx, HMX_ERR_STATE, "hmx_mapping_confidence needs a query handle: hmx_map_query first");
  if (K != ctx->K || d != ctx->d)
    return fail(ctx, HMX_ERR_ARG, "the moments have K = " + std::to_string(K) + ", d = " + std::to_string(d) + ", the handle K = " + std::to_string(ctx->K) +
                                  ", d = " + std::to_string(ctx->d));
  const double t0 = now_ms();
  const Dev& D = ctx->D;
  const int zs = D.zs;
  const int64_t Nq = ctx->N;

  // ---- K Cholesky factors and their inverses in fp64 on the host -> the fp32 tables
  std::vector<float> U((size_t)K * zs * zs, 0.f), mu((size_t)K * zs, 0.f);
  std::vector<int> bad((size_t)K, 0);
  {
    unsigned nt = std::thread::hardware_concurrency(); if (nt < 1) nt = 1; if (nt > 16) nt = 16; if ((int)nt > K) nt = K;
    if ((size_t)K * d * d * d < 4000000) nt = 1;
    auto run = [&](int k) { bad[k] = conf_whiten(mean, cov, K, d, zs, k, ridge, U.data(), mu.data()) ? 0 : 1; };
    if (nt == 1) for (int k = 0; k < K; k++) run(k);
    else {
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] { for (int k = (int)t; k < K; k += (int)nt) run(k); });
      for (auto& x : th) x.join();
    }
  }
  for (int k = 0; k < K; k++)
    if (bad[k]) return fail(ctx, HMX_ERR_SOLVE, "mapping confidence: cov + ridge I of cluster " + std::to_string(k) + " is not positive definite");

  HIPCHK(hipSetDevice(ctx->device));
  CallBufs B;
  ConfDev P{};
  P.Q = ctx->qd; P.Q.out = nullptr; P.Q.Rout = nullptr;
  P.Zs = space == HMX_SPACE_CORR ? D.Zc : D.Zo;
  P.perm = D.perm;
  float* dU; float* dmu;
  HIPCHK(B.put(&dU, U.data(), U.size(), ctx->L.stream)); HIPCHK(B.put(&dmu, mu.data(), mu.size(), ctx->L.stream));
  HIPCHK(B.get(&P.score, (size_t)Nq));
  P.dist = nullptr;
  if (dist) HIPCHK(B.get(&P.dist, (size_t)Nq * K));
  P.U = dU; P.mu = dmu;
  l_conf_score(ctx->L, P); KCHK();
  HIPCHK(download(score, P.score, (size_t)Nq, ctx->L.stream));
  if (dist) HIPCHK(download(dist, P.dist, (size_t)Nq * K, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  ctx->timers["mapping_confidence"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
