// hmx_api_call.inc -- part of hmx_api.cpp (included there, ONE translation unit, ahead of the sections that use it: metrics, silhouette,
// confidence, project): what a call that keeps no state on the handle needs -- its device and stream, its device buffers, the ingest of
// a matrix of rows, the argument checks, and the rows a metric scores (the caller's X or the handle's own embedding).

namespace {

struct CallBufs {        // device buffers of one call
  std::vector<void*> v;
  ~CallBufs() { for (void* p : v) (void)hipFree(p); }
  template <class T> hipError_t get(T** p, size_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) v.push_back(q);
    *p = (T*)q;
    return e;
  }
};

int call_device(hmx_ctx* ctx) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ctx, HMX_ERR_DEVICE, "no HIP device available: libharmony_mi355x has no CPU fallback");
  if (ctx->device < 0) { int cur = 0; (void)hipGetDevice(&cur); ctx->device = cur; }
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->L.stream) { HIPCHK(hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking)); ctx->own_stream = true; }
  return 0;
}

// rows of either element type, host or HBM -> fp32 rows of stride zs and squared norms, both owned by `B`
int call_rows(hmx_ctx* ctx, CallBufs& B, const void* X, int32_t dtype, int32_t location, int64_t N, int32_t d, int zs, float** rows, float** nrm) {
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

// ---- the rows a metric scores: the caller's X, or (X == nullptr) the handle's current Z_corr ----------------------------------------------
// the argument errors of such a call, then (score_limits) those of the envelope; a caller's own argument checks go between the two.
// With the handle's own embedding d becomes the handle's.
int score_args(hmx_ctx* ctx, const void* X, int32_t dtype, int32_t location, int64_t N, int32_t& d, const void* out) {
  if (!X) {
    if (!(ctx->ran_setup || ctx->query_done)) return fail(ctx, HMX_ERR_STATE, "no embedding on this handle: setup or map_query first, or pass X");
    if (N != ctx->N) return fail(ctx, HMX_ERR_ARG, "N is not the handle's cell count");
    d = ctx->d;
  } else {
    CHK(check_rows(ctx, X, dtype, location, "X"));
  }
  if (!out) return fail(ctx, HMX_ERR_ARG, "null output");
  if (N <= 0 || d <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  return 0;
}
int score_limits(hmx_ctx* ctx, int64_t N, int32_t d) {
  if (d > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= 128");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  return 0;
}
// ... and their ingest (call_rows); Z_corr is read in the order the cells were given in
int score_rows(hmx_ctx* ctx, CallBufs& B, const void* X, int32_t dtype, int32_t location, int64_t N, int32_t d, int zs, float** rows, float** nrm) {
  if (X) return call_rows(ctx, B, X, dtype, location, N, d, zs, rows, nrm);
  CHK(sync_solve_results(ctx));      // (a singular system of the last correction surfaces here, as in hmx_get_matrix)
  float* dense;
  HIPCHK(B.get(&dense, (size_t)N * d));
  l_convert_out(ctx->L, ctx->D.Zc, dense, 1, ctx->D.invperm, ctx->D.n, d, ctx->D.zs); KCHK();
  return call_rows(ctx, B, dense, HMX_F32, HMX_DEVICE, N, d, zs, rows, nrm);
}

}  // namespace
