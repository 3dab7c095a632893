// hmx_api_umap.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_umap_layout (include/harmony_mi355x_umap.h; DESIGN "The
// UMAP layout").  Kernels: hmx_umap.hip; the pattern's check: hmx_graph.hip; the weights' check: hmx_louvain.hip.  Device, stream and buffers
// are the call seam's (hmx_api_call.inc, CallBufs).  The call keeps no state on the handle but the timer and the counters of the last call.
// The host synchronises once, for the checks' flags, the largest weight and the count of long rows; from there every epoch is queued behind
// the one before it, over two position buffers that swap, and the last one is copied out.

namespace {

uint32_t um_h_fmix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}

struct UmArgs {
  int32_t dim, n_epochs, epoch_begin, epoch_end, negative_sample_rate;
  double a, b, gamma, learning_rate;
  uint32_t seed;
};

int umap_device(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, const float* Y0, const UmArgs& A, float* Y) {
  hipStream_t st = ctx->L.stream;
  CallBufs B;
  const int64_t nnz = indptr[N];
  const size_t cnt = (size_t)N * A.dim;
  const int short_cap = ctx->umap_short_cap >= 0 ? (int)std::min<int64_t>(ctx->umap_short_cap, 2147483647ll) : UM_SHORT_CAP;
  // ---- the caller's graph: the pattern's and the weights' checks, the largest weight, the long rows
  long long* dptr; int* dind; float* dw; int* flags; unsigned* words; float* ya; float* yb;      // words: wbits, nlong
  HIPCHK(B.put(&dptr, indptr, (size_t)N + 1, st));
  HIPCHK(B.put(&dind, indices, (size_t)nnz, st)); HIPCHK(B.put(&dw, weights, (size_t)nnz, st));
  HIPCHK(B.put(&ya, Y0, cnt, st)); HIPCHK(B.get(&yb, cnt));
  HIPCHK(B.get(&flags, 2)); HIPCHK(B.get(&words, 2));
  HIPCHK(zero_fill(flags, 2, st)); HIPCHK(zero_fill(words, 2, st));
  CcDev C{};
  C.N = N; C.indptr = dptr; C.indices = dind; C.flag = flags;
  LvIn I{};
  I.N = N; I.indptr = dptr; I.indices = dind; I.weights = dw; I.flag = flags + 1;
  UmDev D{};
  D.N = N; D.indptr = dptr; D.indices = dind; D.weights = dw; D.short_cap = short_cap;
  D.wbits = words; D.nlong = words + 1;
  HIPCHK(B.get(&D.longrows, (size_t)N)); HIPCHK(B.get(&D.fired, (size_t)N)); HIPCHK(B.get(&D.total, 1));
  HIPCHK(zero_fill(D.total, 1, st));
  l_cc_check(ctx->L, C); KCHK();
  l_lv_check(ctx->L, I); KCHK();
  l_um_wmax(ctx->L, D); KCHK();
  int flag[2] = {0, 0};
  unsigned word[2] = {0u, 0u};
  HIPCHK(download(flag, flags, 2, st)); HIPCHK(download(word, words, 2, st));
  HIPCHK(hipStreamSynchronize(st));
  if (flag[0] & GR_FLAG_RANGE) return fail(ctx, HMX_ERR_ARG, "an index of the graph is outside [0, N)");
  if (flag[0] & GR_FLAG_ORDER) return fail(ctx, HMX_ERR_ARG, "a row of the graph is not strictly ascending");
  if (flag[0] & GR_FLAG_ASYM) return fail(ctx, HMX_ERR_ARG, "the graph is not symmetric: an edge has no mirror");
  if (flag[1] & LV_FLAG_WEIGHT) return fail(ctx, HMX_ERR_ARG, "a weight is outside [0, 1] or not finite (divide by the largest weight first)");
  if (flag[1] & LV_FLAG_MIRROR) return fail(ctx, HMX_ERR_ARG, "the graph is not symmetric: an edge and its mirror carry different weights");
  ctx->umap_long_rows = (int64_t)word[1];
  float wmax;
  std::memcpy(&wmax, &word[0], sizeof wmax);
  if (!(wmax > 0.0f) || A.epoch_begin == A.epoch_end) {   // no edge of a positive weight, or no epoch asked for: the positions as they came
    std::memcpy(Y, Y0, cnt * sizeof(float));
    return 0;
  }
  // ---- the epochs: queued one behind the other, the two buffers swapping
  D.wmax = (double)wmax;
  D.a = (float)A.a; D.b = (float)A.b; D.m2ab = (float)(-2.0 * A.a * A.b); D.g2b = (float)(2.0 * A.gamma * A.b);
  D.nneg = A.negative_sample_rate;
  const uint32_t hseed = um_h_fmix32(A.seed);
  for (int n = A.epoch_begin; n < A.epoch_end; n++) {
    D.n = n;
    D.alpha = (float)(A.learning_rate * (1.0 - (double)n / (double)A.n_epochs));
    D.kbase = hseed + 32u * (uint32_t)n + 1u;
    D.yold = ya; D.ynew = yb;
    l_um_epoch(ctx->L, D, A.dim, word[1] > 0); KCHK();
    std::swap(ya, yb);
  }
  l_um_fired(ctx->L, D); KCHK();
  unsigned long long fired = 0;
  HIPCHK(download(&fired, D.total, 1, st));
  HIPCHK(download(Y, ya, cnt, st));
  HIPCHK(hipStreamSynchronize(st));
  ctx->umap_fired = (int64_t)fired;
  ctx->umap_epochs = A.epoch_end - A.epoch_begin;
  return 0;
}

}  // namespace

extern "C" {

int hmx_umap_layout(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, int32_t dim, const float* Y0,
                    int32_t n_epochs, int32_t epoch_begin, int32_t epoch_end, double a, double b, double gamma, double learning_rate,
                    int32_t negative_sample_rate, uint32_t seed, float* Y) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  ctx->umap_fired = ctx->umap_epochs = ctx->umap_long_rows = 0;
  if (!indptr || !Y0 || !Y) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (N < 1) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (dim != 2 && dim != 3) return fail(ctx, HMX_ERR_ARG, "dim must be 2 or 3");
  if (n_epochs < 1 || n_epochs > UM_MAX_EPOCHS) return fail(ctx, HMX_ERR_ARG, "n_epochs must lie in 1 .. 1048576");
  if (epoch_begin < 0 || epoch_end < epoch_begin || epoch_end > n_epochs) return fail(ctx, HMX_ERR_ARG, "the epochs [epoch_begin, epoch_end) must lie in [0, n_epochs)");
  if (!(a > 0.0 && std::isfinite(a)) || !(b > 0.0 && std::isfinite(b))) return fail(ctx, HMX_ERR_ARG, "a and b must be positive and finite");
  if (!(gamma >= 0.0 && std::isfinite(gamma))) return fail(ctx, HMX_ERR_ARG, "gamma must be non-negative and finite");
  if (!(learning_rate > 0.0 && std::isfinite(learning_rate))) return fail(ctx, HMX_ERR_ARG, "learning_rate must be positive and finite");
  if (negative_sample_rate < 0 || negative_sample_rate > UM_MAX_NEG) return fail(ctx, HMX_ERR_ARG, "negative_sample_rate must lie in 0 .. 31");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  if (indptr[0] != 0) return fail(ctx, HMX_ERR_ARG, "indptr must start at 0");
  for (int64_t i = 0; i < N; i++)
    if (indptr[i + 1] < indptr[i] || indptr[i + 1] - indptr[i] > N) return fail(ctx, HMX_ERR_ARG, "indptr must ascend by at most N per row (row " + std::to_string(i) + ")");
  const int64_t nnz = indptr[N];
  if (nnz >= (1ll << 31)) return fail(ctx, HMX_ERR_LIMIT, "at most 2^31 - 1 stored entries");
  if (nnz > 0 && (!indices || !weights)) return fail(ctx, HMX_ERR_ARG, "null indices / weights");
  for (int64_t t = 0; t < N * dim; t++)
    if (!std::isfinite(Y0[t])) return fail(ctx, HMX_ERR_ARG, "Y0 holds a value that is not finite (cell " + std::to_string(t / dim) + ")");
  CHK(call_device(ctx));
  const double t0 = now_ms();
  const UmArgs A{dim, n_epochs, epoch_begin, epoch_end, negative_sample_rate, a, b, gamma, learning_rate, seed};
  const int s = umap_device(ctx, indptr, indices, weights, N, Y0, A, Y);
  ctx->timers["umap"] = now_ms() - t0;
  return s;
}

}  // extern "C"
