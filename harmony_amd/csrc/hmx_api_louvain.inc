// hmx_api_louvain.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_louvain (include/harmony_mi355x_louvain.h; DESIGN
// "Louvain clustering").  Kernels: hmx_louvain.hip; the pattern's checks, the scans and the segment sort: hmx_graph.hip.  Device, stream and
// buffers are the call seam's (hmx_api_call.inc, CallBufs).  The call keeps no state on the handle but the timer and the counters of the last
// call.  The host forms g = resolution / M once, reads the count of moves once per sweep, and adds a level's modularity in ascending order of
// the communities: fp64, one operation per statement, never contracted.

namespace {

// Q = sum_c (in_c / M - (resolution * (tot_c / M)) * (tot_c / M)), added in ascending c
double lv_modularity(const std::vector<long long>& in, const std::vector<long long>& tot, long long M, double resolution) {
#pragma clang fp contract(off)
  const double dM = (double)M;
  double Q = 0.0;
  for (size_t c = 0; c < tot.size(); c++) {
    const double a = (double)(in.empty() ? 0ll : in[c]) / dM;
    const double t = (double)tot[c] / dM;
    const double rt = resolution * t;
    const double p = rt * t;
    const double term = a - p;
    Q = c == 0 ? term : Q + term;
  }
  return Q;
}

struct LvOut { int32_t* labels; int32_t* n_clusters; double* modularity; int32_t* level_clusters; int32_t* level_sweeps; double* level_modularity; };

int louvain_device(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, double resolution,
                   int32_t max_levels, int32_t max_sweeps, const LvOut& out) {
  hipStream_t st = ctx->L.stream;
  CallBufs B;
  const int64_t nnz = indptr[N];
  const int short_cap = ctx->louvain_short_cap >= 0 ? (int)std::min<int64_t>(ctx->louvain_short_cap, LV_SHORT_CAP) : LV_SHORT_CAP;
  // ---- the caller's graph: the pattern's and the weights' checks, integer weights, degrees
  long long* dptr; int* dind; float* dw; int* flags;
  HIPCHK(B.put(&dptr, indptr, (size_t)N + 1, st));
  HIPCHK(B.put(&dind, indices, (size_t)nnz, st)); HIPCHK(B.put(&dw, weights, (size_t)nnz, st));
  HIPCHK(B.get(&flags, 2));
  HIPCHK(zero_fill(flags, 2, st));
  CcDev C{};
  C.N = N; C.indptr = dptr; C.indices = dind; C.flag = flags;
  LvIn I{};
  I.N = N; I.indptr = dptr; I.indices = dind; I.weights = dw; I.flag = flags + 1;
  l_cc_check(ctx->L, C); KCHK();
  l_lv_check(ctx->L, I); KCHK();
  int flag[2] = {0, 0};
  HIPCHK(download(flag, flags, 2, st));
  HIPCHK(hipStreamSynchronize(st));
  if (flag[0] & GR_FLAG_RANGE) return fail(ctx, HMX_ERR_ARG, "an index of the graph is outside [0, N)");
  if (flag[0] & GR_FLAG_ORDER) return fail(ctx, HMX_ERR_ARG, "a row of the graph is not strictly ascending");
  if (flag[0] & GR_FLAG_ASYM) return fail(ctx, HMX_ERR_ARG, "the graph is not symmetric: an edge has no mirror");
  if (flag[1] & LV_FLAG_WEIGHT) return fail(ctx, HMX_ERR_ARG, "a weight is outside [0, 1] or not finite (divide by the largest weight first)");
  if (flag[1] & LV_FLAG_MIRROR) return fail(ctx, HMX_ERR_ARG, "the graph is not symmetric: an edge and its mirror carry different weights");
  HIPCHK(B.get(&I.q, (size_t)nnz)); HIPCHK(B.get(&I.k, (size_t)N));
  l_lv_quantise(ctx->L, I); KCHK();
  std::vector<long long> hk((size_t)N), hin;
  HIPCHK(download(hk.data(), I.k, (size_t)N, st));
  HIPCHK(hipStreamSynchronize(st));
  long long M = 0;
  for (long long v : hk) M += v;
  ctx->louvain_clusters = N;
  if (M == 0) {                                          // no edge of a positive weight: every cell its own cluster
    for (int64_t i = 0; i < N; i++) out.labels[i] = (int32_t)i;
    *out.n_clusters = (int32_t)N; *out.modularity = 0.0;
    return 0;
  }
  const double g = resolution / (double)M;
  double best_q = lv_modularity(hin, hk, M, resolution);
  int64_t best_c = N;

  // ---- buffers every level uses, sized for level 0 (a level never has more nodes or entries than the one before)
  LvDev D{};
  LvAgg A{};
  long long* bsum; long long* newid; long long* soff; int* lab; int* best; unsigned* words;      // words: nlong, moved, the sort's nlong
  GraphDev G{};
  HIPCHK(B.get(&D.comm, (size_t)N)); HIPCHK(B.get(&D.tot, (size_t)N)); HIPCHK(B.get(&D.target, (size_t)N)); HIPCHK(B.get(&D.longrows, (size_t)N));
  HIPCHK(B.get(&words, 3));
  D.nlong = words; D.moved = words + 1; G.nlong = words + 2;
  HIPCHK(B.get(&A.mark, (size_t)N)); HIPCHK(B.get(&newid, (size_t)N + 1)); HIPCHK(B.get(&bsum, ((size_t)N + GR_SCAN_CHUNK - 1) / GR_SCAN_CHUNK + 1));
  HIPCHK(B.get(&A.ecount, (size_t)N)); HIPCHK(B.get(&soff, (size_t)N + 1)); HIPCHK(B.get(&A.cursor, (size_t)N)); HIPCHK(B.get(&A.len, (size_t)N));
  HIPCHK(B.get(&A.keys, (size_t)nnz)); HIPCHK(B.get(&G.tother, (size_t)nnz)); HIPCHK(B.get(&G.longrows, (size_t)nnz / GR_WAVE_KEYS + 1));
  HIPCHK(B.get(&lab, (size_t)N)); HIPCHK(B.get(&best, (size_t)N));
  A.newid = newid; A.soff = soff; A.lab = lab; A.cells = N;
  G.tkey = A.keys; G.toff = soff;

  // the level's graph: the caller's at level 0, then the coarse graph of the aggregation before
  long long n = N, lnnz = nnz;
  const long long* lptr = dptr; const int* lind = dind; const long long* lq = I.q; const long long* lk = I.k; const long long* lin = nullptr;
  bool have_best = false;
  for (int level = 0; level < max_levels; level++) {
    D.n = n; D.indptr = lptr; D.indices = lind; D.q = lq; D.k = lk; D.g = g; D.short_cap = short_cap;
    HIPCHK(zero_fill(words, 3, st));
    l_lv_init(ctx->L, D); KCHK();
    unsigned nlong = 0;
    HIPCHK(download(&nlong, D.nlong, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (level == 0) ctx->louvain_long_rows = (int64_t)nlong;
    int sweeps = 0;
    unsigned long long moved_total = 0;
    for (int t = 0; t < max_sweeps; t++) {
      D.key = h_fmix32((uint32_t)(64u * (uint32_t)t + (uint32_t)level + 1u));
      HIPCHK(zero_fill(D.moved, 1, st));
      for (int b = 0; b < LV_SUBROUNDS; b++) {
        D.bucket = b;
        l_lv_decide(ctx->L, D, nlong > 0); KCHK();
        l_lv_apply(ctx->L, D); KCHK();
      }
      unsigned moved = 0;
      HIPCHK(download(&moved, D.moved, 1, st));
      HIPCHK(hipStreamSynchronize(st));
      sweeps++; ctx->louvain_sweeps++;
      moved_total += moved;
      if (!moved) break;
    }
    if (!moved_total) break;                             // nothing moved at this level: the call ends, the level is not recorded
    // ---- aggregation
    A.n = n; A.indptr = lptr; A.indices = lind; A.q = lq; A.k = lk; A.in = lin; A.comm = D.comm;
    HIPCHK(zero_fill(A.mark, (size_t)n, st));
    l_lv_mark(ctx->L, A); KCHK();
    l_graph_scan(ctx->L, A.mark, n, newid, bsum); KCHK();
    long long Cn = 0;
    HIPCHK(download(&Cn, newid + n, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (Cn < 1 || Cn > n) return fail(ctx, HMX_ERR_INTERNAL, "louvain: the communities do not add up");
    A.C = Cn;
    long long* cptr;
    HIPCHK(B.get(&A.ck, (size_t)Cn)); HIPCHK(B.get(&A.cin, (size_t)Cn)); HIPCHK(B.get(&cptr, (size_t)Cn + 1));
    HIPCHK(zero_fill(A.ck, (size_t)Cn, st)); HIPCHK(zero_fill(A.cin, (size_t)Cn, st));
    HIPCHK(zero_fill(A.ecount, (size_t)Cn, st)); HIPCHK(zero_fill(A.cursor, (size_t)Cn, st)); HIPCHK(zero_fill(G.nlong, 1, st));
    l_lv_count(ctx->L, A); KCHK();
    l_graph_scan(ctx->L, A.ecount, Cn, soff, bsum); KCHK();
    l_lv_place(ctx->L, A); KCHK();
    G.N = Cn;
    l_graph_sort(ctx->L, G); KCHK();
    l_lv_reduce(ctx->L, A, false); KCHK();
    l_graph_scan(ctx->L, A.len, Cn, cptr, bsum); KCHK();
    long long cnnz = 0;
    HIPCHK(download(&cnnz, cptr + Cn, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (cnnz < 0 || cnnz > lnnz) return fail(ctx, HMX_ERR_INTERNAL, "louvain: the coarse rows do not add up");
    HIPCHK(B.get(&A.cindices, (size_t)cnnz)); HIPCHK(B.get(&A.cq, (size_t)cnnz));
    A.cindptr = cptr;
    l_lv_reduce(ctx->L, A, true); KCHK();
    l_lv_compose(ctx->L, A, level == 0); KCHK();
    std::vector<long long> ck((size_t)Cn), cin((size_t)Cn);
    HIPCHK(download(ck.data(), A.ck, (size_t)Cn, st)); HIPCHK(download(cin.data(), A.cin, (size_t)Cn, st));
    HIPCHK(hipStreamSynchronize(st));
    const double Q = lv_modularity(cin, ck, M, resolution);
    const int rec = (int)ctx->louvain_levels;
    if (out.level_clusters) out.level_clusters[rec] = (int32_t)Cn;
    if (out.level_sweeps) out.level_sweeps[rec] = sweeps;
    if (out.level_modularity) out.level_modularity[rec] = Q;
    ctx->louvain_levels = rec + 1;
    if (Q > best_q) {                                    // the first level of the largest Q
      best_q = Q; best_c = Cn; have_best = true; ctx->louvain_best_level = rec + 1;
      HIPCHK(hipMemcpyAsync(best, lab, (size_t)N * sizeof(int), hipMemcpyDeviceToDevice, st));
    }
    n = Cn; lnnz = cnnz; lptr = cptr; lind = A.cindices; lq = A.cq; lk = A.ck; lin = A.cin;
  }
  if (have_best) HIPCHK(download(out.labels, best, (size_t)N, st));
  else for (int64_t i = 0; i < N; i++) out.labels[i] = (int32_t)i;
  HIPCHK(hipStreamSynchronize(st));
  *out.n_clusters = (int32_t)best_c; *out.modularity = best_q;
  ctx->louvain_clusters = best_c;
  return 0;
}

}  // namespace

extern "C" {

int hmx_louvain(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, double resolution,
                int32_t max_levels, int32_t max_sweeps, int32_t* labels, int32_t* n_clusters, double* modularity,
                int32_t* level_clusters, int32_t* level_sweeps, double* level_modularity) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!indptr || !labels || !n_clusters || !modularity) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (N < 1) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (!(resolution > 0.0 && resolution <= 100.0)) return fail(ctx, HMX_ERR_ARG, "resolution must lie in (0, 100]");
  if (max_levels < 1 || max_levels > 64) return fail(ctx, HMX_ERR_ARG, "max_levels must lie in 1 .. 64");
  if (max_sweeps < 1 || max_sweeps > 4096) return fail(ctx, HMX_ERR_ARG, "max_sweeps must lie in 1 .. 4096");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  if (indptr[0] != 0) return fail(ctx, HMX_ERR_ARG, "indptr must start at 0");
  for (int64_t i = 0; i < N; i++)
    if (indptr[i + 1] < indptr[i] || indptr[i + 1] - indptr[i] > N) return fail(ctx, HMX_ERR_ARG, "indptr must ascend by at most N per row (row " + std::to_string(i) + ")");
  const int64_t nnz = indptr[N];
  if (nnz >= (1ll << 31)) return fail(ctx, HMX_ERR_LIMIT, "at most 2^31 - 1 stored entries");
  if (nnz > 0 && (!indices || !weights)) return fail(ctx, HMX_ERR_ARG, "null indices / weights");
  ctx->louvain_levels = ctx->louvain_best_level = ctx->louvain_sweeps = ctx->louvain_clusters = ctx->louvain_long_rows = 0;
  CHK(call_device(ctx));
  const double t0 = now_ms();
  const LvOut out{labels, n_clusters, modularity, level_clusters, level_sweeps, level_modularity};
  const int s = louvain_device(ctx, indptr, indices, weights, N, resolution, max_levels, max_sweeps, out);
  ctx->timers["louvain"] = now_ms() - t0;
  return s;
}

}  // extern "C"
