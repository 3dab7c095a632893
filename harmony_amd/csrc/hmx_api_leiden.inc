// hmx_api_leiden.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_leiden (include/harmony_mi355x_leiden.h; DESIGN
// "Leiden clustering").  Kernels: hmx_leiden.hip; the weights' check, the quantisation and the aggregation: hmx_louvain.hip, with the refined
// partition in the place of comm; the pattern's checks, the scans and the segment sort: hmx_graph.hip.  Device, stream and buffers are the call
// seam's (hmx_api_call.inc, CallBufs).  The call keeps no state on the handle but the timers and the counters of the last call.  The host forms
// g = resolution / M once, reads the counts of moves and of blocked pairs in one copy per sweep, the level's C, tot and in once per level, and
// adds the level's modularity in ascending order of the communities' ids (lv_modularity's operations).

namespace {

// Q over the ids in use, in ascending order: lv_modularity's terms
double ld_modularity(const std::vector<unsigned>& used, const std::vector<long long>& in, const std::vector<long long>& tot, long long M, double resolution) {
#pragma clang fp contract(off)
  const double dM = (double)M;
  double Q = 0.0;
  bool first = true;
  for (size_t c = 0; c < tot.size(); c++) {
    if (!used[c]) continue;
    const double a = (double)in[c] / dM;
    const double t = (double)tot[c] / dM;
    const double rt = resolution * t;
    const double p = rt * t;
    const double term = a - p;
    Q = first ? term : Q + term;
    first = false;
  }
  return Q;
}

struct LdOut {
  int32_t* labels; int32_t* n_clusters; double* modularity; int32_t* converged;
  int32_t* level_clusters; int32_t* level_nodes; int32_t* level_sweeps; int32_t* level_refine_sweeps; double* level_modularity;
};

int leiden_device(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, double resolution,
                  int32_t max_levels, int32_t max_sweeps, const LdOut& out) {
  hipStream_t st = ctx->L.stream;
  CallBufs B;
  const int64_t nnz = indptr[N];
  const int short_cap = ctx->louvain_short_cap >= 0 ? (int)std::min<int64_t>(ctx->louvain_short_cap, LV_SHORT_CAP) : LV_SHORT_CAP;
  // ---- the caller's graph: Louvain's checks, integer weights and degrees
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
  std::vector<long long> hk((size_t)N);
  HIPCHK(download(hk.data(), I.k, (size_t)N, st));
  HIPCHK(hipStreamSynchronize(st));
  long long M = 0;
  for (long long v : hk) M += v;
  ctx->leiden_clusters = N;
  if (M == 0) {                                          // no edge of a positive weight: every cell its own cluster
    for (int64_t i = 0; i < N; i++) out.labels[i] = (int32_t)i;
    *out.n_clusters = (int32_t)N; *out.modularity = 0.0; *out.converged = 1;
    ctx->leiden_converged = 1;
    return 0;
  }
  const double g = resolution / (double)M;

  // ---- buffers every level uses, sized for level 0 (a level never has more nodes or entries than the one before)
  LdDev D{};
  LvAgg A{};
  long long* bsum; long long* newid; long long* soff; int* lab; int* comm2; unsigned* words; unsigned* pmin;      // words: nlong, moved, blocked, the sort's nlong
  GraphDev G{};
  HIPCHK(B.get(&D.comm, (size_t)N)); HIPCHK(B.get(&comm2, (size_t)N)); HIPCHK(B.get(&D.tot, (size_t)N)); HIPCHK(B.get(&D.target, (size_t)N));
  HIPCHK(B.get(&D.longrows, (size_t)N)); HIPCHK(B.get(&D.ref, (size_t)N)); HIPCHK(B.get(&D.rtot, (size_t)N)); HIPCHK(B.get(&D.size, (size_t)N));
  HIPCHK(B.get(&D.ok, (size_t)N)); HIPCHK(B.get(&D.cut, (size_t)N)); HIPCHK(B.get(&D.cin, (size_t)N)); HIPCHK(B.get(&pmin, (size_t)N));
  HIPCHK(B.get(&words, 4));
  D.nlong = words; D.moved = words + 1; D.blocked = words + 2; G.nlong = words + 3;
  HIPCHK(B.get(&A.mark, (size_t)N)); HIPCHK(B.get(&newid, (size_t)N + 1)); HIPCHK(B.get(&bsum, ((size_t)N + GR_SCAN_CHUNK - 1) / GR_SCAN_CHUNK + 1));
  HIPCHK(B.get(&A.ecount, (size_t)N)); HIPCHK(B.get(&soff, (size_t)N + 1)); HIPCHK(B.get(&A.cursor, (size_t)N)); HIPCHK(B.get(&A.len, (size_t)N));
  HIPCHK(B.get(&lab, (size_t)N));
  D.mark = A.mark;
  A.newid = newid; A.soff = soff; A.lab = lab; A.cells = N;

  // ---- level 0's graph: the entries that are edges (no diagonal, no q == 0)
  LdKeep K{};
  long long* kptr;
  HIPCHK(B.get(&kptr, (size_t)N + 1));
  K.N = N; K.indptr = dptr; K.indices = dind; K.q = I.q; K.cnt = A.len; K.kptr = kptr;
  l_ld_keep(ctx->L, K, false); KCHK();
  l_graph_scan(ctx->L, A.len, N, kptr, bsum); KCHK();
  long long knnz = 0;
  HIPCHK(download(&knnz, kptr + N, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  if (knnz < 1 || knnz > nnz) return fail(ctx, HMX_ERR_INTERNAL, "leiden: the edges do not add up");
  HIPCHK(B.get(&K.kindices, (size_t)knnz)); HIPCHK(B.get(&K.kq, (size_t)knnz));
  l_ld_keep(ctx->L, K, true); KCHK();
  HIPCHK(B.get(&A.keys, (size_t)knnz)); HIPCHK(B.get(&G.tother, (size_t)knnz)); HIPCHK(B.get(&G.longrows, (size_t)knnz / GR_WAVE_KEYS + 1));
  G.tkey = A.keys; G.toff = soff;

  // the level's graph: the kept entries at level 0, then the coarse graph of the aggregation before
  long long n = N, lnnz = knnz;
  const long long* lptr = kptr; const int* lind = K.kindices; const long long* lq = K.kq; const long long* lk = I.k; const long long* lin = nullptr;
  D.n = n;
  l_ld_iota(ctx->L, D); KCHK();
  bool composed = false;                                 // lab holds the cells' nodes (before the first aggregation a cell is its node)
  int converged = 0;
  long long Cn = N;
  double Q = 0.0;
  double t_moves = 0.0, t_refine = 0.0, t_agg = 0.0;
  std::vector<long long> htot, hin;
  std::vector<unsigned> hused;
  for (int level = 0; level < max_levels; level++) {
    double t0 = now_ms();
    D.n = n; D.indptr = lptr; D.indices = lind; D.q = lq; D.k = lk; D.in = lin; D.g = g; D.short_cap = short_cap;
    // ---- 1. local moves from comm
    HIPCHK(zero_fill(words, 4, st));
    HIPCHK(zero_fill(D.tot, (size_t)n, st));
    l_ld_start(ctx->L, D); KCHK();
    unsigned nlong = 0;
    HIPCHK(download(&nlong, D.nlong, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (level == 0) ctx->leiden_long_rows = (int64_t)nlong;
    int sweeps = 0, rsweeps = 0;
    unsigned long long moved_total = 0;
    for (int t = 0; t < max_sweeps; t++) {
      D.key = h_fmix32((uint32_t)(64u * (uint32_t)t + (uint32_t)level + 1u));
      HIPCHK(zero_fill(D.moved, 1, st));
      for (int b = 0; b < LV_SUBROUNDS; b++) {
        D.bucket = b;
        l_ld_decide(ctx->L, D, nlong > 0); KCHK();
        l_ld_apply(ctx->L, D); KCHK();
      }
      unsigned moved = 0;
      HIPCHK(download(&moved, D.moved, 1, st));
      HIPCHK(hipStreamSynchronize(st));
      sweeps++; ctx->leiden_sweeps++;
      moved_total += moved;
      if (!moved) break;
    }
    // ---- 2. the level's record: C, tot and in per community id
    HIPCHK(zero_fill(D.cin, (size_t)n, st)); HIPCHK(zero_fill(D.mark, (size_t)n, st));
    l_ld_sums(ctx->L, D); KCHK();
    l_graph_scan(ctx->L, D.mark, n, newid, bsum); KCHK();
    htot.resize((size_t)n); hin.resize((size_t)n); hused.resize((size_t)n);
    HIPCHK(download(&Cn, newid + n, 1, st));
    HIPCHK(download(htot.data(), D.tot, (size_t)n, st)); HIPCHK(download(hin.data(), D.cin, (size_t)n, st));
    HIPCHK(download(hused.data(), D.mark, (size_t)n, st));
    HIPCHK(hipStreamSynchronize(st));
    if (Cn < 1 || Cn > n) return fail(ctx, HMX_ERR_INTERNAL, "leiden: the communities do not add up");
    Q = ld_modularity(hused, hin, htot, M, resolution);
    const int rec = (int)ctx->leiden_levels;
    if (out.level_clusters) out.level_clusters[rec] = (int32_t)Cn;
    if (out.level_nodes) out.level_nodes[rec] = (int32_t)n;
    if (out.level_sweeps) out.level_sweeps[rec] = sweeps;
    if (out.level_refine_sweeps) out.level_refine_sweeps[rec] = 0;
    if (out.level_modularity) out.level_modularity[rec] = Q;
    ctx->leiden_levels = rec + 1;
    t_moves += now_ms() - t0;
    // ---- 3. every node a community of its own: converged; the last level allowed: the call ends with comm as well (newid: comm's numbering)
    A.n = n; A.comm = D.comm;
    if (Cn == n) { converged = 1; break; }
    if (level == max_levels - 1) break;
    // ---- 4. refinement inside the communities of comm
    t0 = now_ms();
    l_ld_refine_setup(ctx->L, D); KCHK();
    for (int t = 0; t < max_sweeps; t++) {
      D.key = h_fmix32((uint32_t)(64u * (uint32_t)t + (uint32_t)level + 1u) ^ 0xFFFFFFFFu);
      HIPCHK(zero_fill(D.moved, 2, st));                 // moved, blocked
      for (int b = 0; b < LV_SUBROUNDS; b++) {
        D.bucket = b;
        HIPCHK(zero_fill(D.cut, (size_t)n, st));
        l_ld_cut(ctx->L, D); KCHK();
        l_ld_refine_decide(ctx->L, D, nlong > 0); KCHK();
        l_ld_refine_apply(ctx->L, D); KCHK();
      }
      unsigned mb[2] = {0, 0};
      HIPCHK(download(mb, D.moved, 2, st));
      HIPCHK(hipStreamSynchronize(st));
      rsweeps++; ctx->leiden_refine_sweeps++;
      if (!mb[0] && !mb[1]) break;
    }
    if (out.level_refine_sweeps) out.level_refine_sweeps[rec] = rsweeps;
    t_refine += now_ms() - t0;
    // ---- 5. aggregation by ref (Louvain's, ref in the place of comm)
    t0 = now_ms();
    A.indptr = lptr; A.indices = lind; A.q = lq; A.k = lk; A.in = lin; A.comm = D.ref;
    HIPCHK(zero_fill(A.mark, (size_t)n, st));
    l_lv_mark(ctx->L, A); KCHK();
    l_graph_scan(ctx->L, A.mark, n, newid, bsum); KCHK();
    long long Rn = 0;
    HIPCHK(download(&Rn, newid + n, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (Rn < Cn || Rn > n) return fail(ctx, HMX_ERR_INTERNAL, "leiden: the refined communities do not add up");
    if (out.level_nodes) out.level_nodes[rec] = (int32_t)Rn;
    if (Rn == n && !moved_total) {                       // a guard: nothing merged and nothing moved.  The call ends with comm.
      A.comm = D.comm;
      HIPCHK(zero_fill(A.mark, (size_t)n, st));
      l_lv_mark(ctx->L, A); KCHK();
      l_graph_scan(ctx->L, A.mark, n, newid, bsum); KCHK();
      break;
    }
    A.C = Rn;
    long long* cptr;
    HIPCHK(B.get(&A.ck, (size_t)Rn)); HIPCHK(B.get(&A.cin, (size_t)Rn)); HIPCHK(B.get(&cptr, (size_t)Rn + 1));
    HIPCHK(zero_fill(A.ck, (size_t)Rn, st)); HIPCHK(zero_fill(A.cin, (size_t)Rn, st));
    HIPCHK(zero_fill(A.ecount, (size_t)Rn, st)); HIPCHK(zero_fill(A.cursor, (size_t)Rn, st)); HIPCHK(zero_fill(G.nlong, 1, st));
    l_lv_count(ctx->L, A); KCHK();
    l_graph_scan(ctx->L, A.ecount, Rn, soff, bsum); KCHK();
    l_lv_place(ctx->L, A); KCHK();
    G.N = Rn;
    l_graph_sort(ctx->L, G); KCHK();
    l_lv_reduce(ctx->L, A, false); KCHK();
    l_graph_scan(ctx->L, A.len, Rn, cptr, bsum); KCHK();
    long long cnnz = 0;
    HIPCHK(download(&cnnz, cptr + Rn, 1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (cnnz < 0 || cnnz > lnnz) return fail(ctx, HMX_ERR_INTERNAL, "leiden: the coarse rows do not add up");
    HIPCHK(B.get(&A.cindices, (size_t)cnnz)); HIPCHK(B.get(&A.cq, (size_t)cnnz));
    A.cindptr = cptr;
    l_lv_reduce(ctx->L, A, true); KCHK();
    l_lv_compose(ctx->L, A, !composed); KCHK();
    composed = true;
    // the next level's start: the refined parts of one community together, under the smallest new id among them
    LdNext X{};
    X.n = n; X.C = Rn; X.comm = D.comm; X.ref = D.ref; X.newid = newid; X.pmin = pmin; X.next = comm2;
    HIPCHK(hipMemsetAsync(pmin, 0xff, (size_t)n * sizeof(unsigned), st));
    l_ld_parent(ctx->L, X); KCHK();
    HIPCHK(hipStreamSynchronize(st));
    std::swap(D.comm, comm2);
    n = Rn; lnnz = cnnz; lptr = cptr; lind = A.cindices; lq = A.cq; lk = A.ck; lin = A.cin;
    t_agg += now_ms() - t0;
  }
  // ---- the last level's partition: the communities in use, numbered in ascending id
  A.C = Cn;
  l_lv_compose(ctx->L, A, !composed); KCHK();
  HIPCHK(download(out.labels, lab, (size_t)N, st));
  HIPCHK(hipStreamSynchronize(st));
  *out.n_clusters = (int32_t)Cn; *out.modularity = Q; *out.converged = converged;
  ctx->leiden_clusters = Cn; ctx->leiden_converged = converged;
  ctx->timers["leiden_moves"] = t_moves; ctx->timers["leiden_refine"] = t_refine; ctx->timers["leiden_aggregate"] = t_agg;
  return 0;
}

}  // namespace

extern "C" {

int hmx_leiden(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, double resolution,
               int32_t max_levels, int32_t max_sweeps, int32_t* labels, int32_t* n_clusters, double* modularity, int32_t* converged,
               int32_t* level_clusters, int32_t* level_nodes, int32_t* level_sweeps, int32_t* level_refine_sweeps, double* level_modularity) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  if (!indptr || !labels || !n_clusters || !modularity || !converged) return fail(ctx, HMX_ERR_ARG, "null argument");
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
  ctx->leiden_levels = ctx->leiden_sweeps = ctx->leiden_refine_sweeps = ctx->leiden_clusters = ctx->leiden_converged = ctx->leiden_long_rows = 0;
  CHK(call_device(ctx));
  const double t0 = now_ms();
  const LdOut out{labels, n_clusters, modularity, converged, level_clusters, level_nodes, level_sweeps, level_refine_sweeps, level_modularity};
  const int s = leiden_device(ctx, indptr, indices, weights, N, resolution, max_levels, max_sweeps, out);
  ctx->timers["leiden"] = now_ms() - t0;
  return s;
}

}  // extern "C"
