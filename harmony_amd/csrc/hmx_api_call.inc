// hmx_api_call.inc -- part of hmx_api.cpp (included there, ONE translation unit, ahead of every section of a call that keeps no state on the
// handle): the call seam.  What such a call needs and shares with its siblings, in one flat layer that no feature section adds to: its device
// and stream, the ingest of a matrix of rows and the argument checks, the rows a metric scores (the caller's X or the handle's own embedding),
// the exact search the "search then score" calls start with, and what the two graph calls share -- the check of neighbour lists, the
// transposed lists and the emit of a CSR matrix.  (A call's device buffers and their typed copies: CallBufs, hmx_api_seam.inc; the
// count-matrix calls' seam: hmx_api_csr.inc.)

namespace {

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
    char* raw = nullptr;      // (bytes: the element size is a run-time value)
    HIPCHK(B.put(&raw, (const char*)X, bytes, ctx->L.stream));
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

// ---- the exact search (hmx_knn.hip) -----------------------------------------------------------------------------------------------------------
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
int knn_device(hmx_ctx* ctx, CallBufs& B, KnnDev P) {
  P.NG = (P.zs + 15) / 16;
  knn_plan(P);
  P.part = nullptr;
  if (P.nchunks > 1) HIPCHK(B.get(&P.part, (size_t)P.Nq * P.nchunks * P.k));
  l_knn(ctx->L, P); KCHK();
  return 0;
}

// The front of a call that searches, then scores: the rows it scores (score_rows), every row's m nearest other rows as device lists [N][m] owned
// by `B`, copied to idx_out / dist_out where those are given.  It returns with the stream drained, the clock read then in K.t1 and
// timers["knn"] = K.t1 - t0.
struct KnnLists { int* idx; float* dist; double t1; };
int knn_front(hmx_ctx* ctx, CallBufs& B, double t0, const void* X, int32_t dtype, int32_t location, int64_t N, int32_t d, int32_t m,
              int32_t* idx_out, float* dist_out, KnnLists& K) {
  KnnDev P{};
  P.zs = (d + 3) / 4 * 4; P.k = m; P.excl = 1; P.N = P.Nq = N;
  float* xr; float* xn;
  CHK(score_rows(ctx, B, X, dtype, location, N, d, P.zs, &xr, &xn));
  P.X = P.Q = xr; P.xn = P.qn = xn;
  const size_t cnt = (size_t)N * m;
  HIPCHK(B.get(&P.idx, cnt)); HIPCHK(B.get(&P.dist, cnt));
  CHK(knn_device(ctx, B, P));
  if (idx_out) HIPCHK(download(idx_out, P.idx, cnt, ctx->L.stream));
  if (dist_out) HIPCHK(download(dist_out, P.dist, cnt, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  K.idx = P.idx; K.dist = P.dist; K.t1 = now_ms();
  ctx->timers["knn"] = K.t1 - t0;
  return 0;
}

// scanpy's n_neighbors and Seurat's k.param count the cell itself: `name` says which one the caller has
int check_neighbor_count(hmx_ctx* ctx, const char* name, int32_t k, int64_t N) {
  static_assert(SNN_MAX_K == 129, "the envelope's text");
  if (k < 2 || k > SNN_MAX_K) return fail(ctx, HMX_ERR_LIMIT, std::string("supported envelope: 2 <= ") + name + " <= 129");
  if (k > N) return fail(ctx, HMX_ERR_LIMIT, std::string(name) + " counts the cell itself: at most N");
  return 0;
}

// ---- what the graph calls share (hmx_graph.hip) -----------------------------------------------------------------------------------------------
// host neighbour lists idx [N][m], self excluded, -1: an unfilled slot; dist (or nullptr): no NaN beside a valid index; no_duplicates: no cell
// twice in a row.  The first error in row order is reported, within a row the entries' before the duplicates'.
int check_lists(hmx_ctx* ctx, const int32_t* idx, const float* dist, bool no_duplicates, int64_t N, int32_t m) {
  if (N <= 0 || m <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (m > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: at most 128 neighbours");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows");
  std::vector<int32_t> row((size_t)m);
  for (int64_t i = 0; i < N; i++) {
    for (int32_t j = 0; j < m; j++) {
      const int32_t v = idx[(size_t)i * m + j];
      if (v < -1 || v >= N) return fail(ctx, HMX_ERR_ARG, "neighbour index outside [-1, N) (row " + std::to_string(i) + ")");
      if (v == i) return fail(ctx, HMX_ERR_ARG, "row " + std::to_string(i) + " lists its own cell: the lists exclude self");
      if (dist && v >= 0 && std::isnan(dist[(size_t)i * m + j])) return fail(ctx, HMX_ERR_ARG, "NaN distance (row " + std::to_string(i) + ")");
      row[(size_t)j] = v;
    }
    if (!no_duplicates) continue;
    std::sort(row.begin(), row.end());
    for (int32_t j = 1; j < m; j++)
      if (row[(size_t)j] >= 0 && row[(size_t)j] == row[(size_t)j - 1]) return fail(ctx, HMX_ERR_ARG, "row " + std::to_string(i) + " lists a cell twice");
  }
  return 0;
}

int graph_outputs(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t capacity) {
  if (!indptr) return fail(ctx, HMX_ERR_ARG, "null indptr");
  if (capacity < 0) return fail(ctx, HMX_ERR_ARG, "negative capacity");
  if (capacity > 0 && (!indices || !weights)) return fail(ctx, HMX_ERR_ARG, "null indices / weights with a positive capacity");
  return 0;
}

// The transposed lists of G.idx [N][m] (G.toff, G.tkey, sorted per row): buffers owned by `B`, counters zeroed, then `degree` -- the caller's
// kernels that count G.deg, returning a status -- and scan, place, sort.  *bsum: the scan's work space, kept for csr_offsets.
template <class F>
int transposed_lists(hmx_ctx* ctx, CallBufs& B, GraphDev& G, long long** bsum, F degree) {
  hipStream_t st = ctx->L.stream;
  const size_t N = (size_t)G.N, cnt = N * G.m;
  HIPCHK(B.get(&G.deg, N)); HIPCHK(B.get(&G.toff, N + 1));
  HIPCHK(B.get(&G.tkey, cnt)); HIPCHK(B.get(&G.tother, cnt));
  HIPCHK(B.get(&G.longrows, cnt / GR_WAVE_KEYS + 1)); HIPCHK(B.get(&G.nlong, 1));
  HIPCHK(B.get(bsum, (N + GR_SCAN_CHUNK - 1) / GR_SCAN_CHUNK + 1));
  HIPCHK(zero_fill(G.deg, N, st));
  HIPCHK(zero_fill(G.nlong, 1, st));
  CHK(degree());
  l_graph_scan(ctx->L, G.deg, G.N, G.toff, *bsum); KCHK();
  l_graph_place(ctx->L, G); KCHK();
  l_graph_sort(ctx->L, G); KCHK();
  return 0;
}

// The emit of a CSR matrix of N rows in two steps.  csr_offsets: the row lengths `len` scanned into *dindptr (owned by `B`), whose copy to the
// host's indptr is queued -- the caller adds what else it reads back and synchronises.  csr_entries: indptr[N] held to `bound` (`what` names
// the stage in the error), the refusal when it exceeds `capacity` -- the callers' retry reads that text --, then indices / weights in HBM.
int csr_offsets(hmx_ctx* ctx, CallBufs& B, unsigned* len, int64_t N, long long* bsum, int64_t* indptr, long long** dindptr) {
  HIPCHK(B.get(dindptr, (size_t)N + 1));
  l_graph_scan(ctx->L, len, N, *dindptr, bsum); KCHK();
  HIPCHK(download(indptr, *dindptr, (size_t)N + 1, ctx->L.stream));
  return 0;
}
int csr_entries(hmx_ctx* ctx, CallBufs& B, const char* what, int64_t nnz, double bound, int64_t capacity, int** indices, float** weights) {
  if (nnz < 0 || (double)nnz > bound) return fail(ctx, HMX_ERR_DEVICE, std::string(what) + ": the row lengths do not add up");
  if (capacity < nnz) return fail(ctx, HMX_ERR_LIMIT, "capacity " + std::to_string(capacity) + " is below the graph's " + std::to_string(nnz) + " entries (indptr is written)");
  HIPCHK(B.get(indices, (size_t)nnz)); HIPCHK(B.get(weights, (size_t)nnz));
  return 0;
}

}  // namespace
