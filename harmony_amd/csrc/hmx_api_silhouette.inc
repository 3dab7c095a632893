// hmx_api_silhouette.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_silhouette
// (include/harmony_mi355x_silhouette.h; DESIGN "Silhouette widths").  Kernels: hmx_silhouette.hip.  The call keeps no state on the handle
// but the timer: every device buffer lives for one call (hmx_api_call.inc).

namespace {

// The sorted layout of one call (host side): cells ordered by (group, label) with a stable sort -- within a segment the cells keep the order
// they were given in --, every (group, label) segment padded to a multiple of 16 rows, and the table of its 16-row tiles.
struct SilLayout {
  std::vector<int32_t> src;        // [Np] the cell of a sorted row, -1: padding
  std::vector<SilTile> tile;       // [Np / 16]
  std::vector<int32_t> grange;     // [groups present][2] tiles [first, end)
};

SilLayout sil_layout(const int32_t* labels, int32_t n_levels, const int32_t* groups, int32_t n_groups, int64_t N) {
  const int64_t K = (int64_t)(groups ? n_groups : 1) * n_levels;
  auto key = [&](int64_t i) { return (int64_t)(groups ? groups[i] : 0) * n_levels + labels[i]; };
  std::vector<int32_t> order((size_t)N);
  if (K <= std::max<int64_t>(1 << 20, 4 * N)) {      // counting sort
    std::vector<int64_t> at((size_t)K + 1, 0);
    for (int64_t i = 0; i < N; i++) at[(size_t)key(i) + 1]++;
    for (int64_t k = 0; k < K; k++) at[(size_t)k + 1] += at[(size_t)k];
    for (int64_t i = 0; i < N; i++) order[(size_t)at[(size_t)key(i)]++] = (int32_t)i;
  } else {                                            // (level counts far above the cell count: no table of that size)
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return key(x) < key(y); });
  }
  SilLayout Y;
  Y.src.reserve((size_t)N + 1024);
  int32_t prev_group = -1;
  for (int64_t i = 0; i < N;) {
    const int64_t k = key(order[(size_t)i]);
    int64_t j = i;
    while (j < N && key(order[(size_t)j]) == k) j++;
    const int32_t grp = (int32_t)(k / n_levels), lab = (int32_t)(k % n_levels), count = (int32_t)(j - i);
    if (grp != prev_group) {
      if (!Y.grange.empty()) Y.grange.back() = (int32_t)Y.tile.size();
      Y.grange.push_back((int32_t)Y.tile.size());
      Y.grange.push_back(0);
      prev_group = grp;
    }
    const int32_t dense = (int32_t)(Y.grange.size() / 2 - 1);
    for (int64_t r = i; r < j; r += 16) {
      const int32_t rows = (int32_t)std::min<int64_t>(16, j - r);
      Y.tile.push_back(SilTile{dense, lab, rows | (r + 16 >= j ? 1 << 8 : 0), count});
      for (int32_t q = 0; q < 16; q++) Y.src.push_back(q < rows ? order[(size_t)(r + q)] : -1);
    }
    i = j;
  }
  Y.grange.back() = (int32_t)Y.tile.size();
  return Y;
}

}  // namespace

extern "C" {

int hmx_silhouette(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d,
                   const int32_t* labels, int32_t n_levels, const int32_t* groups, int32_t n_groups,
                   double* s, double* a, double* b) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(score_args(ctx, X, x_dtype, x_location, N, d, s));      // (X == nullptr: the handle's current Z_corr)
  CHK(score_limits(ctx, N, d));
  CHK(check_labels(ctx, labels, N, 1, &n_levels));
  if (groups) CHK(check_labels(ctx, groups, N, 1, &n_groups));
  CHK(call_device(ctx));
  const double t0 = now_ms();
  const SilLayout Y = sil_layout(labels, n_levels, groups, n_groups, N);
  if (Y.src.size() > 2000000000ull) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 rows once every (group, label) segment is padded to 16");
  CallBufs B;
  SilDev P{};
  P.zs = (d + 3) / 4 * 4; P.NG = (P.zs + 15) / 16; P.Np = (long long)Y.src.size();
  float* xr; float* xn;
  CHK(score_rows(ctx, B, X, x_dtype, x_location, N, d, P.zs, &xr, &xn));
  int* dsrc; SilTile* dtile; int* dgrange; float* sr; float* sn;
  HIPCHK(B.put(&dsrc, Y.src.data(), Y.src.size(), ctx->L.stream)); HIPCHK(B.put(&dtile, Y.tile.data(), Y.tile.size(), ctx->L.stream));
  HIPCHK(B.put(&dgrange, Y.grange.data(), Y.grange.size(), ctx->L.stream));
  HIPCHK(B.get(&sr, (size_t)P.Np * P.zs)); HIPCHK(B.get(&sn, (size_t)P.Np));
  HIPCHK(B.get(&P.s, (size_t)N)); HIPCHK(B.get(&P.a, (size_t)N)); HIPCHK(B.get(&P.b, (size_t)N));
  l_sil_gather(ctx->L, xr, xn, dsrc, P.Np, P.zs, sr, sn); KCHK();
  P.X = sr; P.xn = sn; P.src = dsrc; P.tile = dtile; P.grange = dgrange;
  l_silhouette(ctx->L, P); KCHK();
  HIPCHK(download(s, P.s, (size_t)N, ctx->L.stream));
  if (a) HIPCHK(download(a, P.a, (size_t)N, ctx->L.stream));
  if (b) HIPCHK(download(b, P.b, (size_t)N, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  ctx->timers["silhouette"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
