// hmx_api_groups.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_gene_stats_grouped (include/harmony_mi355x_groups.h;
// DESIGN "Gene statistics per group").  Kernel: k_gene_stats_grouped in hmx_pca.hip; the work list: hmx_group_plan.h.  The count matrix's
// checks, slabs, sweep and fixed-point steps are the count-matrix seam's (hmx_api_csr.inc).  The call leaves nothing on the handle but the timer.

extern "C" {

int hmx_gene_stats_grouped(hmx_ctx* ctx, int64_t N, int32_t G_all, const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype,
                           int32_t csr_location, double scale, const double* totals, const int32_t* labels, int32_t B, int64_t* n_obs, int64_t* n,
                           double* s1, double* s2, double* step) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(csr_args(ctx, N, G_all, indptr, indices, data, data_dtype, csr_location, scale, totals));
  if (!labels) return fail(ctx, HMX_ERR_ARG, "null labels");
  if (!n_obs || !n || !s1 || !s2) return fail(ctx, HMX_ERR_ARG, "null output");
  if (B <= 0) return fail(ctx, HMX_ERR_ARG, "at least one group");
  if (B > 4096 || (int64_t)B * G_all > ((int64_t)1 << 25)) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: B <= 4096, B G_all <= 2^25");
  const double t0 = now_ms();
  const int esz = data_dtype == HMX_F32 ? 4 : 8;
  if (csr_location == HMX_HOST) CHK(csr_host_pass(ctx, N, G_all, indptr, indices));
  // the slabs csr_sweep will cut (a pure function of indptr and the cap), then the chunks of every slab, once
  std::vector<int64_t> slab{0, N};
  if (csr_location == HMX_HOST) {
    slab.assign(1, 0);
    for (const CsrSlab& s : csr_slabs(indptr, N, csr_slab_cap(ctx, esz))) slab.push_back(s.row1);
  }
  GroupPlan plan;
  int64_t bad_cell = 0;
  if (group_plan(labels, N, B, slab.data(), (int64_t)slab.size() - 1, GROUP_CHUNK, plan, &bad_cell))
    return fail(ctx, HMX_ERR_ARG, "a label is outside [-1, B) (cell " + std::to_string(bad_cell) + ")");
  CHK(call_device(ctx));
  const GeneSteps T = gene_steps(N, scale, totals != nullptr);      // the steps of hmx_gene_stats
  const int F1 = T.F1, F2 = T.F2;
  CallBufs bufs;
  GroupStatDev Q{};
  PcaStatDev& S = Q.S;
  CHK(csr_uploads(ctx, bufs, S.C, N, G_all, data_dtype, scale, totals));
  hipStream_t st = ctx->L.stream;
  const size_t cells = (size_t)B * G_all;
  unsigned long long* acc; int* dperm; GroupChunk* dchunks;
  HIPCHK(bufs.get(&acc, 3 * cells)); HIPCHK(bufs.get(&dperm, plan.perm.size())); HIPCHK(bufs.get(&dchunks, plan.chunks.size()));
  HIPCHK(zero_fill(acc, 3 * cells, st));
  HIPCHK(upload(dperm, plan.perm.data(), plan.perm.size(), st));
  HIPCHK(upload(dchunks, plan.chunks.data(), plan.chunks.size(), st));
  S.ymax = T.ymax; S.q1 = std::ldexp(1.0, F1); S.q2 = std::ldexp(1.0, F2); S.s1 = acc; S.s2 = acc + cells; S.n = acc + 2 * cells;
  Q.perm = dperm;
  bool cut_ok = true;      // every launch found its slab in the table cut above
  CHK(csr_sweep(ctx, bufs, N, indptr, indices, data, esz, csr_location, "gene_stats_grouped",
                [&](const CsrRows& R) {
                  R.into(S.C);
                  const size_t s = (size_t)(std::lower_bound(slab.begin(), slab.end(), (int64_t)R.row0) - slab.begin());      // the slab that starts at row0
                  if (s + 1 >= slab.size() || slab[s] != R.row0 || slab[s + 1] != R.row0 + R.nrows) { cut_ok = false; return; }
                  Q.chunks = dchunks + plan.first[s]; Q.nchunks = plan.first[s + 1] - plan.first[s];
                  l_gene_stats_grouped(Q, st);
                }));
  if (!cut_ok) return fail(ctx, HMX_ERR_STATE, "gene_stats_grouped: the sweep's slabs are not the ones the chunks were cut for");
  std::vector<unsigned long long> h(3 * cells);
  HIPCHK(download(h.data(), acc, h.size(), st));
  CHK(csr_flag(ctx, S.C));
  for (size_t c = 0; c < cells; c++) {
    s1[c] = std::ldexp((double)h[c], -F1);
    s2[c] = std::ldexp((double)h[cells + c], -F2);
    n[c] = (int64_t)h[2 * cells + c];
  }
  for (int32_t b = 0; b < B; b++) n_obs[b] = plan.n_obs[(size_t)b];
  if (step) { step[0] = std::ldexp(1.0, -F1); step[1] = std::ldexp(1.0, -F2); }
  ctx->timers["gene_stats_grouped"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
