// hmx_api_ranksum.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_rank_sums (include/harmony_mi355x_ranksum.h; DESIGN
// "Rank sums per group").  Kernels: hmx_ranksum.hip; the plan: hmx_ranksum_plan.h.  The count matrix's checks, sweep and gene map are the
// count-matrix seam's (hmx_api_csr.inc).  The call leaves nothing on the handle but its timers and the number of gene blocks it ran
// ("ranksum_blocks").

namespace {
constexpr int64_t RANKSUM_LIST_BYTES = (int64_t)8 << 30;      // a gene block's list and second buffer (the "ranksum_list_bytes" lab field overrides it)
}

extern "C" {

int hmx_rank_sums(hmx_ctx* ctx, int64_t N, int32_t G_all, const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype,
                  int32_t csr_location, double scale, const double* totals, const int32_t* labels, int32_t B, const int32_t* gene_slot, int32_t G,
                  int64_t* n_obs, int64_t* n_pos, int64_t* rank2, uint64_t* tie3) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(csr_args(ctx, N, G_all, indptr, indices, data, data_dtype, csr_location, scale, totals));
  if (!labels) return fail(ctx, HMX_ERR_ARG, "null labels");
  if (!n_obs || !n_pos || !rank2 || !tie3) return fail(ctx, HMX_ERR_ARG, "null output");
  if (B <= 0) return fail(ctx, HMX_ERR_ARG, "at least one group");
  if (G <= 0) return fail(ctx, HMX_ERR_ARG, "at least one selected gene");
  if (!gene_slot && G != G_all) return fail(ctx, HMX_ERR_ARG, "a null gene_slot selects every gene: G must be G_all");
  if (B > 4096 || (int64_t)B * G > ((int64_t)1 << 25)) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: B <= 4096, B G <= 2^25");
  std::vector<char> taken;
  if (gene_slot) CHK(gene_slot_check(ctx, gene_slot, G_all, G, "gene_slot", "genes to output row", taken));
  std::vector<int64_t> obs((size_t)B, 0);
  int64_t Nk = 0;
  for (int64_t i = 0; i < N; i++) {
    if (labels[i] < -1 || labels[i] >= B) return fail(ctx, HMX_ERR_ARG, "a label is outside [-1, B) (cell " + std::to_string(i) + ")");
    if (labels[i] >= 0) { obs[(size_t)labels[i]]++; Nk++; }
  }
  if (Nk > ((int64_t)1 << 30)) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: at most 2^30 cells with a label");
  const double t0 = now_ms();
  const int esz = data_dtype == HMX_F32 ? 4 : 8;
  if (csr_location == HMX_HOST) CHK(csr_host_pass(ctx, N, G_all, indptr, indices));
  CHK(call_device(ctx));
  hipStream_t st = ctx->L.stream;
  const size_t cells = (size_t)B * G;
  CallBufs bufs;
  RankSweepDev S{};
  CHK(csr_uploads(ctx, bufs, S.C, N, G_all, data_dtype, scale, totals));
  int* dlabels; int* dslot = nullptr; unsigned long long* dcount;
  HIPCHK(bufs.put(&dlabels, labels, (size_t)N, st)); HIPCHK(bufs.get(&dcount, (size_t)G));
  HIPCHK(zero_fill(dcount, (size_t)G, st));
  if (gene_slot) HIPCHK(bufs.put(&dslot, gene_slot, (size_t)G_all, st));
  S.C.slot = dslot; S.C.G = G; S.labels = dlabels; S.count = dcount;
  auto sweep = [&](bool fill) {
    CallBufs staging;      // (a pass returns with its streams drained: a sweep's staging sets are gone before the next one allocates its own)
    return csr_sweep(ctx, staging, N, indptr, indices, data, esz, csr_location, "rank_sums",
                     [&](const CsrRows& R) { R.into(S.C); l_rank_sweep(S, fill, st); });
  };
  // ---- the count sweep (it validates the matrix), then the plan
  S.j0 = 0; S.j1 = G;
  CHK(sweep(false));
  std::vector<int64_t> count((size_t)G);
  HIPCHK(download(count.data(), dcount, (size_t)G, st));      // (the counts are read as they are)
  CHK(csr_flag(ctx, S.C));
  const double t_count = now_ms();
  for (int32_t j = 0; j < G; j++)
    if (count[(size_t)j] > Nk) return fail(ctx, HMX_ERR_ARG, "a row stores a gene more than once (output row " + std::to_string(j) + ")");
  RankSumPlan plan;
  int32_t bad_gene = 0;
  if (ranksum_plan(count.data(), G, ctx->ranksum_list_bytes > 0 ? ctx->ranksum_list_bytes : RANKSUM_LIST_BYTES, RS_SORT_LDS, plan, &bad_gene))
    return fail(ctx, HMX_ERR_DEVICE, "rank_sums: a negative count");
  const int64_t nblocks = (int64_t)plan.block.size() - 1;
  bool radix = false;
  for (int32_t j = 0; j < G; j++) radix = radix || plan.path[(size_t)j] == RANKSUM_RADIX;
  long long* dseg; unsigned* dcursor; int* dorder; unsigned* dnext; unsigned long long* dlist; unsigned long long* dother;
  unsigned long long* drank; unsigned* dnpos; unsigned long long* dtie;
  HIPCHK(bufs.put(&dseg, plan.seg.data(), (size_t)G + 1, st)); HIPCHK(bufs.get(&dcursor, (size_t)G)); HIPCHK(bufs.put(&dorder, plan.order.data(), plan.order.size(), st));
  HIPCHK(bufs.get(&dnext, (size_t)nblocks)); HIPCHK(bufs.get(&dlist, (size_t)plan.max_entries)); HIPCHK(bufs.get(&dother, radix ? (size_t)plan.max_entries : 1));
  HIPCHK(bufs.get(&drank, cells)); HIPCHK(bufs.get(&dnpos, cells)); HIPCHK(bufs.get(&dtie, 2 * (size_t)G));
  HIPCHK(zero_fill(dcursor, (size_t)G, st));
  HIPCHK(zero_fill(dnext, (size_t)nblocks, st));
  HIPCHK(zero_fill(drank, cells, st));
  HIPCHK(zero_fill(dnpos, cells, st));
  HIPCHK(zero_fill(dtie, 2 * (size_t)G, st));
  S.seg = dseg; S.cursor = dcursor; S.list = dlist;
  RankSortDev R{};
  R.seg = dseg; R.list = dlist; R.other = dother; R.B = B; R.G = G; R.Nk = Nk; R.rank2 = drank; R.npos = dnpos; R.tie3 = dtie;
  double ms_fill = 0, ms_sort = 0;
  // ---- per gene block: one fill sweep, then every gene of the block is sorted and ranked
  for (int64_t k = 0; k < nblocks; k++) {
    const int32_t j0 = plan.block[(size_t)k], j1 = plan.block[(size_t)k + 1];
    const int64_t entries = plan.seg[(size_t)j1] - plan.seg[(size_t)j0];
    if (entries <= 0) continue;
    const double ta = now_ms();
    HIPCHK(zero_fill(dlist, (size_t)entries, st));      // (a host matrix that changes between two sweeps leaves defined entries)
    S.j0 = j0; S.j1 = j1; S.base = plan.seg[(size_t)j0]; S.entries = entries;
    CHK(sweep(true));
    HIPCHK(hipStreamSynchronize(st));      // (a device-resident sweep returns with its kernel queued: the stage timers are split here)
    const double tb = now_ms();
    R.base = S.base; R.entries = entries; R.order = dorder + plan.first[(size_t)k]; R.ngenes = (int)(plan.first[(size_t)k + 1] - plan.first[(size_t)k]);
    R.next = dnext + k;
    l_rank_sort(R, st); KCHK();
    HIPCHK(hipStreamSynchronize(st));
    ms_fill += tb - ta; ms_sort += now_ms() - tb;
  }
  std::vector<unsigned long long> hrank(cells), htie(2 * (size_t)G);
  std::vector<unsigned> hnpos(cells);
  HIPCHK(download(hrank.data(), drank, cells, st));
  HIPCHK(download(hnpos.data(), dnpos, cells, st));
  HIPCHK(download(htie.data(), dtie, htie.size(), st));
  CHK(csr_flag(ctx, S.C));
  // ---- the zeros' share: a cell without a positive entry of gene g has the doubled midrank z_g + 1, z_g = N_k - P_g
  for (int32_t b = 0; b < B; b++) {
    n_obs[b] = obs[(size_t)b];
    for (int32_t j = 0; j < G; j++) {
      const size_t c = (size_t)b * G + j;
      const int64_t z = Nk - count[(size_t)j];
      n_pos[c] = (int64_t)hnpos[c];
      rank2[c] = (int64_t)hrank[c] + (obs[(size_t)b] - (int64_t)hnpos[c]) * (z + 1);
    }
  }
  for (size_t i = 0; i < htie.size(); i++) tie3[i] = (uint64_t)htie[i];
  ctx->ranksum_blocks = nblocks;
  ctx->timers["rank_sums_count"] = t_count - t0;
  ctx->timers["rank_sums_fill"] = ms_fill;
  ctx->timers["rank_sums_sort"] = ms_sort;
  ctx->timers["rank_sums"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
