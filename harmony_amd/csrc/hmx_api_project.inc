// hmx_api_project.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_project_counts
// (include/harmony_mi355x_project.h; DESIGN "Projecting query counts").  Kernel: hmx_project.hip.  The count matrix's checks, sweep and tables
// are the count-matrix seam's (hmx_api_csr.inc).  The call keeps no state on the handle but the timer: every device buffer lives for one call.

extern "C" {

int hmx_project_counts(hmx_ctx* ctx, int64_t Nq, int32_t G_all, const int64_t* indptr, const int32_t* indices, const void* data,
                       int32_t data_dtype, int32_t csr_location, const int32_t* slot, const double* U, const double* mean, const double* sd,
                       int32_t G, int32_t d, double scale, double clip, const double* totals, void* out, int32_t out_location) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->err.clear();
  CHK(csr_args(ctx, Nq, G_all, indptr, indices, data, data_dtype, csr_location, scale, totals));
  if (!slot || !U || !mean || !sd || !out) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (G <= 0 || d <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (out_location != HMX_HOST && out_location != HMX_DEVICE) return fail(ctx, HMX_ERR_ARG, "a location must be HMX_HOST or HMX_DEVICE");
  if (d > 128) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= 128");
  if (G > (1 << 24)) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: G, G_all <= 2^24");
  if (std::isnan(clip) || std::isinf(clip)) return fail(ctx, HMX_ERR_ARG, "clip must be finite (<= 0: none)");
  CHK(gene_moments_check(ctx, mean, sd, G, "reference gene"));
  for (int64_t i = 0; i < (int64_t)G * d; i++) if (!std::isfinite(U[i])) return fail(ctx, HMX_ERR_ARG, "the loadings must be finite");
  std::vector<char> present;
  CHK(gene_slot_check(ctx, slot, G_all, G, "slot", "query genes to reference gene", present));
  const int esz = data_dtype == HMX_F32 ? 4 : 8;
  const double t0 = now_ms();      // (the timer covers the host's pass over a host-resident matrix)
  if (csr_location == HMX_HOST) CHK(csr_host_pass(ctx, Nq, G_all, indptr, indices));
  CHK(call_device(ctx));

  // ---- the tables: b in fp64, the rest as the kernel's fp32
  const int zs = (d + 63) / 64 * 64;
  std::vector<float> U32((size_t)G * zs, 0.f), inv_sd, cap;
  std::vector<double> b((size_t)d, 0.0);
  gene_tables(mean, sd, G, clip, inv_sd, cap);
  for (int32_t j = 0; j < G; j++) {
    const double c = -mean[j] / sd[j];
    for (int32_t q = 0; q < d; q++) {
      U32[(size_t)j * zs + q] = (float)U[(size_t)j * d + q];
      if (present[(size_t)j]) b[(size_t)q] += c * U[(size_t)j * d + q];
    }
  }

  CallBufs B;
  ProjDev P{};
  hipStream_t st = ctx->L.stream;
  int* dslot; float* dU; float* dinv; float* dcap; double* db; float* dout;
  HIPCHK(B.put(&dslot, slot, (size_t)G_all, st)); HIPCHK(B.put(&dU, U32.data(), U32.size(), st)); HIPCHK(B.put(&dinv, inv_sd.data(), (size_t)G, st));
  HIPCHK(B.put(&dcap, cap.data(), (size_t)G, st)); HIPCHK(B.put(&db, b.data(), (size_t)d, st));
  CHK(csr_uploads(ctx, B, P, Nq, G_all, data_dtype, scale, totals));
  if (out_location == HMX_DEVICE) dout = (float*)out; else HIPCHK(B.get(&dout, (size_t)Nq * d));
  P.slot = dslot; P.U = dU; P.inv_sd = dinv; P.cap = dcap; P.b = db; P.G = G; P.d = d; P.out = dout;

  CHK(csr_sweep(ctx, B, Nq, indptr, indices, data, esz, csr_location, "project", [&](const CsrRows& R) { R.into(P); l_project(ctx->L, P, st); }));
  if (out_location == HMX_HOST) HIPCHK(download((float*)out, dout, (size_t)Nq * d, st));
  CHK(csr_flag(ctx, P));
  ctx->timers["project"] = now_ms() - t0;
  return 0;
}

}  // extern "C"
