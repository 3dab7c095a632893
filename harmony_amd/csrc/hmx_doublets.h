// hmx_doublets.h -- what hmx_doublets.hip and hmx_api_doublets.inc share (include/harmony_mi355x_doublets.h; DESIGN "Doublet detection"):
// the device view of a doublet simulation and the two launchers.
#pragma once
#include "hmx_internal.h"
#include "hmx_doublet_plan.h"

namespace hmx {

struct DoubletDev {
  ProjDev C;                    // the WHOLE count matrix (base 0, nrows = N observed cells) and the reference's tables; out [n_sim][d]; totals [N] or nullptr
  const long long* pairs;       // [n_sim][2] the parents of every synthetic cell, each in [0, N) (checked on the host)
  long long n_sim;
  int gp;                       // words of a wave's slot table in LDS (DoubletPlan::gp)
};
void l_doublet_project(const Launch& L, const DoubletDev& D, const DoubletPlan& plan, hipStream_t stream);

// cnt[i] = the entries of row i of idx [N][m] that are >= n_obs (the synthetic cells among a row's neighbours)
void l_doublet_count(const Launch& L, const int* idx, long long N, int m, long long n_obs, int* cnt, hipStream_t stream);

}  // namespace hmx
