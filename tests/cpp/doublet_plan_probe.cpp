// Host-side probe of the launch plan of the doublet simulation (harmony_amd/csrc/hmx_doublet_plan.h, HIP-free): built by
// tests/test_doublets_cpu.py with the host compiler and called through ctypes.
#include "../../harmony_amd/csrc/hmx_doublet_plan.h"

// -> the plan's status (DBL_PLAN_*); out = {waves, gp, lds_bytes, nc, grid}
extern "C" int probe_doublet_plan(int G, int d, long long n_sim, long long* out) {
  hmx::DoubletPlan p;
  const int st = hmx::doublet_plan(G, d, n_sim, p);
  out[0] = p.waves; out[1] = p.gp; out[2] = p.lds_bytes; out[3] = p.nc; out[4] = (long long)p.grid;
  return st;
}

// the constants the plan is derived from: {queue entries, LDS bytes of a workgroup, largest G at 4, 2, 1 waves, largest d, largest grid}
extern "C" void probe_doublet_constants(long long* out) {
  out[0] = hmx::DBL_QUEUE; out[1] = hmx::DBL_LDS_BYTES; out[2] = hmx::doublet_max_genes(4); out[3] = hmx::doublet_max_genes(2);
  out[4] = hmx::doublet_max_genes(1); out[5] = hmx::DBL_MAX_D; out[6] = hmx::DBL_MAX_GRID;
}
