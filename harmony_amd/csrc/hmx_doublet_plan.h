// hmx_doublet_plan.h -- the launch plan of the doublet simulation (hmx_simulate_doublets; kernel k_doublet_project in hmx_doublets.hip).
// A pure function of (G, d, n_sim).  Plain C++17 like hmx_group_plan.h and hmx_ranksum_plan.h: no HIP, no handle
// (tests/cpp/doublet_plan_probe.cpp drives it on the CPU; hmx_api_doublets.inc launches what it returns).
//
// A wave owns one synthetic cell at a time and keeps in LDS a table of one fp32 word per reference gene (stride gp = G rounded up to the 64
// slots of a sweep) and a queue of DBL_QUEUE (slot, weight) pairs.  waves: as many waves per workgroup, of 4, 2, 1, as keep
// waves (4 gp + 8 DBL_QUEUE) bytes within DBL_LDS_BYTES; a G that one wave's table cannot hold is outside the envelope.
// grid: a workgroup per `waves` cells, at most DBL_MAX_GRID (the cells then go round in a grid-stride loop).
#pragma once
#include <stdint.h>
#include <algorithm>

namespace hmx {

constexpr int DBL_QUEUE = 128;                // entries of a wave's queue: a sweep appends at most 64 to fewer than 64 waiting ones
constexpr int DBL_LDS_BYTES = 64 * 1024;      // of a workgroup
constexpr int DBL_MAX_D = 128;
constexpr int DBL_MAX_GRID = 256 * 8;

// the largest G whose tables `waves` waves can hold
constexpr int doublet_max_genes(int waves) { return (DBL_LDS_BYTES - waves * DBL_QUEUE * 8) / (4 * waves) / 64 * 64; }
constexpr int DBL_MAX_GENES = doublet_max_genes(1);

struct DoubletPlan {
  int waves = 0;            // per workgroup
  int gp = 0;               // words of a wave's table
  int lds_bytes = 0;        // dynamic LDS of a workgroup
  int nc = 0;               // 64-PC chunks a lane accumulates: 1 | 2
  unsigned grid = 0;
};

enum { DBL_PLAN_OK = 0, DBL_PLAN_GENES = 1, DBL_PLAN_PCS = 2, DBL_PLAN_ARG = 3 };

inline int doublet_plan(int32_t G, int32_t d, int64_t n_sim, DoubletPlan& out) {
  out = DoubletPlan();
  if (G < 1 || d < 1 || n_sim < 1) return DBL_PLAN_ARG;
  if (d > DBL_MAX_D) return DBL_PLAN_PCS;
  if (G > DBL_MAX_GENES) return DBL_PLAN_GENES;
  out.waves = G <= doublet_max_genes(4) ? 4 : G <= doublet_max_genes(2) ? 2 : 1;
  out.gp = (G + 63) / 64 * 64;
  out.lds_bytes = out.waves * (4 * out.gp + 8 * DBL_QUEUE);
  out.nc = (d + 63) / 64;
  out.grid = (unsigned)std::min<int64_t>((n_sim + out.waves - 1) / out.waves, DBL_MAX_GRID);
  return DBL_PLAN_OK;
}

}  // namespace hmx
