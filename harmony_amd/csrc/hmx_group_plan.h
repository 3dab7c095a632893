// hmx_group_plan.h -- the work list of the grouped gene statistics (hmx_gene_stats_grouped; kernel k_gene_stats_grouped in hmx_pca.hip).
// A pure function of (labels, slab boundaries, B, the chunk constant).  Plain C++17 like hmx_plan.h: no HIP, no handle
// (tests/cpp/group_plan_probe.cpp drives it on the CPU; hmx_api_groups.inc uploads what it returns).
//
// perm   the cells with a label in [0, B), stably sorted by label: cells ascending within a group.
// chunks <= `chunk` consecutive entries of perm, all of ONE group and all inside ONE slab [slab[s], slab[s + 1]) of cells.  A slab's cells are a
//        contiguous sub-range of each group's part of perm, so the chunks are cut slab by slab, within a slab group by group, within a group in
//        order; slab s owns chunks [first[s], first[s + 1]).  Every kept cell lies in exactly one chunk; a cell labelled -1 in none.
// The list depends on nothing but its arguments: never on a grid, a device or the matrix's values.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace hmx {

struct GroupChunk { int group; int len; long long start; };      // entries [start, start + len) of perm, all of group `group`

struct GroupPlan {
  std::vector<int32_t> perm;            // [kept cells]
  std::vector<GroupChunk> chunks;
  std::vector<int64_t> first;           // [nslabs + 1] the chunks of a slab
  std::vector<int64_t> n_obs;           // [B] cells of every group
};

// labels [N] in [-1, B); slab [nslabs + 1] ascending from 0 to N.  0, or 1 with the first cell whose label is outside [-1, B) in *bad_cell.
inline int group_plan(const int32_t* labels, int64_t N, int32_t B, const int64_t* slab, int64_t nslabs, int chunk, GroupPlan& out, int64_t* bad_cell) {
  out.perm.clear(); out.chunks.clear();
  out.first.assign((size_t)nslabs + 1, 0);
  out.n_obs.assign((size_t)B, 0);
  for (int64_t i = 0; i < N; i++) {
    if (labels[i] < -1 || labels[i] >= B) { *bad_cell = i; return 1; }
    if (labels[i] >= 0) out.n_obs[(size_t)labels[i]]++;
  }
  std::vector<int64_t> seg((size_t)B + 1, 0);      // group b's part of perm: [seg[b], seg[b + 1])
  for (int32_t b = 0; b < B; b++) seg[(size_t)b + 1] = seg[(size_t)b] + out.n_obs[(size_t)b];
  out.perm.resize((size_t)seg[(size_t)B]);
  std::vector<int64_t> at(seg.begin(), seg.end() - 1);
  for (int64_t i = 0; i < N; i++)
    if (labels[i] >= 0) out.perm[(size_t)at[(size_t)labels[i]]++] = (int32_t)i;
  // cells ascend within a group: a slab takes the next run of every group
  std::vector<int64_t> done(seg.begin(), seg.end() - 1);
  chunk = std::max(chunk, 1);
  for (int64_t s = 0; s < nslabs; s++) {
    out.first[(size_t)s] = (int64_t)out.chunks.size();
    for (int32_t b = 0; b < B; b++) {
      int64_t lo = done[(size_t)b], hi = lo;
      while (hi < seg[(size_t)b + 1] && out.perm[(size_t)hi] < slab[s + 1]) hi++;
      done[(size_t)b] = hi;
      for (; lo < hi; lo += chunk) out.chunks.push_back({(int)b, (int)std::min<int64_t>(chunk, hi - lo), (long long)lo});
    }
  }
  out.first[(size_t)nslabs] = (int64_t)out.chunks.size();
  return 0;
}

}  // namespace hmx
