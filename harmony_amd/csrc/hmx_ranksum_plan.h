// hmx_ranksum_plan.h -- the plan of the rank-sum call (hmx_rank_sums; kernels in hmx_ranksum.hip): from the number of positive entries of every
// selected gene, where each gene's list lies, which genes share a fill sweep, how each gene is sorted and in which order the genes are handed out.
// A pure function of (counts, the byte budget, the LDS sort's capacity).  Plain C++17 like hmx_group_plan.h: no HIP, no handle
// (tests/cpp/ranksum_plan_probe.cpp drives it on the CPU; hmx_api_ranksum.inc uploads what it returns).
//
// seg    [G + 1] gene j's entries are [seg[j], seg[j + 1]) of the gene-major list of ALL selected genes (a block's buffer starts at seg[block[k]]).
// block  [nblocks + 1] block k holds the genes (output rows) [block[k], block[k + 1]): a contiguous run, taken greedily while the run's lists and
//        the sort's second buffer (RANKSUM_ENTRY_BYTES per entry together) fit the budget.  A block always holds at least one gene, so a gene
//        that exceeds the budget on its own gets a block of its own; genes without entries cost nothing and join the block in reach.
// path   [G] RANKSUM_NONE (no entry: nothing runs), RANKSUM_LDS (<= sort_lds entries: sorted in LDS), RANKSUM_RADIX (sorted between the two buffers).
// order  the genes WITH entries, block by block ([first[k], first[k + 1]) are block k's), within a block the longest list first, ties by gene.
// The plan depends on nothing but its arguments: never on a grid, a device or the matrix's values.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cstddef>
#include <vector>

namespace hmx {

constexpr int64_t RANKSUM_ENTRY_BYTES = 16;      // an entry of the list (a 64-bit word) and its place in the sort's second buffer
enum { RANKSUM_NONE = 0, RANKSUM_LDS = 1, RANKSUM_RADIX = 2 };

struct RankSumPlan {
  std::vector<int64_t> seg;
  std::vector<int32_t> block;
  std::vector<uint8_t> path;
  std::vector<int32_t> order;
  std::vector<int64_t> first;
  int64_t max_entries = 0;      // of a block: the size of the two buffers
};

// count [G] >= 0.  0, or 1 with the first gene whose count is negative in *bad_gene.
inline int ranksum_plan(const int64_t* count, int32_t G, int64_t budget_bytes, int64_t sort_lds, RankSumPlan& out, int32_t* bad_gene) {
  out.seg.assign((size_t)G + 1, 0);
  out.block.assign(1, 0);
  out.path.assign((size_t)G, RANKSUM_NONE);
  out.order.clear();
  out.first.assign(1, 0);
  out.max_entries = 0;
  for (int32_t j = 0; j < G; j++) {
    if (count[j] < 0) { *bad_gene = j; return 1; }
    out.seg[(size_t)j + 1] = out.seg[(size_t)j] + count[j];
    out.path[(size_t)j] = (uint8_t)(count[j] == 0 ? RANKSUM_NONE : count[j] <= sort_lds ? RANKSUM_LDS : RANKSUM_RADIX);
  }
  const int64_t cap = std::max<int64_t>(budget_bytes, 0) / RANKSUM_ENTRY_BYTES;      // entries of a block
  for (int32_t j = 0; j < G;) {
    int32_t e = j + 1;
    while (e < G && out.seg[(size_t)e + 1] - out.seg[(size_t)j] <= cap) e++;
    out.block.push_back(e);
    out.max_entries = std::max(out.max_entries, out.seg[(size_t)e] - out.seg[(size_t)j]);
    const size_t at = out.order.size();
    for (int32_t g = j; g < e; g++) if (count[g] > 0) out.order.push_back(g);
    std::stable_sort(out.order.begin() + (std::ptrdiff_t)at, out.order.end(), [&](int32_t a, int32_t b) { return count[a] > count[b]; });
    out.first.push_back((int64_t)out.order.size());
    j = e;
  }
  return 0;
}

}  // namespace hmx
