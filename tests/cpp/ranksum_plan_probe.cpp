// Host-side probe of the plan of the rank-sum call (harmony_amd/csrc/hmx_ranksum_plan.h, HIP-free): built by tests/test_rank_sums_cpu.py with the
// host compiler and called through ctypes.
#include "../../harmony_amd/csrc/hmx_ranksum_plan.h"

// -> the number of gene blocks (or -1 - the first gene whose count is negative).  seg [G + 1], block and first [up to G + 1 each], path [G], order
// [up to G] are written; *norder = the entries of order, *max_entries = the largest block's entries.
extern "C" long long probe_ranksum_plan(const long long* count, int G, long long budget, long long sort_lds, long long* seg, int* block, unsigned char* path,
                                        int* order, long long* first, long long* norder, long long* max_entries) {
  hmx::RankSumPlan p;
  int32_t bad = 0;
  std::vector<int64_t> c(count, count + G);
  if (hmx::ranksum_plan(c.data(), G, budget, sort_lds, p, &bad)) return -1 - (long long)bad;
  for (size_t j = 0; j < p.seg.size(); j++) seg[j] = p.seg[j];
  for (size_t k = 0; k < p.block.size(); k++) block[k] = p.block[k];
  for (size_t k = 0; k < p.first.size(); k++) first[k] = p.first[k];
  for (size_t j = 0; j < p.path.size(); j++) path[j] = p.path[j];
  for (size_t j = 0; j < p.order.size(); j++) order[j] = p.order[j];
  *norder = (long long)p.order.size();
  *max_entries = p.max_entries;
  return (long long)p.block.size() - 1;
}
