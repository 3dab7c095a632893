// Host-side probe of the work list of the grouped gene statistics (harmony_amd/csrc/hmx_group_plan.h, HIP-free): built by
// tests/test_group_stats_cpu.py with the host compiler and called through ctypes.
#include "../../harmony_amd/csrc/hmx_group_plan.h"

// -> the number of chunks (or -1 - the first cell whose label is out of range).  perm [N], n_obs [B], first [nslabs + 1] and up to `room` chunks as
// (group, len, start) triples are written; *kept = the entries of perm.
extern "C" long long probe_group_plan(const int32_t* labels, long long N, int B, const long long* slab, long long nslabs, int chunk, int32_t* perm,
                                      long long* kept, long long* n_obs, long long* first, long long* chunks, long long room) {
  hmx::GroupPlan p;
  int64_t bad = 0;
  std::vector<int64_t> s(slab, slab + nslabs + 1);
  if (hmx::group_plan(labels, N, B, s.data(), nslabs, chunk, p, &bad)) return -1 - (long long)bad;
  *kept = (long long)p.perm.size();
  for (size_t i = 0; i < p.perm.size(); i++) perm[i] = p.perm[i];
  for (int b = 0; b < B; b++) n_obs[b] = p.n_obs[(size_t)b];
  for (long long t = 0; t <= nslabs; t++) first[t] = p.first[(size_t)t];
  for (size_t c = 0; c < p.chunks.size() && (long long)c < room; c++) {
    chunks[3 * c] = p.chunks[c].group; chunks[3 * c + 1] = p.chunks[c].len; chunks[3 * c + 2] = p.chunks[c].start;
  }
  return (long long)p.chunks.size();
}
