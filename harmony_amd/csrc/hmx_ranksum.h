// hmx_ranksum.h -- what hmx_ranksum.hip (the kernels) and hmx_api_ranksum.inc (the host's orchestration) share: the constants, the argument
// structs and the launchers of the rank-sum call (include/harmony_mi355x_ranksum.h; DESIGN "Rank sums per group").
#pragma once
#include "hmx_internal.h"

namespace hmx {

constexpr int RS_GENES = 32768;            // genes whose 32-bit table a workgroup of the count / fill sweep keeps in LDS (128 KB); grid.y sweeps the ranges
constexpr int RS_SORT_LDS = 8192;          // entries of a gene's list sorted in LDS (64 KB of 64-bit words); longer lists take the radix sort
constexpr int RS_CHUNK = 4096;             // entries a workgroup (16 waves, 4 entries per lane) handles at a time in the radix scatter and the two rank scans

struct RankSweepDev {
  ProjDev C;                               // the rows of this launch (U, inv_sd, cap, b, out unused); C.slot: [G_all] output row of a gene or -1, nullptr: the identity
  const int* labels;                       // [N] group of every cell of the WHOLE matrix (row C.row0 + i), -1: the row is not read
  int j0, j1;                              // the output rows this sweep takes: [j0, j1)
  unsigned long long* count;               // [G] count sweep: positive entries per output row (integer adds)
  const long long* seg; long long base;    // [G + 1] fill sweep: the genes' segments; the buffer's first entry is seg[j0] = base
  unsigned* cursor;                        // [G] fill sweep: entries of a segment handed out so far
  unsigned long long* list; long long entries;      // the block's buffer: key bits << 32 | group
};
void l_rank_sweep(const RankSweepDev& S, bool fill, hipStream_t stream);

struct RankSortDev {
  const long long* seg; long long base;    // as above
  unsigned long long* list; unsigned long long* other; long long entries;      // the block's buffer and the sort's second one
  const int* order; int ngenes;            // the block's genes with entries, longest first
  unsigned* next;                          // the draw counter (zero at launch)
  int B, G; long long Nk;                  // groups, output rows, kept cells
  unsigned long long* rank2; unsigned* npos;      // [B][G] doubled midrank sums of the positive entries (+ 2 z each), their number
  unsigned long long* tie3;                // [G][2] sum of t^3 over the tie blocks: low, high word
};
void l_rank_sort(const RankSortDev& R, hipStream_t stream);

}  // namespace hmx
