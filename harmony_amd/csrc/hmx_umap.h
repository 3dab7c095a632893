// hmx_umap.h -- what hmx_umap.hip (the kernels) and hmx_api_umap.inc (the host's orchestration) share: the constants, the argument struct and
// the launchers of the UMAP layout (include/harmony_mi355x_umap.h; DESIGN "The UMAP layout").  The pattern's and the weights' checks are the
// graph stage's and Louvain's (hmx_graph.h, hmx_louvain.h).
#pragma once
#include "hmx_louvain.h"

namespace hmx {

constexpr int UM_SHORT_CAP = 1024;         // entries of a row one wave walks (16 per lane): longer rows take one workgroup each
constexpr int UM_LONG_WGS = 512;           // workgroups that share the long rows
constexpr int UM_MAX_NEG = 31;             // negative samples per firing: key(n, s) leaves s five bits
constexpr int UM_MAX_EPOCHS = 1 << 20;

struct UmDev {
  long long N; const long long* indptr; const int* indices; const float* weights;
  const float* yold; float* ynew;                      // [N][dim] the epoch's snapshot and its result
  unsigned* wbits;                                     // the bits of the largest off-diagonal weight (k_um_wmax)
  double wmax; int n;                                  // ... as the epochs read it; the epoch
  float alpha, a, b, m2ab, g2b;                        // float(learning_rate (1 - n / n_epochs)), float(a), float(b), float(-2ab), float(2 gamma b)
  unsigned kbase; int nneg;                            // fmix32(seed) + 32 n + 1: key(n, s) = fmix32(kbase + s); negative samples per firing
  int short_cap; int* longrows; unsigned* nlong;       // the rows above short_cap, listed once per call
  unsigned long long* fired; unsigned long long* total;      // [N] firings per row, added up by every epoch; their sum
};
void l_um_wmax(const Launch& L, const UmDev& D);       // wbits, the long rows listed, fired zeroed
void l_um_epoch(const Launch& L, const UmDev& D, int dim, bool with_long);
void l_um_fired(const Launch& L, const UmDev& D);      // total[0] += the sum of fired

}  // namespace hmx
