// hmx_umap_transform.h -- what hmx_umap_transform.hip (the kernels) and hmx_api_umap_transform.inc (the host's orchestration) share: the argument
// structs and the launchers of the projection of query cells into a fitted layout (include/harmony_mi355x_umap_transform.h; DESIGN "Query cells
// in a fitted layout").  The distance sum is the graph stage's (hmx_graph.h), the sum of the firing counters the layout's (hmx_umap.h).
#pragma once
#include "hmx_umap.h"

namespace hmx {

constexpr int UT_MAX_K = 128;              // entries of a list: two per lane of the wave that walks it
constexpr int UT_SMALL_K = 16;             // up to this many entries a cell takes 16 lanes (four cells to a wave), above it a whole wave

struct UqDev {
  const int* idx; const float* dist; long long Nq; int k;     // the lists [Nq][k] of reference cells, ascending by distance, no self column
  const double* total;                                        // total[0]: the sum of all distances (k_graph_distsum)
  float* w; double* sigma;                                    // [Nq][k] the weights, [Nq] the rows' scales
};
void l_ut_weights(const Launch& L, const UqDev& Q);

struct UtDev {
  long long Nq; int k; long long Nr;
  const int* idx; const float* w; const float* yref;          // the lists and their weights [Nq][k]; the reference's positions [Nr][dim]
  float* y0; float* y;                                        // [Nq][dim] the start (written by l_ut_init, or the caller's), the result
  const float* alpha;                                         // [n1 - n0] float(alpha0 (1 - n / n_epochs)) of the epochs run, formed on the host
  double wmax; int n0, n1;                                    // the largest weight of the call; the epochs [n0, n1)
  float a, b, m2ab, g2b;                                      // float(a), float(b), float(-2ab), float(2 gamma b)
  unsigned kbase0; int nneg;                                  // fmix32(seed) + 1: key(n, s) = fmix32(kbase0 + 32 n + s); negative samples per firing
  unsigned long long* fired;                                  // [Nq] firings per cell over the epochs run
};
void l_ut_init(const Launch& L, const UtDev& D, int dim);      // y0: the weighted mean of the listed positions
void l_ut_transform(const Launch& L, const UtDev& D, int dim); // y, fired: every epoch of every cell in one launch

}  // namespace hmx
