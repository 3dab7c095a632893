// hmx_graph.h -- what hmx_graph.hip (the kernels) and hmx_api_graph.inc (the host's orchestration) share: the constants, the argument struct and
// the launchers of the neighbour graph and its connected components (include/harmony_mi355x_graph.h; DESIGN "The neighbour graph"), and of
// Seurat's SNN graph over the same transposed lists (hmx_api_snn.inc; include/harmony_mi355x_snn.h; DESIGN "Seurat's SNN graph").
#pragma once
#include "hmx_internal.h"

namespace hmx {

constexpr int GR_WAVE_KEYS = 128;          // keys a wave sorts in registers (two per lane): a transposed row up to this length takes the fast path
constexpr int GR_SCAN_CHUNK = 2048;        // counts a workgroup of the scan handles (256 threads, 8 each)
constexpr int GR_SUM_PARTS = 1024;         // at most this many workgroup partials of the distance sum
constexpr int GR_LONG_WGS = 64;            // workgroups that share the long transposed rows
constexpr int GR_CC_HOPS = 16;             // parents a cell follows per pointer-jumping launch
constexpr int GR_CC_ROUNDS = 64;           // hook-and-jump rounds before the call gives up

constexpr int GR_FLAG_DUP = 1;             // a row lists a cell twice
constexpr int GR_FLAG_RANGE = 1, GR_FLAG_ORDER = 2, GR_FLAG_ASYM = 4;      // components: an index outside [0, N), a row not strictly ascending, an edge without its mirror
constexpr int GR_FLAG_CHANGED = 1, GR_FLAG_DEEP = 2;                       // components: a hook lowered an entry; a tree was not flat after the round's jumps

struct GraphDev {
  const int* idx; const float* dist; long long N; int m;      // the neighbour lists [N][m], self excluded; idx -1: an unfilled slot
  int nparts; double* part; double* total;                    // the distance sum: workgroup partials [nparts], then total[0]
  double* rho; double* sigma; double* w;                      // [N], [N], [N][m] memberships of the directed edges
  unsigned* deg;                                              // [N] in-degree; the placement counts it down again
  long long* toff;                                            // [N + 1] the transposed rows' offsets
  unsigned long long* tkey; unsigned long long* tother;       // the transposed lists: source * m + slot, sorted per row; the long rows' second buffer
  int* longrows; unsigned* nlong;                             // the rows of more than GR_WAVE_KEYS entries
  unsigned* len; const long long* indptr; int* indices; float* weights;      // the union: row lengths, then (indptr scanned) the CSR
  int* flag;
};
long long graph_sum_parts(long long count);
void l_graph_distsum(const Launch& L, const GraphDev& G);
void l_graph_smooth(const Launch& L, const GraphDev& G);
// exclusive scan of n 32-bit counts into 64-bit offsets off[0 .. n] (off[n]: the total); bsum: ceil(n / GR_SCAN_CHUNK) + 1 words of work space
void l_graph_scan(const Launch& L, const unsigned* cnt, long long n, long long* off, long long* bsum);
void l_graph_place(const Launch& L, const GraphDev& G);
void l_graph_sort(const Launch& L, const GraphDev& G);
void l_graph_union(const Launch& L, const GraphDev& G, bool write);

// ---- Seurat's shared-nearest-neighbour graph (include/harmony_mi355x_snn.h; DESIGN "Seurat's SNN graph") ---------------------------------------------
constexpr int SNN_SHORT_CAP = 2048;        // candidates (with multiplicity) one wave sorts in LDS: a row up to this count takes the short path
constexpr int SNN_WINDOW = 8192;           // cells of the long path's dense window: one 8-bit counter each, four to an LDS word
constexpr int SNN_LONG_WGS = 1024;         // workgroups that share the long rows
constexpr int SNN_MAX_K = 129;             // the cell itself and at most 128 neighbours

struct SnnDev {
  const int* idx; long long N; int m;                         // the neighbour lists [N][m], self excluded; the sets N+(i) add the cell itself
  const long long* toff; const unsigned long long* tkey;      // the transposed lists of hmx_graph.hip: offsets [N + 1], source * m + slot ascending per row
  int s_min; const float* jtab;                               // an entry is kept iff its shared count s >= s_min; jtab [m + 2]: the weight of s
  unsigned* cand;                                             // [N] candidates with multiplicity C_i (saturated at 2^32 - 1)
  int* longrows; unsigned* nlong;                             // the rows with C_i > SNN_SHORT_CAP
  unsigned* len; const long long* indptr; int* indices; float* weights;      // row lengths, then (indptr scanned) the CSR
};
void l_snn_indegree(const Launch& L, const GraphDev& G);      // deg[j] += 1 per valid slot (what k_smooth_knn counts beside its search)
void l_snn_rowweight(const Launch& L, const SnnDev& S);
void l_snn_short(const Launch& L, const SnnDev& S, bool write);
void l_snn_long(const Launch& L, const SnnDev& S, bool write);

struct CcDev {
  long long N; const long long* indptr; const int* indices; const int* labels;      // a symmetric CSR pattern, rows ascending; labels [N] or nullptr
  int* comp; int* flag;
};
void l_cc_check(const Launch& L, const CcDev& C);
void l_cc_init(const Launch& L, const CcDev& C);
void l_cc_hook(const Launch& L, const CcDev& C);
void l_cc_jump(const Launch& L, const CcDev& C, bool check);

}  // namespace hmx
