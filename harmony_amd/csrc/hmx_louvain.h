// hmx_louvain.h -- what hmx_louvain.hip (the kernels) and hmx_api_louvain.inc (the host's orchestration) share: the constants, the argument
// structs and the launchers of the Louvain clustering (include/harmony_mi355x_louvain.h; DESIGN "Louvain clustering").  The pattern's checks, the
// scans and the segment sort are the graph stage's (hmx_graph.h).
#pragma once
#include "hmx_graph.h"

namespace hmx {

constexpr int LV_SHORT_CAP = 1024;         // entries of a row one wave groups by community in LDS (a bitonic sort of 64-bit keys): longer rows take the long path
constexpr int LV_WINDOW = 2048;            // community ids of the long path's window: one 64-bit LDS counter each
constexpr int LV_LONG_WGS = 512;           // workgroups that share the long rows
constexpr int LV_SUBROUNDS = 8;            // sub-rounds of a sweep
constexpr int LV_FLAG_WEIGHT = 1, LV_FLAG_MIRROR = 2;      // a weight outside [0, 1] or not finite; an edge whose mirror carries other bits
constexpr double LV_SCALE = 16777216.0;    // q = llrint(w * 2^24)

struct LvIn {                              // the caller's graph: checks and integer weights
  long long N; const long long* indptr; const int* indices; const float* weights;
  long long* q; long long* k; int* flag;
};
struct LvDev {                             // one level's local moves
  long long n; const long long* indptr; const int* indices; const long long* q; const long long* k;
  int* comm; long long* tot; int* target;
  double g; unsigned key; int bucket, short_cap;      // key: fmix32(64 t + level + 1) of the sweep
  int* longrows; unsigned* nlong; unsigned* moved;
};
struct LvAgg {                             // one level's aggregation
  long long n, C; const long long* indptr; const int* indices; const long long* q; const long long* k; const long long* in;      // in: nullptr at level 0
  const int* comm; unsigned* mark; const long long* newid;                    // newid [n + 1]: the scan of mark
  unsigned* ecount; const long long* soff; unsigned* cursor; unsigned long long* keys;      // the communities' segments of keys c' << 32 | entry
  unsigned* len; const long long* cindptr; int* cindices; long long* cq; long long* ck; long long* cin;      // the coarse graph
  int* lab; long long cells;
};
void l_lv_check(const Launch& L, const LvIn& I);
void l_lv_quantise(const Launch& L, const LvIn& I);
void l_lv_init(const Launch& L, const LvDev& D);                 // comm[i] = i, tot[i] = k[i], the rows above short_cap listed
void l_lv_decide(const Launch& L, const LvDev& D, bool with_long);
void l_lv_apply(const Launch& L, const LvDev& D);
void l_lv_mark(const Launch& L, const LvAgg& A);
void l_lv_count(const Launch& L, const LvAgg& A);
void l_lv_place(const Launch& L, const LvAgg& A);
void l_lv_reduce(const Launch& L, const LvAgg& A, bool write);
void l_lv_compose(const Launch& L, const LvAgg& A, bool first);  // first: lab[cell] = newid[comm[cell]]

}  // namespace hmx
