// hmx_leiden.h -- what hmx_leiden.hip (the kernels) and hmx_api_leiden.inc (the host's orchestration) share: the argument structs and the
// launchers of the Leiden clustering (include/harmony_mi355x_leiden.h; DESIGN "Leiden clustering").  The constants, the checks, the
// quantisation and the aggregation are Louvain's (hmx_louvain.h); the pattern's checks, the scans and the segment sort the graph stage's.
#pragma once
#include "hmx_louvain.h"

namespace hmx {

struct LdKeep {                            // level 0: the caller's entries without the diagonal and without q == 0
  long long N; const long long* indptr; const int* indices; const long long* q;
  unsigned* cnt; const long long* kptr; int* kindices; long long* kq;      // kptr [N + 1]: the scan of cnt
};
struct LdDev {                             // one level: local moves from the partition comm, then the refinement inside its communities
  long long n; const long long* indptr; const int* indices; const long long* q; const long long* k; const long long* in;      // in: nullptr at level 0
  int* comm; long long* tot; int* target;
  int* ref; long long* rtot; int* size; int* ok; long long* cut;      // the refined partition: ref, its degrees and sizes, node_ok, cut per refined id
  long long* cin; unsigned* mark;          // the level's sums per community id: inner weight, in use
  double g; unsigned key; int bucket, short_cap;      // key: of the sweep, fmix32(64 t + level + 1) or fmix32 of its complement
  int* longrows; unsigned* nlong; unsigned* moved; unsigned* blocked;
};
struct LdNext {                            // the next level's start: the new nodes of one community share the smallest new id among them
  long long n, C; const int* comm; const int* ref; const long long* newid; unsigned* pmin; int* next;      // pmin [n]: all ones on entry
};
void l_ld_keep(const Launch& L, const LdKeep& K, bool write);
void l_ld_iota(const Launch& L, const LdDev& D);                 // comm[i] = i
void l_ld_parent(const Launch& L, const LdNext& X);              // pmin per community of the level before, then next[new id] gathered
void l_ld_start(const Launch& L, const LdDev& D);                // tot from comm (zero on entry), the rows above short_cap listed
void l_ld_decide(const Launch& L, const LdDev& D, bool with_long);
void l_ld_apply(const Launch& L, const LdDev& D);
void l_ld_sums(const Launch& L, const LdDev& D);                 // cin, mark (zero on entry)
void l_ld_refine_setup(const Launch& L, const LdDev& D);
void l_ld_cut(const Launch& L, const LdDev& D);                  // cut (zero on entry)
void l_ld_refine_decide(const Launch& L, const LdDev& D, bool with_long);
void l_ld_refine_apply(const Launch& L, const LdDev& D);

}  // namespace hmx
