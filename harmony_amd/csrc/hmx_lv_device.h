// hmx_lv_device.h -- the device helpers hmx_louvain.hip and hmx_leiden.hip share: the hash of the sub-rounds, the three-operation score and the
// order of the candidates.  One definition, so that the two stages round and break ties alike.
#pragma once
#include "hmx_louvain.h"

namespace hmx {
typedef unsigned long long u64;

__device__ __forceinline__ unsigned lv_fmix32(unsigned x) {
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ int lv_bucket(long long i, unsigned key) { return (int)(lv_fmix32((unsigned)i ^ key) & (LV_SUBROUNDS - 1)); }
// dbl(w) - kg * dbl(t): three correctly rounded operations, never fused.  (__dmul_rn is a plain product to the compiler, which contracts it
// with the difference into one fma under the default -ffp-contract=fast; the empty asm makes the rounded product a value of its own.)
__device__ __forceinline__ double lv_score(long long w, double kg, long long t) {
#pragma clang fp contract(off)
  double p = __dmul_rn(kg, __ll2double_rn(t));
  asm volatile("" : "+v"(p));
  return __dsub_rn(__ll2double_rn(w), p);
}
__device__ __forceinline__ double lv_kg(long long k, double g) {
#pragma clang fp contract(off)
  return __dmul_rn(__ll2double_rn(k), g);
}
// a candidate (s, c) against the best so far: the larger score, ties to the smaller community
__device__ __forceinline__ void lv_better(bool& has, double& bs, int& bc, bool h, double s, int c) {
  if (h && (!has || s > bs || (s == bs && c < bc))) { has = true; bs = s; bc = c; }
}

}  // namespace hmx
