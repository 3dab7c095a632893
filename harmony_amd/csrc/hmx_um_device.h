// hmx_um_device.h -- the device helpers hmx_umap.hip and hmx_umap_transform.hip share: the hash of the negative samples, the load of a position,
// the clip and the fp32 expression of one term.  One definition, so that the layout and the projection of query cells into it round alike.
#pragma once
#include "hmx_internal.h"

namespace hmx {

__device__ __forceinline__ unsigned um_fmix32(unsigned x) {
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}
template <int DIM>
__device__ __forceinline__ void um_load(const float* Y, long long i, float& x, float& y, float& z) {
  if (DIM == 2) { const float2 p = *reinterpret_cast<const float2*>(Y + 2 * i); x = p.x; y = p.y; z = 0.0f; }
  else { x = Y[3 * i]; y = Y[3 * i + 1]; z = Y[3 * i + 2]; }
}
__device__ __forceinline__ float um_clip(float v) { return fminf(fmaxf(v, -4.0f), 4.0f); }
// one term of the sum from the difference y_i - y_other: the attraction clip(c_a d) -- twice it where TWICE, the layout's form, in which the
// mirror entry pushes the cell by the same amount -- or the repulsion clip(c_r d); d2^b = exp2(b log2 d2).  P: the stage's argument struct
// with the floats a, b, m2ab = float(-2ab), g2b = float(2 gamma b).
template <int DIM, bool ATTRACT, bool TWICE = true, class P>
__device__ __forceinline__ void um_term(const P& D, float dx, float dy, float dz, float& ax, float& ay, float& az) {
  float d2 = dx * dx + dy * dy;
  if (DIM == 3) d2 += dz * dz;
  if (!(d2 > 0.0f)) return;
  const float pw = exp2f(D.b * log2f(d2));
  const float den = D.a * pw + 1.0f;
  const float c = ATTRACT ? (D.m2ab * pw) / (d2 * den) : D.g2b / ((0.001f + d2) * den);
  const float f = ATTRACT && TWICE ? 2.0f : 1.0f;
  ax += f * um_clip(c * dx);
  ay += f * um_clip(c * dy);
  if (DIM == 3) az += f * um_clip(c * dz);
}

}  // namespace hmx
