// hmx_silhouette.hip -- gfx950 kernels of the silhouette widths (include/harmony_mi355x_silhouette.h; DESIGN "Silhouette widths").
//
// The cells are sorted by (group, label) on the host and every (group, label) segment is padded to a multiple of 16 rows, so that each
// 16-column MFMA tile of a data slab carries ONE group and ONE label (SilTile, wave-uniform), and so do the 16 query rows of a wave.
//
//   k_sil_gather      fp32 rows / squared norms in the given order (k_knn_ingest) -> the sorted, padded layout (pads 0);
//   k_silhouette<MG>  workgroup = 64 query rows of the sorted order (16 per wave, A operand in registers); it streams the data rows of the
//                     groups its rows belong to in 64-row slabs through LDS, on the distance tile it shares with k_knn
//                     (hmx_dist_tile.h): d2 = |q|^2 + |x|^2 - 2 q.x with the dot product on v_mfma_f32_16x16x4_f32,
//                     dist = sqrt(max(d2, 0)), padding rows and self (by index) masked to 0.
//                     A lane adds the distances of (its 4 query rows, its data column) in fp32 over at most SIL_FLUSH tiles; the 16
//                     lanes that share a query row then reduce (4 more additions) into an fp64 segment sum.  At a segment's end the mean
//                     is folded: a (own label, divisor count - 1) or a candidate of b = min (another label of the group).  O(1) state
//                     per row, no atomics: the order of every addition is fixed by the layout -- bit-reproducible.
#include "hmx_dist_tile.h"

namespace hmx {
typedef int i32x4 __attribute__((ext_vector_type(4)));      // a SilTile in registers: x group, y label, z rows | last << 8, w count

// v + the value of lane (lane ^ ...) / rotated within its row of 16 lanes: DPP, no LDS
template <int CTRL>
__device__ __forceinline__ float sil_dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// the sum over the 16 lanes of a row, in every one of them
__device__ __forceinline__ float sil_row_sum(float v) {
  v = sil_dpp_add<0x128>(v);                          // row_ror:8
  v = sil_dpp_add<0x124>(v);                          // row_ror:4
  v = sil_dpp_add<0x4e>(v);                           // quad_perm:[2,3,0,1]
  return sil_dpp_add<0xb1>(v);                        // quad_perm:[1,0,3,2]
}

// one thread per float4 of a sorted row
__global__ __launch_bounds__(256) void k_sil_gather(const float* __restrict__ rows, const float* __restrict__ nrm, const int* __restrict__ src,
                                                    long long Np, int zs, float* __restrict__ dst, float* __restrict__ dnrm) {
  const int nf4 = zs >> 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long r = i / nf4;
  const int col = (int)(i - r * nf4);
  if (r >= Np) return;
  const int o = src[r];
  *(f32x4*)(dst + (size_t)r * zs + 4 * col) = o >= 0 ? *(const f32x4*)(rows + (size_t)o * zs + 4 * col) : f32x4{0.f, 0.f, 0.f, 0.f};
  if (col == 0) dnrm[r] = o >= 0 ? nrm[o] : 0.f;
}

// MG: PC groups of 16 the kernel is built for (P.NG <= MG of them are run)
template <int MG>
__global__ __launch_bounds__(256) void k_silhouette(SilDev P) {
  typedef DistTile<MG> Tile;                          // hmx_dist_tile.h: the A operand, the slab staging and the MFMA loop
  __shared__ __attribute__((aligned(16))) float slab[KNN_SLAB][Tile::S];
  __shared__ float sxn[KNN_SLAB];
  __shared__ i32x4 stile[KNN_SLAB / 16];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, g = l >> 4;
  const long long ntiles = P.Np >> 4;
  const long long qt0 = (long long)blockIdx.x * (KNN_QROWS / 16), qt = qt0 + w, q0 = 16 * qt;
  const bool have = qt < ntiles;                      // (the last workgroup may hold fewer than four query tiles)
  const i32x4* tiles = (const i32x4*)P.tile;
  const i32x4 none{-1, -1, 0, 0};
  const i32x4 mine = have ? tiles[qt] : none;         // the wave's own (group, label): one per 16 query rows
  const int own_group = __builtin_amdgcn_readfirstlane(have ? mine.x : -2);      // (-2: never the group of a data tile)
  const int own_label = __builtin_amdgcn_readfirstlane(mine.y), own_count = __builtin_amdgcn_readfirstlane(mine.w);
  // data rows: from the first tile of the group of the first query tile to the last tile of the group of the last one
  const long long c0 = 16ll * P.grange[2 * tiles[qt0].x], c1 = 16ll * P.grange[2 * tiles[min(qt0 + KNN_QROWS / 16, ntiles) - 1].x + 1];
  const int zs = P.zs, NG = P.NG;

  Tile DT;
  DT.init(have ? P.X + (size_t)(q0 + c) * zs : nullptr, zs, NG, slab);
  float qn[4], part[4];                               // the lane's rows of the result tile: query rows q0 + 4 g + i
  double seg[4], av[4], bv[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    qn[i] = have ? P.xn[q0 + 4 * g + i] : 0.f;
    part[i] = 0.f;
    seg[i] = av[i] = 0.0;
    bv[i] = INFINITY;
  }
  int nacc = 0;                                       // tiles added into part[] since the last reduction (wave-uniform)

  i32x4 pretile = none;                               // the slab's four SilTiles travel with it: fetched and staged next to the rows
  auto fetch = [&](long long base) {
    DT.fetch(P.X, P.xn, base, c1, zs);
    if (tid < KNN_SLAB / 16) pretile = base + 16 * tid < c1 ? tiles[(base >> 4) + tid] : none;
  };
  fetch(c0);
  for (long long base = c0; base < c1; base += KNN_SLAB) {
    __syncthreads();                                  // the previous slab has been read by every wave
    DT.stage(slab, sxn, zs);
    if (tid < KNN_SLAB / 16) stile[tid] = pretile;
    __syncthreads();
    if (base + KNN_SLAB < c1) fetch(base + KNN_SLAB);

    f32x4 acc[4];                                     // acc[tt][i] = q . x of (query row q0 + 4 g + i, data row base + 16 tt + c)
    DT.dots(slab, NG, acc);
#pragma unroll
    for (int tt = 0; tt < 4; tt++) {
      const i32x4 T = stile[tt];
      if (__builtin_amdgcn_readfirstlane(T.x) != own_group) continue;      // another group, or behind the last row: wave-uniform
      const int tlabel = __builtin_amdgcn_readfirstlane(T.y), trows = __builtin_amdgcn_readfirstlane(T.z), tcount = __builtin_amdgcn_readfirstlane(T.w);
      const long long x = base + 16 * tt + c;
      const float xn = sxn[16 * tt + c];
      const bool pad = c >= (trows & 0xff);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float d2 = fmaf(-2.0f, acc[tt][i], qn[i] + xn);
        const float dist = __builtin_amdgcn_sqrtf(fmaxf(d2, 0.f));
        part[i] += (pad || x == q0 + 4 * g + i) ? 0.f : dist;
      }
      nacc++;
      const bool last = (trows >> 8) != 0;
      if (!last && nacc < SIL_FLUSH) continue;
      nacc = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        seg[i] += (double)sil_row_sum(part[i]);         // the 16 lanes of a query row
        part[i] = 0.f;
      }
      if (!last) continue;
      const bool same = tlabel == own_label;          // (the only cell of its label: its sum is 0, self being masked)
      const double cells = (double)(same ? max(tcount - 1, 1) : tcount);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const double mean = seg[i] / cells;
        if (same) av[i] = mean;
        else bv[i] = fmin(bv[i], mean);
        seg[i] = 0.0;
      }
    }
  }
  if (!have || c != 0) return;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int o = P.src[q0 + 4 * g + i];
    if (o < 0) continue;
    double s, aa = av[i], bb = bv[i];
    if (isinf(bb)) s = aa = bb = NAN;                 // fewer than two labels in the group
    else if (own_count == 1) s = 0.0;
    else { const double m = fmax(aa, bb); s = m > 0.0 ? (bb - aa) / m : 0.0; }
    P.s[o] = s; P.a[o] = aa; P.b[o] = bb;
  }
}

void l_sil_gather(const Launch& L, const float* rows, const float* nrm, const int* src, long long Np, int zs, float* dst, float* dnrm) {
  const long long n = Np * (zs >> 2);
  hipLaunchKernelGGL(k_sil_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L.stream, rows, nrm, src, Np, zs, dst, dnrm);
}
void l_silhouette(const Launch& L, const SilDev& P) {
  const dim3 grid((unsigned)(((P.Np >> 4) + KNN_QROWS / 16 - 1) / (KNN_QROWS / 16)));
  if (P.NG <= 2) hipLaunchKernelGGL(k_silhouette<2>, grid, dim3(256), 0, L.stream, P);
  else if (P.NG <= 4) hipLaunchKernelGGL(k_silhouette<4>, grid, dim3(256), 0, L.stream, P);
  else hipLaunchKernelGGL(k_silhouette<8>, grid, dim3(256), 0, L.stream, P);
}

}  // namespace hmx
