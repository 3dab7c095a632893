// hmx_plan.h -- the launch plan of a fit: which execution path hmx_setup chooses for a shape, as a pure function of the environment
// switches and the shape.  Plain C++17: no HIP, no handle (tests/cpp/plan_probe.cpp builds it with a host compiler; hmx_api_setup.inc
// copies the result into Dev / hmx_ctx, allocates and uploads).  Every measured threshold is a named constant here, once.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace hmx {

// ---- the environment switches hmx_setup reads (INTEGRATION.md "Environment switches"), parsed once ------------------------------------
struct Switches {
  int grid = 2048;                                       // HMX_GRID
  bool nrep_set = false; int nrep = 8;                   // HMX_NREP
  bool moe_v1 = false;                                   // HMX_MOE_IMPL=v1
  bool r_store_always = false;                           // HMX_R_STORE=1
  bool dot_f32 = false;                                  // HMX_DOT=f32
  int upd_threads = 512;                                 // HMX_UPD_THREADS=256
  bool usig_off = false;                                 // HMX_USIG=0
  int upd_wps = 4;                                       // HMX_UPD_WPS
  bool upd_maxblocks_set = false; int upd_maxblocks = 0;         // HMX_UPD_MAXBLOCKS
  bool static_maxblocks_set = false; int static_maxblocks = 0;   // HMX_STATIC_MAXBLOCKS
  int oldsum_stream = 1;                                 // HMX_OLDSUM_IMPL=gather|stream1 -> 0 | 2 (1: 16-byte stream, 2: dword stream)
  int upd_tpw = 1;                                       // HMX_UPD_TPW
  bool sold_carry_set = false, sold_carry = false;       // HMX_SOLD_CARRY=0|1
  int shuffle_inv = 1;                                   // HMX_SHUFFLE_INV: 0 counting sort always; 2 sort-free form on sharded runs too
  bool solve_host = false;                               // HMX_MOE_SOLVE=host
  bool solve_lds_off = false;                            // HMX_SOLVE_LDS=0: the device solve's systems in the global scratch
  bool fused_fold_off = false;                           // HMX_FUSED_FOLD=0
  int fold_impl = 0;                                     // HMX_FOLD_IMPL=split|merged -> 1 | 2: force the two-kernel fold + penalty / k_foldpen of the step loop (tests)
  int chain = -1, chain_pair = -1;                       // HMX_CHAIN / HMX_CHAIN_PAIR: 0 off | 1 forced | -1 (unset, anything else) by the thresholds
  bool chain_wgs_set = false; int chain_wgs = 0;         // HMX_CHAIN_WGS (tests: two ranks sharing one GPU)
  bool chain_max_tpw_set = false; double chain_max_tpw = 0;      // HMX_CHAIN_MAX_TPW (tests: move the threshold between two shards)
  bool chain_folders_set = false; int chain_folders = 0; // HMX_CHAIN_FOLDERS
};
inline Switches read_switches() {
  Switches s;
  const auto is = [](const char* e, const char* v) { return e && std::string(e) == v; };
  const auto tri = [&](const char* e) { return is(e, "0") ? 0 : is(e, "1") ? 1 : -1; };
  const char* e;
  if ((e = getenv("HMX_GRID"))) s.grid = atoi(e);
  if ((e = getenv("HMX_NREP"))) { s.nrep_set = true; s.nrep = atoi(e); }
  s.moe_v1 = is(getenv("HMX_MOE_IMPL"), "v1");
  if ((e = getenv("HMX_R_STORE"))) s.r_store_always = atoi(e) == 1;
  s.dot_f32 = is(getenv("HMX_DOT"), "f32");
  if ((e = getenv("HMX_UPD_THREADS"))) s.upd_threads = atoi(e) == 256 ? 256 : 512;
  if ((e = getenv("HMX_USIG"))) s.usig_off = atoi(e) == 0;
  if ((e = getenv("HMX_UPD_WPS"))) s.upd_wps = atoi(e);
  if ((e = getenv("HMX_UPD_MAXBLOCKS"))) { s.upd_maxblocks_set = true; s.upd_maxblocks = atoi(e); }
  if ((e = getenv("HMX_STATIC_MAXBLOCKS"))) { s.static_maxblocks_set = true; s.static_maxblocks = atoi(e); }
  e = getenv("HMX_OLDSUM_IMPL"); s.oldsum_stream = is(e, "gather") ? 0 : is(e, "stream1") ? 2 : 1;
  if ((e = getenv("HMX_UPD_TPW"))) s.upd_tpw = atoi(e);
  if ((e = getenv("HMX_SOLD_CARRY"))) { s.sold_carry_set = true; s.sold_carry = atoi(e) == 1; }
  if ((e = getenv("HMX_SHUFFLE_INV"))) s.shuffle_inv = atoi(e);
  s.solve_host = is(getenv("HMX_MOE_SOLVE"), "host");
  s.fused_fold_off = is(getenv("HMX_FUSED_FOLD"), "0");
  s.solve_lds_off = is(getenv("HMX_SOLVE_LDS"), "0");
  e = getenv("HMX_FOLD_IMPL"); s.fold_impl = is(e, "split") ? 1 : is(e, "merged") ? 2 : 0;
  s.chain = tri(getenv("HMX_CHAIN"));
  s.chain_pair = tri(getenv("HMX_CHAIN_PAIR"));
  if ((e = getenv("HMX_CHAIN_WGS"))) { s.chain_wgs_set = true; s.chain_wgs = atoi(e); }
  if ((e = getenv("HMX_CHAIN_MAX_TPW"))) { s.chain_max_tpw_set = true; s.chain_max_tpw = atof(e); }
  if ((e = getenv("HMX_CHAIN_FOLDERS"))) { s.chain_folders_set = true; s.chain_folders = atoi(e); }
  return s;
}

// ---- what the decisions depend on ----------------------------------------------------------------------------------------------------
struct Shape {
  int64_t N = 0, N_global = 0;                 // cells of this shard / of the whole run
  int d = 0, K = 0, B = 0, C = 0, Q = 0;       // PCs, clusters, levels, covariates, level combinations present
  int nb = 1; uint64_t cells_per_block = 1;    // blocks of a clustering round
  int world = 1; bool sharded = false;         // ranks; world > 1 || comm_force (the collectives are issued)
  int cus = 0;                                 // compute units of the device
  bool usig = true;                            // all clusters share one sigma
  int ridge_arith = 0, oe_arith = 0, obj_arith = 0, solve_arith = 0;
  int tun_wps = -1, tun_tpw = -1;              // hmx_set_int tunables (<= 0: not set)
  int grid = 2048;                             // workgroups of the streaming kernels
  int ntitems = 0;                             // static 16-cell tiles (every combination's cells in tiles of its own)
};

// ---- the measured thresholds ---------------------------------------------------------------------------------------------------------
// The chain pays off while a block step is latency-bound: a few 16-cell tiles per resident wave (1.5 at 1M cells).  Round 3 measured the per-step launches
// 6 % faster at 10M cells per GPU (15 tiles per wave) and drew the line at 6 tiles; re-measured in round 6 on the chain as it is now (K = 100, 20 batches, to
// convergence): 5M cells 37.5 -> 33.8 ms, 7.5M 52.5 -> 49.2, 10M 65.9 -> 61.7 ON the chain, 15M (23 tiles per wave) 97.4 / 98.0: the line is at 20 tiles.
constexpr double CHAIN_MAX_TILES_PER_WAVE = 20.0;
// wave-pair chain (measured at configs[4]'s shape: 8 tiles per pair and block -- 2.5M cells -- 94.2 -> 79.1 ms on the chain; 16 -- 5M cells, old contributions
// carried on both paths -- 137.8 / 139.0: the launch-per-step path from 12 on)
constexpr double PAIR_MAX_TILES_PER_PAIR = 12.0;
// Old contributions carried from round to round (update_R): tiles keyed by (block, combination, NEXT block) cost up to 16 padding slots per key -- worth it
// while the expected padding (8 per key) stays below 1/8 = 12 % of the cells.
// (round 4: with the R stores of carried rounds gone as well -- Dev::r_store -- the carry saves ~200 us per round at 1M cells where the persistent chain runs
//  (K <= 112): worth up to ~12 % of padding there; measured at 1.25M cells / 20 batches, 5.1 %: 15.5 -> 12.7 ms per run.  On the launch-per-step path
//  (configs[4] shape, 41 %: 63 -> 70 ms) the old bound, 4 %, stayed.  Round 6: 12 % of padding for K > 112 as well -- configs[4] at its full 5M cells
//  (8.2 %): 165.9 -> 140.5 ms per run (no pass over R for the old contributions: 21.8 ms, no R stores in 21 of 28 rounds); 2.5M cells (16 %): 95.3 / 94.0 ms,
//  break-even.)
constexpr int64_t CARRY_PAD_PER_KEY = 8, CARRY_CELLS_PER_PAD = 8;
constexpr size_t LDS_PER_CU = 160 * 1024;           // LDS of a compute unit: what the workgroups resident on it share
constexpr size_t LDS_BUDGET = 150 * 1024;           // what the workgroup(s) owning a CU ask for at most: its LDS less room for the kernels' static objects
constexpr size_t FOLD_LDS_BYTES = LDS_BUDGET, FOLD_LDS_SLACK = 64;       // LDS a tile kernel with the fold in its prologue (fused fold, both chains) may take, less its static words
// device ridge solve (k_moe_solve): index words + body (Cholesky panel or, where they fit beside the index words in SOLVE_RHS_LDS_BYTES, the d right-hand sides) within
// SOLVE_LDS_BYTES; the coupling masks of the Schur complement ride behind them while the whole stays within SOLVE_MASK_LDS_BYTES
constexpr size_t SOLVE_LDS_BYTES = 158 * 1024, SOLVE_RHS_LDS_BYTES = LDS_BUDGET, SOLVE_MASK_LDS_BYTES = 159 * 1024;
constexpr int64_t INT32_CELLS = 2147483000ll;       // positions of a padded block order are int32
// the launch-per-step path gives a wave a contiguous range of a block's tiles once it has several tiles per block
constexpr double CONTIG_MIN_TILES_PER_WAVE = 4.0;

struct Plan {
  const char* limit = nullptr;                 // the shape exceeds the envelope (HMX_ERR_LIMIT): which limit
  // tile geometry
  int KP = 0, zs = 0, NCT = 0, NQ = 0, NT4 = 0, tail = 0, NS = 0, NS2 = 0, wNQ = 0, wNT4 = 0, wtail = 0, wNS = 0;
  int moe_mfma = 0, dot_bf = 0, usig = 0, rvec = 0, pen_lds = 0;
  int upd_wps = 2, upd_threads = 512, upd_maxblocks = 256, upd_tpw = 1, static_maxblocks = 0, oldsum_stream = 1, need_lorder = 0;
  int nwmax = 0, objslots = 0;
  bool r_store_always = false;
  // a round's shuffle
  bool carry_ok = false; int qmask = 0, nkeys = 0, npad = 0; bool shuf_inv = false;
  // ridge correction
  bool solve_on_device = false; int st_KH = 0, st_halves = 1, st_dma = 0, st_cpw = 0, st_nwg = 0;
  // update_R: fold in the tile kernel's prologue, persistent block chain, wave-pair chain (chain_ok / fused_ok / chain_pair: this rank's
  // view until the ranks of a sharded run have agreed on the minimum)
  bool fused_ok = false, chain_ok = false; int chain_wgs = 0;
  int chain_pair = 0, KH = 0, chain_folders = 0, chain_kw = 0;
  int nrep = 1, upd_contig = 0;
};

inline double tiles_per_wave(const Shape& s) { return (double)s.N / std::max(s.nb, 1) / 16.0 / (8.0 * std::max(s.cus - 1, 1)); }
// ---- the LDS of a k_tile launch, term by term (every budget below and plan_tile_launch are sums of these) ---------------------------------
// centroid image of the fp32 build, [NQ][NS][64 lanes] float4, and of the split-bf16 build, [nct][NS2][3 parts][64 lanes][8 bf16]
inline size_t image_bytes_f32(int NQ, int NS) { return (size_t)NQ * NS * 1024; }
inline size_t image_bytes_bf(int nct, int NS2) { return (size_t)nct * NS2 * 3 * 1024; }
// fold tables behind the image: O' [B][K] int64 (`fold`: the launch folds in its prologue), the penalty table [B][K] fp32 and the combinations' levels [Q][C] (`pen`, or with
// the fold).  pad4: the launches round the penalty table up to four entries; the budget of fold_lds_fits was written without that rounding and keeps its value (<= 12 bytes apart).
inline size_t fold_table_bytes(int B, int K, int Q, int C, bool fold, bool pen, bool pad4) {
  const size_t bk = (size_t)(pad4 ? (B * K + 3) & ~3 : B * K);
  return (fold ? (size_t)B * K * 8 : 0) + ((pen || fold) ? (bk + (size_t)Q * C) * 4 : 0);
}
inline size_t lloyd_sum_bytes(int K, int d) { return ((size_t)K * d + K) * sizeof(long long); }      // Lloyd: int64 sums [K][d] and counts [K]
// wave-pair chain (MODE 6): workers [ both halves' images | qlev | exchange slots | [8 waves][4 tiles][16 nctp] log2 penalties ], folders [ O slice | cluster masses | this rank's deltas (sharded) ]
inline size_t pair_worker_bytes(int nctp, int NS2, int Q, int C) { return 2 * image_bytes_bf(nctp, NS2) + (size_t)((Q * C + 3) & ~3) * 4 + 4 * 2 * 2 * 16 * 8 + (size_t)8 * 4 * 16 * nctp * 4; }
inline size_t pair_folder_bytes(int B, int kw) { return ((size_t)2 * B * kw + kw) * 8; }
// centroid image + O / Snew / penalty tables + combination levels of a tile kernel that folds in its prologue
inline bool fold_lds_fits(const Plan& p, const Shape& s) { return image_bytes_f32(p.NQ, p.NS) + fold_table_bytes(s.B, s.K, s.Q, s.C, true, true, false) + FOLD_LDS_SLACK <= FOLD_LDS_BYTES; }
// Lloyd on the tile kernel: the fp32 image and the sum table fit a CU's LDS (else k_lloyd sums into memory)
inline bool lloyd_tile_fits(int NQ, int NS, int K, int d) { return image_bytes_f32(NQ, NS) + lloyd_sum_bytes(K, d) <= LDS_PER_CU; }

// ---- the LDS of a k_moe_solve launch, term by term (plan_shape's envelope and plan_ridge_launch are sums of these) ------------------------------
// index words in front of the fp64 space: row_of, keepl, okb [B] each, misc [4 + C], prow [B + 1], rounded up to an even count (the kernel's PAN_OFF).  envelope: the
// budget of solve_on_device was written as 4 B + 8 + C words without that rounding and keeps its value -- 8 or 12 bytes MORE than a launch takes, so every admitted
// shape's launch fits, and no shape flips: with either formula the last B admitted is 1122 (for every C <= 16), 1123 is 72 bytes and more over.
inline size_t solve_index_bytes(int B, int C, bool envelope) { return (envelope ? (size_t)4 * B + 8 + C : ((size_t)4 * B + 6 + C) & ~(size_t)1) * sizeof(int); }
inline size_t solve_panel_bytes(int B) { return ((size_t)B + 1) * 16 * sizeof(double); }                  // Cholesky panel: 16 columns of M = B + 1 rows
inline size_t solve_rhs_bytes(int B, int d) { return ((size_t)B + 1) * d * sizeof(double); }              // the d right-hand sides, during the substitution
inline size_t solve_mask_bytes(int B) { return ((size_t)B + 1) * (((size_t)B + 1 + 63) / 64) * 8; }       // coupling masks: one bit per (row, eliminated level)

// Stage 1: everything up to this rank's view of fused_ok / chain_ok.  (Sharded runs then agree on the minimum of both flags.)
inline Plan plan_shape(const Switches& sw, const Shape& s) {
  Plan p;
  const int K = s.K, d = s.d, B = s.B, C = s.C, Q = s.Q;
  p.KP = (K + 63) / 64 * 64;
  // (rows padded to whole 128-byte lines -- 208 -> 256 B at d = 50 -- were measured in round 4: the block step stayed where it was for 23 % more memory; the switch is gone)
  p.zs = (d + 3) / 4 * 4;
  { static const int sup[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 14, 16};     // (13: K = 200, BASELINE configs[4])
    const int need = (K + 15) / 16; p.NCT = 16; for (int v : sup) if (v >= need) { p.NCT = v; break; } }
  p.moe_mfma = (K % 4 == 0 && d <= 64 && K <= 256 && !sw.moe_v1) ? 1 : 0;   // K > 128: split statistics kernel
  p.wNT4 = K / 16; p.wtail = (K - 16 * p.wNT4) / 4; p.wNS = 4 * p.wNT4 + p.wtail; p.wNQ = ((d + 15) / 16 + 3) / 4;
  p.r_store_always = sw.r_store_always;
  p.nwmax = 4 * s.grid; p.objslots = std::min(s.nb, 64);
  p.rvec = (K % 4 == 0) ? 1 : 0;
  p.NQ = (p.NCT + 3) / 4; p.NT4 = p.zs / 16; p.tail = (p.zs - 16 * p.NT4) / 4; p.NS = 4 * p.NT4 + p.tail;
  p.pen_lds = ((size_t)B * K * 4 + (size_t)Q * C * 4 <= 24576) ? 1 : 0;
  // the static-tile launches (head, seeding race, Lloyd) stage this centroid image in LDS: across the envelope (d <= 128, K <= 256) it is at most
  // 4 quads x 32 PC steps x 1 KB = 128 KB, so they need no fallback (Lloyd's K x d sum table beside it may not fit: k_lloyd, hmx_api_kmeans.inc)
  if ((size_t)p.NQ * p.NS * 1024 > 128 * 1024) { p.limit = "centroid image exceeds 128 KB of LDS"; return p; }
  // split-bf16 form of the tile kernels' distance GEMM (hmx_tile_bf.hip): offered where its register form covers the shapes the fp32
  // register form covers (rows of <= 64 PCs in four 16-byte groups); each launch takes it when its LDS image fits (l_update & co)
  p.NS2 = (p.zs + 31) / 32;
  p.dot_bf = !sw.dot_f32 && (p.NT4 > 4 || p.NS2 <= 2) && p.NS2 <= 4;
  // uniform sigma (the reference's default): scalar-constant kernel variants; with K <= 64 they also fit the register
  // budget of 4 waves per SIMD (1024-thread workgroups) -- measured 16 % faster per launch than 2 waves at K = 64
  p.usig = (s.usig && !sw.usig_off) ? 1 : 0;
  p.upd_wps = ((s.tun_wps > 0 ? s.tun_wps : sw.upd_wps) == 4 && p.usig && p.NCT <= 4) ? 4 : 2;
  p.upd_threads = p.upd_wps == 4 ? 1024 : sw.upd_threads;
  p.upd_maxblocks = std::max(1, sw.upd_maxblocks_set ? sw.upd_maxblocks : (p.upd_threads >= 512 ? 256 : 512));
  // static-tile launches (head / Lloyd / seeding): one resident generation of 256-thread workgroups (2 per CU at the 2 waves
  // per SIMD the K > 64 kernels get) re-stages the centroid image once instead of four times: head 213 -> 200 us at 1M
  p.static_maxblocks = sw.static_maxblocks_set ? sw.static_maxblocks : (p.NCT >= 5 ? 512 : p.NCT >= 3 ? 768 : 1024);
  p.oldsum_stream = sw.oldsum_stream;
  p.need_lorder = (p.oldsum_stream == 0 || (size_t)s.nb * K * 8 > 64 * 1024) ? 1 : 0;
  p.upd_tpw = std::max(1, s.tun_tpw > 0 ? s.tun_tpw : sw.upd_tpw);
  { const bool fits = s.nb <= 63 && Q < (1 << 19) && s.N + (int64_t)s.nb * s.nb * Q * 16 <= INT32_CELLS;
    const bool pays = (int64_t)s.nb * s.nb * Q * CARRY_PAD_PER_KEY * CARRY_CELLS_PER_PAD <= s.N;
    p.carry_ok = fits && (sw.sold_carry_set ? sw.sold_carry : pays) && !s.oe_arith;      // (oe_arith: the tables follow the reference, nothing is carried)
    p.qmask = p.carry_ok ? 0x7FFFF : 0x7FFFFFFF; }
  p.nkeys = p.carry_ok ? s.nb * s.nb : s.nb;      // sort keys of a round
  if (s.N + (int64_t)p.nkeys * Q * 16 > INT32_CELLS) {
    p.limit = "padded block order (N + n_blocks * combinations * 16) exceeds the int32 index range of one shard"; return p; }
  p.npad = (int)(s.N + (int64_t)p.nkeys * Q * 16);
  // sort-free form of the batched shuffle (lpair packs the combination in 19 bits and the blocks in 6; posr the combination in 11)
  p.shuf_inv = sw.shuffle_inv != 0 && (s.world == 1 || sw.shuffle_inv == 2) && p.carry_ok &&      /* (without the carry every round needs D.blk: the counting sort has it for free) */
               s.nb < 64 && Q < 2048 && s.N_global < ((int64_t)1 << 31) &&
               ((size_t)s.nb * Q + (size_t)Q + 1) * sizeof(int) + 5 * 4096 <= 64 * 1024;
  p.solve_on_device = !sw.solve_host && solve_index_bytes(B, C, true) + solve_panel_bytes(B) <= SOLVE_LDS_BYTES;
  // deterministic statistics pass (k_moe_stats_q): static split of the 16-cell tiles over ~2 workgroups per CU
  // (round 6: K in (128, 256] -- configs[4]'s 200 -- as two halves of <= 8 cluster tiles each, by the same kernel: deterministic there too.  Every shape with
  //  moe_mfma takes it -- K % 4 == 0 and K <= 256 give NCT <= 8 or two such halves -- so st_dma == moe_mfma; the fp64-atomic kernel it replaced is gone)
  p.st_KH = ((K + 1) / 2 + 3) & ~3;
  p.st_halves = (p.NCT > 8 && K % 4 == 0 && (p.st_KH + 15) / 16 <= 8 && K - p.st_KH >= 4 && K - p.st_KH <= 16 * ((p.st_KH + 15) / 16)) ? 2 : 1;
  p.st_dma = (p.moe_mfma && (p.NCT <= 8 || p.st_halves == 2)) ? 1 : 0;
  if (p.st_dma) { p.st_cpw = std::max(16, (s.ntitems + 2 * 256 - 1) / (2 * 256)); p.st_nwg = (s.ntitems + p.st_cpw - 1) / p.st_cpw; }
  p.fused_ok = !sw.fused_fold_off && fold_lds_fits(p, s);
  // persistent block chain: one workgroup per CU must be resident at once (they synchronise inside the launch)
  p.chain_wgs = sw.chain_wgs_set ? std::max(8, std::min(s.cus, sw.chain_wgs)) : s.cus;
  const bool chain_pays = sw.chain == 1 || tiles_per_wave(s) <= (sw.chain_max_tpw_set ? sw.chain_max_tpw : CHAIN_MAX_TILES_PER_WAVE);
  p.chain_ok = sw.chain != 0 && chain_pays && p.fused_ok && s.cus >= 8 && p.NCT <= 7 && p.NT4 <= 4 && s.nb <= 64 && fold_lds_fits(p, s);
  return p;
}

// Stage 2, on the agreed chain_ok: this rank's view of the wave-pair chain (k_tile MODE 6) for 112 < K <= 224 -- BASELINE configs[4]: K = 200 -- where no single
// wave holds a row's clusters and no LDS holds the K x B table: two halves of the clusters on the two waves of a SIMD, several folder workgroups, the penalty
// rows from memory.  (Sharded runs then agree on the minimum of chain_pair.)
inline void plan_pair(const Switches& sw, const Shape& s, Plan& p) {
  const int K = s.K, KH = ((K + 1) / 2 + 3) & ~3, nctp = (KH + 15) / 16;
  int kw = ((K + 11) / 12 + 3) & ~3;                                  // clusters per folder workgroup (a multiple of 4): ~12 folders
  if (sw.chain_folders_set) { const int want = std::max(1, sw.chain_folders); kw = ((K + want - 1) / want + 3) & ~3; }
  const int F = (K + kw - 1) / kw;
  const double tiles_per_stream = (double)s.N / std::max(s.nb, 1) / 16.0 / (4.0 * std::max(p.chain_wgs - F, 1));
  const size_t lds_w = pair_worker_bytes(nctp, p.NS2, s.Q, s.C), lds_f = pair_folder_bytes(s.B, kw);
  const bool want = sw.chain != 0 && sw.chain_pair != 0 &&
                    (sw.chain_pair == 1 || sw.chain == 1 || tiles_per_stream <= (sw.chain_max_tpw_set ? sw.chain_max_tpw : PAIR_MAX_TILES_PER_PAIR));
  p.chain_pair = (want && !p.chain_ok && p.NCT > 7 && nctp >= 4 && nctp <= 7 && K % 4 == 0 && K - KH <= 16 * nctp && K - KH >= 4 && p.usig && p.dot_bf && p.NS2 <= 2 &&
                  p.NT4 <= 4 && s.nb <= 64 && s.cus >= 64 && F < p.chain_wgs / 4 && !s.oe_arith && !s.obj_arith && std::max(lds_w, lds_f) + FOLD_LDS_SLACK <= FOLD_LDS_BYTES) ? 1 : 0;
  p.KH = KH; p.chain_folders = F; p.chain_kw = kw;
}

// Stage 3, on the agreed flags: what follows from the path taken.
inline void plan_finish(const Switches& sw, const Shape& s, Plan& p) {
  const int want = std::min(sw.nrep, 8);      // replicas of the per-block contribution table (a power of two, <= 8 MB in all)
  p.nrep = 1; while (p.nrep * 2 <= want && (size_t)p.nrep * 2 * s.B * s.K <= (1u << 20)) p.nrep *= 2;
  // the folder reads AND resets every replica of the contribution table inside a block step (atomic exchanges on its critical
  // path): 4 replicas measured 0.4 us per step faster than 8 there (2: the workers' atomics start to queue, +2 us)
  if (p.chain_ok && !sw.nrep_set) p.nrep = std::min(p.nrep, 4);
  // wave-pair chain: 40 000 table entries spread the workers' atomics by themselves
  if (p.chain_pair && !sw.nrep_set) p.nrep = 1;
  p.upd_contig = (!p.chain_ok && !p.chain_pair && tiles_per_wave(s) >= CONTIG_MIN_TILES_PER_WAVE) ? 1 : 0;
}

// the whole plan of an unsharded fit (one rank has nobody to agree with)
inline Plan plan_unsharded(const Switches& sw, const Shape& s) {
  Plan p = plan_shape(sw, s);
  if (!p.limit) { plan_pair(sw, s, p); plan_finish(sw, s, p); }
  return p;
}

// ---- one k_tile launch: which instantiation, of which build, on what grid, with how much LDS -- a pure function of the scalar fields of Dev the tile launchers decide on (hmx_k_launch.inc: tile_geom)
struct TileGeom {
  int n = 0, nb = 1, K = 0, d = 0, B = 0, C = 0, Q = 0, NCT = 0, NQ = 0, NS = 0, NS2 = 0, KH = 0, ntitems = 0, nwmax = 0;
  int upd_tpw = 1, upd_threads = 512, upd_maxblocks = 256, upd_wps = 2, static_maxblocks = 0, usig = 0, dot_bf = 0;
  bool img3 = false;                           // the split-bf16 image exists (Dev::Yimg3)
  int fused_fold = 0, pen_lds = 0, chain_pair = 0, chain_kw = 0, r_store = 1;      // (fused_fold, r_store: set per launch by the callers)
};
enum class TileKind { Update = 0, Head = 1, Lloyd = 2, Seed = 3, Chain = 4 };      // (= k_tile's MODE of the plain variant)
constexpr const char* TILE_KIND_NAME[5] = {"update", "head", "lloyd", "seed", "chain"};
// k_tile<nct, mode, wps, usig> of the split-bf16 (bf) or the fp32 build, `blocks` workgroups of `threads`, `lds` bytes.  mode: the MODE that runs, 5 = chain without R stores,
// 6 = wave-pair chain (nct: cluster tiles of a half).  valid = false: nothing may be launched (LDS over the CU's, or -- set by the launcher -- no such instantiation).
struct TileLaunch { bool valid = false, bf = false; int nct = 0, mode = 0, wps = 2; bool usig = false; int threads = 0, blocks = 0; size_t lds = 0; };
// the split-bf16 build of a launch is taken when the workgroups that are to share a CU still fit its LDS with the larger image
inline bool bf_fits(const TileGeom& g, size_t rest, long long blocks) {
  const long long per_cu = (blocks + 255) / 256;
  return g.dot_bf && g.img3 && (image_bytes_bf(g.NCT, g.NS2) + rest) * (size_t)(per_cu < 1 ? 1 : per_cu) <= LDS_PER_CU;
}
inline TileLaunch plan_tile_launch(const TileGeom& g, TileKind kind, int workgroups) {
  TileLaunch t; t.nct = g.NCT; t.mode = (int)kind;
  long long blocks = workgroups; size_t rest = 0;
  if (kind == TileKind::Chain) {      // two waves per SIMD, two accumulator sets; one workgroup per CU (the caller's count)
    t.threads = 512; t.usig = g.usig != 0;
    rest = fold_table_bytes(g.B, g.K, g.Q, g.C, true, true, true);
    if (g.chain_pair) {      // (the wave-pair chain exists in the split-bf16 build only; cluster tiles of a half: K = 116 .. 128 -> 4, .. 160 -> 5, .. 192 -> 6, .. 224 -> 7)
      t.bf = true; t.nct = (g.KH + 15) / 16; t.mode = 6; t.usig = true;
      t.lds = std::max(pair_worker_bytes(t.nct, g.NS2, g.Q, g.C), pair_folder_bytes(g.B, g.chain_kw));
    } else {
      t.bf = image_bytes_bf(g.NCT, g.NS2) + rest + FOLD_LDS_SLACK <= FOLD_LDS_BYTES && bf_fits(g, rest, 1);
      if (t.bf && g.usig && !g.r_store) t.mode = 5;      // the variant without R stores: split-bf16 build only
    }
  } else if (kind == TileKind::Update) {
    const long long tiles = ((long long)g.n / (g.nb > 0 ? g.nb : 1) + 15) / 16 + (long long)g.Q + 1;
    const int wpb = g.upd_threads / 64;
    blocks = ((tiles + g.upd_tpw - 1) / g.upd_tpw + wpb - 1) / wpb;
    if (blocks > g.upd_maxblocks) blocks = g.upd_maxblocks;   // resident capacity (workgroups per CU x CUs)
    if (blocks > g.nwmax / wpb) blocks = g.nwmax / wpb;
    if (blocks < 1) blocks = 1;
    rest = fold_table_bytes(g.B, g.K, g.Q, g.C, g.fused_fold != 0, g.pen_lds != 0, true);
    t.bf = bf_fits(g, rest, blocks);
    if (g.upd_wps == 4) { t.wps = 4; t.usig = true; t.threads = 1024; }   // plan_shape: upd_threads == 1024, uniform sigma, K <= 64
    else { t.usig = g.usig != 0; t.threads = g.upd_threads; }
  } else {
    // MFMA tile passes over the static 16-cell tiles (head, Lloyd, seeding race): 256-thread workgroups, capped at one resident generation --
    // measured: 768-thread workgroups (one per CU) are 30% slower (tail effect)
    const bool lloyd = kind == TileKind::Lloyd;
    const int wpb = 256 / 64;
    blocks = (((long long)g.ntitems + g.upd_tpw - 1) / g.upd_tpw + wpb - 1) / wpb;
    if (blocks > g.nwmax / wpb) blocks = g.nwmax / wpb;
    if (g.static_maxblocks > 0 && blocks > g.static_maxblocks) blocks = g.static_maxblocks;      // (seeding with three workgroups per CU -- 166 registers would allow it -- measured: no gain, 1.53 / 1.55 ms of k-means initialisation)
    rest = lloyd ? lloyd_sum_bytes(g.K, g.d) : 0;
    if (lloyd && blocks > 512) blocks = 512;
    if (blocks < 1) blocks = 1;
    t.threads = 256; t.bf = bf_fits(g, rest, blocks) || (lloyd && bf_fits(g, rest, 256));
    // Lloyd with the larger image: two 256-thread workgroups per CU no longer fit next to their K x d sum tables -> one of 512 threads
    if (t.bf && lloyd && !bf_fits(g, rest, blocks)) {
      t.threads = 512; blocks = (blocks + 1) / 2; if (blocks > 256) blocks = 256;
      // one workgroup per CU (image + K x d sum table: 84 KB): THREE waves per SIMD -- the kernel needs 150 registers, and the MFMA chain, the
      // arg-min and the LDS sums of a tile run one after the other on one accumulator set: a third wave fills the gaps (round 6: 0.13 ms of 1.69 per
      // k-means initialisation at 1M cells against two waves per SIMD)
      if (g.NCT >= 5 && g.NCT <= 7) { t.wps = 3; t.threads = 768; }
    }
    // head variants: general sigma | uniform sigma | uniform sigma at 4 waves per SIMD (K <= 64)
    if (kind == TileKind::Head) { if (g.upd_wps == 4) { t.wps = 4; t.usig = true; } else t.usig = g.usig != 0; }
  }
  if (t.mode != 6) t.lds = (t.bf ? image_bytes_bf(g.NCT, g.NS2) : image_bytes_f32(g.NQ, g.NS)) + rest;
  t.blocks = (int)blocks; t.valid = t.lds <= LDS_PER_CU && t.blocks >= 1;
  return t;
}

// ---- one launch of the ridge correction (moe_correct_ridge): statistics, device solve, apply -- a pure function of the scalar fields of Dev and Launch its
// launchers decide on (hmx_k_launch.inc: ridge_geom)
struct RidgeGeom {
  int K = 0, KP = 0, d = 0, B = 0, C = 0, Q = 0, NCT = 0;
  int moe_mfma = 0, st_dma = 0, st_halves = 1, st_KH = 0, st_nwg = 0, wNQ = 0, wNS = 0;
  int nitems = 0, naitems = 0, grid = 2048;      // static work lists of <= 256 / <= 1024 cells; workgroups of the streaming kernels (Launch::grid)
  int solve_lds = 0;      // Dev::solve_lds: the solve may keep its systems in LDS
};
enum class RidgeKind { Stats = 0, Solve = 1, Apply = 2 };
constexpr const char* RIDGE_KIND_NAME[3] = {"stats", "solve", "apply"};
// mfma = false: the first-generation kernels k_moe_stats<p0 = DP> / k_moe_apply<p0 = KPL, p1 = DPL>; true: k_moe_stats_q<p0 = cluster tiles of a half or of the whole,
// p1 = SHL> (+ k_moe_stats_reduce on rgx x rgy workgroups behind it) / k_moe_apply_mfma<p0 = NPT>.  The solve is one kernel (mfma: it also writes the table's MFMA image);
// its three lds_* values go into SolveArgs.  valid = false: nothing may be launched (LDS over the limit, or no instantiation for the parameters).
struct RidgeLaunch {
  bool valid = false, mfma = false; int p0 = 0, p1 = 0, gx = 1, gy = 1, gz = 1, threads = 0; size_t lds = 0;
  size_t lds_b_bytes = 0, lds_body_bytes = 0, lds_mask_off = 0; int rgx = 0, rgy = 0;
  // the solve: lds_sys_off > 0 -- cov and rhs live in LDS at that byte offset, behind the `lds` bytes of the form above (which keep their meaning); lds_total = what the launch asks for
  size_t lds_sys_off = 0, lds_total = 0;
};
inline size_t solve_sys_bytes(int B, int d) { return ((size_t)B + 1) * ((size_t)B + 1 + d) * sizeof(double); }      // cov [M][M] and rhs [d][M], M = B + 1
inline RidgeLaunch plan_ridge_launch(const RidgeGeom& g, RidgeKind kind) {
  RidgeLaunch t; t.mfma = g.moe_mfma != 0;
  if (g.K < 1 || g.d < 1) return t;
  const auto clamp = [](long long v, long long hi) { return (int)std::max<long long>(1, std::min(v, hi)); };
  if (kind == RidgeKind::Solve) {      // one workgroup per cluster
    const size_t ints = solve_index_bytes(g.B, g.C, false), panel = solve_panel_bytes(g.B), ball = solve_rhs_bytes(g.B, g.d);
    // the d right-hand sides live in LDS during the substitution where they fit the budget beside the index words -- or the panel's space anyway (d <= 16)
    const size_t body = ints + ball <= SOLVE_RHS_LDS_BYTES ? std::max(panel, ball) : panel;
    t.lds_b_bytes = body >= ball ? ball : 0; t.lds_body_bytes = body; t.lds = ints + body;
    // coupling masks of the Schur complement -- only with several covariates, and only while they are small
    const size_t moff = (ints + body + 7) & ~(size_t)7, maskb = solve_mask_bytes(g.B);
    if (g.C > 1 && moff + maskb <= SOLVE_MASK_LDS_BYTES) { t.lds_mask_off = moff; t.lds = moff + maskb; }
    t.gx = g.K; t.threads = g.B + 1 > 48 ? 1024 : 256;
    t.valid = ints + body <= SOLVE_LDS_BYTES;      // (plan_shape: solve_on_device admits no shape beyond it)
    t.lds_total = t.lds;
    // (measured at 11 rows only: 37.4 -> 32.8 us per launch; what a design near the limit, ~115 rows and 150 KB of LDS per workgroup, gains or loses is not measured)
    if (g.solve_lds) {      // the systems in LDS where they fit behind all of that (11 rows at 10 levels: 5.4 KB); larger designs keep the global scratch
      const size_t soff = (t.lds + 7) & ~(size_t)7;
      if (soff + solve_sys_bytes(g.B, g.d) <= SOLVE_LDS_BYTES) { t.lds_sys_off = soff; t.lds_total = soff + solve_sys_bytes(g.B, g.d); }
    }
  } else if (kind == RidgeKind::Stats && t.mfma) {
    // slot form: 16-byte operand loads + deterministic slot reduction; a wave per PC tile incl. the ones column at index d; y: the halves of the clusters (K > 128)
    t.p0 = g.st_halves == 2 ? (g.st_KH + 15) / 16 : g.NCT;
    t.gx = g.st_nwg; t.gy = g.st_halves; t.threads = 64 * ((g.d + 16) / 16);
    // (round 6) fp64 shadow sums in LDS + operands one tile ahead where two workgroups still fit a CU next to them (else the round-3 form)
    const size_t shl = (size_t)(t.threads / 64) * t.p0 * 4 * 64 * sizeof(double);
    t.p1 = 2 * shl <= LDS_BUDGET ? 1 : 0; t.lds = t.p1 ? shl : 0;
    t.rgx = g.Q; t.rgy = (int)(((size_t)g.K * g.d + g.K + 255) / 256);
    t.valid = g.st_dma && t.p0 >= 1 && t.p0 <= 8 && t.threads <= 320 && t.gx >= 1;
  } else if (kind == RidgeKind::Stats) {      // first generation: PCs in chunks of DP <= 32 (grid.z), 128 clusters per grid.y
    const int zch = (g.d + 31) / 32;
    t.p0 = ((g.d + zch - 1) / zch + 3) / 4 * 4;
    t.gx = clamp(((long long)g.nitems + 3) / 4, g.grid); t.gy = (g.K + 127) / 128; t.gz = (g.d + t.p0 - 1) / t.p0; t.threads = 256;
    t.valid = t.p0 >= 4 && t.p0 <= 32;
  } else {      // apply: one workgroup per apply item, at most four per streaming workgroup
    t.gx = clamp(g.naitems, 4ll * g.grid); t.threads = 256;
    if (t.mfma) { t.p0 = (g.d + 15) / 16; t.lds = (size_t)g.wNQ * g.wNS * 1024; t.valid = t.p0 >= 1 && t.p0 <= 4; }      // the table's image of one combination
    else { t.p0 = g.KP / 64; t.p1 = g.d > 64 ? 2 : 1; t.lds = (size_t)g.K * 64 * t.p1 * sizeof(float); t.valid = t.p0 >= 1 && t.p0 <= 4 && g.d <= 128; }
    t.valid = t.valid && t.lds <= LDS_PER_CU;
  }
  return t;
}

}  // namespace hmx
