// Host-side probe of the launch plan hmx_setup makes (harmony_amd/csrc/hmx_plan.h, HIP-free): built by tests/test_plan_cpu.py with the host
// compiler and called through ctypes.  Reads the HMX_* switches from the environment, like the library.
#include "../../harmony_amd/csrc/hmx_plan.h"
#include <cstring>
static hmx::Shape shape_of(const long long* v) {
  hmx::Shape s;
  s.N = v[0]; s.N_global = v[1]; s.d = (int)v[2]; s.K = (int)v[3]; s.B = (int)v[4]; s.C = (int)v[5]; s.Q = (int)v[6]; s.nb = (int)v[7];
  s.cells_per_block = (uint64_t)v[8]; s.world = (int)v[9]; s.sharded = v[10] != 0; s.cus = (int)v[11]; s.usig = v[12] != 0;
  s.ridge_arith = (int)v[13]; s.oe_arith = (int)v[14]; s.obj_arith = (int)v[15]; s.solve_arith = (int)v[16];
  s.tun_wps = (int)v[17]; s.tun_tpw = (int)v[18]; s.grid = (int)v[19]; s.ntitems = (int)v[20];
  return s;
}
// the geometry hmx_setup writes into Dev for this plan (the split image is always allocated); r_store and fused_fold are set per launch by the callers
static hmx::TileGeom geom_of(const hmx::Shape& s, const hmx::Plan& p, int r_store, int fused_fold) {
  hmx::TileGeom g;
  g.n = (int)s.N; g.nb = s.nb; g.K = s.K; g.d = s.d; g.B = s.B; g.C = s.C; g.Q = s.Q;
  g.NCT = p.NCT; g.NQ = p.NQ; g.NS = p.NS; g.NS2 = p.NS2; g.KH = p.KH; g.ntitems = s.ntitems; g.nwmax = p.nwmax;
  g.upd_tpw = p.upd_tpw; g.upd_threads = p.upd_threads; g.upd_maxblocks = p.upd_maxblocks; g.upd_wps = p.upd_wps; g.static_maxblocks = p.static_maxblocks;
  g.usig = p.usig; g.dot_bf = p.dot_bf; g.img3 = true;
  g.fused_fold = fused_fold; g.pen_lds = p.pen_lds; g.chain_pair = p.chain_pair; g.chain_kw = p.chain_kw; g.r_store = r_store;
  return g;
}
// out: RAN (0: the library never makes this launch for the shape), then LAUNCH_FIELDS of tests/test_plan_cpu.py
static void launch_row(const hmx::Shape& s, const hmx::Plan& p, int kind, int workgroups, int r_store, int fused_fold, long long* out) {
  const bool chain = p.chain_ok || p.chain_pair;
  // the path of the unsharded plan: the chain folds in its prologue; off it the update does where the tables fit (fused_fold < 0: as the plan says)
  const int ff = fused_fold >= 0 ? fused_fold : (kind == 4 || (!chain && p.fused_ok)) ? 1 : 0;
  const hmx::TileLaunch t = hmx::plan_tile_launch(geom_of(s, p, r_store, ff), (hmx::TileKind)kind, workgroups);
  // Lloyd runs on the tile kernel where the fp32 image and the sum table fit (else k_lloyd), the chain where the plan takes it
  out[0] = kind == 2 ? hmx::lloyd_tile_fits(p.NQ, p.NS, s.K, s.d) : kind == 4 ? chain : 1;
  const long long f[] = {t.valid, t.bf, t.nct, t.mode, t.wps, t.usig, t.threads, t.blocks, (long long)t.lds};
  for (int i = 0; i < 9; i++) out[1 + i] = f[i];
}
// the geometry hmx_setup writes into Dev / Launch for this plan (RIDGE_GEOM of tests/test_plan_cpu.py); nitems / naitems: the static work lists of <= 256 / <= 1024 cells
static void ridge_geom_row(const hmx::Shape& s, const hmx::Plan& p, int nitems, int naitems, long long* g) {
  const long long f[] = {s.K, p.KP, s.d, s.B, s.C, s.Q, p.NCT, p.moe_mfma, p.st_dma, p.st_halves, p.st_KH, p.st_nwg, p.wNQ, p.wNS, nitems, naitems, s.grid};
  for (int i = 0; i < 17; i++) g[i] = f[i];
}
static hmx::RidgeGeom ridge_geom_of(const long long* g) {
  hmx::RidgeGeom r;
  r.K = (int)g[0]; r.KP = (int)g[1]; r.d = (int)g[2]; r.B = (int)g[3]; r.C = (int)g[4]; r.Q = (int)g[5]; r.NCT = (int)g[6]; r.moe_mfma = (int)g[7]; r.st_dma = (int)g[8];
  r.st_halves = (int)g[9]; r.st_KH = (int)g[10]; r.st_nwg = (int)g[11]; r.wNQ = (int)g[12]; r.wNS = (int)g[13]; r.nitems = (int)g[14]; r.naitems = (int)g[15]; r.grid = (int)g[16];
  return r;
}
extern "C" {
// the ridge correction: the geometry of the shape's plan (returns 1 when the plan refuses the shape; solve_on_device: the plan's) ...
int probe_ridge_geom(const long long* v, int nitems, int naitems, long long* geom, int* solve_on_device) {
  const hmx::Shape s = shape_of(v);
  const hmx::Plan p = hmx::plan_unsharded(hmx::read_switches(), s);
  if (p.limit) return 1;
  ridge_geom_row(s, p, nitems, naitems, geom); *solve_on_device = p.solve_on_device;
  return 0;
}
// ... and one launch of a geometry (kind = RidgeKind): out = RIDGE_FIELDS of tests/test_plan_cpu.py
void probe_ridge_launch(const long long* geom, int kind, long long* out) {
  const hmx::RidgeLaunch t = hmx::plan_ridge_launch(ridge_geom_of(geom), (hmx::RidgeKind)kind);
  const long long f[] = {t.valid, t.mfma, t.p0, t.p1, t.gx, t.gy, t.gz, t.threads, (long long)t.lds, (long long)t.lds_b_bytes, (long long)t.lds_body_bytes, (long long)t.lds_mask_off, t.rgx, t.rgy};
  for (int i = 0; i < 14; i++) out[i] = f[i];
}
// one k_tile launch of the shape's plan: kind = TileKind, workgroups = the chain's; out: 10 values (launch_row); returns 1 when the plan refuses the shape
int probe_tile_launch(const long long* v, int kind, int workgroups, int r_store, int fused_fold, long long* out) {
  const hmx::Shape s = shape_of(v);
  const hmx::Plan p = hmx::plan_unsharded(hmx::read_switches(), s);
  if (p.limit) return 1;
  launch_row(s, p, kind, workgroups, r_store, fused_fold, out);
  return 0;
}
// the same for K = 1 .. 256 and the five kinds, one chain workgroup per CU: out [256][5][10]; refused shapes have RAN = -1
void probe_tile_sweep(const long long* v, int r_store, long long* out) {
  hmx::Shape s = shape_of(v);
  const hmx::Switches sw = hmx::read_switches();
  for (int K = 1; K <= 256; K++) {
    s.K = K;
    const hmx::Plan p = hmx::plan_unsharded(sw, s);
    for (int kind = 0; kind < 5; kind++) {
      long long* row = out + ((size_t)(K - 1) * 5 + kind) * 10;
      if (p.limit) row[0] = -1; else launch_row(s, p, kind, s.cus, r_store, -1, row);
    }
  }
}
// shape: PLAN_SHAPE of tests/test_plan_cpu.py, out: its PLAN_FIELDS; returns 1 and the limit's message when the plan refuses the shape
int probe_plan(const long long* v, int* out, char* limit, int cap) {
  const hmx::Shape s = shape_of(v);
  const hmx::Plan p = hmx::plan_unsharded(hmx::read_switches(), s);
  if (p.limit) { strncpy(limit, p.limit, (size_t)cap - 1); limit[cap - 1] = 0; return 1; }
  const int f[] = {p.KP, p.zs, p.NCT, p.NQ, p.NT4, p.tail, p.NS, p.NS2, p.wNQ, p.wNT4, p.wtail, p.wNS, p.moe_mfma, p.dot_bf, p.usig, p.rvec, p.pen_lds,
                   p.upd_wps, p.upd_threads, p.upd_maxblocks, p.upd_tpw, p.static_maxblocks, p.oldsum_stream, p.need_lorder, p.nwmax, p.objslots,
                   p.r_store_always, p.carry_ok, p.qmask, p.nkeys, p.npad, p.shuf_inv, p.solve_on_device, p.st_KH, p.st_halves, p.st_dma, p.st_cpw, p.st_nwg,
                   p.fused_ok, p.chain_ok, p.chain_wgs, p.chain_pair, p.KH, p.chain_folders, p.chain_kw, p.nrep, p.upd_contig};
  for (size_t i = 0; i < sizeof(f) / sizeof(f[0]); i++) out[i] = f[i];
  return 0;
}
}
