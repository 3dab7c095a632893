// Host-side probe of the launch plan hmx_setup makes (harmony_amd/csrc/hmx_plan.h, HIP-free): built by tests/test_plan_cpu.py with the host
// compiler and called through ctypes.  Reads the HMX_* switches from the environment, like the library.
#include "../../harmony_amd/csrc/hmx_plan.h"
#include <cstring>
extern "C" {
// shape: PLAN_SHAPE of tests/test_plan_cpu.py, out: its PLAN_FIELDS; returns 1 and the limit's message when the plan refuses the shape
int probe_plan(const long long* v, int* out, char* limit, int cap) {
  hmx::Shape s;
  s.N = v[0]; s.N_global = v[1]; s.d = (int)v[2]; s.K = (int)v[3]; s.B = (int)v[4]; s.C = (int)v[5]; s.Q = (int)v[6]; s.nb = (int)v[7];
  s.cells_per_block = (uint64_t)v[8]; s.world = (int)v[9]; s.sharded = v[10] != 0; s.cus = (int)v[11]; s.usig = v[12] != 0;
  s.ridge_arith = (int)v[13]; s.oe_arith = (int)v[14]; s.obj_arith = (int)v[15]; s.solve_arith = (int)v[16];
  s.tun_wps = (int)v[17]; s.tun_tpw = (int)v[18]; s.grid = (int)v[19]; s.ntitems = (int)v[20];
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
