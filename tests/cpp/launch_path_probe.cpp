// Host-side probe of the launch diet's decisions (harmony_amd/csrc/hmx_round.h, hmx_plan.h; HIP-free): built by tests/test_launch_path_cpu.py with the host
// compiler and called through ctypes.  A script of operations drives one RoundLedger the way hmx_init_cluster / hmx_cluster / hmx_restart drive the handle's
// (head_pass and update_R, hmx_api_seam.inc / hmx_api_update.inc) and returns, for every head, the clears and the objective flag plan_head decided.
#include "../../harmony_amd/csrc/hmx_round.h"
#include "../../harmony_amd/csrc/hmx_plan.h"
namespace {
enum Op { OP_HEAD = 0, OP_ROUND = 1, OP_RESTART = 2 };
}
extern "C" {
// cfg: LP_CFG of the test; ops: [n][4] = (op, a, b, c); out: [n][8] = HEAD_FIELDS of the test for a head, (path, close, clear_sets) for a round
void probe_launch_path(const long long* cfg, const long long* ops, int n, long long* out) {
  hmx::RoundIn in; hmx::HeadIn head; hmx::RoundLedger lg; uint64_t round_counter = 0;
  in.sharded = cfg[0] != 0; in.B = (int)cfg[1]; in.K = (int)cfg[2]; in.nb = (int)cfg[3]; in.nrep = (int)cfg[4]; in.fused_ok = cfg[5] != 0; in.chain_ok = cfg[6] != 0;
  in.chain_pair = cfg[7] != 0; in.carry_ok = cfg[8] != 0; in.shuf_inv = in.carry_ok; in.poll = cfg[9] != 0; in.r_store_always = cfg[10] != 0; in.obj_arith = cfg[11] != 0; in.seed = 1;
  head.carry_ok = in.carry_ok; head.NT4 = 3; head.NCT = 7; head.upd_wps = 2; head.max_iter_kmeans = (int)cfg[12]; head.poll = in.poll; head.r_store_always = in.r_store_always;
  head.sharded = in.sharded; head.ref_arith = in.obj_arith; head.seed = in.seed;
  const auto prepare = [&](uint64_t round, bool host_order) {      // prepare_round
    if (!host_order) { if (!lg.is_order(round, in.seed)) for (uint64_t r = round; r <= (round | 3); r++) lg.sorted(r, in.seed, in.carry_ok); }
    else { lg.lost(round); in.injected_round = (int64_t)round; }
  };
  for (int i = 0; i < n; i++) {
    const long long* op = ops + 4 * i; long long* row = out + 8 * i;
    for (int k = 0; k < 8; k++) row[k] = 0;
    if (op[0] == OP_HEAD) {      // head_pass(normalise = a), b: a host order is queued
      head.normalise = op[1] != 0; head.host_order = op[2] != 0; head.round = (int64_t)round_counter;
      if (hmx::head_gathers(head)) prepare(round_counter, false);
      lg.r_rewritten();
      const hmx::HeadPlan p = hmx::plan_head(head, lg);
      if (p.files) lg.head_filed(head.round, head.seed);
      lg.head_started(); lg.head_folded();
      const long long f[] = {p.clear_O, p.clear_set, p.clear_objpart, p.clear_first, p.skip_obj, p.r_store, p.files, 0};
      for (int k = 0; k < 8; k++) row[k] = f[k];
    } else if (op[0] == OP_ROUND) {      // update_R with last_round_hint = a, round_may_be_last = b, c: this round's order comes from the host
      prepare(round_counter, op[3] != 0);
      in.round = (int64_t)round_counter++; in.last_round_hint = op[1] != 0; in.round_may_be_last = op[2] != 0;
      const hmx::RoundPlan p = hmx::plan_round(in, lg);
      lg.round_started();
      if (p.path == hmx::PATH_STEP_LOOP) lg.step_loop_used();
      if (p.write_next) lg.round_filed_next(in.round, in.seed);
      if (p.close != hmx::CLOSE_REDUCE_SNAPSHOT) lg.tail_cleared();
      lg.flip();
      row[0] = p.path; row[1] = p.close; row[2] = p.clear_sets;
    } else if (op[0] == OP_RESTART) { lg.restart(); round_counter = 0; }
  }
}
// the solve's launch with its systems in LDS or not: out = (lds, lds_sys_off, lds_total) for (K, d, B, C, solve_lds)
void probe_solve_lds(int K, int d, int B, int C, int solve_lds, long long* out) {
  hmx::RidgeGeom g; g.K = K; g.KP = (K + 63) / 64 * 64; g.d = d; g.B = B; g.C = C; g.Q = B; g.NCT = (K + 15) / 16; g.moe_mfma = 1; g.st_dma = 1; g.st_nwg = 64; g.solve_lds = solve_lds;
  const hmx::RidgeLaunch t = hmx::plan_ridge_launch(g, hmx::RidgeKind::Solve);
  out[0] = (long long)t.lds; out[1] = (long long)t.lds_sys_off; out[2] = (long long)t.lds_total;
}
}
