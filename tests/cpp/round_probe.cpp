// Host-side probe of the round plan and its ledger (harmony_amd/csrc/hmx_round.h, HIP-free): built by tests/test_round_cpu.py with the host
// compiler and called through ctypes.  A script of operations drives one RoundLedger the way the library's entry points do -- prepare_round,
// head_pass, update_R, update_R_ref, hmx_restart (hmx_api_*.inc) -- and returns what plan_head / plan_round decided for every operation.
#include "../../harmony_amd/csrc/hmx_round.h"
#include "../../harmony_amd/csrc/hmx_plan.h"
namespace {
enum Op { OP_HEAD = 0, OP_ROUND = 1, OP_ROUND_REF = 2, OP_RESTART = 3, OP_SEED = 4, OP_RESORT = 5 };
struct Handle {      // the fields of hmx_ctx the round decisions read
  hmx::RoundIn in; hmx::HeadIn head; hmx::RoundLedger lg; uint64_t round_counter = 0;
  // prepare_round: a round of the counter-based shuffle is sorted with the rest of its group of four unless its set already holds it;
  // a host-provided order goes into the round's set on its own, keyed by the block alone
  void prepare(uint64_t round, bool host_order) {
    if (!host_order) { if (!lg.is_order(round, in.seed)) for (uint64_t r = round; r <= (round | 3); r++) lg.sorted(r, in.seed, in.carry_ok); }
    else { lg.lost(round); in.injected_round = (int64_t)round; }
  }
};
}  // namespace
extern "C" {
// cfg: ROUND_CFG of tests/test_round_cpu.py; ops: [n][4] = (op, a, b, c); out: [n][ROW_FIELDS] (rows of operations that plan nothing stay zero).
// HMX_FOLD_IMPL comes from the environment, like the library's.
void probe_round_script(const long long* cfg, const long long* ops, int n, long long* out) {
  Handle h;
  hmx::RoundIn& in = h.in;
  in.sharded = cfg[0] != 0; in.inbox_ok = cfg[1] != 0; in.B = (int)cfg[2]; in.K = (int)cfg[3]; in.nb = (int)cfg[4]; in.nrep = (int)cfg[5];
  in.fused_ok = cfg[6] != 0; in.chain_ok = cfg[7] != 0; in.chain_pair = cfg[8] != 0; in.carry_ok = cfg[9] != 0; in.shuf_inv = cfg[10] != 0; in.obj_arith = cfg[11] != 0;
  in.poll = cfg[12] != 0; in.r_store_always = cfg[13] != 0; in.seed = (uint64_t)cfg[14]; in.fold_impl = hmx::read_switches().fold_impl;
  h.head.carry_ok = in.carry_ok; h.head.NT4 = (int)cfg[15]; h.head.NCT = (int)cfg[16]; h.head.upd_wps = (int)cfg[17]; h.head.max_iter_kmeans = (int)cfg[18];
  h.head.poll = in.poll; h.head.r_store_always = in.r_store_always;
  for (int i = 0; i < n; i++) {
    const long long* op = ops + 4 * i; long long* row = out + 20 * i;
    for (int k = 0; k < 20; k++) row[k] = 0;
    hmx::RoundLedger& lg = h.lg;
    if (op[0] == OP_HEAD) {      // head_pass(normalise = a), b: a host order is queued / the R-compatible stream draws the shuffles
      hmx::HeadIn& hi = h.head;
      hi.normalise = op[1] != 0; hi.host_order = op[2] != 0; hi.seed = in.seed; hi.round = (int64_t)h.round_counter;
      if (hmx::head_gathers(hi)) h.prepare(h.round_counter, false);
      lg.r_rewritten();
      const hmx::HeadPlan p = hmx::plan_head(hi, lg);
      if (p.files) lg.head_filed(hi.round, hi.seed);
      const long long f[] = {p.gather, p.fused_norm, p.files, p.clear_first, p.r_store};
      for (int k = 0; k < 5; k++) row[k] = f[k];
    } else if (op[0] == OP_ROUND) {      // update_R with last_round_hint = a, round_may_be_last = b, c: this round's order comes from the host
      h.prepare(h.round_counter, op[3] != 0);
      in.round = (int64_t)h.round_counter++; in.last_round_hint = op[1] != 0; in.round_may_be_last = op[2] != 0;
      const long long before[] = {lg.old[lg.cur].state, lg.old[lg.cur ^ 1].state, lg.sets_clean};
      const hmx::RoundPlan p = hmx::plan_round(in, lg);
      lg.round_started();
      if (p.write_next) lg.round_filed_next(in.round, in.seed);
      if (p.close != hmx::CLOSE_REDUCE_SNAPSHOT) lg.tail_cleared();
      lg.flip();
      const long long f[] = {p.path, p.merged, p.chain_tail, p.carried, p.write_next, p.r_store, p.close, p.exchanges, p.p2p, p.gen_blocks, p.clear_sets, p.clear_cur, p.clear_next,
                             p.reduce_old, before[0], before[1], before[2]};
      for (int k = 0; k < 17; k++) row[k] = f[k];
    } else if (op[0] == OP_ROUND_REF) {      // update_R_ref: its own shuffle lists, the tile kernels' order from prepare_round, R rewritten outside the tables
      h.prepare(h.round_counter++, op[3] != 0);
      lg.sets_used(); lg.r_rewritten();
    } else if (op[0] == OP_RESTART) { lg.restart(); h.round_counter = 0; }
    else if (op[0] == OP_SEED) in.seed = (uint64_t)op[1];
    else if (op[0] == OP_RESORT) lg.sorted((uint64_t)op[1], in.seed, op[2] != 0);      // an order set sorted again for round a, keyed by the next block or not (b)
  }
}
}
#ifdef ROUND_PROBE_MAIN
// stand-alone (sanitizer builds): init_cluster + one cluster_cpp of m = 1 .. 8 rounds on the headline shape; carried rounds m, rounds without R min(m - 1, 4)
#include <cstdio>
int main() {
  const long long cfg[19] = {0, 0, 20, 100, 20, 4, 1, 1, 0, 1, 1, 0, 0, 0, 1, 3, 7, 2, 4};
  int bad = 0;
  for (int m = 1; m <= 8; m++) {
    long long ops[9 * 4] = {OP_HEAD, 0, 0, 0}, out[9 * 20];
    for (int it = 0; it < m; it++) { long long* o = ops + 4 * (it + 1); o[0] = OP_ROUND; o[1] = it == m - 1; o[2] = it == m - 1 || it > 3; o[3] = 0; }
    probe_round_script(cfg, ops, m + 1, out);
    int carried = 0, without = 0;
    for (int it = 1; it <= m; it++) { carried += (int)out[20 * it + 3]; without += out[20 * it + 5] == 0; }
    printf("m %d carried %d without_R %d\n", m, carried, without);
    bad += carried != m || without != (m - 1 < 4 ? m - 1 : 4) || out[20 * m + 5] != 1;
  }
  return bad;
}
#endif
