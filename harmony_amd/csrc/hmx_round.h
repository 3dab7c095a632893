// hmx_round.h -- what a clustering round decides between its launches, as pure functions of the handle's switches and a small ledger:
// which path runs, whether old contributions are carried, which buffers are cleared up front, whether R rows are written, how the round
// closes.  Plain C++17 like hmx_plan.h: no HIP, no handle (tests/cpp/plan_probe.cpp drives it on the CPU; update_R and head_pass dispatch on it).
#pragma once
#include <cstddef>
#include <cstdint>

namespace hmx {

// What the host knows about the four order sets (round & 3), the two old-contribution tables and the three replica sets.  A wrong entry
// does not crash: it subtracts a stale table or skips R rows a getter serves later -- so every transition is a method, written once.
struct RoundLedger {
  struct OrderSet { int64_t round = -1; uint64_t seed = 0; bool nxt = false; };      // nxt: tiles keyed by (block, block of the NEXT round)
  struct OldTable { int state = 1; int64_t round = -1; uint64_t seed = 0; };         // state: 0 all zero | 1 unknown contents | 2 filed for `round`
  OrderSet sets[4];
  OldTable old[2]; int cur = 0;      // `cur`: what this round's block steps subtract; the other table collects the next round's
  bool sets_clean = false;           // the three replica sets are all zero
  // The head's own tables (O, its replica set Dev::Snew_fx, the objective slots).  head_set_clean: the head's replica set is all zero -- k_fold re-zeroes what
  // it sums, and on the chain / fold-in-prologue paths nothing else writes that buffer (the rounds use the three sets).  fresh: no head has run since setup
  // or hmx_restart -- that head clears everything, whatever the rest of the ledger says.
  bool head_set_clean = false, fresh = true;

  void sorted(uint64_t round, uint64_t seed, bool nxt) { sets[round & 3] = OrderSet{(int64_t)round, seed, nxt}; }
  void lost(uint64_t round) { sets[round & 3] = OrderSet{}; }      // (a host-provided order went into the set, or the set's run is over)
  bool is_order(uint64_t round, uint64_t seed) const { return sets[round & 3].round == (int64_t)round && sets[round & 3].seed == seed; }
  bool keyed_by_next(uint64_t round) const { return sets[round & 3].nxt; }
  void r_rewritten() { for (OldTable& t : old) if (t.state == 2) t.state = 1; }      // filed sums describe rows that are gone
  bool filed_for(int64_t round, uint64_t seed) const { return old[cur].state == 2 && old[cur].round == round && old[cur].seed == seed; }
  void head_filed(int64_t round, uint64_t seed) { old[cur] = OldTable{2, round, seed}; }
  void round_filed_next(int64_t round, uint64_t seed) { old[cur ^ 1] = OldTable{2, round + 1, seed}; }
  void sets_used() { sets_clean = false; }
  void round_started() { old[cur].state = 1; sets_used(); }      // the block steps subtract `cur` and sum into the replica sets
  void tail_cleared() { old[cur].state = 0; sets_clean = true; }      // the closing launch zeroed the consumed table and the replica sets
  void flip() { cur ^= 1; }
  void head_started() { head_set_clean = false; }      // the head's tiles sum into its replica set ...
  void head_folded() { head_set_clean = true; fresh = false; }      // ... and k_fold behind them has been queued: zero again
  void step_loop_used() { head_set_clean = false; }      // the launch-per-step rounds ping-pong through the head's replica set
  void restart() { r_rewritten(); for (OrderSet& s : sets) s = OrderSet{}; head_set_clean = false; fresh = true; }
  void reset() { *this = RoundLedger{}; }
};

enum RoundPath { PATH_CHAIN = 0, PATH_FOLD_PROLOGUE = 1, PATH_STEP_LOOP = 2 };
enum RoundClose { CLOSE_CHAIN_TAIL = 0, CLOSE_WIDE_CLEAR_TAIL = 1, CLOSE_TAIL = 2, CLOSE_REDUCE_SNAPSHOT = 3 };
// k_foldpen (one launch, K/16 workgroups, every thread walks B/16 levels x the replicas) suits small tables: its LDS holds B <= 512 levels, and with
// thousands of entries (configs[4]: 200 levels x 200 clusters) one thread per entry in two launches is faster, unless the fused / chain paths apply
constexpr size_t FOLDPEN_MAX_LEVELS = 64 * 1024 / 128, FOLDPEN_MAX_ENTRIES = 8192;
// k_round_tail clears the consumed tables with its few workgroups, one per slot row: beyond this many entries (configs[4]: 7.4 MB of tables, 88 us
// of a tail -- rocprofv3, round 6: 2.5 ms of a 52 ms run) a wide clearing launch goes in front of it
constexpr size_t TAIL_CLEAR_MAX_ENTRIES = (size_t)1 << 18;
constexpr int CHAIN_TAIL_MAX_BLOCKS = 62;      // the sharded chain's objective exchange rides behind nb + 1 block exchanges

struct RoundIn {
  bool sharded = false, inbox_ok = false;      // world > 1 || comm_force; p2p_on && p2p_world == world && !comm_force
  int B = 0, K = 0, nb = 1, nrep = 1, p2p_cap = 65536;      // (p2p_cap: P2P_CAP, entries an inbox holds per plane and source)
  bool fused_ok = false, chain_ok = false, chain_pair = false, carry_ok = false, shuf_inv = false, obj_arith = false;
  bool poll = false, r_store_always = false, last_round_hint = false, round_may_be_last = true;
  uint64_t seed = 0; int64_t round = 0, injected_round = -1;
  int fold_impl = 0;      // Switches::fold_impl
};
struct RoundPlan {
  bool merged = false, p2p = false; int path = PATH_STEP_LOOP; bool chain_tail = false;
  unsigned exchanges = 0;                      // what this round adds to p2p_xseq
  bool carried = false, gen_blocks = false;    // no pass over R for the old contributions | the pass needs k_shuf_blocks first
  bool clear_sets = false, clear_cur = false, clear_next = false;      // memsets in front of the round
  bool write_next = false; int r_store = 1;
  bool reduce_old = false;                     // the old sums are all-reduced (the p2p chain's folder exchanges them itself)
  int close = CLOSE_REDUCE_SNAPSHOT;
};
// the ledger as prepare_round left it: the round's order set is in place
inline RoundPlan plan_round(const RoundIn& in, const RoundLedger& lg) {
  RoundPlan p;
  const size_t nBK = (size_t)in.B * in.K;
  p.merged = (size_t)in.B <= FOLDPEN_MAX_LEVELS && in.fold_impl != 1 && (in.fused_ok || nBK <= FOLDPEN_MAX_ENTRIES || in.fold_impl == 2);
  // sharded: the chain needs the in-launch exchange over the peers' inboxes (hmx_p2p_*); without it, one launch + one collective per block
  p.p2p = in.sharded && in.inbox_ok && nBK <= (size_t)in.p2p_cap;
  const bool chain = ((p.merged && in.fused_ok && in.chain_ok) || in.chain_pair) && (!in.sharded || p.p2p);
  p.path = chain ? PATH_CHAIN : (p.merged && in.fused_ok) ? PATH_FOLD_PROLOGUE : PATH_STEP_LOOP;
  // one GPU: the chain's folder also closes the round (objective snapshot, table clears, control reset); sharded with the in-launch exchange too -- the
  // ranks' objective sums travel through the inboxes, entries nBK and nBK + 1.  (Pair chain: several folders, a slice each: k_round_tail closes.)
  p.chain_tail = chain && (!in.sharded || (p.p2p && nBK + 2 <= (size_t)in.p2p_cap && in.nb <= CHAIN_TAIL_MAX_BLOCKS)) && !in.obj_arith && !in.chain_pair;
  p.exchanges = (chain && p.p2p) ? (unsigned)in.nb + 1u + (p.chain_tail ? 1u : 0u) : 0u;      // nb + 1 block steps (+ the objective's)
  p.clear_sets = !lg.sets_clean;
  p.carried = lg.filed_for(in.round, in.seed) && lg.is_order((uint64_t)in.round, in.seed);      // (same Feistel permutation as the sort's)
  p.clear_cur = !p.carried && lg.old[lg.cur].state != 0;
  p.gen_blocks = !p.carried && in.shuf_inv && in.injected_round != in.round;      // (the sort-free shuffle leaves D.blk alone; a host order brought its own)
  p.reduce_old = !(chain && p.p2p);
  // this round's tile kernels collect the next round's old contributions if this round's tiles are keyed by the next block
  p.write_next = in.carry_ok && lg.keyed_by_next((uint64_t)in.round) && !in.last_round_hint;
  p.clear_next = p.write_next && lg.old[lg.cur ^ 1].state != 0;
  // R rows nobody reads are not written: this round's rows are dead if the NEXT round takes its old contributions from the carried sums
  // (write_next) and this round cannot be the call's last (round_may_be_last, set by hmx_cluster) -- moe_correct_ridge_cpp, the getters
  // and a stand-alone compute_objective only ever see the last round's R.  (A host with an abort poll may leave the call early: it
  // always gets its rows.  HMX_R_STORE=1: always store.  obj_arith: the round's objective is summed from R itself -- k_obj_terms_mfma and
  // every pass of k_seq_objr_pass read the rows -- so every round stores them.)
  p.r_store = (p.write_next && !in.round_may_be_last && !in.poll && !in.r_store_always && !in.obj_arith) ? 0 : 1;
  const size_t cleared = (size_t)in.nb * nBK + 3 * (size_t)in.nrep * nBK;      // the table this round consumed + the replica sets
  p.close = p.chain_tail ? CLOSE_CHAIN_TAIL : (in.sharded || in.obj_arith) ? CLOSE_REDUCE_SNAPSHOT : cleared > TAIL_CLEAR_MAX_ENTRIES ? CLOSE_WIDE_CLEAR_TAIL : CLOSE_TAIL;
  return p;
}

struct HeadIn {
  bool carry_ok = false, host_order = false;      // host_order: an injected order is queued, or the R-compatible stream draws the shuffles
  bool normalise = false; int NT4 = 0, NCT = 0, upd_wps = 2;
  int max_iter_kmeans = 0; bool poll = false, r_store_always = false;
  uint64_t seed = 0; int64_t round = 0;            // the round that follows the head
  // sharded: world > 1 || comm_force; ref_arith: any of oe_arith / obj_arith (their heads and rounds keep their own sums)
  bool sharded = false, ref_arith = false;
};
// clear_O / clear_set / clear_objpart (and clear_first, the stale old-contribution table): what the launch in front of the head's tiles zeroes -- none: no launch.
// skip_obj: the head leaves no objective partials (Dev::head_noobj) and no reduction follows it.
struct HeadPlan {
  bool gather = false, fused_norm = false, files = false, clear_first = false; int r_store = 1;
  bool clear_O = true, clear_set = true, clear_objpart = true, skip_obj = false;
};
// With the round-to-round carry the head runs over the padded order of the round that FOLLOWS it (init_cluster_cpp's too) and files its R sums
// as that round's old contributions: no pass over R between the head and the first round.
inline bool head_gathers(const HeadIn& in) { return in.carry_ok && !in.host_order; }
// the ledger as prepare_round left it (head_gathers: the following round's order set is in place)
inline HeadPlan plan_head(const HeadIn& in, const RoundLedger& lg) {
  HeadPlan p;
  p.gather = head_gathers(in);
  // the register-pipelined head (two accumulator sets, rows of a tile in registers) normalises the rows it has loaded anyway
  p.fused_norm = in.normalise && in.NT4 <= 4 && in.NCT <= 7 && in.upd_wps != 4;
  p.files = p.gather && lg.keyed_by_next((uint64_t)in.round) && lg.is_order((uint64_t)in.round, in.seed);
  p.clear_first = p.files && lg.old[lg.cur].state != 0;
  // the head of cluster_cpp is followed, inside the same call, by a round that rewrites every R row and takes its old contributions from
  // the sums filed here: the head's own rows are never read (Dev::r_store) -- 4K bytes per cell less.  (init_cluster_cpp's head is followed
  // by the caller, who may read R: it stores.)
  p.r_store = (p.files && in.normalise && in.max_iter_kmeans >= 1 && !in.poll && !in.r_store_always) ? 0 : 1;
  // The clears.  O: k_fold behind the head overwrites it (fold mode 3) -- no clear.  The head's replica set: zero since the last head's k_fold
  // (head_set_clean).  The objective slots: every launch that sums them zeroes what it read, so they are zero between the passes.  The first head
  // after setup / hmx_restart, a host that provides the order, polls or asked for every R row, sharded and reference-arithmetic handles keep every
  // clear: their calls may end or interleave in ways the ledger does not follow.
  const bool keep_all = lg.fresh || in.host_order || in.poll || in.r_store_always || in.sharded || in.ref_arith;
  p.clear_O = keep_all; p.clear_objpart = keep_all; p.clear_set = keep_all || !lg.head_set_clean;
  // cluster_cpp's head (normalise) with at least one round behind it and no poll: obj[0..1] is overwritten by the first round's close before anything
  // reads it -- hmx_cluster takes no snapshot between them --, so the head's partial sums and their reduction are not needed
  p.skip_obj = !keep_all && in.normalise && in.max_iter_kmeans >= 1;
  return p;
}

}  // namespace hmx
