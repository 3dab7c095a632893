"""The round plan and its ledger (harmony_amd/csrc/hmx_round.h) as pure functions, checked without a GPU: tests/cpp/round_probe.cpp drives one ledger
the way hmx_init_cluster / hmx_cluster drive the handle's.  Every expected value below is derived from the expressions of update_R, head_pass and
prepare_round as they stood inline before the plan was lifted out of them, with the derivation beside it."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND_CFG = ("sharded", "inbox_ok", "B", "K", "nb", "nrep", "fused_ok", "chain_ok", "chain_pair", "carry_ok", "shuf_inv", "obj_arith", "poll", "r_store_always", "seed",
             "NT4", "NCT", "upd_wps", "max_iter_kmeans")
LAST_FIELDS = ("path", "merged", "chain_tail", "carried", "write_next", "r_store", "close", "exchanges")      # hmx_get("round:last"), in this order
ROUND_FIELDS = LAST_FIELDS + ("p2p", "gen_blocks", "clear_sets", "clear_cur", "clear_next", "reduce_old", "cur_before", "next_before", "sets_clean_before")
HEAD_FIELDS = ("gather", "fused_norm", "files", "clear_first", "r_store")
HEAD, ROUND, ROUND_REF, RESTART, SEED, RESORT = range(6)
CHAIN, FOLD_PROLOGUE, STEP_LOOP = range(3)                                       # RoundPlan::path
CHAIN_TAIL, WIDE_CLEAR_TAIL, TAIL, REDUCE_SNAPSHOT = range(4)                    # RoundPlan::close
P2P_CAP = 65536
WINDOW = 3                                                                       # window_size of the reference's convergence check
_probe = []


def round_probe():
    if not _probe:
        import tempfile
        so = os.path.join(tempfile.mkdtemp(prefix="round_probe_"), "round_probe.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "round_probe.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.probe_round_script.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_longlong)]
        lib.probe_round_script.restype = None
        _probe.append(lib)
    return _probe[0]


def run(ops, **kw):
    """the rows of a script: a dict of HEAD_FIELDS / ROUND_FIELDS per HEAD / ROUND operation, None for the others.  Defaults: the headline shape on one GPU
    (K = 100, 20 levels, 20 blocks: chain, carry, sort-free shuffle)"""
    c = dict(sharded=0, inbox_ok=0, B=20, K=100, nb=20, nrep=4, fused_ok=1, chain_ok=1, chain_pair=0, carry_ok=1, shuf_inv=1, obj_arith=0, poll=0, r_store_always=0, seed=1,
             NT4=3, NCT=7, upd_wps=2, max_iter_kmeans=4)
    assert not set(kw) - set(c), kw
    c.update(kw)
    flat = [int(v) for op in ops for v in (tuple(op) + (0, 0, 0))[:4]]
    out = (C.c_longlong * (20 * len(ops)))()
    round_probe().probe_round_script((C.c_longlong * len(ROUND_CFG))(*[int(c[k]) for k in ROUND_CFG]), (C.c_longlong * len(flat))(*flat), len(ops), out)
    rows = []
    for i, op in enumerate(ops):
        names = HEAD_FIELDS if op[0] == HEAD else ROUND_FIELDS if op[0] == ROUND else None
        rows.append(dict(zip(names, out[20 * i:20 * i + len(names)])) if names else None)
    for r in rows:      # what every script must satisfy: a memset is asked for exactly where a table may hold something (state 0: all zero; 1 unknown, 2 filed)
        if r and "path" in r:
            assert r["clear_cur"] == int(not r["carried"] and r["cur_before"] != 0), r
            assert r["clear_next"] == int(r["write_next"] and r["next_before"] != 0), r
            assert r["clear_sets"] == int(not r["sets_clean_before"]), r
    return rows


def init_cluster(host_order=0):
    return [(HEAD, 0, host_order)]                   # hmx_init_cluster: head_pass(normalise = false)


def cluster(m, first_call, max_iter=None, host_rounds=(), head_host_order=0):
    """hmx_cluster running m rounds: the head unless this is the first call after init_cluster (objective_harmony has one entry), then per iteration
    last_round_hint = iter == max_iter_kmeans - 1 and round_may_be_last = last_round_hint || iter > window_size"""
    max_iter = m if max_iter is None else max_iter
    ops = [] if first_call else [(HEAD, 1, head_host_order)]
    for it in range(m):
        last = it == max_iter - 1
        ops.append((ROUND, int(last), int(last or it > WINDOW), int(it in host_rounds)))
    return ops


def rounds(rows):
    return [r for r in rows if r and "path" in r]


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in [k for k in os.environ if k.startswith("HMX_")]:
        monkeypatch.delenv(k)


# ---- ledger scripts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 9))
def test_call_of_m_rounds_carries_every_round_and_stores_the_last(m):
    """the figures tests/test_gpu_stage_spec.py asserts on hardware.  Round 0 finds the sums init_cluster's head filed (gather: carry on, no host order; its set is keyed
    by the next block), round i > 0 those round i - 1 filed (write_next = carry_ok && keyed by next && !last_round_hint: every round but the last): carried_rounds = m.
    r_store = 0 iff write_next && !round_may_be_last: iterations 0 .. m - 2 that are <= window_size = 3, i.e. min(m - 1, 4) of them."""
    rows = run(init_cluster() + cluster(m, True), max_iter_kmeans=m)
    assert rows[0] == dict(gather=1, fused_norm=0, files=1, clear_first=1, r_store=1)      # (both tables start in state 1, unknown: cleared; init's head stores its rows)
    r = rounds(rows)
    assert sum(x["carried"] for x in r) == m and sum(1 - x["r_store"] for x in r) == min(m - 1, 4)
    assert [x["r_store"] for x in r] == [0] * min(m - 1, 4) + [1] * (m - min(m - 1, 4)) and r[-1]["r_store"] == 1 and r[-1]["write_next"] == 0
    assert [x["write_next"] for x in r] == [1] * (m - 1) + [0]
    # one GPU on the chain: the folder closes every round and clears what the round consumed -- after round 0 no memset at all
    assert all(x["close"] == CHAIN_TAIL and x["path"] == CHAIN for x in r)
    # (round 0: the replica sets, and -- where it files, m > 1 -- the other table, both still in their initial unknown state)
    assert [(x["clear_sets"], x["clear_cur"], x["clear_next"]) for x in r] == [(1, 0, int(m > 1))] + [(0, 0, 0)] * (m - 1)


def test_second_call_continues_the_carry_only_through_its_head():
    # the last round of a call files nothing (last_round_hint); the next call's head (normalise) files the sums of the round that follows it and stores no R rows
    # (max_iter_kmeans >= 1, no poll, no HMX_R_STORE): that round is carried
    rows = run(init_cluster() + cluster(3, True) + cluster(3, False), max_iter_kmeans=3)
    assert rows[4] == dict(gather=1, fused_norm=1, files=1, clear_first=0, r_store=0)      # (the chain's tail left both tables zero: nothing to clear)
    assert [x["carried"] for x in rounds(rows)] == [1, 1, 1, 1, 1, 1]
    # a head that cannot gather (a host order is queued when it runs) files nothing: the round behind it sums its old contributions from R, the ones behind that are carried
    rows = run(init_cluster() + cluster(3, True) + cluster(3, False, head_host_order=1), max_iter_kmeans=3)
    assert rows[4] == dict(gather=0, fused_norm=1, files=0, clear_first=0, r_store=1)
    assert [x["carried"] for x in rounds(rows)] == [1, 1, 1, 0, 1, 1]
    assert rounds(rows)[3]["gen_blocks"] == 1 and rounds(rows)[3]["clear_cur"] == 0      # (sort-free shuffle: k_shuf_blocks first; the table is zero: no memset)
    # the fused normalisation of the head: rows of <= 64 PCs, <= 7 cluster tiles, not the 4-waves-per-SIMD kernels
    for kw, fused in ((dict(NT4=4, NCT=7, upd_wps=2), 1), (dict(NT4=5), 0), (dict(NCT=8), 0), (dict(upd_wps=4), 0)):
        assert run([(HEAD, 1, 0)], **kw)[0]["fused_norm"] == fused and run([(HEAD, 0, 0)], **kw)[0]["fused_norm"] == 0
    # the cluster head stores its rows when anything may read them
    for kw in (dict(poll=1), dict(r_store_always=1), dict(max_iter_kmeans=0), dict(carry_ok=0)):
        assert run([(HEAD, 1, 0)], **kw)[0]["r_store"] == 1, kw


def test_what_voids_the_carry_voids_it_for_exactly_those_rounds():
    four = lambda **kw: cluster(4, True, **kw)      # noqa: E731
    seq = lambda rows, k: [x[k] for x in rounds(rows)]      # noqa: E731
    base = run(init_cluster() + four())
    assert (seq(base, "carried"), seq(base, "write_next"), seq(base, "r_store")) == ([1, 1, 1, 1], [1, 1, 1, 0], [0, 0, 0, 1])
    # a changed seed between init_cluster and the call: the head's sums were filed for (round 0, old seed) -> round 0 sums from R (and clears the stale table: state 2),
    # its tiles are sorted anew under the new seed, keyed by the next block: it files round 1's sums
    rows = run(init_cluster() + [(SEED, 2)] + four())
    assert (seq(rows, "carried"), seq(rows, "clear_cur"), seq(rows, "write_next")) == ([0, 1, 1, 1], [1, 0, 0, 0], [1, 1, 1, 0])
    # ... before a later call: that call's head sorts and files under the new seed, nothing is lost
    assert seq(run(init_cluster() + four() + [(SEED, 2)] + cluster(2, False)), "carried") == [1] * 6
    # hmx_restart: filed sums are void and no set counts as sorted; init_cluster's head sorts and files again (clearing the table: state 1)
    rows = run(init_cluster() + [(RESTART,)] + init_cluster() + four())
    assert rows[2] == dict(gather=1, fused_norm=0, files=1, clear_first=1, r_store=1) and seq(rows, "carried") == [1, 1, 1, 1]
    # a round of update_R_ref rewrites R outside the tables: the sums filed for the round behind it are void (state 2 -> 1: cleared, summed from R)
    rows = run(init_cluster() + [(ROUND_REF,)] + four())
    assert (seq(rows, "carried"), seq(rows, "clear_cur"), seq(rows, "clear_sets")) == ([0, 1, 1, 1], [1, 0, 0, 0], [1, 0, 0, 0])
    # a host-injected order for iteration 1: its set is not the order of (round, seed) -> not carried although round 0 filed its sums (cleared: state 2); its D.blk came
    # with the order (no k_shuf_blocks); keyed by the block alone -> it files nothing and stores its rows; iteration 2 finds nothing filed and generates its block ids
    rows = run(init_cluster() + four(host_rounds=(1,)))
    assert (seq(rows, "carried"), seq(rows, "write_next"), seq(rows, "r_store")) == ([1, 0, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1])
    assert (seq(rows, "gen_blocks"), seq(rows, "clear_cur")) == ([0, 0, 1, 0], [0, 1, 0, 0])
    # ... for the first round: the head of init_cluster does not gather while the order is queued
    rows = run(init_cluster(host_order=1) + four(host_rounds=(0,)))
    assert rows[0]["files"] == 0 and (seq(rows, "carried"), seq(rows, "r_store"), seq(rows, "gen_blocks")) == ([0, 0, 1, 1], [1, 0, 0, 1], [0, 1, 0, 0])
    # round 1's set sorted again without next-block keys: round 1 is still carried (same permutation), files nothing and stores; round 2 sums from R
    rows = run(init_cluster() + four()[:1] + [(RESORT, 1, 0)] + four()[1:])
    assert (seq(rows, "carried"), seq(rows, "write_next"), seq(rows, "r_store")) == ([1, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1])


@pytest.mark.parametrize("kw", [dict(poll=1), dict(r_store_always=1), dict(obj_arith=1), dict(carry_ok=0, shuf_inv=0)])
def test_every_round_stores_its_rows(kw):
    # r_store = (write_next && !round_may_be_last && !poll && !r_store_always && !obj_arith) ? 0 : 1; without the carry nothing is filed (write_next = 0) or carried
    r = rounds(run(init_cluster() + cluster(6, True), **kw))
    assert [x["r_store"] for x in r] == [1] * 6
    assert [x["carried"] for x in r] == ([0] * 6 if "carry_ok" in kw else [1] * 6)


def test_tables_that_no_launch_cleared_are_cleared_up_front():
    # sharded without inboxes: reduce + snapshot closes the round, nothing clears the tables -> the replica sets every round, the table that files the next round's sums
    # (state 1 after the round that consumed it) every round that files; the carried table itself never
    r = rounds(run(init_cluster() + cluster(4, True), sharded=1))
    assert all(x["close"] == REDUCE_SNAPSHOT and x["reduce_old"] == 1 for x in r) and [x["carried"] for x in r] == [1] * 4
    assert [(x["clear_sets"], x["clear_cur"], x["clear_next"]) for x in r] == [(1, 0, 1)] * 3 + [(1, 0, 0)]
    # ... and without the carry: the consumed table (state 1) before every pass over R
    r = rounds(run(init_cluster() + cluster(3, True), sharded=1, carry_ok=0, shuf_inv=0))
    assert [(x["clear_sets"], x["clear_cur"], x["clear_next"], x["gen_blocks"]) for x in r] == [(1, 1, 0, 0)] * 3


# ---- path table ----------------------------------------------------------------------------------------------------------------------------------
def one_round(**kw):
    return rounds(run(init_cluster() + cluster(1, True), **kw))[0]


def test_merged_fold_thresholds_and_both_switch_values(monkeypatch):
    # merged = B * 128 <= 64 KB (k_foldpen's LDS) && !split && (fused_ok || B * K <= 8192 || "merged")
    assert [one_round(B=B, K=16, chain_ok=0)["merged"] for B in (512, 513)] == [1, 0]
    assert [one_round(B=B, K=K, fused_ok=0, chain_ok=0)["merged"] for B, K in ((64, 128), (1, 8193), (8193, 1))] == [1, 0, 0]
    # off the chain: fold in the prologue where fused_ok, else the step loop -- merged (k_foldpen) or not (k_fold + k_penalty)
    assert [one_round(chain_ok=0, fused_ok=f)["path"] for f in (1, 0)] == [FOLD_PROLOGUE, STEP_LOOP]
    monkeypatch.setenv("HMX_FOLD_IMPL", "split")
    assert [(r["merged"], r["path"]) for r in (one_round(), one_round(chain_ok=0), one_round(chain_pair=1, chain_ok=0))] == [(0, STEP_LOOP), (0, STEP_LOOP), (0, CHAIN)]
    monkeypatch.setenv("HMX_FOLD_IMPL", "merged")
    assert [one_round(B=B, K=K, fused_ok=0, chain_ok=0)["merged"] for B, K in ((1, 8193), (513, 16))] == [1, 0]


def test_chain_needs_the_inboxes_when_sharded():
    # chain_path = ((merged && fused_ok && chain_ok) || chain_pair) && (!sharded || p2p); p2p = sharded && inboxes usable && B * K <= P2P_CAP
    one, off, on = one_round(), one_round(sharded=1), one_round(sharded=1, inbox_ok=1)
    assert (one["path"], one["p2p"], one["reduce_old"], one["exchanges"], one["close"]) == (CHAIN, 0, 1, 0, CHAIN_TAIL)
    assert (off["path"], off["p2p"], off["reduce_old"], off["exchanges"], off["close"]) == (FOLD_PROLOGUE, 0, 1, 0, REDUCE_SNAPSHOT)
    # the p2p chain's folder exchanges the old sums itself; exchanges: nb + 1 block steps + the objective's
    assert (on["path"], on["p2p"], on["reduce_old"], on["exchanges"], on["chain_tail"], on["close"]) == (CHAIN, 1, 0, 22, 1, CHAIN_TAIL)
    assert one_round(inbox_ok=1)["p2p"] == 0                                     # (one rank: nobody to exchange with)
    # B * K = P2P_CAP against P2P_CAP + 1 (the pair chain: K = 256 x 256 levels)
    cap = [one_round(sharded=1, inbox_ok=1, chain_ok=0, fused_ok=0, chain_pair=1, B=256, K=K) for K in (256, 257)]
    assert [(r["p2p"], r["path"]) for r in cap] == [(1, CHAIN), (0, STEP_LOOP)] and 256 * 256 == P2P_CAP
    assert [(r["exchanges"], r["chain_tail"], r["close"]) for r in cap] == [(21, 0, REDUCE_SNAPSHOT), (0, 0, REDUCE_SNAPSHOT)]


def test_chain_tail():
    # chain_tail = (!sharded || (p2p && B * K + 2 <= P2P_CAP && nb <= 62)) && !obj_arith && !chain_pair, on the chain only
    sh = dict(sharded=1, inbox_ok=1, B=1)
    got = [(r["path"], r["chain_tail"], r["exchanges"], r["close"]) for r in (one_round(K=P2P_CAP - 2, nb=62, **sh), one_round(K=P2P_CAP - 1, nb=62, **sh), one_round(K=P2P_CAP - 2, nb=63, **sh))]
    assert got == [(CHAIN, 1, 64, CHAIN_TAIL), (CHAIN, 0, 63, REDUCE_SNAPSHOT), (CHAIN, 0, 64, REDUCE_SNAPSHOT)]
    assert one_round(nb=63)["chain_tail"] == 1                                   # (one GPU: no exchange to fit)
    # obj_arith: the objective is summed from R behind the chain; the pair chain: several folders, k_round_tail closes
    assert [(r["path"], r["chain_tail"], r["close"]) for r in (one_round(obj_arith=1), one_round(chain_pair=1, chain_ok=0, fused_ok=0, B=200, K=200, nrep=1))] == \
        [(CHAIN, 0, REDUCE_SNAPSHOT), (CHAIN, 0, WIDE_CLEAR_TAIL)]
    assert one_round(chain_ok=0)["chain_tail"] == 0


def test_closing_form_on_both_sides_of_2_to_the_18_entries():
    # off the chain tail, one GPU: k_round_tail clears nb * B * K + 3 * nrep * B * K entries itself up to 2^18; (20 + 3 * 4) * 8192 = 2^18 exactly
    assert [one_round(chain_ok=0, B=1, K=K, nb=20, nrep=4)["close"] for K in (8192, 8193)] == [TAIL, WIDE_CLEAR_TAIL] and 32 * 8192 == 1 << 18
    assert [one_round(chain_ok=0, fused_ok=0, B=64, K=128, nb=nb, nrep=4)["close"] for nb in (20, 21)] == [TAIL, WIDE_CLEAR_TAIL]
    assert one_round(chain_ok=0, sharded=1)["close"] == REDUCE_SNAPSHOT and one_round(chain_ok=0, obj_arith=1)["close"] == REDUCE_SNAPSHOT
