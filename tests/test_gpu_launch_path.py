"""The launch diet of a harmony iteration (events per call instead of per round, clears that follow the ledger, no objective partials from cluster_cpp's
head, k_moe_solve's systems in LDS) changes no result: every run below is compared BIT FOR BIT with a run that takes
the global-scratch solve (HMX_SOLVE_LDS=0), with the same run issued from two handles on two streams, and with the same run whose host asks for
the objective after every call.  The launch and event-record counts of an iteration are pinned per path.

Shapes (the smallest that take each path): 4000 cells x 50 PCs, K = 100, 10 levels with the carry forced on (the flagship's path: block chain whose folder closes
the round, carried old contributions, slot-form statistics, 11-row systems in LDS); 6000 x 50, K = 200, 8 > 64 > 128 nested levels (wave-pair chain, k_round_tail
behind a wide clear, the general Cholesky with its systems in the global scratch); 6000 x 50, K = 100, 8 > 16 > 32 nested levels (57-row systems IN LDS behind the
coupling masks: Schur step, blocked Cholesky, substitution); 4000 x 50, K = 99 (first-generation statistics: Sq / nq must still be cleared); the flagship's shape
with one level shifted far away from the others and a level of 40 cells in one corner (subset AND skipped clusters).

The arrays (Z_corr, R, Y, O, E, W) and the rounds per call are compared in the three tests of the paths; the objective series, bit for bit as well, in
test_objective_series_bit_for_bit.  THAT TEST FAILS NOW AND THEN, AND DID BEFORE THIS CHANGE: the order of the cells inside a (block, combination) bin of a
round's shuffle is unspecified (atomic ranks; DESIGN 4.5 -- the fixed-point tables do not depend on it, and neither do Z_corr, R, Y, O, E, W), while the two
per-cell objective terms are fp64 sums per wave in tile order.  Their last bits differ from run to run, and where a round's total lies next to an fp32 rounding
boundary the reported value moves by one ulp.  Measured on one MI355X on the flagship case here (seed 1): on the PARENT commit 12 of 250 solo runs, and 2 of 80
in a second batch, differed from the first run -- always in entry 12 of objective_kmeans alone, 290.52679 against 290.52676, with the dist / entropy / cross
series equal --, two alternating handles 1 of 160 on the parent and 1 of 160 on this change; this file failed that way in 1 of 12 runs.  Any case whose series
holds such a value can be hit: the small_level case was, once, in entry 11 (350.05634 against 350.05637, global-scratch run against the default run, every array
equal).  Nothing but one entry of objective_kmeans (and objective_harmony where it is a call's last) ever differed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harmony_amd import Harmony, prepare_setup_args  # noqa: E402
from helpers import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ITERS = 3
ARRAYS = ("Z_corr", "R", "Y", "O", "E", "W", "kmeans_rounds")
SERIES = ("objective_kmeans", "objective_harmony")
FIELDS = ARRAYS + SERIES


def _data(name):
    if name == "nested_K200":
        Z, meta, _ = synth(6000, d=50, levels=(8, 64, 128), seed=11, nested=True)
        return Z, meta, 200
    if name == "nested_K100":
        Z, meta, _ = synth(6000, d=50, levels=(8, 16, 32), seed=11, nested=True)
        return Z, meta, 100
    Z, meta, _ = synth(4000, d=50, levels=(10,), seed=11)
    if name == "small_level":
        lev = np.random.default_rng(5).integers(0, 6, Z.shape[0])
        lev[np.argsort(Z[:, 0])[-40:]] = 7        # a small level in one corner: below the cutoff in the clusters far from it
        far = np.argsort(Z[:, 1])[:400]
        lev[far] = 6                              # ... and a level of its own far from all others: the clusters that settle on it hold no second level
        Z = Z.copy()
        Z[far, 49] += 1000.0                      # (along the PC of the smallest spread: the other cells' rows are all but orthogonal to that direction)
        meta = {"cov0": lev}
    return Z, meta, 99 if name == "K99" else 100


# environment of a shape, and per iteration WITH a head (the second call onwards) the kernel launches and the event records.
#   flagship / small_level: head tiles + k_fold (no clearing launch, no objective reduction) 2, the sort-free shuffle of the call's four rounds 3, four chain
#     launches 4 (carried: no pass over R; the folder closes the round), statistics + k_moe_stats_reduce + solve + apply 4
#   nested_K200 (no carry at this size): k_normalize4 + head 3 (13 cluster tiles: the head does not normalise in registers), counting sort of four rounds 4, per round k_oldsum + chain + wide clear + k_round_tail 16, correction 4
#   nested_K100 (no carry): head 2, counting sort 4, per round k_oldsum + chain 8 (the folder closes the round), correction 4
#   K99 (no carry): head 2, counting sort 4, per round k_oldsum + chain 8, correction k_zero4 + first-generation statistics + solve + apply 4
# one event record per call: obj_event at the end of hmx_cluster.  Last: the design's levels (the solve's systems have 1 + levels rows).
CASES = {
    "flagship": ({"HMX_SOLD_CARRY": "1"}, 13, 1, 10),
    "nested_K200": ({}, 27, 1, 200),
    "nested_K100": ({}, 18, 1, 56),
    "K99": ({}, 18, 1, 10),
    "small_level": ({"HMX_SOLD_CARRY": "1"}, 13, 1, 8),
}


def _setup(name, seed):
    Z, meta, K = _data(name)
    # (small_level: sigma 0.05 -- a cell 1.77 away in cosine distance from the far level's clusters weighs < e^-29 there, whatever the diversity penalty adds: those clusters are skipped)
    skw, _ = prepare_setup_args(Z, meta, list(meta), nclust=K, sigma=0.05 if name == "small_level" else 0.1)
    skw["max_iter_kmeans"] = 4
    h = Harmony(seed=seed)
    h.setup(**skw)
    return h


def _results(h):
    out = {"Z_corr": h.getZcorr(), "R": h.getR()}
    for f in FIELDS[2:]:
        out[f] = np.array(h._get(f))
    return out


def _solo(name, seed, poll=False):
    """ITERS harmony iterations; poll: the host asks for the convergence verdict and the objective series after every call"""
    h = _setup(name, seed)
    h.init_cluster_cpp()
    counts, polled = [], []
    for it in range(ITERS):
        c0 = (h._scalar("diag:launches"), h._scalar("diag:event_records") - h._scalar("diag:gate_records"))
        h.cluster_cpp()
        if poll:
            polled.append((h.check_convergence(1), np.array(h._get("objective_kmeans"))))
        h.moe_correct_ridge_cpp()
        if poll:
            polled.append(np.array(h._get("objective_kmeans")))
        # (the chain gate's records depend on which stream of the PROCESS launched a chain last -- an earlier test's handle may still own the gate: counted apart)
        counts.append((int(h._scalar("diag:launches") - c0[0]), int(h._scalar("diag:event_records") - h._scalar("diag:gate_records") - c0[1])))
    info = {"counts": counts, "solve": [int(v) for v in h._get("launch:solve")], "chain": int(h._scalar("chain")), "chain_pair": int(h._scalar("chain_pair")),
            "carry": int(h._scalar("sold_carry")), "moe_mfma": int(h._scalar("moe_mfma")), "round": [int(v) for v in h._get("round:last")],
            "subset": int(h._scalar("subset_clusters")), "skipped": int(h._scalar("skipped_clusters")), "polled": polled}
    return _results(h), info


def _same(a, b, what, fields=ARRAYS):
    for f in fields:
        assert a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), (what, f, float(np.abs(a[f].astype(np.float64) - b[f].astype(np.float64)).max()) if a[f].shape == b[f].shape else "shape")


_base, _others = {}, {}


def _baseline(name, monkeypatch):
    """the default run of a shape with seed 1 (computed once, shared by the tests of the shape, never changed)"""
    for k in [k for k in os.environ if k.startswith("HMX_")]:
        monkeypatch.delenv(k)
    for k, v in CASES[name][0].items():
        monkeypatch.setenv(k, v)
    if name not in _base:
        _base[name] = _solo(name, 1)
    return _base[name]


def _other(name, kind, monkeypatch):
    """the runs a shape's baseline is compared with (computed once each): "global" HMX_SOLVE_LDS=0, "seed2" the solo run of seed 2, "pair" two handles
    alternating, "polled" the host asks after every call"""
    _baseline(name, monkeypatch)
    key = (name, kind)
    if key in _others:
        return _others[key]
    if kind == "global":
        monkeypatch.setenv("HMX_SOLVE_LDS", "0")
        _others[key] = _solo(name, 1)
        monkeypatch.delenv("HMX_SOLVE_LDS")
    elif kind == "seed2":
        _others[key] = _solo(name, 2)
    elif kind == "polled":
        _others[key] = _solo(name, 1, poll=True)
    else:
        ha, hb = _setup(name, 1), _setup(name, 2)
        ha.init_cluster_cpp()
        hb.init_cluster_cpp()
        g0 = ha._scalar("diag:gate_records") + hb._scalar("diag:gate_records")
        e0 = ha._scalar("diag:event_records") + hb._scalar("diag:event_records")
        for it in range(ITERS):
            ha.cluster_cpp()
            hb.cluster_cpp()
            ha.moe_correct_ridge_cpp()
            hb.moe_correct_ridge_cpp()
        gate = int(ha._scalar("diag:gate_records") + hb._scalar("diag:gate_records") - g0)
        events = int(ha._scalar("diag:event_records") + hb._scalar("diag:event_records") - e0)
        ra, rb = _results(ha), _results(hb)
        del ha
        _others[key] = (ra, rb, _results(hb), gate, events)
    return _others[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_lds_and_global_scratch_solves_agree_bit_for_bit_and_counts(name, monkeypatch):
    res, info = _baseline(name, monkeypatch)
    print("LAUNCH PATH", name, {k: v for k, v in info.items() if k != "polled"})
    _, launches, events, B = CASES[name]
    # the path the case is here for
    assert info["chain"] == 1 and info["moe_mfma"] == int(name != "K99")
    assert info["chain_pair"] == int(name == "nested_K200") and info["carry"] == int(name in ("flagship", "small_level"))
    assert info["round"][0] == 0 and info["round"][2] == int(name != "nested_K200")           # chain; its folder closes the round unless it is the wave-pair chain
    sys_off, lds_total = info["solve"][14:16]
    in_lds = name != "nested_K200"          # 201 rows: 201 x 251 doubles do not fit
    assert (sys_off > 0) == in_lds and sys_off == (((info["solve"][8] + 7) & ~7) if in_lds else 0)
    assert lds_total == (sys_off + (B + 1) * (B + 1 + 50) * 8 if in_lds else info["solve"][8])
    if name == "nested_K100":
        assert info["solve"][11] > 0          # the coupling masks of the Schur complement, in front of the systems
    if name == "small_level":
        assert info["subset"] > 0 and info["skipped"] > 0, (info["subset"], info["skipped"])
    # d. the diet: launches and event records of the iterations that start with a head
    assert info["counts"][1:] == [(launches, events)] * (ITERS - 1), info["counts"]
    # (the first call has no head; with the carry init_cluster's head already sorted its rounds, without it the first round does)
    assert info["counts"][0] == (launches - (3 if name == "nested_K200" else 2) - (3 if info["carry"] else 0), events), info["counts"]
    # a. the global-scratch solve
    res0, info0 = _other(name, "global", monkeypatch)
    assert info0["solve"][14:16] == [0, info0["solve"][8]]
    assert info0["counts"] == info["counts"], info0["counts"]
    _same(res, res0, "HMX_SOLVE_LDS=0")


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_handles_on_two_streams_equal_two_solo_runs(name, monkeypatch):
    """every handle has a stream of its own: alternating calls hand the chain gate from one stream to the other at every call"""
    res1, _ = _baseline(name, monkeypatch)
    res2, _ = _other(name, "seed2", monkeypatch)
    ra, rb, rb_alone, gate, events = _other(name, "pair", monkeypatch)
    # per call one objective record and one record of the gate's event on the stream that owned it -- but for the pair's very first chain launch if nobody
    # owned the process' gate then (an earlier test's handle may have)
    assert events - gate == 2 * ITERS and 2 * ITERS - 1 <= gate <= 2 * ITERS, (events, gate)
    _same(res1, ra, "handle a")
    _same(res2, rb, "handle b")
    _same(res2, rb_alone, "handle b after its neighbour is gone")


@pytest.mark.parametrize("name", sorted(CASES))
def test_asking_after_every_call_returns_the_same_series(name, monkeypatch):
    res, _ = _baseline(name, monkeypatch)
    resp, infop = _other(name, "polled", monkeypatch)
    _same(res, resp, "polled")
    series = resp["objective_kmeans"]
    for it in range(ITERS):      # what the host saw after call it + 1 and after the correction behind it: the series up to that call, as the same handle returns it at the end
        (conv, after_call), after_moe = infop["polled"][2 * it], infop["polled"][2 * it + 1]
        n = 1 + 4 * (it + 1)
        assert np.array_equal(after_call, series[:n]) and np.array_equal(after_moe, series[:n]), (it, after_call, series[:n])
        oh = resp["objective_harmony"].astype(np.float32)      # the verdict: the reference's rule (src/harmony.cpp:197-201) on the values of this call and the one before, in fp32
        assert conv == bool((oh[it] - oh[it + 1]) / np.abs(oh[it]) < np.float32(1e-2)), (it, conv, oh)
    # no record more for the polls: the call recorded its event once, the getters wait for it
    assert [c[1] for c in infop["counts"]] == [1] * ITERS, infop["counts"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_objective_series_bit_for_bit(name, monkeypatch):
    """the objective series of the same runs: global-scratch solve, two handles, polled host -- all against the solo runs, bit for bit.  Fails now and then where a
    round's total lies next to an fp32 rounding boundary (the module's docstring has the cause and the figures: the flagship case's entry 12 in about one solo run
    in twenty on the parent commit already, the small_level case's entry 11)."""
    res1, _ = _baseline(name, monkeypatch)
    _same(res1, _other(name, "global", monkeypatch)[0], "HMX_SOLVE_LDS=0", SERIES)
    _same(res1, _other(name, "polled", monkeypatch)[0], "polled", SERIES)
    res2, _ = _other(name, "seed2", monkeypatch)
    ra, rb, rb_alone = _other(name, "pair", monkeypatch)[:3]
    _same(res1, ra, "handle a", SERIES)
    _same(res2, rb, "handle b", SERIES)
    _same(res2, rb_alone, "handle b after its neighbour is gone", SERIES)
