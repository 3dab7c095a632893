"""The plan tests/test_plan_cpu.py checks on the CPU IS the plan the library runs: for shapes the suite sets up elsewhere, the path flags of a
live handle equal what the probe of harmony_amd/csrc/hmx_plan.h returns for the same shape and the device's real CU count -- and every k_tile
launch the handle then makes, and every launch of the ridge correction behind them (hmx_get "launch:<kind>"), is, field by field, the launch the
probe plans for it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from harmony_amd import Harmony, HarmonyError, prepare_setup_args  # noqa: E402
from helpers import synth  # noqa: E402
from test_plan_cpu import LAUNCH_FIELDS, RIDGE_FIELDS, plan, ridge_launch, tile_launch  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {                               # N, d, levels, K, sigma[, environment]
    "uniform_K50": (30000, 50, (2,), 50, 0.1),
    "uniform_K100": (300000, 50, (10,), 100, 0.1),      # (20^2 blocks x 10 combinations x 64 <= N: old contributions carried, sort-free shuffle)
    "K200_three_covariates": (120000, 50, (4, 10, 20), 200, 0.1),
    "K_not_multiple_of_4": (20000, 30, (5,), 50 + 1, 0.1),
    "sigma_vector": (6000, 30, (4,), 40, "vector"),
    "d68": (20000, 68, (4,), 100, 0.1),                 # (rows of 68 PCs: the split-bf16 form is not offered, every launch is of the fp32 build)
    "uniform_K100_dot_f32": (300000, 50, (10,), 100, 0.1, {"HMX_DOT": "f32"}),
    # the correction's branches the cases above miss: five waves x 8 cluster tiles of fp64 shadows do not fit LDS twice (slot statistics without them);
    # 1100 levels: the right-hand sides stay outside LDS, body = the Cholesky panel, 1024 threads (tests/test_gpu_stage_spec.py: h_device_1100)
    "d64_K128_no_lds_shadows": (20000, 64, (4,), 128, 0.1),
    "levels_1100_device_solve": (60000, 30, (1100,), 40, 0.1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_live_handle_runs_the_probed_plan(name, monkeypatch):
    for k in [k for k in os.environ if k.startswith("HMX_")]:
        monkeypatch.delenv(k)
    N, d, levels, K, sigma = CASES[name][:5]
    for k, v in (CASES[name][5] if len(CASES[name]) > 5 else {}).items():
        monkeypatch.setenv(k, v)
    Z, meta, _ = synth(N, d=d, levels=levels, seed=7)
    skw, _ = prepare_setup_args(Z, meta, list(meta), nclust=K, sigma=np.linspace(0.08, 0.16, K) if sigma == "vector" else sigma)
    skw["max_iter_kmeans"] = 2
    h = Harmony(seed=1)
    h.setup(**skw)                      # (no HMX_CHAIN_WGS: the chain's workgroup count "chain_wgs" is the device's CU count)
    phi_i, phi_p, _, B = skw["Phi"]
    C_ = len(levels)
    combos, counts = np.unique(np.asarray(phi_i).reshape(N, C_), axis=0, return_counts=True)      # (one level per covariate and cell, grouped by covariate)
    cus = int(h._scalar("chain_wgs"))
    shape = dict(d=d, B=int(B), C_=C_, Q=len(combos), nb=int(h._scalar("n_blocks")), cells_per_block=int(h._scalar("cells_per_block")),
                 cus=cus, usig=int(sigma != "vector"), ntitems=int(((counts + 15) // 16).sum()))
    p = plan(N, K, **shape)
    live = {g: int(h._scalar(g)) for g in ("chain", "chain_pair", "dot_bf", "sold_carry", "shuffle_inv", "usig", "upd_wps")}
    want = {"chain": int(p["chain_ok"] or p["chain_pair"]), "chain_pair": p["chain_pair"], "dot_bf": p["dot_bf"], "sold_carry": p["carry_ok"],
            "shuffle_inv": p["shuf_inv"], "usig": p["usig"], "upd_wps": p["upd_wps"]}
    print("PLAN", name, live)
    assert live == want, (name, live, p)

    def ran(kind):
        """the handle's last launch of a kind, or None where it made none"""
        try:
            return dict(zip(LAUNCH_FIELDS, (int(v) for v in h._get("launch:" + kind))))
        except HarmonyError:
            return None

    assert all(ran(k) is None for k in ("head", "seed", "lloyd", "update", "chain")), "nothing is launched before init_cluster"
    h.init_cluster_cpp()                # seeding race, ten Lloyd iterations, head
    h.cluster_cpp()                     # head, two rounds
    rounds = int(h._get("kmeans_rounds")[-1])
    # what is set per launch, from the handle's own counters: the last round's launches stored their R rows unless every round of the call went
    # without (the call's last round always stores); the fold is in the prologue of the chain, and of the update where the plan's path says so
    r_store = 0 if int(h._scalar("rounds_without_R")) >= rounds else 1
    on_chain = int(h._scalar("chain"))
    got = {k: ran(k) for k in ("head", "seed", "lloyd", "update", "chain")}
    print("LAUNCH", name, {"rounds": rounds, "rounds_without_R": int(h._scalar("rounds_without_R")), "r_store": r_store}, got)
    for kind in ("head", "seed", "lloyd", "update", "chain"):
        t = tile_launch(kind, N, K, workgroups=cus, r_store=r_store, **shape)
        runs = t.pop("ran") and kind != ("update" if on_chain else "chain")
        assert got[kind] == (t if runs else None), (name, kind, got[kind], t)
    assert got["head"] and got["seed"] and (got["chain"] if on_chain else got["update"]), (name, got)

    # the ridge correction behind the clustering call: statistics, device solve, apply
    def ridge_ran(kind):
        try:
            return dict(zip(RIDGE_FIELDS, (int(v) for v in h._get("launch:" + kind))))
        except HarmonyError:
            return None

    assert all(ridge_ran(k) is None for k in ("stats", "solve", "apply")), "no launch of the correction before moe_correct_ridge_cpp"
    h.moe_correct_ridge_cpp()
    items = dict(nitems=int(((counts + 255) // 256).sum()), naitems=int(((counts + 1023) // 1024).sum()))      # static work lists: <= 256 / <= 1024 cells of one combination
    rgot = {k: ridge_ran(k) for k in ("stats", "solve", "apply")}
    print("RIDGE", name, rgot)
    for kind in ("stats", "solve", "apply"):
        t = ridge_launch(kind, N, K, **items, **shape)
        assert t.pop("solve_on_device") == 1 and t["valid"] == 1, (name, kind, t)
        assert rgot[kind] == t, (name, kind, rgot[kind], t)
    want_form = {"d64_K128_no_lds_shadows": ("stats", dict(mfma=1, p0=8, p1=0, threads=320, lds=0)),
                 "levels_1100_device_solve": ("solve", dict(threads=1024, lds_b_bytes=0, lds_body_bytes=1101 * 128, lds=158552)),
                 "K200_three_covariates": ("stats", dict(mfma=1, gy=2, p0=7)), "K_not_multiple_of_4": ("stats", dict(mfma=0)), "d68": ("apply", dict(mfma=0, p1=2))}
    if name in want_form:               # the branch the case is here for
        kind, fields = want_form[name]
        assert {k: rgot[kind][k] for k in fields} == fields, (name, rgot[kind])


# ---- the round plan (harmony_amd/csrc/hmx_round.h): what the handle's last round decided is what the CPU probe plans for it ---------------------------
ROUND_ENVS = {                          # environment, the path it claims: (RoundPlan::path, merged)
    "chain": ({}, (0, 1)),
    "fold_in_prologue": ({"HMX_CHAIN": "0"}, (1, 1)),
    "merged_step_loop": ({"HMX_CHAIN": "0", "HMX_FUSED_FOLD": "0"}, (2, 1)),
    "two_kernel_step_loop": ({"HMX_CHAIN": "0", "HMX_FOLD_IMPL": "split"}, (2, 0)),
    "chain_pushed_first_order": ({}, (0, 1)),
}


@pytest.mark.parametrize("name", sorted(ROUND_ENVS))
def test_live_handle_runs_the_probed_round_plan(name, monkeypatch):
    """6000 cells, d = 30, 4 levels, K = 40, up to 6 rounds with the carry forced on: hmx_get("round:last") and the handle's counters against the script
    tests/test_round_cpu.py drives through the probe for the same switches -- init_cluster's head, then the m rounds the call really ran."""
    from test_round_cpu import LAST_FIELDS, cluster, init_cluster, rounds, run
    for k in [k for k in os.environ if k.startswith("HMX_")]:
        monkeypatch.delenv(k)
    env, (path, merged) = ROUND_ENVS[name]
    monkeypatch.setenv("HMX_SOLD_CARRY", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pushed = name.endswith("pushed_first_order")
    N, d, K = 6000, 30, 40
    Z, meta, _ = synth(N, d=d, levels=(4,), seed=7)
    skw, _ = prepare_setup_args(Z, meta, list(meta), nclust=K, sigma=0.1)

    def fit(max_iter):
        skw["max_iter_kmeans"] = max_iter
        h = Harmony(seed=1)
        h.setup(**skw)
        if pushed:                      # queued before init_cluster: its head cannot gather, round 0 takes the order
            h.push_update_order(np.random.default_rng(3).permutation(N))
        h.init_cluster_cpp()
        h.cluster_cpp()
        return h

    h = fit(6)
    m = int(h._get("kmeans_rounds")[-1])
    phi_i, _, _, B = skw["Phi"]
    combos, counts = np.unique(np.asarray(phi_i).reshape(N, 1), axis=0, return_counts=True)
    p = plan(N, K, d=d, B=int(B), C_=1, Q=len(combos), nb=int(h._scalar("n_blocks")), cells_per_block=int(h._scalar("cells_per_block")), cus=int(h._scalar("chain_wgs")),
             usig=1, ntitems=int(((counts + 15) // 16).sum()))
    cfg = dict(B=int(B), K=K, nb=int(h._scalar("n_blocks")), nrep=p["nrep"], fused_ok=p["fused_ok"], chain_ok=p["chain_ok"], chain_pair=p["chain_pair"], carry_ok=p["carry_ok"],
               shuf_inv=p["shuf_inv"], seed=1, NT4=p["NT4"], NCT=p["NCT"], upd_wps=p["upd_wps"])

    def script(rounds_run, max_iter):
        return rounds(run(init_cluster(host_order=int(pushed)) + cluster(rounds_run, True, max_iter=max_iter, host_rounds=(0,) if pushed else ()), max_iter_kmeans=max_iter, **cfg))

    want = script(m, 6)
    live = dict(zip(LAST_FIELDS, (int(v) for v in h._get("round:last"))))
    counters = {g: int(h._scalar(g)) for g in ("carried_rounds", "rounds_without_R", "chain_rounds", "sold_carry")}
    print("ROUND", name, {"m": m, "live": live, "counters": counters})
    assert counters["sold_carry"] == 1 and 5 <= m <= 6, (name, m, counters)
    assert live == {k: want[-1][k] for k in LAST_FIELDS}, (name, live, want[-1])
    assert (live["path"], live["merged"]) == (path, merged), (name, live)
    assert counters["chain_rounds"] == (m if path == 0 else 0), (name, counters)
    if not pushed:
        assert counters["carried_rounds"] == m and counters["rounds_without_R"] == min(m - 1, 4), (name, m, counters)
        return
    # the pushed order is round 0's: not carried, rows stored (its tiles are keyed by the block alone: it files nothing); round 1 finds nothing filed either
    assert (want[0]["carried"], want[0]["r_store"], want[1]["carried"]) == (0, 1, 0)
    assert counters["carried_rounds"] == sum(r["carried"] for r in want) == m - 2, (name, m, counters)
    assert counters["rounds_without_R"] == sum(1 - r["r_store"] for r in want), (name, m, counters)
    h1 = fit(1)                         # the same first round as a call's only one: its plan, read back
    first = dict(zip(LAST_FIELDS, (int(v) for v in h1._get("round:last"))))
    assert first == {k: script(1, 1)[0][k] for k in LAST_FIELDS} and (first["carried"], first["r_store"]) == (0, 1), (name, first)
    assert (int(h1._scalar("carried_rounds")), int(h1._scalar("rounds_without_R"))) == (0, 0)
