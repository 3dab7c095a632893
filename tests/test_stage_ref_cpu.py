"""The fp64 stage spec (tests/stage_ref.py) anchored to the CPU oracle, stage by stage, at the oracle's fp32 level; and the spec's streamed
forms (prefix sums over blocks, per-combination sums) against its direct per-cell forms."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stage_ref as ref  # noqa: E402
from harmony_amd import harmony_options, prepare_setup_args  # noqa: E402
from helpers import synth  # noqa: E402
from oracle.oracle import OracleHarmony  # noqa: E402
from oracle.oracle import feistel_order  # noqa: E402
from stage_check import phi_matrix, run_ladder, run_stages  # noqa: E402
import stage_lattice as lattice  # noqa: E402
import test_gpu_kmeans as gpu_kmeans  # noqa: E402
import test_gpu_stage_spec as gpu_spec  # noqa: E402
from test_gpu_stage_spec import LADDERS, LATTICE, SMALL_LADDERS, PLAN_CASES, _case, _ladder  # noqa: E402  (the GPU cases: their claims are checked here first)
from test_plan_cpu import plan  # noqa: E402

BAR = 1e-5      # the oracle keeps R, O, E, Z, Y in fp32


def _cases():
    small = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines_small.npz"))
    cl = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines.npz"))
    Zn, metan, _ = synth(1500, d=20, levels=(3, 6, 12), nested=True, seed=5)
    rng = np.random.default_rng(3)
    return {
        "cell_lines_small": (small["pcs"], {"dataset": small["dataset_levels"][small["dataset"]]}, "dataset", dict(nclust=10)),
        "cell_lines_two_covariates": (cl["pcs"], {"dataset": cl["dataset_levels"][cl["dataset"]],
                                                  "cell_type": cl["cell_type_levels"][cl["cell_type"]]},
                                      ["dataset", "cell_type"], dict(nclust=20)),
        # a raised cutoff: clusters drop levels (the subset path) and some lose every covariate (skipped)
        "nested_three_covariates": (Zn, metan, ["cov0", "cov1", "cov2"],
                                    dict(nclust=20, options=harmony_options(batch_prop_cutoff=0.05))),
        "fixed_lambda_sigma_vector": (cl["pcs"], {"dataset": cl["dataset_levels"][cl["dataset"]]}, "dataset",
                                      dict(nclust=15, lambda_=1.0, sigma=0.08 + 0.07 * rng.random(15), theta=3.0)),
    }


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_stages_match_the_spec(name):
    Z, meta, var, kw = CASES[name]
    _oracle_stages(name, Z, meta, var, kw)


def _oracle_stages(name, Z, meta, var, kw):
    skw, _ = prepare_setup_args(Z, meta, var, **kw)
    h = OracleHarmony(accurate=True, seed=1)
    h.setup(**skw)
    N, K = Z.shape[0], skw["K"]
    rng = np.random.default_rng(11)
    Y0 = skw["Z"][:, rng.choice(N, K, replace=False)]
    orders = [rng.permutation(N) for _ in range(2)]

    def order_of_round(r):
        h.push_update_order(orders[r])
        return orders[r]

    err, info = run_stages(h, skw, Y0, order_of_round)
    msg = repr((err, info))
    assert info["keep_margin"] >= 1e-3, msg
    for k in ("init_R", "round_R", "cold_R"):
        assert err[k] <= BAR, msg
    for k in ("init_argmax", "round_argmax", "cold_argmax"):
        assert err[k] == 0, msg
    for k in ("init_O", "init_E", "round_O", "round_E", "cold_O", "cold_E", "init_obj", "round_obj", "cold_obj", "stale_obj", "Z_rel", "Z_maxabs",
              "Y", "W", "Lambda"):
        assert err[k] <= BAR, (k, msg)
    assert (info["subset"], info["skipped"]) == (info["subset_h"], info["skipped_h"]), msg
    if name == "nested_three_covariates":
        assert info["subset"] > 0 and info["skipped"] > 0, msg


def _small_problem(seed, levels, N=300, K=7, d=6):
    rng = np.random.default_rng(seed)
    Z, meta, _ = synth(N, d=d, levels=levels, seed=seed)
    skw, _ = prepare_setup_args(Z, meta, ["cov%d" % i for i in range(len(levels))], nclust=K, sigma=0.1 + 0.1 * rng.random(K))
    Phi = phi_matrix(skw["Phi"])
    Zn = ref.normalise_cols(skw["Z"])
    Y = ref.normalise_cols(skw["Z"][:, rng.choice(N, K, replace=False)])
    Pr_b = np.asarray(Phi.sum(axis=1)).ravel() / N
    return rng, skw, Phi, Zn, Y, Pr_b


@pytest.mark.parametrize("block_size", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("levels", [(4,), (3, 5)])
def test_streamed_round_equals_the_direct_loop(block_size, levels):
    rng, skw, Phi, Zn, Y, Pr_b = _small_problem(1, levels, N=293)
    N = Zn.shape[1]
    nb, cpb, _ = ref.block_partition(N, block_size)
    R_prev, _, _, _ = ref.head(Y, Zn, skw["sigma"], Phi, Pr_b)
    order = rng.permutation(N)
    args = (Y, Zn, Phi, Pr_b, skw["sigma"], skw["theta"], order, nb, cpb)
    R_free = ref._update_round_direct(R_prev, *args)                       # the reference's own sequence
    assert np.abs(ref.update_round(R_prev, R_free, *args) - R_free).max() <= 1e-12
    R_next = np.abs(R_free + 0.01 * rng.random(R_free.shape))             # any observed values: the teacher-forced forms agree
    R_next /= R_next.sum(axis=0)
    assert np.abs(ref.update_round(R_prev, R_next, *args) - ref._update_round_direct(R_prev, *args, R_next=R_next)).max() <= 1e-12


def test_block_partition_follows_the_fp32_formula():
    assert ref.block_partition(1000, 0.05)[:2] == (20, 50)
    assert ref.block_partition(1000, 0.3)[:2] == (4, 300)
    assert ref.block_partition(1000, 1.0)[:2] == (1, 1000)
    nb, cpb, bounds = ref.block_partition(100003, 0.05)
    assert (nb, cpb) == (20, 5000) and bounds[-1] == (95000, 100003)
    assert sum(hi - lo for lo, hi in bounds) == 100003
    # the block sizes of the many-block GPU cases at their N: (n_blocks, cells_per_block, cells of the last block)
    for N, bs, want in ((40000, 0.01, (100, 400, 400)), (80000, 0.016, (63, 1280, 640)), (60000, 0.016, (63, 960, 480)), (40000, 1.0 / 64, (64, 625, 625)),
                        (40000, 0.0155, (65, 620, 320)), (30000, 0.001, (1000, 30, 30))):
        nb, cpb, bounds = ref.block_partition(N, bs)
        assert (nb, cpb, bounds[-1][1] - bounds[-1][0]) == want, (N, bs)
        assert len(bounds) == nb and bounds[-1][1] == N and sum(hi - lo for lo, hi in bounds) == N


@pytest.mark.parametrize("levels,lam,cutoff", [((4,), None, 1e-5), ((4,), "fixed", 0.2), ((3, 5), None, 0.15), ((2, 3, 4), "fixed", 1e-5)])
def test_combination_sums_equal_the_per_cell_products(levels, lam, cutoff):
    rng, skw, Phi, Zn, Y, Pr_b = _small_problem(2, levels)
    R, _, O, E = ref.head(Y, Zn, skw["sigma"], Phi, Pr_b)
    B = Phi.shape[0]
    lam_vec = None if lam is None else np.concatenate([[0.0], 0.5 + rng.random(B)])
    Zo = skw["Z"]
    B_vec = skw["B_vec"]
    s = ref.moe_correct_ridge(R, Zo, O, E, Phi, B_vec, lam_vec, 0.2, cutoff, Y)
    Zd, Yd, Wd = ref._moe_correct_ridge_direct(R, Zo, O, E, Phi, B_vec, lam_vec, 0.2, cutoff, Y)
    assert np.abs(s["Z_corr"] - Zd).max() <= 1e-12 * np.abs(Zo).max()
    assert np.abs(s["Y"] - Yd).max() <= 1e-12
    assert np.abs(s["W"] - Wd).max() <= 1e-12 * max(1.0, np.abs(Wd).max())
    if cutoff > 1e-3:
        assert s["subset"].any()


# ---- the many-block / d 65..76 / launch-geometry cases of tests/test_gpu_stage_spec.py, before a GPU sees them ------------------------------
def _design(skw):
    """(B, C, Q, ntitems) of a setup: levels, covariates, level combinations present, 16-cell tiles with every combination's cells in tiles of its own"""
    Phi = phi_matrix(skw["Phi"])
    q_of, levels = ref._combinations(Phi, skw["B_vec"])
    return Phi.shape[0], len(skw["B_vec"]), levels.shape[0], int(sum((n + 15) // 16 for n in np.bincount(q_of)))


def _plan_of(skw, env, monkeypatch):
    """the launch plan hmx_setup would take at 256 CUs: as the handle's getters report it"""
    for k in [k for k in os.environ if k.startswith("HMX_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, C, Q, ntitems = _design(skw)
    d, N = skw["Z"].shape
    nb, cpb, _ = ref.block_partition(N, skw["block_size"])
    p = plan(N, skw["K"], d=d, B=B, C_=C, Q=Q, nb=nb, cells_per_block=cpb, ntitems=ntitems, usig=int(np.ptp(skw["sigma"]) == 0))
    assert "limit" not in p, p
    p.update(chain=int(p["chain_ok"] or p["chain_pair"]), sold_carry=p["carry_ok"], shuffle_inv=p["shuf_inv"], n_blocks=nb, cells_per_block=cpb)
    return p, Q


@pytest.mark.parametrize("name", PLAN_CASES + sorted(LATTICE))
def test_gpu_cases_claim_what_the_plan_gives(name, monkeypatch):
    """a later change of a threshold must not silently empty a case: its claimed path is the plan's, for its own B, Q and tile count"""
    Z, meta, var, kw, env, _seed, path = _case(name)
    skw, _ = prepare_setup_args(Z, meta, var, **kw)
    p, Q = _plan_of(skw, env, monkeypatch)
    N = Z.shape[0]
    claims = {g: v for g, v in path.items() if g not in ("host", "push", "last_block")}
    assert {g: p[g] for g in claims} == claims
    assert p["solve_on_device"] == 1 - path["host"]
    if "last_block" in path:
        assert N - (p["n_blocks"] - 1) * p["cells_per_block"] == path["last_block"]
    if name in LATTICE:
        # the instantiations the table credits the case with are the ledger's for the case's own design; its K is the one its name files it under
        got, _bounds = ledger_of("stages", name)
        credit = LATTICE[name][8]
        assert {(("k_tile",) if kind in ("head", "update", "chain") else (kind,)) + tuple(v) for kind, v in credit.items()} == \
            {v for v, kind in got.items() if kind not in ("seed", "lloyd")}, (credit, got)
        assert ("chain" in credit) == bool(path["chain"]) and p["NCT"] == int(name[1:3]) and "K%d_" % skw["K"] in name
    if name == "o_blocks_63_carried":
        # the padded order with 63 * 63 keys stays inside int32, and the blocks inside lpair's 6 bits
        assert (p["nkeys"], p["npad"]) == (3969, N + 3969 * Q * 16) and p["npad"] < 2 ** 31 and p["n_blocks"] - 1 < 64
    if name == "o_blocks_1000_four_waves":
        assert p["cells_per_block"] <= 32 and Q == 6          # two 16-cell tiles over six combinations
    if name == "p_contiguous_ranges":
        assert 4.0 <= N / 16 / (8 * 255) < 4.5
    if name.startswith("q_d"):
        assert (p["NT4"], p["NS2"], p["chain_ok"]) == (4, 3, 1) and 68 <= p["zs"] <= 76
    if name == "r_launch_geometry":
        assert (p["nrep"], p["upd_threads"], p["upd_maxblocks"], p["upd_tpw"]) == (1, 256, 64, 3)


@pytest.mark.parametrize("name", sorted(LADDERS) + sorted(SMALL_LADDERS))
def test_gpu_ladders_claim_what_the_plan_gives(name, monkeypatch):
    Z, meta, var, kw, env, _seed, path = _ladder(name)
    skw, _ = prepare_setup_args(Z, meta, var, **kw)
    p, _Q = _plan_of(skw, env, monkeypatch)
    assert {g: p[g] for g in path} == path
    assert skw["epsilon_kmeans"] < -1e8         # the windowed check never ends a call


@pytest.mark.parametrize("name", ["o_blocks_100", "o_blocks_64", "o_blocks_65", "o_blocks_1000_four_waves", "q_d68_fp32_on_the_chain",
                                  "q_d76_fp32_on_the_chain"] + sorted(LATTICE))
def test_oracle_stages_match_the_spec_on_the_small_gpu_cases(name):
    """the small new GPU cases through the CPU oracle: the spec handles 63..1000 blocks and d = 68 / 76, and the cases' keep decisions sit away
    from the cutoff because of their data (everything they depend on but the library's own fp32 tables)"""
    Z, meta, var, kw, _env, _seed, _path = _case(name)
    _oracle_stages(name, Z, meta, var, kw)


def test_oracle_round_ladder_matches_the_spec():
    """the ladder's spec on the oracle (five rounds in one call, the documented generator's orders) before it judges a kernel"""
    Z, meta, _ = synth(3000, d=20, levels=(3,), seed=6)
    skw, _ = prepare_setup_args(Z, meta, "cov0", nclust=12, options=harmony_options(epsilon_cluster=-1e9))
    seed = 5
    Y0 = skw["Z"][:, np.random.default_rng(12).choice(3000, 12, replace=False)]

    def make_handle():
        h = OracleHarmony(accurate=True, seed=seed)
        h.setup(**skw)
        return h

    rungs = run_ladder(make_handle, skw, Y0, lambda h, r: feistel_order(seed, r, 3000), rounds=5)
    assert [r["m"] for r in rungs] == [1, 2, 3, 4, 5]
    for r in rungs:
        assert r["R"] <= BAR and r["argmax"] == 0 and max(r["O"], r["E"], r["obj"]) <= BAR, r
        assert r["first"] == rungs[0]["first"], r      # the oracle repeats itself bit for bit


# ---- the coverage ledger (tests/stage_lattice.py): the cases between them launch every instantiation the plan reaches at small shapes --------------------------
_ledger = {}


def ledger_of(kind, name):
    """(instantiations, loop bounds) of one stage-spec case, ladder or k-means case, for its own design"""
    if (kind, name) not in _ledger:
        if kind == "stages":
            Z, meta, var, kw, env, _seed, _path = _case(name)
            script = "stages"
        elif kind == "ladder":
            Z, meta, var, kw, env, _seed, _path = _ladder(name)
            script = ("ladder", gpu_spec.ladder_rounds(name))
        elif kind == "kmeans":
            Z, meta, var, kw, env = gpu_kmeans.case_data(name)
            script = "kmeans"
        else:       # tests/test_gpu_parity2.py::test_kmeans_centers_headline_shape: (N, d, K)
            Z, meta, _ = synth(name[0], d=name[1], levels=(10,), seed=9)
            var, kw, env, script = "cov0", dict(nclust=name[2]), {}, "kmeans"
        skw, _ = prepare_setup_args(Z, meta, var, **kw)
        N, K, shape, items = lattice.shape_of(skw)
        got, p = lattice.launches(N, K, shape, items, env, script)
        assert got, (kind, name, p)
        _ledger[(kind, name)] = (got, lattice.loop_bounds(got, p))
    return _ledger[(kind, name)]


def _older_cases():
    return [("stages", n) for n in gpu_spec.CASES if n not in LATTICE and not n.endswith("_pushed")] + [("ladder", n) for n in sorted(LADDERS) + sorted(SMALL_LADDERS)]


def ledger_of_existing_cases():
    return set().union(*[set(ledger_of(*c)[0]) for c in _older_cases()])


def bounds_of_existing_cases():
    return set().union(*[ledger_of(*c)[1] for c in _older_cases()])


# Instantiations of the envelope that no case can reach below 100 000 cells, each with the plan expression that keeps it out of reach.  At most 5 % of the envelope.
EXCLUSIONS = {}


def test_the_cases_launch_every_instantiation_the_envelope_reaches():
    """Every kernel instantiation the plan reaches across the envelope (tests/stage_lattice.py: K = 1 .. 256, 17 values of d, both sigma forms, one and two covariates,
    4000 and 6000 cells, with and without HMX_CHAIN=0, two rounds with the carry forced on) is launched by a stage-spec case, a ladder or a k-means case -- each for its
    own B, C, Q, tile counts and block partition --, and so held to an fp64 spec on the GPU.  What the cases launch beyond the envelope (shapes only many cells reach) is printed."""
    reach, _ = lattice.envelope()
    cases = _older_cases() + [("stages", n) for n in sorted(LATTICE)] + [("kmeans", n) for n in sorted(gpu_kmeans.CASES)] + \
        [("kmeans_old", (100000, 50, 100)), ("kmeans_old", (20000, 128, 256))]
    held, bounds = {}, set()
    for c in cases:
        got, b = ledger_of(*c)
        bounds |= b
        for v in got:
            held.setdefault(v, []).append(c)
    print("envelope: %d instantiations; cases: %d, launching %d" % (len(reach), len(cases), len(held)))
    print("exclusions (%d):" % len(EXCLUSIONS))
    for v, why in sorted(EXCLUSIONS.items()):
        print("  ", v, why)
    print("launched beyond the envelope:", sorted(set(held) - set(reach)))
    assert len(EXCLUSIONS) <= 0.05 * len(reach) and set(EXCLUSIONS) <= set(reach) and not set(EXCLUSIONS) & set(held)
    missing = sorted(set(reach) - set(held) - set(EXCLUSIONS))
    assert not missing, [(v, reach[v]) for v in missing]
    assert set(held) & set(reach) == set(reach) - set(EXCLUSIONS)
    # the seeding race and Lloyd: every instantiation by a k-means case of its own (centres judged, not only handed on)
    km = {v for v, cs in held.items() if any(c[0] == "kmeans" for c in cs)}
    assert {v for v in reach if v == ("k_lloyd",) or (v[0] == "k_tile" and v[3] in (2, 3))} <= km
    assert {("k_tile", 1, n, 2, 3, 0) for n in (5, 6, 7)} <= km          # (the three-wave Lloyd: beyond the envelope, more than 1024 static tiles)
    # the chain without R stores at 1 .. 7 cluster tiles by a ladder
    assert {("k_tile", 1, n, 5, 2, 1) for n in range(1, 8)} <= {v for v, cs in held.items() if any(c[0] == "ladder" for c in cs)}
    # the loop bounds of d, in each build that the plan admits them in: NT4 = 0 .. 8, tail = 0 .. 3, NS2 = 1 .. 4
    want = lattice.admitted_loop_bounds()
    assert {(bf, f, v) for bf in (0, 1) for f, vs in (("NT4", range(9)), ("tail", range(4)), ("NS2", range(1, 5))) for v in vs} == want
    assert want <= bounds, sorted(want - bounds)
