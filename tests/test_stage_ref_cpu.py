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
from stage_check import phi_matrix, run_stages  # noqa: E402

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
