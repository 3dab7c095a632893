"""Each stage of the HIP path against the fp64 spec (tests/stage_ref.py) across the dispatch envelope: init, one clustering round
(teacher-forced), the ridge correction, a stand-alone objective after it and the next call's cold start.  Both sides start from the
handle's own state, so nothing drifts and the bars sit near fp32 rounding.  Every case asserts the path it claims through the getters."""
import json
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from harmony_amd import Harmony, harmony_options, prepare_setup_args  # noqa: E402
from helpers import synth  # noqa: E402
from oracle.oracle import feistel_order  # noqa: E402
from stage_check import run_stages  # noqa: E402

pytestmark = pytest.mark.gpu

# Bars: at most 10x the worst error measured over these cases on an MI355X (in brackets).  Both sides share the fp32 inputs; what is left is
# the library's own fp32 rounding.
BARS = {
    "R": 5e-6,          # teacher-forced R, max-abs, d <= 64 [2.7e-6]
    "R_d128": 1e-5,     # ... d = 128: dist sums more than twice as many fp32 products, and R moves by R (1 - R) ddist / sigma [5.1e-6]
    "tab": 3e-7,        # O and E against fp64 sums over the handle's own R, relative Frobenius [3.0e-8]
    "obj": 1e-6,        # objective terms of a head or a round, relative to the sum of the terms' absolute values [3.7e-7]
    "stale_obj": 4e-7,  # the stand-alone objective after a correction [3.7e-8]
    "Z_rel": 1e-6,      # Z_corr, relative Frobenius [1.1e-7]
    "Z_maxabs": 3e-6,   # Z_corr, max-abs over max |Z_orig| [2.8e-7]
    "Y": 3e-7,          # per column over max(1, cond(A_k)); a skipped cluster's column is the old one renormalised in fp32 [5.8e-8]
    "W": 3e-8,          # per row over max(1, cond(A_k)) * ||W|| [2.7e-9]
    "Lambda": 2.4e-7,   # alpha * E[k, b]: E and the product rounded to fp32 [7.2e-8]
}
# The keep decisions (float(O[k, b]) / N_b > cutoff) are comparable while no level lies closer to the cutoff than many times the tables'
# relative error (3.0e-8 at most): 1e-5.  A bound of 1e-3 is missed by one or two of the 24 000 - 48 000 cluster x level entries of the
# many-level cases whatever the seed; the subset / skip counts and the shape of the last W are compared exactly in every case anyway.
KEEP_MARGIN = 1e-5


def _skipped_population(N, d, seed):
    """four levels sharing one population, and a fifth whose cells point the opposite way along the last PC: the clusters that settle there
    see one level only (no covariate with two kept levels) and are skipped"""
    Z, meta, _ = synth(N, d=d, levels=(4,), seed=seed)
    rng = np.random.default_rng(seed)
    far = rng.random(N) < 0.1
    Z[~far, -1] += 30.0
    Z[far] = rng.normal(size=(int(far.sum()), d)) * 0.5
    Z[far, -1] = -30.0
    lev = meta["cov0"].copy()
    lev[far] = 4
    return Z, {"cov0": lev}


def _case(name):
    """(Z, meta, vars_use, setup kwargs, environment, handle seed, path assertions)"""
    o = {}
    if name == "a_chain_schur":
        Z, meta, _ = synth(100000, d=50, levels=(10,), seed=1)
        return Z, meta, "cov0", dict(nclust=100), o, 3, dict(chain=1, chain_pair=0, usig=1, upd_wps=2, host=0, min_kept=8)
    if name == "b_four_waves_dense":
        Z, meta, _ = synth(30000, d=50, levels=(6,), seed=2)
        return Z, meta, "cov0", dict(nclust=48), o, 4, dict(chain=1, upd_wps=4, host=0, max_kept=7)
    if name == "c_first_generation_k30_d17":
        Z, meta, _ = synth(20000, d=17, levels=(5,), seed=3)
        return Z, meta, "cov0", dict(nclust=30), o, 5, dict(host=0)
    if name == "c_first_generation_k256_d128":
        Z, meta, _ = synth(20000, d=128, levels=(4,), seed=4)
        return Z, meta, "cov0", dict(nclust=256), o, 6, dict(chain=0, chain_pair=0, dot_bf=1, host=0)
    if name == "d_wave_pair_nested_subset":
        Z, meta, _ = synth(60000, d=50, levels=(8, 64, 128), nested=True, seed=7)
        return Z, meta, ["cov0", "cov1", "cov2"], dict(nclust=200), o, 7, dict(chain_pair=1, subset=1, host=0)
    if name == "e_launch_per_step_k152":
        Z, meta, _ = synth(40000, d=50, levels=(4, 30), seed=8)
        return Z, meta, ["cov0", "cov1"], dict(nclust=152), {"HMX_CHAIN_PAIR": "0"}, 8, dict(chain=0, chain_pair=0, host=0)
    if name == "f_host_closed_form_1200":
        Z, meta, _ = synth(60000, d=30, levels=(1200,), seed=9)
        return Z, meta, "cov0", dict(nclust=40), o, 9, dict(chain=0, sold_carry=0, host=1)
    if name == "g_host_cholesky_1200x3":
        Z, meta, _ = synth(60000, d=30, levels=(1200, 3), seed=10)
        return Z, meta, ["cov0", "cov1"], dict(nclust=40), o, 10, dict(chain=0, sold_carry=0, host=1)
    if name == "h_device_1100":
        Z, meta, _ = synth(60000, d=30, levels=(1100,), seed=11)
        return Z, meta, "cov0", dict(nclust=40), o, 11, dict(chain=0, host=0, min_kept=8)
    if name == "i_crossed_small_combinations":
        Z, meta, _ = synth(30000, d=32, levels=(40, 50), seed=12)
        return Z, meta, ["cov0", "cov1"], dict(nclust=64), o, 12, dict(host=0)
    if name == "j_skipped":
        Z, meta = _skipped_population(20000, 30, 13)
        return Z, meta, "cov0", dict(nclust=20), o, 13, dict(skipped=1, host=0)
    if name == "k_fixed_lambda_sigma_theta0":
        Z, meta, _ = synth(20000, d=30, levels=(5, 3), seed=14)
        sig = 0.08 + 0.07 * np.random.default_rng(14).random(40)
        return Z, meta, ["cov0", "cov1"], dict(nclust=40, lambda_=[1.0, 2.0], sigma=sig, theta=[2.0, 0.0]), o, 14, dict(usig=0, host=0)
    if name == "l_forced_fallbacks":
        Z, meta, _ = synth(30000, d=50, levels=(10,), seed=1)
        env = {"HMX_MOE_SOLVE": "host", "HMX_MOE_IMPL": "v1", "HMX_MOE_STATS": "atomic", "HMX_FUSED_FOLD": "0", "HMX_CHAIN": "0"}
        return Z, meta, "cov0", dict(nclust=100), env, 3, dict(chain=0, host=1)
    if name == "m_block_0.3_prime_pushed":
        Z, meta, _ = synth(20011, d=30, levels=(6,), seed=15)
        return Z, meta, "cov0", dict(nclust=32, options=harmony_options(block_size=0.3)), o, 15, dict(host=0, push=1)
    if name == "m_block_1.0":
        Z, meta, _ = synth(20011, d=30, levels=(6,), seed=16)
        return Z, meta, "cov0", dict(nclust=32, options=harmony_options(block_size=1.0)), o, 16, dict(host=0)
    if name == "n_baseline_1M":
        Z, meta, _ = synth(1000000, d=50, levels=(10,), seed=17)
        return Z, meta, "cov0", dict(nclust=100), o, 17, dict(chain=1, host=0)
    raise KeyError(name)


CASES = ["a_chain_schur", "b_four_waves_dense", "c_first_generation_k30_d17", "c_first_generation_k256_d128", "d_wave_pair_nested_subset",
         "e_launch_per_step_k152", "f_host_closed_form_1200", "g_host_cholesky_1200x3", "h_device_1100", "i_crossed_small_combinations",
         "j_skipped", "k_fixed_lambda_sigma_theta0", "l_forced_fallbacks", "m_block_0.3_prime_pushed", "m_block_1.0", "n_baseline_1M"]


@pytest.mark.parametrize("name", CASES)
def test_stages_match_the_spec(name, monkeypatch):
    t0 = time.time()
    Z, meta, var, kw, env, seed, path = _case(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    skw, _ = prepare_setup_args(Z, meta, var, **kw)
    del Z
    h = Harmony(seed=seed, stale_dist=1)
    h.setup(**skw)
    N = int(h.N)
    Y0 = h.kmeans_centers()
    pushed = [None, None]

    def order_of_round(r):
        if path.get("push"):
            pushed[r] = np.random.default_rng(seed + r).permutation(N)
            h.push_update_order(pushed[r])
            return pushed[r]
        return feistel_order(seed, r, N)         # hmx_api_update.inc: round r of the handle's round_counter, counted from setup

    err, info = run_stages(h, skw, Y0, order_of_round)
    info["seconds"] = round(time.time() - t0, 1)
    print("STAGE_SPEC", name, json.dumps({"err": err, "info": info}, default=str))
    msg = repr((name, err, info))

    # the path this case claims
    for g in ("chain", "chain_pair", "usig", "upd_wps", "dot_bf", "sold_carry"):
        if g in path:
            assert int(h._scalar(g)) == path[g], (g, msg)
    if path["host"]:
        assert h.timer("moe_solve_host") > 0, msg
    else:
        assert h.timer("moe_solve_host") == 0, msg
    if path.get("subset"):
        assert info["subset"] > 0, msg
    if path.get("skipped"):
        assert info["skipped"] > 0, msg
    if "min_kept" in path:
        assert info["max_kept"] >= path["min_kept"], msg
    if "max_kept" in path:
        assert info["max_kept"] <= path["max_kept"], msg
    assert (int(h._scalar("n_blocks")), int(h._scalar("cells_per_block"))) == (info["n_blocks"], info["cells_per_block"]), msg

    # the keep decisions are comparable only away from the cutoff
    assert info["keep_margin"] >= KEEP_MARGIN, msg
    bar_R = BARS["R_d128"] if int(h.d) > 64 else BARS["R"]
    for st in ("init", "round", "cold"):
        assert err[st + "_R"] <= bar_R, (st, msg)
        assert err[st + "_argmax"] == 0, (st, msg)
        assert err[st + "_O"] <= BARS["tab"] and err[st + "_E"] <= BARS["tab"], (st, msg)
        assert err[st + "_obj"] <= BARS["obj"], (st, msg)
    assert err["stale_obj"] <= BARS["stale_obj"], msg
    assert err["Z_rel"] <= BARS["Z_rel"] and err["Z_maxabs"] <= BARS["Z_maxabs"], msg
    assert err["Y"] <= BARS["Y"], msg
    assert err["W"] <= BARS["W"], msg
    assert err["Lambda"] <= BARS["Lambda"], msg
    assert (info["subset_h"], info["skipped_h"]) == (info["subset"], info["skipped"]), msg
