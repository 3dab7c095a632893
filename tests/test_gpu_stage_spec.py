"""Each stage of the HIP path against the fp64 spec (tests/stage_ref.py) across the dispatch envelope: init, one clustering round
(teacher-forced), the ridge correction, a stand-alone objective after it and the next call's cold start.  Both sides start from the
handle's own state, so nothing drifts and the bars sit near fp32 rounding.  Every case asserts the path it claims through the getters.
The o_ .. r_ cases walk the branches of the launch plan (harmony_amd/csrc/hmx_plan.h) on the block count -- 63 | 64 | 65 | 100 | 1000 blocks --, the
d window 65..76 and the launch geometry switches; tests/test_stage_ref_cpu.py holds their claimed paths to the plan itself, without a GPU.
The round ladder (run_ladder) judges what a round hands to the next one -- carried old contributions, elided R stores, the 4-round sort
groups -- against the same spec.
The t01_ .. t16_ cases (LATTICE) are small shapes, one per kernel instantiation the others leave out; tests/stage_lattice.py proves on the CPU that all cases together
launch every instantiation the plan reaches at such shapes, and each lattice case asserts that the instantiation that ran is the one it is credited with.  What a case
would catch: in k_tile<3, 0, 2, false> of the split-bf16 build (the update, per-cluster sigma) only t03_K40_d80_v runs, with K = 40 on 48 columns: by kcol (hmx_internal.h)
lane c holds clusters 3 c + {0, 1, 2}, so lane 13 holds 39 | 40 | 41 -- one valid, two past K -- and lanes 14 and 15 none.  Two cluster columns exchanged at that edge
(38 and 39, say) leave round_R off by |R[38] - R[39]| of the cells near either cluster (bar 1e-5) and its O / E tables by whole columns (bar 3e-7).
No other case launches that instantiation."""
import json
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from harmony_amd import Harmony, HarmonyError, harmony_options, prepare_setup_args  # noqa: E402
from helpers import synth  # noqa: E402
from oracle.oracle import feistel_order  # noqa: E402
from stage_check import run_ladder, run_stages  # noqa: E402
from test_plan_cpu import LAUNCH_FIELDS, RIDGE_FIELDS  # noqa: E402

pytestmark = pytest.mark.gpu

# Bars: at most 10x the worst error measured over these cases on an MI355X (in brackets).  Both sides share the fp32 inputs; what is left is
# the library's own fp32 rounding.  The o_ .. r_ cases and the round ladders stay below the a_ .. n_ figures in every column (d = 68 / 76: R 3.7e-6 /
# 3.9e-6 under R_d128; the ladders' rungs: R 2.0e-6 .. 2.3e-6, tables 2.8e-8, objective 1.2e-7 .. 2.7e-7): no bar was added or moved for them.
# The LATTICE cases (73 small shapes, one per kernel instantiation the older cases leave out) use the same bars.  Worst figures on an MI355X (over the 72 cases of the set cover; t16_K232_d64_v, added by hand, passes the same bars): R 2.3e-6 (d <= 64,
# t08_K128_d64_u) and 4.4e-6 (d > 64, t03_K33_d128_v_dotf32), O 8.6e-8 / E 8.1e-8 and stale objective 1.4e-7 (all three at t16_K225_d1_u: d = 1, every cell is +1 or -1),
# objective 3.5e-7, Z_corr 1.1e-7 rel. / 2.7e-7 max-abs, Y 6.1e-9, W 1.2e-8, Lambda 7.2e-8, no argmax off; the two-round ladders of the chain without R stores: R 1.8e-6,
# tables 2.8e-8, objective 2.8e-7.  The tables and the stale objective exceed the older cases' worst (3.0e-8, 3.7e-8) and stay below a third of their bars.
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


def _case(name, cus=256):
    """(Z, meta, vars_use, setup kwargs, environment, handle seed, path assertions); cus: compute units of the device (one case sizes itself by it)"""
    o = {}
    if name.endswith("_pushed") and name[:-7] in PUSHED:      # the same case under host-injected orders (prepare_round's pos / cells_per_block path)
        Z, meta, var, kw, env, seed, path = _case(name[:-7], cus)
        return Z, meta, var, kw, env, seed, dict(path, push=1)
    if name in LATTICE:
        N, d, levels, K, sigma, env, dseed, path, _credit = LATTICE[name]
        Z, meta, _ = synth(N, d=d, levels=levels, seed=dseed)
        kw = dict(nclust=K) if sigma == "u" else dict(nclust=K, sigma=0.08 + 0.07 * np.random.default_rng(dseed).random(K))
        return Z, meta, sorted(meta), kw, env, dseed, path
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
        env = {"HMX_MOE_SOLVE": "host", "HMX_MOE_IMPL": "v1", "HMX_FUSED_FOLD": "0", "HMX_CHAIN": "0"}
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
    # ---- the block count against the plan's thresholds: nb <= 63 (carry, 6-bit block fields of lpair), nb < 64 (sort-free shuffle), nb <= 64 (chains),
    #      objslots = min(nb, 64) (above it k_tile adds into slot row j % objslots), need_lorder = nb * K * 8 > 64 KB
    if name == "o_blocks_100":
        Z, meta, _ = synth(40000, d=50, levels=(10,), seed=18)
        return Z, meta, "cov0", dict(nclust=100, options=harmony_options(block_size=0.01)), o, 18, dict(
            n_blocks=100, cells_per_block=400, chain=0, sold_carry=0, shuffle_inv=0, need_lorder=1, objslots=64, host=0)
    if name == "o_blocks_63_carried":       # the last block index that fits lpair's 6 bits
        Z, meta, _ = synth(80000, d=50, levels=(4,), seed=19)
        return Z, meta, "cov0", dict(nclust=100, options=harmony_options(block_size=0.016)), {"HMX_SOLD_CARRY": "1"}, 19, dict(
            n_blocks=63, chain=1, sold_carry=1, shuffle_inv=1, objslots=63, host=0)
    if name == "o_blocks_64":
        Z, meta, _ = synth(40000, d=50, levels=(10,), seed=20)
        return Z, meta, "cov0", dict(nclust=100, options=harmony_options(block_size=1.0 / 64)), o, 20, dict(
            n_blocks=64, cells_per_block=625, chain=1, sold_carry=0, shuffle_inv=0, host=0)
    if name == "o_blocks_65":               # objslots < n_blocks: block 64 adds into block 0's slot row
        Z, meta, _ = synth(40000, d=50, levels=(10,), seed=21)
        return Z, meta, "cov0", dict(nclust=100, options=harmony_options(block_size=0.0155)), o, 21, dict(
            n_blocks=65, cells_per_block=620, last_block=320, chain=0, objslots=64, host=0)
    if name == "o_blocks_1000_four_waves":  # blocks of two 16-cell tiles spread over 6 combinations
        Z, meta, _ = synth(30000, d=50, levels=(6,), seed=22)
        return Z, meta, "cov0", dict(nclust=48, options=harmony_options(block_size=0.001)), o, 22, dict(
            n_blocks=1000, cells_per_block=30, upd_wps=4, chain=0, need_lorder=1, host=0)
    if name == "p_contiguous_ranges":       # launch-per-step path, one block: from 4 tiles per wave a wave owns a contiguous range (4.29 here)
        N = 140000 if cus == 256 else int(4.29 * 16 * 8 * (cus - 1)) // 16 * 16
        Z, meta, _ = synth(N, d=50, levels=(10,), seed=23)
        return Z, meta, "cov0", dict(nclust=100, options=harmony_options(block_size=1.0)), {"HMX_CHAIN": "0"}, 23, dict(
            chain=0, upd_contig=1, host=0)
    # ---- 64 < d <= 76: zs 68..76, NT4 = 4, NS2 = 3: the fp32 register form of the distance GEMM on rows longer than 64 PCs, on the chain,
    #      with the first-generation ridge kernels (d > 64)
    if name in ("q_d68_fp32_on_the_chain", "q_d76_fp32_on_the_chain"):
        d = int(name[3:5])
        Z, meta, _ = synth(30000, d=d, levels=(10,), seed=24 + d)
        return Z, meta, "cov0", dict(nclust=100), o, 24, dict(dot_bf=0, chain=1, moe_mfma=0, host=0)
    if name == "r_launch_geometry":
        Z, meta, _ = synth(30000, d=50, levels=(10,), seed=25)
        env = {"HMX_NREP": "1", "HMX_UPD_THREADS": "256", "HMX_UPD_MAXBLOCKS": "64", "HMX_UPD_TPW": "3", "HMX_CHAIN": "0"}
        return Z, meta, "cov0", dict(nclust=100), env, 25, dict(chain=0, host=0)
    raise KeyError(name)


CASES = ["a_chain_schur", "b_four_waves_dense", "c_first_generation_k30_d17", "c_first_generation_k256_d128", "d_wave_pair_nested_subset",
         "e_launch_per_step_k152", "f_host_closed_form_1200", "g_host_cholesky_1200x3", "h_device_1100", "i_crossed_small_combinations",
         "j_skipped", "k_fixed_lambda_sigma_theta0", "l_forced_fallbacks", "m_block_0.3_prime_pushed", "m_block_1.0", "n_baseline_1M"]
PLAN_CASES = ["o_blocks_100", "o_blocks_63_carried", "o_blocks_64", "o_blocks_65", "o_blocks_1000_four_waves", "p_contiguous_ranges",
              "q_d68_fp32_on_the_chain", "q_d76_fp32_on_the_chain", "r_launch_geometry"]
PUSHED = ["o_blocks_100", "o_blocks_65", "o_blocks_1000_four_waves"]
CASES += PLAN_CASES + [n + "_pushed" for n in PUSHED]
# ---- one small case per kernel instantiation: chosen by greedy set cover over the coverage ledger (tests/stage_lattice.py, tools/make_stage_lattice.py) so that, with the
#      cases above and the ladders, every k_tile head / update / chain / wave-pair variant of both builds and every ridge statistics / apply kernel that the plan reaches at
#      4000 - 6000 cells is launched by a case.  K: per cluster-tile count a full last tile (16 NCT), one valid lane in it (16 (NCT - 1) + 1), inside a quad (16 NCT - 8 | 4) and
#      the lowest K of a kernel that serves two tile counts (129, 225); d rotated over 1 .. 128 (68 / 72 / 76: the fp32 build without a switch; 64 with K = 128: statistics
#      without LDS shadows); u | v: uniform | per-cluster sigma; c2: two covariates.
#      name -> (cells, PCs, levels, clusters, sigma form, environment, seed of the data and the handle, the path it claims, the launches the ledger credits it with:
#      k_tile (bf, nct, mode, wps, usig), ridge (mfma, p0, p1)); tests/test_stage_ref_cpu.py holds both to the plan for the case's own design
LATTICE = {
    't01_K8_d32_v': (4000, 32, (4,), 8, 'v', {}, 200,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 1, 1, 2, 0), 'chain': (1, 1, 4, 2, 0), 'stats': (1, 1, 1), 'apply': (1, 2, 0)}),
    't01_K8_d100_u_dotf32': (4000, 100, (4,), 8, 'u', {'HMX_DOT': 'f32'}, 201,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 1, 1, 4, 1), 'update': (0, 1, 0, 4, 1), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't01_K8_d128_v': (4000, 128, (4,), 8, 'v', {}, 202,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 1, 1, 2, 0), 'update': (1, 1, 0, 2, 0), 'stats': (0, 32, 0), 'apply': (0, 1, 2)}),
    't01_K16_d8_u_dotf32': (4000, 8, (4,), 16, 'u', {'HMX_DOT': 'f32'}, 203,
        {'chain': 1, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 0, 'moe_mfma': 1, 'host': 0},
        {'head': (0, 1, 1, 4, 1), 'chain': (0, 1, 4, 2, 1), 'stats': (1, 1, 1), 'apply': (1, 1, 0)}),
    't01_K16_d76_v': (4000, 76, (4,), 16, 'v', {}, 204,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 1, 1, 2, 0), 'chain': (0, 1, 4, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't01_K16_d76_v_c2_chain0': (4000, 76, (3, 2), 16, 'v', {'HMX_CHAIN': '0'}, 205,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 1, 1, 2, 0), 'update': (0, 1, 0, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't01_K16_d80_u_c2': (4000, 80, (3, 2), 16, 'u', {}, 206,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 1, 1, 4, 1), 'update': (1, 1, 0, 4, 1), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't02_K17_d96_v_c2': (4000, 96, (3, 2), 17, 'v', {}, 207,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 2, 1, 2, 0), 'update': (1, 2, 0, 2, 0), 'stats': (0, 32, 0), 'apply': (0, 1, 2)}),
    't02_K17_d128_u': (4000, 128, (4,), 17, 'u', {}, 208,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 2, 1, 4, 1), 'update': (1, 2, 0, 4, 1), 'stats': (0, 32, 0), 'apply': (0, 1, 2)}),
    't02_K24_d65_u_c2': (4000, 65, (3, 2), 24, 'u', {}, 209,
        {'chain': 1, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 2, 1, 4, 1), 'chain': (0, 2, 4, 2, 1), 'stats': (0, 24, 0), 'apply': (0, 1, 2)}),
    't02_K24_d68_v': (4000, 68, (4,), 24, 'v', {}, 210,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 2, 1, 2, 0), 'chain': (0, 2, 4, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 1, 2)}),
    't02_K32_d17_v_c2': (4000, 17, (3, 2), 32, 'v', {}, 211,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 2, 1, 2, 0), 'chain': (1, 2, 4, 2, 0), 'stats': (1, 2, 1), 'apply': (1, 2, 0)}),
    't02_K32_d80_u_dotf32': (4000, 80, (4,), 32, 'u', {'HMX_DOT': 'f32'}, 212,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 2, 1, 4, 1), 'update': (0, 2, 0, 4, 1), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't02_K32_d128_v_c2_dotf32': (4000, 128, (3, 2), 32, 'v', {'HMX_DOT': 'f32'}, 213,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 2, 1, 2, 0), 'update': (0, 2, 0, 2, 0), 'stats': (0, 32, 0), 'apply': (0, 1, 2)}),
    't03_K33_d76_v_c2': (4000, 76, (3, 2), 33, 'v', {}, 214,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 3, 1, 2, 0), 'chain': (0, 3, 4, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't03_K33_d128_v_dotf32': (4000, 128, (4,), 33, 'v', {'HMX_DOT': 'f32'}, 215,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 3, 1, 2, 0), 'update': (0, 3, 0, 2, 0), 'stats': (0, 32, 0), 'apply': (0, 1, 2)}),
    't03_K40_d80_v': (4000, 80, (4,), 40, 'v', {}, 216,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 3, 1, 2, 0), 'update': (1, 3, 0, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't03_K48_d68_u': (4000, 68, (4,), 48, 'u', {}, 217,
        {'chain': 1, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 3, 1, 4, 1), 'chain': (0, 3, 4, 2, 1), 'stats': (0, 24, 0), 'apply': (0, 1, 2)}),
    't03_K48_d100_u_c2_dotf32': (4000, 100, (3, 2), 48, 'u', {'HMX_DOT': 'f32'}, 218,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 3, 1, 4, 1), 'update': (0, 3, 0, 4, 1), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't04_K49_d80_v': (4000, 80, (4,), 49, 'v', {}, 219,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 4, 1, 2, 0), 'update': (1, 4, 0, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't04_K49_d96_u_c2': (4000, 96, (3, 2), 49, 'u', {}, 220,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 4, 1, 4, 1), 'update': (1, 4, 0, 4, 1), 'stats': (0, 32, 0), 'apply': (0, 1, 2)}),
    't04_K56_d72_v': (4000, 72, (4,), 56, 'v', {}, 221,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 4, 1, 2, 0), 'chain': (0, 4, 4, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 1, 2)}),
    't04_K56_d76_u_c2': (4000, 76, (3, 2), 56, 'u', {}, 222,
        {'chain': 1, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 4, 1, 4, 1), 'chain': (0, 4, 4, 2, 1), 'stats': (0, 28, 0), 'apply': (0, 1, 2)}),
    't04_K64_d48_v': (4000, 48, (4,), 64, 'v', {}, 223,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 4, 1, 2, 0), 'chain': (1, 4, 4, 2, 0), 'stats': (1, 4, 1), 'apply': (1, 3, 0)}),
    't04_K64_d96_v_dotf32': (4000, 96, (4,), 64, 'v', {'HMX_DOT': 'f32'}, 224,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 4, 1, 2, 0), 'update': (0, 4, 0, 2, 0), 'stats': (0, 32, 0), 'apply': (0, 1, 2)}),
    't04_K64_d116_u_dotf32': (4000, 116, (4,), 64, 'u', {'HMX_DOT': 'f32'}, 225,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 4, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 4, 1, 4, 1), 'update': (0, 4, 0, 4, 1), 'stats': (0, 32, 0), 'apply': (0, 1, 2)}),
    't05_K65_d116_v_c2': (4000, 116, (3, 2), 65, 'v', {}, 226,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 5, 1, 2, 0), 'update': (1, 5, 0, 2, 0), 'stats': (0, 32, 0), 'apply': (0, 2, 2)}),
    't05_K65_d116_u': (4000, 116, (4,), 65, 'u', {}, 227,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 5, 1, 2, 1), 'update': (1, 5, 0, 2, 1), 'stats': (0, 32, 0), 'apply': (0, 2, 2)}),
    't05_K72_d65_v_c2': (4000, 65, (3, 2), 72, 'v', {}, 228,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 5, 1, 2, 0), 'chain': (0, 5, 4, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 2, 2)}),
    't05_K72_d96_u_c2_dotf32': (4000, 96, (3, 2), 72, 'u', {'HMX_DOT': 'f32'}, 229,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 5, 1, 2, 1), 'update': (0, 5, 0, 2, 1), 'stats': (0, 32, 0), 'apply': (0, 2, 2)}),
    't05_K80_d63_v_c2': (4000, 63, (3, 2), 80, 'v', {}, 230,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 5, 1, 2, 0), 'chain': (1, 5, 4, 2, 0), 'stats': (1, 5, 1), 'apply': (1, 4, 0)}),
    't05_K80_d76_u_c2': (4000, 76, (3, 2), 80, 'u', {}, 231,
        {'chain': 1, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 5, 1, 2, 1), 'chain': (0, 5, 4, 2, 1), 'stats': (0, 28, 0), 'apply': (0, 2, 2)}),
    't05_K80_d116_v_c2_dotf32': (4000, 116, (3, 2), 80, 'v', {'HMX_DOT': 'f32'}, 232,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 5, 1, 2, 0), 'update': (0, 5, 0, 2, 0), 'stats': (0, 32, 0), 'apply': (0, 2, 2)}),
    't06_K81_d17_v': (4000, 17, (4,), 81, 'v', {}, 233,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 6, 1, 2, 0), 'chain': (1, 6, 4, 2, 0), 'stats': (0, 20, 0), 'apply': (0, 2, 1)}),
    't06_K81_d100_v_c2': (4000, 100, (3, 2), 81, 'v', {}, 234,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 6, 1, 2, 0), 'update': (1, 6, 0, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 2, 2)}),
    't06_K88_d68_v': (4000, 68, (4,), 88, 'v', {}, 235,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 6, 1, 2, 0), 'chain': (0, 6, 4, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 2, 2)}),
    't06_K88_d116_u_dotf32': (4000, 116, (4,), 88, 'u', {'HMX_DOT': 'f32'}, 236,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 6, 1, 2, 1), 'update': (0, 6, 0, 2, 1), 'stats': (0, 32, 0), 'apply': (0, 2, 2)}),
    't06_K96_d32_u_c2_dotf32': (4000, 32, (3, 2), 96, 'u', {'HMX_DOT': 'f32'}, 237,
        {'chain': 1, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 1, 'host': 0},
        {'head': (0, 6, 1, 2, 1), 'chain': (0, 6, 4, 2, 1), 'stats': (1, 6, 1), 'apply': (1, 2, 0)}),
    't06_K96_d68_v_chain0': (4000, 68, (4,), 96, 'v', {'HMX_CHAIN': '0'}, 238,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 6, 1, 2, 0), 'update': (0, 6, 0, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 2, 2)}),
    't06_K96_d80_u': (4000, 80, (4,), 96, 'u', {}, 239,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 6, 1, 2, 1), 'update': (1, 6, 0, 2, 1), 'stats': (0, 28, 0), 'apply': (0, 2, 2)}),
    't07_K97_d65_v_chain0': (4000, 65, (4,), 97, 'v', {'HMX_CHAIN': '0'}, 240,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 7, 1, 2, 0), 'update': (0, 7, 0, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 2, 2)}),
    't07_K97_d76_v_c2': (4000, 76, (3, 2), 97, 'v', {}, 241,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 7, 1, 2, 0), 'chain': (0, 7, 4, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 2, 2)}),
    't07_K104_d100_v_c2': (4000, 100, (3, 2), 104, 'v', {}, 242,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 7, 1, 2, 0), 'update': (1, 7, 0, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 2, 2)}),
    't07_K112_d63_v_c2': (4000, 63, (3, 2), 112, 'v', {}, 243,
        {'chain': 1, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 7, 1, 2, 0), 'chain': (1, 7, 4, 2, 0), 'stats': (1, 7, 1), 'apply': (1, 4, 0)}),
    't07_K112_d72_u_c2_chain0': (4000, 72, (3, 2), 112, 'u', {'HMX_CHAIN': '0'}, 244,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 7, 1, 2, 1), 'update': (0, 7, 0, 2, 1), 'stats': (0, 24, 0), 'apply': (0, 2, 2)}),
    't08_K113_d16_u': (4000, 16, (4,), 113, 'u', {}, 245,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 8, 1, 2, 1), 'update': (1, 8, 0, 2, 1), 'stats': (0, 16, 0), 'apply': (0, 2, 1)}),
    't08_K113_d72_u': (4000, 72, (4,), 113, 'u', {}, 246,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 8, 1, 2, 1), 'update': (0, 8, 0, 2, 1), 'stats': (0, 24, 0), 'apply': (0, 2, 2)}),
    't08_K120_d60_v': (4000, 60, (4,), 120, 'v', {}, 247,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 8, 1, 2, 0), 'update': (1, 8, 0, 2, 0), 'stats': (1, 8, 1), 'apply': (1, 4, 0)}),
    't08_K128_d64_u': (4000, 64, (4,), 128, 'u', {}, 248,
        {'chain': 1, 'chain_pair': 1, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 8, 1, 2, 1), 'chain': (1, 4, 6, 2, 1), 'stats': (1, 8, 0), 'apply': (1, 4, 0)}),
    't08_K128_d72_v_c2': (4000, 72, (3, 2), 128, 'v', {}, 249,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 8, 1, 2, 0), 'update': (0, 8, 0, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 2, 2)}),
    't10_K129_d3_u': (4000, 3, (4,), 129, 'u', {}, 250,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 10, 1, 2, 1), 'update': (1, 10, 0, 2, 1), 'stats': (0, 4, 0), 'apply': (0, 3, 1)}),
    't10_K145_d1_v_c2': (4000, 1, (3, 2), 145, 'v', {}, 251,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 10, 1, 2, 0), 'update': (1, 10, 0, 2, 0), 'stats': (0, 4, 0), 'apply': (0, 3, 1)}),
    't10_K152_d72_v': (4000, 72, (4,), 152, 'v', {}, 252,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 10, 1, 2, 0), 'update': (0, 10, 0, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 3, 2)}),
    't10_K160_d60_u_c2': (4000, 60, (3, 2), 160, 'u', {}, 253,
        {'chain': 1, 'chain_pair': 1, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 10, 1, 2, 1), 'chain': (1, 5, 6, 2, 1), 'stats': (1, 5, 1), 'apply': (1, 4, 0)}),
    't10_K160_d68_u_c2': (4000, 68, (3, 2), 160, 'u', {}, 254,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 10, 1, 2, 1), 'update': (0, 10, 0, 2, 1), 'stats': (0, 24, 0), 'apply': (0, 3, 2)}),
    't12_K161_d65_v_c2': (4000, 65, (3, 2), 161, 'v', {}, 255,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 12, 1, 2, 0), 'update': (0, 12, 0, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 3, 2)}),
    't12_K177_d3_u': (4000, 3, (4,), 177, 'u', {}, 256,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 12, 1, 2, 1), 'update': (1, 12, 0, 2, 1), 'stats': (0, 4, 0), 'apply': (0, 3, 1)}),
    't12_K184_d50_v': (4000, 50, (4,), 184, 'v', {}, 257,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 12, 1, 2, 0), 'update': (1, 12, 0, 2, 0), 'stats': (1, 6, 1), 'apply': (1, 4, 0)}),
    't12_K192_d24_u': (4000, 24, (4,), 192, 'u', {}, 258,
        {'chain': 1, 'chain_pair': 1, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 12, 1, 2, 1), 'chain': (1, 6, 6, 2, 1), 'stats': (1, 6, 1), 'apply': (1, 2, 0)}),
    't12_K192_d65_u_c2': (4000, 65, (3, 2), 192, 'u', {}, 259,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 12, 1, 2, 1), 'update': (0, 12, 0, 2, 1), 'stats': (0, 24, 0), 'apply': (0, 3, 2)}),
    't13_K193_d8_u_c2': (4000, 8, (3, 2), 193, 'u', {}, 260,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 13, 1, 2, 1), 'update': (1, 13, 0, 2, 1), 'stats': (0, 8, 0), 'apply': (0, 4, 1)}),
    't13_K193_d16_u_c2_dotf32': (4000, 16, (3, 2), 193, 'u', {'HMX_DOT': 'f32'}, 261,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 13, 1, 2, 1), 'update': (0, 13, 0, 2, 1), 'stats': (0, 16, 0), 'apply': (0, 4, 1)}),
    't13_K200_d68_v': (4000, 68, (4,), 200, 'v', {}, 262,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 13, 1, 2, 0), 'update': (0, 13, 0, 2, 0), 'stats': (0, 24, 0), 'apply': (0, 4, 2)}),
    't13_K208_d64_v_c2': (4000, 64, (3, 2), 208, 'v', {}, 263,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 13, 1, 2, 0), 'update': (1, 13, 0, 2, 0), 'stats': (1, 7, 1), 'apply': (1, 4, 0)}),
    't14_K209_d50_u_dotf32': (4000, 50, (4,), 209, 'u', {'HMX_DOT': 'f32'}, 264,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 0, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 14, 1, 2, 1), 'update': (0, 14, 0, 2, 1), 'stats': (0, 28, 0), 'apply': (0, 4, 1)}),
    't14_K216_d100_v': (4000, 100, (4,), 216, 'v', {}, 265,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 14, 1, 2, 0), 'update': (0, 14, 0, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 4, 2)}),
    't14_K224_d24_v': (4000, 24, (4,), 224, 'v', {}, 266,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 14, 1, 2, 0), 'update': (1, 14, 0, 2, 0), 'stats': (1, 7, 1), 'apply': (1, 2, 0)}),
    't14_K224_d96_u_c2': (4000, 96, (3, 2), 224, 'u', {}, 267,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 14, 1, 2, 1), 'update': (1, 14, 0, 2, 1), 'stats': (0, 32, 0), 'apply': (0, 4, 2)}),
    't16_K225_d1_u': (4000, 1, (4,), 225, 'u', {}, 268,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 16, 1, 2, 1), 'update': (1, 16, 0, 2, 1), 'stats': (0, 4, 0), 'apply': (0, 4, 1)}),
    't16_K232_d64_v': (4000, 64, (4,), 232, 'v', {}, 272,      # (the statistics without LDS shadows as two halves of 116 clusters: grid.y = 2)
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 16, 1, 2, 0), 'update': (1, 16, 0, 2, 0), 'stats': (1, 8, 0), 'apply': (1, 4, 0)}),
    't16_K241_d28_v_c2': (4000, 28, (3, 2), 241, 'v', {}, 269,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (1, 16, 1, 2, 0), 'update': (1, 16, 0, 2, 0), 'stats': (0, 28, 0), 'apply': (0, 4, 1)}),
    't16_K248_d128_v_c2': (4000, 128, (3, 2), 248, 'v', {}, 270,
        {'chain': 0, 'chain_pair': 0, 'usig': 0, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 0, 'host': 0},
        {'head': (0, 16, 1, 2, 0), 'update': (0, 16, 0, 2, 0), 'stats': (0, 32, 0), 'apply': (0, 4, 2)}),
    't16_K256_d48_u_c2': (4000, 48, (3, 2), 256, 'u', {}, 271,
        {'chain': 0, 'chain_pair': 0, 'usig': 1, 'upd_wps': 2, 'dot_bf': 1, 'moe_mfma': 1, 'host': 0},
        {'head': (1, 16, 1, 2, 1), 'update': (1, 16, 0, 2, 1), 'stats': (1, 8, 1), 'apply': (1, 3, 0)}),
}
CASES += sorted(LATTICE)
# the getters a case may claim (hmx_get scalars)
PATH_GETTERS = ("chain", "chain_pair", "usig", "upd_wps", "dot_bf", "sold_carry", "shuffle_inv", "need_lorder", "objslots", "upd_contig", "moe_mfma",
                "n_blocks", "cells_per_block")


def _device_cus():
    """compute units of the device, as the library's plan sees them: the chain's workgroups of a small fit (one per CU unless HMX_CHAIN_WGS says otherwise)"""
    Z, meta, _ = synth(2000, d=20, levels=(2,), seed=1)
    skw, _ = prepare_setup_args(Z, meta, "cov0", nclust=8)
    h = Harmony(seed=1)
    h.setup(**skw)
    return int(h._scalar("chain_wgs"))


@pytest.mark.parametrize("name", CASES)
def test_stages_match_the_spec(name, monkeypatch):
    t0 = time.time()
    Z, meta, var, kw, env, seed, path = _case(name, _device_cus() if name == "p_contiguous_ranges" else 256)      # (the one case sized by the CU count)
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
    for g in PATH_GETTERS:
        if g in path:
            assert int(h._scalar(g)) == path[g], (g, msg)
    if "last_block" in path:
        assert N - (path["n_blocks"] - 1) * path["cells_per_block"] == path["last_block"], msg
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
    if name in LATTICE:      # the instantiations that ran last are the ones the ledger credits the case with (tests/test_stage_ref_cpu.py holds the table to the plan)
        credit = LATTICE[name][8]
        for kind, want in credit.items():
            ran = dict(zip(RIDGE_FIELDS if kind in ("stats", "apply") else LAUNCH_FIELDS, (int(v) for v in h._get("launch:" + kind))))
            got = (ran["mfma"], ran["p0"], ran["p1"]) if kind in ("stats", "apply") else (ran["bf"], ran["nct"], ran["mode"], ran["wps"], ran["usig"])
            assert got == want, (kind, ran, msg)
        with pytest.raises(HarmonyError):
            h._get("launch:" + ("update" if "chain" in credit else "chain"))

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


# ---- the round ladder: what a round hands to the next one (stage_check.run_ladder) --------------------------------------------------------
# name -> (cells, clusters, levels, nested, environment, seed, the path it claims)
LADDERS = {
    # the carry pays by itself: 400 keys x 10 combinations x 64 <= N
    "chain": (300000, 100, (10,), False, {}, 31, dict(chain=1, chain_pair=0, sold_carry=1)),
    "launch_per_step": (300000, 100, (10,), False, {"HMX_CHAIN": "0"}, 31, dict(chain=0, chain_pair=0, sold_carry=1)),
    "wave_pair_chain": (60000, 200, (8, 64, 128), True, {"HMX_SOLD_CARRY": "1"}, 32, dict(chain=1, chain_pair=1, sold_carry=1)),
}
LADDER_ROUNDS = 5       # rounds 0..3 are one sort group, round 4 opens the next
# The chain without R stores (k_tile MODE 5) at 1 .. 6 cluster tiles: two rounds at 6000 cells with the carry forced on (it never pays by itself below 100 000
# cells); the first round of the second rung stores no R and is judged through what it hands to the second.  name -> (cells, clusters, PCs, levels, environment, seed, path)
SMALL_LADDERS = {
    "chain_1_tile_K16": (6000, 16, 50, (4,), {"HMX_SOLD_CARRY": "1"}, 41, dict(chain=1, chain_pair=0, sold_carry=1)),
    "chain_2_tiles_K17": (6000, 17, 32, (4,), {"HMX_SOLD_CARRY": "1"}, 42, dict(chain=1, chain_pair=0, sold_carry=1)),
    "chain_3_tiles_K40": (6000, 40, 64, (3, 2), {"HMX_SOLD_CARRY": "1"}, 43, dict(chain=1, chain_pair=0, sold_carry=1)),
    "chain_4_tiles_K64": (6000, 64, 17, (4,), {"HMX_SOLD_CARRY": "1"}, 44, dict(chain=1, chain_pair=0, sold_carry=1)),
    "chain_5_tiles_K65": (6000, 65, 50, (3, 2), {"HMX_SOLD_CARRY": "1"}, 45, dict(chain=1, chain_pair=0, sold_carry=1)),
    "chain_6_tiles_K92": (6000, 92, 48, (4,), {"HMX_SOLD_CARRY": "1"}, 46, dict(chain=1, chain_pair=0, sold_carry=1)),
}
SMALL_LADDER_ROUNDS = 2


def ladder_rounds(name):
    return SMALL_LADDER_ROUNDS if name in SMALL_LADDERS else LADDER_ROUNDS


def _ladder(name):
    """(Z, meta, vars_use, setup kwargs, environment, seed, path); epsilon_cluster = -1e9: the windowed check (iter > window_size) never ends a call"""
    if name in SMALL_LADDERS:
        N, K, d, levels, env, seed, path = SMALL_LADDERS[name]
        nested = False
    else:
        (N, K, levels, nested, env, seed, path), d = LADDERS[name], 50
    Z, meta, _ = synth(N, d=d, levels=levels, nested=nested, seed=seed)
    return Z, meta, ["cov%d" % i for i in range(len(levels))], dict(nclust=K, options=harmony_options(epsilon_cluster=-1e9)), env, seed, path


@pytest.mark.parametrize("name", sorted(LADDERS) + sorted(SMALL_LADDERS))
def test_round_ladder_matches_the_spec(name, monkeypatch):
    """H_m, m = 1..5: one cluster_cpp of m rounds from the same setup, seed and Y0; rung m = round m - 1 of H_m against the fp64 spec, from
    H_{m-1}'s stored R to H_m's own.  The counters must show that the rounds before the last really took the path under test.  Every one of
    the m rounds took its old contributions from sums filed before it, none from a pass over R: round 0 from init_cluster_cpp's head
    (head_pass files them, Dev::head_gather), rounds 1 .. m - 1 from the round before (Sold_next) -- carried_rounds == m, of which H_1's single
    one is the head's, so m - 1 come from a round.  min(m - 1, 4) rounds stored no R: only a round that wrote the next round's sums may elide
    its stores, and a round that the windowed check could end stores them (from the fifth on).  A dead carry reads 1 / 0 there and fails
    here instead of passing on the fresh-pass path.
    Run to run: DESIGN 3 item 5 (exact integer tables, independent of the atomics' order) and 4.5 (elided stores: bit-identical results)
    document this path as bit-reproducible, so every H_m's first round entry is asserted BITWISE equal to H_1's only one."""
    t0 = time.time()
    Z, meta, var, kw, env, seed, path = _ladder(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    skw, _ = prepare_setup_args(Z, meta, var, **kw)
    del Z

    def make_handle():
        h = Harmony(seed=seed)
        h.setup(**skw)
        return h

    h = make_handle()
    N = int(h.N)
    Y0 = h.kmeans_centers()
    del h
    orders = {}

    def order_of_round(h, r):
        if r not in orders:
            orders[r] = feistel_order(seed, r, N)
        return orders[r]

    def probe(h):
        return {g: int(h._scalar(g)) for g in ("carried_rounds", "rounds_without_R", "chain_rounds", "chain", "chain_pair", "sold_carry", "shuffle_inv")}

    rungs = run_ladder(make_handle, skw, Y0, order_of_round, rounds=ladder_rounds(name), probe=probe)
    for rung in rungs:
        print("STAGE_SPEC", "ladder_%s_rung_%d" % (name, rung["m"]), json.dumps({"err": rung, "seconds": round(time.time() - t0, 1)}, default=str))
    for rung in rungs:
        m, p, msg = rung["m"], rung["probe"], repr((name, rung))
        for g in ("chain", "chain_pair", "sold_carry"):
            assert p[g] == path[g], (g, msg)
        assert p["carried_rounds"] == m, ("rounds that took their old contributions from the pass before them (the head, then m - 1 rounds)", msg)
        assert p["carried_rounds"] - rungs[0]["probe"]["carried_rounds"] == m - 1, ("rounds that took their old contributions from the round before", msg)
        assert p["rounds_without_R"] == min(m - 1, 4), ("rounds that stored no R", msg)
        assert p["chain_rounds"] == (m if path["chain"] else 0), msg
        assert rung["R"] <= BARS["R"], msg
        assert rung["argmax"] == 0, msg
        assert rung["O"] <= BARS["tab"] and rung["E"] <= BARS["tab"], msg
        assert rung["obj"] <= BARS["obj"], msg
        assert rung["first"] == rungs[0]["first"], ("round 0 of H_%d is not round 0 of H_1 bit for bit" % m, msg, rungs[0]["first"])
