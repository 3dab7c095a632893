"""kmeans_centers on the GPU -- the seeding race (k_tile MODE 3), ten Lloyd iterations (MODE 2, or k_lloyd where the sum table does not fit LDS) -- against the
fp64 spec tests/kmeans_ref.py, one case per instantiation of both kernels that the coverage ledger (tests/stage_lattice.py) lists: 13 cluster-tile counts in the
split-bf16 and the fp32 build, the three-wave Lloyd at 5 .. 7 cluster tiles, k_lloyd.  Every case is CLEAR: each discrete decision of the spec -- a race's winner,
a cell's centre in every iteration -- lies at least twice its fp32 rounding bound from the next candidate (tests/test_kmeans_ref_cpu.py asserts it for every
committed case, on the CPU), so the chosen cells must be the spec's exactly, and the centres differ by rounding alone.
What a case would catch: one cell sent to the wrong centre by the three-wave Lloyd k_tile<6, 2, 3> reaches only three_waves_t06_K96_d64; with about eleven cells per
cluster the two centres involved move by |x - y| / 11, some 1e-2 after normalisation, against a bar of 2.6e-7 (tests/test_kmeans_ref_cpu.py measures this move for
every case: more than 100 bars).
And the R-compatible stream's race in several anchor batches against the oracle."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kmeans_ref  # noqa: E402
from helpers import synth  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (cells, PCs, clusters, levels -- "own": a level per cell, so every cell has a 16-cell tile of its own and 1100 cells make the > 1024 static tiles at
# which two Lloyd workgroups would share a CU --, environment, data seed, (bf, nct) of the seeding race, the Lloyd launch (bf, nct, wps) or "k_lloyd").
# N = max(4 K, 640): the smallest margin over N cells x 10 iterations stays above twice the bound for the data seeds searched on the CPU (tools/make_kmeans_cases.py).
CASES = {
    'bf_t01_K16_d16': (640, 16, 16, (2,), {}, 1, (1, 1), (1, 1, 2)),
    'bf_t02_K17_d8': (640, 8, 17, (2,), {}, 1, (1, 2), (1, 2, 2)),
    'bf_t03_K40_d20': (640, 20, 40, (2,), {}, 1, (1, 3), (1, 3, 2)),
    'bf_t04_K64_d32': (640, 32, 64, (2,), {}, 2, (1, 4), (1, 4, 2)),
    'bf_t05_K65_d16': (640, 16, 65, (2,), {}, 1, (1, 5), (1, 5, 2)),
    'bf_t06_K92_d24': (640, 24, 92, (2,), {}, 1, (1, 6), (1, 6, 2)),
    'bf_t07_K112_d50': (640, 50, 112, (2,), {}, 1, (1, 7), (1, 7, 2)),
    'bf_t08_K113_d17': (640, 17, 113, (2,), {}, 4, (1, 8), (1, 8, 2)),
    'bf_t10_K150_d32': (640, 32, 150, (2,), {}, 3, (1, 10), (1, 10, 2)),
    'bf_t12_K192_d20': (768, 20, 192, (2,), {}, 1, (1, 12), (1, 12, 2)),
    'bf_t13_K200_d50': (800, 50, 200, (2,), {}, 2, (1, 13), (1, 13, 2)),
    'bf_t14_K209_d16': (836, 16, 209, (2,), {}, 2, (1, 14), (1, 14, 2)),
    'bf_t16_K256_d28': (1024, 28, 256, (2,), {}, 2, (1, 16), (1, 16, 2)),
    'bf_t10_K129_d12': (640, 12, 129, (2,), {}, 1, (1, 10), (1, 10, 2)),
    'f32_t16_K225_d100_image_over_lds': (900, 100, 225, (2,), {}, 45, (0, 16), 'k_lloyd'),
    'f32_t01_K8_d16': (640, 16, 8, (2,), {'HMX_DOT': 'f32'}, 2, (0, 1), (0, 1, 2)),
    'f32_t02_K32_d68': (640, 68, 32, (2,), {}, 2, (0, 2), (0, 2, 2)),
    'f32_t03_K33_d20': (640, 20, 33, (2,), {'HMX_DOT': 'f32'}, 1, (0, 3), (0, 3, 2)),
    'f32_t04_K49_d8': (640, 8, 49, (2,), {'HMX_DOT': 'f32'}, 1, (0, 4), (0, 4, 2)),
    'f32_t05_K80_d17': (640, 17, 80, (2,), {'HMX_DOT': 'f32'}, 1, (0, 5), (0, 5, 2)),
    'f32_t06_K81_d76': (640, 76, 81, (2,), {}, 1, (0, 6), (0, 6, 2)),
    'f32_t07_K97_d32': (640, 32, 97, (2,), {'HMX_DOT': 'f32'}, 2, (0, 7), (0, 7, 2)),
    'f32_t08_K128_d16': (640, 16, 128, (2,), {'HMX_DOT': 'f32'}, 1, (0, 8), (0, 8, 2)),
    'f32_t10_K145_d24': (640, 24, 145, (2,), {'HMX_DOT': 'f32'}, 1, (0, 10), (0, 10, 2)),
    'f32_t12_K177_d68': (708, 68, 177, (2,), {}, 2, (0, 12), (0, 12, 2)),
    'f32_t13_K208_d20': (832, 20, 208, (2,), {'HMX_DOT': 'f32'}, 1, (0, 13), (0, 13, 2)),
    'f32_t14_K224_d16': (896, 16, 224, (2,), {'HMX_DOT': 'f32'}, 1, (0, 14), (0, 14, 2)),
    'f32_t16_K241_d32': (964, 32, 241, (2,), {'HMX_DOT': 'f32'}, 1, (0, 16), (0, 16, 2)),
    'three_waves_t05_K65_d80': (1100, 80, 65, 'own', {}, 27, (1, 5), (1, 5, 3)),
    'three_waves_t06_K96_d64': (1100, 64, 96, 'own', {}, 5, (1, 6), (1, 6, 3)),
    'three_waves_t07_K112_d50': (1100, 50, 112, 'own', {}, 12, (1, 7), (1, 7, 3)),
    'k_lloyd_K256_d64': (1024, 64, 256, (2,), {}, 3, (1, 16), 'k_lloyd'),
    'k_lloyd_K256_d128': (1024, 128, 256, (2,), {}, 152, (0, 16), 'k_lloyd'),
}
# Normalised centres against the spec, max-abs: within twice the fp32 oracle's distance on the same case, and no tighter than four ulps of a unit-norm entry.
# Measured over the cases: the oracle (centres rounded to fp32 every iteration, fp32 normalisation) 6.1e-8 .. 2.1e-7; the GPU (fixed-point sums, centres in fp32) 1.8e-8 .. 3.3e-8.
CENTRE_FLOOR = 2.0 ** -22


def case_data(name):
    """(Z, meta, vars_use, setup kwargs, environment) of a case"""
    N, d, K, levels, env, dseed = CASES[name][:6]
    Z, meta, _ = synth(N, d=d, levels=(2,) if levels == "own" else levels, seed=dseed)
    if levels == "own":
        meta = {"cov0": np.arange(N)}
    return Z, meta, "cov0", dict(nclust=K), env


def oracle_distance(skw, seed, spec_of):
    """the fp32 oracle's kmeans_centers on the same setup: (its seed cells, max-abs distance of its normalised centres from the spec on ITS cells)"""
    from oracle.oracle import OracleHarmony
    c = OracleHarmony(accurate=True, seed=seed)
    c.setup(**skw)
    X = c.getZcorr().T
    c.init_cluster_cpp()             # kmeans_centers + normalise
    s = spec_of(X)
    return c._get("seed_cells").astype(np.int64), float(np.abs(c.Y.T - kmeans_ref.normalised(s["centers"])).max()), s


@pytest.mark.parametrize("name", sorted(CASES))
def test_kmeans_centers_match_the_spec(name, monkeypatch):
    from harmony_amd import Harmony, HarmonyError, prepare_setup_args
    from test_plan_cpu import LAUNCH_FIELDS
    for k in [k for k in os.environ if k.startswith("HMX_")]:
        monkeypatch.delenv(k)
    N, d, K, _levels, _env, dseed, seed_credit, lloyd_credit = CASES[name]
    Z, meta, var, kw, env = case_data(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    skw, _ = prepare_setup_args(Z, meta, var, **kw)
    g = Harmony(seed=dseed)
    g.setup(**skw)
    X = g.getZcorr().T
    Yg = g.kmeans_centers().T
    s = kmeans_ref.kmeans_centers(X, K, dseed)
    sc_o, dist_o, _ = oracle_distance(skw, dseed, lambda Xo: kmeans_ref.kmeans_centers(Xo, K, dseed))
    dist_g = float(np.abs(kmeans_ref.normalised(Yg) - kmeans_ref.normalised(s["centers"])).max())
    moved = np.where(g._get("seed_cells").astype(np.int64) != s["seed_cells"])[0]
    print("KMEANS_SPEC", name, {"gpu": dist_g, "oracle": dist_o, "race_clear": float(s["race_clear"].min()), "lloyd_clear": float(s["lloyd_clear"].min()),
                                "seed_cells_off": moved.tolist()})
    # the instantiations the ledger credits the case with are the ones that ran
    ran = dict(zip(LAUNCH_FIELDS, (int(v) for v in g._get("launch:seed"))))
    assert (ran["bf"], ran["nct"], ran["mode"]) == seed_credit + (3,), ran
    if lloyd_credit == "k_lloyd":
        with pytest.raises(HarmonyError):
            g._get("launch:lloyd")       # no Lloyd launch of the tile kernel
    else:
        ran = dict(zip(LAUNCH_FIELDS, (int(v) for v in g._get("launch:lloyd"))))
        assert (ran["bf"], ran["nct"], ran["wps"], ran["mode"]) == lloyd_credit + (2,), ran
    assert kmeans_ref.is_clear(s), (name, s["race_clear"].min(), s["lloyd_clear"].min())      # (on the handle's own cells: they are the oracle's up to an ulp)
    assert moved.size == 0, (name, moved)
    assert np.array_equal(sc_o, s["seed_cells"]), name
    assert dist_g <= max(2.0 * dist_o, CENTRE_FLOOR), (name, dist_g, dist_o)


def tight_groups(groups, d, seed=5):
    """the data of tests/test_gpu_parity2.py::test_kmeans_duplicate_winner_resample: tight groups of 10 cells -- far more anchors than distinct places to win"""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(groups, d))
    Z = np.repeat(base, 10, axis=0) + 1e-3 * rng.normal(size=(10 * groups, d))
    return Z, {"b": np.arange(10 * groups) % 2}


def test_r_stream_race_in_three_anchor_batches():
    """rng = "R": the host draws the uniforms for A = min(K, 64 MB / 4 n, 12288 / d) anchors at a time.  d = 128, K = 200: batches of 96, 96 and 8 anchors, so the second
    and third batch race at an offset (a0 > 0), and their duplicates are raced again at i - a0 with the cells taken so far excluded -- 200 winners among 300 cells in
    30 tight groups collide in every batch.  The chosen cells must be the oracle's, cell for cell."""
    from harmony_amd import Harmony, prepare_setup_args
    from oracle.oracle import OracleHarmony
    K, d = 200, 128
    assert (12288 // d, K - 2 * (12288 // d)) == (96, 8)
    Z, meta = tight_groups(30, d)
    skw, _ = prepare_setup_args(Z, meta, "b", nclust=K)
    for seed in (1, 2):
        g = Harmony(seed=seed, rng="R")
        g.setup(**skw)
        g.kmeans_centers()
        c = OracleHarmony(accurate=True, seed=seed, rng=1)
        c.setup(**skw)
        c.init_cluster_cpp()
        sg, sc = g._get("seed_cells").astype(np.int64), c._get("seed_cells").astype(np.int64)
        assert len(set(sc.tolist())) == K
        assert np.array_equal(sg, sc), (seed, np.where(sg != sc)[0])
