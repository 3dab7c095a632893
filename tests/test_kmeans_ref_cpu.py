"""The fp64 spec of kmeans_centers (tests/kmeans_ref.py) anchored to the CPU oracle, and the committed GPU cases of tests/test_gpu_kmeans.py held to what they claim
before a GPU sees them: every case is clear, the fp32 oracle reaches the spec's cells and centres on it, and the ledger credits it with the launches the table names."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kmeans_ref  # noqa: E402
import stage_lattice as lattice  # noqa: E402
import test_gpu_kmeans as gpu_kmeans  # noqa: E402
from harmony_amd import prepare_setup_args  # noqa: E402
from oracle.oracle import OracleHarmony, load  # noqa: E402

# The oracle's centres against the spec's, normalised, max-abs: the last mean rounded to fp32 (half an ulp) and the oracle's fp32 normalisation -- a sum of d squares
# (d / 2 ulps of the norm at worst), the root and the division -- on entries of at most 1.  Measured over the committed cases: 5.0e-8 .. 2.3e-7.
def oracle_bar(d):
    return (d / 2 + 3) * 2.0 ** -24


def test_uniforms_are_the_oracles():
    lib = load()
    rng = np.random.default_rng(0)
    args = [(0, 0, 0), (1, 0, 1), (17, 5, 123456), (2 ** 40 + 3, 257, 2 ** 33), (2 ** 63 + 11, 2 ** 31, 2 ** 40)]
    args += [tuple(int(v) for v in rng.integers(0, 2 ** 62, size=3)) for _ in range(200)]
    for seed, stream, idx in args:
        assert float(kmeans_ref.u01(seed, stream, [idx])[0]) == lib.orc_u01(seed, stream, idx), (seed, stream, idx)
    u = kmeans_ref.u01(3, 1, np.arange(100000))
    assert u.dtype == np.float32 and 0.0 < u.min() and u.max() <= 1.0 and abs(float(u.mean()) - 0.5) < 0.01


@pytest.mark.parametrize("name", sorted(gpu_kmeans.CASES))
def test_committed_case_is_clear_and_the_oracle_reaches_the_spec(name):
    N, d, K, _levels, env, dseed, seed_credit, lloyd_credit = gpu_kmeans.CASES[name]
    Z, meta, var, kw, _ = gpu_kmeans.case_data(name)
    skw, _ = prepare_setup_args(Z, meta, var, **kw)
    assert N == (1100 if _levels == "own" else max(4 * K, 640)) and Z.shape == (N, d)
    cells, dist, s = gpu_kmeans.oracle_distance(skw, dseed, lambda X: kmeans_ref.kmeans_centers(X, K, dseed))
    print("KMEANS_ORACLE", name, {"oracle": dist, "race_clear": float(s["race_clear"].min()), "race_gap": float(s["race_gap"].min()),
                                  "lloyd_clear": float(s["lloyd_clear"].min()), "lloyd_gap": float(s["lloyd_gap"].min()), "empty": len(s["empty"])})
    assert kmeans_ref.is_clear(s), (s["race_clear"].min(), s["lloyd_clear"].min())
    assert np.array_equal(cells, s["seed_cells"]) and len(set(cells.tolist())) == K
    assert dist <= oracle_bar(d), dist
    # the launches the table credits the case with are the ledger's, for the case's own design
    _N, _K, shape, items = lattice.shape_of(skw)
    by = {kind: v for v, kind in lattice.launches(N, K, shape, items, env, "kmeans")[0].items()}
    assert by["seed"][1:4] == seed_credit + (3,)
    assert (by["lloyd"] == ("k_lloyd",)) if lloyd_credit == "k_lloyd" else (by["lloyd"][1], by["lloyd"][2], by["lloyd"][4], by["lloyd"][3]) == lloyd_credit + (2,)
    # teeth: one cell of the last iteration sent to its second-best centre moves the normalised centres by far more than any bar a GPU case can have
    X = skw["Z"].T / np.linalg.norm(skw["Z"].T, axis=1, keepdims=True)
    wrong = s["last_assign"].copy()
    wrong[N // 2] = s["last_second"][N // 2]
    moved = np.abs(kmeans_ref.normalised(kmeans_ref.centers_after(X, s, wrong)) - kmeans_ref.normalised(kmeans_ref.centers_after(X, s, s["last_assign"]))).max()
    assert moved > 100 * max(2 * oracle_bar(d), gpu_kmeans.CENTRE_FLOOR), moved


def test_spec_passes_over_taken_cells_like_the_oracle():
    """more clusters than places to win (tests/test_gpu_parity2.py::test_kmeans_duplicate_winner_resample): the spec's re-draws are the oracle's"""
    Z, meta = gpu_kmeans.tight_groups(6, 5)
    skw, _ = prepare_setup_args(Z, meta, "b", nclust=40)
    for seed in (1, 2, 3):
        c = OracleHarmony(accurate=True, seed=seed)
        c.setup(**skw)
        X = c.getZcorr().T
        c.init_cluster_cpp()
        s = kmeans_ref.kmeans_centers(X, 40, seed)
        assert np.array_equal(c._get("seed_cells").astype(np.int64), s["seed_cells"]) and len(set(s["seed_cells"].tolist())) == 40
        first = np.array([np.argmin(-np.log(kmeans_ref.u01(seed, 1 + i, np.arange(60)).astype(np.float64)) / np.abs(2 * (1 - X @ X[s["anchors"][i]]))) for i in range(40)])
        assert len(set(first.tolist())) < 40        # (some cluster's first winner was taken: the pass-over ran)
