"""Mapping confidence on the MI355X: hmx_mapping_confidence (distances and score of a mapped query) and hmx_reference_moments (one handle and
two virtual shards) against the fp64 spec (tests/confidence_ref.py) within its derived error bars, reproducibility, the state rules of the two
entry points, and the whole workflow on cell_lines: a cell type the reference never saw scores far above the ones it did."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import confidence_ref as cr  # noqa: E402
from harmony_amd import Harmony, HarmonyError, HarmonyReference, _lib, map_query, mapping_confidence, prepare_setup_args  # noqa: E402
from harmony_amd.utils import harmonize  # noqa: E402
from helpers import synth  # noqa: E402

pytestmark = pytest.mark.gpu

HMX_ERR_ARG, HMX_ERR_SOLVE, HMX_ERR_STATE = 1, 4, 6


def fit(Z, meta, var, K, seed=1, max_iter=3):
    skw, _ = prepare_setup_args(Z, meta, var, nclust=K)
    h = Harmony(seed=seed)
    h.setup(**skw)
    h.init_cluster_cpp()
    harmonize(h, max_iter, verbose=False)
    return h


def random_reference(rng, K, d, space="orig"):
    A = rng.standard_normal((K, d, d))
    return HarmonyReference(rng.random(K) * 100 + 1, rng.standard_normal((K, d)), np.full(K, 0.1) * (1 + rng.random(K)),
                            mean=rng.standard_normal((K, d)), cov=A @ A.transpose(0, 2, 1) / d + np.eye(d), space=space)


def check_confidence(obj, ref, ridge=0.0):
    """distances within delta of the spec, the score equal to the fp64 sum of getR() x the returned distances"""
    score, dist = obj.mapping_confidence(ref, ridge=ridge, return_dist=True)
    Z = obj.getZorig() if ref.space == "orig" else obj.getZcorr()
    R = obj.getR()
    want = cr.distances(Z, ref.mean, ref.cov, ridge)
    delta = cr.distance_bars(Z, ref.mean, ref.cov, ridge)
    ratio = np.abs(dist.astype(np.float64) - want) / delta
    print("Nq %d d %d K %d %s ridge %.1f: |dist - spec| / delta max %.3f" % (dist.shape[0], Z.shape[0], dist.shape[1], ref.space, ridge, ratio.max()))
    assert dist.dtype == np.float32 and dist.shape == (Z.shape[1], ref.K) and score.shape == (Z.shape[1],)
    assert ratio.max() <= 1.0
    mine = cr.score(R, dist)
    rel = np.abs(score - mine).max() / np.abs(mine).max()
    print("   score vs sum_k float64(R) float64(dist): %.2e relative" % rel)
    assert np.abs(score - mine).max() <= 1e-12 * np.abs(mine).max()
    return score, dist


@pytest.mark.parametrize("Nq,d,K,levels", [(1, 1, 1, 1), (17, 3, 5, 1), (1000, 50, 100, 3), (4099, 68, 100, 1), (333, 128, 256, 1)])
def test_distances_and_score_against_the_spec(Nq, d, K, levels):
    rng = np.random.default_rng(1000 * K + d)
    ref = random_reference(rng, K, d)
    Zq = rng.standard_normal((Nq, d)).astype(np.float32)
    meta = {"b": np.arange(Nq) % levels}
    obj = map_query(Zq, meta, ref, vars_use="b", lambda_=1.0, return_object=True)
    assert np.array_equal(obj.getZorig(), Zq.T.astype(np.float64))
    score, dist = check_confidence(obj, ref)
    # dist = NULL and a second call: the same bits
    assert np.array_equal(obj.mapping_confidence(ref), score)
    s2, d2 = obj.mapping_confidence(ref, return_dist=True)
    assert np.array_equal(s2, score) and np.array_equal(d2, dist)
    assert obj.timer("mapping_confidence") > 0


@pytest.fixture(scope="module")
def two_covariate_query():
    rng = np.random.default_rng(5)
    K, d, Nq = 100, 50, 1000
    ref = random_reference(rng, K, d)
    Zq = rng.standard_normal((Nq, d)).astype(np.float32)
    meta = {"q0": rng.integers(0, 4, Nq), "q1": rng.integers(0, 3, Nq)}      # 12 combinations: the internal order is not the given one
    return map_query(Zq, meta, ref, vars_use=["q0", "q1"], lambda_=1.0, return_object=True), ref


def test_two_covariates_results_come_back_in_the_given_order(two_covariate_query):
    obj, ref = two_covariate_query
    check_confidence(obj, ref)


def test_corr_space_and_ridge(two_covariate_query):
    obj, ref = two_covariate_query
    corr = HarmonyReference(ref.Nr, ref.C, ref.sigma, mean=ref.mean, cov=ref.cov, space="corr")
    s_orig = obj.mapping_confidence(ref)
    s_corr, _ = check_confidence(obj, corr)
    assert not np.array_equal(s_orig, s_corr)
    s_ridge, _ = check_confidence(obj, ref, ridge=0.5)
    assert (s_ridge < s_orig).all()                   # a larger covariance: every distance shrinks
    assert np.array_equal(mapping_confidence(obj, ref, ridge=0.5), s_ridge)
    assert np.array_equal(obj.getZcorr(), obj.getZcorr())


def check_moments(ref, R, Z, factor=1.0, against=None):
    mean, cov = cr.reference_moments(R, Z)
    mean_bar, cov_bar = cr.moment_bars(R, Z, cov)
    if against is not None:
        mean, cov = against
    rm, rc = np.abs(ref.mean - mean) / mean_bar, np.abs(ref.cov - cov) / cov_bar
    print("N %d d %d K %d %s: |mean - spec| / bar max %.3f, |cov - spec| / bar max %.3f" % (Z.shape[1], Z.shape[0], R.shape[0], ref.space, rm.max(), rc.max()))
    assert rm.max() <= factor and rc.max() <= factor
    assert np.array_equal(ref.cov, ref.cov.transpose(0, 2, 1))


@pytest.mark.parametrize("N,d,K,max_iter", [(1000, 50, 20, 3), (3001, 68, 100, 2), (2000, 5, 7, 3)])
def test_moments_against_the_spec(N, d, K, max_iter):
    Z, meta, _ = synth(N, d=d, levels=(3,), seed=11)
    h = fit(Z, meta, "cov0", K, seed=2, max_iter=max_iter)
    R = h.getR()
    for space, rows in (("orig", h.getZorig()), ("corr", h.getZcorr())):
        ref = h.reference_summary(moments=space)
        assert ref.space == space and ref.mean.shape == (K, d) and ref.cov.shape == (K, d, d)
        check_moments(ref, R, rows)
        again = h.reference_summary(moments=space)
        assert np.array_equal(again.mean, ref.mean) and np.array_equal(again.cov, ref.cov)      # fixed-order fold: bit-reproducible
    plain = h.reference_summary()
    assert plain.mean is None and np.array_equal(plain.Nr, ref.Nr) and np.array_equal(plain.C, ref.C)
    assert h.timer("reference_moments") > 0
    assert np.array_equal(h.getR(), R)                # the handle is left as it was


def test_moments_on_two_virtual_shards():
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    Z, meta, _ = synth(30000, d=50, levels=(10,), seed=21)
    K, seed, G, N = 100, 4, 2, Z.shape[0]
    one = fit(Z, meta, "cov0", K, seed=seed, max_iter=3)
    ref1 = one.reference_summary(moments="orig")
    bounds = [(0, N // 2), (N // 2, N)]
    N_b = np.bincount(meta["cov0"]).astype(float)
    barrier = threading.Barrier(G)
    slots, out, errors = [None] * G, [None] * G, []

    def hook_for(rank):
        def hook(user, buf, count, dtype, stream):
            assert hip.hipDeviceSynchronize() == 0
            host = np.empty(count, dtype=np.float64 if dtype == 1 else np.int64)
            assert hip.hipMemcpy(host.ctypes.data, buf, host.nbytes, 2) == 0
            slots[rank] = host
            barrier.wait()
            st = np.stack(slots)
            red = st.min(axis=0) if dtype == 2 else st.sum(axis=0)
            barrier.wait()
            assert hip.hipMemcpy(buf, red.ctypes.data, red.nbytes, 1) == 0
            barrier.wait()
            return 0
        return hook

    def work(rank):
        try:
            lo, hi = bounds[rank]
            skw, _ = prepare_setup_args(Z[lo:hi], {k: v[lo:hi] for k, v in meta.items()}, "cov0", nclust=K, N_b=N_b,
                                        levels={"cov0": np.arange(len(N_b))})
            g = Harmony(seed=seed)
            g.set_shard(rank, G, lo, N, hook_for(rank))
            g.setup(**skw)
            g.init_cluster_cpp()
            harmonize(g, 3, verbose=False)
            out[rank] = (g.reference_summary(moments="orig"), g.getR(), g.getZorig())
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(G)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    a, b = out[0][0], out[1][0]
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.cov, b.cov)           # every rank gets the global moments
    R, Zo = np.concatenate([o[1] for o in out], axis=1), np.concatenate([o[2] for o in out], axis=1)
    check_moments(a, R, Zo)                                                            # the spec over the shards' own R and rows
    check_moments(a, one.getR(), one.getZorig(), factor=2.0, against=(ref1.mean, ref1.cov))      # the one-handle result: two orders of summation


def test_state_rules_and_failures(two_covariate_query):
    obj, ref = two_covariate_query
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    K, d = ref.K, ref.d
    mean, cov = np.asfortranarray(ref.mean), np.ascontiguousarray(ref.cov)
    score = np.zeros(obj.N)

    def conf(h, m=mean, c=cov, K_=K, d_=d):
        return lib.hmx_mapping_confidence(h, 0, m.ctypes.data_as(dp), c.ctypes.data_as(dp), K_, d_, 0.0, score.ctypes.data_as(dp), None)

    Z, meta, _ = synth(2000, d=50, levels=(2,), seed=1)
    fresh = Harmony()
    assert conf(fresh._h) == HMX_ERR_STATE
    fitted = fit(Z, meta, "cov0", 100, max_iter=1)
    assert conf(fitted._h) == HMX_ERR_STATE and "hmx_map_query" in lib.hmx_last_error(fitted._h).decode()
    m2, c2 = np.zeros((K, d), order="F"), np.zeros((K, d, d))
    assert lib.hmx_reference_moments(obj._h, 0, m2.ctypes.data_as(dp), c2.ctypes.data_as(dp)) == HMX_ERR_STATE
    with pytest.raises(HarmonyError):
        obj.reference_summary(moments="orig")
    # a wrong K or d
    assert conf(obj._h, m=np.asfortranarray(mean[:K - 1]), c=cov[:K - 1], K_=K - 1) == HMX_ERR_ARG
    assert conf(obj._h, m=np.asfortranarray(mean[:, :d - 1]), c=np.ascontiguousarray(cov[:, :d - 1, :d - 1]), d_=d - 1) == HMX_ERR_ARG
    small = HarmonyReference(ref.Nr[:5], ref.C[:5], ref.sigma[:5], mean=ref.mean[:5], cov=ref.cov[:5])
    with pytest.raises(ValueError):
        obj.mapping_confidence(small)
    with pytest.raises(ValueError):
        obj.mapping_confidence(HarmonyReference(ref.Nr, ref.C, ref.sigma))
    # a covariance with a negative eigenvalue: the cluster is named
    bad = cov.copy()
    bad[37] = np.eye(d)
    bad[37, 3, 3] = -1.0
    assert conf(obj._h, c=bad) == HMX_ERR_SOLVE and "cluster 37" in lib.hmx_last_error(obj._h).decode()
    with pytest.raises(HarmonyError, match="cluster 37"):
        obj.mapping_confidence(HarmonyReference(ref.Nr, ref.C, ref.sigma, mean=ref.mean, cov=bad))
    # ... and the handle still serves its results
    assert np.isfinite(obj.getZcorr()).all() and obj.getZcorr().shape == (d, obj.N)
    assert conf(obj._h) == 0 and np.isfinite(score).all() and (score > 0).all()


def test_cell_lines_unseen_cell_type_scores_high(tmp_path):
    """Reference: the t293 dataset alone (K = 20, seed 1), moments in the "orig" space, saved and loaded; query: the `half` dataset (293T and
    jurkat cells).  The 10th percentile of the jurkat cells' scores exceeds the 90th percentile of the 293T cells' (the fp64 spec on the
    oracle's fit: 27.2 against 9.1, tests/test_confidence_cpu.py)."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines.npz"))
    ds = fx["dataset_levels"][fx["dataset"]]
    ct = fx["cell_type_levels"][fx["cell_type"]]
    sel = ds == "t293"
    skw, _ = prepare_setup_args(fx["pcs"][sel], {"dataset": ds[sel]}, "dataset", nclust=20)
    h = Harmony(seed=1)
    h.setup(**skw)
    h.init_cluster_cpp()
    harmonize(h, 10, verbose=False)
    p = str(tmp_path / "t293.npz")
    h.reference_summary(moments="orig").save(p)
    ref = HarmonyReference.load(p)
    assert ref.space == "orig" and ref.mean.shape == (20, fx["pcs"].shape[1])
    half = ds == "half"
    obj = map_query(fx["pcs"][half], None, ref, return_object=True)
    s = mapping_confidence(obj, ref)
    jur, t293 = np.percentile(s[ct[half] == "jurkat"], 10), np.percentile(s[ct[half] != "jurkat"], 90)
    print("jurkat p10 %.2f, 293T p90 %.2f" % (jur, t293))
    assert jur > t293
