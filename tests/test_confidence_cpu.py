"""Mapping confidence without a GPU: the fp64 spec (tests/confidence_ref.py) against numpy.cov and the quadratic form, its separation of
an unseen cell type on the oracle's fit of cell_lines, honest fp32 against the distance bar, the saved reference formats, the C ABI of
include/harmony_mi355x_confidence.h against the library and harmony_amd/_lib.py, and every check the two entry points make before the device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import confidence_ref as cr  # noqa: E402
import helpers  # noqa: E402
import map_query_ref as mq  # noqa: E402
import harmony_amd  # noqa: E402
from harmony_amd import HarmonyReference, _lib, mapping_confidence  # noqa: E402

HMX_ERR_ARG, HMX_ERR_STATE, HMX_ERR_SOLVE = 1, 6, 4
SHAPES = [(1, 1, 1), (17, 3, 5), (1000, 50, 100), (4099, 68, 100), (333, 128, 256)]      # (Nq, d, K) of the GPU test


def synthetic_moments(rng, K, d):
    A = rng.standard_normal((K, d, d))
    return rng.standard_normal((K, d)), A @ A.transpose(0, 2, 1) / d + np.eye(d)


def test_status_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "harmony_mi355x.h")).read()
    for name, v in (("HMX_ERR_ARG", HMX_ERR_ARG), ("HMX_ERR_STATE", HMX_ERR_STATE), ("HMX_ERR_SOLVE", HMX_ERR_SOLVE)):
        assert re.search(r"\b%s\s*=?\s*%d\b" % (name, v), hdr), name


def test_spec_equals_numpy_cov_and_the_quadratic_form():
    rng = np.random.default_rng(1)
    K, d, N = 6, 9, 400
    R = rng.random((K, N)) ** 4
    R /= R.sum(axis=0)
    Z = rng.standard_normal((d, N)) * np.linspace(3, 0.3, d)[:, None] + 2.0
    mean, cov = cr.reference_moments(R, Z)
    for k in range(K):
        assert np.allclose(cov[k], np.cov(Z, aweights=R[k]), rtol=1e-12, atol=1e-14)
        assert np.allclose(mean[k], np.average(Z, axis=1, weights=R[k]), rtol=1e-12, atol=1e-14)
        assert np.array_equal(cov[k], cov[k].T) or np.allclose(cov[k], cov[k].T, rtol=0, atol=1e-15)
    Zq = rng.standard_normal((d, 50)) * 2 + 2.0
    for ridge in (0.0, 0.5):
        dist = cr.distances(Zq, mean, cov, ridge)
        for k in range(K):
            Y = Zq - mean[k][:, None]
            quad = np.einsum("ji,ji->i", Y, np.linalg.solve(cov[k] + ridge * np.eye(d), Y))
            assert np.abs(dist[:, k] ** 2 - quad).max() <= 1e-10 * quad.max()
        U = cr.whitening(cov, ridge)
        assert not np.triu(U, 1).any()
    Rq = rng.random((K, 50))
    assert np.allclose(cr.score(Rq, dist), [np.dot(Rq[:, i], dist[i]) for i in range(50)], rtol=1e-15)
    R0 = R.copy()
    R0[2] = 0
    with pytest.raises(ValueError, match="cluster 2"):
        cr.reference_moments(R0, Z)
    R1 = np.zeros((1, N))
    R1[0, 7] = 1.0                        # all the weight on one cell: 1 - sum w^2 = 0
    with pytest.raises(ValueError, match="cluster 0"):
        cr.reference_moments(R1, Z)


@pytest.fixture(scope="module")
def oracle_t293_fit():
    from helpers import run_backend
    from oracle.oracle import OracleHarmony
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines.npz"))
    ds = fx["dataset_levels"][fx["dataset"]]
    ct = fx["cell_type_levels"][fx["cell_type"]]
    ref = ds == "t293"
    c = OracleHarmony(accurate=True, seed=1)
    run_backend(c, fx["pcs"][ref], {"dataset": ds[ref]}, "dataset", nclust=20, max_iter=10)
    half = ds == "half"
    return c, fx["pcs"][half].T, ct[half]


def test_spec_separates_jurkat_from_293t_on_the_oracle_fit(oracle_t293_fit):
    """Reference: the t293 dataset alone (oracle fit, K = 20, seed 1), moments in the "orig" space; query: the `half` dataset, a mix of 293T
    and jurkat cells, mapped with tests/map_query_ref.py.  Measured here: the jurkat cells' scores have their 10th percentile at 27.2, the 293T
    cells' their 90th at 9.1; the reference's own cells have a median of 4.3 (d = 20: the root of a chi-square's mean is 4.5).  The unseen
    cell type sits three times as far out as the worst tenth of the seen one."""
    c, Zq, ct = oracle_t293_fit
    R, Zo, Zc = c.getR(), c.getZorig(), c.getZcorr()
    mean, cov = cr.reference_moments(R, Zo)
    Nr, Cr = mq.reference_summary(R, Zc)
    sigma = np.full(R.shape[0], 0.1)
    _, Rq = mq.map_query(Zq, [np.zeros(Zq.shape[1], dtype=int)], [1], Nr, Cr, sigma, lambda_=None)
    s = cr.score(Rq, cr.distances(Zq, mean, cov))
    own = cr.score(R, cr.distances(Zo, mean, cov))
    jur, t293 = np.percentile(s[ct == "jurkat"], 10), np.percentile(s[ct != "jurkat"], 90)
    print("jurkat p10 %.2f, 293T p90 %.2f, reference median %.2f" % (jur, t293, np.median(own)))
    assert set(ct) == {"jurkat", "t293"}
    assert jur > t293
    assert jur == pytest.approx(27.2, abs=0.5) and t293 == pytest.approx(9.1, abs=0.5) and np.median(own) == pytest.approx(4.3, abs=0.2)


@pytest.mark.parametrize("Nq,d,K", SHAPES)
def test_honest_fp32_stays_inside_the_distance_bar(Nq, d, K):
    """a plain float32 NumPy evaluation of the whitening form against the fp64 spec, in units of the bar delta: the bar is not violated by honest
    fp32 (ratio < 1) and is not vacuous (it is a small fraction of the distance)"""
    rng = np.random.default_rng(100 * d + K)
    mean, cov = synthetic_moments(rng, K, d)
    Z = rng.standard_normal((d, Nq)).astype(np.float32).astype(np.float64)
    for ridge in (0.0, 0.5):
        dist = cr.distances(Z, mean, cov, ridge)
        delta = cr.distance_bars(Z, mean, cov, ridge)
        ratio = np.abs(cr.distances_fp32(Z, mean, cov, ridge).astype(np.float64) - dist) / delta
        print("Nq %d d %d K %d ridge %.1f: fp32 error / delta max %.3f; delta / dist median %.1e max %.1e"
              % (Nq, d, K, ridge, ratio.max(), np.median(delta / dist), (delta / dist).max()))
        assert ratio.max() < 1.0
        assert np.median(delta / dist) < 1e-4


def _ref(K=5, d=7, moments=True, space=None):
    rng = np.random.default_rng(0)
    kw = {}
    if moments:
        kw["mean"], kw["cov"] = synthetic_moments(rng, K, d)
        kw["space"] = space
    return HarmonyReference(rng.random(K) * 10, rng.standard_normal((K, d)), np.full(K, 0.1), **kw)


def test_reference_formats_save_and_load(tmp_path):
    ref = _ref(space="corr")
    p = str(tmp_path / "ref2.npz")
    ref.save(p)
    assert str(np.load(p)["format"]) == "harmony_amd.reference/2"
    back = HarmonyReference.load(p)
    for f in ("Nr", "C", "sigma", "mean", "cov"):
        assert np.array_equal(getattr(back, f), getattr(ref, f)), f
    assert back.space == "corr" and _ref().space == "orig"
    old = _ref(moments=False)                     # the three-positional-argument constructor, the /1 file
    p1 = str(tmp_path / "ref1.npz")
    old.save(p1)
    assert str(np.load(p1)["format"]) == "harmony_amd.reference/1"
    back = HarmonyReference.load(p1)
    assert back.mean is None and back.cov is None and back.space is None and np.array_equal(back.C, old.C)
    np.savez(str(tmp_path / "bad.npz"), format=np.array("harmony_amd.reference/3"), Nr=ref.Nr, C=ref.C, sigma=ref.sigma)
    with pytest.raises(ValueError):
        HarmonyReference.load(str(tmp_path / "bad.npz"))
    rng = np.random.default_rng(1)
    mean, cov = synthetic_moments(rng, 5, 7)
    for kw in (dict(mean=mean), dict(cov=cov), dict(mean=mean[:4], cov=cov), dict(mean=mean, cov=cov[:, :6]), dict(mean=mean, cov=cov, space="pca"),
               dict(space="orig")):
        with pytest.raises(ValueError):
            HarmonyReference(old.Nr, old.C, old.sigma, **kw)


def test_python_errors_come_before_the_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(ValueError, match="no moments"):
        mapping_confidence(None, _ref(moments=False))
    with pytest.raises(ValueError, match="ridge"):
        mapping_confidence(None, _ref(), ridge=-1.0)
    with pytest.raises(ValueError, match="ridge"):
        mapping_confidence(None, _ref(), ridge=float("nan"))
    with pytest.raises(ValueError, match="Harmony object"):
        mapping_confidence(None, _ref())
    assert "mapping_confidence" in harmony_amd.__all__ and hasattr(harmony_amd.Harmony, "mapping_confidence")


def test_confidence_header_matches_the_library_and_the_binding():
    mine = ["hmx_reference_moments", "hmx_mapping_confidence"]
    assert helpers.header_names("harmony_mi355x_confidence.h") == set(_lib.CONFIDENCE_SIGNATURES) == set(mine)
    found = helpers.header_functions("harmony_mi355x_confidence.h")
    assert [n for n, _ in found] == mine
    helpers.assert_header_stands_alone("harmony_mi355x_confidence.h", mine)
    for n, types in found:
        helpers.assert_binding_matches(_lib.load(), n, types, _lib.CONFIDENCE_SIGNATURES[n][1])
    hdr = helpers.header_text("harmony_mi355x_confidence.h")
    assert re.search(r"#define HMX_SPACE_ORIG 0\b", hdr) and re.search(r"#define HMX_SPACE_CORR 1\b", hdr)
    assert harmony_amd.mapping.SPACES == ("orig", "corr")


def test_library_checks_arguments_and_state_before_the_device():
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    K, d = 3, 4
    rng = np.random.default_rng(0)
    mean, cov = synthetic_moments(rng, K, d)
    mean = np.asfortranarray(mean)
    score, dist = np.zeros(8), np.zeros((8, K), dtype=np.float32)
    P = lambda v: None if v is None else v.ctypes.data_as(fp if v.dtype == np.float32 else dp)  # noqa: E731

    def conf(space=0, m=mean, c=cov, K_=K, d_=d, ridge=0.0, s=score, ds=dist, handle=h):
        return lib.hmx_mapping_confidence(handle, space, P(m), P(c), K_, d_, ridge, P(s), P(ds))

    def mom(space=0, m=mean, c=cov, handle=h):
        return lib.hmx_reference_moments(handle, space, P(m), P(c))

    def refused(fn, status, **kw):
        assert fn(**kw) == status, kw
        assert len(lib.hmx_last_error(h)) > 0, kw

    bad_mean, bad_cov = mean.copy(), cov.copy()
    bad_mean[1, 2] = np.nan
    bad_cov[2, 3, 3] = np.inf
    try:
        refused(conf, HMX_ERR_ARG, space=2)
        refused(conf, HMX_ERR_ARG, space=-1)
        refused(conf, HMX_ERR_ARG, m=None)
        refused(conf, HMX_ERR_ARG, c=None)
        refused(conf, HMX_ERR_ARG, s=None)
        refused(conf, HMX_ERR_ARG, ridge=-1e-3)
        refused(conf, HMX_ERR_ARG, ridge=float("nan"))
        refused(conf, HMX_ERR_ARG, ridge=float("inf"))
        refused(conf, HMX_ERR_ARG, K_=0)
        refused(conf, HMX_ERR_ARG, d_=0)
        refused(conf, HMX_ERR_ARG, K_=257)
        refused(conf, HMX_ERR_ARG, d_=129)
        refused(conf, HMX_ERR_ARG, m=bad_mean)
        refused(conf, HMX_ERR_ARG, c=bad_cov)
        refused(conf, HMX_ERR_STATE)                        # valid arguments, but a fresh handle holds no mapped query
        refused(conf, HMX_ERR_STATE, ds=None)
        assert "hmx_map_query" in lib.hmx_last_error(h).decode()
        refused(mom, HMX_ERR_ARG, space=2)
        refused(mom, HMX_ERR_ARG, m=None)
        refused(mom, HMX_ERR_ARG, c=None)
        refused(mom, HMX_ERR_STATE)                         # a fresh handle has no fitted state
        refused(mom, HMX_ERR_STATE, space=1)
        out = (C.c_double * 1)()
        for t in (b"timer:reference_moments", b"timer:mapping_confidence"):
            assert lib.hmx_get(h, t, out, 1) == 1 and out[0] == 0.0
    finally:
        lib.hmx_destroy(h)
    assert conf(handle=None) == HMX_ERR_ARG and mom(handle=None) == HMX_ERR_ARG
