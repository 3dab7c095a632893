"""Integration metrics without a GPU: the fp64 spec (tests/metrics_ref.py) on cases computable by hand, the C ABI of
include/harmony_mi355x_metrics.h against the library and harmony_amd/_lib.py, the argument checks of harmony_amd/metrics.py (raised before
the library is loaded) and of the library (before the device is touched), and the refusal to run without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import metrics_ref as mr  # noqa: E402
import harmony_amd  # noqa: E402
from harmony_amd import _lib, metrics  # noqa: E402

HMX_ERR_ARG, HMX_ERR_DEVICE, HMX_ERR_STATE, HMX_ERR_LIMIT = 1, 5, 6, 7
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))


def test_spec_lisi_on_hand_computable_cases():
    rng = np.random.default_rng(0)
    D = np.sort(rng.random(89)) + 0.5
    assert mr.lisi_row(D, np.zeros((1, 89), int), 30)[0] == pytest.approx(1.0, abs=1e-12)          # one label: 1
    for B in (2, 5, 10):                                                                              # equal distances, B labels in equal numbers: B
        m = 10 * B
        for D, p in ((np.full(m, 0.7), float(m)), (np.zeros(m), 3.0)):      # (entropy ln m at every beta: met at once for perplexity m; never for 3, and the weights stay uniform at distance 0)
            assert mr.lisi_row(D, (np.arange(m) % B)[None], p)[0] == pytest.approx(B, rel=1e-12)
    assert mr.lisi_row(np.full(89, np.float32(1e15), dtype=np.float64), (np.arange(89) % 4)[None], 30)[0] == -1.0      # every weight underflows: H = 0 -> 1 / (-1)
    two = mr.lisi_row(np.array([1.0, 1.0, 1.0, 1.0]), np.array([[0, 0, 0, 1], [0, 1, 2, 3]]), 2.0)
    assert two[0] == pytest.approx(1.0 / (0.75 ** 2 + 0.25 ** 2)) and two[1] == pytest.approx(4.0)


def test_spec_knn_ties_duplicates_and_self_exclusion():
    X = np.array([[0.0, 0], [1, 0], [0, 1], [1, 0], [3, 3], [0, 0]])
    idx, d2 = mr.knn(X, 3)
    assert idx.tolist()[0] == [5, 1, 2] and d2[0].tolist() == [0.0, 1.0, 1.0]           # the duplicate first, then ties by index
    assert idx.tolist()[1] == [3, 0, 5] and idx.tolist()[5] == [0, 1, 2]
    idx, d2 = mr.knn(X, 2, Q=np.array([[1.0, 0]]))
    assert idx.tolist() == [[1, 3]] and d2.tolist() == [[0.0, 0.0]]
    rng = np.random.default_rng(3)                                                      # the preselection changes nothing
    Y, Q = rng.standard_normal((400, 7)), rng.standard_normal((50, 7))
    for q in (None, Q):
        i1, e1 = mr.knn(Y, 20, q, extra=1)
        D = mr.sqdist_block(mr.as_f32_f64(Y if q is None else q), mr.as_f32_f64(Y))
        if q is None:
            np.fill_diagonal(D, np.inf)
        o = np.argsort(D, axis=1, kind="stable")[:, :21]
        assert np.array_equal(i1, o) and np.array_equal(e1, np.take_along_axis(D, o, axis=1))
    win, share = mr.knn_predict(np.array([[0, 1, 2], [2, 3, 4]]), np.array([1, 1, 0, 0, 2]), 3)
    assert win.tolist() == [1, 0] and share.tolist() == [2 / 3.0, 2 / 3.0]


def test_metrics_header_matches_the_library_and_the_binding():
    met = helpers.header_names("harmony_mi355x_metrics.h")
    assert met == set(_lib.METRICS_SIGNATURES) and len(met) == 3
    found = helpers.header_functions("harmony_mi355x_metrics.h")
    assert {n for n, _ in found} == met
    helpers.assert_header_stands_alone("harmony_mi355x_metrics.h", met)
    loose = {"int32_t*": (C.c_void_p, C.POINTER(C.c_int32)), "float*": (C.c_void_p, C.POINTER(C.c_float))}      # (the outputs: host or device pointers)
    for n, types in found:
        helpers.assert_binding_matches(_lib.load(), n, types, _lib.METRICS_SIGNATURES[n][1], loose)
    assert {"knn", "compute_lisi", "lisi_from_knn", "knn_predict"} <= set(harmony_amd.__all__) and hasattr(harmony_amd.Harmony, "lisi")


def test_python_argument_errors_come_before_the_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((100, 5))
    meta = {"b": np.arange(100) % 3, "f": np.where(np.arange(100) == 7, np.nan, 1.0)}
    bad_knn = [dict(data=X, k=0), dict(data=X, k=129), dict(data=X, k=100), dict(data=X, k=5, query=rng.standard_normal((3, 4))),
               dict(data=X[0], k=1), dict(data=rng.standard_normal((10, 129)), k=1), dict(data=X, k=101, query=X)]
    for kw in bad_knn:
        with pytest.raises(ValueError):
            metrics.knn(**kw)
    for kw in (dict(perplexity=43.1), dict(perplexity=34), dict(perplexity=0), dict(label_colnames="nope"), dict(label_colnames="f"),
               dict(meta_data={"b": np.arange(99)}), dict(meta_data=np.arange(100))):       # 128 < 3 p - 1; N - 1 < 3 p - 1; ...
        args = dict(X=X, meta_data=meta, label_colnames="b", perplexity=5)
        args.update(kw)
        with pytest.raises(ValueError):
            metrics.compute_lisi(**args)
    idx, dist, lab = np.zeros((4, 3), np.int32), np.ones((4, 3), np.float32), np.zeros((1, 10), np.int32)
    for kw in (dict(idx=idx[:, :2]), dict(idx=idx + 10), dict(label_codes=lab + 2), dict(label_codes=np.full((1, 10), np.nan)), dict(n_levels=[1, 1]),
               dict(perplexity=-1.0), dict(dist=np.full((4, 3), np.nan, np.float32)), dict(idx=np.zeros((4, 129), np.int32), dist=np.ones((4, 129), np.float32))):
        args = dict(idx=idx, dist=dist, label_codes=lab, n_levels=[2], perplexity=1.5)
        args.update(kw)
        with pytest.raises(ValueError):
            metrics.lisi_from_knn(**args)
    for kw in (dict(reference_labels=np.arange(99)), dict(reference_labels=np.where(np.arange(100) == 3, np.nan, 0.0)), dict(k=0), dict(k=101)):
        args = dict(query=X[:5], reference=X, reference_labels=np.arange(100) % 2, k=5)
        args.update(kw)
        with pytest.raises(ValueError):
            metrics.knn_predict(**args)


def test_library_checks_the_envelope_before_the_device():
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    X = np.zeros((10, 4))
    idx, dist = np.zeros((10, 3), np.int32), np.zeros((10, 3), np.float32)
    xp, oi, od = C.c_void_p(X.ctypes.data), C.c_void_p(idx.ctypes.data), C.c_void_p(dist.ctypes.data)
    lab, nl, out = np.zeros(10, np.int32), np.array([1], np.int32), np.zeros(10)
    try:
        k = lambda *a: lib.hmx_knn(h, *a)  # noqa: E731
        assert k(xp, 0, 0, 10, None, 0, 0, 0, 4, 0, oi, od, 0) == HMX_ERR_ARG
        assert k(xp, 0, 0, 10, None, 0, 0, 0, 4, 10, oi, od, 0) == HMX_ERR_LIMIT           # k <= N - 1 with self excluded
        assert k(xp, 0, 0, 10, xp, 0, 0, 10, 4, 11, oi, od, 0) == HMX_ERR_LIMIT
        assert k(xp, 0, 0, 10, None, 0, 0, 0, 129, 3, oi, od, 0) == HMX_ERR_LIMIT
        assert k(xp, 0, 0, 1000, None, 0, 0, 0, 4, 129, oi, od, 0) == HMX_ERR_LIMIT
        assert k(xp, 2, 0, 10, None, 0, 0, 0, 4, 3, oi, od, 0) == HMX_ERR_ARG
        assert k(None, 0, 0, 10, None, 0, 0, 0, 4, 3, oi, od, 0) == HMX_ERR_ARG
        assert k(xp, 0, 0, 10, None, 0, 0, 0, 4, 3, oi, None, 0) == HMX_ERR_ARG
        assert b"envelope" in lib.hmx_last_error(h) or len(lib.hmx_last_error(h)) > 0
        li = lambda i, m, lb, p: lib.hmx_lisi(h, i.ctypes.data_as(ip), dist.ctypes.data_as(fp), 10, m, lb.ctypes.data_as(ip), 10, 1,  # noqa: E731
                                              nl.ctypes.data_as(ip), p, out.ctypes.data_as(dp))
        assert li(idx, 129, lab, 1.5) == HMX_ERR_LIMIT
        assert li(idx + 10, 3, lab, 1.5) == HMX_ERR_ARG
        assert li(idx, 3, lab + 1, 1.5) == HMX_ERR_ARG
        assert li(idx, 3, lab, 0.0) == HMX_ERR_ARG
        cl = lambda x, n, p: lib.hmx_compute_lisi(h, x, 0, 0, n, 4, lab.ctypes.data_as(ip), 1, nl.ctypes.data_as(ip), p, out.ctypes.data_as(dp))  # noqa: E731
        assert cl(xp, 10, 30.0) == HMX_ERR_LIMIT and cl(xp, 10, 43.1) == HMX_ERR_LIMIT
        assert cl(None, 10, 2.0) == HMX_ERR_STATE                                           # no embedding on a fresh handle
        outv = (C.c_double * 1)()
        assert lib.hmx_get(h, b"timer:knn", outv, 1) == 1 and outv[0] == 0.0 and lib.hmx_get(h, b"timer:lisi", outv, 1) == 1
    finally:
        lib.hmx_destroy(h)
    assert lib.hmx_knn(None, xp, 0, 0, 10, None, 0, 0, 0, 4, 3, oi, od, 0) == HMX_ERR_ARG


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_no_cpu_fallback():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((200, 6))
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        metrics.knn(X, 5)
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        metrics.compute_lisi(X, {"b": np.arange(200) % 2}, "b", perplexity=10)
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        metrics.lisi_from_knn(np.zeros((5, 3), np.int32), np.ones((5, 3), np.float32), np.zeros(10, np.int32), [1], 1.5)
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        metrics.knn_predict(X[:5], X, np.arange(200) % 3, k=5)
