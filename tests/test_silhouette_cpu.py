"""Silhouette widths without a GPU: the fp64 spec (tests/silhouette_ref.py) against sklearn and on hand-made cases, the C ABI of
include/harmony_mi355x_silhouette.h against the library and harmony_amd/_lib.py, the argument checks of harmony_amd/silhouette.py (raised
before the library is loaded) and of the library (before the device is touched), and the refusal to run without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import silhouette_ref as sr  # noqa: E402
import harmony_amd  # noqa: E402
from harmony_amd import _lib, silhouette  # noqa: E402

HMX_ERR_ARG, HMX_ERR_DEVICE, HMX_ERR_STATE, HMX_ERR_LIMIT = 1, 5, 6, 7
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))


def spec_case():
    """300 x 7, 4 labels of which one is a singleton, one duplicated row (under another label than its original)"""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((300, 7)).astype(np.float32).astype(np.float64)
    lab = rng.integers(0, 3, 300)
    lab[17] = 3                                   # the singleton
    X[200] = X[5]
    lab[5], lab[200] = 0, 1
    X[201] = X[6]                                 # ... and one under its original's label
    lab[6] = lab[201] = 2
    return X, lab


def test_spec_equals_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    X, lab = spec_case()
    s, a, b = sr.silhouette(X, lab)
    want = skm.silhouette_samples(X, lab, metric="euclidean")
    assert np.abs(s - want).max() <= 1e-12
    assert s[17] == 0.0 and a[17] == 0.0 and b[17] > 0
    assert np.all(np.isfinite(s)) and np.all(a >= 0) and np.all(b > 0)
    m = np.maximum(a, b)
    assert np.abs(s - (b - a) / m)[np.arange(300) != 17].max() <= 1e-15
    # the bars are positive and small at this scale
    _, _, _, da, db, ds = sr.silhouette(X, lab, bars=True)
    assert (da[np.arange(300) != 17] > 0).all() and da[17] == 0 and (db > 0).all() and ds.max() < 1e-4


def test_grouped_spec_equals_sklearn_per_group():
    skm = pytest.importorskip("sklearn.metrics")
    X, lab = spec_case()
    rng = np.random.default_rng(8)
    grp = rng.integers(0, 3, 300)
    grp[:12] = 3
    lab = lab.copy()
    lab[:12] = 2                                  # group 3 holds one label
    s, a, b = sr.silhouette(X, lab, grp)
    for g in range(3):
        sel = grp == g
        assert np.abs(s[sel] - skm.silhouette_samples(X[sel], lab[sel], metric="euclidean")).max() <= 1e-12
        sg, ag, bg = sr.silhouette(X[sel], lab[sel])
        assert np.array_equal(s[sel], sg) and np.array_equal(a[sel], ag) and np.array_equal(b[sel], bg)
    one = grp == 3
    assert np.isnan(s[one]).all() and np.isnan(a[one]).all() and np.isnan(b[one]).all() and not np.isnan(s[~one]).any()
    s1, a1, b1 = sr.silhouette(X, lab, np.zeros(300, int))
    s0, a0, b0 = sr.silhouette(X, lab)
    assert np.array_equal(s1, s0) and np.array_equal(a1, a0) and np.array_equal(b1, b0)


def test_spec_on_hand_computable_cases():
    # two pairs on a line: 0, 1 | 4, 6
    X = np.array([[0.0], [1.0], [4.0], [6.0]])
    s, a, b = sr.silhouette(X, [0, 0, 1, 1])
    assert a.tolist() == [1.0, 1.0, 2.0, 2.0] and b.tolist() == [5.0, 4.0, 3.5, 5.5]
    assert np.allclose(s, [4 / 5.0, 3 / 4.0, 1.5 / 3.5, 3.5 / 5.5], rtol=0, atol=1e-15)
    # all rows identical: max(a, b) = 0 -> 0, no NaN; a cell and its duplicate under different labels
    s, a, b = sr.silhouette(np.ones((6, 3)), [0, 0, 0, 1, 1, 1])
    assert not s.any() and not a.any() and not b.any()
    s, a, b = sr.silhouette(np.array([[0.0, 0], [0, 0], [3, 4]]), [0, 1, 1])
    assert s[0] == 0.0 and a[0] == 0.0 and b[0] == 2.5 and a[1] == 5.0 and b[1] == 0.0 and s[1] == -1.0


def test_scib_aggregates_on_a_hand_made_case():
    s = np.array([0.5, -0.5, 0.25, 0.75, 0.1, 0.3, 0.9, -0.2, 0.0])
    assert sr.asw_label(s) == pytest.approx((np.mean(s) + 1) / 2) and sr.asw_label(s, rescale=False) == pytest.approx(np.mean(s))
    batch = np.array([0, 1, 0, 1, 0, 0, 0, 1, 2])
    group = np.array(["A", "A", "A", "A", "B", "B", "C", "C", "C"])      # B: one batch; C: as many batches as cells -- both skipped
    score, per = sr.asw_batch(s, batch, group)
    assert per == {"A": pytest.approx(1 - 0.5)} and score == pytest.approx(0.5)
    group2 = np.array(["A", "A", "A", "A", "B", "B", "B", "B", "B"])
    score, per = sr.asw_batch(s, batch, group2)
    assert per["B"] == pytest.approx(1 - np.mean([0.1, 0.3, 0.9, 0.2, 0.0])) and score == pytest.approx((0.5 + per["B"]) / 2)
    score_raw, per_raw = sr.asw_batch(s, batch, group2, rescale=False)
    assert per_raw["A"] == pytest.approx(0.5) and score_raw == pytest.approx(1 - score)
    assert np.isnan(sr.asw_batch(s, np.zeros(9, int), group)[0])
    # the package's aggregation is the same function of the same widths
    codes, levels = harmony_amd.ui.as_factor(group2)
    got, got_per = silhouette.batch_asw(s, batch, codes, levels)
    assert got == pytest.approx(score) and got_per == pytest.approx(per)
    got, got_per = silhouette.batch_asw(s, batch, *harmony_amd.ui.as_factor(group))
    assert got == pytest.approx(0.5) and list(got_per) == ["A"]


def test_silhouette_header_matches_the_library_and_the_binding():
    assert helpers.header_names("harmony_mi355x_silhouette.h") == set(_lib.SILHOUETTE_SIGNATURES) == {"hmx_silhouette"}
    found = helpers.header_functions("harmony_mi355x_silhouette.h")
    assert [n for n, _ in found] == ["hmx_silhouette"] and len(found[0][1]) == 13
    helpers.assert_header_stands_alone("harmony_mi355x_silhouette.h", ["hmx_silhouette"])
    helpers.assert_binding_matches(_lib.load(), "hmx_silhouette", found[0][1], _lib.SILHOUETTE_SIGNATURES["hmx_silhouette"][1])
    assert {"silhouette_samples", "silhouette_label", "silhouette_batch"} <= set(harmony_amd.__all__) and hasattr(harmony_amd.Harmony, "silhouette")


def test_python_argument_errors_come_before_the_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((100, 5))
    lab = np.arange(100) % 3
    nanlab = np.where(np.arange(100) == 7, np.nan, 1.0)
    objlab = np.array(["a"] * 99 + [None], dtype=object)
    for kw in (dict(labels=np.zeros(100, int)), dict(labels=lab[:99]), dict(labels=nanlab), dict(labels=objlab), dict(groups=lab[:5]),
               dict(groups=nanlab), dict(X=X[0]), dict(X=rng.standard_normal((100, 129))), dict(labels=np.zeros((100, 2), int))):
        args = dict(X=X, labels=lab)
        args.update(kw)
        with pytest.raises(ValueError):
            silhouette.silhouette_samples(**args)
    meta = {"b": lab, "one": np.zeros(100, int), "f": nanlab}
    for kw in (dict(label_col="nope"), dict(label_col="f"), dict(label_col="one"), dict(meta_data=np.arange(100)), dict(meta_data={"b": lab[:99]}),
               dict(label_col=["b"])):
        args = dict(X=X, meta_data=meta, label_col="b")
        args.update(kw)
        with pytest.raises(ValueError):
            silhouette.silhouette_label(**args)
    for kw in (dict(batch_col="nope"), dict(label_col="nope"), dict(batch_col="f"), dict(label_col="f"), dict(meta_data=None)):
        args = dict(X=X, meta_data=meta, batch_col="b", label_col="one")
        args.update(kw)
        with pytest.raises(ValueError):
            silhouette.silhouette_batch(**args)


def test_library_checks_the_arguments_before_the_device():
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    X = np.zeros((10, 4))
    xp = C.c_void_p(X.ctypes.data)
    lab, grp = (np.arange(10) % 2).astype(np.int32), (np.arange(10) % 3).astype(np.int32)
    s, a, b = np.zeros(10), np.zeros(10), np.zeros(10)
    P = lambda v: None if v is None else v.ctypes.data_as(ip if v.dtype == np.int32 else dp)  # noqa: E731

    def call(x=xp, dtype=0, loc=0, N=10, d=4, labels=lab, n_levels=2, groups=None, n_groups=0, so=s, ao=a, bo=b, handle=h):
        return lib.hmx_silhouette(handle, x, dtype, loc, N, d, P(labels), n_levels, P(groups), n_groups, P(so), P(ao), P(bo))

    def refused(status, **kw):
        assert call(**kw) == status, kw
        assert len(lib.hmx_last_error(h)) > 0, kw

    try:
        refused(HMX_ERR_ARG, labels=None)
        refused(HMX_ERR_ARG, so=None)
        refused(HMX_ERR_ARG, dtype=2)
        refused(HMX_ERR_ARG, loc=2)
        refused(HMX_ERR_ARG, N=0)
        refused(HMX_ERR_ARG, d=0)
        refused(HMX_ERR_ARG, n_levels=0)
        refused(HMX_ERR_ARG, n_levels=1)                    # a code outside [0, n_levels)
        refused(HMX_ERR_ARG, labels=lab - 1)
        refused(HMX_ERR_ARG, groups=grp, n_groups=0)
        refused(HMX_ERR_ARG, groups=grp, n_groups=2)
        refused(HMX_ERR_LIMIT, d=129)
        refused(HMX_ERR_LIMIT, N=2000000001)
        refused(HMX_ERR_STATE, x=None)                      # no embedding on a fresh handle
        if NO_GPU:                                          # valid calls get as far as the device
            refused(HMX_ERR_DEVICE)
            refused(HMX_ERR_DEVICE, groups=grp, n_groups=3, ao=None, bo=None)
            refused(HMX_ERR_DEVICE, dtype=1, n_levels=1 << 30, n_groups=5)      # (n_groups is ignored without groups)
        out = (C.c_double * 1)()
        assert lib.hmx_get(h, b"timer:silhouette", out, 1) == 1 and (out[0] == 0.0 or not NO_GPU)
    finally:
        lib.hmx_destroy(h)
    assert call(handle=None) == HMX_ERR_ARG


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_no_cpu_fallback():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((200, 6))
    meta = {"b": np.arange(200) % 2, "t": np.arange(200) % 3}
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        silhouette.silhouette_samples(X, meta["b"])
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        silhouette.silhouette_samples(X, meta["b"], groups=meta["t"], return_ab=True)
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        silhouette.silhouette_label(X, meta, "t")
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        silhouette.silhouette_batch(X, meta, "b", "t")
