"""Query cells in a fitted UMAP layout held to their spec (tests/umap_transform_ref.py) without a GPU: the header, the library and the binding
agree; every argument error is raised in Python before the library is loaded, and every host-decided status comes from the built library
before a device is needed (all its checks are host-side); the weights, the start and one epoch worked by hand; the schedule; and the quality
bar (tests/test_gpu_umap_transform.py runs the library).

The quality bar: the synchronous, hashed epochs against umap-learn's one-thread loop (umap_transform_ref.sequential) from the same start, by
D, the mean layout distance from a query cell to its k listed reference cells: |D_spec / D_seq - 1| <= 0.03 on groups(750, 6) split 600 / 150,
k = 30, 100 epochs, and the layout's 15 nearest reference cells vote every query cell its own label on both sides.  Measured: printed by the
test (D_spec / D_seq 1.2399 / 1.2390 with the prototype of this spec)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

sp = pytest.importorskip("scipy.sparse")

import graph_ref as gr  # noqa: E402
import helpers  # noqa: E402
import metrics_ref as mr  # noqa: E402
import umap_ref as ur  # noqa: E402
import umap_transform_ref as tr  # noqa: E402
from harmony_amd import Harmony, _lib, umap_query_weights, umap_transform, umap_transform_from_knn  # noqa: E402

HEADER = "harmony_mi355x_umap_transform.h"
AB = ur.find_ab(0.5)


def test_header_matches_the_library_and_the_binding():
    found = helpers.header_functions(HEADER)
    mine = [n for n, _ in found]
    assert mine == ["hmx_umap_query_weights", "hmx_umap_transform"] and set(mine) == set(_lib.UMAP_TRANSFORM_SIGNATURES)
    earlier = helpers.PUBLIC_HEADERS + (("harmony_mi355x_louvain.h", "LOUVAIN_SIGNATURES"), ("harmony_mi355x_leiden.h", "LEIDEN_SIGNATURES"),
                                        ("harmony_mi355x_umap.h", "UMAP_SIGNATURES"))
    for other, table in earlier:                           # every header before this one
        assert other != HEADER and not (set(mine) & helpers.header_names(other)), other
        assert not (set(mine) & set(getattr(_lib, table))), table
    tables = [t for t in dir(_lib) if t.endswith("SIGNATURES") and t != "UMAP_TRANSFORM_SIGNATURES"]
    assert len(tables) >= 13 and not any(set(mine) & set(getattr(_lib, t)) for t in tables)
    declared = set(n for other in os.listdir(helpers.INCLUDE) if other != HEADER for n in helpers.header_names(other))
    assert not (set(mine) & declared)                      # no other header names them, comments included
    ctypes_of = dict(helpers.CTYPES, uint32_t=(C.c_uint32,))      # the seed
    lib = _lib.load()
    for (name, types), count in zip(found, (8, 20)):
        fn, sig = getattr(lib, name), _lib.UMAP_TRANSFORM_SIGNATURES[name][1]
        assert fn.restype is C.c_int and list(fn.argtypes) == sig and len(types) == len(sig) == count
        for t, s in zip(types, sig):
            assert any(s is o or s == o for o in ctypes_of[t]), (name, t, s)


# ---- the weights by hand -------------------------------------------------------------------------------------------------------------------------
def test_weights_of_a_row_of_three_written_out():
    """d = 1, 2, 3: the search runs over columns 1 and 2 alone, target log2 3; the weights over all three"""
    d = [1.0, 2.0, 3.0]
    target = np.log2(3.0)
    lo, hi, mid = 0.0, float("inf"), 1.0
    for _ in range(64):
        psum = np.exp(-d[1] / mid) + np.exp(-d[2] / mid)    # column 0 is left out
        if abs(psum - target) < 1e-5:
            break
        if psum > target:
            hi = mid
            mid = (lo + hi) / 2.0
        else:
            lo = mid
            mid = mid * 2.0 if hi == float("inf") else (lo + hi) / 2.0
    assert abs(np.exp(-2.0 / mid) + np.exp(-3.0 / mid) - target) < 1e-5 and 8.0 < mid < 16.0
    idx = np.array([[0, 1, 2]], dtype=np.int32)
    w, sigma = tr.query_weights(idx, np.array([d], dtype=np.float32))
    assert sigma[0] == mid and mid > 1e-3 * 2.0              # the floor 1e-3 mean(d) is far below
    assert w.dtype == np.float32 and np.array_equal(w[0], np.exp(-np.array(d) / mid).astype(np.float32))
    assert 0.9 < w[0, 0] < 1.0                               # column 0 has a weight of its own: no rho is taken off
    with_col0 = np.exp(-1.0 / mid) + np.exp(-2.0 / mid) + np.exp(-3.0 / mid)
    assert abs(with_col0 - target) > 0.5                     # ... and the sum that includes it is not what the search held to the target
    mids, steps, open_ = tr.search(np.array([d], dtype=np.float32))
    assert mids[0] == mid and 0 < steps[0] <= 30 and not open_.any()


def test_weights_of_all_zero_distances_and_of_a_query_on_a_reference_cell():
    for k, want in ((1, 1.0), (2, 1.0), (3, 2.0 ** -64), (15, 2.0 ** -64)):
        idx = np.tile(np.arange(k, dtype=np.int32), (4, 1))
        w, sigma = tr.query_weights(idx, np.zeros((4, k), dtype=np.float32))
        assert np.all(sigma == want) and np.all(w == 1.0), k      # k = 1: psum = 0 = log2 1; k = 2: psum = 1 = log2 2; k >= 3: halved 64 times
    d = np.array([[0.0, 0.5, 0.7, 0.9], [0.1, 0.5, 0.7, 0.9]], dtype=np.float32)
    w, sigma = tr.query_weights(np.tile(np.arange(4, dtype=np.int32), (2, 1)), d)
    assert w[0, 0] == 1.0 and w[1, 0] < 1.0 and sigma[0] == sigma[1]      # d_0 = 0: w_0 == 1; the search does not see column 0
    assert np.all(np.diff(w, axis=1) < 0)
    # the floor: a row whose search ends far below the global mean takes 1e-3 of it
    d = np.array([[0.0, 1e-9, 1e-9], [100.0, 200.0, 300.0]], dtype=np.float32)
    w, sigma = tr.query_weights(np.tile(np.arange(3, dtype=np.int32), (2, 1)), d)
    assert sigma[0] == 1e-3 * (np.float64(d.astype(np.float64).sum()) / 6.0) and sigma[1] > 50.0


# ---- the start and the epochs by hand ---------------------------------------------------------------------------------------------------------
YREF = np.array([[0.0, 0.0], [1.0, 0.0], [3.0, 1.0], [0.1, 0.0], [-2.0, 5.0]], dtype=np.float32)


def test_start_by_hand():
    idx = np.array([[0, 1, 2], [2, 4, 1], [3, 0, 1]], dtype=np.int32)
    w = np.array([[1.0, 0.5, 0.25], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    Y = tr.init(idx, w, YREF)
    assert np.allclose(Y[0], [(0.5 * 1.0 + 0.25 * 3.0) / 1.75, 0.25 / 1.75], atol=1e-15)
    assert np.allclose(Y[1], [(3.0 - 2.0 + 1.0) / 3.0, 6.0 / 3.0], atol=1e-15)      # every weight 0: the plain mean of the listed positions
    assert np.array_equal(Y[2], [1.0, 0.0])


def test_one_epoch_by_hand_with_a_clipped_sample_and_an_entry_that_never_fires():
    """a = b = 1: c_a = -2 / (1 + d2), no factor 2.  One cell at (0, 0.1) with the list (1, 2, 4) and the weights 1, 0.5, 0.005 of a
    100-epoch schedule: the third entry is below wmax / n_epochs and never fires; epoch 1 fires the first two"""
    idx = np.array([[1, 2, 4]], dtype=np.int32)
    w = np.array([[1.0, 0.5, 0.005]], dtype=np.float32)
    Y = np.array([[0.0, 0.1]])
    assert [int(ur.firings(tr.rates(w)[0][0, t], 100)) for t in range(3)] == [100, 50, 0]
    step0 = tr.epoch(idx, w, YREF, Y, 0, 100, 1.0, 1.0, negative_sample_rate=0, alpha0=0.25)
    step1 = tr.epoch(idx, w, YREF, Y, 1, 100, 1.0, 1.0, negative_sample_rate=0, alpha0=0.25)
    assert step0.fired == 1 and step1.fired == 2

    def attract(y, j):
        d = y - YREF[j].astype(np.float64)
        return np.clip(-2.0 / (1.0 + d @ d) * d, -4.0, 4.0)
    assert np.allclose(step0.Y, Y[0] + 0.25 * attract(Y[0], 1), atol=1e-15)
    al = ur.alpha_of(1, 100, 0.25)
    assert al == float(np.float32(0.25 * 0.99))
    assert np.allclose(step1.Y, Y[0] + al * (attract(Y[0], 1) + attract(Y[0], 2)), atol=1e-15)
    assert np.all(step1.B > 0) and np.all(step1.B < 1e-5)
    # one sample per firing; a seed for which entry 0 draws cell 3 at (0.1, 0): d = (-0.1, 0.1), d2 = 0.02, c_r d = 2 gamma / (0.021 * 1.02) d: clipped
    seed = next(s for s in range(1000) if ur.negative_sample(0, 0, 0, 5, s) == 3)
    step = tr.epoch(idx, w, YREF, Y, 0, 100, 1.0, 1.0, gamma=1.5, negative_sample_rate=1, seed=seed, alpha0=0.25)
    assert step.fired == 1 and 2.0 * 1.5 / (0.021 * 1.02) * 0.1 > 4.0
    assert np.allclose(step.Y, Y[0] + 0.25 * (attract(Y[0], 1) + np.array([-4.0, 4.0])), atol=1e-15)
    # a sample is not skipped for carrying the query cell's index: cell 0 of the query and cell 0 of the reference are different cells
    seed = next(s for s in range(1000) if ur.negative_sample(0, 0, 0, 5, s) == 0)
    step = tr.epoch(idx, w, YREF, Y, 0, 100, 1.0, 1.0, negative_sample_rate=1, seed=seed, alpha0=0.25)
    d = Y[0] - YREF[0]
    assert np.allclose(step.Y, Y[0] + 0.25 * (attract(Y[0], 1) + np.clip(2.0 / ((0.001 + d @ d) * (d @ d + 1.0)) * d, -4.0, 4.0)), atol=1e-15)
    # a cell on a listed position: the attraction is 0 there
    on = tr.epoch(idx[:, :1], w[:, :1], YREF, YREF[1:2], 0, 100, 1.0, 1.0, negative_sample_rate=0)
    assert np.array_equal(on.Y, YREF[1:2]) and on.fired == 1
    assert tr.depth(15, 5) == 6 + 4 and tr.depth(16, 5) == 10 and tr.depth(17, 5) == 6 + 6 and tr.depth(65, 5) == 12 + 6 and tr.depth(128, 0) == 2 + 6


@functools.lru_cache(maxsize=None)
def case(N, Nq, G, k, ref_epochs=100):
    """a reference laid out by the layout's own spec from its graph of n_neighbors = k (k - 1 other cells), and a query's lists into it"""
    Xr, lab_r, Xq, lab_q, idx, dist = tr.problem(N, Nq, G, k)
    ridx, rdist = mr.knn(Xr, k - 1)[:2]
    g = gr.connectivities(ridx.astype(np.int32), np.sqrt(np.maximum(np.asarray(rdist, dtype=np.float64), 0.0)).astype(np.float32))
    Yref = ur.layout(g, ur.pca_init(Xr, 2), ref_epochs, *AB)[0].astype(np.float32)
    w = tr.query_weights(idx, dist)[0]
    return Yref, lab_r, lab_q, idx, dist, w


def test_firing_counts_and_a_schedule_run_in_two_parts():
    Yref, _, _, idx, dist, w = case(750, 150, 6, 30)
    hand = np.array([[0.8, 0.7992, 0.6, 0.4, 0.8 / 3.0, 0.08, 0.00808, 0.008, 0.00792, 0.0032, 0.0]], dtype=np.float32)
    rh = tr.rates(hand)[0]                                 # over the whole schedule an entry fires floor(n_epochs r) times: never below wmax / n_epochs
    for n_epochs in (1, 7, 100, 200):
        count = ur.firings(rh, n_epochs)
        assert count.tolist() == np.floor(n_epochs * rh).astype(np.int64).tolist()
        assert np.all(count[rh < 1.0 / n_epochs] == 0) and count[0, 0] == n_epochs
    r = tr.rates(w)[0]
    assert ur.firings(r, 100).tolist() == np.floor(100 * r).astype(np.int64).tolist() and r.max() == 1.0
    whole, f, snap = tr.transform(idx, w, Yref, 100, *AB, snapshots=(10,))
    first, f1, _ = tr.transform(idx, w, Yref, 100, *AB, epochs=(0, 10))
    both, f2, _ = tr.transform(idx, w, Yref, 100, *AB, Y0=first, epochs=(10, 100))
    assert np.array_equal(both, whole) and f1 + f2 == f == int(ur.firings(r, 100).sum()) and np.array_equal(snap[10], first)
    assert not np.array_equal(whole, tr.transform(idx, w, Yref, 100, *AB, seed=1)[0])
    start = tr.init(idx, w, Yref)
    assert np.array_equal(tr.transform(idx, w, Yref, 100, *AB, epochs=(7, 7))[0], start)
    assert np.array_equal(tr.transform(idx, np.zeros_like(w), Yref, 100, *AB)[0], tr.init(idx, np.zeros_like(w), Yref))      # wmax == 0
    mids, steps, open_ = tr.search(dist)
    print("umap transform (600 / 150, k = 30): bisection steps at most %d, unconverged rows %d" % (steps.max(), open_.sum()))
    assert not open_.any()


# ---- quality: against umap-learn's sequential loop ----------------------------------------------------------------------------------------------
def test_quality_against_the_sequential_loop():
    Yref, lab_r, lab_q, idx, dist, w = case(750, 150, 6, 30)
    start = tr.init(idx, w, Yref)
    Y = tr.transform(idx, w, Yref, 100, *AB)[0]
    Ys = tr.sequential(idx, w, Yref, start, 100, *AB)
    D, Ds, D0 = tr.spread_to_neighbours(Y, idx, Yref), tr.spread_to_neighbours(Ys, idx, Yref), tr.spread_to_neighbours(start, idx, Yref)
    print("umap transform quality (600 / 150, k = 30, 100 epochs): D synchronous %.4f, sequential %.4f, ratio %.4f; the start %.4f"
          % (D, Ds, D / Ds, D0))
    assert np.all(np.isfinite(Y)) and abs(D / Ds - 1.0) <= 0.03
    assert np.array_equal(tr.vote(Y, Yref, lab_r), lab_q) and np.array_equal(tr.vote(Ys, Yref, lab_r), lab_q)


def spec_spread(seeds=range(5)):
    """what tests/test_gpu_umap_transform.py records: the spec's D at (2000, 500, k = 15), 100 epochs, per seed"""
    Yref, lab_r, lab_q, idx, dist, w = case(2500, 500, 8, 15)
    out = []
    for s in seeds:
        Y = tr.transform(idx, w, Yref, 100, *AB, seed=s)[0]
        assert np.array_equal(tr.vote(Y, Yref, lab_r), lab_q)
        out.append((tr.spread_to_neighbours(Y, idx, Yref), float(np.abs(Y - tr.init(idx, w, Yref)).mean())))
    return out


def test_constants_for_the_gpu_test():
    from test_gpu_umap_transform import SPEC_D
    got = spec_spread()
    D = [d for d, _ in got]
    print("umap transform spec at (2000, 500, k = 15), 100 epochs, seeds 0 .. 4: D = %s, mean %.6f, spread %.6f; mean |Y - Y0| = %s"
          % (", ".join("%.6f" % d for d in D), np.mean(D), max(D) - min(D), ", ".join("%.4f" % m for _, m in got)))
    assert abs(np.mean(D) - SPEC_D[0]) < 1e-5 and abs(max(D) - min(D) - SPEC_D[1]) < 1e-5


# ---- every argument error is raised before a device is needed --------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device():
    idx = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)
    dist = np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3]], dtype=np.float32)
    w = np.array([[1.0, 0.5, 0.25], [1.0, 0.5, 0.25]], dtype=np.float32)
    for args, msg in (((idx[0], dist[0], 5), "one shape"), ((idx, dist[:, :2], 5), "one shape"), ((idx, dist, 0), "n_reference"),
                      ((idx, dist, 2), "exceeds"), ((idx, dist, 4), r"\[0, 4\)"), ((idx.astype(np.float64), dist, 5), "integers"),
                      ((-idx - 1, dist, 5), r"\[0, 5\)"), ((idx, -dist, 5), "non-negative"), ((idx, dist * np.nan, 5), "finite"),
                      ((idx, np.full_like(dist, np.inf), 5), "finite"),
                      ((np.zeros((1, 129), dtype=np.int32), np.zeros((1, 129)), 500), "at most 128")):
        with pytest.raises(ValueError, match=msg):
            umap_query_weights(*args)
    for bad, msg in ((YREF[:, :1], "2 or 3"), (np.zeros((5, 4)), "2 or 3"), (np.zeros(5), "2 or 3"), (np.full((5, 2), np.nan), "not finite"),
                     (YREF[:4], r"\[0, 4\)"), (YREF[:2], "exceeds")):
        with pytest.raises(ValueError, match=msg):
            umap_transform_from_knn(idx, w, bad, a=1.0, b=1.0)
    for bad, msg in ((w * 1.5, r"\[0, 1\]"), (-w, r"\[0, 1\]"), (w * np.nan, r"\[0, 1\]"), (w[:1], "one shape")):
        with pytest.raises(ValueError, match=msg):
            umap_transform_from_knn(idx, bad, YREF, a=1.0, b=1.0)
    for kw, msg in (({"n_epochs": 0}, "n_epochs"), ({"n_epochs": 2 ** 20 + 1}, "n_epochs"), ({"n_epochs": 1.5}, "n_epochs"),
                    ({"n_epochs": 20, "epochs": (5, 21)}, "epochs"), ({"n_epochs": 20, "epochs": (-1, 5)}, "epochs"),
                    ({"n_epochs": 20, "epochs": (6, 5)}, "begin <= end"), ({"epochs": 3}, "pair"), ({"gamma": -0.5}, "gamma"),
                    ({"gamma": float("nan")}, "gamma"), ({"learning_rate": 0.0}, "learning_rate"), ({"learning_rate": float("inf")}, "learning_rate"),
                    ({"negative_sample_rate": -1}, "negative_sample_rate"), ({"negative_sample_rate": 32}, "negative_sample_rate"),
                    ({"seed": -1}, "seed"), ({"seed": 2 ** 32}, "seed"), ({"a": 1.0}, "both a and b"), ({"a": 0.0, "b": 1.0}, "a must"),
                    ({"a": 1.0, "b": float("nan")}, "b must"), ({"min_dist": 5.0}, "min_dist"), ({"spread": -1.0}, "spread"),
                    ({"init": np.zeros((2, 3))}, "init must be"), ({"init": np.zeros((3, 2))}, "init must be"),
                    ({"init": np.full((2, 2), np.inf)}, "not finite")):
        kw = dict({"a": 1.0, "b": 1.0} if "a" not in kw and "min_dist" not in kw and "spread" not in kw else {}, **kw)
        with pytest.raises(ValueError, match=msg):
            umap_transform_from_knn(idx, w, YREF, **kw)
    X = ur.groups(40, 2)[0]
    layout = np.zeros((30, 2), dtype=np.float32)
    for args, kw, msg in (((X[30:], X[:30], layout), {"n_neighbors": 0}, "n_neighbors"), ((X[30:], X[:30], layout), {"n_neighbors": 31}, "n_neighbors"),
                          ((X[30:], X[:30], layout), {"n_neighbors": 2.5}, "n_neighbors"), ((X[30:], X[:30], layout[:29]), {}, "29 rows"),
                          ((X[30:, :5], X[:30], layout), {}, "PCs"), ((np.zeros(5), X[:30], layout), {}, "cells x PCs"),
                          ((X[30:], X[:30], np.zeros((30, 4))), {}, "2 or 3"), ((X[30:], X[:30], layout), {"init": np.zeros((9, 2))}, "init must be"),
                          ((X[30:], X[:30], layout), {"n_epochs": 0}, "n_epochs")):
        with pytest.raises(ValueError, match=msg):
            umap_transform(*args, a=1.0, b=1.0, **kw)
    assert callable(Harmony.umap_transform)


def test_library_statuses_are_decided_on_the_host():
    lib = _lib.load()
    ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    h = C.c_void_p(lib.hmx_create())
    ARG, LIMIT = 1, 7
    idx0 = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)
    dist0 = np.array([[0.1, 0.2, 0.3], [0.0, 0.2, 0.3]], dtype=np.float32)
    w0 = np.array([[1.0, 0.5, 0.25], [1.0, 0.0, 0.25]], dtype=np.float32)
    try:
        def weights(Nq=2, k=3, Nr=5, idx=idx0, dist=dist0, null=None):
            idx, dist = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float32)
            out, sig = np.zeros((2, 3), dtype=np.float32), np.zeros(2)
            arg = {"idx": idx.ctypes.data_as(ip), "dist": dist.ctypes.data_as(fp), "weights": out.ctypes.data_as(fp)}
            if null:
                arg[null] = None
            s = lib.hmx_umap_query_weights(h, arg["idx"], arg["dist"], Nq, k, Nr, arg["weights"], sig.ctypes.data_as(dp))
            assert not out.any() and not sig.any()
            return s
        for null in ("idx", "dist", "weights"):
            assert weights(null=null) == ARG, null
        assert weights(Nq=0) == ARG and weights(Nq=-1) == ARG
        for bad in (0, -1, 129):
            assert weights(k=bad, Nr=500) == ARG and b"k must" in lib.hmx_last_error(h)
        assert weights(Nr=2) == ARG and b"exceeds" in lib.hmx_last_error(h)
        assert weights(Nq=2 ** 31 // 3 + 1) == LIMIT and weights(Nq=2 ** 24, k=128, Nr=500) == LIMIT      # (refused before an entry is read)
        assert weights(Nr=2000000001) == LIMIT
        for bad in (-1, 5, 2 ** 31 - 1):
            idx = idx0.copy()
            idx[1, 2] = bad
            assert weights(idx=idx) == ARG and b"outside [0, Nr)" in lib.hmx_last_error(h) and b"row 1" in lib.hmx_last_error(h)
        assert weights(Nr=4) == ARG                          # the index 4 is out of range there
        for bad in (np.nan, -0.5, np.inf, -np.inf):
            dist = dist0.copy()
            dist[1, 0] = bad
            assert weights(dist=dist) == ARG and b"distance" in lib.hmx_last_error(h) and b"row 1" in lib.hmx_last_error(h)
        assert lib.hmx_umap_query_weights(None, None, None, 1, 1, 1, None, None) == ARG

        def transform(Nq=2, k=3, Nr=5, dim=2, n_epochs=20, begin=0, end=20, a=1.0, b=1.0, gamma=1.0, alpha0=0.25, neg=5, seed=0, idx=idx0, w=w0,
                      ref=YREF, start=None, null=None):
            idx, w = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(w, dtype=np.float32)
            ref = np.ascontiguousarray(np.concatenate([ref, np.zeros((5, 1), dtype=np.float32)], axis=1) if dim == 3 and ref.shape[1] == 2 else ref, dtype=np.float32)
            Y, Yinit = np.zeros((2, 3), dtype=np.float32), np.zeros((2, 3), dtype=np.float32)
            arg = {"idx": idx.ctypes.data_as(ip), "weights": w.ctypes.data_as(fp), "Yref": ref.ctypes.data_as(fp), "Y": Y.ctypes.data_as(fp)}
            if null:
                arg[null] = None
            y0 = None if start is None else np.ascontiguousarray(start, dtype=np.float32)
            s = lib.hmx_umap_transform(h, arg["idx"], arg["weights"], Nq, k, arg["Yref"], Nr, dim, None if y0 is None else y0.ctypes.data_as(fp),
                                       n_epochs, begin, end, a, b, gamma, alpha0, neg, seed, Yinit.ctypes.data_as(fp), arg["Y"])
            assert not Y.any() and not Yinit.any()         # neither is written
            return s
        for null in ("idx", "weights", "Yref", "Y"):
            assert transform(null=null) == ARG, null
        assert transform(Nq=0) == ARG and transform(Nq=-3) == ARG
        for bad in (0, -1, 129):
            assert transform(k=bad, Nr=500) == ARG and b"k must" in lib.hmx_last_error(h)
        assert transform(Nr=2) == ARG and b"exceeds" in lib.hmx_last_error(h)
        for bad in (1, 4, 0, -2):
            assert transform(dim=bad) == ARG and b"dim" in lib.hmx_last_error(h)
        for bad in (0, -1, 2 ** 20 + 1):
            assert transform(n_epochs=bad, begin=0, end=0) == ARG and b"n_epochs" in lib.hmx_last_error(h)
        for begin, end in ((-1, 5), (5, 21), (6, 5), (21, 21)):
            assert transform(begin=begin, end=end) == ARG and b"epoch_begin" in lib.hmx_last_error(h)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert transform(a=bad) == ARG and transform(b=bad) == ARG and b"a and b" in lib.hmx_last_error(h)
            assert transform(alpha0=bad) == ARG and b"alpha0" in lib.hmx_last_error(h)
        for bad in (-0.5, float("nan"), float("inf")):
            assert transform(gamma=bad) == ARG and b"gamma" in lib.hmx_last_error(h)
        for bad in (-1, 32):
            assert transform(neg=bad) == ARG and b"negative_sample_rate" in lib.hmx_last_error(h)
        assert transform(Nq=2 ** 31 // 3 + 1) == LIMIT and transform(Nr=2000000001) == LIMIT
        for bad in (-1, 5):
            idx = idx0.copy()
            idx[1, 0] = bad
            assert transform(idx=idx) == ARG and b"outside [0, Nr)" in lib.hmx_last_error(h)
        for bad in (1.5, -0.25, np.nan, np.inf):
            w = w0.copy()
            w[1, 1] = bad
            assert transform(w=w) == ARG and b"[0, 1]" in lib.hmx_last_error(h) and b"row 1" in lib.hmx_last_error(h)
        for bad in (np.nan, np.inf, -np.inf):
            ref = YREF.copy()
            ref[3, 1] = bad
            assert transform(ref=ref) == ARG and b"Yref" in lib.hmx_last_error(h) and b"cell 3" in lib.hmx_last_error(h)
            start = np.zeros((2, 2), dtype=np.float32)
            start[1, 0] = bad
            assert transform(start=start) == ARG and b"Yq0" in lib.hmx_last_error(h) and b"cell 1" in lib.hmx_last_error(h)
        assert lib.hmx_umap_transform(None, None, None, 1, 1, None, 1, 2, None, 1, 0, 1, 1.0, 1.0, 1.0, 0.25, 5, 0, None, None) == ARG
        out1 = (C.c_double * 1)()
        for key in (b"umap_transform:fired", b"umap_transform:epochs", b"timer:umap_transform", b"timer:umap_transform_epochs", b"timer:umap_query_weights"):
            assert lib.hmx_get(h, key, out1, 1) == 1 and out1[0] == 0, key
    finally:
        lib.hmx_destroy(h)
