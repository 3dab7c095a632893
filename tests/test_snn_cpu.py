"""Seurat's SNN graph held to its spec (tests/snn_ref.py) without a GPU: the header, the library and the binding agree; the spec equals
set intersections computed row by row and a hand-computed example; the pruning threshold at its edges; the argument errors need no device
(tests/test_gpu_snn.py runs the library)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytest.importorskip("scipy.sparse")

import helpers  # noqa: E402
import metrics_ref as mr  # noqa: E402
import snn_ref as sr  # noqa: E402
from harmony_amd import Harmony, _lib, neighbors, snn, snn_from_knn  # noqa: E402


def test_snn_header_matches_the_library_and_the_binding():
    found = helpers.header_functions("harmony_mi355x_snn.h")
    mine = [n for n, _ in found]
    assert mine == ["hmx_snn_from_knn", "hmx_snn_graph"] and set(mine) == set(_lib.SNN_SIGNATURES)
    helpers.assert_header_stands_alone("harmony_mi355x_snn.h", mine)
    for name, types in found:
        helpers.assert_binding_matches(_lib.load(), name, types, _lib.SNN_SIGNATURES[name][1])


# ---- the spec against independent arithmetic -------------------------------------------------------------------------------------------------
def lists(N, m, d=5, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, d)) * rng.uniform(0.2, 3.0, size=(N, 1))
    return mr.knn(X, m)[0].astype(np.int32)


@pytest.mark.parametrize("N,m,prune", [(300, 19, 1.0 / 15.0), (120, 1, 0.0), (90, 64, 0.5), (200, 7, 1.0 / 15.0), (150, 29, 0.0)])
def test_spec_equals_set_intersections_row_by_row(N, m, prune):
    idx = lists(N, m, seed=m)
    idx[3, m // 2:] = -1                                   # a row with unfilled slots
    idx[7, :] = -1                                         # a row without neighbours
    k = m + 1
    sets = [set([i]) | set(int(v) for v in idx[i] if v >= 0) for i in range(N)]
    smin = next(s for s in range(1, k + 2) if s / (2 * k - s) >= prune)
    indptr, indices, weights, shared = sr.snn(idx, prune)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and weights.dtype == np.float32 and indptr[0] == 0 and indptr[N] == indices.size
    cand = sr.candidates(idx)
    indeg = np.bincount(idx[idx >= 0], minlength=N)
    for i in range(N):
        want = [(j, len(sets[i] & sets[j])) for j in range(N)]
        want = [(j, s) for j, s in want if s >= max(smin, 1)]
        got = list(zip(indices[indptr[i]:indptr[i + 1]].tolist(), shared[indptr[i]:indptr[i + 1]].tolist()))
        assert got == want, i
        assert cand[i] == sum(indeg[j] + 1 for j in sets[i])
    assert np.array_equal(weights, np.array([np.float32(s / (2.0 * k - s)) for s in shared.tolist()], dtype=np.float32))
    dense = np.zeros((N, N), dtype=np.float32)
    dense[np.repeat(np.arange(N), np.diff(indptr)), indices] = weights
    assert np.array_equal(dense, dense.T)
    A = sr.nn_matrix(idx)
    assert all(A.indices[A.indptr[i]:A.indptr[i + 1]].tolist() == sorted(sets[i]) for i in range(N))


def test_hand_computed_four_cells():
    """N+ = {0,1}, {0,1}, {1,2}, {2,3}; k = 2.  s: (0,0) (0,1) (1,1) (2,2) (3,3) = 2; (0,2) (1,2) (2,3) = 1; (0,3) (1,3) = 0.  J(2) = 1, J(1) = 1/3;
    prune = 1/15 keeps s >= 1, prune = 0.5 keeps s = 2"""
    idx = np.array([[1], [0], [1], [2]], dtype=np.int32)
    third = np.float32(1.0 / 3.0)
    indptr, indices, weights, shared = sr.snn(idx, 1.0 / 15.0)
    assert indptr.tolist() == [0, 3, 6, 10, 12]
    assert indices.tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 2, 3]
    assert shared.tolist() == [2, 2, 1, 2, 2, 1, 1, 1, 2, 1, 1, 2]
    assert np.array_equal(weights, np.where(shared == 2, np.float32(1.0), third).astype(np.float32)) and weights.dtype == np.float32
    indptr, indices, weights, shared = sr.snn(idx, 0.5)
    assert list(zip(np.repeat(np.arange(4), np.diff(indptr)).tolist(), indices.tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (3, 3)]
    assert np.all(weights == 1.0) and np.all(shared == 2)
    assert sr.candidates(idx).tolist() == [2 + 3, 2 + 3, 3 + 2, 2 + 1]


def test_s_min_values():
    assert sr.s_min(20, 1.0 / 15.0) == 3                   # 2 / 38 < 1 / 15 <= 3 / 37
    assert sr.s_min(8, 1.0 / 15.0) == 1                    # 1 / 15 == 1 / 15: the test is <, equality is kept
    assert 1.0 / 15.0 == float(1) / float(2 * 8 - 1)
    for k in (2, 8, 20, 129):
        assert sr.s_min(k, 0.0) == 1 and sr.s_min(k, 1.0) == k


# ---- every argument error is raised before a device is needed --------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device():
    X = np.random.default_rng(0).normal(size=(40, 5))
    for bad in (1, 130, 2.5, 41):
        with pytest.raises(ValueError, match="k "):
            snn(X, k=bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="prune"):
            snn(X, prune=bad)
        with pytest.raises(ValueError, match="prune"):
            snn_from_knn(np.array([[1, 2], [0, 2], [0, 1]]), prune=bad)
    with pytest.raises(ValueError, match="cells x PCs"):
        snn(np.zeros(5))
    for idx, msg in ((np.array([[1, 2], [1, 2], [0, 1]]), "own cell"), (np.array([[1, 1], [0, 2], [0, 1]]), "twice"),
                     (np.array([[1, 3], [0, 2], [0, 1]]), r"\[-1, 3\)"), (np.array([[1, -2], [0, 2], [0, 1]]), r"\[-1, 3\)"),
                     (np.array([[1.0, 2.0], [0.0, 2.0], [0.0, 1.0]]), "integers"), (np.zeros((3, 129), dtype=int), "at most 128"),
                     (np.zeros(3, dtype=int), "N x m")):
        with pytest.raises(ValueError, match=msg):
            snn_from_knn(idx)
    assert callable(Harmony.snn)


def test_library_argument_errors_come_before_the_device():
    lib = _lib.load()
    ip, fp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    h = C.c_void_p(lib.hmx_create())
    ARG, STATE, LIMIT = 1, 6, 7
    try:
        def lists_call(idx, N, m, prune=1.0 / 15.0, cap=100, null=None):
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            indptr, indices, weights = np.zeros(min(max(N, 0), 100) + 1, dtype=np.int64), np.zeros(100, dtype=np.int32), np.zeros(100, dtype=np.float32)
            return lib.hmx_snn_from_knn(h, None if null == "idx" else idx.ctypes.data_as(ip), N, m, prune,
                                        None if null == "indptr" else indptr.ctypes.data_as(lp), None if null == "indices" else indices.ctypes.data_as(ip),
                                        None if null == "weights" else weights.ctypes.data_as(fp), cap)
        ok = np.array([[1, 2], [0, 2], [0, 1]])
        assert lists_call(np.array([[1, 3], [0, 2], [0, 1]]), 3, 2) == ARG and b"[-1, N)" in lib.hmx_last_error(h)
        assert lists_call(np.array([[1, -2], [0, 2], [0, 1]]), 3, 2) == ARG
        assert lists_call(np.array([[1, 2], [1, 2], [0, 1]]), 3, 2) == ARG and b"own cell" in lib.hmx_last_error(h)
        assert lists_call(np.array([[1, 1], [0, 2], [0, 1]]), 3, 2) == ARG and b"twice" in lib.hmx_last_error(h)
        assert lists_call(np.array([[-1, -1], [0, 2], [0, 1]]), 3, 2, prune=2.0) == ARG      # (two unfilled slots are no duplicate: prune is what fails)
        for bad in (-0.1, 1.5, float("nan")):
            assert lists_call(ok, 3, 2, prune=bad) == ARG and b"prune" in lib.hmx_last_error(h)
        assert lists_call(ok, 3, 2, cap=-1) == ARG
        assert lists_call(ok, 0, 2) == ARG and lists_call(ok, 3, 0) == ARG
        for null in ("idx", "indptr", "indices", "weights"):
            assert lists_call(ok, 3, 2, null=null) == ARG, null
        assert lists_call(np.zeros((1, 129)), 1, 129) == LIMIT
        assert lists_call(ok, 2000000001, 2) == LIMIT       # (refused before a row is read)
        X = np.zeros((10, 4))
        out = np.zeros(11, dtype=np.int64)

        def graph_call(N, d, k, prune=1.0 / 15.0, x=X, indptr=out, cap=0):
            return lib.hmx_snn_graph(h, None if x is None else C.c_void_p(x.ctypes.data), 0, 0, N, d, k, prune, None, None,
                                     None if indptr is None else indptr.ctypes.data_as(lp), None, None, cap)
        assert graph_call(10, 4, 1) == LIMIT and graph_call(10, 4, 130) == LIMIT and graph_call(10, 4, 11) == LIMIT
        assert graph_call(10, 129, 5) == LIMIT and graph_call(0, 4, 5) == ARG and graph_call(10, 4, 5, indptr=None) == ARG
        assert graph_call(10, 4, 5, prune=-0.1) == ARG and graph_call(10, 4, 5, prune=float("nan")) == ARG
        assert graph_call(10, 4, 5, cap=-1) == ARG and graph_call(10, 4, 5, cap=5) == ARG      # (a positive capacity needs indices and weights)
        assert graph_call(10, 4, 5, x=None) == STATE        # no embedding on a fresh handle
        out1 = (C.c_double * 1)()
        for key in (b"snn:s_min", b"snn:short_cap", b"snn:window", b"snn:long_rows", b"timer:snn", b"timer:knn"):
            assert lib.hmx_get(h, key, out1, 1) == 1, key
        assert lib.hmx_get(h, b"snn:short_cap", out1, 1) == 1 and out1[0] >= 129 * 2      # a row whose neighbours nobody else lists is short
        assert lib.hmx_get(h, b"snn:window", out1, 1) == 1 and out1[0] >= 256 and out1[0] % 4 == 0
    finally:
        lib.hmx_destroy(h)


def test_graph_and_snn_calls_refuse_alike():
    """the neighbour graph and the SNN graph share the check of neighbour lists and the envelope of the neighbour count: the same bad input is
    refused with the same status and the same text, up to the parameter's name"""
    for call, name in ((lambda v: neighbors(np.zeros((10, 4)), n_neighbors=v), "n_neighbors"), (lambda v: snn(np.zeros((10, 4)), k=v), "k")):
        for bad in (float("nan"), float("inf"), 1, 130, 11):
            with pytest.raises(ValueError, match=name + " "):
                call(bad)
    lib = _lib.load()
    ip, fp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    h = C.c_void_p(lib.hmx_create())
    ARG, LIMIT = 1, 7
    try:
        def both_from_knn(idx, N, m):
            idx, dist = np.ascontiguousarray(idx, dtype=np.int32), np.ones((N, m), dtype=np.float32)
            indptr, indices, weights = np.zeros(N + 1, dtype=np.int64), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.float32)
            out = indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip), weights.ctypes.data_as(fp), 8
            g = lib.hmx_graph_from_knn(h, idx.ctypes.data_as(ip), dist.ctypes.data_as(fp), N, m, *out, None, None), lib.hmx_last_error(h)
            s = lib.hmx_snn_from_knn(h, idx.ctypes.data_as(ip), N, m, 0.1, *out), lib.hmx_last_error(h)
            return g, s
        for idx, N, m, status, text in ((np.array([[1, 3], [0, 2], [0, 1]]), 3, 2, ARG, b"[-1, N) (row 0)"),
                                        (np.array([[1, 2], [1, 2], [0, 1]]), 3, 2, ARG, b"row 1 lists its own cell"),
                                        (np.zeros((1, 129)), 1, 129, LIMIT, b"at most 128 neighbours")):
            g, s = both_from_knn(idx, N, m)
            assert g == s and g[0] == status and text in g[1], (g, s)
        X, indptr = np.zeros((10, 4)), np.zeros(11, dtype=np.int64)
        for k, text in ((1, b"2 <= k <= 129"), (130, b"2 <= k <= 129"), (11, b"k counts the cell itself: at most N")):
            g = lib.hmx_neighbor_graph(h, C.c_void_p(X.ctypes.data), 0, 0, 10, 4, k, None, None, indptr.ctypes.data_as(lp), None, None, 0,
                                       None, None), lib.hmx_last_error(h)
            s = lib.hmx_snn_graph(h, C.c_void_p(X.ctypes.data), 0, 0, 10, 4, k, 0.1, None, None, indptr.ctypes.data_as(lp), None, None, 0), lib.hmx_last_error(h)
            assert g[0] == s[0] == LIMIT and text in s[1] and b"n_neighbors" in g[1] and g[1].replace(b"n_neighbors", b"k") == s[1], (g, s)
    finally:
        lib.hmx_destroy(h)
