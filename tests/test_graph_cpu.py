"""The neighbour graph held to its spec (tests/graph_ref.py) without a GPU: the header, the library and the binding agree; the spec equals
independent arithmetic (scipy's fuzzy union of the directed membership matrix, the perplexity condition of the search, a hand-computed example,
scipy's connected components); the argument errors need no device (tests/test_gpu_graph.py runs the library)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graph_ref as gr  # noqa: E402
import helpers  # noqa: E402
import metrics_ref as mr  # noqa: E402
from harmony_amd import Harmony, _lib, connected_components, graph_connectivity, graph_from_knn, neighbors  # noqa: E402

sp = pytest.importorskip("scipy.sparse")
csgraph = pytest.importorskip("scipy.sparse.csgraph")


def test_graph_header_matches_the_library_and_the_binding():
    found = helpers.header_functions("harmony_mi355x_graph.h")
    mine = [n for n, _ in found]
    assert mine == ["hmx_graph_from_knn", "hmx_neighbor_graph", "hmx_graph_components"] and set(mine) == set(_lib.GRAPH_SIGNATURES)
    helpers.assert_header_stands_alone("harmony_mi355x_graph.h", mine)
    for name, types in found:
        helpers.assert_binding_matches(_lib.load(), name, types, _lib.GRAPH_SIGNATURES[name][1])


# ---- the spec against independent arithmetic -------------------------------------------------------------------------------------------------
def lists(N, m, d=5, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, d)) * rng.uniform(0.2, 3.0, size=(N, 1))
    idx, d2 = mr.knn(X, m)
    return idx.astype(np.int32), np.sqrt(d2).astype(np.float32)


@pytest.mark.parametrize("N,m", [(300, 14), (120, 1), (90, 64), (200, 29)])
def test_union_equals_scipys_fuzzy_union_of_the_directed_memberships(N, m):
    idx, dist = lists(N, m, seed=m)
    idx[3, m // 2:] = -1                                   # a row with unfilled slots
    w = gr.memberships(idx, dist)
    valid = idx >= 0
    A = sp.csr_matrix((w[valid], (np.repeat(np.arange(N), m)[valid.ravel()], idx[valid])), shape=(N, N))
    U = (A + A.T - A.multiply(A.T)).tocsr()
    U.sort_indices()
    indptr, indices, weights = gr.connectivities(idx, dist)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and weights.dtype == np.float32
    P = sp.csr_matrix((np.ones(valid.sum()), (np.repeat(np.arange(N), m)[valid.ravel()], idx[valid])), shape=(N, N))
    P = (P + P.T).tocsr()
    P.sort_indices()
    assert np.array_equal(indptr, P.indptr) and np.array_equal(indices, P.indices)      # the pattern is a function of idx alone
    dense = np.zeros((N, N))
    dense[np.repeat(np.arange(N), np.diff(indptr)), indices] = weights
    assert np.array_equal(dense, dense.T)
    assert np.abs(dense - U.toarray()).max() <= 2.0 ** -24
    assert not dense.diagonal().any() and indptr[N] <= 2 * N * m


def test_psum_of_sigma_meets_the_target_where_the_floor_does_not_decide():
    for N, m in ((400, 14), (300, 29), (150, 100)):
        idx, dist = lists(N, m, seed=7)
        rho, sigma = gr.smooth_knn(idx, dist)
        d = dist.astype(np.float64)
        floor = 1e-3 * d.sum(axis=1) / (m + 1)
        free = sigma > floor
        assert free.mean() > 0.9
        p = gr.psum(d, idx >= 0, rho, sigma)
        assert np.abs(p - np.log2(m + 1))[free].max() < 1e-5
        assert np.array_equal(rho, d[:, 0]) and (sigma > 0).all()


def test_hand_computed_four_cells():
    """cells on a line at 0, 1, 3, 7 with m = 1: every row has one neighbour at its rho, so psum = 1 = log2(2) at once, sigma = 1 and every
    directed weight is 1: 0 <-> 1 mutual, 2 -> 1, 3 -> 2; the union is the path 0 - 1 - 2 - 3 with unit weights"""
    idx = np.array([[1], [0], [1], [2]], dtype=np.int32)
    dist = np.array([[1.0], [1.0], [2.0], [4.0]], dtype=np.float32)
    rho, sigma = gr.smooth_knn(idx, dist)
    assert np.array_equal(rho, [1.0, 1.0, 2.0, 4.0]) and np.array_equal(sigma, [1.0, 1.0, 1.0, 1.0])
    indptr, indices, weights = gr.connectivities(idx, dist)
    assert indptr.tolist() == [0, 1, 3, 5, 6] and indices.tolist() == [1, 0, 2, 1, 3, 2] and weights.tolist() == [1.0] * 6
    # m = 2, cell 0 at distances 1 and 3: rho = 1, target log2(3); psum(s) = 1 + exp(-2 / s), so sigma = -2 / ln(log2(3) - 1)
    idx2 = np.array([[1, 2], [0, 2], [1, 0]], dtype=np.int32)
    dist2 = np.array([[1.0, 3.0], [1.0, 2.0], [2.0, 3.0]], dtype=np.float32)
    rho2, sigma2 = gr.smooth_knn(idx2, dist2)
    want = -2.0 / np.log(np.log2(3.0) - 1.0)
    assert rho2[0] == 1.0 and abs(1.0 + np.exp(-2.0 / sigma2[0]) - np.log2(3.0)) < 1e-5 and abs(sigma2[0] - want) < 1e-4 * want
    w = gr.memberships(idx2, dist2)
    assert w[0, 0] == 1.0 and abs(w[0, 1] - (np.log2(3.0) - 1.0)) < 1e-5


def test_degenerate_rows():
    """equal distances: psum = m for every sigma, the floor decides; all zero: rho = 0 and the floor is 1e-3 mean_all = 0, so sigma is what 64
    halvings leave of 1 (2^-64: zero against any distance), and w = 1; no valid entry: rho = sigma = 0 and an empty graph"""
    idx = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], dtype=np.int32)
    rho, sigma = gr.smooth_knn(idx, np.full((4, 3), 2.0, dtype=np.float32))
    assert np.array_equal(rho, np.full(4, 2.0)) and np.array_equal(sigma, np.full(4, 1e-3 * 1.5))
    rho, sigma = gr.smooth_knn(idx, np.zeros((4, 3), dtype=np.float32))
    assert not rho.any() and np.array_equal(sigma, np.full(4, 2.0 ** -64)) and np.array_equal(gr.memberships(idx, np.zeros((4, 3))), np.ones((4, 3)))
    rho, sigma = gr.smooth_knn(np.full((2, 3), -1), np.ones((2, 3)))
    assert not rho.any() and not sigma.any() and gr.connectivities(np.full((2, 3), -1), np.ones((2, 3)))[0].tolist() == [0, 0, 0]


def relabelled(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_components_equal_scipys(seed):
    rng = np.random.default_rng(seed)
    N = 400
    A = sp.random(N, N, density=0.004, random_state=seed, format="csr")
    A = (A + A.T).tocsr()
    A.sort_indices()
    n, lab = csgraph.connected_components(A, directed=False)
    comp = gr.components(A.indptr, A.indices)
    assert relabelled(comp, lab) and len(set(comp.tolist())) == n and n > 1
    assert all(comp[i] == np.nonzero(comp == comp[i])[0][0] for i in range(N))      # the smallest index names the component
    labels = rng.integers(-1, 3, N)
    coo = A.tocoo()
    keep = (labels[coo.row] == labels[coo.col]) & (labels[coo.row] >= 0)
    F = sp.csr_matrix((np.ones(keep.sum()), (coo.row[keep], coo.col[keep])), shape=(N, N))
    n2, lab2 = csgraph.connected_components(F, directed=False)
    comp2 = gr.components(A.indptr, A.indices, labels)
    assert relabelled(comp2, lab2) and np.all(comp2[labels < 0] == np.nonzero(labels < 0)[0])


def two_label_example():
    """label 0: the path 0-1-2-3 (whole); label 1: 4-5 and 6-7, joined only through cell 0 of label 0"""
    edges = [(0, 1), (1, 2), (2, 3), (4, 5), (6, 7), (5, 0), (0, 6)]
    r = np.array([e[0] for e in edges] + [e[1] for e in edges])
    c = np.array([e[1] for e in edges] + [e[0] for e in edges])
    A = sp.csr_matrix((np.ones(r.size), (r, c)), shape=(8, 8))
    A.sort_indices()
    return A, np.array([0, 0, 0, 0, 1, 1, 1, 1])


def test_graph_connectivity_values():
    A, labels = two_label_example()
    assert gr.graph_connectivity(A.indptr, A.indices, labels, 2) == (1 + 1 / 2) / 2
    assert gr.graph_connectivity(A.indptr, A.indices, labels, 3) == (1 + 1 / 2) / 2      # a level without cells is left out
    comp = gr.components(A.indptr, A.indices)
    assert not comp.any()
    B = sp.block_diag([np.ones((3, 3)) - np.eye(3), np.ones((5, 5)) - np.eye(5)]).tocsr()
    own = gr.components(B.indptr, B.indices)
    assert gr.graph_connectivity(B.indptr, B.indices, (own > 0).astype(int), 2) == 1.0


# ---- every argument error is raised before a device is needed --------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device():
    X = np.random.default_rng(0).normal(size=(40, 5))
    for bad in (1, 130, 2.5, 41):
        with pytest.raises(ValueError, match="n_neighbors"):
            neighbors(X, n_neighbors=bad)
    with pytest.raises(ValueError, match="cells x PCs"):
        neighbors(np.zeros(5))
    ok_i, ok_d = np.array([[1, 2], [0, 2], [0, 1]]), np.ones((3, 2))
    for idx, dist, msg in ((np.array([[1, 3], [0, 2], [0, 1]]), ok_d, r"\[-1, 3\)"), (np.array([[1, -2], [0, 2], [0, 1]]), ok_d, r"\[-1, 3\)"),
                           (np.array([[1, 2], [1, 2], [0, 1]]), ok_d, "own cell"), (ok_i, np.array([[1, np.nan], [1, 1], [1, 1]]), "NaN"),
                           (ok_i, np.ones((3, 3)), "one shape"), (ok_i.astype(float), ok_d, "integers"),
                           (np.zeros((3, 129), dtype=int), np.ones((3, 129)), "at most 128")):
        with pytest.raises(ValueError, match=msg):
            graph_from_knn(idx, dist)
    A, labels = two_label_example()
    with pytest.raises(ValueError, match="one label per cell"):
        connected_components(A, labels[:5])
    with pytest.raises(ValueError, match="square"):
        connected_components(sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(ValueError, match="indptr"):
        connected_components((np.array([0, 2, 1]), np.array([1, 0])))
    with pytest.raises(ValueError, match="column"):
        graph_connectivity(A, {"cell_type": labels}, "no_such_column")
    with pytest.raises(ValueError, match="one label per cell"):
        graph_connectivity(A, {"cell_type": labels[:3]}, "cell_type")
    assert callable(Harmony.neighbors)


def test_library_argument_errors_come_before_the_device():
    lib = _lib.load()
    ip, fp, lp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    h = C.c_void_p(lib.hmx_create())
    try:
        def lists_call(idx, dist, N, m, cap=100):
            idx, dist = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float32)
            indptr, indices, weights = np.zeros(N + 1, dtype=np.int64), np.zeros(100, dtype=np.int32), np.zeros(100, dtype=np.float32)
            return lib.hmx_graph_from_knn(h, idx.ctypes.data_as(ip), dist.ctypes.data_as(fp), N, m, indptr.ctypes.data_as(lp),
                                          indices.ctypes.data_as(ip), weights.ctypes.data_as(fp), cap, None, None)
        ok_i, ok_d = np.array([[1, 2], [0, 2], [0, 1]]), np.ones((3, 2))
        ARG, LIMIT = 1, 7
        assert lists_call(np.array([[1, 3], [0, 2], [0, 1]]), ok_d, 3, 2) == ARG and b"[-1, N)" in lib.hmx_last_error(h)
        assert lists_call(np.array([[1, -2], [0, 2], [0, 1]]), ok_d, 3, 2) == ARG
        assert lists_call(np.array([[1, 2], [1, 2], [0, 1]]), ok_d, 3, 2) == ARG and b"own cell" in lib.hmx_last_error(h)
        assert lists_call(ok_i, np.array([[1, np.nan], [1, 1], [1, 1]]), 3, 2) == ARG and b"NaN" in lib.hmx_last_error(h)
        assert lists_call(ok_i, ok_d, 3, 2, cap=-1) == ARG
        assert lists_call(ok_i, ok_d, 0, 2) == ARG and lists_call(ok_i, ok_d, 3, 0) == ARG
        assert lists_call(np.zeros((1, 129)), np.zeros((1, 129)), 1, 129) == LIMIT
        X = np.zeros((10, 4))
        out = np.zeros(11, dtype=np.int64)

        def graph_call(N, d, nn, x=X, indptr=out):
            return lib.hmx_neighbor_graph(h, None if x is None else C.c_void_p(x.ctypes.data), 0, 0, N, d, nn, None, None,
                                          None if indptr is None else indptr.ctypes.data_as(lp), None, None, 0, None, None)
        assert graph_call(10, 4, 1) == LIMIT and graph_call(10, 4, 130) == LIMIT and graph_call(10, 4, 11) == LIMIT
        assert graph_call(10, 129, 5) == LIMIT and graph_call(0, 4, 5) == ARG and graph_call(10, 4, 5, indptr=None) == ARG
        assert graph_call(10, 4, 5, x=None) == 6                                  # HMX_ERR_STATE: no embedding on a fresh handle
        comp = np.zeros(3, dtype=np.int32)

        def cc_call(indptr, indices, labels=None, N=3):
            indptr, indices = np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32)
            labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
            return lib.hmx_graph_components(h, N, indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip),
                                            None if labels is None else labels.ctypes.data_as(ip), comp.ctypes.data_as(ip), None)
        assert cc_call([1, 1, 2, 2], [1, 0]) == ARG and cc_call([0, 2, 1, 2], [1, 0]) == ARG and cc_call([0, 4, 4, 4], [1, 2, 1, 2]) == ARG
        assert cc_call([0, 1, 2, 2], [1, 0], labels=[0, -2, 0]) == ARG and cc_call([0, 1, 2, 2], [1, 0], N=0) == ARG
        out1 = (C.c_double * 1)()
        assert lib.hmx_get(h, b"graph:cc_rounds", out1, 1) == 1 and lib.hmx_get(h, b"timer:graph", out1, 1) == 1
    finally:
        lib.hmx_destroy(h)
