"""Louvain clustering held to its spec (tests/louvain_ref.py) without a GPU: the header, the library and the binding agree; every argument
error that the host can see is raised before a device is needed; the hash; the spec on graphs small enough to check by hand, against a
plain sequential Louvain (and networkx where it imports), and its modularity against a dense matrix (tests/test_gpu_louvain.py runs the
library).

The quality bar: Q_spec >= 0.95 Q_seq on every input.  The hashed sub-rounds move eight times fewer nodes at once than a synchronous sweep,
which is what keeps a ring or a path from collapsing; the worst ratio measured is 0.966, on the path of 12 cells, and the margin covers a
sequential Louvain that visits the nodes in another order."""
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

import helpers  # noqa: E402
import louvain_ref as lr  # noqa: E402
import metrics_ref as mr  # noqa: E402
import snn_ref as sr  # noqa: E402
from harmony_amd import Harmony, _lib, louvain  # noqa: E402
from harmony_amd.louvain import seurat_order  # noqa: E402

HEADER = "harmony_mi355x_louvain.h"


def test_louvain_header_matches_the_library_and_the_binding():
    found = helpers.header_functions(HEADER)
    mine = [n for n, _ in found]
    assert mine == ["hmx_louvain"] and set(mine) == set(_lib.LOUVAIN_SIGNATURES)
    for other, table in helpers.PUBLIC_HEADERS:            # every header before this one: none names the function, no other table binds it
        assert other != HEADER and not (set(mine) & helpers.header_names(other)), other
        assert not (set(mine) & set(getattr(_lib, table))), table
    tables = [t for t in dir(_lib) if t.endswith("SIGNATURES") and t != "LOUVAIN_SIGNATURES"]
    assert len(tables) >= 10 and not any(set(mine) & set(getattr(_lib, t)) for t in tables)
    for name, types in found:
        helpers.assert_binding_matches(_lib.load(), name, types, _lib.LOUVAIN_SIGNATURES[name][1])


# ---- the hash ----------------------------------------------------------------------------------------------------------------------------------------
def test_fmix32_known_answers():
    """murmur3's finaliser: 0 is its fixed point; the other values follow from the definition with Python's integers, step by step"""
    assert lr.fmix32(0) == 0

    def by_hand(x):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) % 2 ** 32
        x ^= x >> 13
        x = (x * 0xC2B2AE35) % 2 ** 32
        return x ^ (x >> 16)
    assert lr.fmix32(1) == by_hand(1) == 0x514E28B7
    assert lr.fmix32(0xFFFFFFFF) == by_hand(0xFFFFFFFF) == 0x81F16F39
    xs = [2, 64, 65, 12345, 2 ** 31, 2 ** 32 - 2]
    assert lr.fmix32_array(np.array(xs)).tolist() == [by_hand(x) for x in xs] == [lr.fmix32(x) for x in xs]
    b = lr.buckets(4096, 3, 1)
    assert b.min() == 0 and b.max() == 7 and np.bincount(b).min() > 4096 / 8 * 0.8      # the sub-rounds are of similar size
    assert b.tolist()[:64] == [lr.fmix32(i ^ lr.fmix32(64 * 3 + 1 + 1)) & 7 for i in range(64)]
    assert not np.array_equal(b, lr.buckets(4096, 4, 1)) and not np.array_equal(b, lr.buckets(4096, 3, 2))


# ---- the spec on graphs that can be checked by hand ------------------------------------------------------------------------------------------------
def test_two_cliques_and_isolated_cells():
    r = lr.louvain(*lr.two_cliques())
    assert r.labels.tolist() == [0] * 6 + [1] * 6 + [2, 3] and r.n_clusters == 4 and r.labels.dtype == np.int32
    # 62 directed entries; each clique: 30 inside, total degree 31: Q = 2 (30 / 62 - (31 / 62)^2)
    assert abs(r.modularity - 2 * (30 / 62 - 0.25)) < 1e-15
    assert r.level_clusters == [4] and r.best_level == 1 and r.sweeps == sum(r.level_sweeps) + 1      # one more level, in which nothing moved


def test_star_and_complete_graph_are_one_cluster():
    for g, n in ((lr.star(40), 40), (lr.complete(20), 20)):
        for resolution, q in ((1.0, 0.0), (0.8, 0.2)):
            r = lr.louvain(*g, resolution=resolution)
            assert r.labels.tolist() == [0] * n and r.n_clusters == 1 and abs(r.modularity - q) < 1e-15


def test_path_of_twelve():
    r = lr.louvain(*lr.path(12))
    assert r.labels.tolist() == [0] * 5 + [1] * 4 + [2] * 3      # three runs: five, four and three cells (the optimum, 4 + 4 + 4, is 0.4835)
    # 22 directed entries; the runs hold 8, 6 and 4 of them inside, at total degrees 9, 8 and 5
    assert abs(r.modularity - (18 / 22 - (81 + 64 + 25) / 22 ** 2)) < 1e-15
    assert r.level_clusters == [5, 3] and r.best_level == 2


def test_ring_is_cut_into_runs():
    r = lr.louvain(*lr.ring(300))
    assert np.all(np.diff(r.labels) >= 0) or r.labels[0] == r.labels[-1]      # contiguous runs (the first may wrap around)
    cuts = int((np.diff(r.labels) != 0).sum())
    assert r.n_clusters in (cuts, cuts + 1) and 10 <= r.n_clusters <= 30 and r.modularity > 0.87


def test_edgeless_and_tiny_graphs():
    empty = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    r = lr.louvain(*empty)
    assert r.labels.tolist() == [0, 1, 2, 3, 4] and r.n_clusters == 5 and r.modularity == 0.0 and r.level_clusters == [] and r.sweeps == 0
    r = lr.louvain(*lr.csr_of_edges(4, [(0, 1, 0.0), (2, 3, 0.0)]))      # M = 0
    assert r.n_clusters == 4 and r.modularity == 0.0 and r.best_level == 0
    r = lr.louvain(*lr.path(2))
    assert r.labels.tolist() == [0, 0] and r.modularity == 0.0 and r.best_level == 1      # Q of the singletons is -1/2
    with_diag = lr.csr_of_edges(14, [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(6 + i, 6 + j) for i in range(6) for j in range(i + 1, 6)]
                                + [(5, 6)], diagonal=True)
    a, b = lr.louvain(*with_diag), lr.louvain(*lr.two_cliques())
    assert np.array_equal(a.labels, b.labels) and a.modularity == b.modularity      # the diagonal is ignored


def test_caps_and_counters_of_the_spec():
    g = planted_graph(600, 4)[0]
    r = lr.louvain(*g, max_sweeps=1)
    assert all(s == 1 for s in r.level_sweeps) and len(r.level_sweeps) > 1
    r = lr.louvain(*g, max_levels=1)
    assert len(r.level_clusters) == 1 and r.sweeps == r.level_sweeps[0] and r.best_level == 1


def test_seurat_order():
    lab = np.array([5, 5, 2, 2, 9, 2, 7, 7])             # sizes: 2 -> 3; 5 and 7 -> 2 (5's first cell is earlier); 9 -> 1
    assert lr.seurat_order(lab).tolist() == [1, 1, 0, 0, 3, 0, 2, 2] == seurat_order(lab).tolist()


# ---- quality: against a sequential Louvain, networkx and the planted labels ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_graph(N, groups):
    X, lab = lr.planted(N, groups)
    return sr.snn(mr.knn(X, 19)[0].astype(np.int32), 1.0 / 15.0)[:3], lab


@functools.lru_cache(maxsize=None)
def quality_inputs():
    out = {"planted %d" % N: planted_graph(N, G) for N, G in ((600, 4), (1500, 7), (3000, 12))}
    X = np.random.default_rng(1).normal(size=(1500, 10))
    out["structureless"] = (sr.snn(mr.knn(X, 19)[0].astype(np.int32), 1.0 / 15.0)[:3], None)
    out.update({"ring 300": (lr.ring(300), None), "path 12": (lr.path(12), None), "star 40": (lr.star(40), None),
                "complete 20": (lr.complete(20), None), "two cliques": (lr.two_cliques(), None)})
    return out


def networkx_q(g, resolution):
    nx = pytest.importorskip("networkx")
    indptr, indices, weights = g
    G = nx.Graph()
    G.add_nodes_from(range(indptr.size - 1))
    src = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    G.add_weighted_edges_from([(int(a), int(b), float(w)) for a, b, w in zip(src, indices, weights) if a < b])
    return nx.community.modularity(G, nx.community.louvain_communities(G, seed=0, resolution=resolution), resolution=resolution)


@pytest.mark.parametrize("resolution", [1.0, 0.8])
@pytest.mark.parametrize("name", ["planted 600", "planted 1500", "planted 3000", "structureless", "ring 300", "path 12", "star 40",
                                  "complete 20", "two cliques"])
def test_quality_against_a_sequential_louvain(name, resolution):
    g, planted = quality_inputs()[name]
    r = lr.louvain(*g, resolution=resolution)
    seq_labels, q_seq = lr.sequential(*g, resolution=resolution)
    print("%s, resolution %.1f: Q %.5f, sequential %.5f, ratio %.4f; %d clusters, levels %s, sweeps %s"
          % (name, resolution, r.modularity, q_seq, r.modularity / q_seq if q_seq else 1.0, r.n_clusters, r.level_clusters, r.level_sweeps))
    assert r.modularity >= 0.95 * q_seq
    assert lr.partition_modularity(*g, r.labels, resolution) == r.modularity      # the returned labels carry the returned Q
    assert abs(lr.partition_modularity(*g, seq_labels, resolution) - q_seq) < 1e-12
    if planted is not None:
        assert lr.adjusted_rand(r.labels, planted) >= 0.99


@pytest.mark.parametrize("name", ["planted 600", "structureless", "ring 300", "path 12", "two cliques"])
def test_quality_against_networkx(name):
    g, _ = quality_inputs()[name]
    for resolution in (1.0, 0.8):
        q_nx = networkx_q(g, resolution)
        r = lr.louvain(*g, resolution=resolution)
        print("%s, resolution %.1f: Q %.5f, networkx %.5f" % (name, resolution, r.modularity, q_nx))
        assert r.modularity >= 0.95 * q_nx


@pytest.mark.parametrize("resolution", [1.0, 0.5, 2.0])
def test_spec_modularity_equals_the_dense_expression(resolution):
    """Q = sum_c (sum of A inside c / M - resolution (degree of c / M)^2) from a dense matrix of the integer weights, N <= 300"""
    X = np.random.default_rng(2).normal(size=(300, 6))
    g = sr.snn(mr.knn(X, 9)[0].astype(np.int32), 1.0 / 15.0)[:3]
    A = sp.csr_matrix((np.rint(g[2].astype(np.float64) * 2 ** 24), g[1], g[0]), shape=(300, 300)).toarray()
    np.fill_diagonal(A, 0.0)
    M = A.sum()
    r = lr.louvain(*g, resolution=resolution)
    for labels in (r.labels, np.arange(300) % 7, np.zeros(300, dtype=int)):
        dense = sum(A[np.ix_(labels == c, labels == c)].sum() / M - resolution * (A[labels == c].sum() / M) ** 2 for c in np.unique(labels))
        assert abs(lr.partition_modularity(*g, labels, resolution) - dense) < 1e-12
    assert lr.partition_modularity(*g, r.labels, resolution) == r.modularity


# ---- every argument error is raised before a device is needed --------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device():
    indptr, indices, weights = lr.two_cliques()
    g = sp.csr_matrix((weights, indices, indptr), shape=(14, 14))
    for bad in (0.0, -1.0, 100.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="resolution"):
            louvain(g, resolution=bad)
    for bad in (0, 65, 2.5, float("nan")):
        with pytest.raises(ValueError, match="max_levels"):
            louvain(g, max_levels=bad)
    for bad in (0, 4097, 1.5):
        with pytest.raises(ValueError, match="max_sweeps"):
            louvain(g, max_sweeps=bad)
    with pytest.raises(ValueError, match="square"):
        louvain(sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(ValueError, match="scipy.sparse matrix or"):
        louvain(np.ones(5))
    for w, msg in ((weights * 1.5, r"\[0, 1\]"), (np.where(np.arange(weights.size) == 3, np.nan, weights), r"\[0, 1\]"),
                   (-weights, r"\[0, 1\]")):
        with pytest.raises(ValueError, match=msg):
            louvain((indptr, indices, w.astype(np.float32)))
    w = weights.copy()
    w[0] = 0.5
    with pytest.raises(ValueError, match="different weights"):
        louvain((indptr, indices, w))
    one_way = sp.csr_matrix(([1.0], ([0], [1])), shape=(3, 3))
    with pytest.raises(ValueError, match="no mirror"):
        louvain(one_way)
    j = indices.copy()
    j[0] = 14
    with pytest.raises(ValueError, match="outside"):
        louvain((indptr, j, weights))
    assert callable(Harmony.clusters)


def test_library_argument_errors_come_before_the_device():
    lib = _lib.load()
    ip, fp, lp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    h = C.c_void_p(lib.hmx_create())
    ARG, LIMIT = 1, 7
    indptr, indices, weights = lr.two_cliques()
    try:
        def call(N=14, resolution=1.0, max_levels=10, max_sweeps=32, ptr=indptr, null=None):
            ptr = np.ascontiguousarray(ptr, dtype=np.int64)
            labels, n, q = np.zeros(64, dtype=np.int32), C.c_int32(0), C.c_double(0.0)
            arg = {"indptr": ptr.ctypes.data_as(lp), "indices": indices.ctypes.data_as(ip), "weights": weights.ctypes.data_as(fp),
                   "labels": labels.ctypes.data_as(ip), "n_clusters": C.byref(n), "modularity": C.byref(q)}
            if null:
                arg[null] = None
            return lib.hmx_louvain(h, arg["indptr"], arg["indices"], arg["weights"], N, resolution, max_levels, max_sweeps, arg["labels"],
                                   arg["n_clusters"], arg["modularity"], None, None, None)
        for null in ("indptr", "indices", "weights", "labels", "n_clusters", "modularity"):
            assert call(null=null) == ARG, null
        assert call(N=0) == ARG and call(N=-3) == ARG
        for bad in (0.0, -1.0, 100.5, float("nan"), float("inf")):
            assert call(resolution=bad) == ARG and b"resolution" in lib.hmx_last_error(h)
        for bad in (0, 65, -1):
            assert call(max_levels=bad) == ARG and b"max_levels" in lib.hmx_last_error(h)
        for bad in (0, 4097, -1):
            assert call(max_sweeps=bad) == ARG and b"max_sweeps" in lib.hmx_last_error(h)
        shifted = indptr.copy()
        shifted[0] = 1
        assert call(ptr=shifted) == ARG and b"start at 0" in lib.hmx_last_error(h)
        down = indptr.copy()
        down[3] = down[2] - 1
        assert call(ptr=down) == ARG and b"ascend" in lib.hmx_last_error(h)
        assert call(N=2, ptr=np.array([0, 3, 4])) == ARG      # a row longer than N
        assert call(N=2000000001) == LIMIT                   # (refused before a row is read)
        assert call(N=3, ptr=np.array([0, 0, 0, 2 ** 31])) == ARG and call(N=2 ** 31 // 1000 + 1000, ptr=np.arange(2 ** 31 // 1000 + 1001) * 1000) == LIMIT
        assert lib.hmx_louvain(None, None, None, None, 1, 1.0, 1, 1, None, None, None, None, None, None) == ARG
        assert lib.hmx_set_int(h, b"louvain_short_cap", -2) == ARG and lib.hmx_set_int(h, b"louvain_short_cap", 16) == 0
        out1 = (C.c_double * 1)()
        for key in (b"louvain:levels", b"louvain:best_level", b"louvain:sweeps", b"louvain:clusters", b"louvain:short_cap", b"louvain:long_rows",
                    b"timer:louvain"):
            assert lib.hmx_get(h, key, out1, 1) == 1, key
        assert lib.hmx_get(h, b"louvain:short_cap", out1, 1) == 1 and out1[0] == 16
        assert lib.hmx_set_int(h, b"louvain_short_cap", -1) == 0 and lib.hmx_get(h, b"louvain:short_cap", out1, 1) == 1 and out1[0] >= 256
    finally:
        lib.hmx_destroy(h)
