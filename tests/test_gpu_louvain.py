"""Louvain clustering on the MI355X against its spec (tests/louvain_ref.py).  The spec and the kernels compute the same integers and the
same three-operation fp64 score in the same schedule, so labels, the clusters and sweeps of every level and the modularities (doubles) are
compared with np.array_equal: there is no tolerance.

Sizes the kernels take another path at: rows of up to 64, 128, .. 1024 entries (the LDS sort's padding) | above "louvain:short_cap" (one
workgroup, windows of community ids); one window | several; a community's segment of <= 128 keys | longer (the graph stage's sort); runs
that end inside a chunk of 64 keys | span chunks; a scan of <= 2048 counts per workgroup | more; levels 0 | 1 and later (inner weights)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
sp = pytest.importorskip("scipy.sparse")

import graph_ref as gr  # noqa: E402
import louvain_ref as lr  # noqa: E402
import metrics_ref as mr  # noqa: E402
import snn_ref as sr  # noqa: E402
from bench_data import synth  # noqa: E402
from harmony_amd import RunHarmony, louvain  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402

ip, fp, lp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_double)
KEYS = ("levels", "best_level", "sweeps", "clusters", "long_rows", "short_cap")


def get(h, key):
    out = (C.c_double * 1)()
    assert h.lib.hmx_get(h.h, key, out, 1) == 1, key
    return out[0]


def library(g, resolution=1.0, max_levels=10, max_sweeps=32, short_cap=None):
    """hmx_louvain on the graph g = (indptr, indices, weights) -> (status, the outputs and counters as a dict)"""
    indptr = np.ascontiguousarray(g[0], dtype=np.int64)
    indices, weights = np.ascontiguousarray(g[1], dtype=np.int32), np.ascontiguousarray(g[2], dtype=np.float32)
    N = indptr.size - 1
    labels = np.full(N, -7, dtype=np.int32)
    n, q = C.c_int32(-7), C.c_double(-7.0)
    lc, ls, lq = np.full(max_levels, -7, dtype=np.int32), np.full(max_levels, -7, dtype=np.int32), np.full(max_levels, -7.0)
    with _Handle() as h:
        if short_cap is not None:
            assert h.lib.hmx_set_int(h.h, b"louvain_short_cap", short_cap) == 0
        status = h.lib.hmx_louvain(h.h, indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip), weights.ctypes.data_as(fp), N, resolution,
                                   max_levels, max_sweeps, labels.ctypes.data_as(ip), C.byref(n), C.byref(q), lc.ctypes.data_as(ip),
                                   ls.ctypes.data_as(ip), lq.ctypes.data_as(dp))
        out = {k: int(get(h, b"louvain:" + k.encode())) for k in KEYS}
        out.update(labels=labels, n_clusters=n.value, modularity=q.value, level_clusters=lc, level_sweeps=ls, level_modularity=lq,
                   timer=get(h, b"timer:louvain"), error=h.lib.hmx_last_error(h.h).decode())
    return status, out


def check(g, what, **kw):
    """the library against the spec on g: equal bits everywhere; -> (the library's outputs, the spec's)"""
    cap = kw.pop("short_cap", None)
    want = lr.louvain(*g, **kw)
    status, got = library(g, short_cap=cap, **kw)
    L = len(want.level_clusters)
    print("louvain %s: N=%d entries=%d %s -> clusters %d Q %.6f; levels %s sweeps %s Q %s; best %d; long rows %d; %.1f ms"
          % (what, g[0].size - 1, g[1].size, kw, want.n_clusters, want.modularity, want.level_clusters, want.level_sweeps,
             ["%.6f" % v for v in want.level_modularity], want.best_level, got["long_rows"], got["timer"]))
    assert status == 0, got["error"]
    assert got["levels"] == L and got["best_level"] == want.best_level and got["sweeps"] == want.sweeps, what
    assert np.array_equal(got["level_clusters"][:L], np.array(want.level_clusters, dtype=np.int32)), what
    assert np.array_equal(got["level_sweeps"][:L], np.array(want.level_sweeps, dtype=np.int32)), what
    assert np.array_equal(got["level_modularity"][:L].view(np.uint64), np.array(want.level_modularity, dtype=np.float64).view(np.uint64)), what
    assert np.all(got["level_clusters"][L:] == -7) and np.all(got["level_modularity"][L:] == -7.0)      # nothing written past the recorded levels
    assert np.array_equal(got["labels"], want.labels), what
    assert got["n_clusters"] == want.n_clusters == got["clusters"], what
    assert np.float64(got["modularity"]).view(np.uint64) == np.float64(want.modularity).view(np.uint64), what
    return got, want


# ---- (a) SNN graphs of the spec's own neighbour lists ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def snn_graph(N, m):
    Z, _, _ = synth(N, d=20, levels=(4,), seed=5)
    return sr.snn(mr.knn(Z, m)[0].astype(np.int32), 1.0 / 15.0)[:3]


@pytest.mark.parametrize("resolution", [0.5, 0.8, 1.0, 2.0])
@pytest.mark.parametrize("N,m", [(2000, 19), (600, 29)])
def test_snn_graphs(N, m, resolution):
    got, _ = check(snn_graph(N, m), "snn", resolution=resolution)
    assert got["long_rows"] == int((np.diff(snn_graph(N, m)[0]) > got["short_cap"]).sum())


def test_more_cells_than_one_workgroup_scans():
    check(snn_graph(5000, 9), "snn 5000")


def test_neighbors_style_float_weights():
    Z, _, _ = synth(1500, d=20, levels=(4,), seed=5)
    idx, dist = mr.knn(Z, 14)[:2]
    g = gr.connectivities(idx.astype(np.int32), np.sqrt(np.maximum(np.asarray(dist, dtype=np.float64), 0.0)).astype(np.float32))
    assert len(np.unique(g[2])) > 1000 and g[2].max() <= 1.0
    check(g, "connectivities")
    check(g, "connectivities", resolution=0.8)


# ---- (b) the hand-checkable graphs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring", "path", "star", "complete", "cliques"])
@pytest.mark.parametrize("resolution", [1.0, 0.8])
def test_small_graphs(name, resolution):
    g = {"ring": lambda: lr.ring(300), "path": lambda: lr.path(12), "star": lambda: lr.star(40), "complete": lambda: lr.complete(20),
         "cliques": lr.two_cliques}[name]()
    got, want = check(g, name, resolution=resolution)
    if name == "cliques":
        assert got["labels"].tolist() == [0] * 6 + [1] * 6 + [2, 3] and want.n_clusters == 4


def test_stored_diagonal_and_explicit_zeros():
    indptr, indices, weights = [a.copy() for a in snn_graph(600, 29)]
    rows = np.repeat(np.arange(600), np.diff(indptr))
    assert (rows == indices).sum() == 600                  # the SNN graph stores its diagonal
    zero = ((rows + indices) % 5 == 0) & (rows != indices)      # a symmetric choice of edges
    weights[zero] = 0.0
    assert zero.sum() > 1000
    check((indptr, indices, weights), "diagonal and zeros")
    plain = lr.csr_of_edges(14, [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(6 + i, 6 + j) for i in range(6) for j in range(i + 1, 6)]
                            + [(5, 6), (12, 13, 0.0), (0, 12, 0.0)], diagonal=True)
    check(plain, "cliques with a diagonal and two edges of weight 0")


def test_lattice_where_every_score_ties():
    """a 16 x 16 torus of unit weights: at the first sub-round every neighbour of a cell scores the same, so the smallest id decides"""
    side = 16
    cell = np.arange(side * side).reshape(side, side)
    edges = [(int(cell[r, c]), int(cell[(r + 1) % side, c])) for r in range(side) for c in range(side)]
    edges += [(int(cell[r, c]), int(cell[r, (c + 1) % side])) for r in range(side) for c in range(side)]
    g = lr.csr_of_edges(side * side, edges)
    assert np.all(np.diff(g[0]) == 4)
    for resolution in (1.0, 0.5):
        check(g, "torus", resolution=resolution)


def test_one_and_two_cells_and_no_edges():
    one = (np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    got, _ = check(one, "one cell")
    assert got["labels"].tolist() == [0] and got["n_clusters"] == 1 and got["modularity"] == 0.0 and got["levels"] == 0
    one_diag = (np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.float32))
    check(one_diag, "one cell with its diagonal")
    got, _ = check(lr.path(2), "two cells")
    assert got["labels"].tolist() == [0, 0]
    empty = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    got, _ = check(empty, "no edges")
    assert got["labels"].tolist() == [0, 1, 2, 3, 4] and got["n_clusters"] == 5 and got["modularity"] == 0.0 and got["sweeps"] == 0
    zeros = lr.csr_of_edges(5, [(0, 1, 0.0), (2, 3, 0.0)])
    got, _ = check(zeros, "edges of weight 0 only")       # M = 0
    assert got["n_clusters"] == 5 and got["levels"] == 0


# ---- (c) the caps and the best level ---------------------------------------------------------------------------------------------------------------
def test_caps_end_the_call():
    g = snn_graph(600, 29)
    got, want = check(g, "max_sweeps = 1", max_sweeps=1)
    assert all(s == 1 for s in want.level_sweeps) and got["levels"] > 1
    got, want = check(g, "max_levels = 1", max_levels=1)
    assert got["levels"] == 1 and got["sweeps"] == want.level_sweeps[0] > 1
    got, _ = check(g, "both", max_levels=1, max_sweeps=1)
    assert got["levels"] == 1 and got["sweeps"] == 1


def test_a_later_level_lowers_q():
    """structureless cells, 2 sweeps per level, resolution 2: the third level's modularity is below the second's, which is returned"""
    X = np.random.default_rng(5).normal(size=(300, 10))
    g = sr.snn(mr.knn(X, 9)[0].astype(np.int32), 1.0 / 15.0)[:3]
    got, want = check(g, "best level", resolution=2.0, max_sweeps=2)
    assert want.best_level == 2 and len(want.level_modularity) == 3 and want.level_modularity[2] < want.level_modularity[1]
    assert got["n_clusters"] == want.level_clusters[1] and got["modularity"] == want.level_modularity[1]


# ---- (d) both sides of short_cap, and the long path alone ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short_cap():
    with _Handle() as h:
        return int(get(h, b"louvain:short_cap"))


@pytest.mark.parametrize("extra", [0, 1, 100])
def test_star_with_a_hub_row_around_short_cap(extra):
    """a star whose hub row holds short_cap + extra entries, and a ring through the leaves so that levels follow"""
    n = short_cap() + extra + 1
    g = lr.csr_of_edges(n, [(0, i) for i in range(1, n)] + [(i, i + 1, 0.5) for i in range(1, n - 1)])
    lens = np.diff(g[0])
    assert lens[0] == short_cap() + extra
    got, _ = check(g, "star and ring, hub row of %d" % lens[0])
    assert got["long_rows"] == int((lens > short_cap()).sum()) == (1 if extra else 0)


def test_everything_through_the_long_path():
    g = snn_graph(600, 29)
    got, want = check(g, "long path alone", short_cap=0, resolution=0.8)
    assert got["short_cap"] == 0 and got["long_rows"] == int((np.diff(g[0]) > 0).sum()) == 600
    status, short = library(g, resolution=0.8)
    assert status == 0 and np.array_equal(short["labels"], got["labels"]) and short["long_rows"] == 0
    # several windows of community ids: more cells than one window holds, every row long
    big = snn_graph(5000, 9)
    got, _ = check(big, "long path, several windows", short_cap=0)
    assert got["long_rows"] == 5000
    check(g, "a cap inside the rows' lengths", short_cap=int(np.median(np.diff(g[0]))))


# ---- (e) the whole call --------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    g = snn_graph(2000, 19)
    a, b = library(g, resolution=0.8)[1], library(g, resolution=0.8)[1]
    for key in ("labels", "level_clusters", "level_sweeps"):
        assert np.array_equal(a[key], b[key])
    assert np.array_equal(a["level_modularity"].view(np.uint64), b["level_modularity"].view(np.uint64)) and a["modularity"] == b["modularity"]


def test_python_louvain_numbers_clusters_by_size():
    g = snn_graph(2000, 19)
    want = lr.louvain(*g, resolution=0.8)
    res = louvain(sp.csr_matrix((g[2], g[1], g[0]), shape=(2000, 2000)), resolution=0.8)
    assert res.labels.dtype == np.int32 and np.array_equal(res.labels, lr.seurat_order(want.labels))
    sizes = np.bincount(res.labels)
    assert np.all(np.diff(sizes) <= 0) and res.n_clusters == want.n_clusters == sizes.size
    assert res.modularity == want.modularity
    assert res.levels == list(zip(want.level_clusters, want.level_sweeps, want.level_modularity))
    tri = louvain((g[0], g[1], g[2]), resolution=0.8)      # the triple form
    assert np.array_equal(tri.labels, res.labels)


def test_harmony_clusters_is_snn_then_louvain():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines_small.npz"))
    meta = {"dataset": fx["dataset_levels"][fx["dataset"]]}
    obj = RunHarmony(fx["pcs"], meta, "dataset", return_object=True, verbose=False, seed=1, max_iter=2, nclust=10)
    a = obj.clusters()
    b = louvain(obj.snn(k=20, prune=1.0 / 15.0)[1], 0.8)
    assert np.array_equal(a.labels, b.labels) and a.n_clusters == b.n_clusters and a.modularity == b.modularity and a.levels == b.levels
    assert a.n_clusters >= 2 and obj.timer("louvain") > 0
    g = obj.snn()[1]
    want = lr.louvain(g.indptr, g.indices, g.data, resolution=0.8)
    assert np.array_equal(a.labels, lr.seurat_order(want.labels)) and a.modularity == want.modularity


# ---- (f) malformed graphs ------------------------------------------------------------------------------------------------------------------------------
def test_malformed_graphs_are_refused_before_anything_else_runs():
    indptr, indices, weights = [a.copy() for a in lr.two_cliques()]

    def refused(g, text):
        status, got = library(g)
        assert status == 1 and text in got["error"], (status, got["error"])      # HMX_ERR_ARG
        assert got["sweeps"] == 0 and got["levels"] == 0 and np.all(got["labels"] == -7) and got["n_clusters"] == -7
    asym = lr.csr_of_edges(14, [(0, 1), (2, 3)])
    ai, aj, aw = asym[0].copy(), asym[1].copy(), asym[2].copy()
    aj[0] = 5                                              # row 0 lists cell 5, which does not list cell 0
    refused((ai, aj, aw), "no mirror")
    w = weights.copy()
    w[0] = 0.5                                             # (0, 1) is 0.5, (1, 0) stays 1
    refused((indptr, indices, w), "different weights")
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        w = weights.copy()
        e = int(indptr[5])                                 # cell 5's first entry is cell 0: both directions carry the bad weight
        assert indices[e] == 0
        w[e] = bad
        w[int(indptr[0]) + 4] = bad
        assert indices[int(indptr[0]) + 4] == 5
        refused((indptr, indices, w), "[0, 1]")
    j = indices.copy()
    j[0] = 20
    refused((indptr, j, weights), "outside [0, N)")
    j = indices.copy()
    j[0], j[1] = j[1], j[0]
    refused((indptr, j, weights), "ascending")
