"""Leiden clustering on the MI355X against its spec (tests/leiden_ref.py).  The spec and the kernels compute the same integers, the same
three-operation fp64 score and the same two-product tests in the same schedule, so the labels, the five arrays of the levels, `converged` and
the modularities (doubles) are compared with np.array_equal: there is no tolerance.

Sizes the kernels take another path at: rows of up to 64, 128, .. 1024 edges (the LDS sort's padding) | above "louvain:short_cap" (one
workgroup, windows of ids), in the moves and in the refinement; one window | several; rows with a diagonal or a stored zero (compacted away) |
without; a scan of <= 2048 counts per workgroup | more; level 0 (the identity) | later levels (the parents' partition, inner weights)."""
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
import leiden_ref as ld  # noqa: E402
import louvain_ref as lr  # noqa: E402
import metrics_ref as mr  # noqa: E402
import snn_ref as sr  # noqa: E402
from bench_data import synth  # noqa: E402
from harmony_amd import RunHarmony, connected_components, leiden, louvain  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402

ip, fp, lp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_double)
KEYS = ("levels", "sweeps", "refine_sweeps", "clusters", "converged", "long_rows")
LEVEL_ARRAYS = ("level_clusters", "level_nodes", "level_sweeps", "level_refine_sweeps")


def get(h, key):
    out = (C.c_double * 1)()
    assert h.lib.hmx_get(h.h, key, out, 1) == 1, key
    return out[0]


def library(g, resolution=1.0, max_levels=20, max_sweeps=32, short_cap=None):
    """hmx_leiden on the graph g = (indptr, indices, weights) -> (status, the outputs and counters as a dict)"""
    indptr = np.ascontiguousarray(g[0], dtype=np.int64)
    indices, weights = np.ascontiguousarray(g[1], dtype=np.int32), np.ascontiguousarray(g[2], dtype=np.float32)
    N = indptr.size - 1
    labels = np.full(N, -7, dtype=np.int32)
    n, q, conv = C.c_int32(-7), C.c_double(-7.0), C.c_int32(-7)
    arrays = {k: np.full(max_levels, -7, dtype=np.int32) for k in LEVEL_ARRAYS}
    lq = np.full(max_levels, -7.0)
    with _Handle() as h:
        if short_cap is not None:
            assert h.lib.hmx_set_int(h.h, b"louvain_short_cap", short_cap) == 0
        status = h.lib.hmx_leiden(h.h, indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip), weights.ctypes.data_as(fp), N, resolution,
                                  max_levels, max_sweeps, labels.ctypes.data_as(ip), C.byref(n), C.byref(q), C.byref(conv),
                                  *[arrays[k].ctypes.data_as(ip) for k in LEVEL_ARRAYS], lq.ctypes.data_as(dp))
        out = {k: int(get(h, b"leiden:" + k.encode())) for k in KEYS}
        out.update(arrays)
        out.update(labels=labels, n_clusters=n.value, modularity=q.value, conv=conv.value, level_modularity=lq,
                   short_cap=int(get(h, b"louvain:short_cap")), timer=get(h, b"timer:leiden"), error=h.lib.hmx_last_error(h.h).decode())
    return status, out


@functools.lru_cache(maxsize=None)
def spec(key, resolution, max_levels, max_sweeps):
    return ld.leiden(*GRAPHS[key], resolution=resolution, max_levels=max_levels, max_sweeps=max_sweeps)


GRAPHS = {}


def check(g, what, resolution=1.0, max_levels=20, max_sweeps=32, short_cap=None):
    """the library against the spec on g: equal bits everywhere; -> (the library's outputs, the spec's)"""
    GRAPHS.setdefault(what, g)                             # (the spec of one graph and one set of arguments is computed once)
    assert GRAPHS[what] is g, what
    want = spec(what, resolution, max_levels, max_sweeps)
    status, got = library(g, resolution, max_levels, max_sweeps, short_cap)
    L = len(want.level_clusters)
    print("leiden %s: N=%d entries=%d resolution %s cap %s -> clusters %d Q %.6f converged %s; levels %s nodes %s sweeps %s refine %s; long rows %d; %.1f ms"
          % (what, g[0].size - 1, g[1].size, resolution, short_cap, want.n_clusters, want.modularity, want.converged, want.level_clusters,
             want.level_nodes, want.level_sweeps, want.level_refine_sweeps, got["long_rows"], got["timer"]))
    assert status == 0, got["error"]
    assert got["levels"] == L and got["sweeps"] == sum(want.level_sweeps) and got["refine_sweeps"] == sum(want.level_refine_sweeps), what
    for k in LEVEL_ARRAYS:
        assert np.array_equal(got[k][:L], np.array(getattr(want, k), dtype=np.int32)), (what, k)
        assert np.all(got[k][L:] == -7), (what, k)         # nothing written past the recorded levels
    assert np.array_equal(got["level_modularity"][:L].view(np.uint64), np.array(want.level_modularity, dtype=np.float64).view(np.uint64)), what
    assert np.all(got["level_modularity"][L:] == -7.0)
    assert np.array_equal(got["labels"], want.labels), what
    assert got["n_clusters"] == want.n_clusters == got["clusters"], what
    assert got["conv"] == int(want.converged) == got["converged"], what
    assert np.float64(got["modularity"]).view(np.uint64) == np.float64(want.modularity).view(np.uint64), what
    return got, want


# ---- (a) SNN graphs of the spec's own neighbour lists, the neighbour graph's connectivities ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def snn_graph(N, m):
    Z, _, _ = synth(N, d=20, levels=(4,), seed=5)
    return sr.snn(mr.knn(Z, m)[0].astype(np.int32), 1.0 / 15.0)[:3]


@pytest.mark.parametrize("resolution", [0.5, 0.8, 1.0, 2.0])
@pytest.mark.parametrize("N,m", [(2000, 19), (600, 29)])
def test_snn_graphs(N, m, resolution):
    got, want = check(snn_graph(N, m), "snn %d" % N, resolution=resolution)
    assert want.converged and got["long_rows"] == 0


def test_more_cells_than_one_workgroup_scans():
    check(snn_graph(5000, 9), "snn 5000")


@functools.lru_cache(maxsize=None)
def connectivities_1500():
    Z, _, _ = synth(1500, d=20, levels=(4,), seed=5)
    idx, dist = mr.knn(Z, 14)[:2]
    return gr.connectivities(idx.astype(np.int32), np.sqrt(np.maximum(np.asarray(dist, dtype=np.float64), 0.0)).astype(np.float32))


def test_neighbors_style_float_weights():
    g = connectivities_1500()
    assert len(np.unique(g[2])) > 1000 and g[2].max() <= 1.0
    check(g, "connectivities")
    check(g, "connectivities", resolution=0.8)


# ---- (b) graphs on which the Louvain spec tears a cluster apart: connected on the device -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def er_graph(N, deg, seed):
    return ld.er(N, deg, seed, True)


@pytest.mark.parametrize("N,deg,seed,resolution", [(60, 2.2, 1, 0.5), (200, 2.2, 1, 1.0), (600, 3, 3, 1.0)])
def test_random_graphs_give_connected_clusters(N, deg, seed, resolution):
    g = er_graph(N, deg, seed)
    got, want = check(g, "er %d %s %d" % (N, deg, seed), resolution=resolution)
    assert got["conv"] == 1 and ld.components_within(g, got["labels"]) == 0
    rows = np.repeat(np.arange(N), np.diff(g[0]))
    edge = g[2] > 0                                        # the pattern of the edges of positive weight, for the library's own components
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[edge], minlength=N))]).astype(np.int64)
    n_comp, _ = connected_components((ptr, g[1][edge].copy()), got["labels"])
    assert n_comp == got["n_clusters"]                     # one component per cluster
    if N < 600:
        assert ld.components_within(g, lr.louvain(*g, resolution=resolution).labels) > 0      # (the Louvain spec's clusters are not)


# ---- (c) the hand-checkable graphs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring", "path", "star", "complete", "cliques"])
def test_small_graphs(name):
    g = SMALL[name]
    for resolution in (1.0, 0.8):
        got, want = check(g, name, resolution=resolution)
        assert got["conv"] == 1
    if name == "cliques":
        assert got["labels"].tolist() == [0] * 6 + [1] * 6 + [2, 3] and want.n_clusters == 4
    if name == "path":
        assert got["labels"].tolist() == [0] * 5 + [1] * 4 + [2] * 3


SMALL = {"ring": lr.ring(300), "path": lr.path(12), "star": lr.star(40), "complete": lr.complete(20), "cliques": lr.two_cliques()}


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


def test_stored_diagonal_and_explicit_zeros():
    indptr, indices, weights = [a.copy() for a in snn_graph(600, 29)]
    rows = np.repeat(np.arange(600), np.diff(indptr))
    assert (rows == indices).sum() == 600                  # the SNN graph stores its diagonal
    zero = ((rows + indices) % 5 == 0) & (rows != indices)      # a symmetric choice of edges
    weights[zero] = 0.0
    assert zero.sum() > 1000
    got, _ = check((indptr, indices, weights), "diagonal and zeros")
    keep = ~zero & (rows != indices)                       # the same graph without them: the same result
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=600))]).astype(np.int64)
    bare, _ = check((ptr, indices[keep].copy(), weights[keep].copy()), "neither diagonal nor zeros")
    assert np.array_equal(got["labels"], bare["labels"]) and got["modularity"] == bare["modularity"]
    plain = lr.csr_of_edges(14, [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(6 + i, 6 + j) for i in range(6) for j in range(i + 1, 6)]
                            + [(5, 6), (12, 13, 0.0), (0, 12, 0.0)], diagonal=True)
    got, _ = check(plain, "cliques with a diagonal and two edges of weight 0")
    assert got["labels"].tolist() == [0] * 6 + [1] * 6 + [2, 3]


def test_one_and_two_cells_and_no_edges():
    one = (np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    got, _ = check(one, "one cell")
    assert got["labels"].tolist() == [0] and got["n_clusters"] == 1 and got["modularity"] == 0.0 and got["levels"] == 0 and got["conv"] == 1
    one_diag = (np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.float32))
    check(one_diag, "one cell with its diagonal")
    got, _ = check(lr.path(2), "two cells")
    assert got["labels"].tolist() == [0, 0] and got["conv"] == 1
    empty = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    got, _ = check(empty, "no edges")
    assert got["labels"].tolist() == [0, 1, 2, 3, 4] and got["n_clusters"] == 5 and got["modularity"] == 0.0 and got["sweeps"] == 0
    zeros = lr.csr_of_edges(5, [(0, 1, 0.0), (2, 3, 0.0)])
    got, _ = check(zeros, "edges of weight 0 only")       # M = 0
    assert got["n_clusters"] == 5 and got["levels"] == 0 and got["conv"] == 1


# ---- (d) the caps ----------------------------------------------------------------------------------------------------------------------------------------
def test_caps_end_the_call():
    g = snn_graph(600, 29)
    got, want = check(g, "snn 600", max_sweeps=1)
    assert all(s == 1 for s in want.level_sweeps) and got["levels"] > 1 and got["sweeps"] == got["levels"]
    got, want = check(g, "snn 600", max_levels=1)
    assert got["levels"] == 1 and got["conv"] == 0 and got["sweeps"] == want.level_sweeps[0] > 1 and got["refine_sweeps"] == 0
    got, want = check(g, "snn 600", max_levels=2)
    assert got["levels"] == 2 and got["conv"] == 0 and got["refine_sweeps"] == want.level_refine_sweeps[0] > 0
    assert got["level_nodes"][1] == want.level_nodes[1] == want.level_nodes[0]      # the level that ended the call keeps its own nodes


# ---- (e) both sides of short_cap, and the long path alone ------------------------------------------------------------------------------------------
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
    big = snn_graph(5000, 9)                               # more cells than one window of ids holds, every row long
    got, _ = check(big, "snn 5000", short_cap=0)
    edges = ld.edges(*big)[0]
    assert got["short_cap"] == 0 and got["long_rows"] == np.unique(edges).size
    g = snn_graph(600, 29)
    lens = np.bincount(ld.edges(*g)[0], minlength=600)
    got, _ = check(g, "snn 600", short_cap=int(np.median(lens)), resolution=0.8)
    assert 0 < got["long_rows"] == int((lens > np.median(lens)).sum()) < 600


# ---- (f) the whole call --------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    g = snn_graph(2000, 19)
    a, b = library(g, resolution=0.8)[1], library(g, resolution=0.8)[1]
    for key in ("labels",) + LEVEL_ARRAYS:
        assert np.array_equal(a[key], b[key])
    assert np.array_equal(a["level_modularity"].view(np.uint64), b["level_modularity"].view(np.uint64)) and a["modularity"] == b["modularity"]


def test_python_leiden_numbers_clusters_by_size():
    g = snn_graph(2000, 19)
    GRAPHS.setdefault("snn 2000", g)
    want = spec("snn 2000", 0.8, 20, 32)
    res = leiden(sp.csr_matrix((g[2].copy(), g[1].copy(), g[0].copy()), shape=(2000, 2000)), resolution=0.8)
    assert res.labels.dtype == np.int32 and np.array_equal(res.labels, lr.seurat_order(want.labels))
    sizes = np.bincount(res.labels)
    assert np.all(np.diff(sizes) <= 0) and res.n_clusters == want.n_clusters == sizes.size
    assert res.modularity == want.modularity and res.converged is True
    assert res.levels == list(zip(want.level_clusters, want.level_nodes, want.level_sweeps, want.level_refine_sweeps, want.level_modularity))
    tri = leiden((g[0], g[1], g[2]), resolution=0.8)       # the triple form
    assert np.array_equal(tri.labels, res.labels)


def test_harmony_leiden_and_clusters():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines_small.npz"))
    meta = {"dataset": fx["dataset_levels"][fx["dataset"]]}
    obj = RunHarmony(fx["pcs"], meta, "dataset", return_object=True, verbose=False, seed=1, max_iter=2, nclust=10)
    a = obj.clusters(algorithm="leiden")
    g = obj.snn()[1]
    b = leiden(g, 0.8)
    assert np.array_equal(a.labels, b.labels) and a[1:] == b[1:] and a.n_clusters >= 2 and a.converged and obj.timer("leiden") > 0
    want = ld.leiden(g.indptr.copy(), g.indices.copy(), g.data.copy(), resolution=0.8)
    assert np.array_equal(a.labels, lr.seurat_order(want.labels)) and a.modularity == want.modularity
    c = obj.leiden()
    d = leiden(obj.neighbors()[1])
    assert np.array_equal(c.labels, d.labels) and c[1:] == d[1:] and c.converged
    e, f = obj.clusters(), louvain(g, 0.8)                 # the default is Louvain, as before
    assert len(e) == 4 and np.array_equal(e.labels, f.labels) and e[1:] == f[1:]
    with pytest.raises(ValueError, match="algorithm"):
        obj.clusters(algorithm="infomap")


# ---- (g) malformed graphs ------------------------------------------------------------------------------------------------------------------------------
def test_malformed_graphs_are_refused_before_anything_else_runs():
    indptr, indices, weights = [a.copy() for a in lr.two_cliques()]

    def refused(g, text):
        status, got = library(g)
        assert status == 1 and text in got["error"], (status, got["error"])      # HMX_ERR_ARG
        assert got["sweeps"] == 0 and got["levels"] == 0 and np.all(got["labels"] == -7) and got["n_clusters"] == -7 and got["conv"] == -7
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
