"""Leiden clustering held to its spec (tests/leiden_ref.py) without a GPU: the header, the library and the binding agree; every argument
error that the host can see is raised before a device is needed; the refinement's hash key; the spec on graphs small enough to check by hand;
the property Leiden exists for -- every cluster of a converged result is connected through edges of positive weight -- on random graphs where
the Louvain spec's result is not; and its quality against a plain sequential Louvain (tests/test_gpu_leiden.py runs the library).

The quality bar is Louvain's: Q >= 0.95 Q_seq on every input of test_louvain_cpu.quality_inputs, ARI >= 0.99 on the planted graphs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

sp = pytest.importorskip("scipy.sparse")

import helpers  # noqa: E402
import leiden_ref as ld  # noqa: E402
import louvain_ref as lr  # noqa: E402
from test_louvain_cpu import planted_graph, quality_inputs  # noqa: E402
from harmony_amd import Harmony, _lib, leiden  # noqa: E402

HEADER = "harmony_mi355x_leiden.h"
EARLIER = helpers.PUBLIC_HEADERS + (("harmony_mi355x_louvain.h", "LOUVAIN_SIGNATURES"), ("harmony_mi355x_umap.h", "UMAP_SIGNATURES"))


def test_leiden_header_matches_the_library_and_the_binding():
    found = helpers.header_functions(HEADER)
    mine = [n for n, _ in found]
    assert mine == ["hmx_leiden"] and set(mine) == set(_lib.LEIDEN_SIGNATURES)
    for other, table in EARLIER:                           # every other header: none names the function, no other table binds it
        assert other != HEADER and not (set(mine) & helpers.header_names(other)), other
        assert not (set(mine) & set(getattr(_lib, table))), table
    tables = [t for t in dir(_lib) if t.endswith("SIGNATURES") and t != "LEIDEN_SIGNATURES"]
    assert len(tables) >= 12 and not any(set(mine) & set(getattr(_lib, t)) for t in tables)
    for name, types in found:
        helpers.assert_binding_matches(_lib.load(), name, types, _lib.LEIDEN_SIGNATURES[name][1])
    assert set(_lib.LOUVAIN_SIGNATURES) == {"hmx_louvain"} and helpers.header_functions("harmony_mi355x_louvain.h")[0][0] == "hmx_louvain"


# ---- the hash ----------------------------------------------------------------------------------------------------------------------------------------
def test_refinement_key_known_answers():
    """key = fmix32((64 t + level + 1) ^ 0xFFFFFFFF): fmix32(0xFFFFFFFF) is Louvain's known answer; the others step by step with Python's integers"""
    def by_hand(x):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) % 2 ** 32
        x ^= x >> 13
        x = (x * 0xC2B2AE35) % 2 ** 32
        return x ^ (x >> 16)
    assert lr.fmix32(0xFFFFFFFF) == 0x81F16F39
    assert ld.refine_key(0, 0) == by_hand(0xFFFFFFFE) and ld.refine_key(0, 0) != lr.fmix32(1)
    for t, level in ((0, 0), (1, 0), (3, 2), (31, 19), (4095, 63)):
        x = 64 * t + level + 1
        assert ld.refine_key(t, level) == by_hand(2 ** 32 - 1 - x)
        assert ld.refine_key(t, level) != lr.fmix32(x)    # never the moves' key of the same sweep
    b = ld.refine_buckets(4096, 3, 1)
    assert b.min() == 0 and b.max() == 7 and np.bincount(b).min() > 4096 / 8 * 0.8
    assert b.tolist()[:64] == [lr.fmix32(i ^ ld.refine_key(3, 1)) & 7 for i in range(64)]
    assert not np.array_equal(b, lr.buckets(4096, 3, 1))


# ---- the spec on graphs that can be checked by hand ------------------------------------------------------------------------------------------------
def test_two_cliques_and_isolated_cells():
    r = ld.leiden(*lr.two_cliques())
    assert r.labels.tolist() == [0] * 6 + [1] * 6 + [2, 3] and r.n_clusters == 4 and r.labels.dtype == np.int32 and r.converged
    assert abs(r.modularity - 2 * (30 / 62 - 0.25)) < 1e-15
    assert r.level_clusters == [4, 4] and r.level_nodes == [4, 4] and r.level_refine_sweeps[-1] == 0
    assert ld.components_within(lr.two_cliques(), r.labels) == 0


def test_star_and_complete_graph_are_one_cluster():
    for g, n in ((lr.star(40), 40), (lr.complete(20), 20)):
        for resolution, q in ((1.0, 0.0), (0.8, 0.2)):
            r = ld.leiden(*g, resolution=resolution)
            assert r.labels.tolist() == [0] * n and r.n_clusters == 1 and abs(r.modularity - q) < 1e-15 and r.converged


def test_path_of_twelve():
    r = ld.leiden(*lr.path(12))
    assert r.labels.tolist() == [0] * 5 + [1] * 4 + [2] * 3 and r.converged
    assert abs(r.modularity - (18 / 22 - (81 + 64 + 25) / 22 ** 2)) < 1e-15      # Louvain's test has the count
    assert r.level_clusters == [5, 3, 3] and r.level_nodes[-1] == 3


def test_edgeless_and_tiny_graphs():
    empty = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    r = ld.leiden(*empty)
    assert r.labels.tolist() == [0, 1, 2, 3, 4] and r.n_clusters == 5 and r.modularity == 0.0 and r.level_clusters == [] and r.converged
    r = ld.leiden(*lr.csr_of_edges(4, [(0, 1, 0.0), (2, 3, 0.0)]))      # M = 0
    assert r.n_clusters == 4 and r.modularity == 0.0 and r.level_sweeps == [] and r.converged
    one = (np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    r = ld.leiden(*one)
    assert r.labels.tolist() == [0] and r.n_clusters == 1 and r.converged
    r = ld.leiden(*lr.path(2))
    assert r.labels.tolist() == [0, 0] and r.modularity == 0.0 and r.converged and r.level_clusters == [1, 1]


def test_a_stored_diagonal_and_explicit_zeros_change_nothing():
    cliques = [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(6 + i, 6 + j) for i in range(6) for j in range(i + 1, 6)] + [(5, 6)]
    a = ld.leiden(*lr.two_cliques())
    b = ld.leiden(*lr.csr_of_edges(14, cliques + [(12, 13, 0.0), (0, 12, 0.0), (3, 9, 0.0)], diagonal=True))
    assert np.array_equal(a.labels, b.labels) and a[1:] == b[1:]
    g = ld.er(200, 3, 0, True)                             # weights k / 16, k = 0 among them
    rows = np.repeat(np.arange(200), np.diff(g[0]))
    assert (g[2] == 0).sum() > 10
    keep = g[2] > 0
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=200))]).astype(np.int64)
    a, b = ld.leiden(*g), ld.leiden(ptr, g[1][keep], g[2][keep])
    assert np.array_equal(a.labels, b.labels) and a[1:] == b[1:]


def test_caps_and_counters_of_the_spec():
    g = planted_graph(600, 4)[0]
    r = ld.leiden(*g, max_sweeps=1)
    assert all(s == 1 for s in r.level_sweeps) and len(r.level_sweeps) > 1 and all(s <= 1 for s in r.level_refine_sweeps)
    r = ld.leiden(*g, max_levels=1)
    assert len(r.level_clusters) == 1 and not r.converged and r.level_refine_sweeps == [0] and r.level_nodes == [600]
    full = ld.leiden(*g)
    assert full.converged and full.level_nodes[-1] == full.level_clusters[-1] == full.n_clusters
    assert all(a >= b for a, b in zip(full.level_nodes, full.level_clusters))


def test_the_phases_on_their_own():
    """local_move from a given partition opens an empty community; refine joins only along inner edges of positive weight"""
    g = lr.two_cliques()
    src, dst, q, k = ld.edges(*g)
    M = int(k.sum())
    gg = np.float64(1.0) / np.float64(M)
    comm, tot, sweeps, moved = ld.local_move(src, dst, q, k, np.arange(14), gg, 0, 32)
    assert len(set(comm[:6])) == 1 and len(set(comm[6:12])) == 1 and comm[12] == 12 and comm[13] == 13 and moved > 0
    assert np.array_equal(tot, np.bincount(comm, weights=k, minlength=14).astype(np.int64))
    ref, rs = ld.refine(src, dst, q, k, comm, tot, gg, 0, 32)
    assert rs >= 1 and np.all(comm[ref] == comm) and ld.components_within(g, ref) == 0
    # everything in one community whose id, 13, is an isolated cell.  At resolution 1 staying beats the empty id (score 0.0) for every cell;
    # at resolution 4 it does not (5 - 4 * 5 * 57 / 62 < 0), and "alone" is the only other candidate: cells open their own ids
    comm2, tot2, _, moved2 = ld.local_move(src, dst, q, k, np.full(14, 13), gg, 0, 32)
    assert moved2 == 0 and np.all(comm2 == 13)
    comm2, tot2, _, moved2 = ld.local_move(src, dst, q, k, np.full(14, 13), np.float64(4.0) / np.float64(M), 0, 32)
    assert moved2 > 0 and not (set(comm2[:12].tolist()) & {12, 13}) and comm2[12] == comm2[13] == 13 and tot2[13] == 0
    assert np.array_equal(tot2, np.bincount(comm2, weights=k, minlength=14).astype(np.int64))


# ---- the property: converged results are connected, where Louvain's are not ------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("deg", [2.2, 3, 5])
@pytest.mark.parametrize("N", [60, 200, 600])
def test_every_converged_cluster_is_connected(N, deg, weighted):
    for seed in range(6):
        g = ld.er(N, deg, seed, weighted)
        for resolution in (0.5, 1.0, 2.0):
            r = ld.leiden(*g, resolution=resolution)
            assert r.converged and len(r.level_clusters) <= 20, (seed, resolution)
            assert ld.components_within(g, r.labels) == 0, (seed, resolution)
            assert abs(lr.partition_modularity(*g, r.labels, resolution) - r.modularity) < 1e-12


def test_the_inputs_tell_the_two_algorithms_apart():
    for (N, deg, seed), resolution in (((60, 2.2, 1), 0.5), ((200, 2.2, 1), 1.0)):
        g = ld.er(N, deg, seed, True)
        assert ld.components_within(g, lr.louvain(*g, resolution=resolution).labels) > 0
        assert ld.components_within(g, ld.leiden(*g, resolution=resolution).labels) == 0
    assert ld.components_within(lr.path(4), [0, 1, 1, 0]) == 1 and ld.components_within(lr.path(4), [0, 0, 1, 1]) == 0
    assert ld.components_within(lr.csr_of_edges(3, [(0, 1, 0.0), (1, 2)]), [0, 0, 0]) == 1      # an edge of weight 0 connects nothing


# ---- quality -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution", [1.0, 0.8])
@pytest.mark.parametrize("name", ["planted 600", "planted 1500", "planted 3000", "structureless", "ring 300", "path 12", "star 40",
                                  "complete 20", "two cliques"])
def test_quality_against_a_sequential_louvain(name, resolution):
    g, planted = quality_inputs()[name]
    r = ld.leiden(*g, resolution=resolution)
    _, q_seq = lr.sequential(*g, resolution=resolution)
    q_lv = lr.louvain(*g, resolution=resolution).modularity
    print("%s, resolution %.1f: Q %.5f, sequential %.5f (ratio %.4f), Louvain spec %.5f (ratio %.4f); %d clusters, levels %s, nodes %s, sweeps %s, refine %s"
          % (name, resolution, r.modularity, q_seq, r.modularity / q_seq if q_seq else 1.0, q_lv, r.modularity / q_lv if q_lv else 1.0,
             r.n_clusters, r.level_clusters, r.level_nodes, r.level_sweeps, r.level_refine_sweeps))
    assert r.converged and ld.components_within(g, r.labels) == 0
    assert r.modularity >= 0.95 * q_seq
    assert abs(lr.partition_modularity(*g, r.labels, resolution) - r.modularity) < 1e-12
    if planted is not None:
        assert lr.adjusted_rand(r.labels, planted) >= 0.99


# ---- every argument error is raised before a device is needed --------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device():
    indptr, indices, weights = lr.two_cliques()
    g = sp.csr_matrix((weights, indices, indptr), shape=(14, 14))
    for bad in (0.0, -1.0, 100.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="resolution"):
            leiden(g, resolution=bad)
    for bad in (0, 65, 2.5, float("nan")):
        with pytest.raises(ValueError, match="max_levels"):
            leiden(g, max_levels=bad)
    for bad in (0, 4097, 1.5):
        with pytest.raises(ValueError, match="max_sweeps"):
            leiden(g, max_sweeps=bad)
    with pytest.raises(ValueError, match="square"):
        leiden(sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(ValueError, match="scipy.sparse matrix or"):
        leiden(np.ones(5))
    for w, msg in ((weights * 1.5, r"\[0, 1\]"), (np.where(np.arange(weights.size) == 3, np.nan, weights), r"\[0, 1\]"),
                   (-weights, r"\[0, 1\]")):
        with pytest.raises(ValueError, match=msg):
            leiden((indptr, indices, w.astype(np.float32)))
    w = weights.copy()
    w[0] = 0.5
    with pytest.raises(ValueError, match="different weights"):
        leiden((indptr, indices, w))
    one_way = sp.csr_matrix(([1.0], ([0], [1])), shape=(3, 3))
    with pytest.raises(ValueError, match="no mirror"):
        leiden(one_way)
    j = indices.copy()
    j[0] = 14
    with pytest.raises(ValueError, match="outside"):
        leiden((indptr, j, weights))
    assert callable(Harmony.leiden) and callable(Harmony.clusters)
    import inspect
    assert inspect.signature(Harmony.clusters).parameters["algorithm"].default == "louvain"
    assert [p.default for p in list(inspect.signature(Harmony.leiden).parameters.values())[1:]] == [15, 1.0]
    assert [p.default for p in list(inspect.signature(leiden).parameters.values())[1:]] == [1.0, 20, 32, None]


def test_library_argument_errors_come_before_the_device():
    lib = _lib.load()
    ip, fp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    h = C.c_void_p(lib.hmx_create())
    ARG, LIMIT = 1, 7
    indptr, indices, weights = lr.two_cliques()
    try:
        def call(N=14, resolution=1.0, max_levels=20, max_sweeps=32, ptr=indptr, null=None):
            ptr = np.ascontiguousarray(ptr, dtype=np.int64)
            labels, n, q, conv = np.zeros(64, dtype=np.int32), C.c_int32(0), C.c_double(0.0), C.c_int32(0)
            arg = {"indptr": ptr.ctypes.data_as(lp), "indices": indices.ctypes.data_as(ip), "weights": weights.ctypes.data_as(fp),
                   "labels": labels.ctypes.data_as(ip), "n_clusters": C.byref(n), "modularity": C.byref(q), "converged": C.byref(conv)}
            if null:
                arg[null] = None
            return lib.hmx_leiden(h, arg["indptr"], arg["indices"], arg["weights"], N, resolution, max_levels, max_sweeps, arg["labels"],
                                  arg["n_clusters"], arg["modularity"], arg["converged"], None, None, None, None, None)
        for null in ("indptr", "indices", "weights", "labels", "n_clusters", "modularity", "converged"):
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
        assert lib.hmx_leiden(None, None, None, None, 1, 1.0, 1, 1, None, None, None, None, None, None, None, None, None) == ARG
        out1 = (C.c_double * 1)()
        for key in (b"leiden:levels", b"leiden:sweeps", b"leiden:refine_sweeps", b"leiden:clusters", b"leiden:converged", b"leiden:long_rows",
                    b"timer:leiden"):
            assert lib.hmx_get(h, key, out1, 1) == 1 and out1[0] == 0, key
        assert lib.hmx_get(h, b"leiden:best_level", out1, 1) != 1      # Leiden returns the last level: there is no such counter
        assert lib.hmx_set_int(h, b"louvain_short_cap", 16) == 0 and lib.hmx_get(h, b"louvain:short_cap", out1, 1) == 1 and out1[0] == 16
    finally:
        lib.hmx_destroy(h)
