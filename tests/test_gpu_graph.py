"""The neighbour graph on the MI355X against its fp64 / integer spec (tests/graph_ref.py): the graph stage on the spec's own neighbour lists
(pattern and rho equal, weights within the derived bar), the shapes that break the transposed lists (a hub, a cell nobody lists, unfilled
slots, duplicates, equal and zero distances), the whole call on lattice data where the kNN is exact, determinism and input forms, and the
connected components with scib's graph connectivity.

Sizes the kernels take another path at: one or two list entries per lane (m <= 64 | above), transposed rows of <= 128 entries (one wave, in
registers) | longer (one workgroup: 128-entry chunks, then merge passes -- one pass up to 256 entries, more beyond), a scan of <= 2048
counts per workgroup, pointer jumping in launches of 16 hops.

The bar of a weight: both searches stop with |psum - target| < 1e-5 and every membership of a row moves the same way with sigma, so a directed
weight differs by at most 2e-5; the union adds two of them; 2^-23 covers the fp32 rounding of a weight that is at most 1."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graph_ref as gr  # noqa: E402
import metrics_ref as mr  # noqa: E402
from bench_data import synth  # noqa: E402
from harmony_amd import RunHarmony, connected_components, graph_connectivity, graph_from_knn, neighbors  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.graph import _components  # noqa: E402
from test_gpu_metrics import lattice  # noqa: E402

pytestmark = pytest.mark.gpu
sp = pytest.importorskip("scipy.sparse")

BAR = 4e-5 + 2.0 ** -23


def check_stage(idx, dist, what):
    """the graph stage on the lists idx, dist against the spec: pattern and rho equal, weights within the bar; -> the library's graph"""
    idx, dist = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float32)
    conn, rho, sigma = graph_from_knn(idx, dist, prune_zeros=False, return_scales=True)
    indptr, indices, weights = gr.connectivities(idx, dist)
    rrho, rsigma = gr.smooth_knn(idx, dist)
    assert conn.data.dtype == np.float32 and conn.shape == (idx.shape[0],) * 2
    assert np.array_equal(conn.indptr, indptr) and np.array_equal(conn.indices, indices), what
    assert np.array_equal(rho, rrho), what
    err = float(np.abs(conn.data.astype(np.float64) - weights.astype(np.float64)).max()) if weights.size else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(rsigma > 0, np.abs(sigma - rsigma) / np.where(rsigma > 0, rsigma, 1.0), np.abs(sigma - rsigma))
    print("graph %s: N=%d m=%d entries=%d max in-degree=%d, max |w - spec| = %.3e (bar %.3e), max rel. sigma difference %.3e"
          % (what, idx.shape[0], idx.shape[1], indptr[-1], np.bincount(idx[idx >= 0], minlength=1).max(), err, BAR, rel.max()))
    assert err <= BAR, what
    return conn


# ---- (a) the graph stage on the spec's own neighbour lists -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spec_lists(N, m):
    Z, _, _ = synth(N, d=20, levels=(4,), seed=5)
    idx, d2 = mr.knn(Z, m)
    return idx.astype(np.int32), np.sqrt(d2).astype(np.float32)


@pytest.mark.parametrize("N,m", [(2000, 14), (1500, 29), (257, 128), (200, 1), (200, 2), (200, 63), (200, 64), (200, 65)])
def test_graph_stage_on_the_specs_neighbours(N, m):
    idx, dist = spec_lists(N, m)
    conn = check_stage(idx, dist, "synth")
    assert (conn != conn.T).nnz == 0                       # symmetric bit for bit


# ---- (b) shapes that break the transposed lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 5000])
def test_hub(N):
    """one centre and N - 1 points on a sphere around it, pairwise further apart than the radius: every point lists the centre first"""
    rng = np.random.default_rng(N)
    S = rng.normal(size=(N - 1, 128))
    X = np.vstack([np.zeros((1, 128)), 10.0 * S / np.linalg.norm(S, axis=1, keepdims=True)])
    idx, d2 = mr.knn(X, 3)
    assert np.all(idx[1:, 0] == 0)                         # the data is what the test says it is
    check_stage(idx, np.sqrt(d2), "hub")
    # ... and a hub of several long rows next to short ones: the first three cells are in every other cell's list (in-degree N - 1, N - 1, N - 1)
    idx3 = np.tile(np.array([0, 1, 2], dtype=np.int32), (N, 1))
    idx3[0], idx3[1], idx3[2] = [1, 2, 3], [0, 2, 3], [0, 1, 3]
    dist3 = np.sort(rng.uniform(0.5, 2.0, size=(N, 3)), axis=1)
    check_stage(idx3, dist3, "three hubs")


def test_outlier_unfilled_slots_and_rows_without_neighbours():
    idx, dist = spec_lists(200, 14)
    Z, _, _ = synth(200, d=20, levels=(4,), seed=5)
    far = np.vstack([Z, 1e3 + np.zeros((1, 20))])
    fidx, fd2 = mr.knn(far, 14)
    assert not (fidx == 200).any()                         # nobody lists the outlier
    conn = check_stage(fidx, np.sqrt(fd2), "outlier")
    assert np.array_equal(conn.indices[conn.indptr[200]:], np.sort(fidx[200]))
    idx = idx.copy()
    idx[5, 3:] = -1
    idx[9, :] = -1
    idx[199, 0] = -1
    dist = dist.copy()
    dist[9, :] = np.nan                                    # the distance of an unfilled slot is ignored
    check_stage(idx, dist, "unfilled slots")


def test_duplicates_and_degenerate_distances():
    X, _, ridx, rd2 = lattice(3, False)
    assert (rd2[:, :14] == 0).sum() > 1000                 # many zero distances
    conn = check_stage(ridx[:, :14], np.sqrt(rd2[:, :14]), "lattice d=3")
    zero = np.nonzero(rd2[:, 0] == 0)[0][0]
    assert conn[zero, ridx[zero, 0]] == 1.0                # w = 1 for a duplicate
    E = np.eye(10)                                         # a simplex: all distances equal, the floor decides
    sidx, sd2 = mr.knn(E, 4)
    assert np.all(sd2 == 2.0)
    g, rho, sigma = graph_from_knn(sidx.astype(np.int32), np.sqrt(sd2), prune_zeros=False, return_scales=True)
    check_stage(sidx, np.sqrt(sd2), "simplex")
    want = 1e-3 * (4 * float(np.float32(np.sqrt(2.0)))) / 5.0
    assert np.all(rho == float(np.float32(np.sqrt(2.0)))) and np.all(np.abs(sigma - want) <= 4 * np.spacing(want)) and np.all(g.data == 1.0)
    zidx, zd2 = mr.knn(np.zeros((50, 3)), 5)               # all distances zero: the mean_all path; what 64 halvings leave of sigma
    g, rho, sigma = graph_from_knn(zidx.astype(np.int32), np.sqrt(zd2), prune_zeros=False, return_scales=True)
    check_stage(zidx, np.sqrt(zd2), "zeros")
    assert not rho.any() and np.all(sigma == 2.0 ** -64) and np.all(g.data == 1.0)


# ---- (c) end to end on lattice data ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 50])
@pytest.mark.parametrize("n_neighbors", [15, 90])
def test_lattice_graph_end_to_end(d, n_neighbors):
    X, _, ridx, rd2 = lattice(d, False)
    m = n_neighbors - 1
    sidx, sdist = ridx[:, :m].astype(np.int32), np.sqrt(rd2[:, :m]).astype(np.float32)
    distances, conn = neighbors(X, n_neighbors=n_neighbors, prune_zeros=False)
    N = X.shape[0]
    assert np.array_equal(distances.indptr, np.arange(N + 1) * m) and np.array_equal(distances.indices.reshape(N, m), sidx)
    assert distances.data.dtype == np.float32 and np.array_equal(distances.data.reshape(N, m).view(np.uint32), sdist.view(np.uint32))
    indptr, indices, weights = gr.connectivities(sidx, sdist)
    assert np.array_equal(conn.indptr, indptr) and np.array_equal(conn.indices, indices)
    err = float(np.abs(conn.data.astype(np.float64) - weights.astype(np.float64)).max())
    print("lattice d=%d n_neighbors=%d: %d entries, max |w - spec| = %.3e (bar %.3e)" % (d, n_neighbors, indptr[-1], err, BAR))
    assert err <= BAR
    pruned = neighbors(X, n_neighbors=n_neighbors)[1]
    assert pruned.nnz == np.count_nonzero(conn.data) and not (pruned.data == 0).any()


def test_harmony_neighbors_reads_the_handles_embedding():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines_small.npz"))
    meta = {"dataset": fx["dataset_levels"][fx["dataset"]]}
    obj = RunHarmony(fx["pcs"], meta, "dataset", return_object=True, verbose=False, seed=1, max_iter=2, nclust=10)
    da, ca = obj.neighbors(n_neighbors=15)
    db, cb = neighbors(obj.getZcorr().T, n_neighbors=15)
    for a, b in ((da, db), (ca, cb)):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32))
    assert obj.timer("knn") > 0 and obj.timer("graph") > 0


# ---- (d) determinism and input forms -----------------------------------------------------------------------------------------------------------
def test_two_calls_and_both_element_types_give_the_same_bits():
    Z, _, _ = synth(3000, d=20, levels=(4,), seed=5)
    Z = Z.astype(np.float32)
    runs = [neighbors(Z, 30, prune_zeros=False), neighbors(Z, 30, prune_zeros=False), neighbors(Z.astype(np.float64), 30, prune_zeros=False)]
    for dist, conn in runs[1:]:
        for a, b in ((dist, runs[0][0]), (conn, runs[0][1])):
            assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32))


def test_capacity_one_short_returns_the_count():
    idx, dist = spec_lists(200, 14)
    nnz = int(gr.connectivities(idx, dist)[0][-1])
    ip, fp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    with _Handle() as h:
        def call(cap):
            indptr = np.zeros(201, dtype=np.int64)
            indices, weights = np.full(nnz, -7, dtype=np.int32), np.full(nnz, -7.0, dtype=np.float32)
            st = h.lib.hmx_graph_from_knn(h.h, idx.ctypes.data_as(ip), dist.ctypes.data_as(fp), 200, 14, indptr.ctypes.data_as(lp),
                                          indices.ctypes.data_as(ip), weights.ctypes.data_as(fp), cap, None, None)
            return st, indptr, indices, weights
        st, indptr, indices, weights = call(nnz - 1)
        assert st == 7 and indptr[200] == nnz and np.all(indices == -7) and np.all(weights == -7.0)      # HMX_ERR_LIMIT, nothing written beyond indptr
        st, indptr, indices, weights = call(nnz)
        assert st == 0 and indptr[200] == nnz and np.array_equal(indices, gr.connectivities(idx, dist)[1])


# ---- (e) connected components --------------------------------------------------------------------------------------------------------------------
def components_with_rounds(indptr, indices, codes=None):
    indptr, indices = np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32)
    N = indptr.size - 1
    comp, n, out = np.empty(N, dtype=np.int32), C.c_int64(0), (C.c_double * 1)()
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    with _Handle() as h:
        st = h.lib.hmx_graph_components(h.h, N, indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip),
                                        None if codes is None else codes.ctypes.data_as(ip), comp.ctypes.data_as(ip), C.byref(n))
        assert h.lib.hmx_get(h.h, b"graph:cc_rounds", out, 1) == 1
    return st, comp, int(n.value), int(out[0])


def path_graph(order):
    """the path that visits the cells in `order`"""
    r, c = np.concatenate([order[:-1], order[1:]]), np.concatenate([order[1:], order[:-1]])
    A = sp.csr_matrix((np.ones(r.size), (r, c)), shape=(order.size,) * 2)
    A.sort_indices()
    return A


@pytest.mark.parametrize("shuffled", [False, True])
def test_a_long_path_settles_within_the_round_bound(shuffled):
    order = np.random.default_rng(3).permutation(5000) if shuffled else np.arange(5000)
    A = path_graph(order)
    st, comp, n, rounds = components_with_rounds(A.indptr, A.indices)
    print("path of 5000 cells (%s): %d rounds" % ("shuffled" if shuffled else "in order", rounds))
    assert st == 0 and n == 1 and not comp.any() and 1 <= rounds <= 64
    assert np.array_equal(comp, gr.components(A.indptr, A.indices))


def test_isolated_cells_interleaved_labels_and_unlabelled_cells():
    n, comp = connected_components((np.zeros(301, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    assert n == 300 and np.array_equal(comp, np.arange(300))
    A = path_graph(np.arange(600))                          # one connected graph, labels alternate in runs of three: components per label
    labels = (np.arange(600) // 3) % 2
    n, comp = connected_components(A, labels)
    ref = gr.components(A.indptr, A.indices, labels)
    assert np.array_equal(comp, ref) and n == 200 and len(set(ref.tolist())) == 200
    n, comp = connected_components(A, np.array(["a", "b"])[labels])
    assert np.array_equal(comp, ref)
    codes = labels.astype(np.int32)
    codes[::7] = -1                                        # the library's own code of a cell without a label
    n, comp = _components(np.ascontiguousarray(A.indptr, dtype=np.int64), A.indices.astype(np.int32), 600, codes, None)
    ref = gr.components(A.indptr, A.indices, codes)
    assert np.array_equal(comp, ref) and np.all(comp[::7] == np.arange(600)[::7]) and n == len(set(ref.tolist()))
    with pytest.raises(Exception, match="symmetric"):
        connected_components(sp.csr_matrix(np.triu(A.toarray())))
    with pytest.raises(Exception, match="ascending"):
        connected_components((np.array([0, 2, 3, 4]), np.array([2, 1, 0, 0])))
    with pytest.raises(Exception, match=r"outside \[0, N\)"):
        connected_components((np.array([0, 1, 2, 2]), np.array([1, 3])))


def test_knn_graph_of_a_clustered_embedding_and_graph_connectivity():
    Z, meta, _ = synth(2000, d=20, levels=(4,), seed=5)
    _, conn = neighbors(Z, n_neighbors=15)
    labels = np.asarray(meta["cov0"])
    n, comp = connected_components(conn)
    assert np.array_equal(comp, gr.components(conn.indptr, conn.indices)) and n == len(set(comp.tolist()))
    levels, codes = np.unique(labels, return_inverse=True)
    n2, comp2 = connected_components(conn, labels)
    assert np.array_equal(comp2, gr.components(conn.indptr, conn.indices, codes)) and n2 >= max(n, levels.size)
    want = gr.graph_connectivity(conn.indptr, conn.indices, codes, levels.size)
    got = graph_connectivity(conn, {"cov0": labels}, "cov0")
    print("graph connectivity of cov0 on the 15-neighbour graph: %.6f (%d components, %d within labels)" % (got, n, n2))
    assert abs(got - want) <= 1e-15 and 0 < got <= 1
    assert abs(graph_connectivity(Z, {"cov0": labels}, "cov0", n_neighbors=15) - want) <= 1e-15
    A = sp.block_diag([np.ones((3, 3)) - np.eye(3), np.ones((5, 5)) - np.eye(5)]).tocsr()
    assert graph_connectivity(A, {"c": np.array([0] * 3 + [1] * 5)}, "c") == 1.0
    split = sp.block_diag([np.ones((4, 4)) - np.eye(4), np.ones((2, 2)) - np.eye(2), np.ones((2, 2)) - np.eye(2)]).tocsr()
    assert graph_connectivity(split, {"c": np.array(["x"] * 4 + ["y"] * 4)}, "c") == (1 + 1 / 2) / 2
