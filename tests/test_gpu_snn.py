"""Seurat's SNN graph on the MI355X against its integer spec (tests/snn_ref.py).  The result is exact, so indptr, indices and weights are
compared with np.array_equal: there is no tolerance.

Sizes the kernels take another path at: one, two or three entries of N+(i) per lane (k <= 64 | <= 128 | 129); candidate counts C_i up to
"snn:short_cap" (one wave sorts them in LDS: padded to a power of two from 64 up) | above (one workgroup walks the index range in windows
of "snn:window" cells: one window | several, with windows no candidate falls into); transposed rows of <= 128 entries | longer (the graph
stage's sort); a scan of <= 2048 counts per workgroup | more; a first capacity that suffices | the retry with the exact count."""
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
import metrics_ref as mr  # noqa: E402
import snn_ref as sr  # noqa: E402
from bench_data import synth  # noqa: E402
from harmony_amd import RunHarmony, connected_components, snn, snn_from_knn  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.snn import _snn_call  # noqa: E402
from test_gpu_metrics import lattice  # noqa: E402

ip, fp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
PRUNES = (0.0, 1.0 / 15.0, 0.5)


def get(h, key):
    out = (C.c_double * 1)()
    assert h.lib.hmx_get(h.h, key, out, 1) == 1, key
    return int(out[0])


@functools.lru_cache(maxsize=None)
def limits():
    with _Handle() as h:
        return get(h, b"snn:short_cap"), get(h, b"snn:window")


def stage(idx, prune):
    """the SNN stage of the library on the lists idx -> (graph, {s_min, long_rows})"""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    N, m = idx.shape
    with _Handle() as h:
        def run(indptr, indices, weights, cap):
            return h.lib.hmx_snn_from_knn(h.h, idx.ctypes.data_as(ip), N, m, prune, indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip),
                                          weights.ctypes.data_as(fp), cap)
        g = _snn_call(h.lib, h.h, h.check, run, N, m)
        info = {"s_min": get(h, b"snn:s_min"), "long_rows": get(h, b"snn:long_rows")}
    return g, info


def check_stage(idx, prune, what):
    """the stage against the spec: equal arrays, the threshold, the rows that took the long path; -> (graph, rows above short_cap)"""
    g, info = stage(idx, prune)
    indptr, indices, weights, _ = sr.snn(idx, prune)
    cand = sr.candidates(idx)
    n_long = int((cand > limits()[0]).sum())
    print("snn %s: N=%d m=%d prune=%.4f s_min=%d entries=%d, candidates per row <= %d, long rows %d (library %d)"
          % (what, idx.shape[0], idx.shape[1], prune, info["s_min"], indptr[-1], cand.max(), n_long, info["long_rows"]))
    assert g.shape == (idx.shape[0],) * 2
    assert g.data.dtype == np.float32 and info["s_min"] == sr.s_min(idx.shape[1] + 1, prune), what
    assert np.array_equal(g.indptr, indptr), what
    assert np.array_equal(g.indices, indices), what
    assert np.array_equal(g.data.view(np.uint32), weights.view(np.uint32)), what
    assert info["long_rows"] == n_long, what
    return g, n_long


# ---- (a) the stage on the spec's own neighbour lists -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spec_lists(N, m):
    Z, _, _ = synth(N, d=20, levels=(4,), seed=5)
    return mr.knn(Z, m)[0].astype(np.int32)


@pytest.mark.parametrize("prune", PRUNES)
@pytest.mark.parametrize("N,m", [(2000, 19), (1500, 29), (300, 128), (200, 1), (200, 2), (200, 63), (200, 64), (200, 65)])
def test_snn_stage_on_the_specs_neighbours(N, m, prune):
    g, _ = check_stage(spec_lists(N, m), prune, "synth")
    assert (g != g.T).nnz == 0                             # symmetric bit for bit


# ---- (b) both sides of short_cap ---------------------------------------------------------------------------------------------------------------
def test_rows_on_both_sides_of_short_cap_over_several_windows():
    """ring lists (cell i lists i + 1, i + 2, i + 3) in which D = short_cap + 100 cells, spread evenly, list cell 0 first: these D rows (and the
    few around cell 0) are long, every other row is short, and a long row's candidates span the whole index range, several windows wide"""
    short_cap, window = limits()
    D = short_cap + 100
    N = max(window + 1000, 4 * D)
    idx = ((np.arange(N)[:, None] + np.arange(1, 4)[None, :]) % N).astype(np.int32)
    listers = 5 + (N // D) * np.arange(D)
    assert listers.max() < N - 4 and N // D >= 4            # (no row lists cell 0 twice)
    idx[listers, 0] = 0
    cand = sr.candidates(idx)
    assert np.all(cand[listers] > short_cap) and (cand > short_cap).sum() <= D + 8 and N > window
    for prune in PRUNES:
        g, n_long = check_stage(idx, prune, "ring with one hub")
        assert n_long > 0 and (g != g.T).nnz == 0


def test_candidate_counts_of_exactly_short_cap_and_one_more():
    """m = 1: cells 1 .. D list cell 0, so each has C = (0 + 1) + (D + 1) = short_cap; cell D + 1 lists cell 1, which lifts C of cell 1 to
    short_cap + 1: the one long row.  prune = 0 keeps the D rows mutually adjacent: D^2 entries, more than the first capacity holds, so the
    call is made a second time with the exact count"""
    short_cap, _ = limits()
    D = short_cap - 2
    N = D + 10
    idx = np.full((N, 1), -1, dtype=np.int32)
    idx[1:D + 1, 0] = 0
    idx[D + 1, 0] = 1
    cand = sr.candidates(idx)
    assert cand[2] == short_cap and cand[1] == short_cap + 1 and cand[D + 1] == 1 + 2 and (cand > short_cap).sum() == 1
    g, n_long = check_stage(idx, 0.0, "C at short_cap")
    assert n_long == 1 and g.nnz > D * D > 6 * N * 2
    check_stage(idx, 0.5, "C at short_cap")


# ---- (c) hubs ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 5000])
def test_hubs(N):
    """cells 0, 1 and 2 are in every other cell's list, in front of six ring neighbours (k = 10): any two rows share the hubs (s >= 3), and at
    prune = 0.5 (s >= 7) only neighbouring rows survive; at N = 5000 every row is long"""
    idx = np.empty((N, 9), dtype=np.int32)
    idx[:, :3] = [0, 1, 2]
    idx[:, 3:] = 3 + (np.arange(N)[:, None] - 3 + np.arange(1, 7)[None, :]) % (N - 3)
    idx[0], idx[1], idx[2] = np.arange(1, 10), [0] + list(range(2, 10)), [0, 1] + list(range(3, 10))
    assert np.bincount(idx.ravel())[:3].tolist() == [N - 1] * 3 and not (idx == np.arange(N)[:, None]).any()
    g, n_long = check_stage(idx, 0.5, "three hubs")
    assert g.nnz < 16 * N and (n_long == N if N == 5000 else n_long == 0)


# ---- (d) other list shapes -------------------------------------------------------------------------------------------------------------------------
def test_a_cell_nobody_lists():
    Z, _, _ = synth(200, d=20, levels=(4,), seed=5)
    fidx = mr.knn(np.vstack([Z, 1e3 + np.zeros((1, 20))]), 19)[0]
    assert not (fidx == 200).any()                         # nobody lists the outlier
    for prune in PRUNES:
        g, _ = check_stage(fidx, prune, "outlier")
        assert g[200, 200] == 1.0                          # s = k on its diagonal


def test_unfilled_slots_and_a_row_without_neighbours():
    idx = spec_lists(200, 19).copy()
    idx[5, 3:] = -1
    idx[9, :] = -1
    idx[199, 0] = -1
    idx[idx == 9] = -1                                     # ... and nobody lists cell 9: its only candidate is itself, s = 1
    g0, _ = check_stage(idx, 0.0, "unfilled slots")
    g1, _ = check_stage(idx, 1.0 / 15.0, "unfilled slots")
    assert g0.indptr[10] - g0.indptr[9] == 1 and g0[9, 9] == np.float32(1.0 / 39.0)      # kept at prune = 0 ...
    assert g1.indptr[10] == g1.indptr[9]                                                 # ... and pruned at 1 / 15 for k = 20 (s_min = 3)
    # wide lists with few filled slots: entries of N+(i) in the second and third slot of a lane, on the short path
    rng = np.random.default_rng(3)
    wide = np.full((400, 128), -1, dtype=np.int32)
    offsets = np.concatenate([np.arange(-15, 0), np.arange(1, 16)])
    for i in range(400):
        slots = np.concatenate([rng.choice(127, size=29, replace=False), [127]])      # the cells 15 places to either side, in 30 of the 128 slots
        wide[i, slots] = rng.permutation((i + offsets) % 400)
    assert sr.candidates(wide).max() == 31 * 31 <= limits()[0] and (wide[:, 64:] >= 0).sum() > 4000
    for prune in (0.0, 1.0 / 15.0):
        _, n_long = check_stage(wide, prune, "wide sparse lists")
        assert n_long == 0


def test_lattice_duplicates():
    _, _, ridx, rd2 = cached_lattice(3)
    assert (rd2[:, :14] == 0).sum() > 1000                 # many duplicates of a cell: equal neighbour sets but for the cells themselves
    for prune in PRUNES:
        check_stage(ridx[:, :14], prune, "lattice d=3")


# ---- (e) capacity ----------------------------------------------------------------------------------------------------------------------------------
def test_capacity_one_short_returns_the_count():
    idx = spec_lists(200, 19)
    indptr_ref, indices_ref, weights_ref, _ = sr.snn(idx, 1.0 / 15.0)
    nnz = int(indptr_ref[-1])
    with _Handle() as h:
        def call(cap):
            indptr = np.zeros(201, dtype=np.int64)
            indices, weights = np.full(nnz, -7, dtype=np.int32), np.full(nnz, -7.0, dtype=np.float32)
            st = h.lib.hmx_snn_from_knn(h.h, idx.ctypes.data_as(ip), 200, 19, 1.0 / 15.0, indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip),
                                        weights.ctypes.data_as(fp), cap)
            return st, indptr, indices, weights
        st, indptr, indices, weights = call(nnz - 1)
        assert st == 7 and np.array_equal(indptr, indptr_ref) and np.all(indices == -7) and np.all(weights == -7.0)      # HMX_ERR_LIMIT, indptr alone is written
        st, indptr, indices, weights = call(nnz)
        assert st == 0 and np.array_equal(indptr, indptr_ref) and np.array_equal(indices, indices_ref) and np.array_equal(weights, weights_ref)


# ---- (f) the whole call ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cached_lattice(d):
    return lattice(d, False)


def same_bits(a, b):
    return np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32))


@pytest.mark.parametrize("d,k", [(3, 20), (50, 20), (50, 90)])
def test_lattice_snn_end_to_end(d, k):
    X, _, ridx, _ = cached_lattice(d)
    sidx = ridx[:, :k - 1].astype(np.int32)
    nn, g = snn(X, k=k)
    A = sr.nn_matrix(sidx)
    assert nn.data.dtype == np.float32 and np.all(nn.data == 1.0) and np.array_equal(nn.indptr, A.indptr) and np.array_equal(nn.indices, A.indices)
    indptr, indices, weights, _ = sr.snn(sidx, 1.0 / 15.0)
    print("lattice d=%d k=%d: %d entries" % (d, k, indptr[-1]))
    assert np.array_equal(g.indptr, indptr) and np.array_equal(g.indices, indices) and np.array_equal(g.data.view(np.uint32), weights.view(np.uint32))
    assert np.all(g.diagonal() == 1.0)                     # no unfilled slot: s_ii = k


def test_harmony_snn_reads_the_handles_embedding():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines_small.npz"))
    meta = {"dataset": fx["dataset_levels"][fx["dataset"]]}
    obj = RunHarmony(fx["pcs"], meta, "dataset", return_object=True, verbose=False, seed=1, max_iter=2, nclust=10)
    na, ga = obj.snn(k=20)
    nb, gb = snn(obj.getZcorr().T, k=20)
    assert same_bits(na, nb) and same_bits(ga, gb)
    assert obj.timer("knn") > 0 and obj.timer("snn") > 0


def test_two_calls_and_both_element_types_give_the_same_bits():
    Z, _, _ = synth(3000, d=20, levels=(4,), seed=5)
    Z = Z.astype(np.float32)
    runs = [snn(Z, 30), snn(Z, 30), snn(Z.astype(np.float64), 30)]
    for nn, g in runs[1:]:
        assert same_bits(nn, runs[0][0]) and same_bits(g, runs[0][1])


# ---- (g) composition with the components ---------------------------------------------------------------------------------------------------------
def test_components_of_the_snn_graph():
    g = snn_from_knn(spec_lists(2000, 19))
    n, comp = connected_components(g)                      # (the diagonal is stored: self loops are allowed there)
    assert np.array_equal(comp, gr.components(g.indptr, g.indices)) and n == len(set(comp.tolist()))
    torn = snn_from_knn(spec_lists(2000, 19), prune=0.5)
    n2, comp2 = connected_components(torn)
    assert np.array_equal(comp2, gr.components(torn.indptr, torn.indices)) and n2 >= n
