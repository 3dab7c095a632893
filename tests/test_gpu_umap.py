"""The UMAP layout on the MI355X against its spec (tests/umap_ref.py).  Which entries fire and which cells they sample are integers and one
fp64 product: "umap:fired" equals the spec's count.  The terms are fp32 on the device and fp64 in the spec, so one epoch from the same fp32
positions is held elementwise to the bound B the spec derives from the device's expression (umap_ref.bound_constants) -- no tuned tolerance.
Whole layouts are chaotic over hundreds of epochs and are held by quality: purity and trustworthiness against the fp64 spec's own runs.

Sizes the kernels take another path at: rows of up to 64 entries (one step of a wave) | more; rows up to "umap:short_cap" (one wave) | above
(one workgroup, four partials); dim 2 | 3; no negative samples | 31; b < 1, where the clip engages at small distances.

Largest |Y_gpu - Y_spec| / B measured per test: printed by `within_bound` (0.49 at most when this was written: where little moves, the rounding of
y itself, half the bound's last term, is what is left)."""
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
import umap_ref as ur  # noqa: E402
from harmony_amd import RunHarmony, find_ab_params, neighbors, umap, umap_layout  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402

ip, fp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
KEYS = ("fired", "epochs", "long_rows", "short_cap")
AB = {0.5: ur.find_ab(0.5), 0.1: ur.find_ab(0.1)}


def get(h, key):
    out = (C.c_double * 1)()
    assert h.lib.hmx_get(h.h, key, out, 1) == 1, key
    return out[0]


def library(g, Y0, n_epochs, epochs=None, a=AB[0.5][0], b=AB[0.5][1], gamma=1.0, learning_rate=1.0, negative_sample_rate=5, seed=0, short_cap=None):
    """hmx_umap_layout on the graph g = (indptr, indices, weights) -> (status, the output and counters as a dict)"""
    indptr = np.ascontiguousarray(g[0], dtype=np.int64)
    indices, weights = np.ascontiguousarray(g[1], dtype=np.int32), np.ascontiguousarray(g[2], dtype=np.float32)
    Y0 = np.ascontiguousarray(Y0, dtype=np.float32)
    N, dim = Y0.shape
    begin, end = (0, n_epochs) if epochs is None else epochs
    Y = np.full((N, dim), -7.0, dtype=np.float32)
    with _Handle() as h:
        if short_cap is not None:
            assert h.lib.hmx_set_int(h.h, b"umap_short_cap", short_cap) == 0
        status = h.lib.hmx_umap_layout(h.h, indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip), weights.ctypes.data_as(fp), N, dim,
                                       Y0.ctypes.data_as(fp), n_epochs, begin, end, a, b, gamma, learning_rate, negative_sample_rate, seed,
                                       Y.ctypes.data_as(fp))
        out = {k: int(get(h, b"umap:" + k.encode())) for k in KEYS}
        out.update(Y=Y, timer=get(h, b"timer:umap"), error=h.lib.hmx_last_error(h.h).decode())
    return status, out


def within_bound(g, Y32, n, n_epochs, what, **kw):
    """epoch n from the fp32 positions Y32 on the library and in the spec: |Y_gpu - Y_spec| <= B elementwise, equal firings"""
    cap = kw.pop("short_cap", None)
    kw.setdefault("a", AB[0.5][0])
    kw.setdefault("b", AB[0.5][1])
    Y32 = np.ascontiguousarray(Y32, dtype=np.float32)
    want = ur.epoch(g, Y32, n, n_epochs, **kw)
    status, got = library(g, Y32, n_epochs, epochs=(n, n + 1), short_cap=cap, **kw)
    assert status == 0, got["error"]
    err = np.abs(got["Y"].astype(np.float64) - want.Y)
    moved = np.abs(want.Y - Y32).max()
    ratio = float((err / np.maximum(want.B, 1e-300)).max())
    print("umap %s: N=%d dim=%d entries=%d epoch %d of %d %s: fired %d, largest move %.3g, largest error %.3g, largest error / bound %.4f, "
          "long rows %d, %.1f ms" % (what, Y32.shape[0], Y32.shape[1], g[1].size, n, n_epochs, kw, want.fired, moved, err.max(), ratio,
                                     got["long_rows"], got["timer"]))
    assert np.all(np.isfinite(got["Y"])) and got["fired"] == want.fired and got["epochs"] == 1, what
    assert np.all(err <= want.B), (what, ratio)
    return got, want


# ---- (a) single epochs on kNN graphs of the spec's own lists ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cells(N, G):
    return ur.groups(N, G)


@functools.lru_cache(maxsize=None)
def knn_graph(N, G, m):
    idx, dist = mr.knn(cells(N, G)[0], m)[:2]
    return gr.connectivities(idx.astype(np.int32), np.sqrt(np.maximum(np.asarray(dist, dtype=np.float64), 0.0)).astype(np.float32))


EPOCHS = (0, 1, 57, 199)


@functools.lru_cache(maxsize=None)
def trajectory(N, G, m, dim, min_dist):
    """the spec's run of the 200-epoch schedule from the PCA start: the positions epochs 0, 1, 57 and 199 start from, rounded to fp32"""
    a, b = AB[min_dist]
    snap = ur.layout(knn_graph(N, G, m), ur.pca_init(cells(N, G)[0], dim), 200, a, b, snapshots=EPOCHS)[2]
    return {n: Y.astype(np.float32) for n, Y in snap.items()}


@pytest.mark.parametrize("n", EPOCHS)
@pytest.mark.parametrize("N,G,m,dim,min_dist", [(2000, 8, 14, 2, 0.5), (2000, 8, 14, 3, 0.5), (600, 4, 29, 2, 0.1)])
def test_single_epochs(N, G, m, dim, min_dist, n):
    a, b = AB[min_dist]
    got, want = within_bound(knn_graph(N, G, m), trajectory(N, G, m, dim, min_dist)[n], n, 200, "kNN graph", a=a, b=b)
    assert want.fired > N and got["long_rows"] == 0
    if n == 199:
        assert 0.0 < ur.alpha_of(n, 200, 1.0) < 0.0051      # the last epoch still moves


def test_the_clip_engages_at_small_distances():
    """min_dist 0.1 (b < 1) from positions squeezed into a small box: many terms sit on the clip"""
    a, b = AB[0.1]
    g = knn_graph(600, 4, 29)
    Y = (trajectory(600, 4, 29, 2, 0.1)[0] * np.float32(0.01)).astype(np.float32)
    got, want = within_bound(g, Y, 0, 200, "squeezed", a=a, b=b)
    assert np.abs(want.Y - Y).max() > 20.0                   # several clipped terms of 4 add up on a cell


# ---- (b) row lengths, hubs and the long path --------------------------------------------------------------------------------------------------------
def weighted(N, edges, seed=0):
    """csr_of_edges with a symmetric random weight in (0, 1] per edge; the first edge carries 1"""
    rng = np.random.default_rng(seed)
    w = np.maximum(rng.random(len(edges)), 0.02).astype(np.float32)
    w[0] = 1.0
    return lr.csr_of_edges(N, [(i, j, float(x)) for (i, j), x in zip(edges, w)])


def start(N, dim, seed=0):
    return np.random.default_rng(seed).normal(size=(N, dim)).astype(np.float32) * np.float32(3.0)


def test_rows_of_1_63_64_65_and_129_entries():
    edges, nxt, hubs = [], 5, {}
    for hub, L in enumerate((1, 63, 64, 65, 129)):
        edges += [(hub, nxt + t) for t in range(L)]
        hubs[hub] = L
        nxt += L
    g = weighted(nxt, edges)
    assert [int(np.diff(g[0])[h]) for h in hubs] == [1, 63, 64, 65, 129] and np.all(np.diff(g[0])[5:] == 1)
    for dim in (2, 3):
        for n in (0, 3, 9):
            within_bound(g, start(nxt, dim), n, 10, "rows of 1, 63, 64, 65, 129")


@pytest.mark.parametrize("N", [130, 5000])
def test_a_hub_of_in_degree_n_minus_1_around_short_cap(N):
    """a star through cell 0 and a ring through the leaves: the hub's row holds N - 1 entries, every other row 3"""
    g = weighted(N, [(0, i) for i in range(1, N)] + [(i, i + 1) for i in range(1, N - 1)] + [(N - 1, 1)])
    lens = np.diff(g[0])
    assert lens[0] == N - 1 and np.all(lens[1:] == 3)
    Y = start(N, 2)
    for cap, long_rows in ((N - 1, 0), (N - 2, 1), (64, 1), (2, N)):      # the hub at the cap, one above it, far above it; every row above it
        got, _ = within_bound(g, Y, 1, 4, "hub of %d, cap %d" % (N - 1, cap), short_cap=cap)
        assert got["short_cap"] == cap and got["long_rows"] == int((lens > cap).sum()) == long_rows
    got, _ = within_bound(g, Y, 1, 4, "hub of %d, the default cap" % (N - 1))
    assert got["long_rows"] == int((lens > got["short_cap"]).sum()) == (1 if N - 1 > got["short_cap"] else 0)


def test_whole_graphs_through_the_long_path():
    g = knn_graph(2000, 8, 14)
    lens = np.diff(g[0])
    Y = trajectory(2000, 8, 14, 2, 0.5)[57]
    got, _ = within_bound(g, Y, 57, 200, "long path alone", short_cap=0)
    assert got["short_cap"] == 0 and got["long_rows"] == int((lens > 0).sum()) == 2000
    med = int(np.median(lens))
    got, _ = within_bound(g, Y, 57, 200, "a cap at the median row", short_cap=med)
    assert got["long_rows"] == int((lens > med).sum()) and 0 < got["long_rows"] < 2000
    got, _ = within_bound(g, trajectory(2000, 8, 14, 3, 0.5)[1], 1, 200, "long path alone, dim 3", short_cap=0)
    assert got["long_rows"] == 2000


# ---- (c) the other arguments and the smallest inputs -------------------------------------------------------------------------------------------------
def test_negative_sample_rates_and_gamma():
    g = knn_graph(600, 4, 29)
    Y = trajectory(600, 4, 29, 2, 0.1)[57]
    a, b = AB[0.1]
    base = within_bound(g, Y, 57, 200, "5 samples", a=a, b=b)[1]
    none = within_bound(g, Y, 57, 200, "no samples", a=a, b=b, negative_sample_rate=0)[1]
    many = within_bound(g, Y, 57, 200, "31 samples", a=a, b=b, negative_sample_rate=31)[1]
    zero = within_bound(g, Y, 57, 200, "gamma 0", a=a, b=b, gamma=0.0)[1]
    assert none.fired == many.fired == zero.fired == base.fired      # the schedule does not depend on them
    assert np.array_equal(zero.Y, none.Y) and not np.array_equal(base.Y, none.Y) and not np.array_equal(base.Y, many.Y)
    within_bound(g, Y, 57, 200, "gamma 2.5, learning rate 0.25, seed 77", a=a, b=b, gamma=2.5, learning_rate=0.25, seed=77)


def test_one_and_two_cells():
    one = (np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    Y = np.array([[0.5, -2.0]], dtype=np.float32)
    status, got = library(one, Y, 10)
    assert status == 0 and np.array_equal(got["Y"].view(np.uint32), Y.view(np.uint32)) and got["fired"] == 0
    one_diag = (np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.float32))
    status, got = library(one_diag, Y, 10)
    assert status == 0 and np.array_equal(got["Y"].view(np.uint32), Y.view(np.uint32)) and got["fired"] == 0
    two = lr.path(2)                                       # every negative sample is the cell itself or the other one
    for dim in (2, 3):
        Y = start(2, dim, seed=3)
        drawn_self = 0
        for n in range(6):
            within_bound(two, Y, n, 6, "two cells")
            drawn_self += sum(ur.negative_sample(e, n, s, 2, 0) == e for e in (0, 1) for s in range(5))      # entry e belongs to cell e
        assert 15 <= drawn_self <= 45                      # of 60 draws


def test_inputs_the_layout_returns_bit_for_bit():
    Y = start(8, 2, seed=1)
    Y[6] = [-0.0, 0.0]                                     # the sign of a zero is kept too
    bits = Y.view(np.uint32)
    zeros = lr.csr_of_edges(8, [(0, 1, 0.0), (2, 3, 0.0)], diagonal=True)      # wmax == 0: the diagonal does not count
    status, got = library(zeros, Y, 30)
    assert status == 0 and np.array_equal(got["Y"].view(np.uint32), bits) and got["fired"] == 0 and got["epochs"] == 0
    # cells 0 .. 2: a triangle; 3 and 4: joined by an explicit zero; 5: its diagonal alone; 6, 7: nothing
    g = lr.csr_of_edges(8, [(0, 1, 1.0), (1, 2, 0.5), (0, 2, 0.25), (3, 4, 0.0)], diagonal=True)
    g = (g[0][:7].tolist() + [g[0][6]] * 2, g[1][:g[0][6]], g[2][:g[0][6]])      # rows 6 and 7 lose their diagonal
    want, fired, _ = ur.layout(g, Y, 30, *AB[0.5])
    status, got = library(g, Y, 30)
    assert status == 0 and got["fired"] == fired == 2 * (30 + 15 + 7) and got["epochs"] == 30
    assert np.array_equal(got["Y"][3:].view(np.uint32), bits[3:]) and not np.any(got["Y"][:3] == Y[:3])
    for n in (0, 1, 29):
        step = within_bound(g, Y, n, 30, "a triangle, zeros and diagonals")[0]
        assert np.array_equal(step["Y"][3:].view(np.uint32), bits[3:])
    same = np.full((8, 3), 1.25, dtype=np.float32)         # all-equal positions: every distance is 0, every term 0
    status, got = library(g, same, 30)
    assert status == 0 and np.array_equal(got["Y"], same) and got["fired"] == fired
    status, got = library(g, Y, 30, epochs=(7, 7))         # no epoch asked for
    assert status == 0 and np.array_equal(got["Y"].view(np.uint32), bits) and got["epochs"] == 0


# ---- (d) repeatability and whole layouts ---------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits_and_parts_add_up():
    g = knn_graph(2000, 8, 14)
    Y0 = ur.pca_init(cells(2000, 8)[0], 2)
    a, b = library(g, Y0, 200, epochs=(0, 20))[1], library(g, Y0, 200, epochs=(0, 20))[1]
    assert np.array_equal(a["Y"].view(np.uint32), b["Y"].view(np.uint32)) and a["fired"] == b["fired"] and a["epochs"] == 20
    first = library(g, Y0, 200, epochs=(0, 10))[1]
    second = library(g, first["Y"], 200, epochs=(10, 20))[1]
    assert np.array_equal(second["Y"].view(np.uint32), a["Y"].view(np.uint32)) and first["fired"] + second["fired"] == a["fired"]
    assert a["fired"] == ur.layout(g, Y0, 200, *AB[0.5], epochs=(0, 20))[1]
    other = library(g, Y0, 200, epochs=(0, 20), seed=1)[1]
    assert not np.array_equal(other["Y"], a["Y"]) and other["fired"] == a["fired"]
    # the long path adds a row in another shape: other last bits, which twenty epochs magnify -- but the same ones in every call
    long_path, again = library(g, Y0, 200, epochs=(0, 20), short_cap=0)[1], library(g, Y0, 200, epochs=(0, 20), short_cap=0)[1]
    assert np.array_equal(long_path["Y"].view(np.uint32), again["Y"].view(np.uint32)) and long_path["fired"] == a["fired"] and long_path["long_rows"] == 2000
    assert np.all(np.isfinite(long_path["Y"]))


# The fp64 spec's own 200-epoch runs on knn_graph(3000, 12, 14) over seeds 0 .. 4 (spec_trustworthiness below, about 5 s a run):
#   from the PCA start      trustworthiness 0.97529, 0.97569, 0.97484, 0.97544, 0.97532: smallest 0.974843, spread 0.000847; purity 1.0
#   from the random start   trustworthiness 0.97500, 0.97535, 0.97531, 0.97506, 0.97588: smallest 0.975001, spread 0.000875; purity 1.0
SPEC_TRUST = {"pca": (0.974843, 0.000847), "random": (0.975001, 0.000875)}


def full_start(init):
    X = cells(3000, 12)[0]
    return ur.pca_init(X, 2) if init == "pca" else ur.random_init(3000, 2, 0)


def spec_trustworthiness(init):
    """what SPEC_TRUST records: (the smallest trustworthiness of the spec's runs over seeds 0 .. 4, max - min)"""
    X, g = cells(3000, 12)[0], knn_graph(3000, 12, 14)
    t = [ur.trustworthiness(X, ur.layout(g, full_start(init), 200, *AB[0.5], seed=s)[0]) for s in range(5)]
    return min(t), max(t) - min(t)


@pytest.mark.parametrize("init", ["pca", "random"])
def test_full_layouts_are_held_by_quality(init):
    X, lab = cells(3000, 12)
    g = knn_graph(3000, 12, 14)
    Y0 = full_start(init)
    Y = umap_layout(sp.csr_matrix((g[2], g[1], g[0]), shape=(3000, 3000)), Y0 if init == "pca" else "random", n_epochs=200, a=AB[0.5][0], b=AB[0.5][1])
    status, got = library(g, Y0, 200)
    assert status == 0 and np.array_equal(Y.view(np.uint32), got["Y"].view(np.uint32)) and Y.dtype == np.float32      # "random" is random_init(seed)
    trust, purity = ur.trustworthiness(X, Y), ur.knn_purity(Y, lab)
    low, spread = SPEC_TRUST[init]
    print("umap full layout from %s: 3000 cells, 200 epochs, %d firings, %.1f ms: trustworthiness %.5f (the spec's runs: %.5f and above, spread "
          "%.5f), purity %.4f, the start's trustworthiness %.5f" % (init, got["fired"], got["timer"], trust, low, spread, purity, ur.trustworthiness(X, Y0)))
    assert np.all(np.isfinite(Y)) and purity >= 0.99
    assert trust >= low - spread
    assert got["fired"] == int(ur.firings(ur.edges(*g)[2][ur.edges(*g)[3]], 200).sum())


# ---- (e) the wrappers ------------------------------------------------------------------------------------------------------------------------------------
def test_umap_is_neighbors_then_umap_layout():
    X = cells(2000, 8)[0]
    Y = umap(X, n_neighbors=15, n_epochs=30)
    conn = neighbors(X, n_neighbors=15)[1]
    again = umap_layout(conn, ur.pca_init(X, 2), n_epochs=30)
    assert Y.shape == (2000, 2) and np.array_equal(Y.view(np.uint32), again.view(np.uint32))
    Y3 = umap(X, n_neighbors=10, init="random", n_components=3, n_epochs=30, min_dist=0.1, seed=4)
    a, b = find_ab_params(1.0, 0.1)
    again = umap_layout(neighbors(X, n_neighbors=10)[1], ur.random_init(2000, 3, 4), n_components=3, n_epochs=30, a=a, b=b, seed=4)
    assert Y3.shape == (2000, 3) and np.array_equal(Y3.view(np.uint32), again.view(np.uint32)) and np.all(np.isfinite(Y3))
    triple = umap_layout((conn.indptr, conn.indices, conn.data), ur.pca_init(X, 2), n_epochs=30)
    assert np.array_equal(triple, Y)
    part = umap_layout(conn, umap_layout(conn, ur.pca_init(X, 2), n_epochs=30, epochs=(0, 12)), n_epochs=30, epochs=(12, 30))
    assert np.array_equal(part, Y)


def test_harmony_umap_is_umap_of_z_corr():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines_small.npz"))
    meta = {"dataset": fx["dataset_levels"][fx["dataset"]]}
    obj = RunHarmony(fx["pcs"], meta, "dataset", return_object=True, verbose=False, seed=1, max_iter=2, nclust=10)
    a = obj.umap(n_epochs=40)
    b = umap(np.asarray(obj.getZcorr()).T, n_epochs=40)
    assert a.shape == (fx["pcs"].shape[0], 2) and a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.all(np.isfinite(a)) and obj.timer("umap") > 0
    c = obj.umap(n_neighbors=10, min_dist=0.1, n_components=3, init="random", n_epochs=40, seed=2)
    d = umap(np.asarray(obj.getZcorr()).T, n_neighbors=10, min_dist=0.1, n_components=3, init="random", n_epochs=40, seed=2)
    assert c.shape[1] == 3 and np.array_equal(c.view(np.uint32), d.view(np.uint32))


# ---- (f) malformed graphs ------------------------------------------------------------------------------------------------------------------------------
def test_malformed_graphs_are_refused_before_any_epoch_runs():
    indptr, indices, weights = [a.copy() for a in lr.two_cliques()]
    Y0 = start(14, 2)

    def refused(g, text):
        status, got = library(g, Y0, 20)
        assert status == 1 and text in got["error"], (status, got["error"])      # HMX_ERR_ARG
        assert got["epochs"] == 0 and got["fired"] == 0 and np.all(got["Y"] == -7.0)
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
    status, got = library((indptr, indices, weights), Y0, 20)      # ... and the graph itself is taken
    assert status == 0 and got["epochs"] == 20 and got["fired"] == 20 * indices.size
