"""The UMAP layout held to its spec (tests/umap_ref.py) without a GPU: the header, the library and the binding agree; every argument error
that the host can see is raised before a device is needed; the hash, the schedule and one epoch worked by hand; the spec's invariances; the
curve fit and the starting positions; and the quality bar (tests/test_gpu_umap.py runs the library).

The quality bar: the synchronous, hashed epoch against umap-learn's one-thread loop (umap_ref.sequential) from the same start, by
trustworthiness at k = 15, N = 600, 100 epochs: trust(spec) >= 0.97 trust(sequential), trust(spec) > trust(start), purity >= 0.99 on the
planted groups.  Measured: groups 0.9378 / 0.9389 (ratio 0.9988), swiss roll 0.9957 / 0.9942 (1.0015), 10-d noise 0.7405 / 0.7479 (0.9901)."""
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
import louvain_ref as lr  # noqa: E402
import metrics_ref as mr  # noqa: E402
import umap_ref as ur  # noqa: E402
from harmony_amd import Harmony, _lib, find_ab_params, umap, umap_layout  # noqa: E402
from harmony_amd.umap import pca_init, random_init  # noqa: E402

HEADER = "harmony_mi355x_umap.h"
AB = ur.find_ab(0.5)


def test_umap_header_matches_the_library_and_the_binding():
    found = helpers.header_functions(HEADER)
    mine = [n for n, _ in found]
    assert mine == ["hmx_umap_layout"] and set(mine) == set(_lib.UMAP_SIGNATURES)
    for other, table in helpers.PUBLIC_HEADERS + (("harmony_mi355x_louvain.h", "LOUVAIN_SIGNATURES"),):      # every header before this one
        assert other != HEADER and not (set(mine) & helpers.header_names(other)), other
        assert not (set(mine) & set(getattr(_lib, table))), table
    tables = [t for t in dir(_lib) if t.endswith("SIGNATURES") and t != "UMAP_SIGNATURES"]
    assert len(tables) >= 11 and not any(set(mine) & set(getattr(_lib, t)) for t in tables)
    ctypes_of = dict(helpers.CTYPES, uint32_t=(C.c_uint32,))      # the seed: the one type no earlier header uses
    lib = _lib.load()
    for name, types in found:
        fn, sig = getattr(lib, name), _lib.UMAP_SIGNATURES[name][1]
        assert fn.restype is C.c_int and list(fn.argtypes) == sig and len(types) == len(sig) == 17
        for t, s in zip(types, sig):
            assert any(s is o or s == o for o in ctypes_of[t]), (name, t, s)


# ---- the hash and the schedule ---------------------------------------------------------------------------------------------------------------
def by_hand(x):
    x %= 2 ** 32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) % 2 ** 32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) % 2 ** 32
    return x ^ (x >> 16)


def test_key_and_negative_sample_known_answers():
    """key(n, s) = fmix32(fmix32(seed) + 32 n + s + 1) mod 2^32; k = (fmix32(e ^ key) N) >> 32"""
    assert ur.key(0, 0, 0) == by_hand(1) == 0x514E28B7                     # fmix32(0) = 0
    assert ur.key(3, 2, 7) == by_hand(by_hand(7) + 32 * 3 + 2 + 1) == 0x6C763D65 and by_hand(7) == 0x18C9AEC4
    assert ur.key(199, 30, 0xFFFFFFFF) == by_hand(0x81F16F39 + 32 * 199 + 31) == 0x719747D9
    n = 2 ** 20 - 1
    wrap = next(s for s in range(100000) if by_hand(s) > 2 ** 32 - 32 * n)      # a seed whose hash wraps around in the last epoch
    assert ur.key(n, 5, wrap) == by_hand((by_hand(wrap) + 32 * n + 6) % 2 ** 32) and by_hand(wrap) + 32 * n + 6 >= 2 ** 32
    for (e, n, s, N, seed), h, k in (((0, 0, 0, 3, 0), 0x2FEF5C8F, 0), ((5, 3, 2, 1000, 7), 0x435057C8, 262),
                                     ((123456, 199, 30, 2 ** 31 - 1, 0xFFFFFFFF), 0xB79E83E8, 1540309491), ((41999, 57, 4, 2000, 0), 0x250ECD5A, 289)):
        assert by_hand(e ^ ur.key(n, s, seed)) == h and ur.negative_sample(e, n, s, N, seed) == (h * N) >> 32 == k
    ks = [ur.negative_sample(e, 4, 1, 7, 0) for e in range(7000)]
    assert min(ks) == 0 and max(ks) == 6 and min(np.bincount(ks)) > 800      # every cell is drawn, about equally often


def test_firing_rule_counts():
    """over the whole schedule an entry fires floor(n_epochs r) times: never for w < wmax / n_epochs, every epoch for w = wmax"""
    w = np.array([1.0, 0.999, 0.75, 0.5, 1.0 / 3.0, 0.1, 0.0101, 0.01, 0.0099, 0.004, 0.0], dtype=np.float32)
    for scale in (1.0, 0.8):
        ws = (w * np.float32(scale)).astype(np.float32)
        r = ws.astype(np.float64) / np.float64(ws.max())
        for n_epochs in (1, 7, 100, 200):
            count = ur.firings(r, n_epochs)
            assert count.tolist() == np.floor(n_epochs * r).astype(np.int64).tolist()
            assert np.all(count[r < 1.0 / n_epochs] == 0) and count[0] == n_epochs
    r = np.float64(np.float32(0.5)) / np.float64(1.0)
    assert [bool(ur.fires(r, n)) for n in range(6)] == [False, True] * 3      # every second epoch, first in epoch 1
    # through edges(): r is dbl(w) / dbl(wmax) with the diagonal left out of wmax
    g = lr.csr_of_edges(3, [(0, 1, 0.5), (1, 2, 0.25)], diagonal=True)
    src, dst, r, off, wmax = ur.edges(*g)
    assert wmax == 0.5 and sorted(r[off].tolist()) == [0.5, 0.5, 1.0, 1.0] and (~off).sum() == 3


def path3(w12=1.0):
    return lr.csr_of_edges(3, [(0, 1, 1.0), (1, 2, w12)])


def test_one_epoch_on_a_path_of_three_by_hand():
    """a = b = 1: c_a = -2 / (1 + d2).  y = 0, 1, 3 on a line, every weight 1, epoch 0 of 10 (alpha = 1), no negative samples:
    cell 0: d = -1, d2 = 1, c = -1: 2 (c d) = +2;  cell 1: from 0: d = 1: -2; from 2: d = -2, d2 = 4, c = -0.4: 2 (0.8) = 1.6;  cell 2: -1.6"""
    Y = np.array([[0.0, 0.0], [1.0, 0.0], [3.0, 0.0]], dtype=np.float32)
    step = ur.epoch(path3(), Y, 0, 10, 1.0, 1.0, negative_sample_rate=0)
    assert step.fired == 4 and np.allclose(step.Y, [[2.0, 0.0], [0.6, 0.0], [1.4, 0.0]], atol=1e-15)
    assert np.all(step.B[:, 0] > 0) and np.all(step.B[:, 0] < 1e-4)
    # weight 1/2 on the second edge: it rests in epoch 0 and fires in epoch 1, where alpha = float32(0.9)
    step = ur.epoch(path3(0.5), Y, 0, 10, 1.0, 1.0, negative_sample_rate=0)
    assert step.fired == 2 and np.allclose(step.Y, [[2.0, 0.0], [-1.0, 0.0], [3.0, 0.0]], atol=1e-15)
    step = ur.epoch(path3(0.5), Y, 1, 10, 1.0, 1.0, negative_sample_rate=0)
    al = float(np.float32(0.9))
    assert step.fired == 4 and np.allclose(step.Y, [[2.0 * al, 0.0], [1.0 - 0.4 * al, 0.0], [3.0 - 1.6 * al, 0.0]], atol=1e-15)
    # one negative sample per firing, by the definition: c_r = 2 gamma b / ((0.001 + d2)(a d2^b + 1)), clipped to [-4, 4]
    Y = np.array([[0.0, 0.0], [0.1, 0.0], [3.0, 1.0]], dtype=np.float64)
    g = path3()
    seed = next(s for s in range(100) if ur.negative_sample(0, 0, 0, 3, s) == 1)      # entry 0 = (0, 1) draws cell 1
    step = ur.epoch(g, Y, 0, 10, 1.0, 1.0, gamma=1.5, negative_sample_rate=1, seed=seed)
    want = Y.copy()
    for e, (i, j) in enumerate([(0, 1), (1, 0), (1, 2), (2, 1)]):
        d = Y[i] - Y[j]
        want[i] += 2.0 * np.clip(-2.0 / (1.0 + d @ d) * d, -4.0, 4.0)
        k = ur.negative_sample(e, 0, 0, 3, seed)
        d = Y[i] - Y[k]
        if k != i and d @ d > 0:
            want[i] += np.clip(2.0 * 1.5 / ((0.001 + d @ d) * (d @ d + 1.0)) * d, -4.0, 4.0)
    assert np.allclose(step.Y, want, atol=1e-14)
    assert abs(step.Y[0, 0] - (2.0 * (2.0 / 1.01 * 0.1) - 4.0)) < 1e-14      # cell 0 against cell 1 at d2 = 0.01: c_r d = -27, clipped to -4


# ---- invariances of the spec -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def knn_graph(name, N, m=14):
    X, lab = {"groups": lambda: ur.groups(N, 4), "roll": lambda: (ur.swiss_roll(N), None), "noise": lambda: (ur.noise(N), None)}[name]()
    idx, dist = mr.knn(X, m)[:2]
    g = gr.connectivities(idx.astype(np.int32), np.sqrt(np.maximum(np.asarray(dist, dtype=np.float64), 0.0)).astype(np.float32))
    return X, lab, g


def test_a_schedule_run_in_two_parts_is_the_whole():
    X, _, g = knn_graph("groups", 300)
    Y0 = ur.pca_init(X, 2)
    half, f1, _ = ur.layout(g, Y0, 50, *AB, epochs=(0, 10))
    both, f2, _ = ur.layout(g, half, 50, *AB, epochs=(10, 20))
    whole, f, snap = ur.layout(g, Y0, 50, *AB, epochs=(0, 20), snapshots=(10,))
    assert np.array_equal(both, whole) and f1 + f2 == f and np.array_equal(snap[10], half)
    assert not np.array_equal(whole, ur.layout(g, Y0, 50, *AB, epochs=(0, 20), seed=1)[0])


def test_inputs_the_layout_returns_unchanged():
    Y = np.random.default_rng(0).normal(size=(5, 2)).astype(np.float32)
    zero = lr.csr_of_edges(5, [(0, 1, 0.0), (2, 3, 0.0)], diagonal=True)      # wmax == 0 (the diagonal does not count)
    out, fired, _ = ur.layout(zero, Y, 30, *AB)
    assert np.array_equal(out, Y) and fired == 0
    one = (np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))      # N = 1
    assert np.array_equal(ur.layout(one, Y[:1], 30, *AB)[0], Y[:1])
    g = lr.csr_of_edges(5, [(0, 1), (1, 2), (0, 2)])       # cells 3 and 4 are isolated
    out = ur.layout(g, Y, 30, *AB)[0]
    assert np.array_equal(out[3:], Y[3:]) and not np.any(out[:3] == Y[:3])
    same = np.full((5, 2), 1.25, dtype=np.float32)         # all-equal starting positions: every d2 is 0
    out, fired, _ = ur.layout(g, same, 30, *AB)
    assert np.array_equal(out, same) and fired == 6 * 30


def test_find_ab_params():
    for min_dist, want in ((0.5, (0.583, 1.334)), (0.1, (1.577, 0.895))):
        a, b = find_ab_params(1.0, min_dist)
        assert abs(a - want[0]) < 1e-3 and abs(b - want[1]) < 1e-3 and ur.find_ab(min_dist) == want
    with pytest.raises(ValueError, match="spread"):
        find_ab_params(0.0, 0.5)
    with pytest.raises(ValueError, match="min_dist"):
        find_ab_params(1.0, 3.0)


def test_starting_positions_are_deterministic():
    X = ur.groups(200, 3)[0]
    for dim in (2, 3):
        r = random_init(200, dim, 5)
        assert r.dtype == np.float32 and r.shape == (200, dim) and np.array_equal(r, random_init(200, dim, 5)) and np.array_equal(r, ur.random_init(200, dim, 5))
        assert np.all(np.abs(r) <= 10.0) and not np.array_equal(r, random_init(200, dim, 6)) and abs(float(r.mean())) < 1.5
        p = pca_init(X, dim)
        assert p.dtype == np.float32 and np.array_equal(p, pca_init(X, dim)) and np.array_equal(p, ur.pca_init(X, dim))
        assert abs(float(np.abs(p).max()) - 10.0) < 1e-5
        cov = np.cov(p.astype(np.float64).T)
        assert np.all(np.diff(np.diag(cov)) < 0) and abs(cov[0, 1]) < 1e-4 * cov[0, 0]      # principal axes: descending variance, uncorrelated
    i = 7                                                  # one coordinate from the definition
    want = 20.0 * (by_hand(i ^ by_hand(5 + 0x51ED)) + 0.5) / 2.0 ** 32 - 10.0
    assert random_init(200, 2, 5).ravel()[i] == np.float32(want)
    assert np.array_equal(pca_init(-X, 2), -pca_init(X, 2))      # the axes' signs follow the loadings, not the data
    flipped = pca_init(X[:, ::-1], 2)                      # reordering the columns changes no coordinate but by rounding
    assert np.allclose(flipped, pca_init(X, 2), atol=1e-4)


# ---- quality: against umap-learn's sequential loop ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["groups", "roll", "noise"])
def test_quality_against_the_sequential_loop(name):
    X, lab, g = knn_graph(name, 600)
    Y0 = ur.pca_init(X, 2)
    Y = ur.layout(g, Y0, 100, *AB)[0]
    Ys = ur.sequential(g, Y0, 100, *AB)
    t, ts, t0 = ur.trustworthiness(X, Y), ur.trustworthiness(X, Ys), ur.trustworthiness(X, Y0)
    print("%s: trustworthiness(15) synchronous %.4f, sequential %.4f, ratio %.4f; the PCA start %.4f" % (name, t, ts, t / ts, t0))
    assert np.all(np.isfinite(Y)) and t >= 0.97 * ts and t > t0
    if lab is not None:
        purity = ur.knn_purity(Y, lab)
        print("%s: purity %.4f" % (name, purity))
        assert purity >= 0.99


def test_quality_measures_on_known_embeddings():
    X, lab = ur.groups(300, 3)
    assert ur.trustworthiness(X, X.astype(np.float64) * 2.0) == 1.0 and ur.knn_purity(X, lab) == 1.0
    shuffled = X[np.random.default_rng(0).permutation(300)]
    assert 0.4 < ur.trustworthiness(X, shuffled) < 0.7 and ur.knn_purity(shuffled, lab) < 0.5
    sk = pytest.importorskip("sklearn.manifold")
    Y = ur.pca_init(X, 2)
    assert abs(ur.trustworthiness(X, Y) - sk.trustworthiness(X.astype(np.float64), Y.astype(np.float64), n_neighbors=15)) < 1e-12


# ---- every argument error is raised before a device is needed --------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device():
    indptr, indices, weights = lr.two_cliques()
    g = sp.csr_matrix((weights, indices, indptr), shape=(14, 14))
    Y0 = np.zeros((14, 2), dtype=np.float32)
    for kw, msg in (({"n_components": 1}, "n_components"), ({"n_components": 4}, "n_components"), ({"n_components": 2.5}, "n_components"),
                    ({"n_epochs": 0}, "n_epochs"), ({"n_epochs": 2 ** 20 + 1}, "n_epochs"), ({"n_epochs": 1.5}, "n_epochs"),
                    ({"n_epochs": 20, "epochs": (5, 21)}, "epochs"), ({"n_epochs": 20, "epochs": (-1, 5)}, "epochs"),
                    ({"n_epochs": 20, "epochs": (6, 5)}, "begin <= end"), ({"epochs": 3}, "pair"), ({"gamma": -0.5}, "gamma"),
                    ({"gamma": float("nan")}, "gamma"), ({"learning_rate": 0.0}, "learning_rate"), ({"learning_rate": float("inf")}, "learning_rate"),
                    ({"negative_sample_rate": -1}, "negative_sample_rate"), ({"negative_sample_rate": 32}, "negative_sample_rate"),
                    ({"seed": -1}, "seed"), ({"seed": 2 ** 32}, "seed"), ({"a": 1.0}, "both a and b"), ({"a": 0.0, "b": 1.0}, "a must"),
                    ({"a": 1.0, "b": float("nan")}, "b must"), ({"min_dist": 5.0}, "min_dist"), ({"spread": -1.0}, "spread")):
        with pytest.raises(ValueError, match=msg):
            umap_layout(g, Y0, **kw)
    for init, msg in ((np.zeros((14, 3), dtype=np.float32), "init must be"), (np.zeros((13, 2)), "init must be"), ("pca", "init must be"),
                      ("spectral", "init must be"), (np.full((14, 2), np.nan), "not finite")):
        with pytest.raises(ValueError, match=msg):
            umap_layout(g, init, a=1.0, b=1.0)
    with pytest.raises(ValueError, match="square"):
        umap_layout(sp.csr_matrix(np.ones((3, 4))), Y0)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        umap_layout((indptr, indices, weights * 1.5), Y0)
    with pytest.raises(ValueError, match="no mirror"):
        umap_layout(sp.csr_matrix(([1.0], ([0], [1])), shape=(14, 14)), Y0)
    X = ur.groups(40, 2)[0]
    for kw, msg in (({"n_neighbors": 1}, "n_neighbors"), ({"n_neighbors": 41}, "n_neighbors"), ({"init": "spectral"}, "'pca'"),
                    ({"n_components": 5}, "n_components"), ({"init": np.zeros((39, 2))}, "init must be")):
        with pytest.raises(ValueError, match=msg):
            umap(X, **kw)
    with pytest.raises(ValueError, match="cells x PCs"):
        umap(np.zeros(5))
    with pytest.raises(ValueError, match="n_components"):
        umap(X[:, :2], n_components=3)                     # 'pca' has only two axes to give
    assert callable(Harmony.umap)


def test_library_argument_errors_come_before_the_device():
    lib = _lib.load()
    ip, fp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    h = C.c_void_p(lib.hmx_create())
    ARG, LIMIT = 1, 7
    indptr, indices, weights = lr.two_cliques()
    Y0 = np.random.default_rng(0).normal(size=(64, 3)).astype(np.float32)
    try:
        def call(N=14, dim=2, n_epochs=20, begin=0, end=20, a=1.0, b=1.0, gamma=1.0, lr_=1.0, neg=5, seed=0, ptr=indptr, null=None, start=Y0):
            ptr = np.ascontiguousarray(ptr, dtype=np.int64)
            start = np.ascontiguousarray(start, dtype=np.float32)
            Y = np.zeros((64, 3), dtype=np.float32)
            arg = {"indptr": ptr.ctypes.data_as(lp), "indices": indices.ctypes.data_as(ip), "weights": weights.ctypes.data_as(fp),
                   "Y0": start.ctypes.data_as(fp), "Y": Y.ctypes.data_as(fp)}
            if null:
                arg[null] = None
            s = lib.hmx_umap_layout(h, arg["indptr"], arg["indices"], arg["weights"], N, dim, arg["Y0"], n_epochs, begin, end, a, b, gamma, lr_,
                                    neg, seed, arg["Y"])
            assert not Y.any()                             # Y is not written
            return s
        for null in ("indptr", "indices", "weights", "Y0", "Y"):
            assert call(null=null) == ARG, null
        assert call(N=0) == ARG and call(N=-3) == ARG
        for bad in (1, 4, 0, -2):
            assert call(dim=bad) == ARG and b"dim" in lib.hmx_last_error(h)
        for bad in (0, -1, 2 ** 20 + 1):
            assert call(n_epochs=bad, begin=0, end=0) == ARG and b"n_epochs" in lib.hmx_last_error(h)
        for begin, end in ((-1, 5), (5, 21), (6, 5), (21, 21)):
            assert call(begin=begin, end=end) == ARG and b"epoch_begin" in lib.hmx_last_error(h)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(a=bad) == ARG and call(b=bad) == ARG and b"a and b" in lib.hmx_last_error(h)
            assert call(lr_=bad) == ARG and b"learning_rate" in lib.hmx_last_error(h)
        for bad in (-0.5, float("nan"), float("inf")):
            assert call(gamma=bad) == ARG and b"gamma" in lib.hmx_last_error(h)
        for bad in (-1, 32):
            assert call(neg=bad) == ARG and b"negative_sample_rate" in lib.hmx_last_error(h)
        shifted = indptr.copy()
        shifted[0] = 1
        assert call(ptr=shifted) == ARG and b"start at 0" in lib.hmx_last_error(h)
        down = indptr.copy()
        down[3] = down[2] - 1
        assert call(ptr=down) == ARG and b"ascend" in lib.hmx_last_error(h)
        assert call(N=2, ptr=np.array([0, 3, 4])) == ARG      # a row longer than N
        assert call(N=2000000001) == LIMIT                   # (refused before a row is read)
        assert call(N=2 ** 31 // 1000 + 1000, ptr=np.arange(2 ** 31 // 1000 + 1001) * 1000) == LIMIT
        for bad in (np.nan, np.inf, -np.inf):
            start = Y0.copy()
            start.ravel()[13 * 2 + 1] = bad
            assert call(start=start) == ARG and b"Y0" in lib.hmx_last_error(h) and b"cell 13" in lib.hmx_last_error(h)
        assert lib.hmx_umap_layout(None, None, None, None, 1, 2, None, 1, 0, 1, 1.0, 1.0, 1.0, 1.0, 5, 0, None) == ARG
        assert lib.hmx_set_int(h, b"umap_short_cap", -2) == ARG and lib.hmx_set_int(h, b"umap_short_cap", 16) == 0
        out1 = (C.c_double * 1)()
        for key in (b"umap:fired", b"umap:epochs", b"umap:long_rows", b"umap:short_cap", b"timer:umap"):
            assert lib.hmx_get(h, key, out1, 1) == 1, key
        assert lib.hmx_get(h, b"umap:short_cap", out1, 1) == 1 and out1[0] == 16
        assert lib.hmx_set_int(h, b"umap_short_cap", 0) == 0 and lib.hmx_get(h, b"umap:short_cap", out1, 1) == 1 and out1[0] == 0
        assert lib.hmx_set_int(h, b"umap_short_cap", -1) == 0 and lib.hmx_get(h, b"umap:short_cap", out1, 1) == 1 and out1[0] >= 256
        assert lib.hmx_get(h, b"umap:epochs", out1, 1) == 1 and out1[0] == 0
    finally:
        lib.hmx_destroy(h)
