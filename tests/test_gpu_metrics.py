"""Integration metrics on the MI355X against the fp64 spec (tests/metrics_ref.py): exact kNN on lattice data (indices and distances must
be equal, ties and duplicates included) and on real-valued data (within the rounding bound of the fp32 distance form), the LISI stage on
the spec's own neighbour lists, compute_lisi end to end, the scores of a Harmony fit of the cell-line data, and kNN label transfer.

Sizes the kNN kernel takes another path at: 64 query rows per workgroup, 64 data rows per slab, data chunks that are multiples of 64 rows
and at least 2 k long (one chunk once the query tiles alone give 512 workgroups), lists of 64 positions for k <= 64 and 128 above, PC
groups of 16 (kernels built for 2, 4 and 8 groups: d <= 32, <= 64, <= 128)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import metrics_ref as mr  # noqa: E402
from bench_data import synth  # noqa: E402
from harmony_amd import Harmony, RunHarmony, _lib, compute_lisi, knn, knn_predict, lisi_from_knn, map_query, prepare_setup_args  # noqa: E402
from harmony_amd.utils import harmonize  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


# ---- 1. lattice: exact ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(d, separate):
    rng = np.random.default_rng(100 + d)
    X = rng.integers(-4, 5, size=(2000, d)).astype(np.float64)
    Q = rng.integers(-4, 5, size=(1000, d)).astype(np.float64) if separate else None
    idx, d2 = mr.knn(X, 128, Q)
    return X, Q, idx, d2


@pytest.mark.parametrize("separate", [False, True])
@pytest.mark.parametrize("d", [3, 50, 76])
def test_lattice_knn_is_exact(d, separate):
    X, Q, ridx, rd2 = lattice(d, separate)
    for k in (1, 15, 89, 128):
        idx, dist = knn(X, k, query=Q)
        assert idx.dtype == np.int32 and dist.dtype == np.float32 and idx.shape == (ridx.shape[0], k)
        bad = np.nonzero((idx != ridx[:, :k]).any(axis=1))[0]
        assert bad.size == 0, (k, bad[:5], idx[bad[:1]], ridx[bad[:1], :k])
        assert np.array_equal(dist, np.sqrt(rd2[:, :k]).astype(np.float32)), k
        if not separate:
            assert not (idx == np.arange(idx.shape[0])[:, None]).any()


def test_duplicates_of_a_cell_are_returned_but_not_the_cell_itself():
    X = np.zeros((70, 5))
    X[40:] = 3.0
    idx, dist = knn(X, 39)
    assert np.array_equal(idx[0], np.arange(1, 40)) and np.array_equal(idx[39], np.arange(0, 39)) and not dist[:40].any()
    assert np.array_equal(idx[69, :29], np.arange(40, 69)) and np.array_equal(idx[69, 29:], np.arange(0, 10))


# ---- 2. real-valued ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(3000, 50, 90), (2000, 20, 30), (1500, 76, 90), (4099, 50, 89), (12000, 50, 89),
          (91, 50, 90),                                   # N = k + 1
          (63, 50, 30), (65, 50, 30), (129, 50, 60), (257, 128, 128), (193, 1, 64), (640, 33, 65)]     # slab / tile / chunk / list / PC-group boundaries


@functools.lru_cache(maxsize=None)
def real_case(N, d):
    Z, meta, _ = synth(N, d=d, levels=(4,), seed=5)
    kk = min(91 if N >= 1500 else 129, N - 1)
    idx, d2 = mr.knn(Z, kk)
    return Z, np.asarray(meta["cov0"]), idx, d2


def true_d2(X, Q, idx):
    X, Q = mr.as_f32_f64(X), mr.as_f32_f64(Q)
    out = np.zeros(idx.shape)
    for j in range(X.shape[1]):
        t = Q[:, j:j + 1] - X[idx, j]
        out += t * t
    return out


def check_knn(X, Q, k, idx, dist, ridx, rd2, self_excl, min_clear=0.95):
    """the three requirements of the real-valued case; returns the clear rows"""
    d = X.shape[1]
    Xf, Qf = mr.as_f32_f64(X), mr.as_f32_f64(Q)
    n2x, n2q = (Xf * Xf).sum(axis=1), (Qf * Qf).sum(axis=1)
    assert (idx >= 0).all() and (idx < X.shape[0]).all()
    if self_excl:
        assert not (idx == np.arange(idx.shape[0])[:, None]).any()
    assert all(len(set(r)) == k for r in idx[:: max(1, idx.shape[0] // 200)])
    bar = (2 * d + 4) * U * (n2q[:, None] + n2x[idx])
    t = true_d2(X, Q, idx)
    e1 = np.abs(dist.astype(np.float64) ** 2 - t) / bar
    rbar = (2 * d + 4) * U * (n2q + np.maximum(n2x[idx].max(axis=1), n2x[ridx[:, :k]].max(axis=1)))
    e2 = np.abs(np.sort(t, axis=1) - rd2[:, :k]) / rbar[:, None]
    if rd2.shape[1] > k:
        kbar = (2 * d + 4) * U * (n2q + n2x[ridx[:, k - 1:k + 1]].max(axis=1))
        clear = (rd2[:, k] - rd2[:, k - 1]) > 2 * kbar
    else:
        clear = np.ones(idx.shape[0], bool)
    same = np.array([set(a) == set(b) for a, b in zip(idx, ridx[:, :k])])
    print("knn N=%d Nq=%d d=%d k=%d: max err/bar to own index %.3f, sorted-set %.3f, clear share %.4f, clear rows with another set %d"
          % (X.shape[0], Q.shape[0], d, k, e1.max(), e2.max(), clear.mean(), int((clear & ~same).sum())))
    assert e1.max() <= 1.0
    assert e2.max() <= 1.0
    assert clear.mean() >= min_clear
    assert same[clear].all()
    assert (np.diff(dist, axis=1) >= 0).all()
    return clear


@pytest.mark.parametrize("N,d,k", SHAPES)
def test_real_valued_knn(N, d, k):
    Z, _, ridx, rd2 = real_case(N, d)
    idx, dist = knn(Z, k)
    check_knn(Z, Z, k, idx, dist, ridx, rd2, True)
    idx2, dist2 = knn(Z, k)
    assert np.array_equal(idx, idx2) and np.array_equal(dist.view(np.uint32), dist2.view(np.uint32))


def test_few_query_rows_against_many_chunks():
    """5 and 70 query rows against 12000 data rows: one and two query tiles, 63 chunks of 192 rows (k = 89)"""
    Z, _, _, _ = real_case(12000, 50)
    Q, _, _ = synth(70, d=50, levels=(4,), seed=5, shard=2)
    ridx, rd2 = mr.knn(Z, 89, Q, extra=1)
    for nq in (5, 70):
        idx, dist = knn(Z, 89, query=Q[:nq])
        check_knn(Z, Q[:nq], 89, idx, dist, ridx[:nq], rd2[:nq], False, min_clear=0.9)


def test_input_forms_give_identical_indices():
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    Z, _, _, _ = real_case(3000, 50)
    a, da = knn(Z, 90)
    b, db = knn(Z.astype(np.float32), 90)
    assert np.array_equal(a, b) and np.array_equal(da, db)
    lib = _lib.load()
    h = ctypes.c_void_p(lib.hmx_create())
    X32 = np.ascontiguousarray(Z, dtype=np.float32)
    bufs = [ctypes.c_void_p() for _ in range(5)]
    sizes = [X32.nbytes, 3000 * 90 * 4, 3000 * 90 * 4, 100 * 5 * 4, 100 * 5 * 4]
    try:
        for p, n in zip(bufs, sizes):
            assert hip.hipMalloc(ctypes.byref(p), n) == 0
        dX, oi, od, qi, qd = bufs
        assert hip.hipMemcpy(dX, X32.ctypes.data, X32.nbytes, 1) == 0
        assert lib.hmx_knn(h, dX, 1, 1, 3000, None, 0, 0, 0, 50, 90, oi, od, 1) == 0, lib.hmx_last_error(h)
        gi, gd = np.empty((3000, 90), np.int32), np.empty((3000, 90), np.float32)
        assert hip.hipMemcpy(gi.ctypes.data, oi, gi.nbytes, 2) == 0 and hip.hipMemcpy(gd.ctypes.data, od, gd.nbytes, 2) == 0
        assert np.array_equal(gi, a) and np.array_equal(gd, da)
        out = (ctypes.c_double * 1)()
        assert lib.hmx_get(h, b"timer:knn", out, 1) == 1 and out[0] > 0
        # separate-query form from the device (the first 100 rows of X, in place): self is then a neighbour at distance 0
        assert lib.hmx_knn(h, dX, 1, 1, 3000, dX, 1, 1, 100, 50, 5, qi, qd, 1) == 0, lib.hmx_last_error(h)
        si = np.empty((100, 5), np.int32)
        assert hip.hipMemcpy(si.ctypes.data, qi, si.nbytes, 2) == 0
        assert np.array_equal(si[:, 0], np.arange(100)) and np.array_equal(si[:, 1:], a[:100, :4])
    finally:
        lib.hmx_destroy(h)
        for p in bufs:
            if p.value:
                hip.hipFree(p)


# ---- 3. the LISI stage alone ---------------------------------------------------------------------------------------------------------------
def label_columns(N, cov0):
    return np.stack([np.unique(cov0, return_inverse=True)[1], np.random.default_rng(N).integers(0, 1000, N)]).astype(np.int32)


def relerr(a, b):
    return np.abs(a - b) / np.abs(b)


@pytest.mark.parametrize("N,d,k", SHAPES[:3])
def test_lisi_stage_on_the_specs_neighbours(N, d, k):
    _, cov0, ridx, rd2 = real_case(N, d)
    m, p = (89, 30) if k == 90 else (29, 10)
    idx = ridx[:, :m].astype(np.int32)
    dist = np.sqrt(rd2[:, :m]).astype(np.float32)
    lab = label_columns(N, cov0)
    idx = np.concatenate([idx, idx[:2]])
    dist = np.concatenate([dist, np.full((1, m), 1e15, np.float32), np.zeros((1, m), np.float32)])
    got = lisi_from_knn(idx, dist, lab, [4, 1000], p)
    want = mr.lisi_from_knn(idx, dist, lab, p)
    err = relerr(got, want)
    print("lisi stage N=%d m=%d: max rel err %.3e" % (N, m, err.max()))
    assert err.max() <= 1e-4
    assert (want[-2] == -1).all() and (got[-2] == -1).all()
    assert got.shape == (N + 2, 2) and np.isfinite(got).all()


def test_lisi_stage_small_perplexity():
    _, cov0, ridx, rd2 = real_case(2000, 20)
    lab = label_columns(2000, cov0)
    idx, dist = ridx[:, :3].astype(np.int32), np.sqrt(rd2[:, :3]).astype(np.float32)
    got = lisi_from_knn(idx, dist, lab, [4, 1000], 1.5)
    want = mr.lisi_from_knn(idx, dist, lab, 1.5)
    assert relerr(got, want).max() <= 1e-4


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------
def lisi_clear_rows(Z, ridx, rd2, m):
    X = mr.as_f32_f64(Z)
    n2 = (X * X).sum(axis=1)
    bar = (2 * Z.shape[1] + 4) * U * (n2 + n2[ridx[:, m - 1:m + 1]].max(axis=1))
    return (rd2[:, m] - rd2[:, m - 1]) > 2 * bar


def check_lisi(got, want, clear, n_levels):
    err = relerr(got[clear], want[clear])
    print("lisi end to end: %d rows, clear share %.4f, max rel err on clear rows %.3e" % (len(got), clear.mean(), err.max()))
    assert err.max() <= 1e-3
    assert np.isfinite(got).all()
    for c, nl in enumerate(n_levels):
        ok = (got[:, c] == -1) | ((got[:, c] >= 1 - 1e-9) & (got[:, c] <= nl + 1e-9))
        assert ok.all()


@pytest.mark.parametrize("N,d,k", SHAPES[:3])
def test_compute_lisi_end_to_end(N, d, k):
    Z, cov0, ridx, rd2 = real_case(N, d)
    lab = label_columns(N, cov0)
    meta = {"cov0": cov0, "rnd": lab[1]}
    got = compute_lisi(Z, meta, ["cov0", "rnd"], perplexity=30)
    want = mr.lisi_from_knn(ridx[:, :89], np.sqrt(rd2[:, :89]), np.stack([lab[0], np.unique(lab[1], return_inverse=True)[1]]), 30)
    check_lisi(got, want, lisi_clear_rows(Z, ridx, rd2, 89), [4, len(np.unique(lab[1]))])


# ---- 5. the point of the feature --------------------------------------------------------------------------------------------------------------
def test_harmony_raises_ilisi_and_keeps_clisi_on_the_cell_lines():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines.npz"))
    pcs = fx["pcs"].astype(np.float64)
    meta = {"dataset": fx["dataset_levels"][fx["dataset"]], "cell_type": fx["cell_type_levels"][fx["cell_type"]]}
    cols = ["dataset", "cell_type"]
    codes = np.stack([np.unique(meta[c], return_inverse=True)[1] for c in cols])
    nl = [len(np.unique(meta[c])) for c in cols]
    obj = RunHarmony(pcs, meta, "dataset", return_object=True, verbose=False, seed=1)
    Zc = obj.getZcorr().T

    def spec(Z):
        ridx, rd2 = mr.knn(Z, 89, extra=1)
        return mr.lisi_from_knn(ridx[:, :89], np.sqrt(rd2[:, :89]), codes, 30), lisi_clear_rows(Z, ridx, rd2, 89)

    s_raw, c_raw = spec(pcs)
    s_cor, c_cor = spec(Zc)
    assert np.median(s_cor[:, 0]) > np.median(s_raw[:, 0]) and np.median(s_cor[:, 1]) < 1.1      # the spec first: a failure here is the data's
    g_raw = compute_lisi(pcs, meta, cols, perplexity=30)
    g_cor = obj.lisi(meta, cols, perplexity=30)
    check_lisi(g_raw, s_raw, c_raw, nl)
    check_lisi(g_cor, s_cor, c_cor, nl)
    print("median iLISI %.3f -> %.3f, median cLISI %.3f -> %.3f" % (np.median(g_raw[:, 0]), np.median(g_cor[:, 0]), np.median(g_raw[:, 1]),
                                                                     np.median(g_cor[:, 1])))
    assert np.median(g_cor[:, 0]) > np.median(g_raw[:, 0])
    assert np.median(g_cor[:, 1]) < 1.1
    assert obj.timer("knn") > 0 and obj.timer("lisi") > 0
    assert np.array_equal(obj.lisi(meta, cols), g_cor)            # the handle is left as it was


# ---- 6. label transfer --------------------------------------------------------------------------------------------------------------------------
def test_knn_predict_on_the_mapped_jurkat_query():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines.npz"))
    ds = fx["dataset_levels"][fx["dataset"]]
    ct = fx["cell_type_levels"][fx["cell_type"]]
    ref = ds != "jurkat"
    skw, _ = prepare_setup_args(fx["pcs"][ref], {"dataset": ds[ref]}, "dataset", nclust=20)
    h = Harmony(seed=1)
    h.setup(**skw)
    h.init_cluster_cpp()
    harmonize(h, 10, verbose=False)
    Zref = h.getZcorr().T
    q = map_query(fx["pcs"][ds == "jurkat"], None, h.reference_summary(), return_object=True)
    Zq = q.getZcorr().T
    labels, share = knn_predict(Zq, Zref, ct[ref], k=5)
    ridx, rd2 = mr.knn(Zref, 5, Zq, extra=1)
    levels, codes = np.unique(ct[ref], return_inverse=True)
    win, rshare = mr.knn_predict(ridx[:, :5], codes, len(levels))
    Xf, Qf = mr.as_f32_f64(Zref), mr.as_f32_f64(Zq)
    n2x, n2q = (Xf * Xf).sum(axis=1), (Qf * Qf).sum(axis=1)
    clear = (rd2[:, 5] - rd2[:, 4]) > 2 * (2 * Zref.shape[1] + 4) * U * (n2q + n2x[ridx[:, 4:6]].max(axis=1))
    print("knn_predict: %d query cells, clear share %.4f, jurkat share %.3f" % (len(labels), clear.mean(), (labels == "jurkat").mean()))
    assert clear.mean() >= 0.95
    assert np.array_equal(labels[clear], levels[win][clear]) and np.array_equal(share[clear], rshare[clear])
    qs = q.lisi({"one": np.zeros(len(labels), int)}, "one", perplexity=10)      # a query handle scores its own Z_corr too
    assert np.allclose(qs, 1.0)
