"""The reference's PCA from raw counts on the MI355X: hmx_gene_stats and hmx_pca_prepare / apply / release against the fp64 spec (tests/pca_ref.py)
within the derived bars on the shape sweep; bit-identity across calls, residence of the matrix, slabs and (statistics) cell order; the kernels'
guard against out-of-contract device-resident input; fit_loadings on the planted cases; counts -> labels with nothing from outside.

The cases (pca_ref.sweep_case): N lies one below, at and one above the transposition's tile of 256 cells and spans four tiles at N = 1000; "every
cell stores" means every cell but the forced empty row and the forced row of unchosen genes.
Worst |gpu - spec| / bar seen over the sweep on an MI355X: see DESIGN "Fitting the loadings"."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pca_ref as pc  # noqa: E402
import project_ref as pr  # noqa: E402
from harmony_amd import (Harmony, HarmonyError, HarmonyLoadings, fit_loadings, gene_stats, knn_predict, map_query_counts,  # noqa: E402
                         prepare_setup_args, project_query)
from harmony_amd.pca import StandardisedMatrix  # noqa: E402
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402
from harmony_amd.utils import harmonize  # noqa: E402

pytestmark = pytest.mark.gpu

SLABBED = ((257, 900, 300, 68), 1500)      # a shape and a slab cap in bytes: several slabs, and the row of 200 entries (8 or 12 bytes each) longer than one


@functools.lru_cache(maxsize=None)
def case(shape, integer=True):
    return pc.sweep_case(shape, integer)[0]


def csr(c, dtype=np.float64):
    return (c["data"].astype(dtype), c["indices"], c["indptr"], (len(c["indptr"]) - 1, c["G_all"]))


def names(c):
    return ["g%d" % g for g in range(c["G_all"])]


def A(c):
    return c["data"], c["indices"], c["indptr"], c["G_all"]


def matrix(c, counts=None, clip=None, totals=None, handle=None):
    return StandardisedMatrix(csr(c) if counts is None else counts, c["G_all"], c["slot"], c["mean"], c["sd"], clip=clip, totals=totals, _handle=handle)


def slab_handle(cap):
    obj = Harmony()
    obj._set("project_slab_bytes", cap)
    return obj, _ObjHandle(obj)


def permuted(c, perm, dtype=np.float64):
    ip = c["indptr"]
    take = np.concatenate([np.arange(ip[i], ip[i + 1]) for i in perm] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    pip = np.concatenate([[0], np.cumsum(np.diff(ip)[perm])]).astype(np.int64)
    return (c["data"][take].astype(dtype), c["indices"][take], pip, (len(ip) - 1, c["G_all"]))


# ---- 1. gene statistics ----------------------------------------------------------------------------------------------------------------------
def stats_ratios(got, c, totals=None):
    st, b = pc.gene_stats(*A(c), totals=totals), pc.gene_stats_bars(*A(c), totals=totals)
    assert np.array_equal(got["n_cells"], st["n_cells"])
    q = pc.stat_steps(len(c["indptr"]) - 1, 1e4, totals is not None)
    assert tuple(got["step"]) == q
    has = b["s1"] > 0
    assert np.all(got["s1"][~has] == 0) and np.all(got["s2"][~has] == 0)
    r = {k: float((np.abs(got[k] - st[k])[has] / b[k][has]).max()) if has.any() else 0.0 for k in ("s1", "s2", "var")}
    assert np.array_equal(got["mean"], got["s1"] / (len(c["indptr"]) - 1))
    return r


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", pc.SHAPES)
def test_gene_stats_within_the_bars(shape, dtype):
    c = case(shape)
    r = stats_ratios(gene_stats(csr(c, dtype), names(c)), c)
    print("gene_stats %s %s: worst |gpu - spec| / bar = %s" % (shape, np.dtype(dtype).name, {k: round(v, 3) for k, v in r.items()}))
    assert all(v <= 1.0 for v in r.values()), r


def test_gene_stats_non_integer_counts_and_given_totals():
    shape = (257, 900, 300, 68)
    c = case(shape, integer=False)
    r = stats_ratios(gene_stats(csr(c), names(c)), c)
    tot = np.random.default_rng(4).uniform(100.0, 5000.0, shape[0])
    tot[3] = 0.0                                                # a caller's zero: y = 0
    rt = stats_ratios(gene_stats(csr(c), names(c), totals=tot), c, totals=tot)
    print("gene_stats non-integer counts: %s; given totals: %s" % (r, rt))
    assert all(v <= 1.0 for v in r.values()) and all(v <= 1.0 for v in rt.values())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gene_stats_bits_do_not_depend_on_residence_slabs_order_or_repetition(dtype):
    shape, cap = SLABBED
    c = case(shape)
    one = gene_stats(csr(c, dtype), names(c))
    same = lambda g: all(np.array_equal(g[k], one[k]) for k in ("n_cells", "s1", "s2", "mean", "var"))
    assert same(gene_stats(csr(c, dtype), names(c)))
    assert same(gene_stats(DeviceCSR(*csr(c, dtype)), names(c)))
    obj, h = slab_handle(cap)
    assert same(gene_stats(csr(c, dtype), names(c), _handle=h))
    assert obj._scalar("project_slabs") >= 3 and int(np.diff(c["indptr"]).max()) * (4 + np.dtype(dtype).itemsize) > cap and obj.timer("gene_stats") > 0
    perm = np.random.default_rng(2).permutation(shape[0])
    assert same(gene_stats(permuted(c, perm, dtype), names(c)))


# ---- 2. the operator -------------------------------------------------------------------------------------------------------------------------
def apply_ratios(c, P, W, V, clip=None, totals=None):
    """worst |gpu - spec| / bar of P, and of W against the spec applied to the device's own P"""
    kw = dict(clip=clip, totals=totals)
    S = pc.dense_S(*A(c), c["slot"], c["mean"], c["sd"], **kw)
    assert P.dtype == np.float32 and W.dtype == np.float64 and np.all(np.isfinite(P)) and np.all(np.isfinite(W))
    bP = pr.bars(*A(c), c["slot"], V, c["mean"], c["sd"], **kw)
    rP = float((np.abs(P - S @ V) / bP).max())
    bW = pc.bars_W(*A(c), c["slot"], c["mean"], c["sd"], P, **kw)
    err = np.abs(W - pc.apply(S, V, P=P)[1])
    assert np.all(err[bW == 0] == 0)
    return rP, float((err[bW > 0] / bW[bW > 0]).max())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", pc.SHAPES)
def test_apply_within_the_bars(shape, dtype):
    c, special = pc.sweep_case(shape)
    V = c["U"]
    with matrix(c, counts=csr(c, dtype)) as S:
        assert S.entries == int((c["slot"][c["indices"]] >= 0).sum())
        W, P = S.apply(V, P="host")
        W2, P2 = S.apply(V, P="host")                            # the prepared state serves again, to the same bits
        assert np.array_equal(W, W2) and np.array_equal(P, P2)
        assert np.array_equal(S.apply(V)[0], W)                  # ... and whether or not P is returned
    rP, rW = apply_ratios(c, P, W, V)
    print("pca apply %s %s: worst |gpu - spec| / bar: P %.3f, W %.3f" % (shape, np.dtype(dtype).name, rP, rW))
    assert rP <= 1.0 and rW <= 1.0
    if special:
        j = c["slot"][special["none"]]                           # the gene no cell stores: the centring alone, exactly
        assert np.array_equal(W[j], -(c["mean"][j] / c["sd"][j]) * pc.colsum_fixed(P))
        b = pr.offset(c["slot"], V, c["mean"], c["sd"]).astype(np.float32)
        for row in (0, pc.UNKNOWN_ROW, pc.ZERO_ROW):             # empty, only unchosen genes, stored zeros: the constant row
            assert np.array_equal(P[row], b), row


@pytest.mark.parametrize("shape", [(257, 900, 300, 68), (1000, 3000, 2000, 60)])
def test_apply_with_a_clip_that_bites(shape):
    c = case(shape)
    assert pr.clipped_entries(c["data"], c["indices"], c["indptr"], c["slot"], c["mean"], c["sd"], clip=3.0) > 0, "no entry is clipped"
    with matrix(c, clip=3.0) as S:
        W, P = S.apply(c["U"], P="host")
    with matrix(c) as S:
        W0 = S.apply(c["U"])[0]
    rP, rW = apply_ratios(c, P, W, c["U"], clip=3.0)
    print("pca apply %s clip 3: worst / bar: P %.3f, W %.3f" % (shape, rP, rW))
    assert rP <= 1.0 and rW <= 1.0 and not np.array_equal(W, W0)


def test_apply_with_given_totals_and_non_integer_counts():
    shape = (257, 900, 300, 68)
    c = case(shape, integer=False)
    tot = np.random.default_rng(4).uniform(100.0, 5000.0, shape[0])
    tot[3] = 0.0
    with matrix(c, totals=tot) as S:
        W, P = S.apply(c["U"], P="host")
    rP, rW = apply_ratios(c, P, W, c["U"], totals=tot)
    print("pca apply given totals: worst / bar: P %.3f, W %.3f" % (rP, rW))
    assert rP <= 1.0 and rW <= 1.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_apply_bits_do_not_depend_on_residence_slabs_or_repetition(dtype):
    shape, cap = SLABBED
    c = case(shape)
    V = c["U"]
    with matrix(c, counts=csr(c, dtype)) as S:
        W, P = S.apply(V, P="host")
    with matrix(c, counts=csr(c, dtype)) as S:
        W1, P1 = S.apply(V, P="host")
    assert np.array_equal(W, W1) and np.array_equal(P, P1)
    with matrix(c, counts=DeviceCSR(*csr(c, dtype))) as S:
        W1, (buf, owner) = S.apply(V, P="device")
        assert buf == (shape[3], shape[0], np.float32, owner.ptr)
        assert np.array_equal(W, W1) and np.array_equal(P, owner.to_host(np.empty_like(P)))
    obj, h = slab_handle(cap)
    with matrix(c, counts=csr(c, dtype), handle=h) as S:
        assert obj._scalar("project_slabs") >= 3 and int(np.diff(c["indptr"]).max()) * (4 + np.dtype(dtype).itemsize) > cap
        W1, P1 = S.apply(V, P="host")
        assert obj.timer("pca_prepare") > 0 and obj.timer("pca_apply") > 0 and obj._scalar("pca_entries") == S.entries
    assert np.array_equal(W, W1) and np.array_equal(P, P1)
    assert obj._scalar("pca_entries") == 0                       # the matrix left nothing behind


def test_apply_needs_a_prepared_matrix():
    c = case((17, 70, 40, 3))
    obj = Harmony()
    h = _ObjHandle(obj)
    W = np.empty((40, 3))
    dp = W.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert obj._lib.hmx_pca_apply(obj._h, dp, 3, dp, None, 0) == 6 and b"hmx_pca_prepare first" in obj._lib.hmx_last_error(obj._h)
    S = matrix(c, handle=h)
    good = S.apply(c["U"])[0]
    S2 = matrix(c, handle=h)                                     # a second prepare replaces the first
    assert np.array_equal(S2.apply(c["U"])[0], good)
    S2.release()
    with pytest.raises(HarmonyError, match="status 6"):
        S2.apply(c["U"])
    S.close()
    S2.close()
    with pytest.raises(ValueError, match="closed"):
        S.apply(c["U"])


# ---- 3. guards ---------------------------------------------------------------------------------------------------------------------------------
def test_guard_on_device_resident_input():
    """out-of-contract input in HBM cannot be validated on the host: the kernels must refuse the entry, raise the flag and end cleanly"""
    shape = (257, 900, 300, 68)
    c = case(shape)
    data, indices, indptr, shp = csr(c)
    good_stats = gene_stats(csr(c), names(c))
    with matrix(c) as S:
        good_W = S.apply(c["U"])[0]
    at = int(indptr[5]) + 3
    known = int(np.nonzero(c["slot"][indices] >= 0)[0][10])

    def broken(name, where, value):
        a = dict(data=data.copy(), indices=indices.copy(), indptr=indptr.copy())
        a[name][where] = value
        return DeviceCSR(a["data"], a["indices"], a["indptr"], shp)

    for name, where, value, text in (("indices", at, shape[1], "column index"), ("indices", at, -1, "column index"),
                                     ("indices", at, 2 ** 30, "column index"), ("data", known, -1.0, "negative"),
                                     ("data", known, np.nan, "not finite"), ("data", known, np.inf, "not finite"),
                                     ("indptr", 9, int(indptr[-1]) + 1000, "indptr")):
        with pytest.raises(HarmonyError, match=text) as e:
            gene_stats(broken(name, where, value), names(c))
        assert "status 1" in str(e.value), str(e.value)
        with pytest.raises(HarmonyError, match=text) as e:
            matrix(c, counts=broken(name, where, value))
        assert "status 1" in str(e.value), str(e.value)
        dev = DeviceCSR(data, indices, indptr, shp)              # the process goes on, correctly
        again = gene_stats(dev, names(c))
        assert all(np.array_equal(again[k], good_stats[k]) for k in ("n_cells", "s1", "s2"))
        with matrix(c, counts=dev) as S:
            assert np.array_equal(S.apply(c["U"])[0], good_W)
    bad = data.copy()
    bad[known] = -2.0
    with pytest.raises(HarmonyError, match="negative"):          # a host-resident matrix: the same flag
        gene_stats((bad, indices, indptr, shp), names(c))
    with pytest.raises(HarmonyError, match="negative"):
        matrix(c, counts=(bad, indices, indptr, shp))


# ---- 4. fit_loadings ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(groups):
    X, lab, Xq, labq = pc.planted_counts(groups, Nq=300)
    nz = X != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    a = (X[nz], np.nonzero(nz)[1].astype(np.int32), indptr, X.shape[1])
    st = pc.gene_stats(*a)
    chosen = pc.top_variance(st["var"], st["n_cells"], 200)
    slot = np.full(X.shape[1], -1, dtype=np.int32)
    slot[chosen] = np.arange(chosen.size)
    mean, sd = st["mean"][chosen], np.sqrt(st["var"][chosen])
    genes = np.array(["gene%d" % g for g in range(X.shape[1])])
    return dict(X=X, lab=lab, Xq=Xq, labq=labq, A=a, chosen=chosen, slot=slot, mean=mean, sd=sd, genes=genes,
                bars=pc.fit_bars(*a, slot, mean, sd, groups - 1))


@pytest.mark.parametrize("groups", [2, 4, 6])
def test_fit_loadings_on_planted_groups(groups):
    p = planted(groups)
    d, fb, X, genes = groups - 1, p["bars"], p["X"], p["genes"]
    lam = fb["lam"]
    L, pcs, ev = fit_loadings(X, genes, n_top_genes=200, d=d)
    assert list(L.genes) == list(genes[p["chosen"]])             # the spec's top-variance set, in its order
    np.testing.assert_allclose(L.mean, p["mean"], rtol=1e-6)
    np.testing.assert_allclose(L.sd, p["sd"], rtol=1e-6)
    s = pc.sin_theta_max(L.loadings, fb["E"])
    ev_bar = fb["bar_sin"] ** 2 + fb["eta"] / lam[0]
    ev_r = float((np.abs(ev - lam[:d]) / lam[0]).max() / ev_bar)
    print("fit_loadings, %d planted groups: sin / bar_sin = %.4f (sin %.1e), explained variance / bar = %.4f" % (groups, s / fb["bar_sin"], s, ev_r))
    assert s <= fb["bar_sin"] and ev_r <= 1.0
    top = np.abs(L.loadings).argmax(axis=0)
    assert np.all(L.loadings[top, np.arange(d)] > 0)             # the sign convention
    assert pcs.shape == (X.shape[0], d) and pcs.dtype == np.float32
    assert np.array_equal(pcs, project_query(X, genes, L))       # one arithmetic for the reference and the query
    L2, (buf, owner), ev2 = fit_loadings(X, genes, genes_use=list(L.genes), d=d, out="device")
    assert buf == (d, X.shape[0], np.float32, owner.ptr)
    assert np.array_equal(L2.loadings, L.loadings) and np.array_equal(ev2, ev)      # two fits with one seed; the genes named or chosen
    assert np.array_equal(owner.to_host(np.empty_like(pcs)), pcs)
    (_, _, _, ptr), own2 = project_query(X, genes, L, out="device")
    assert np.array_equal(own2.to_host(np.empty_like(pcs)), pcs)


# ---- 5. counts -> labels with nothing from outside ----------------------------------------------------------------------------------------------
def test_counts_to_labels_with_fitted_loadings():
    groups, d = 4, 3
    p = planted(groups)
    X, genes, Xq = p["X"], p["genes"], p["Xq"]
    rng = np.random.default_rng(5)
    batch = rng.integers(0, 2, X.shape[0])
    keep = np.setdiff1d(np.arange(X.shape[1]), p["chosen"][::25])      # the query lacks 8 of the reference's genes ...
    order = rng.permutation(keep)                                       # ... and names the others in its own order
    Xq, qgenes = Xq[:, order], genes[order]
    L_gpu, pcs_gpu, _ = fit_loadings(X, genes, n_top_genes=200, d=d)
    L_spec = HarmonyLoadings(genes[p["chosen"]], p["bars"]["U_spec"], p["mean"], p["sd"])
    pcs_spec = pc.dense_S(*p["A"], p["slot"], p["mean"], p["sd"]) @ p["bars"]["U_spec"]

    def labels(L, pcs):
        skw, _ = prepare_setup_args(pcs, {"batch": batch}, "batch", nclust=10)
        fit = Harmony(seed=1)
        fit.setup(**skw)
        fit.init_cluster_cpp()
        harmonize(fit, 5, verbose=False)
        Z = map_query_counts(Xq, qgenes, None, fit.reference_summary(), L)
        return knn_predict(Z, fit.getZcorr().T, p["lab"], k=5)[0]

    lab_gpu, lab_spec = labels(L_gpu, pcs_gpu), labels(L_spec, pcs_spec)
    assert np.array_equal(lab_gpu, lab_spec)
    assert (lab_gpu == p["labq"]).mean() >= 0.95 and (lab_spec == p["labq"]).mean() >= 0.95
