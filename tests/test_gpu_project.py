"""Count projection on the MI355X: hmx_project_counts against the fp64 spec (tests/project_ref.py) within the derived bar on the shape sweep,
both value types, a clip that bites, caller-given totals; bit-identity across calls, residence of the matrix, cell order and slabs; the
kernel's guard against out-of-contract device-resident input; and counts -> project -> map_query -> knn_predict end to end.

Worst |gpu - spec| / bar seen over the sweep on an MI355X: see DESIGN "Projecting query counts"."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import map_query_ref as mq  # noqa: E402
import project_ref as pr  # noqa: E402
from harmony_amd import (Harmony, HarmonyError, HarmonyLoadings, knn_predict, map_query, map_query_counts, prepare_setup_args,  # noqa: E402
                         project_query)
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402
from harmony_amd.utils import harmonize  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (17, 70, 40, 3), (1000, 3000, 2000, 50), (333, 500, 500, 128), (257, 900, 300, 68)]      # (Nq, G_all, G, d)
ROWS = (0, 1, 63, 64, 65, 200)
UNKNOWN_ROW, ZERO_ROW = 6, 7


@functools.lru_cache(maxsize=None)
def case(shape, integer=True):
    """the synthetic query of a shape with the forced rows, its loadings and gene names; built once"""
    Nq, G_all, G, d = shape
    probe = pr.random_case(Nq, G_all, G, d, seed=sum(shape))
    unknown = np.nonzero(probe["slot"] < 0)[0]
    lens = (1,) if Nq == 1 else ROWS + (min(64, unknown.size), 5)
    c = pr.random_case(Nq, G_all, G, d, seed=sum(shape), row_lengths=lens, integer=integer)
    assert np.array_equal(c["slot"], probe["slot"])
    if Nq > ZERO_ROW:
        ip = c["indptr"]
        assert unknown.size > 0 and (c["slot"] >= 0).sum() < G       # query genes the reference lacks, reference genes the query lacks
        c["indices"][ip[UNKNOWN_ROW]:ip[UNKNOWN_ROW + 1]] = unknown[:ip[UNKNOWN_ROW + 1] - ip[UNKNOWN_ROW]]
        c["data"][ip[ZERO_ROW]:ip[ZERO_ROW + 1]] = 0.0
        assert list(np.diff(ip)[:6]) == [min(n, G_all) for n in ROWS]
        assert any(np.any(np.diff(c["indices"][ip[i]:ip[i + 1]]) < 0) for i in range(Nq))      # unsorted rows
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    genes = np.array(["r%d" % j if j >= 0 else "q%d" % g for g, j in enumerate(c["slot"])])
    return c, genes


def loadings(c, clip=None):
    return HarmonyLoadings(["r%d" % j for j in range(c["U"].shape[0])], c["U"], c["mean"], c["sd"], clip=clip)


def csr(c, dtype=np.float64):
    return (c["data"].astype(dtype), c["indices"], c["indptr"], (len(c["indptr"]) - 1, c["G_all"]))


@functools.lru_cache(maxsize=None)
def spec(shape, clip=None, integer=True):
    c, _ = case(shape, integer)
    return pr.project(clip=clip, **c), pr.bars(clip=clip, **c)


def worst(got, shape, clip=None, integer=True):
    P, bar = spec(shape, clip, integer)
    assert got.shape == P.shape and got.dtype == np.float32 and np.all(np.isfinite(got))
    r = float((np.abs(got.astype(np.float64) - P) / bar).max())
    print("project %s clip %s: worst |gpu - spec| / bar = %.3f" % (shape, clip, r))
    return r


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_spec_within_the_bar(shape, dtype):
    c, genes = case(shape)
    got = project_query(csr(c, dtype), genes, loadings(c))
    assert worst(got, shape) <= 1.0
    if shape[0] > ZERO_ROW:
        b = pr.offset(c["slot"], c["U"], c["mean"], c["sd"]).astype(np.float32)
        for row in (0, UNKNOWN_ROW, ZERO_ROW):                  # empty, only genes the reference lacks, stored zeros: the constant row
            assert np.array_equal(got[row], b), row


@pytest.mark.parametrize("shape", [(257, 900, 300, 68), (1000, 3000, 2000, 50)])
def test_clip_that_bites(shape):
    c, genes = case(shape)
    n = pr.clipped_entries(c["data"], c["indices"], c["indptr"], c["slot"], c["mean"], c["sd"], clip=10.0)
    assert n > 0, "no entry is clipped: the case does not test the clip"
    got = project_query(csr(c), genes, loadings(c, clip=10.0))
    assert worst(got, shape, clip=10.0) <= 1.0
    assert not np.array_equal(got, project_query(csr(c), genes, loadings(c)))


def test_non_integer_counts_and_given_totals():
    shape = (257, 900, 300, 68)
    c, genes = case(shape, integer=False)
    got = project_query(csr(c), genes, loadings(c))
    assert worst(got, shape, integer=False) <= 1.0
    tot = np.random.default_rng(4).uniform(100.0, 5000.0, shape[0])
    tot[3] = 0.0                                                # a caller's zero: y = 0
    got = project_query(csr(c), genes, loadings(c), totals=tot)
    P, bar = pr.project(totals=tot, **c), pr.bars(totals=tot, **c)
    r = float((np.abs(got.astype(np.float64) - P) / bar).max())
    print("project given totals: worst / bar = %.3f" % r)
    assert r <= 1.0
    assert np.array_equal(got[3], pr.offset(c["slot"], c["U"], c["mean"], c["sd"]).astype(np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bits_do_not_depend_on_residence_order_or_repetition(dtype):
    shape = (1000, 3000, 2000, 50)
    c, genes = case(shape)
    L = loadings(c)
    host = project_query(csr(c, dtype), genes, L)
    assert np.array_equal(host, project_query(csr(c, dtype), genes, L))
    dev = DeviceCSR(*csr(c, dtype))
    assert np.array_equal(host, project_query(dev, genes, L))
    (d, Nq, dt, ptr), owner = project_query(dev, genes, L, out="device")
    assert (d, Nq, dt, ptr) == (shape[3], shape[0], np.float32, owner.ptr)
    assert np.array_equal(host, owner.to_host(np.empty((Nq, d), dtype=np.float32)))
    perm = np.random.default_rng(2).permutation(shape[0])
    ip = c["indptr"]
    lens = np.diff(ip)[perm]
    pip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.concatenate([np.arange(ip[i], ip[i + 1]) for i in perm])
    out = project_query((c["data"][take].astype(dtype), c["indices"][take], pip, (shape[0], shape[1])), genes, L)
    assert np.array_equal(out, host[perm])


@pytest.mark.parametrize("shape,cap", [((17, 70, 40, 3), 600), ((257, 900, 300, 68), 2000)])
def test_slabs_give_the_one_slab_result(shape, cap):
    c, genes = case(shape)
    L = loadings(c)
    one = project_query(csr(c), genes, L)
    obj = Harmony()
    h = _ObjHandle(obj)
    assert np.array_equal(project_query(csr(c), genes, L, _handle=h), one) and obj._scalar("project_slabs") == 1
    obj._set("project_slab_bytes", cap)
    got = project_query(csr(c), genes, L, _handle=h)
    slabs = obj._scalar("project_slabs")
    assert slabs >= 3 and int(np.diff(c["indptr"]).max()) * 12 > cap      # several slabs, and a row longer than one
    assert np.array_equal(got, one)
    assert obj.timer("project") > 0


def test_guard_on_device_resident_input():
    """out-of-contract input in HBM cannot be validated on the host: the kernel must refuse the entry, raise the flag and end cleanly"""
    shape = (257, 900, 300, 68)
    c, genes = case(shape)
    L = loadings(c)
    good = project_query(csr(c), genes, L)
    data, indices, indptr, shp = csr(c)
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
            project_query(broken(name, where, value), genes, L)
        assert "status 1" in str(e.value), str(e.value)
        assert np.array_equal(project_query(DeviceCSR(data, indices, indptr, shp), genes, L), good)      # the process goes on, correctly
    with pytest.raises(HarmonyError, match="negative"):          # a host-resident matrix: the same flag
        bad = data.copy()
        bad[known] = -2.0
        project_query((bad, indices, indptr, shp), genes, L)


def planted(seed=11):
    """counts of a two-group reference and of a query with a batch shift, the reference's PCA in NumPy"""
    rng = np.random.default_rng(seed)
    G_all, Nr, Nq, d = 400, 1000, 300, 10
    base = rng.gamma(0.6, 1.0, G_all) + 0.02
    prof = np.stack([base, base.copy()])
    marker = rng.permutation(G_all)[:80]
    prof[0, marker[:40]] *= 6.0
    prof[1, marker[40:]] *= 6.0
    prof /= prof.sum(axis=1, keepdims=True)
    gr, gq = rng.integers(0, 2, Nr), rng.integers(0, 2, Nq)
    Xr = rng.poisson(prof[gr] * rng.uniform(600, 1500, Nr)[:, None]).astype(np.float64)
    shift = np.exp(rng.normal(0.0, 0.35, G_all))
    Xq = rng.poisson(prof[gq] * shift * rng.uniform(300, 900, Nq)[:, None]).astype(np.float64)
    Y = np.log1p(Xr * 1e4 / Xr.sum(axis=1, keepdims=True))
    var = np.argsort(-Y.var(axis=0))[:200]
    mean, sd = Y[:, var].mean(axis=0), Y[:, var].std(axis=0, ddof=1)
    S = (Y[:, var] - mean) / sd
    U = np.linalg.svd(S, full_matrices=False)[2][:d].T          # 200 x d loadings
    names = np.array(["gene%d" % g for g in range(G_all)])
    L = HarmonyLoadings(names[var], U, mean, sd)
    keep = np.setdiff1d(np.arange(G_all), var[::25])            # the query lacks 8 of the reference's genes ...
    order = rng.permutation(keep)                               # ... and names the others in its own order
    return dict(L=L, ref_pcs=S @ U, gr=gr, gq=gq, Xq=Xq[:, order], qgenes=names[order], batch=rng.integers(0, 2, Nr))


def test_counts_to_labels_end_to_end():
    sp = pytest.importorskip("scipy.sparse")
    p = planted()
    L, Xq, genes = p["L"], sp.csr_matrix(p["Xq"]), p["qgenes"]
    skw, _ = prepare_setup_args(p["ref_pcs"], {"batch": p["batch"]}, "batch", nclust=10)
    fit = Harmony(seed=1)
    fit.setup(**skw)
    fit.init_cluster_cpp()
    harmonize(fit, 5, verbose=False)
    ref = fit.reference_summary()
    slot = np.array([{g: j for j, g in enumerate(L.genes)}.get(g, -1) for g in genes], dtype=np.int32)
    assert (slot >= 0).sum() == L.G - 8 and (slot < 0).sum() > 0
    pcs = project_query(Xq, genes, L)
    P = pr.project(Xq.data, Xq.indices, Xq.indptr, Xq.shape[1], slot, L.loadings, L.mean, L.sd)
    bar = pr.bars(Xq.data, Xq.indices, Xq.indptr, Xq.shape[1], slot, L.loadings, L.mean, L.sd)
    assert (np.abs(pcs - P) / bar).max() <= 1.0
    assert np.array_equal(pcs, project_query(Xq.T.tocsr(), genes, L)) and np.array_equal(pcs, project_query(p["Xq"], genes, L))
    two = map_query(pcs, None, ref, return_object=True)
    one = map_query_counts(Xq, genes, None, ref, L, return_object=True)
    assert np.array_equal(one.getZcorr(), two.getZcorr()) and np.array_equal(one.getR(), two.getR())
    assert one.timer("project") > 0 and one.timer("map_query") > 0
    assert np.array_equal(map_query_counts(Xq, genes, None, ref, L), one.getZcorr().T)
    Zc, Rc = mq.map_query(P.T, [np.zeros(P.shape[0], int)], [1], ref.Nr, ref.C, ref.sigma)      # the spec's PCs through the spec's mapping
    Zg = one.getZcorr()
    assert np.linalg.norm(Zg - Zc) / np.linalg.norm(Zc) <= 1e-5 and np.abs(one.getR() - Rc).max() <= 1e-4
    ref_cells = fit.getZcorr().T
    lab_gpu, _ = knn_predict(Zg.T, ref_cells, p["gr"], k=5)
    lab_spec, _ = knn_predict(Zc.T, ref_cells, p["gr"], k=5)
    assert np.array_equal(lab_gpu, lab_spec)
    assert (lab_gpu == p["gq"]).mean() >= 0.95 and (lab_spec == p["gq"]).mean() >= 0.95
