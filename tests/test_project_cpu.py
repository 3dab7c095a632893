"""Count projection without a GPU: the fp64 spec (tests/project_ref.py) against a plain NumPy normalise / scale / matmul, the sparse identity
the kernel uses against the dense form, honest fp32 against the error bar, HarmonyLoadings and its saved format, gene matching and orientation
of project_query's input, the C ABI of include/harmony_mi355x_project.h against the library and harmony_amd/_lib.py, and every check the entry
point makes before the device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import project_ref as pr  # noqa: E402
import harmony_amd  # noqa: E402
from harmony_amd import HarmonyError, HarmonyLoadings, _lib, project, project_query  # noqa: E402

HMX_ERR_ARG, HMX_ERR_DEVICE, HMX_ERR_LIMIT = 1, 5, 7
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
ROWS = (0, 1, 63, 64, 65, 200)
# (Nq, G_all, G, d, clip, integer counts, shared genes): the GPU test's shapes at CPU-sized cell counts, plus a clip, non-integer counts, one shared gene
FP32_CASES = [(1, 1, 1, 1, None, True, None), (17, 70, 40, 3, None, True, None), (60, 3000, 2000, 50, None, True, None),
              (40, 500, 500, 128, 10.0, True, None), (40, 900, 300, 68, 2.0, False, None), (20, 200, 50, 7, None, False, 1)]


def test_status_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "harmony_mi355x.h")).read()
    for name, v in (("HMX_ERR_ARG", HMX_ERR_ARG), ("HMX_ERR_DEVICE", HMX_ERR_DEVICE), ("HMX_ERR_LIMIT", HMX_ERR_LIMIT)):
        assert re.search(r"\b%s\s*=?\s*%d\b" % (name, v), hdr), name


@pytest.mark.parametrize("clip", [None, 1.5])
def test_spec_equals_plain_numpy_on_a_dense_matrix(clip):
    """every reference gene present, identity gene map: the textbook pipeline"""
    rng = np.random.default_rng(3)
    Nq, G, d = 30, 25, 4
    X = rng.poisson(0.6, size=(Nq, G)).astype(np.float64)
    X[5] = 0                                                     # an empty cell
    U, mean, sd = rng.standard_normal((G, d)), rng.uniform(0, 1, G), rng.uniform(0.3, 2, G)
    T = X.sum(axis=1, keepdims=True)
    Y = np.log1p(np.divide(X * 1e4, T, out=np.zeros_like(X), where=T > 0))
    S = (Y - mean) / sd
    if clip is not None:
        S = np.clip(S, None, clip)
        assert (S == clip).any()
    nz = X != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    indices = np.nonzero(nz)[1].astype(np.int32)
    P = pr.project(X[nz], indices, indptr, G, np.arange(G, dtype=np.int32), U, mean, sd, clip=clip)
    np.testing.assert_allclose(P, S @ U, rtol=1e-12, atol=1e-12)
    assert np.allclose(P[5], (-mean / sd) @ U)


@pytest.mark.parametrize("clip,totals", [(None, False), (1.0, False), (None, True), (3.0, True)])
def test_sparse_identity_equals_the_dense_form(clip, totals):
    c = pr.random_case(50, 300, 120, 9, seed=5, row_lengths=ROWS, integer=False)
    c["indices"][c["indptr"][3]:c["indptr"][4]] = np.nonzero(c["slot"] < 0)[0][:64]      # a row whose genes the reference does not know
    tot = np.random.default_rng(1).uniform(50, 500, 50) if totals else None
    a = pr.project(clip=clip, totals=tot, **c)
    b = pr.project_sparse(clip=clip, totals=tot, **c)
    assert np.abs(a - b).max() <= 1e-12
    assert np.abs(b[3] - pr.offset(c["slot"], c["U"], c["mean"], c["sd"])).max() <= 1e-13 and np.abs(b[0] - b[3]).max() <= 1e-13
    if clip is not None:
        assert pr.clipped_entries(clip=clip, totals=tot, **{k: c[k] for k in ("data", "indices", "indptr", "slot", "mean", "sd")}) > 0


@pytest.mark.parametrize("Nq,G_all,G,d,clip,integer,shared", FP32_CASES)
def test_honest_fp32_stays_inside_the_bar(Nq, G_all, G, d, clip, integer, shared):
    """the bar is sound: a sequential float32 evaluation of the sparse form stays inside it -- and it is not vacuous"""
    c = pr.random_case(Nq, G_all, G, d, seed=Nq + d, row_lengths=ROWS, integer=integer, shared=shared)
    spec = pr.project(clip=clip, **c)
    bar = pr.bars(clip=clip, **c)
    got = pr.project_fp32(clip=clip, **c).astype(np.float64)
    ratio = np.abs(got - spec) / bar
    print("fp32 / bar:", ratio.max())
    assert ratio.max() <= 1.0, ratio.max()
    if G >= 40:
        big = np.abs(spec) >= 0.1 * np.abs(spec).max()
        assert (bar[big] / np.abs(spec[big])).min() <= 1e-3                     # tight where the entries are not cancelling sums


def _loadings(G=6, d=3, **kw):
    rng = np.random.default_rng(0)
    return HarmonyLoadings(["g%d" % j for j in range(G)], rng.standard_normal((G, d)), rng.uniform(0, 1, G), rng.uniform(0.5, 1, G), **kw)


def test_loadings_validate_and_round_trip(tmp_path):
    L = _loadings(clip=10.0, scale=1e4)
    assert (L.G, L.d) == (6, 3)
    p = str(tmp_path / "loadings.npz")
    L.save(p)
    with np.load(p, allow_pickle=False) as z:
        assert str(z["format"]) == "harmony_amd.loadings/1" and z["genes"].dtype.kind == "U"
    M = HarmonyLoadings.load(p)
    assert list(M.genes) == list(L.genes) and M.clip == 10.0 and M.scale == 1e4
    for a, b in ((M.loadings, L.loadings), (M.mean, L.mean), (M.sd, L.sd)):
        assert np.array_equal(a, b)
    _loadings().save(p)
    assert HarmonyLoadings.load(p).clip is None
    np.savez(p, format=np.array("something/else"), genes=L.genes)
    with pytest.raises(ValueError, match="not a saved HarmonyLoadings"):
        HarmonyLoadings.load(p)
    g, U, m, s = L.genes, L.loadings, L.mean, L.sd
    bad_sd, neg_sd, neg_mean = s.copy(), s.copy(), m.copy()
    bad_sd[2], neg_sd[0], neg_mean[1] = 0.0, np.nan, -0.1
    for args, kw in (((g[:5], U, m, s), {}), ((g, U[:, 0], m, s), {}), ((g, U, m[:5], s), {}), ((g, U, m, bad_sd), {}), ((g, U, m, neg_sd), {}),
                     ((g, U, neg_mean, s), {}), ((["a"] * 6, U, m, s), {}), ((g, U, m, s), dict(scale=0.0)), ((g, U, m, s), dict(clip=0.0)),
                     ((g, U, m, s), dict(clip=-1.0))):
        with pytest.raises(ValueError):
            HarmonyLoadings(*args, **kw)


def test_genes_are_matched_by_name():
    L = _loadings()
    slot = project.gene_slots(["x", "g4", "g0", "y", "g5"], L)
    assert slot.dtype == np.int32 and list(slot) == [-1, 4, 0, -1, 5]            # extra query genes, permuted order, g1..g3 absent
    with pytest.raises(ValueError, match="twice"):
        project.gene_slots(["g1", "g1"], L)


def _capture(monkeypatch):
    """project_query up to the library call: the arguments it would pass"""
    seen = {}

    class FakeLib(object):
        def hmx_project_counts(self, h, Nq, G_all, indptr, indices, data, dtype, loc, slot, U, mean, sd, G, d, scale, clip, totals, out, oloc):
            n = Nq + 1
            ip = np.ctypeslib.as_array(C.cast(indptr, C.POINTER(C.c_int64)), (n,)).copy()
            nnz = int(ip[-1])
            seen.update(Nq=Nq, G_all=G_all, indptr=ip, dtype=dtype, loc=loc, G=G, d=d, scale=scale, clip=clip, oloc=oloc, totals=totals,
                        indices=np.ctypeslib.as_array(C.cast(indices, C.POINTER(C.c_int32)), (max(nnz, 1),))[:nnz].copy(),
                        data=np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_float if dtype else C.c_double)), (max(nnz, 1),))[:nnz].copy(),
                        slot=np.ctypeslib.as_array(slot, (G_all,)).copy())
            return 0

    class FakeHandle(object):
        lib, h = FakeLib(), None

        def check(self, st, what):
            assert st == 0
    return seen, FakeHandle()


def test_input_forms_and_orientation(monkeypatch):
    sp = pytest.importorskip("scipy.sparse")
    L = _loadings()
    genes = ["g2", "q", "g0", "g5"]
    X = np.array([[0, 2, 1, 0], [3, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 5, 0]], dtype=np.float64)      # 5 cells x 4 genes
    seen, h = _capture(monkeypatch)
    want = sp.csr_matrix(X)
    forms = {"csr": sp.csr_matrix(X), "csc": sp.csc_matrix(X), "coo": sp.coo_matrix(X), "genes x cells csc": sp.csc_matrix(X.T),
             "genes x cells csr": sp.csr_matrix(X.T), "dense": X, "dense genes x cells": X.T, "float32 dense": X.astype(np.float32),
             "tuple": (want.data, want.indices, want.indptr, want.shape)}
    for name, form in forms.items():
        seen.clear()
        out = project_query(form, genes, L, _handle=h)
        assert out.shape == (5, 3) and out.dtype == np.float32, name
        assert seen["Nq"] == 5 and seen["G_all"] == 4 and seen["loc"] == 0 and seen["oloc"] == 0, name
        assert np.array_equal(seen["indptr"], want.indptr) and list(seen["slot"]) == [2, -1, 0, 5], name
        got = sp.csr_matrix((seen["data"], seen["indices"], seen["indptr"]), shape=(5, 4)).toarray()
        assert np.array_equal(got, X), name
        assert seen["dtype"] == (1 if name == "float32 dense" else 0), name
        assert seen["clip"] == 0.0 and seen["scale"] == 1e4 and not seen["totals"], name
    Tt = sp.csc_matrix(X.T)
    seen.clear()
    project_query(Tt, genes, L, _handle=h)                       # the transposed CSC is handed over as it is: same arrays, no copy
    assert np.shares_memory(Tt.T.data, Tt.data) and np.array_equal(seen["data"], Tt.data)
    dup = sp.coo_matrix((np.array([1.0, 2.0]), (np.array([0, 0]), np.array([1, 1]))), shape=(5, 4))
    seen.clear()
    project_query(dup, genes, L, _handle=h)
    assert list(seen["data"]) == [3.0]                           # duplicates are summed
    seen.clear()
    project_query(X, genes, _loadings(clip=7.0, scale=1e3), totals=np.arange(5.0), _handle=h)
    assert seen["clip"] == 7.0 and seen["scale"] == 1e3 and seen["totals"]


def test_python_errors_come_before_the_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    L = _loadings()
    X = np.ones((5, 4))
    genes = ["g2", "q", "g0", "g5"]
    with pytest.raises(ValueError, match="HarmonyLoadings"):
        project_query(X, genes, None)
    with pytest.raises(ValueError, match="shares no gene"):
        project_query(X, ["a", "b", "c", "d"], L)
    with pytest.raises(ValueError, match="genes were named"):
        project_query(X, genes[:3], L)
    with pytest.raises(ValueError, match="out must be"):
        project_query(X, genes, L, out="gpu")
    with pytest.raises(ValueError, match="totals"):
        project_query(X, genes, L, totals=np.ones(4))
    with pytest.raises(ValueError, match="totals"):
        project_query(X, genes, L, totals=-np.ones(5))
    with pytest.raises(ValueError, match="twice"):
        project_query(X, ["g2", "g2", "g0", "g5"], L)
    with pytest.raises(ValueError, match="indptr"):
        project_query((np.ones(2), np.array([0, 1]), np.array([0, 1, 2]), (5, 4)), genes, L)
    with pytest.raises(ValueError, match="cells x genes"):
        project_query((np.ones(2), np.array([0, 1]), np.array([0, 1, 1, 1, 2]), (4, 5)), genes, L)
    with pytest.raises(ValueError, match="2-D"):
        project_query(np.ones(4), genes, L)
    for name in ("HarmonyLoadings", "project_query", "map_query_counts"):
        assert name in harmony_amd.__all__ and hasattr(harmony_amd, name)


def test_module_imports_without_scipy():
    import subprocess
    code = ("import sys; sys.modules['scipy'] = None; sys.modules['scipy.sparse'] = None\n"
            "import harmony_amd.project as p, numpy as np\n"
            "L = p.HarmonyLoadings(['a', 'b'], np.eye(2), [0.1, 0.2], [1.0, 1.0])\n"
            "d, i, ip, n, dev = p._as_csr(np.array([[0.0, 2.0], [1.0, 0.0]]), 2)\n"
            "assert list(i) == [1, 0] and list(ip) == [0, 1, 2] and not dev\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_project_header_matches_the_library_and_the_binding():
    assert helpers.header_names("harmony_mi355x_project.h") == set(_lib.PROJECT_SIGNATURES) == {"hmx_project_counts"}
    found = helpers.header_functions("harmony_mi355x_project.h")
    assert [n for n, _ in found] == ["hmx_project_counts"] and len(found[0][1]) == 19
    helpers.assert_header_stands_alone("harmony_mi355x_project.h", ["hmx_project_counts"])
    loose = {"const int32_t*": (C.POINTER(C.c_int32), C.c_void_p), "const int64_t*": (C.c_void_p,)}      # (the count matrix: host or device pointers)
    helpers.assert_binding_matches(_lib.load(), "hmx_project_counts", found[0][1], _lib.PROJECT_SIGNATURES["hmx_project_counts"][1], loose)


def _call_factory(lib, h):
    c = pr.random_case(6, 12, 8, 3, seed=2, row_lengths=(0, 1, 5))
    base = dict(Nq=6, G_all=12, indptr=c["indptr"], indices=c["indices"], data=c["data"], dtype=0, loc=0, slot=c["slot"], U=c["U"].copy(),
                mean=c["mean"].copy(), sd=c["sd"].copy(), G=8, d=3, scale=1e4, clip=0.0, totals=None, out=np.zeros((6, 3), dtype=np.float32), oloc=0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    V = lambda v: None if v is None else C.c_void_p(v.ctypes.data)  # noqa: E731
    D = lambda v: None if v is None else v.ctypes.data_as(dp)  # noqa: E731

    def call(handle=h, **kw):
        a = dict(base)
        a.update(kw)
        return lib.hmx_project_counts(handle, a["Nq"], a["G_all"], V(a["indptr"]), V(a["indices"]), V(a["data"]), a["dtype"], a["loc"],
                                      None if a["slot"] is None else a["slot"].ctypes.data_as(ip), D(a["U"]), D(a["mean"]), D(a["sd"]), a["G"], a["d"],
                                      a["scale"], a["clip"], D(a["totals"]), V(a["out"]), a["oloc"])
    return call, base


def test_library_checks_the_arguments_before_the_device():
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    call, base = _call_factory(lib, h)

    def refused(status, match=None, **kw):
        assert call(**kw) == status, kw
        msg = lib.hmx_last_error(h).decode()
        assert msg and (match is None or match in msg), (kw, msg)

    def changed(name, at, v):
        a = base[name].copy()
        a[at] = v
        return {name: a}

    two = base["slot"].copy()
    j = np.nonzero(two >= 0)[0]
    two[j[1]] = two[j[0]]
    free = np.nonzero(base["slot"] < 0)[0]
    try:
        for name in ("indptr", "indices", "data", "slot", "U", "mean", "sd", "out"):
            refused(HMX_ERR_ARG, **{name: None})
        refused(HMX_ERR_ARG, Nq=0)
        refused(HMX_ERR_ARG, G_all=0)
        refused(HMX_ERR_ARG, G=0)
        refused(HMX_ERR_ARG, d=0)
        refused(HMX_ERR_ARG, dtype=2)
        refused(HMX_ERR_ARG, loc=2)
        refused(HMX_ERR_ARG, oloc=-1)
        refused(HMX_ERR_ARG, "scale", scale=0.0)
        refused(HMX_ERR_ARG, "scale", scale=float("nan"))
        refused(HMX_ERR_ARG, "clip", clip=float("nan"))
        refused(HMX_ERR_ARG, "sd", **changed("sd", 3, 0.0))
        refused(HMX_ERR_ARG, "sd", **changed("sd", 0, float("inf")))
        refused(HMX_ERR_ARG, "mean", **changed("mean", 7, -1e-9))
        refused(HMX_ERR_ARG, "loadings", **changed("U", (2, 1), float("nan")))
        refused(HMX_ERR_ARG, "slot", **changed("slot", free[0], 8))
        refused(HMX_ERR_ARG, "slot", **changed("slot", free[0], -2))
        refused(HMX_ERR_ARG, "two query genes", slot=two)
        refused(HMX_ERR_ARG, "totals", totals=np.array([1.0, 2.0, -1.0, 1.0, 1.0, 1.0]))
        refused(HMX_ERR_ARG, "indptr", **changed("indptr", 0, 1))
        refused(HMX_ERR_ARG, "indptr", **changed("indptr", 3, 0))
        refused(HMX_ERR_ARG, "column", **changed("indices", 3, 12))
        refused(HMX_ERR_ARG, "column", **changed("indices", 0, -1))
        refused(HMX_ERR_LIMIT, d=129)
        refused(HMX_ERR_LIMIT, G=(1 << 24) + 1)
        refused(HMX_ERR_LIMIT, G_all=(1 << 24) + 1)
        assert lib.hmx_set_int(h, b"project_slab_bytes", -1) != 0 and lib.hmx_set_int(h, b"project_slab_bytes", 4096) == 0
        if NO_GPU:                                              # valid calls get as far as the device
            refused(HMX_ERR_DEVICE)
            refused(HMX_ERR_DEVICE, dtype=1, data=base["data"].astype(np.float32), clip=10.0, totals=np.ones(6))
        out = (C.c_double * 1)()
        assert lib.hmx_get(h, b"timer:project", out, 1) == 1 and (out[0] == 0.0 or not NO_GPU)
    finally:
        lib.hmx_destroy(h)
    assert call(handle=None) == HMX_ERR_ARG


def test_xfer_slab_bytes_is_a_lab_field_with_the_same_conventions():
    """the cap on a staging slab of the host matrix seam (hmx_setup / hmx_map_query / hmx_get_matrix with host buffers): 0 is the default"""
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    try:
        assert lib.hmx_set_int(h, b"xfer_slab_bytes", -1) == HMX_ERR_ARG
        assert b"xfer_slab_bytes" in lib.hmx_last_error(h)
        assert lib.hmx_set_int(h, b"xfer_slab_bytes", 4096) == 0 and lib.hmx_set_int(h, b"xfer_slab_bytes", 0) == 0
    finally:
        lib.hmx_destroy(h)
    lab = open(os.path.join(ROOT, "include", "harmony_mi355x_lab.h")).read()
    assert '"xfer_slab_bytes"' in lab


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_no_cpu_fallback():
    c = pr.random_case(6, 12, 8, 3, seed=2)
    L = HarmonyLoadings(["r%d" % j for j in range(8)], c["U"], c["mean"], c["sd"])
    genes = ["r%d" % j if j >= 0 else "q%d" % g for g, j in enumerate(c["slot"])]
    with pytest.raises(HarmonyError, match="no HIP device"):
        project_query((c["data"], c["indices"], c["indptr"], (6, 12)), genes, L)
