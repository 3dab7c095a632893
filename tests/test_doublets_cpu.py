"""Doublet detection without a GPU: the C ABI of include/harmony_mi355x_doublets.h against the library and harmony_amd/_lib.py, every Python
argument error, every status the library decides on the host, the launch plan as a pure function (hmx_doublet_plan.h through
tests/cpp/doublet_plan_probe.cpp), the fp64 spec (tests/doublets_ref.py) by hand on a 3-cell matrix, the score formulas and the threshold
against values written out by hand, honest fp32 against the derived error bar on the GPU test's shapes, and the quality constants of the GPU
test measured from the spec alone (tests/test_gpu_doublets.py runs the library).

Measured here (the figures DESIGN "Doublet detection" quotes):
  honest fp32 / bar on the GPU test's shapes: worst 0.48 (the sweep), 0.47 (the tier shapes)
  AUROC of the spec's score for the planted doublets, seeds 0..4: see SPEC_AUROC below."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import doublets_ref as dr  # noqa: E402
import helpers  # noqa: E402
import project_ref as pr  # noqa: E402
import harmony_amd  # noqa: E402
from harmony_amd import (HarmonyError, HarmonyLoadings, _lib, doublet_neighbors, doublet_scores_from_counts, doublet_threshold,  # noqa: E402
                         doublets, scrub_doublets, simulate_doublets)

HMX_ERR_ARG, HMX_ERR_DEVICE, HMX_ERR_LIMIT = 1, 5, 7
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
HEADER = "harmony_mi355x_doublets.h"
# AUROC of the spec's doublet score for the planted heterotypic doublets (N = 1500, G_all = 600, G = 300, d = 10, r = 2), seeds 0..4, measured by
# test_quality_constants_from_the_spec_alone below: the GPU test asks for SPEC_AUROC_MIN - SPEC_AUROC_SPREAD
SPEC_AUROC, SPEC_AUROC_MIN, SPEC_AUROC_SPREAD = dr.SPEC_AUROC, dr.SPEC_AUROC_MIN, dr.SPEC_AUROC_SPREAD


# ---- the header, the library and the binding -------------------------------------------------------------------------------------------------
def test_header_matches_the_library_and_the_binding():
    found = helpers.header_functions(HEADER)
    mine = [n for n, _ in found]
    assert mine == ["hmx_simulate_doublets", "hmx_doublet_neighbors"] and set(mine) == set(_lib.DOUBLETS_SIGNATURES)
    for other in os.listdir(helpers.INCLUDE):                    # no other header names them, comments included
        if other != HEADER:
            assert not (set(mine) & helpers.header_names(other)), other
    tables = [t for t in dir(_lib) if t.endswith("SIGNATURES") and t != "DOUBLETS_SIGNATURES"]
    assert len(tables) >= 14 and not any(set(mine) & set(getattr(_lib, t)) for t in tables)
    lib = _lib.load()
    loose = {"const int32_t*": (C.POINTER(C.c_int32), C.c_void_p), "const int64_t*": (C.POINTER(C.c_int64), C.c_void_p)}      # (the count matrix: host or device pointers)
    for (name, types), count in zip(found, (21, 11)):
        assert len(types) == count
        helpers.assert_binding_matches(lib, name, types, _lib.DOUBLETS_SIGNATURES[name][1], loose)
    for name in ("simulate_doublets", "doublet_neighbors", "doublet_scores_from_counts", "doublet_threshold", "scrub_doublets"):
        assert name in harmony_amd.__all__ and hasattr(harmony_amd, name)


# ---- Python argument errors ------------------------------------------------------------------------------------------------------------------
def _loadings(G=6, d=3, **kw):
    rng = np.random.default_rng(0)
    return HarmonyLoadings(["g%d" % j for j in range(G)], rng.standard_normal((G, d)), rng.uniform(0, 1, G), rng.uniform(0.5, 1, G), **kw)


def test_python_errors_come_before_the_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    L = _loadings()
    X = np.ones((5, 4))
    genes = ["g2", "q", "g0", "g5"]
    for bad, match in ((dict(loadings=None), "HarmonyLoadings"), (dict(genes=["a", "b", "c", "d"]), "shares no gene"), (dict(genes=genes[:3]), "genes were named"),
                       (dict(totals=np.ones(4)), "totals"), (dict(totals=-np.ones(5)), "totals"), (dict(genes=["g2", "g2", "g0", "g5"]), "twice"),
                       (dict(pairs=np.zeros((0, 2), int)), "n_sim x 2"), (dict(pairs=np.zeros((3, 3), int)), "n_sim x 2"), (dict(pairs=[[0, 5]]), "name cells"),
                       (dict(pairs=[[-1, 0]]), "name cells"), (dict(pairs=[[0.5, 1.0]]), "integers"), (dict(sim_doublet_ratio=0.0), "ratio"),
                       (dict(sim_doublet_ratio=0.01), "no synthetic"), (dict(sim_doublet_ratio=float("nan")), "ratio"),
                       (dict(counts=np.ones(4)), "2-D"), (dict(loadings=_loadings(G=doublets.MAX_TABLE_GENES + 1, d=1), genes=["g0", "a", "b", "c"]), "at most")):
        kw = dict(counts=X, genes=genes, loadings=L)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            simulate_doublets(**kw)
    O, S = np.zeros((6, 3)), np.zeros((4, 3))
    for args, match in (((O, np.zeros((4, 2)), 3), "PCs"), ((O, S, 0), "k_adj"), ((O, S, 129), "k_adj"), ((O, S, 10), "other cells"), ((O, S, 2.5), "k_adj"),
                        ((np.zeros(6), S, 2), "cells x PCs"), ((O, np.zeros((0, 3)), 2), "cells x PCs"), ((np.zeros((6, 129)), np.zeros((4, 129)), 2), "at most")):
        with pytest.raises(ValueError, match=match):
            doublet_neighbors(*args)
    for args, kw in ((([1, 2], 0, 5, 5), {}), (([1, 9], 8, 5, 5), {}), (([-1], 8, 5, 5), {}), (([1.5], 8, 5, 5), {}), (([[1]], 8, 5, 5), {}), (([1], 8, 0, 5), {}),
                     (([1], 8, 5, 0), {}), (([1], 8, 5, 5), dict(expected_doublet_rate=0.0)), (([1], 8, 5, 5), dict(expected_doublet_rate=1.0)),
                     (([1], 8, 5, 5), dict(stdev_doublet_rate=-0.1))):
        with pytest.raises(ValueError):
            doublet_scores_from_counts(*args, **kw)
    for bad in ([], [float("nan")]):
        with pytest.raises(ValueError):
            doublet_threshold(bad)
    with pytest.raises(ValueError):
        doublet_threshold([0.1, 0.2], n_bins=2)
    for kw in (dict(loadings="x"), dict(sim_doublet_ratio=-1.0), dict(expected_doublet_rate=1.5), dict(stdev_doublet_rate=float("nan")), dict(threshold=float("inf")),
               dict(n_neighbors=0), dict(genes=genes[:3]), dict(counts=np.ones((1, 4)))):
        a = dict(counts=X, genes=genes, loadings=L)
        a.update(kw)
        with pytest.raises(ValueError):
            scrub_doublets(**a)


def test_default_pairs_are_the_documented_draw(monkeypatch):
    """pairs=None: round(ratio N) pairs from default_rng(seed).integers(0, N, (n_sim, 2)), handed to the library as they are"""
    seen = {}

    class FakeLib(object):
        def hmx_simulate_doublets(self, h, N, G_all, indptr, indices, data, dtype, loc, slot, U, mean, sd, G, d, scale, clip, totals, n_sim, pairs, out, oloc):
            seen.update(N=N, n_sim=n_sim, pairs=np.ctypeslib.as_array(pairs, (n_sim, 2)).copy(), oloc=oloc, loc=loc, clip=clip)
            return 0

    class FakeHandle(object):
        lib, h = FakeLib(), None

        def check(self, st, what):
            assert st == 0
    X = np.ones((7, 4))
    out, pairs = simulate_doublets(X, ["g2", "q", "g0", "g5"], _loadings(clip=5.0), sim_doublet_ratio=1.5, seed=3, _handle=FakeHandle())
    assert seen["n_sim"] == 10 and out.shape == (10, 3) and out.dtype == np.float32 and pairs.dtype == np.int64        # round(10.5) = 10: NumPy's round half to even
    assert np.array_equal(pairs, np.random.default_rng(3).integers(0, 7, (10, 2))) and np.array_equal(seen["pairs"], pairs)
    assert seen["oloc"] == 0 and seen["loc"] == 0 and seen["clip"] == 5.0
    given = np.array([[6, 6], [0, 3]])
    _, back = simulate_doublets(X, ["g2", "q", "g0", "g5"], _loadings(), pairs=given, _handle=FakeHandle())
    assert np.array_equal(back, given) and seen["n_sim"] == 2


def test_neighbour_defaults_and_the_cap():
    """Scrublet's defaults, and the cap at the 128 neighbours the exact search returns: k_adj = 128, n_neighbors reduced to fit"""
    assert doublets.default_neighbors(1500, 2.0) == (19, 57, False)
    assert doublets.default_neighbors(7000, 2.0) == (42, 126, False)
    n, k, capped = doublets.default_neighbors(7400, 2.0)
    assert (n, k, capped) == (42, 128, True) and round(43 * 3.0) > 128 >= round(n * 3.0)
    assert doublets.default_neighbors(10 ** 6, 2.0) == (42, 128, True)
    assert doublets.default_neighbors(100, 1.0, n_neighbors=200) == (64, 128, True)
    assert doublets.default_neighbors(100, 1.0, n_neighbors=10) == (10, 20, False)
    assert "CAPPED at 128" in scrub_doublets.__doc__


# ---- what the library decides on the host ----------------------------------------------------------------------------------------------------
def _sim_call(lib, h):
    c = pr.random_case(6, 12, 8, 3, seed=2, row_lengths=(0, 1, 5))
    base = dict(N=6, G_all=12, indptr=c["indptr"], indices=c["indices"], data=c["data"], dtype=0, loc=0, slot=c["slot"], U=c["U"].copy(),
                mean=c["mean"].copy(), sd=c["sd"].copy(), G=8, d=3, scale=1e4, clip=0.0, totals=None, n_sim=4,
                pairs=np.array([[0, 1], [2, 2], [5, 0], [3, 4]], dtype=np.int64), out=np.full((4, 3), 7.0, dtype=np.float32), oloc=0)
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    V = lambda v: None if v is None else C.c_void_p(v.ctypes.data)  # noqa: E731
    D = lambda v: None if v is None else v.ctypes.data_as(dp)  # noqa: E731

    def call(handle=h, **kw):
        a = dict(base)
        a.update(kw)
        return lib.hmx_simulate_doublets(handle, a["N"], a["G_all"], V(a["indptr"]), V(a["indices"]), V(a["data"]), a["dtype"], a["loc"],
                                         None if a["slot"] is None else a["slot"].ctypes.data_as(ip), D(a["U"]), D(a["mean"]), D(a["sd"]), a["G"], a["d"],
                                         a["scale"], a["clip"], D(a["totals"]), a["n_sim"], None if a["pairs"] is None else a["pairs"].ctypes.data_as(lp),
                                         V(a["out"]), a["oloc"])
    return call, base


def test_simulate_checks_the_arguments_before_the_device():
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    call, base = _sim_call(lib, h)

    def refused(status, match=None, **kw):
        assert call(**kw) == status, kw
        msg = lib.hmx_last_error(h).decode()
        assert msg and (match is None or match in msg), (kw, msg)
        assert np.all(base["out"] == 7.0)                       # the output is unwritten

    def changed(name, at, v):
        a = base[name].copy()
        a[at] = v
        return {name: a}

    two = base["slot"].copy()
    j = np.nonzero(two >= 0)[0]
    two[j[1]] = two[j[0]]
    free = np.nonzero(base["slot"] < 0)[0]
    big = doublets.MAX_TABLE_GENES + 1
    try:
        for name in ("indptr", "indices", "data", "slot", "U", "mean", "sd", "pairs", "out"):
            refused(HMX_ERR_ARG, **{name: None})
        for kw in (dict(N=0), dict(G_all=0), dict(G=0), dict(d=0), dict(dtype=2), dict(loc=2), dict(oloc=-1)):
            refused(HMX_ERR_ARG, **kw)
        refused(HMX_ERR_ARG, "n_sim", n_sim=0)
        refused(HMX_ERR_ARG, "n_sim", n_sim=-3)
        refused(HMX_ERR_ARG, "pairs[1][0] = 6", **changed("pairs", (1, 0), 6))
        refused(HMX_ERR_ARG, "pairs[3][1] = -1", **changed("pairs", (3, 1), -1))
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
        refused(HMX_ERR_ARG, "column", **changed("indices", 3, 12))
        refused(HMX_ERR_LIMIT, "d <= 128", d=129)
        refused(HMX_ERR_LIMIT, "G <= %d" % doublets.MAX_TABLE_GENES, G=big, U=np.zeros((big, 3)), mean=np.zeros(big), sd=np.ones(big))
        refused(HMX_ERR_LIMIT, G_all=(1 << 24) + 1)
        if NO_GPU:                                              # valid calls get as far as the device
            refused(HMX_ERR_DEVICE, "no HIP device")
            refused(HMX_ERR_DEVICE, dtype=1, data=base["data"].astype(np.float32), clip=10.0, totals=np.ones(6))
        out = (C.c_double * 1)()
        assert lib.hmx_get(h, b"timer:simulate_doublets", out, 1) == 1 and (out[0] == 0.0 or not NO_GPU)
    finally:
        lib.hmx_destroy(h)
    assert call(handle=None) == HMX_ERR_ARG


def test_neighbors_checks_the_arguments_before_the_device():
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    X = np.zeros((12, 4))
    cnt = np.full(12, -5, dtype=np.int32)
    ip = C.POINTER(C.c_int32)

    def call(handle=h, X=X, dtype=0, loc=0, n_obs=8, n_sim=4, d=4, k_adj=3, out=cnt):
        return lib.hmx_doublet_neighbors(handle, None if X is None else C.c_void_p(X.ctypes.data), dtype, loc, n_obs, n_sim, d, k_adj,
                                         None if out is None else out.ctypes.data_as(ip), None, None)

    def refused(status, match=None, **kw):
        assert call(**kw) == status, kw
        msg = lib.hmx_last_error(h).decode()
        assert msg and (match is None or match in msg), (kw, msg)
        assert np.all(cnt == -5)
    try:
        for kw in (dict(X=None), dict(out=None), dict(dtype=3), dict(loc=2), dict(n_obs=0), dict(n_sim=0), dict(d=0)):
            refused(HMX_ERR_ARG, **kw)
        refused(HMX_ERR_LIMIT, "1 <= k_adj <= 128", k_adj=0)
        refused(HMX_ERR_LIMIT, "1 <= k_adj <= 128", k_adj=129)
        refused(HMX_ERR_LIMIT, "n_obs + n_sim - 1", k_adj=12)
        refused(HMX_ERR_LIMIT, "d <= 128", d=129)
        if NO_GPU:
            refused(HMX_ERR_DEVICE, "no HIP device")
            refused(HMX_ERR_DEVICE, k_adj=11)
    finally:
        lib.hmx_destroy(h)
    assert call(handle=None) == HMX_ERR_ARG


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_no_cpu_fallback():
    c = pr.random_case(6, 12, 8, 3, seed=2)
    L = HarmonyLoadings(["r%d" % j for j in range(8)], c["U"], c["mean"], c["sd"])
    genes = ["r%d" % j if j >= 0 else "q%d" % g for g, j in enumerate(c["slot"])]
    with pytest.raises(HarmonyError, match="no HIP device"):
        simulate_doublets((c["data"], c["indices"], c["indptr"], (6, 12)), genes, L)
    with pytest.raises(HarmonyError, match="no HIP device"):
        doublet_neighbors(np.zeros((6, 3)), np.ones((4, 3)), 3)


# ---- the launch plan -------------------------------------------------------------------------------------------------------------------------
_probe = []


def plan_probe():
    if not _probe:
        so = os.path.join(tempfile.mkdtemp(prefix="doublet_plan_probe_"), "doublet_plan_probe.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared",
                               os.path.join(ROOT, "tests", "cpp", "doublet_plan_probe.cpp"), "-o", so])
        _probe.append(C.CDLL(so))
    return _probe[0]


def plan(G, d, n_sim):
    out = (C.c_longlong * 5)()
    st = plan_probe().probe_doublet_plan(C.c_int(G), C.c_int(d), C.c_longlong(n_sim), out)
    return st, dict(zip(("waves", "gp", "lds", "nc", "grid"), list(out)))


def test_plan_tiers_follow_from_the_queue_and_64_kb():
    k = (C.c_longlong * 7)()
    plan_probe().probe_doublet_constants(k)
    queue, lds, g4, g2, g1, max_d, max_grid = list(k)
    assert (queue, lds, max_d, max_grid) == (128, 65536, 128, 2048)
    # the rule: w waves keep w tables of gp words and w queues of `queue` (slot, weight) pairs in `lds` bytes, gp a multiple of the 64 slots of a sweep
    for w, g in ((4, g4), (2, g2), (1, g1)):
        assert g % 64 == 0 and w * (4 * g + 8 * queue) <= lds < w * (4 * (g + 64) + 8 * queue)
    assert (g4, g2, g1) == (3840, 7936, 16128) and g1 == doublets.MAX_TABLE_GENES
    for G, waves in ((1, 4), (64, 4), (65, 4), (2000, 4), (g4 - 1, 4), (g4, 4), (g4 + 1, 2), (g2, 2), (g2 + 1, 1), (g1 - 63, 1), (g1, 1)):
        st, p = plan(G, 50, 10 ** 6)
        assert st == 0 and p["waves"] == waves and p["gp"] == (G + 63) // 64 * 64 and p["gp"] >= G, (G, p)
        assert p["lds"] == waves * (4 * p["gp"] + 8 * queue) <= lds, (G, p)
        assert p["grid"] == max_grid and p["nc"] == 1
    assert plan(g1 + 1, 50, 10)[0] == 1 and plan(1 << 24, 50, 10)[0] == 1      # the genes' limit
    assert plan(100, 129, 10)[0] == 2 and plan(g1 + 1, 129, 10)[0] == 2        # the PCs' limit, named first
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0)):
        assert plan(*bad)[0] == 3
    for d, nc in ((1, 1), (64, 1), (65, 2), (128, 2)):
        assert plan(300, d, 7)[1]["nc"] == nc
    for G, n_sim, grid in ((300, 1, 1), (300, 4, 1), (300, 5, 2), (300, 8192, 2048), (300, 8193, 2048), (5000, 5, 3), (9000, 5, 5), (9000, 4000, 2048)):
        assert plan(G, 10, n_sim)[1]["grid"] == grid, (G, n_sim)


# ---- the spec by hand ------------------------------------------------------------------------------------------------------------------------
def _tiny():
    """3 cells x 4 genes.  cell 0: g0 = 1, g1 = 3; cell 1: g1 = 1, g2 = 2; cell 2: empty.  The reference has 3 genes: g0 -> 0, g1 -> 1, its gene 2 is
    absent from the matrix; g2 and g3 are unknown to it.  scale = 7 makes the rates round numbers."""
    data, indices, indptr = np.array([3.0, 1.0, 2.0, 1.0]), np.array([1, 0, 2, 1], dtype=np.int32), np.array([0, 2, 4, 4], dtype=np.int64)
    slot = np.array([0, 1, -1, -1], dtype=np.int32)
    U = np.array([[1.0, 0.0], [0.0, 1.0], [2.0, -1.0]])
    mean, sd = np.array([0.5, 0.25, 1.0]), np.array([2.0, 0.5, 4.0])
    return dict(data=data, indices=indices, indptr=indptr, G_all=4, slot=slot, U=U, mean=mean, sd=sd, scale=7.0)


def test_spec_by_hand():
    t = _tiny()
    b = np.array([-0.25, -0.5])                                  # -(0.5 / 2) U[0] - (0.25 / 0.5) U[1]; reference gene 2 is absent: nothing
    ln = math.log
    pairs = [(0, 1), (0, 0), (0, 2), (2, 2), (1, 0), (1, 1), (1, 2)]
    for f in (dr.simulate, dr.simulate_sparse):
        P = f(pairs=pairs, **t)
        # (0, 1): T = 4 + 3 = 7; g0: 1 -> log1p(1), the shared g1: 3 + 1 = 4 BEFORE the log -> log1p(4); g2 only counts in T
        assert np.allclose(P[0], b + [ln(2.0) / 2.0, ln(5.0) / 0.5], rtol=0, atol=1e-14)
        assert abs(P[0, 1] - (b[1] + (ln(1 + 21.0 / 4) + ln(1 + 7.0 / 3)) / 0.5)) > 1.0      # not the sum of the parents' logs
        # a == b is the single cell: 2 x / 2 T
        one = pr.project(t["data"], t["indices"], t["indptr"], 4, t["slot"], t["U"], t["mean"], t["sd"], scale=7.0)
        assert np.allclose(P[1], one[0], rtol=0, atol=1e-14) and np.allclose(P[5], one[1], rtol=0, atol=1e-14)
        assert np.allclose(P[1], b + [ln(1 + 7.0 / 4) / 2.0, ln(1 + 21.0 / 4) / 0.5], rtol=0, atol=1e-14)
        # an empty parent adds nothing, not even to T
        assert np.allclose(P[2], one[0], rtol=0, atol=1e-14) and np.allclose(P[6], one[1], rtol=0, atol=1e-14)
        # T_s = 0: y = 0 and P = b
        assert np.array_equal(P[3], b)
        assert np.array_equal(P[4], P[0])                        # (b, a) is (a, b)
        # a clip that bites on the sum: cap_1 = 0.25 + 2 x 0.5 = 1.25 < log1p(4) = 1.609 although parent 1's own y = log1p(7 / 3) = 1.204 stays
        # under it (the pair's rate is a weighted mean of its parents': the other parent, log1p(21 / 4), is over the cap too); cap_0 = 4.5 never bites
        Pc = f(pairs=pairs, clip=2.0, **t)
        assert np.allclose(Pc[0], b + [ln(2.0) / 2.0, 1.25 / 0.5], rtol=0, atol=1e-14)
        assert np.allclose(Pc[5], P[5], rtol=0, atol=1e-14) and Pc[0, 1] < P[0, 1] - 0.5
        # caller-given totals replace the row sums: T_s = 10 + 4
        Pt = f(pairs=[(0, 1)], totals=np.array([10.0, 4.0, 1.0]), **t)
        assert np.allclose(Pt[0], b + [ln(1.5) / 2.0, ln(3.0) / 0.5], rtol=0, atol=1e-14)
    bar = dr.bars(pairs=pairs, **t)
    w = np.array([ln(2.0) / 2.0, ln(5.0) / 0.5])
    assert np.allclose(bar[0], (2 + 18) * 2.0 ** -24 * w + 2 * 2.0 ** -24 * np.abs(b), rtol=1e-12)
    assert np.allclose(bar[3], 2 * 2.0 ** -24 * np.abs(b), rtol=1e-12)
    assert np.array_equal(dr.simulate_fp32(pairs=pairs, **t)[3], b.astype(np.float32))


def test_sparse_identity_equals_the_dense_form():
    for shape, clip, integer in (((17, 70, 40, 3, 5), None, True), ((90, 400, 257, 68, 7), 1.0, False), ((120, 500, 500, 128, 64), 10.0, True)):
        c, pairs = dr.case(shape, integer)
        a, b = dr.simulate(pairs=pairs, clip=clip, **c), dr.simulate_sparse(pairs=pairs, clip=clip, **c)
        assert np.abs(a - b).max() <= 1e-12


# ---- the scores ------------------------------------------------------------------------------------------------------------------------------
def test_scores_against_values_written_out_by_hand():
    # n = 3 of k_adj = 8, r = 2, rho = 0.1, stdev = 0.02: q = 4 / 10; rho / r = 0.05; the denominator 0.9 - 0.4 x 0.85 = 0.56; L = 0.02 / 0.56 = 1 / 28
    L, se = doublet_scores_from_counts([3], 8, 100, 200)
    assert abs(L[0] - 1.0 / 28.0) <= 1e-16
    # se_q^2 = 0.24 / 11; (se_q / q (1 - rho))^2 = 0.24 / 11 / 0.16 x 0.81; (stdev / rho (1 - q))^2 = (0.2 x 0.6)^2 = 0.0144
    want = 0.02 / 0.3136 * math.sqrt(0.24 / 11.0 / 0.16 * 0.81 + 0.0144)
    assert abs(se[0] - want) <= 1e-15 and abs(want - 0.0225349) <= 1e-6
    # n = 0 of k_adj = 30, r = 1, rho = 0.25, stdev = 0.05: q = 1 / 32; the denominator 0.75 - 0.5 / 32 = 0.734375; L = (1 / 128) / 0.734375 = 1 / 94
    L, se = doublet_scores_from_counts(np.array([0], dtype=np.int32), 30, 50, 50, expected_doublet_rate=0.25, stdev_doublet_rate=0.05)
    assert abs(L[0] - 1.0 / 94.0) <= 1e-16
    # se_q^2 = (1 / 32)(31 / 32) / 33; (se_q / q x 0.75)^2 = 31 / 33 x 0.5625; (0.05 / 0.25 x 31 / 32)^2 = 0.19375^2
    want = (1.0 / 128.0) / 0.734375 ** 2 * math.sqrt(31.0 / 33.0 * 0.5625 + 0.19375 ** 2)
    assert abs(se[0] - want) <= 1e-15 and abs(want - 0.0108979) <= 1e-6
    # every count at once, monotone in n, and the largest score at n = k_adj: q = 9 / 10
    L, se = doublet_scores_from_counts(np.arange(9), 8, 100, 200)
    assert L.dtype == np.float64 and np.all(np.diff(L) > 0) and abs(L[8] - 0.9 * 0.05 / (0.9 - 0.9 * 0.85)) <= 1e-15 and np.all(se > 0)


def _sample(counts, lo=0.0, hi=1.0):
    """a sample whose 256-bin histogram over its own range is `counts` (both end bins occupied): every bin's centre, count times"""
    assert counts[0] > 0 and counts[-1] > 0
    edges = np.linspace(lo, hi, len(counts) + 1)
    return np.repeat(0.5 * (edges[:-1] + edges[1:]), counts)


def test_threshold_between_two_planted_modes_and_none_for_one():
    x = np.arange(256)
    two = np.round(900 * np.exp(-0.5 * ((x - 40) / 12.0) ** 2) + 300 * np.exp(-0.5 * ((x - 190) / 20.0) ** 2)).astype(int)
    rng = np.random.default_rng(0)
    noisy = np.maximum(two + rng.integers(-3, 4, 256) * (two > 5), 0)      # ragged: many local maxima before the smoothing
    for counts in (two, noisy):
        t = doublet_threshold(_sample(counts))
        assert t is not None and 80 / 256.0 < t < 150 / 256.0, t            # between the modes at 40 / 256 and 190 / 256, where the histogram is empty
    one = np.round(900 * np.exp(-0.5 * ((x - 128) / 60.0) ** 2)).astype(int)
    assert doublet_threshold(_sample(one)) is None
    assert doublet_threshold(np.full(10, 0.3)) is None                      # one distinct score
    assert doublet_threshold(_sample(np.round(500 * np.exp(-x / 60.0)).astype(int))) is None      # a monotone decay: one mode at the edge
    # scaled and shifted scores: the threshold moves with them
    t0, t1 = doublet_threshold(_sample(two)), doublet_threshold(_sample(two, lo=2.0, hi=6.0))
    assert abs((t1 - 2.0) / 4.0 - t0) <= 1e-9


# ---- the error bar ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,integer,clip", [(s, True, None) for s in dr.SHAPES + dr.TIER_SHAPES] + [(s, False, 10.0) for s in dr.SHAPES])
def test_honest_fp32_stays_inside_the_bar(shape, integer, clip):
    """the bar is sound and not vacuous: a sequential float32 evaluation of the kernel's slot-ordered form stays inside it on the GPU test's
    shapes (the tier shapes run with integer counts only, here and on the GPU)"""
    c, pairs = dr.case(shape, integer)
    if shape[0] > 64:
        pairs = pairs[:64]                                       # (the forced pairs and some random ones: the Python loop is slow)
    spec = dr.simulate(pairs=pairs, clip=clip, **c)
    bar = dr.bars(pairs=pairs, clip=clip, **c)
    got = dr.simulate_fp32(pairs=pairs, clip=clip, **c).astype(np.float64)
    ratio = np.abs(got - spec) / bar
    print("doublets %s integer %s clip %s: fp32 / bar = %.3f" % (shape, integer, clip, ratio.max()))
    assert ratio.max() <= 1.0, ratio.max()
    if shape[2] >= 40:
        big = np.abs(spec) >= 0.1 * np.abs(spec).max()
        assert (bar[big] / np.abs(spec[big])).min() <= 1e-3                     # tight where the entries are not cancelling sums


# ---- the quality constants of the GPU test ---------------------------------------------------------------------------------------------------
def test_quality_constants_from_the_spec_alone():
    """five planted data sets through the fp64 spec and the brute-force search: the AUROC of the doublet score for the planted doublets.
    SPEC_AUROC records what this prints; tests/test_gpu_doublets.py holds the library to min - spread of these five."""
    got, flagged = [], []
    for seed in range(5):
        p = dr.planted(seed)
        assert p["is_doublet"].sum() == 75
        obs, sim = dr.spec_scores(p, seed=seed, score_fn=doublet_scores_from_counts)
        got.append(dr.auroc(obs, p["is_doublet"]))
        assert sim.mean() > obs.mean()
        t = doublet_threshold(sim)
        flagged.append((round(t, 3), round(float((obs[p["is_doublet"]] > t).mean()), 3), round(float((obs[~p["is_doublet"]] > t).mean()), 4)))
    print("spec AUROC, seeds 0..4:", ", ".join("%.4f" % a for a in got), " mean %.4f min %.4f spread %.4f" % (np.mean(got), min(got), max(got) - min(got)))
    assert np.allclose(got, SPEC_AUROC, rtol=0, atol=2e-4), got      # (one swapped doublet / singlet pair of 75 x 1425 moves it by 9.4e-6: a LAPACK that rounds the SVD differently may swap a few)
    # the threshold on the SPEC's scores: (threshold, planted doublets above it, singlets above it).  k_adj = 57 allows 58 scores; the heterotypic
    # synthetic cells pile up on the largest three, 35-50 histogram bins apart, and threshold_minimum's smoothing may settle between two of those
    # instead of in the wide valley below them: on seed 3 it does, in the fp64 spec itself
    print("spec threshold, doublets flagged, singlets flagged:", flagged)
    want = [(0.157, 1.0, 0.0182), (0.116, 1.0, 0.0288), (0.2, 1.0, 0.0133), (0.575, 0.173, 0.0007), (0.166, 1.0, 0.0133)]
    assert np.allclose(flagged, want, rtol=0, atol=0.03), flagged      # (a bin or two of the 256, a doublet or two of the 75)
    assert SPEC_AUROC_MIN - SPEC_AUROC_SPREAD > 0.8             # the planted doublets are found: the GPU test's bound is not vacuous
    assert dr.auroc([0.1, 0.4, 0.35, 0.8], [0, 0, 1, 1]) == 0.75 and dr.auroc([1, 1, 1, 1], [0, 1, 0, 1]) == 0.5
