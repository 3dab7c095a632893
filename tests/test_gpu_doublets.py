"""Doublet detection on the MI355X: hmx_simulate_doublets against the fp64 spec (tests/doublets_ref.py) within the derived bar on the shape
sweep and at every tier of the launch plan, both value types, forced parent rows, a clip that bites, caller-given totals; bit-identity across
calls, residence of the matrix, the order of the entries inside a row, the order of the pairs and of the two parents; the kernel's guard
against out-of-contract device-resident input; hmx_doublet_neighbors against the library's own knn() and, on integer embeddings, the fp64
spec; scrub_doublets end to end on planted doublets; and the bits of project_query, knn and fit_loadings as they were before this feature.

Worst |gpu - spec| / bar and the AUROCs seen on an MI355X: see DESIGN "Doublet detection"."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import doublets_golden as dg  # noqa: E402
import doublets_ref as dr  # noqa: E402
import metrics_ref as mr  # noqa: E402
import project_ref as pr  # noqa: E402
from harmony_amd import (Harmony, HarmonyError, HarmonyLoadings, doublet_neighbors, doublet_scores_from_counts, doublet_threshold,  # noqa: E402
                         fit_loadings, knn, project_query, scrub_doublets, simulate_doublets)
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = (300, 900, 300, 50, 601)
# the spec's own AUROC for the planted doublets over seeds 0..4 (tests/test_doublets_cpu.py measures and pins them): 0.99818, 0.99849, 0.99821,
# 0.99855, 0.99979 -- min 0.99818, spread 0.00161.  The library must reach the minimum less one spread: the spec's seed-to-seed movement.
SPEC_AUROC_MIN, SPEC_AUROC_SPREAD = dr.SPEC_AUROC_MIN, dr.SPEC_AUROC_SPREAD


@functools.lru_cache(maxsize=None)
def case(shape, integer=True):
    c, pairs = dr.case(shape, integer)
    genes = np.array(["r%d" % j if j >= 0 else "q%d" % g for g, j in enumerate(c["slot"])])
    return c, pairs, genes


def loadings(c, clip=None):
    return HarmonyLoadings(["r%d" % j for j in range(c["U"].shape[0])], c["U"], c["mean"], c["sd"], clip=clip)


def csr(c, dtype=np.float64):
    return (c["data"].astype(dtype), c["indices"], c["indptr"], (len(c["indptr"]) - 1, c["G_all"]))


@functools.lru_cache(maxsize=None)
def spec(shape, clip=None, integer=True):
    c, pairs, _ = case(shape, integer)
    return dr.simulate(pairs=pairs, clip=clip, **c), dr.bars(pairs=pairs, clip=clip, **c)


def sim(shape, dtype=np.float64, clip=None, integer=True, pairs=None, **kw):
    c, own, genes = case(shape, integer)
    out, back = simulate_doublets(csr(c, dtype), genes, loadings(c, clip), pairs=own if pairs is None else pairs, **kw)
    assert np.array_equal(back, own if pairs is None else pairs)
    return out


def worst(got, shape, clip=None, integer=True):
    P, bar = spec(shape, clip, integer)
    assert got.shape == P.shape and got.dtype == np.float32 and np.all(np.isfinite(got))
    r = float((np.abs(got.astype(np.float64) - P) / bar).max())
    print("doublets %s clip %s: worst |gpu - spec| / bar = %.3f" % (shape, clip, r))
    return r


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", dr.SHAPES + dr.TIER_SHAPES)
def test_against_the_spec_within_the_bar(shape, dtype):
    """the sweep and one G at and above each boundary of the plan's tiers; the forced pairs: parent rows of 0, 1, 63, 64, 65 and 200 entries,
    a == b, an empty parent, parents sharing all of their genes and none, a parent of genes the reference lacks, stored zeros"""
    c, pairs, _ = case(shape)
    got = sim(shape, dtype)
    assert worst(got, shape) <= 1.0
    if shape[0] > dr.APART_B:
        ip, n = c["indptr"], min(len(dr.FORCED), shape[4])
        assert [tuple(p) for p in pairs[:n]] == dr.FORCED[:n] and list(np.diff(ip)[:6]) == [min(r, shape[1]) for r in dr.ROWS]
        b = pr.offset(c["slot"], c["U"], c["mean"], c["sd"]).astype(np.float32)
        for s, (pa, pb) in enumerate(dr.FORCED[:n]):             # nothing but empty rows, unknown genes or stored zeros: the constant row
            if pa in (0, dr.UNKNOWN_ROW, dr.ZERO_ROW) and pb in (0, dr.UNKNOWN_ROW, dr.ZERO_ROW):
                assert np.array_equal(got[s], b), (pa, pb)
        if n > 14:
            cols = lambda r: set(c["indices"][ip[r]:ip[r + 1]].tolist())  # noqa: E731
            assert cols(dr.SAME_A) == cols(dr.SAME_B) and not (cols(dr.APART_A) & cols(dr.APART_B))
            assert np.array_equal(got[13], got[14])              # (a, b) against (b, a)


def test_clip_that_bites():
    c, pairs, _ = case(BIG)
    plain = sim(BIG)
    got = sim(BIG, clip=10.0)
    assert worst(got, BIG, clip=10.0) <= 1.0
    assert not np.array_equal(got, plain)                       # the clip lowered something: the case tests it
    P0, P1 = spec(BIG)[0], spec(BIG, clip=10.0)[0]
    assert np.abs(P0 - P1).max() > 100 * spec(BIG)[1].max()


def test_non_integer_counts_and_given_totals():
    c, pairs, genes = case(BIG, integer=False)
    for dtype in (np.float32, np.float64):
        got = sim(BIG, dtype, integer=False)
        if dtype == np.float32:                                 # the spec of the values the kernel was given
            c32 = dict(c, data=c["data"].astype(np.float32).astype(np.float64))
            P, bar = dr.simulate(pairs=pairs, **c32), dr.bars(pairs=pairs, **c32)
            r = float((np.abs(got.astype(np.float64) - P) / bar).max())
        else:
            r = worst(got, BIG, integer=False)
        print("doublets non-integer %s: worst / bar = %.3f" % (dtype.__name__, r))
        assert r <= 1.0
    tot = np.random.default_rng(4).uniform(100.0, 5000.0, BIG[0])
    tot[0] = tot[dr.ZERO_ROW] = 0.0                             # a caller's zeros: the pair (0, 0) has T_s = 0, y = 0
    got = sim(BIG, integer=False, totals=tot)
    P, bar = dr.simulate(pairs=pairs, totals=tot, **c), dr.bars(pairs=pairs, totals=tot, **c)
    r = float((np.abs(got.astype(np.float64) - P) / bar).max())
    print("doublets given totals: worst / bar = %.3f" % r)
    assert r <= 1.0
    assert np.array_equal(got[0], pr.offset(c["slot"], c["U"], c["mean"], c["sd"]).astype(np.float32))


@pytest.mark.parametrize("n_sim", [1, 3, 5])
def test_fewer_cells_than_waves_equal_the_same_pairs_inside_a_larger_call(n_sim):
    c, pairs, _ = case(BIG)
    big = sim(BIG)
    for start in (0, 12, 40):
        sub = np.ascontiguousarray(pairs[start:start + n_sim])
        assert np.array_equal(sim(BIG, pairs=sub), big[start:start + n_sim]), (n_sim, start)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bits_do_not_depend_on_repetition_residence_or_any_order(dtype):
    c, pairs, genes = case(BIG)
    L = loadings(c)
    host = sim(BIG, dtype)
    assert np.array_equal(host, sim(BIG, dtype))                                   # two calls
    dev = DeviceCSR(*csr(c, dtype))
    assert np.array_equal(host, simulate_doublets(dev, genes, L, pairs=pairs)[0])      # host- against device-resident
    obj = Harmony()
    obj._set("project_slab_bytes", 4096)                                           # the upload of the whole matrix in many chunked copies
    assert np.array_equal(host, simulate_doublets(csr(c, dtype), genes, L, pairs=pairs, _handle=_ObjHandle(obj))[0])
    assert obj.timer("simulate_doublets") > 0
    rng = np.random.default_rng(7)
    ip = c["indptr"]
    take = np.concatenate([ip[i] + rng.permutation(ip[i + 1] - ip[i]) for i in range(BIG[0])]).astype(np.int64)
    assert not np.array_equal(take, np.arange(take.size))
    shuffled = (c["data"][take].astype(dtype), c["indices"][take], ip, (BIG[0], BIG[1]))
    assert np.array_equal(host, simulate_doublets(shuffled, genes, L, pairs=pairs)[0])      # entries shuffled inside every CSR row
    perm = rng.permutation(BIG[4])
    assert np.array_equal(host[perm], sim(BIG, dtype, pairs=np.ascontiguousarray(pairs[perm])))      # pairs permuted: rows permuted
    assert np.array_equal(host, sim(BIG, dtype, pairs=np.ascontiguousarray(pairs[:, ::-1])))         # (a, b) against (b, a)


def test_same_parent_twice_and_an_empty_parent_are_the_cell_itself():
    """(a, a) and (a, empty cell) against project_query of row a, within the sum of the two bars"""
    c, _, genes = case(BIG)
    L = loadings(c)
    rows = np.array([1, 2, 3, 4, 5, dr.SAME_A, dr.APART_B, 20, 77, 299])
    pairs = np.concatenate([np.stack([rows, rows], axis=1), np.stack([rows, np.zeros_like(rows)], axis=1), np.stack([np.zeros_like(rows), rows], axis=1)])
    got = simulate_doublets(csr(c), genes, L, pairs=pairs)[0].astype(np.float64)
    own = project_query(csr(c), genes, L).astype(np.float64)[rows]
    bar = pr.bars(**c)[rows]
    for k in range(3):
        part = slice(k * rows.size, (k + 1) * rows.size)
        r = float((np.abs(got[part] - own) / (bar + dr.bars(pairs=pairs[part], **c))).max())
        print("doublets %s against project_query: worst / (bar + bar) = %.3f" % (("(a, a)", "(a, empty)", "(empty, a)")[k], r))
        assert r <= 1.0
    assert np.array_equal(got[rows.size:2 * rows.size], got[2 * rows.size:])


def test_guard_on_device_resident_input():
    """out-of-contract input in HBM cannot be validated on the host: the kernel must refuse the entry, raise the flag and end cleanly"""
    c, pairs, genes = case(BIG)
    L = loadings(c)
    good = simulate_doublets(csr(c), genes, L, pairs=pairs)[0]
    data, indices, indptr, shp = csr(c)
    at = int(indptr[5]) + 3                                      # row 5: a parent of the forced pairs (4, 5), (5, 5), (5, 0)
    known = int(indptr[5] + np.nonzero(c["slot"][indices[indptr[5]:indptr[6]]] >= 0)[0][2])

    def broken(name, where, value):
        a = dict(data=data.copy(), indices=indices.copy(), indptr=indptr.copy())
        a[name][where] = value
        return DeviceCSR(a["data"], a["indices"], a["indptr"], shp)

    for name, where, value, text in (("indices", at, BIG[1], "column index"), ("indices", at, -1, "column index"),
                                     ("indices", at, 2 ** 30, "column index"), ("data", known, -1.0, "negative"),
                                     ("data", known, np.nan, "not finite"), ("data", known, np.inf, "not finite"),
                                     ("indptr", 9, int(indptr[-1]) + 1000, "indptr")):      # rows 8 and 9: the forced pair (8, 9)
        with pytest.raises(HarmonyError, match=text) as e:
            simulate_doublets(broken(name, where, value), genes, L, pairs=pairs)
        assert "status 1" in str(e.value), str(e.value)
        assert np.array_equal(simulate_doublets(DeviceCSR(data, indices, indptr, shp), genes, L, pairs=pairs)[0], good)      # the process goes on, correctly
    with pytest.raises(HarmonyError, match="negative"):          # a host-resident matrix: the same flag
        bad = data.copy()
        bad[known] = -2.0
        simulate_doublets((bad, indices, indptr, shp), genes, L, pairs=pairs)


# ---- the neighbour counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obs,n_sim,d,k_adj", [(200, 400, 10, 30), (65, 64, 3, 128), (50, 1, 4, 1)])
def test_neighbour_counts(n_obs, n_sim, d, k_adj):
    rng = np.random.default_rng(n_obs + k_adj)
    X = rng.standard_normal((n_obs + n_sim, d)).astype(np.float32)
    cnt, idx, dist = doublet_neighbors(X[:n_obs], X[n_obs:], k_adj, return_knn=True)
    kidx, kdist = knn(X, k_adj)
    assert cnt.dtype == np.int32 and cnt.shape == (n_obs + n_sim,)
    assert np.array_equal(idx, kidx) and np.array_equal(dist, kdist)                 # the optional lists are knn()'s
    assert np.array_equal(cnt, (kidx >= n_obs).sum(axis=1))                          # the counts, recomputed on the host from those lists
    assert np.array_equal(cnt, doublet_neighbors(X[:n_obs], X[n_obs:], k_adj)) and np.array_equal(cnt, doublet_neighbors(X[:n_obs].astype(np.float64), X[n_obs:], k_adj))
    # integer-valued embeddings: every product and sum below 2^24, the library's d^2 is exact and ties go to the smaller index on both sides
    Z = rng.integers(-6, 7, (n_obs + n_sim, d)).astype(np.float32)
    want, ridx = dr.neighbor_counts(Z, n_obs, k_adj)
    got, gidx, _ = doublet_neighbors(Z[:n_obs], Z[n_obs:], k_adj, return_knn=True)
    assert np.array_equal(gidx, ridx) and np.array_equal(got, want)
    assert got.max() <= min(k_adj, n_sim) and (got.sum() > 0 or n_sim == 1)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_scrub_doublets_finds_the_planted_doublets(seed):
    """AUROC, a threshold, and at least half of the planted doublets flagged, as the issue sets them.  The threshold is the fragile part: the
    fp64 spec's own thresholds over seeds 0..4 are 0.157, 0.116, 0.200, 0.575, 0.166 and flag 100, 100, 100, 17, 100 % of the planted doublets
    (tests/test_doublets_cpu.py pins these figures; DESIGN "Doublet detection" says why: 58 possible scores, the synthetic heterotypic cells on
    the top three, threshold_minimum able to settle between two of them).  The library's pipeline met the check on all five seeds on an MI355X."""
    p = dr.planted(seed)
    genes = np.array(["gene%d" % g for g in range(p["X"].shape[1])])
    res = scrub_doublets(p["X"], genes, n_top_genes=300, d=10, seed=seed)
    N = p["X"].shape[0]
    assert res["score"].shape == (N,) and res["score_se"].shape == (N,) and res["sim_score"].shape == (2 * N,) and res["k_adj"] == 57
    assert np.array_equal(res["pairs"], np.random.default_rng(seed).integers(0, N, (2 * N, 2)))
    a = dr.auroc(res["score"], p["is_doublet"])
    found = float(res["predicted"][p["is_doublet"]].mean()) if res["predicted"] is not None else -1.0
    print("scrub_doublets seed %d: AUROC %.5f (spec %.5f), threshold %s, planted doublets flagged %.3f, singlets flagged %.4f"
          % (seed, a, dr.SPEC_AUROC[seed], res["threshold"], found, -1.0 if res["predicted"] is None else float(res["predicted"][~p["is_doublet"]].mean())))
    assert a >= SPEC_AUROC_MIN - SPEC_AUROC_SPREAD, a
    assert res["threshold"] is not None and res["threshold"] == doublet_threshold(res["sim_score"])
    assert res["predicted"].dtype == bool and found >= 0.5
    again = scrub_doublets(p["X"], genes, n_top_genes=300, d=10, seed=seed, threshold=0.25)
    assert np.array_equal(again["score"], res["score"]) and again["threshold"] == 0.25 and np.array_equal(again["predicted"], res["score"] > 0.25)


def test_scores_are_the_closed_form_of_the_counts():
    p = dr.planted(0)
    genes = np.array(["gene%d" % g for g in range(p["X"].shape[1])])
    L, _, _ = fit_loadings(p["X"], genes, n_top_genes=300, d=10, seed=0)
    obs = project_query(p["X"], genes, L)
    simp, pairs = simulate_doublets(p["X"], genes, L, seed=0)
    n = doublet_neighbors(obs, simp, 57)
    res = scrub_doublets(p["X"], genes, loadings=L, seed=0)
    score, se = doublet_scores_from_counts(n, 57, 1500, 3000)
    assert np.array_equal(res["score"], score[:1500]) and np.array_equal(res["sim_score"], score[1500:]) and np.array_equal(res["score_se"], se[:1500])


# ---- what was here before --------------------------------------------------------------------------------------------------------------------
def test_project_query_knn_and_fit_loadings_are_unchanged_in_bits():
    """k_project's queue moved into hmx_proj_row.h, where k_doublet_project shares it: the results recorded before the move"""
    gold = np.load(dg.GOLDEN)
    got = dg.earlier_results()
    assert sorted(gold.files) == sorted(got)
    for name in got:
        assert np.array_equal(got[name], gold[name]), name
