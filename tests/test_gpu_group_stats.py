"""Gene statistics per group on the MI355X: hmx_gene_stats_grouped against the fp64 spec (tests/group_stats_ref.py) within the derived bars on the
shapes that reach each path of the kernel; the group sums partition hmx_gene_stats' bit for bit; bit-identity across calls, residence of the
matrix, slabs, cell order and the numbering of the groups; the guards; variable_genes and rank_genes_groups on planted cases.

The cases (group_stats_ref.group_case): one cell per group; a level no cell carries; labels i mod 5; one group of one below, at and one above the
work list's chunk of 256 cells beside a group of one cell; groups of exactly 16 and 17 cells (the workgroup's 16 waves take one cell each at a
time); 7700 genes with entries at genes 7679, 7680 and 7699, on both sides of the 7680 genes a workgroup's LDS tables hold.
Worst |gpu - spec| / bar seen over the sweep on an MI355X: see DESIGN "Gene statistics per group"."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import group_stats_ref as gr  # noqa: E402
import pca_ref as pc  # noqa: E402
from harmony_amd import (Harmony, HarmonyError, fit_loadings, gene_stats, gene_stats_by_group, markers_from_sums,  # noqa: E402
                         rank_genes_groups, variable_genes)
from harmony_amd.pca import choose_genes  # noqa: E402
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402

pytestmark = pytest.mark.gpu

SLAB_CAP = 1500      # bytes: several slabs at 257 x 900, and the row of 200 entries (8 or 12 bytes each) longer than one
KEYS = ("n_obs", "n_cells", "s1", "s2", "mean", "var")


@functools.lru_cache(maxsize=None)
def case(name, integer=True):
    return gr.group_case(name, integer)


def csr(c, dtype=np.float64):
    return (c["data"].astype(dtype), c["indices"], c["indptr"], (len(c["indptr"]) - 1, c["G_all"]))


def names(c):
    return ["g%d" % g for g in range(c["G_all"])]


def A(c):
    return c["data"], c["indices"], c["indptr"], c["G_all"]


def capped_handle(cap):
    """a handle whose host-resident matrices are uploaded in slabs of at most `cap` bytes"""
    obj = Harmony()
    obj._set("project_slab_bytes", cap)
    return obj, _ObjHandle(obj)


def permuted(c, perm, dtype=np.float64):
    ip = c["indptr"]
    take = np.concatenate([np.arange(ip[i], ip[i + 1]) for i in perm] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    pip = np.concatenate([[0], np.cumsum(np.diff(ip)[perm])]).astype(np.int64)
    return (c["data"][take].astype(dtype), c["indices"][take], pip, (len(ip) - 1, c["G_all"]))


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def ratios(got, c, codes, B, totals=None):
    """n_obs, n_cells and the steps exact; -> worst |gpu - spec| / bar of s1, s2, var"""
    st, b = gr.group_stats(*A(c), codes, B, totals=totals), gr.group_bars(*A(c), codes, B, totals=totals)
    assert np.array_equal(got["n_obs"], st["n_obs"]) and np.array_equal(got["n_cells"], st["n_cells"])
    assert got["s1"].shape == (B, c["G_all"]) and tuple(got["step"]) == pc.stat_steps(len(c["indptr"]) - 1, 1e4, totals is not None)
    has = b["s1"] > 0
    assert np.all(got["s1"][~has] == 0) and np.all(got["s2"][~has] == 0)
    r = {k: float((np.abs(got[k] - st[k])[has] / b[k][has]).max()) if has.any() else 0.0 for k in ("s1", "s2")}
    assert np.array_equal(np.isnan(got["var"]), np.isnan(st["var"])) and np.array_equal(np.isnan(got["mean"]), np.isnan(st["mean"]))
    hv = has & np.isfinite(b["var"])
    r["var"] = float((np.abs(got["var"] - st["var"])[hv] / b["var"][hv]).max()) if hv.any() else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(got["mean"], np.where(got["n_obs"][:, None] >= 1, got["s1"] / got["n_obs"][:, None], np.nan), equal_nan=True)
    return r


# ---- 1. within the bars ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", gr.CASES)
def test_group_stats_within_the_bars(name, dtype):
    c, codes, B = case(name)
    got = gene_stats_by_group(csr(c, dtype), names(c), codes, levels=np.arange(B))
    r = ratios(got, c, codes, B)
    print("gene_stats_by_group %s %s: worst |gpu - spec| / bar = %s" % (name, np.dtype(dtype).name, {k: round(v, 3) for k, v in r.items()}))
    assert all(v <= 1.0 for v in r.values()), r
    if name == "two_ranges":
        for g in gr.EDGE_GENES:
            assert got["n_cells"][:, g].sum() > 0 and np.all((got["s1"][:, g] > 0) == (got["n_cells"][:, g] > 0))


def test_group_stats_non_integer_counts_and_given_totals():
    c, codes, B = case("mod5", integer=False)
    lv = np.arange(B)
    r = ratios(gene_stats_by_group(csr(c), names(c), codes, levels=lv), c, codes, B)
    tot = np.random.default_rng(4).uniform(100.0, 5000.0, codes.size)
    tot[3] = 0.0                                                # a caller's zero: y = 0
    rt = ratios(gene_stats_by_group(csr(c), names(c), codes, levels=lv, totals=tot), c, codes, B, totals=tot)
    print("gene_stats_by_group non-integer counts: %s; given totals: %s" % (r, rt))
    assert all(v <= 1.0 for v in r.values()) and all(v <= 1.0 for v in rt.values())


# ---- 2. the groups partition the ungrouped sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gr.CASES)
def test_group_sums_add_up_to_gene_stats_bit_for_bit(name):
    c, codes, B = case(name)
    out, pooled = gene_stats_by_group(csr(c), names(c), codes, levels=np.arange(B)), gene_stats(csr(c), names(c))
    assert np.array_equal(out["step"], pooled["step"])
    assert np.array_equal(out["s1"].sum(0), pooled["s1"]) and np.array_equal(out["s2"].sum(0), pooled["s2"])
    assert np.array_equal(out["n_cells"].sum(0), pooled["n_cells"]) and out["n_obs"].sum() == codes.size
    assert pooled["s1"].max() / pooled["step"][0] < 2.0 ** 53 and pooled["s2"].max() / pooled["step"][1] < 2.0 ** 53      # the doubles hold the integers


def test_cells_left_out_change_no_other_group():
    c, codes, B = case("mod5")
    groups = np.where(np.isin(codes, (1, 4)), 9, codes)          # the cells to leave out form a level of their own ...
    full = gene_stats_by_group(csr(c), names(c), groups, levels=[0, 2, 3, 9])
    kept = gene_stats_by_group(csr(c), names(c), groups, levels=[0, 2, 3])      # ... or none
    assert list(kept["n_obs"]) == [52, 51, 51] and full["n_obs"][3] == 103
    assert all(np.array_equal(kept[k], full[k][:3], equal_nan=True) for k in KEYS)
    none = gene_stats_by_group(csr(c), names(c), groups, levels=[77])
    assert none["n_obs"][0] == 0 and not none["s1"].any() and not none["n_cells"].any() and np.all(np.isnan(none["mean"]))


# ---- 3. the bits depend on nothing but the matrix and the groups -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bits_do_not_depend_on_residence_slabs_order_or_numbering(dtype):
    c, codes, B = case("mod5")
    lv = np.arange(B)
    one = gene_stats_by_group(csr(c, dtype), names(c), codes, levels=lv)
    assert same(gene_stats_by_group(csr(c, dtype), names(c), codes, levels=lv), one)
    assert same(gene_stats_by_group(DeviceCSR(*csr(c, dtype)), names(c), codes, levels=lv), one)
    obj, h = capped_handle(SLAB_CAP)
    assert same(gene_stats_by_group(csr(c, dtype), names(c), codes, levels=lv, _handle=h), one)
    assert obj._scalar("project_slabs") >= 3 and int(np.diff(c["indptr"]).max()) * (4 + np.dtype(dtype).itemsize) > SLAB_CAP
    assert obj.timer("gene_stats_grouped") > 0
    perm = np.random.default_rng(2).permutation(codes.size)
    assert same(gene_stats_by_group(permuted(c, perm, dtype), names(c), codes[perm], levels=lv), one)
    renumber = np.array([3, 0, 4, 1, 2])                         # row i of the second call is level renumber[i]
    other = gene_stats_by_group(csr(c, dtype), names(c), codes, levels=renumber)
    assert all(np.array_equal(other[k], one[k][renumber], equal_nan=True) for k in KEYS)
    assert same(gene_stats_by_group(csr(c, dtype), names(c), codes, levels=renumber, _handle=h), other)      # ... in slabs too


# ---- 4. guards ---------------------------------------------------------------------------------------------------------------------------------------
def test_guard_on_device_resident_input():
    c, codes, B = case("mod5")
    data, indices, indptr, shp = csr(c)
    lv = np.arange(B)
    good = gene_stats_by_group(csr(c), names(c), codes, levels=lv)
    at, positive = int(indptr[5]) + 3, int(np.nonzero(data > 0)[0][10])

    def broken(name, where, value):
        a = dict(data=data.copy(), indices=indices.copy(), indptr=indptr.copy())
        a[name][where] = value
        return DeviceCSR(a["data"], a["indices"], a["indptr"], shp)

    for name, where, value, text in (("data", positive, -1.0, "negative"), ("indices", at, shp[1], "column index"), ("indices", at, -1, "column index")):
        with pytest.raises(HarmonyError, match=text) as e:
            gene_stats_by_group(broken(name, where, value), names(c), codes, levels=lv)
        assert "status 1" in str(e.value), str(e.value)
        assert same(gene_stats_by_group(DeviceCSR(data, indices, indptr, shp), names(c), codes, levels=lv), good)      # the process goes on, correctly
    bad = data.copy()
    bad[positive] = -2.0
    with pytest.raises(HarmonyError, match="negative"):          # a host-resident matrix: the same flag
        gene_stats_by_group((bad, indices, indptr, shp), names(c), codes, levels=lv)


def test_labels_and_limits_are_refused_on_the_host():
    c, codes, B = case("empty_level")
    data, indices, indptr, shp = csr(c)
    obj = Harmony()
    N, G = shp
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def call(labels, nb):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        rows = nb if 0 < nb <= 4096 else 1                      # (the outputs are [nb] and [nb][G])
        n_obs, n, s1, s2 = np.zeros(rows, np.int64), np.zeros((rows, G), np.int64), np.zeros((rows, G)), np.zeros((rows, G))
        st = obj._lib.hmx_gene_stats_grouped(obj._h, N, G, C.c_void_p(indptr.ctypes.data), C.c_void_p(indices.ctypes.data), C.c_void_p(data.ctypes.data),
                                             0, 0, 1e4, None, labels.ctypes.data_as(C.POINTER(C.c_int32)), nb, n_obs.ctypes.data_as(lp),
                                             n.ctypes.data_as(lp), s1.ctypes.data_as(dp), s2.ctypes.data_as(dp), None)
        return st, obj._lib.hmx_last_error(obj._h).decode(), n_obs

    lab = codes.copy()
    lab[6] = B
    st, msg, _ = call(lab, B)
    assert st == 1 and "cell 6" in msg and "[-1, B)" in msg
    lab[6], lab[2] = 0, -2
    st, msg, _ = call(lab, B)
    assert st == 1 and "cell 2" in msg
    assert call(codes, 0)[0] == 1 and call(codes, 4097)[0] == 7
    st, _, n_obs = call(codes, 4096)                            # (4096 groups of 70 genes: within 2^25)
    assert st == 0 and list(n_obs[:3]) == [9, 0, 8] and not n_obs[3:].any()
    with pytest.raises(ValueError, match="2\\^25"):
        gene_stats_by_group(np.ones((2, 1 << 14)), ["g%d" % g for g in range(1 << 14)], np.arange(2), levels=np.arange(2049))


# ---- 5. variable genes of a reference in two batches ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shifted():
    X, batch, genes_shifted = gr.shifted_batches(seed=21)
    a = gr.csr_of(X)
    return X, batch, genes_shifted, a, gr.group_stats(*a, batch, 2), gr.group_bars(*a, batch, 2)


def test_variable_genes_within_batches_leave_out_the_batch_genes():
    X, batch, genes_shifted, a, st, b = shifted()
    n_top = 100
    names_ = np.array(["gene%d" % g for g in range(X.shape[1])])
    # owed, not lucky: on the spec every pair of neighbours in a batch's ranking differs by more than their two bars (so the ranks are the same
    # for any variances within the bars), and at each batch's cut the gap exceeds twice the larger bar
    gaps = gr.rank_gaps(st["var"], b["var"], st["n_cells"], st["n_obs"])
    for k in range(2):
        o = np.argsort(-st["var"][k], kind="stable")
        cut = (st["var"][k, o[n_top - 1]] - st["var"][k, o[n_top]]) / (2.0 * max(b["var"][k, o[n_top - 1]], b["var"][k, o[n_top]]))
        print("batch %d: gap at the cut / (2 bar) = %.1f, smallest gap of neighbours / their bars = %.2f" % (k, cut, gaps[k]))
        assert cut > 1.0 and gaps[k] > 1.0
    want = gr.select(st["var"], st["n_cells"], st["n_obs"], n_top, "rank")
    got = variable_genes(X, names_, groups=batch, flavor="rank", n_top_genes=n_top)
    assert np.array_equal(got, want) and got.size == n_top
    union = variable_genes(X, names_, groups=batch, flavor="union", n_top_genes=n_top)
    assert np.array_equal(union, gr.select(st["var"], st["n_cells"], st["n_obs"], n_top, "union")) and np.all(np.diff(union) > 0)
    gs = gene_stats(X, names_)
    pooled = choose_genes(gs["var"], gs["n_cells"], n_top)
    assert np.array_equal(variable_genes(X, names_, n_top_genes=n_top), pooled)
    in_pooled, in_ranked = int(np.isin(pooled, genes_shifted).sum()), int(np.isin(got, genes_shifted).sum())
    print("of the %d shifted genes: %d among the pooled top %d, %d among the within-batch choice" % (genes_shifted.size, in_pooled, n_top, in_ranked))
    assert genes_shifted.size == 40 and in_pooled >= 30 and in_ranked < in_pooled
    L, pcs, ev = fit_loadings(X, names_, genes_use=names_[got], d=3)
    assert list(L.genes) == list(names_[got]) and pcs.shape == (X.shape[0], 3) and np.all(np.isfinite(pcs)) and np.all(ev > 0)


# ---- 6. marker genes of planted groups ------------------------------------------------------------------------------------------------------------------
def test_rank_genes_groups_finds_the_private_genes():
    X, lab, private = gr.private_genes()
    names_ = ["gene%d" % g for g in range(X.shape[1])]
    out = rank_genes_groups(X, names_, lab)
    assert list(out["levels"]) == [0, 1, 2, 3] and list(out["order"][:, 0]) == list(private)
    gs = gene_stats_by_group(X, names_, lab)
    again = markers_from_sums(gs["n_obs"], gs["n_cells"], gs["s1"], gs["s2"], step=gs["step"])
    assert all(np.array_equal(out[k], again[k], equal_nan=True) for k in again)
    a = gr.csr_of(X)
    Y, _ = pc.log_normalised(*a)
    want = gr.markers(Y, X, lab, 4)
    for b, g in enumerate(private):
        assert out["pct_in"][b, g] == 1.0 and out["pct_out"][b, g] == 0.0 and out["mean_out"][b, g] == 0.0
    np.testing.assert_allclose(out["mean_in"], want["mean_in"], rtol=1e-5, atol=1e-7)
    np.testing.assert_array_equal(out["pct_in"], want["pct_in"])
    one = rank_genes_groups(X, names_, lab, reference=1)
    ref = markers_from_sums(gs["n_obs"], gs["n_cells"], gs["s1"], gs["s2"], reference=1, step=gs["step"])
    assert all(np.array_equal(one[k], ref[k], equal_nan=True) for k in ref) and one["order"][0, 0] == private[0] and np.all(one["score"][1] == 0)
