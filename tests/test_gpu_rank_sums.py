"""Rank sums per group on the MI355X: hmx_rank_sums against the integer spec (tests/rank_sums_ref.py).  Every comparison is EXACT equality of n_obs,
n_pos, rank2 and tie3.  With caller-given totals = scale the rate is 1 and key = x, so a case chooses the key bits itself; S (the longest list
sorted in LDS) and C (the chunk of the radix sort and of the rank scans) are read from the handle, not copied.

The cases: one cell per group; a level no cell carries and cells left out; tie blocks of hundreds; lists of S - 1, S and S + 1 entries (distinct
keys, then all equal); a list of 3 C + 5 entries whose tie blocks straddle every chunk boundary, one of them longer than C, then keys that
differ only in their top byte, only in their bottom byte, and +inf keys; tie blocks of 1, 2, 63, 64 and 65; a gene-block budget that cuts the
genes into four blocks; a shuffled subset of the genes; residence, slabs, element type, unsorted rows, stored zeros and zero totals; 4096 groups;
determinism; the guards; markers end to end."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import group_stats_ref as gr  # noqa: E402
import rank_sums_ref as rr  # noqa: E402
from harmony_amd import (Harmony, HarmonyError, gene_stats_by_group, markers_from_sums, rank_genes_groups, rank_sums_by_group,  # noqa: E402
                         wilcoxon_from_rank_sums)
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = 1e4


@functools.lru_cache(maxsize=None)
def constants():
    obj = Harmony()
    return int(obj._scalar("ranksum_sort_lds")), int(obj._scalar("ranksum_chunk"))


def names(G):
    return ["g%d" % g for g in range(G)]


def csr(a):
    data, indices, indptr, G_all = a
    return (data, indices, indptr, (len(indptr) - 1, G_all))


def same(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in ("n_obs", "n_pos", "rank2")) and a["rank2"].dtype == np.int64
            and [int(t) for t in a["tie3"]] == [int(t) for t in b["tie3"]])


def check(a, codes, B, totals=None, device=False, **kw):
    """the library on the CSR arrays `a` == the spec; -> the library's dict"""
    got = rank_sums_by_group(DeviceCSR(*csr(a)) if device else csr(a), names(a[3]), codes, levels=np.arange(B), totals=totals, scale=SCALE, **kw)
    want = rr.rank_sums(*a, codes, B, scale=SCALE, totals=totals)
    assert same(got, want), {k: (got[k], want[k]) for k in ("n_obs", "n_pos", "rank2", "tie3") if not np.array_equal(got[k], want[k])}
    Nk = int((np.asarray(codes) >= 0).sum())
    assert np.all(got["rank2"].sum(0) == Nk * (Nk + 1))
    return got


def keyed(K, dtype=np.float32):
    """dense float32 keys [N, G] (0: no entry) -> (the CSR arrays, totals = scale: the rate is 1 and key = x)"""
    K = np.asarray(K, dtype=np.float32)
    return rr.csr_of_dense(K, dtype), np.full(K.shape[0], SCALE)


def counts(N, G, seed, lam=1.5):
    return np.random.default_rng(seed).poisson(lam, (N, G)).astype(np.float64)


# ---- 1 - 3: small shapes ---------------------------------------------------------------------------------------------------------------------------------
def test_one_cell_per_group():
    got = check(rr.csr_of_dense(np.array([[3.0, 0.0, 1.0], [1.0, 0.0, 1.0]])), np.array([0, 1]), 2)
    assert got["n_obs"].tolist() == [1, 1] and got["rank2"][:, 1].tolist() == [3, 3]


def test_a_level_no_cell_carries_and_cells_left_out():
    rng = np.random.default_rng(1)
    codes = rng.choice([0, 2], 17)
    codes[[3, 11]] = -1
    got = check(rr.csr_of_dense(counts(17, 70, 2)), codes, 3)
    assert got["n_obs"][1] == 0 and not got["rank2"][1].any() and got["n_obs"].sum() == 15


def tied_counts(N=257, G=40, seed=3):
    """every row a permutation of the same counts 0 .. 3: equal row totals, so a gene's keys form three tie blocks of dozens to hundreds"""
    rng = np.random.default_rng(seed)
    base = np.repeat([0.0, 1.0, 2.0, 3.0], G // 4)
    return np.stack([rng.permutation(base) for _ in range(N)])


def test_tie_blocks_of_hundreds():
    X = tied_counts()
    got = check(rr.csr_of_dense(X), np.arange(257) % 5, 5)
    assert min(int(t) for t in got["tie3"]) > 3 * 40 ** 3            # (three blocks of about 64 each)


# ---- 4: on both sides of the LDS sort's capacity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equal", [False, True])
def test_lists_of_one_below_at_and_one_above_the_lds_capacity(equal):
    S, _ = constants()
    N = S + 1
    rng = np.random.default_rng(4)
    K = np.zeros((N, 4), dtype=np.float32)
    for g, n in enumerate((S - 1, S, S + 1)):
        K[rng.permutation(N)[:n], g] = 2.0 if equal else rng.permutation(np.arange(1, n + 1)).astype(np.float32)
    a, tot = keyed(K)
    got = check(a, rng.integers(0, 2, N), 2, totals=tot)
    assert got["n_pos"].sum(0).tolist() == [S - 1, S, S + 1, 0]
    assert [int(t) for t in got["tie3"]] == ([(S - 1) ** 3, S ** 3, (S + 1) ** 3, 0] if equal else [S - 1, S, S + 1, 0])


# ---- 5: the radix path -----------------------------------------------------------------------------------------------------------------------------------
def long_case(values, seed=5, B=3):
    """one gene that every cell expresses with the given float32 keys, in a random order of the cells"""
    rng = np.random.default_rng(seed)
    v = np.asarray(values, dtype=np.float32)
    K = v[rng.permutation(v.size)].reshape(-1, 1)
    return keyed(K), rng.integers(0, B, v.size)


def test_tie_blocks_straddle_every_chunk_boundary_and_one_is_longer_than_a_chunk():
    S, C = constants()
    assert 3 * C + 5 > S
    blocks = [1] * (C - 2) + [5, C + 7] + [1] * (C - 12) + [4] + [1] * 3       # in sorted order: the blocks of 5, C + 7 and 4 lie across C, 2 C and 3 C
    assert sum(blocks) == 3 * C + 5
    ends = np.cumsum(blocks)
    for edge in (C, 2 * C, 3 * C):
        k = int(np.searchsorted(ends, edge, side="right"))
        assert ends[k] - blocks[k] < edge < ends[k] and blocks[k] > 1             # a tie block lies across the boundary
    values = np.repeat(np.arange(1, len(blocks) + 1, dtype=np.float32) * 0.5, blocks)
    (a, tot), codes = long_case(values)
    got = check(a, codes, 3, totals=tot)
    assert int(got["tie3"][0]) == sum(b ** 3 for b in blocks)


@pytest.mark.parametrize("kind", ["top_byte", "bottom_byte", "inf", "distinct"])
def test_every_radix_pass_matters(kind):
    S, C = constants()
    n = 3 * C + 5
    rng = np.random.default_rng(6)
    rate = 1.0
    if kind == "top_byte":
        bits = (rng.integers(1, 0x80, n).astype(np.uint32) << 24) | np.uint32(0x00123456)       # 0x01123456 .. 0x7f123456: finite, below 3e38
    elif kind == "bottom_byte":
        bits = np.uint32(0x3f800000) | rng.integers(0, 256, n).astype(np.uint32)
    elif kind == "distinct":
        bits = np.uint32(0x3f000000) + rng.permutation(1 << 22)[:n].astype(np.uint32) * np.uint32(37)      # all four bytes vary, no ties
    else:
        bits = np.uint32(0x7e800000) + rng.integers(0, 0x00e00000, n).astype(np.uint32)          # 8.5e37 .. 2.98e38, doubled by the rate: from 2^127 on +inf (3 in 7)
        rate = 2.0
    values = bits.view(np.float32)
    assert np.all(np.isfinite(values)) and np.all(values > 0) and np.all(values <= 3.0e38)
    (a, _), codes = long_case(values)
    tot = np.full(n, SCALE / rate)
    got = check(a, codes, 3, totals=tot)
    if kind == "inf":
        keys, pos, _ = rr.entry_keys(a[0], a[1], a[2], SCALE, tot)
        assert np.isinf(keys).sum() > C and np.all(pos) and int(got["tie3"][0]) >= int(np.isinf(keys).sum()) ** 3
    if kind == "distinct":
        assert int(got["tie3"][0]) == n


# ---- 6: tie blocks around the wave width -----------------------------------------------------------------------------------------------------------------
def test_tie_blocks_of_1_2_63_64_65():
    blocks = [1, 2, 63, 64, 65]
    values = np.repeat([1.5, 2.5, 3.5, 4.5, 5.5], blocks)
    K = np.zeros((sum(blocks) + 20, 1), dtype=np.float32)
    K[np.random.default_rng(7).permutation(K.shape[0])[:values.size], 0] = values
    a, tot = keyed(K)
    got = check(a, np.arange(K.shape[0]) % 2, 2, totals=tot)
    assert int(got["tie3"][0]) == sum(b ** 3 for b in blocks)


# ---- 7: gene blocks --------------------------------------------------------------------------------------------------------------------------------------
def test_gene_blocks_give_the_one_block_result():
    N, per_gene = 300, [100, 20, 20, 250, 30, 10]
    rng = np.random.default_rng(8)
    X = np.zeros((N, len(per_gene)))
    for g, n in enumerate(per_gene):
        X[rng.permutation(N)[:n], g] = rng.integers(1, 6, n)
    a, codes = rr.csr_of_dense(X), rng.integers(-1, 3, N)
    obj = Harmony()
    h = _ObjHandle(obj)
    one = check(a, codes, 3, _handle=h)
    assert obj._scalar("ranksum_blocks") == 1
    obj._set("ranksum_list_bytes", 16 * 60)                              # genes 0 and 3 exceed it on their own; 1 + 2 and 4 + 5 fit together
    cut = check(a, codes, 3, _handle=h)
    assert obj._scalar("ranksum_blocks") == 4 and same(cut, one)
    assert cut["n_pos"].sum(0).tolist() == [int((X[codes >= 0, g] > 0).sum()) for g in range(6)]
    obj._set("ranksum_list_bytes", 1)                                    # smaller than every gene: one block each
    assert same(check(a, codes, 3, _handle=h), one) and obj._scalar("ranksum_blocks") == 6
    assert obj.timer("rank_sums") > 0 and obj.timer("rank_sums_count") > 0 and obj.timer("rank_sums_fill") > 0 and obj.timer("rank_sums_sort") > 0


# ---- 8: a subset of the genes ----------------------------------------------------------------------------------------------------------------------------
def test_gene_slot_chooses_a_shuffled_subset():
    X, codes = counts(120, 30, 9), np.random.default_rng(9).integers(-1, 4, 120)
    a = rr.csr_of_dense(X)
    full = check(a, codes, 4)
    nm = np.array(names(30))
    ident = rank_sums_by_group(csr(a), nm, codes, levels=np.arange(4), genes_use=nm)
    assert same(ident, full)
    pick = np.random.default_rng(10).permutation(30)[:11]
    part = rank_sums_by_group(csr(a), nm, codes, levels=np.arange(4), genes_use=nm[pick])
    slot = np.full(30, -1)
    slot[pick] = np.arange(11)
    want = rr.rank_sums(*a, codes, 4, gene_slot=slot, G=11)
    assert same(part, want) and list(part["genes"]) == list(nm[pick])
    assert np.array_equal(part["rank2"], full["rank2"][:, pick]) and np.array_equal(part["n_pos"], full["n_pos"][:, pick])


# ---- 9: the bits do not depend on how the matrix arrives ---------------------------------------------------------------------------------------------------
def with_stored_zeros(X, rows):
    """CSR of X in which the given rows store EVERY gene, zeros included"""
    stored = X != 0
    stored[rows] = True
    indptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int64)
    return X[stored], np.nonzero(stored)[1].astype(np.int32), indptr, X.shape[1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bits_do_not_depend_on_residence_slabs_type_or_row_order(dtype):
    N, G, B = 257, 60, 4
    X = counts(N, G, 11)
    X[5] = 0.0                                                            # a row of stored zeros: its total is 0
    X[6] = 0.0                                                            # an empty row
    codes = np.random.default_rng(11).integers(-1, B, N)
    codes[[5, 6]] = 1
    data, indices, indptr, _ = with_stored_zeros(X, [5])
    assert indptr[6] - indptr[5] == G and indptr[7] == indptr[6]
    a = (data.astype(dtype), indices, indptr, G)
    one = check(a, codes, B)
    assert same(check(a, codes, B, device=True), one)
    obj = Harmony()
    obj._set("project_slab_bytes", 1500)
    assert same(check(a, codes, B, _handle=_ObjHandle(obj)), one) and obj._scalar("project_slabs") >= 3
    rev = rr.csr_of_dense(X, dtype, reverse_rows=True)                    # unsorted rows (and row 5 not stored at all: the same keys)
    assert np.any(np.diff(rev[1][rev[2][0]:rev[2][1]]) < 0) and same(check(rev, codes, B), one) and same(check(rev, codes, B, device=True), one)
    other = np.float64 if dtype == np.float32 else np.float32
    assert same(check((data.astype(other), indices, indptr, G), codes, B), one)
    tot = np.random.default_rng(12).uniform(200.0, 3000.0, N)
    tot[3] = 0.0                                                          # a caller's zero total: the cell has no positive key
    given = check(a, codes, B, totals=tot)
    assert same(check(a, codes, B, totals=tot, device=True), given) and not same(given, one)


# ---- 10: many groups -------------------------------------------------------------------------------------------------------------------------------------
def test_4096_groups():
    rng = np.random.default_rng(13)
    codes = rng.integers(0, 4096, 5000)
    got = check(rr.csr_of_dense(counts(5000, 3, 13, lam=0.8)), codes, 4096)
    assert got["rank2"].shape == (4096, 3) and got["n_obs"].max() >= 3


# ---- 11, 12: determinism; the counts of expressing cells ---------------------------------------------------------------------------------------------------
def test_determinism_permutation_and_renumbering():
    X, codes = tied_counts(200, 24, 14), np.random.default_rng(14).integers(-1, 5, 200)
    a = rr.csr_of_dense(X)
    one = check(a, codes, 5)
    assert same(check(a, codes, 5), one)
    perm = np.random.default_rng(15).permutation(200)
    assert same(check(rr.csr_of_dense(X[perm]), codes[perm], 5), one)
    renumber = np.array([3, 0, 4, 1, 2])                                 # row i of the second call is level renumber[i]
    other = rank_sums_by_group(csr(a), names(24), codes, levels=renumber)
    assert all(np.array_equal(other[k], one[k][renumber]) for k in ("n_obs", "n_pos", "rank2")) and list(other["tie3"]) == list(one["tie3"])


def test_n_pos_is_the_grouped_statistics_n_cells():
    X, codes = counts(300, 50, 16), np.random.default_rng(16).integers(-1, 6, 300)
    a = rr.csr_of_dense(X)
    got = check(a, codes, 6)
    gs = gene_stats_by_group(csr(a), names(50), codes, levels=np.arange(6))
    assert np.array_equal(got["n_pos"], gs["n_cells"]) and np.array_equal(got["n_obs"], gs["n_obs"])


# ---- 13: guards ------------------------------------------------------------------------------------------------------------------------------------------
def test_guard_on_device_resident_input():
    X, codes = counts(100, 20, 17), np.arange(100) % 3
    data, indices, indptr, G = rr.csr_of_dense(X)
    good = check((data, indices, indptr, G), codes, 3, device=True)
    at = int(indptr[5]) + 2

    def broken(name, where, value):
        a = dict(data=data.copy(), indices=indices.copy(), indptr=indptr.copy())
        a[name][where] = value
        return DeviceCSR(a["data"], a["indices"], a["indptr"], (100, G))

    for name, where, value, text in (("data", at, -1.0, "negative"), ("indices", at, G, "column index"), ("indices", at, -1, "column index")):
        with pytest.raises(HarmonyError, match=text) as e:
            rank_sums_by_group(broken(name, where, value), names(G), codes, levels=np.arange(3))
        assert "status 1" in str(e.value), str(e.value)
        assert same(check((data, indices, indptr, G), codes, 3, device=True), good)      # the process goes on, correctly


# ---- 14: markers end to end ------------------------------------------------------------------------------------------------------------------------------
def test_wilcoxon_markers_find_the_private_genes():
    X, lab, private = gr.private_genes()
    names_ = ["gene%d" % g for g in range(X.shape[1])]
    out = rank_genes_groups(X, names_, lab, method="wilcoxon")
    assert list(out["levels"]) == [0, 1, 2, 3] and list(out["order"][:, 0]) == list(private)
    again = wilcoxon_from_rank_sums(out["n_obs"], out["n_pos"], out["rank2"], out["tie3"])
    assert all(np.array_equal(out[k], again[k], equal_nan=True) for k in ("u", "auc", "score", "order"))
    want = rr.rank_sums(*gr.csr_of(X), lab, 4)
    assert same(dict(n_obs=out["n_obs"], n_pos=out["n_pos"], rank2=out["rank2"], tie3=out["tie3"]), want)
    for b, g in enumerate(private):
        assert out["auc"][b, g] == 1.0 and out["pct_in"][b, g] == 1.0 and out["pct_out"][b, g] == 0.0
    # the default is the t-test it was: markers_from_sums on the grouped sums, and its means are the Wilcoxon call's too
    gs = gene_stats_by_group(X, names_, lab)
    ttest, default = markers_from_sums(gs["n_obs"], gs["n_cells"], gs["s1"], gs["s2"], step=gs["step"]), rank_genes_groups(X, names_, lab)
    assert all(np.array_equal(default[k], ttest[k], equal_nan=True) for k in ttest) and sorted(default) == sorted(list(ttest) + ["levels", "n_obs"])
    assert all(np.array_equal(out[k], ttest[k], equal_nan=True) for k in ("mean_in", "mean_out", "pct_in", "pct_out", "logfoldchange")) and "df" not in out
    # one level against another: the two groups' cells alone
    one = rank_genes_groups(X, names_, lab, reference=1, method="wilcoxon")
    pair = np.where(lab == 0, 0, np.where(lab == 1, 1, -1))
    w = rr.rank_sums(*gr.csr_of(X), pair, 2)
    u, auc, score = rr.wilcoxon(w["n_obs"], w["n_pos"], w["rank2"], w["tie3"])
    assert np.array_equal(one["rank2"][0], w["rank2"][0]) and np.array_equal(one["u"][0], u[0])
    np.testing.assert_allclose(one["score"][0], score[0], rtol=1e-13, atol=0)
    assert one["order"][0, 0] == private[0] and np.all(one["score"][1] == 0) and np.all(one["auc"][1] == 0.5)
