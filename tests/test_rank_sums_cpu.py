"""The rank sums per group held to their spec (tests/rank_sums_ref.py) without a GPU: the header, the library and the binding agree; the spec's
integers equal a brute-force pair count, scipy's midranks and scipy's U; the pure test arithmetic equals scipy's asymptotic Mann-Whitney test
through the p-value of the score; the plan (hmx_ranksum_plan.h, through tests/cpp/ranksum_plan_probe.cpp) puts every selected gene in exactly
one block within the budget; the argument errors need no device; rank_genes_groups without `method` is what it was
(tests/test_gpu_rank_sums.py runs the library)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import rank_sums_ref as rr  # noqa: E402
from harmony_amd import _lib  # noqa: E402
from harmony_amd import rank_genes_groups, rank_sums_by_group, wilcoxon_from_rank_sums  # noqa: E402

def test_ranksum_header_matches_the_library_and_the_binding():
    assert helpers.header_names("harmony_mi355x_ranksum.h") == set(_lib.RANKSUM_SIGNATURES) == {"hmx_rank_sums"}
    found = helpers.header_functions("harmony_mi355x_ranksum.h")
    assert [n for n, _ in found] == ["hmx_rank_sums"] and len(found[0][1]) == 18
    helpers.assert_header_stands_alone("harmony_mi355x_ranksum.h", ["hmx_rank_sums"])
    loose = {"const int32_t*": (C.POINTER(C.c_int32), C.c_void_p), "const int64_t*": (C.c_void_p,)}      # (the count matrix: host or device pointers)
    helpers.assert_binding_matches(_lib.load(), "hmx_rank_sums", found[0][1], _lib.RANKSUM_SIGNATURES["hmx_rank_sums"][1], loose)
    mine = re.findall(r"int hmx_rank_sums\(([^)]*)\)", helpers.header_text("harmony_mi355x_ranksum.h"))[0]
    args = [a.split() for a in mine.replace("\n", " ").split(",")]
    # hmx_gene_stats_grouped's arguments up to `labels, B`, then gene_slot, G and the four outputs
    grouped = helpers.header_text("harmony_mi355x_groups.h")
    gargs = [a.split() for a in re.findall(r"int hmx_gene_stats_grouped\(([^)]*)\)", grouped)[0].replace("\n", " ").split(",")]
    assert args[:12] == gargs[:12] and [a[-1] for a in args[12:]] == ["gene_slot", "G", "n_obs", "n_pos", "rank2", "tie3"]


# ---- the spec's integers ---------------------------------------------------------------------------------------------------------------------------
def small_case(seed, N=120, G=7, B=3, left_out=9):
    """counts with ties (small integers), a gene nobody expresses (0), a gene that is one tie block under equal totals (1); some cells left out"""
    rng = np.random.default_rng(seed)
    X = rng.poisson(1.2, (N, G)).astype(np.float64)
    X[:, 0] = 0.0
    X[:, 1] = 3.0
    codes = rng.integers(0, B, N)
    codes[rng.permutation(N)[:left_out]] = -1
    return X, codes.astype(np.int32), B


@pytest.mark.parametrize("seed,totals", [(0, None), (1, "equal"), (2, "random"), (3, None)])
def test_spec_equals_a_brute_force_pair_count(seed, totals):
    X, codes, B = small_case(seed, N=300 if seed == 3 else 120)
    a = rr.csr_of_dense(X, np.float64 if seed % 2 else np.float32)
    tot = None if totals is None else (np.full(X.shape[0], 1e4) if totals == "equal" else np.random.default_rng(9).uniform(50.0, 5e4, X.shape[0]))
    got = rr.rank_sums(*a, codes, B, totals=tot)
    n_obs, n_pos, rank2, tie3 = rr.rank_sums_brute(rr.dense_keys(*a, totals=tot), codes, B)
    assert np.array_equal(got["n_obs"], n_obs) and np.array_equal(got["n_pos"], n_pos) and np.array_equal(got["rank2"], rank2)
    assert list(got["tie3"]) == list(tie3)
    Nk = int((codes >= 0).sum())
    assert np.all(got["rank2"].sum(0) == Nk * (Nk + 1))                      # the midranks of N_k cells add up to N_k (N_k + 1) / 2
    assert not got["n_pos"][:, 0].any() and got["tie3"][0] == 0 and np.all(got["rank2"][:, 0] == n_obs * (Nk + 1))      # the gene nobody expresses
    if totals == "equal":
        assert got["tie3"][1] == Nk ** 3 and np.all(got["rank2"][:, 1] == n_obs * (Nk + 1))      # one tie block


def test_spec_selects_genes_through_gene_slot():
    X, codes, B = small_case(4)
    a = rr.csr_of_dense(X)
    full = rr.rank_sums(*a, codes, B)
    slot = np.array([-1, 2, -1, 0, -1, 1, -1], dtype=np.int32)               # output rows 0, 1, 2 = genes 3, 5, 1
    part = rr.rank_sums(*a, codes, B, gene_slot=slot, G=3)
    for k in ("n_pos", "rank2"):
        assert np.array_equal(part[k], full[k][:, [3, 5, 1]])
    assert list(part["tie3"]) == [full["tie3"][g] for g in (3, 5, 1)] and np.array_equal(part["n_obs"], full["n_obs"])


def scipy_stats():
    try:
        import scipy.stats as st
    except ImportError:
        pytest.skip("scipy does not import")
    return st


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_spec_equals_scipy_midranks_and_u(seed):
    st = scipy_stats()
    X, codes, B = small_case(seed, N=232 + 9)
    a = rr.csr_of_dense(X)
    got = rr.rank_sums(*a, codes, B)
    K = rr.dense_keys(*a)[codes >= 0].astype(np.float64)
    c = codes[codes >= 0]
    u, _, _ = rr.wilcoxon(got["n_obs"], got["n_pos"], got["rank2"], got["tie3"])
    for g in range(X.shape[1]):
        twice = 2.0 * st.rankdata(K[:, g], method="average")
        assert np.all(twice == np.round(twice))
        for b in range(B):
            assert got["rank2"][b, g] == int(twice[c == b].sum())
            assert u[b, g] == st.mannwhitneyu(K[c == b, g], K[c != b, g], use_continuity=False, method="asymptotic").statistic


# ---- the test arithmetic ---------------------------------------------------------------------------------------------------------------------------
def check_against_scipy(X, codes, B):
    st = scipy_stats()
    a = rr.csr_of_dense(X)
    s = rr.rank_sums(*a, codes, B)
    out = wilcoxon_from_rank_sums(s["n_obs"], s["n_pos"], s["rank2"], s["tie3"])
    u, auc, score = rr.wilcoxon(s["n_obs"], s["n_pos"], s["rank2"], s["tie3"])
    np.testing.assert_array_equal(out["u"], u)
    np.testing.assert_allclose(out["auc"], auc, rtol=1e-15, atol=0, equal_nan=True)
    np.testing.assert_allclose(out["score"], score, rtol=1e-13, atol=0, equal_nan=True)
    assert np.array_equal(out["order"], np.argsort(-out["score"], axis=1, kind="stable"))
    K = rr.dense_keys(*a)[codes >= 0].astype(np.float64)
    c = codes[codes >= 0]
    seen = 0
    for b in range(B):
        n1, n2 = int((c == b).sum()), int((c != b).sum())
        for g in range(X.shape[1]):
            if n1 == 0 or n2 == 0:
                assert np.isnan(out["score"][b, g]) and np.isnan(out["auc"][b, g])
                continue
            if np.all(K[:, g] == K[0, g]):                                # zero variance: score 0 by definition (scipy divides 0 by 0)
                assert out["score"][b, g] == 0.0 and out["auc"][b, g] == 0.5
                continue
            ref = st.mannwhitneyu(K[c == b, g], K[c != b, g], use_continuity=False, method="asymptotic")
            assert out["u"][b, g] == ref.statistic
            np.testing.assert_allclose(2.0 * st.norm.sf(abs(out["score"][b, g])), ref.pvalue, rtol=1e-12, atol=0)
            seen += 1
    return out, seen


def test_wilcoxon_equals_scipy_asymptotic_test():
    X, codes, B = small_case(5, N=241)                                       # 232 kept cells, three groups, seven genes, ties throughout
    assert int((codes >= 0).sum()) == 232
    out, seen = check_against_scipy(X, codes, B)
    assert seen == 3 * 6 and np.all(out["score"][:, 0] == 0)                 # (gene 0 nobody expresses: zero variance; the six others all vary)
    # without the tie term: scanpy's default, never a smaller variance
    a = rr.csr_of_dense(X)
    s = rr.rank_sums(*a, codes, B)
    plain = wilcoxon_from_rank_sums(s["n_obs"], s["n_pos"], s["rank2"], s["tie3"], tie_correct=False)
    _, _, want = rr.wilcoxon(s["n_obs"], s["n_pos"], s["rank2"], s["tie3"], tie_correct=False)
    np.testing.assert_allclose(plain["score"], want, rtol=1e-13, atol=0, equal_nan=True)
    assert np.all(np.abs(plain["score"]) <= np.abs(out["score"]) + 1e-12)


def test_wilcoxon_one_tie_block_a_group_of_one_and_a_single_group():
    rng = np.random.default_rng(6)
    X = rng.poisson(2.0, (40, 5)).astype(np.float64)
    X[:, 0] = 0.0
    X[:, 1] = 2.0
    codes = np.repeat([0, 1, 2], [1, 19, 20]).astype(np.int32)               # a group of one cell
    out, seen = check_against_scipy(X, codes, 3)
    assert seen >= 3 * 3
    tot = np.full(40, 1e4)
    s = rr.rank_sums(*rr.csr_of_dense(X), codes, 3, totals=tot)              # equal totals: gene 1 is ONE tie block
    w = wilcoxon_from_rank_sums(s["n_obs"], s["n_pos"], s["rank2"], s["tie3"])
    assert s["tie3"][1] == 40 ** 3 and np.all(w["score"][:, 1] == 0) and np.all(w["auc"][:, 1] == 0.5) and np.all(w["score"][:, 0] == 0)
    one = rr.rank_sums(*rr.csr_of_dense(X), np.zeros(40, dtype=np.int32), 1)      # B = 1: no other cells
    w = wilcoxon_from_rank_sums(one["n_obs"], one["n_pos"], one["rank2"], one["tie3"])
    assert np.all(np.isnan(w["score"])) and np.all(np.isnan(w["auc"])) and np.all(one["rank2"] == 40 * 41)
    empty = rr.rank_sums(*rr.csr_of_dense(X), np.where(codes == 1, 0, 2).astype(np.int32), 3)      # a level no cell carries
    w = wilcoxon_from_rank_sums(empty["n_obs"], empty["n_pos"], empty["rank2"], empty["tie3"])
    assert np.all(np.isnan(w["score"][1])) and not np.any(np.isnan(w["score"][[0, 2]])) and np.all(w["order"][1] == np.arange(5))
    with pytest.raises(ValueError, match="do not agree"):
        wilcoxon_from_rank_sums([1, 2], np.zeros((3, 2)), np.zeros((3, 2)), [0, 0])
    with pytest.raises(ValueError, match="one integer per gene"):
        wilcoxon_from_rank_sums([1, 2], np.zeros((2, 2)), np.zeros((2, 2)), [0])


def test_tie_term_is_exact_beyond_64_bits():
    """N_k = 2^22 cells in one tie block: t^3 = 2^66 arrives as two words and is used as a Python integer"""
    Nk = 1 << 22
    n_obs = np.array([Nk // 2, Nk // 2])
    rank2 = (n_obs * (Nk + 1)).reshape(2, 1)
    w = wilcoxon_from_rank_sums(n_obs, n_obs.reshape(2, 1), rank2, [Nk ** 3])
    assert np.all(w["score"] == 0) and np.all(w["auc"] == 0.5)
    w = wilcoxon_from_rank_sums(n_obs, n_obs.reshape(2, 1), rank2, [Nk ** 3 - 6])      # a tie term just below: a positive variance, rank sums in balance
    assert np.all(np.isfinite(w["score"])) and np.all(w["score"] == 0)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------------------
_probe = []


def plan_probe():
    if not _probe:
        so = os.path.join(tempfile.mkdtemp(prefix="ranksum_plan_probe_"), "ranksum_plan_probe.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared",
                               os.path.join(ROOT, "tests", "cpp", "ranksum_plan_probe.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.probe_ranksum_plan.restype = C.c_longlong
        _probe.append(lib)
    return _probe[0]


def plan(count, budget, sort_lds=8):
    count = np.ascontiguousarray(count, dtype=np.int64)
    G = count.size
    seg, block, first = np.zeros(G + 1, np.int64), np.full(G + 1, -7, np.int32), np.full(G + 1, -7, np.int64)
    path, order = np.zeros(G, np.uint8), np.full(G, -7, np.int32)
    norder, biggest = C.c_longlong(0), C.c_longlong(0)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = plan_probe().probe_ranksum_plan(P(count), C.c_int(G), C.c_longlong(budget), C.c_longlong(sort_lds), P(seg), P(block), P(path), P(order), P(first),
                                        C.byref(norder), C.byref(biggest))
    if n < 0:
        return n
    return seg, block[:n + 1], path, order[:norder.value], first[:n + 1], biggest.value


COUNTS = {"mixed": [5, 0, 0, 9, 1, 8, 0, 30, 2, 2, 0], "empty_first_and_last": [0, 0, 4, 4, 0], "all_empty": [0, 0, 0], "one": [7], "equal": [4, 4, 4, 4, 4, 4]}


@pytest.mark.parametrize("budget", [0, 15, 16, 16 * 4, 16 * 8, 16 * 9, 16 * 10, 16 * 12, 16 * 30, 16 * 57, 1 << 40])
@pytest.mark.parametrize("kind", sorted(COUNTS))
def test_plan_puts_every_gene_in_exactly_one_block_within_the_budget(kind, budget):
    count = np.array(COUNTS[kind], dtype=np.int64)
    G = count.size
    seg, block, path, order, first, biggest = plan(count, budget)
    assert np.array_equal(seg, np.concatenate([[0], np.cumsum(count)]))
    assert block[0] == 0 and block[-1] == G and np.all(np.diff(block) >= 1)      # contiguous runs: every gene in exactly one block, no block empty
    assert np.array_equal(path, np.where(count == 0, 0, np.where(count <= 8, 1, 2)))
    entries = seg[block[1:]] - seg[block[:-1]]
    assert biggest == entries.max()
    for k in range(block.size - 1):
        genes = np.arange(block[k], block[k + 1])
        with_entries = genes[count[genes] > 0]
        assert 16 * entries[k] <= budget or with_entries.size <= 1             # within the budget unless a single gene exceeds it
        if k + 2 < block.size:                                                   # greedy: the next gene would not have fitted
            assert 16 * (entries[k] + count[block[k + 1]]) > budget
        mine = order[first[k]:first[k + 1]]
        assert sorted(mine.tolist()) == with_entries.tolist()                    # the block's genes with entries, each once ...
        assert mine.tolist() == sorted(with_entries.tolist(), key=lambda g: (-count[g], g))      # ... the longest first, ties by gene
    assert first[0] == 0 and first[-1] == order.size == int((count > 0).sum())
    if budget == 0 or budget == 15:                                              # a budget smaller than every gene
        assert np.all(np.diff(block)[:-1] >= 1) and all(int((count[block[k]:block[k + 1]] > 0).sum()) <= 1 for k in range(block.size - 1))
    if budget >= 16 * count.sum():
        assert block.size == 2


def test_plan_cuts_after_every_gene_and_refuses_a_negative_count():
    seg, block, path, order, first, biggest = plan([4, 4, 4, 4, 4, 4], 16 * 4)   # the budget of exactly one gene: a cut after every gene
    assert block.tolist() == [0, 1, 2, 3, 4, 5, 6] and biggest == 4
    seg, block, path, order, first, biggest = plan([4, 4, 4, 4, 4, 4], 16 * 8)
    assert block.tolist() == [0, 2, 4, 6] and order.tolist() == [0, 1, 2, 3, 4, 5]
    assert plan([3, -1, 2], 1 << 20) == -1 - 1


# ---- argument errors that need no device -------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_handle():
    X, genes = np.ones((3, 2)), ["a", "b"]
    with pytest.raises(ValueError, match="one label per cell"):
        rank_sums_by_group(X, genes, [0, 1])
    with pytest.raises(ValueError, match="no levels"):
        rank_sums_by_group(X, genes, [0, 1, 1], levels=[])
    with pytest.raises(ValueError, match="distinct"):
        rank_sums_by_group(X, genes, [0, 1, 1], genes_use=["a", "a"])
    with pytest.raises(ValueError, match="not among genes"):
        rank_sums_by_group(X, genes, [0, 1, 1], genes_use=["c"])
    with pytest.raises(ValueError, match="selects no gene"):
        rank_sums_by_group(X, genes, [0, 1, 1], genes_use=[])
    with pytest.raises(ValueError, match="scale"):
        rank_sums_by_group(X, genes, [0, 1, 1], scale=0.0)
    with pytest.raises(ValueError, match="2\\^25"):
        rank_sums_by_group(np.ones((2, 1 << 14)), ["g%d" % g for g in range(1 << 14)], np.arange(2), levels=np.arange(2049))
    with pytest.raises(ValueError, match="method"):
        rank_genes_groups(X, genes, [0, 1, 1], method="logreg")
    with pytest.raises(ValueError, match="reference"):
        rank_genes_groups(X, genes, [0, 1, 1], reference=2, method="wilcoxon")


def test_library_refuses_arguments_and_limits_without_a_device():
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    N, G_all = 4, 3
    indptr, indices, data = np.array([0, 1, 2, 3, 3], np.int64), np.array([0, 1, 2], np.int32), np.ones(3)
    dp, ip, lp, up = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)

    def call(labels, B, slot, G, N=N):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        rows, cols = (B if 0 < B <= 4096 else 1), max(G, 1)
        n_obs, n_pos, rank2, tie = np.zeros(rows, np.int64), np.zeros((rows, cols), np.int64), np.zeros((rows, cols), np.int64), np.zeros((cols, 2), np.uint64)
        slot = None if slot is None else np.ascontiguousarray(slot, dtype=np.int32)
        st = lib.hmx_rank_sums(h, N, G_all, C.c_void_p(indptr.ctypes.data), C.c_void_p(indices.ctypes.data), C.c_void_p(data.ctypes.data), 0, 0, 1e4, None,
                               labels.ctypes.data_as(ip), B, None if slot is None else slot.ctypes.data_as(ip), G,
                               n_obs.ctypes.data_as(lp), n_pos.ctypes.data_as(lp), rank2.ctypes.data_as(lp), tie.ctypes.data_as(up))
        return st, lib.hmx_last_error(h).decode()

    try:
        ARG, LIMIT = 1, 7
        st, msg = call([0, 1, 2, 1], 2, None, 3)
        assert st == ARG and "cell 2" in msg and "[-1, B)" in msg
        st, msg = call([0, -2, 1, 1], 2, None, 3)
        assert st == ARG and "cell 1" in msg
        assert call([0, 1, 0, 1], 0, None, 3)[0] == ARG and call([0, 1, 0, 1], 2, None, 0)[0] == ARG
        assert call([0, 1, 0, 1], 4097, None, 3)[0] == LIMIT
        st, msg = call([0, 1, 0, 1], 2, None, 2)                         # NULL selects every gene
        assert st == ARG and "G_all" in msg
        st, msg = call([0, 1, 0, 1], 2, [0, 2, -1], 2)
        assert st == ARG and "gene_slot[1]" in msg
        st, msg = call([0, 1, 0, 1], 2, [0, -2, -1], 2)
        assert st == ARG and "gene_slot[1]" in msg
        st, msg = call([0, 1, 0, 1], 2, [1, -1, 1], 2)
        assert st == ARG and "two genes" in msg
        st, msg = call([0, 1, 0, 1], 2, [1, -1, 0], 2)                   # nothing left to refuse: the call reaches for a device
        assert st != ARG and st != LIMIT or "device" in msg.lower()
        out = (C.c_double * 1)()
        assert lib.hmx_set_int(h, b"ranksum_list_bytes", 1 << 20) == 0 and lib.hmx_set_int(h, b"ranksum_list_bytes", -1) == ARG
        assert lib.hmx_get(h, b"ranksum_sort_lds", out, 1) == 1 and out[0] >= 64 and int(out[0]) & (int(out[0]) - 1) == 0
        assert lib.hmx_get(h, b"ranksum_chunk", out, 1) == 1 and out[0] >= 64
        assert lib.hmx_get(h, b"ranksum_blocks", out, 1) == 1 and out[0] == 0
    finally:
        lib.hmx_destroy(h)


def test_rank_genes_groups_keeps_its_default():
    sig = inspect.signature(rank_genes_groups)
    assert list(sig.parameters)[-1] == "method" and sig.parameters["method"].default == "t-test"
    assert list(sig.parameters)[:-1] == ["counts", "genes", "groups", "levels", "reference", "scale", "totals", "device", "_handle"]
