"""The grouped gene statistics held to their spec (tests/group_stats_ref.py) without a GPU: the header, the library and the binding agree; the
derived bars per (group, gene) are neither violated by honest float32 nor more than ten times what it does; the marker arithmetic from sums
equals the dense formulas; the selection rules equal the spec on hand-made variances with ties; the work list (hmx_group_plan.h, through
tests/cpp/group_plan_probe.cpp) covers every kept cell exactly once; the argument errors need no device (tests/test_gpu_group_stats.py runs it)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import group_stats_ref as gr  # noqa: E402
import helpers  # noqa: E402
from harmony_amd import _lib  # noqa: E402
from harmony_amd import gene_stats_by_group, markers_from_sums, rank_genes_groups, variable_genes  # noqa: E402
from harmony_amd.group_stats import select_variable_genes  # noqa: E402


def test_groups_header_matches_the_library_and_the_binding():
    assert helpers.header_names("harmony_mi355x_groups.h") == set(_lib.GROUPS_SIGNATURES) == {"hmx_gene_stats_grouped"}
    found = helpers.header_functions("harmony_mi355x_groups.h")
    assert [n for n, _ in found] == ["hmx_gene_stats_grouped"] and len(found[0][1]) == 17
    helpers.assert_header_stands_alone("harmony_mi355x_groups.h", ["hmx_gene_stats_grouped"])
    loose = {"const int32_t*": (C.POINTER(C.c_int32), C.c_void_p), "const int64_t*": (C.c_void_p,)}      # (the count matrix: host or device pointers)
    helpers.assert_binding_matches(_lib.load(), "hmx_gene_stats_grouped", found[0][1], _lib.GROUPS_SIGNATURES["hmx_gene_stats_grouped"][1], loose)


def A(c):
    return c["data"], c["indices"], c["indptr"], c["G_all"]


@functools.lru_cache(maxsize=None)
def sweep_ratios(name):
    """worst |honest fp32 - spec| / bar of one case: s1, s2, var"""
    c, codes, B = gr.group_case(name)
    st, sf, b = gr.group_stats(*A(c), codes, B), gr.group_stats_fp32(*A(c), codes, B), gr.group_bars(*A(c), codes, B)
    assert np.array_equal(st["n_cells"], sf["n_cells"]) and np.array_equal(st["n_obs"], sf["n_obs"])
    has = b["s1"] > 0
    assert np.all(sf["s1"][~has] == 0) and np.all(sf["s2"][~has] == 0)
    out = {k: float((np.abs(sf[k] - st[k])[has] / b[k][has]).max()) if has.any() else 0.0 for k in ("s1", "s2")}
    hv = has & np.isfinite(b["var"])
    assert np.array_equal(np.isnan(st["var"]), np.isnan(b["var"])) and np.array_equal(np.isnan(st["var"]), np.isnan(sf["var"]))
    out["var"] = float((np.abs(sf["var"] - st["var"])[hv] / b["var"][hv]).max()) if hv.any() else 0.0
    return out


@pytest.mark.parametrize("name", gr.CASES)
def test_honest_fp32_stays_within_every_group_bar(name):
    r = sweep_ratios(name)
    print("group bars %s: honest fp32 / bar = %s" % (name, {k: round(v, 3) for k, v in r.items()}))
    assert all(v <= 1.0 for v in r.values()), r


def test_no_group_bar_is_looser_than_ten_times_honest_fp32():
    worst = {k: max(sweep_ratios(n)[k] for n in gr.CASES) for k in ("s1", "s2", "var")}
    print("group bars, worst honest fp32 / bar over the sweep: %s" % {k: round(v, 3) for k, v in worst.items()})
    assert all(v >= 0.1 for v in worst.values()), worst


def test_cases_carry_their_edges():
    sizes = {}
    for name in gr.CASES:
        c, codes, B = gr.group_case(name)
        assert codes.size == len(c["indptr"]) - 1 and codes.min() >= 0 and codes.max() < B
        sizes[name] = np.bincount(codes, minlength=B).tolist()
    assert sizes["one_each"] == [1, 1] and sizes["empty_level"][1] == 0 and sizes["16_17"] == [16, 17]
    assert [sizes[n] for n in ("chunk-1", "chunk", "chunk+1")] == [[gr.CHUNK - 1, 1], [gr.CHUNK, 1], [gr.CHUNK + 1, 1]]
    c, codes, _ = gr.group_case("two_ranges")
    assert c["G_all"] > gr.STAT_GENES and all(np.any((c["indices"] == g) & (c["data"] > 0)) for g in gr.EDGE_GENES)
    ip = c["indptr"]
    assert all(len(set(c["indices"][ip[i]:ip[i + 1]].tolist())) == ip[i + 1] - ip[i] for i in range(codes.size))      # no gene twice in a row
    assert list(np.diff(ip)[:6]) == [0, 1, 63, 64, 65, 200]


# ---- markers from sums -----------------------------------------------------------------------------------------------------------------------------
def hand_made(sizes, left_out=1, seed=0):
    """dense Y of exactly representable values (so the sums are exact), X its support; genes: 0 expressed nowhere, 1 the same value in every cell of
    group 0 and nowhere else, 2 the same value everywhere, the rest random"""
    rng = np.random.default_rng(seed)
    codes = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), -np.ones(left_out, dtype=np.int64)])
    codes = codes[rng.permutation(codes.size)]
    Y = rng.integers(0, 16, (codes.size, 7)) / 8.0
    Y[:, 0] = 0.0
    Y[:, 1] = np.where(codes == 0, 1.5, 0.0)
    Y[:, 2] = 0.75
    return Y, (Y > 0).astype(np.float64), codes


def sums(Y, X, codes, B):
    return (np.bincount(codes[codes >= 0], minlength=B), np.stack([(X[codes == b] > 0).sum(0) for b in range(B)]),
            np.stack([Y[codes == b].sum(0) for b in range(B)]), np.stack([(Y[codes == b] ** 2).sum(0) for b in range(B)]))


@pytest.mark.parametrize("sizes,reference", [((4, 5, 6), "rest"), ((4, 5, 6), 2), ((4, 5, 6), 0), ((5, 1), "rest"), ((4, 1, 3, 0), "rest"), ((4, 1, 3, 0), 1)])
def test_markers_from_sums_equal_the_dense_formulas(sizes, reference):
    Y, X, codes = hand_made(sizes)
    B = len(sizes)
    got, want = markers_from_sums(*sums(Y, X, codes, B), reference=reference), gr.markers(Y, X, codes, B, reference)
    for k in ("mean_in", "mean_out", "pct_in", "pct_out", "logfoldchange", "score", "df"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=0, equal_nan=True, err_msg=k)
    assert np.array_equal(got["order"], want["order"])
    s = want["score"]
    few = np.array(sizes) < 2
    other_few = (sum(sizes) - np.array(sizes) < 2) if reference == "rest" else np.full(B, sizes[reference] < 2)
    assert np.all(np.isnan(s[few | other_few])) and np.all(np.isnan(got["df"][few | other_few]))
    ok = np.nonzero(~(few | other_few))[0]
    assert np.all(s[ok, 0] == 0) and np.all(s[ok, 2] == 0)                        # zero denominators, equal means
    if 0 in ok and reference != 0:
        assert s[0, 1] == np.inf and got["score"][0, 1] == np.inf                 # ... and unequal ones
    if reference == 0:
        assert np.all(got["score"][ok[ok != 0], 1] == -np.inf)
    # the exact-subtraction check: with the steps given and sums beyond 2^53 steps the integer path gives the same answer
    again = markers_from_sums(*sums(Y, X, codes, B), reference=reference, step=(2.0 ** -50, 2.0 ** -50))
    assert all(np.array_equal(again[k], got[k], equal_nan=True) for k in got)
    with pytest.raises(ValueError, match="reference"):
        markers_from_sums(*sums(Y, X, codes, B), reference=B)


# ---- the selection rules ---------------------------------------------------------------------------------------------------------------------------
def test_selection_rules_equal_the_spec_on_hand_made_variances():
    var = np.array([[5.0, 3.0, 3.0, 1.0, 9.0, 0.0, 2.0, 2.0],
                    [1.0, 4.0, 4.0, 4.0, 0.5, 7.0, 2.0, 6.0],
                    [9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0],      # a group of one cell: ignored
                    [2.0, 2.0, 8.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    n_cells = np.array([[5, 5, 5, 5, 1, 5, 5, 5], [5, 5, 5, 5, 5, 5, 2, 1], [1] * 8, [3] * 8])
    n_obs = np.array([6, 6, 1, 3])
    for n_top in (1, 2, 3, 4, 8, 20):
        for flavor in ("union", "rank"):
            for min_cells in (2, 3):
                got = select_variable_genes(var, n_cells, n_obs, n_top, flavor, min_cells)
                want = gr.select(var, n_cells, n_obs, n_top, flavor, min_cells)
                assert np.array_equal(got, want), (n_top, flavor, min_cells, got, want)
    # group 0 ranks 0, 1, 2 (tie by gene order), 6, 7, 3; group 1: 5, 1, 2, 3, 6, 0, 4; group 3: 2, 0, 1, 3, ...
    assert list(select_variable_genes(var, n_cells, n_obs, 2, "union")) == [0, 1, 2, 5]
    assert list(select_variable_genes(var, n_cells, n_obs, 2, "rank")) == [0, 1]      # two groups each; median ranks 1 and 1; then gene order
    assert list(select_variable_genes(var, n_cells, n_obs, 3, "rank")) == [1, 2, 0]   # 1 and 2 in all three groups
    assert select_variable_genes(var, n_cells, n_obs, 20, "rank").size == 8           # fewer qualify than asked for
    assert select_variable_genes(np.ones((2, 3)), np.ones((2, 3)), [5, 5], 2, "rank").size == 0


# ---- the work list -----------------------------------------------------------------------------------------------------------------------------------
_probe = []


def plan_probe():
    if not _probe:
        so = os.path.join(tempfile.mkdtemp(prefix="group_plan_probe_"), "group_plan_probe.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared",
                               os.path.join(ROOT, "tests", "cpp", "group_plan_probe.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.probe_group_plan.restype = C.c_longlong
        _probe.append(lib)
    return _probe[0]


def plan(labels, B, slab, chunk):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    slab = np.ascontiguousarray(slab, dtype=np.int64)
    N, room = labels.size, labels.size + B * (slab.size - 1) + 1
    perm, n_obs, first = np.full(max(N, 1), -7, dtype=np.int32), np.zeros(B, dtype=np.int64), np.zeros(slab.size, dtype=np.int64)
    chunks, kept = np.zeros((room, 3), dtype=np.int64), C.c_longlong(0)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = plan_probe().probe_group_plan(P(labels), C.c_longlong(N), C.c_int(B), P(slab), C.c_longlong(slab.size - 1), C.c_int(chunk), P(perm),
                                      C.byref(kept), P(n_obs), P(first), P(chunks), C.c_longlong(room))
    if n < 0:
        return n
    assert n <= room
    return perm[:kept.value], n_obs, first, chunks[:n]


@pytest.mark.parametrize("chunk", [1, 3, 4, 256])
@pytest.mark.parametrize("slab", [(0, 40), (0, 1, 40), (0, 13, 14, 30, 40), tuple(range(41))])
@pytest.mark.parametrize("kind", ["mod3", "empty_group", "all_out", "three_slabs", "mixed"])
def test_chunk_plan_covers_every_kept_cell_once(kind, slab, chunk):
    N, B = 40, 4
    rng = np.random.default_rng(5)
    labels = {"mod3": np.arange(N) % 3,                               # (level 3: no cell)
              "empty_group": np.where(np.arange(N) % 2 == 0, 0, 3),
              "all_out": np.full(N, -1),
              "three_slabs": np.zeros(N, dtype=np.int64),             # one group over every slab there is
              "mixed": rng.integers(-1, B, N)}[kind]
    perm, n_obs, first, chunks = plan(labels, B, slab, chunk)
    kept = np.nonzero(labels >= 0)[0]
    assert np.array_equal(n_obs, np.bincount(labels[kept], minlength=B))
    assert np.array_equal(perm, kept[np.argsort(labels[kept], kind="stable")])          # stable by label: cells ascend within a group
    assert first[0] == 0 and first[-1] == len(chunks) and np.all(np.diff(first) >= 0)
    seen = np.zeros(N, dtype=np.int64)
    for s in range(len(slab) - 1):
        for g, ln, start in chunks[first[s]:first[s + 1]]:
            cells = perm[start:start + ln]
            assert 1 <= ln <= chunk and cells.size == ln
            assert np.all(labels[cells] == g) and np.all((cells >= slab[s]) & (cells < slab[s + 1]))      # one group, one slab
            seen[cells] += 1
    assert np.array_equal(seen, (labels >= 0).astype(np.int64))
    if kind == "all_out":
        assert len(chunks) == 0 and perm.size == 0
    if kind == "three_slabs" and len(slab) == 5:
        assert len({s for s in range(4) if first[s + 1] > first[s]}) == 4
    # the list depends on the labels, the slabs and the constant alone: the chunks of one slab are those of the same cells cut on their own
    if len(slab) == 2 and chunk == 256:
        assert len(chunks) == int((n_obs > 0).sum())


def test_chunk_plan_refuses_a_label_out_of_range():
    assert plan([0, 1, 2, 1], 2, (0, 4), 4) == -1 - 2
    assert plan([0, -2, 1, 1], 2, (0, 4), 4) == -1 - 1


# ---- argument errors that need no device -------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_handle():
    X, genes = np.ones((3, 2)), ["a", "b"]
    with pytest.raises(ValueError, match="one label per cell"):
        gene_stats_by_group(X, genes, [0, 1])
    with pytest.raises(ValueError, match="no levels"):
        gene_stats_by_group(X, genes, [0, 1, 1], levels=[])
    with pytest.raises(ValueError, match="distinct"):
        gene_stats_by_group(X, genes, [0, 1, 1], levels=[1, 1])
    with pytest.raises(ValueError, match="1-D"):
        gene_stats_by_group(X, genes, [[0, 1, 1]])
    with pytest.raises(ValueError, match="reference"):
        rank_genes_groups(X, genes, [0, 1, 1], reference=2)
    with pytest.raises(ValueError, match="reference"):
        rank_genes_groups(X, genes, ["a", "b", "b"], levels=["a"], reference="b")
    with pytest.raises(ValueError, match="flavor"):
        variable_genes(X, genes, [0, 1, 1], flavor="vst")
    with pytest.raises(ValueError, match="n_top_genes"):
        variable_genes(X, genes, [0, 1, 1], n_top_genes=0)
    with pytest.raises(ValueError, match="one label per cell"):
        variable_genes(X, genes, [0, 1], flavor="rank")


def test_levels_code_the_cells():
    from harmony_amd.group_stats import _codes
    codes, lv = _codes(np.array(["b", "a", "c", "a"]), None, "t")
    assert list(lv) == ["a", "b", "c"] and list(codes) == [1, 0, 2, 0] and codes.dtype == np.int32
    codes, lv = _codes(np.array(["b", "a", "c", "a"]), ["c", "a"], "t")
    assert list(lv) == ["c", "a"] and list(codes) == [-1, 1, 0, 1]
    codes, lv = _codes(np.array([3, 1, 7]), [7, 3], "t")
    assert list(codes) == [1, -1, 0]
