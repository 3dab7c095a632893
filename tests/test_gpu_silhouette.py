"""Silhouette widths on the MI355X against the fp64 spec (tests/silhouette_ref.py).

The rounding bar.  The device forms d2 = |x|^2 + |y|^2 - 2 x.y in fp32: an error of at most e = (2 d + 4) 2^-24 (|x|^2 + |y|^2) on d2, hence
min(sqrt e, e / D) on the distance D; the square root is one fp32 instruction (<= 1 ulp), a distance passes at most 64 fp32 additions
(32 in its lane, 4 across the 16 lanes of a query row in the kernel as built) and one conversion before it reaches an fp64 sum: 66 2^-24 D.
Per pair delta = min(sqrt e, e / D) + 66 2^-24 D; da is the mean of delta over the pairs of a, db the largest such mean over the other
labels, and the bar on s is 2 (da + db) / max(a, b).  On integer lattice data d2 is exact, and a and b are held to 66 2^-24 relative.

Sizes the kernel takes another path at: 64 query rows per workgroup (16 per wave), 64 data rows per slab, (group, label) segments padded
to 16 rows, a reduction into fp64 every 32 tiles (512 cells) of a segment, PC groups of 16 (kernels built for 2, 4 and 8 groups:
d <= 32, <= 64, <= 128), a counting sort of the (group, label) keys below about a million levels and a comparison sort above."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import silhouette_ref as sr  # noqa: E402
from bench_data import synth  # noqa: E402
from harmony_amd import (Harmony, RunHarmony, _lib, map_query, prepare_setup_args, silhouette, silhouette_batch, silhouette_label,  # noqa: E402
                         silhouette_samples)
from harmony_amd.utils import harmonize  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


def check(got, ref, what, rows=None):
    """|a - a_ref| <= da, |b - b_ref| <= db, s within its bar, NaN exactly where the spec has NaN; prints the worst error / bar ratios"""
    (s, a, b), (rs, ra, rb, da, db, ds) = got, ref
    if rows is not None:
        rs, ra, rb, da, db, ds = (v[rows] for v in ref)
    nan = np.isnan(rs)
    assert np.array_equal(np.isnan(s), nan) and np.array_equal(np.isnan(a), nan) and np.array_equal(np.isnan(b), nan), what
    ok = ~nan
    with np.errstate(divide="ignore", invalid="ignore"):
        ea = np.where(ra[ok] == a[ok], 0.0, np.abs(a[ok] - ra[ok]) / da[ok])
        eb = np.where(rb[ok] == b[ok], 0.0, np.abs(b[ok] - rb[ok]) / db[ok])
        es = np.where(rs[ok] == s[ok], 0.0, np.abs(s[ok] - rs[ok]) / ds[ok])
    print("silhouette %s: %d cells, worst error / bar: a %.3f, b %.3f, s %.3f" % (what, int(ok.sum()), ea.max(initial=0), eb.max(initial=0), es.max(initial=0)))
    assert ea.max(initial=0) <= 1.0 and eb.max(initial=0) <= 1.0 and es.max(initial=0) <= 1.0, what
    assert (s[ok] >= -1).all() and (s[ok] <= 1).all()


def raw_call(X, codes, n_levels, gcodes=None, n_groups=1):
    """hmx_silhouette with level counts of the caller's choosing (the Python functions always pass the levels present)"""
    X, xdt = silhouette._rows(X, "X")
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    gcodes = None if gcodes is None else np.ascontiguousarray(gcodes, dtype=np.int32)
    with silhouette._Handle() as h:
        return silhouette._call(h.lib, h.h, h.check, X, xdt, X.shape[0], X.shape[1], codes, n_levels, gcodes, n_groups, True)


# ---- 1. lattice: d2 is exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 50, 76])
def test_lattice(d):
    rng = np.random.default_rng(200 + d)
    X = rng.integers(-4, 5, size=(2000, d)).astype(np.float64)
    lab = rng.integers(0, 5, 2000)
    ref = sr.silhouette(X, lab, bars=True)
    s, a, b = silhouette_samples(X, lab, return_ab=True)
    ra, rb = ref[1], ref[2]
    ea, eb = np.abs(a - ra) / ra / (66 * U), np.abs(b - rb) / rb / (66 * U)
    print("silhouette lattice d=%d: worst relative error of a %.3f, of b %.3f (in units of 66 2^-24)" % (d, ea.max(), eb.max()))
    assert ea.max() <= 1.0 and eb.max() <= 1.0
    es = np.abs(s - ref[0]) / (2 * (ref[3] + ref[4]) / np.maximum(ra, rb))
    print("silhouette lattice d=%d: worst error / bar of s %.3f" % (d, es.max()))
    assert es.max() <= 1.0
    assert same_bits(s, silhouette_samples(X, lab))


# ---- 2. real-valued -----------------------------------------------------------------------------------------------------------------------
SHAPES = [(63, 50), (65, 50), (129, 50), (1000, 20), (3000, 50), (1500, 76), (257, 128), (193, 1), (640, 33)]


def labeling(N, kind):
    rng = np.random.default_rng(1000 + N)
    if kind == "two":
        return rng.integers(0, 2, N)
    if kind == "four":
        return np.asarray(synth(N, d=2, levels=(4,), seed=5)[1]["cov0"])
    # 200 labels whose sizes include 1, 15, 16, 17 and 65 cells, every label present, scattered over the cells
    sizes = [1, 15, 16, 17, 65]
    lab = np.concatenate([np.full(n, i) for i, n in enumerate(sizes)] + [np.arange(5, 200), rng.integers(5, 200, N - sum(sizes) - 195)])
    return rng.permutation(lab)


@functools.lru_cache(maxsize=None)
def real_data(N, d):
    """the rows and their pairwise distances, computed once for every labeling"""
    Z = synth(N, d=d, levels=(4,), seed=5)[0]
    return Z, sr.distances(Z)


@functools.lru_cache(maxsize=None)
def real_case(N, d, kind):
    Z, D = real_data(N, d)
    lab = labeling(N, kind)
    return Z, lab, sr.silhouette(Z, lab, bars=True, D=D)


CASES = [(N, d, kind) for N, d in SHAPES for kind in ("two", "four", "many") if kind != "many" or N >= 640]      # (200 labels with a 65-cell one need the cells)


@pytest.mark.parametrize("N,d,kind", CASES)
def test_real_valued(N, d, kind):
    Z, lab, ref = real_case(N, d, kind)
    if kind == "many":
        assert sorted(np.bincount(lab))[0] == 1 and {15, 16, 17, 65} <= set(np.bincount(lab)) and len(np.unique(lab)) == 200
    got = silhouette_samples(Z, lab, return_ab=True)
    check(got, ref, "N=%d d=%d %s" % (N, d, kind))
    if kind == "many":
        assert (got[0][np.bincount(lab)[lab] == 1] == 0).all()


def test_more_levels_than_labels_present():
    """codes with gaps under level counts far above the labels present: the same widths, bit for bit -- through the counting sort (1000
    levels) and through the comparison sort (2^30 levels)"""
    Z, lab, ref = real_case(1000, 20, "four")
    base = raw_call(Z, lab, 4)
    check(base, ref, "dense codes")
    for n_levels, codes in ((1000, 7 * lab + 3), (1 << 30, (1 << 28) * lab + 12345)):
        got = raw_call(Z, codes, n_levels)
        assert all(same_bits(x, y) for x, y in zip(got, base)), n_levels
    got = raw_call(Z, codes, 1 << 30, np.full(1000, 2), 1 << 30)
    assert all(same_bits(x, y) for x, y in zip(got, base))


# ---- 3. groups ----------------------------------------------------------------------------------------------------------------------------
def test_one_group_is_the_ungrouped_call():
    Z, lab, _ = real_case(1000, 20, "four")
    got = silhouette_samples(Z, lab, groups=np.full(1000, "g"), return_ab=True)
    base = silhouette_samples(Z, lab, return_ab=True)
    assert all(same_bits(x, y) for x, y in zip(got, base))


def test_three_groups_of_700_299_and_1():
    """no group size is a multiple of 64: query tiles straddle groups; the one-cell group gives NaN"""
    Z, lab, _ = real_case(1000, 20, "four")
    rng = np.random.default_rng(3)
    grp = rng.permutation(np.repeat(["a", "b", "c"], [700, 299, 1]))
    ref = sr.silhouette(Z, lab, grp, bars=True)
    got = silhouette_samples(Z, lab, groups=grp, return_ab=True)
    check(got, ref, "groups 700 / 299 / 1")
    assert np.isnan(got[0][grp == "c"]).all() and np.isnan(got[0]).sum() == 1
    for g in ("a", "b"):                                     # ... and a separate call on the group's rows
        sel = grp == g
        alone = silhouette_samples(Z[sel], lab[sel], return_ab=True)
        check(alone, ref, "group %s alone" % g, rows=sel)
        for x, y, bar in zip(alone, (v[sel] for v in got), (ref[5][sel], ref[3][sel], ref[4][sel])):
            assert (np.abs(x - y) <= 2 * bar).all()


def test_a_group_with_a_single_label_gives_nan_for_exactly_its_cells():
    Z, lab, _ = real_case(1000, 20, "four")
    rng = np.random.default_rng(4)
    grp = rng.integers(0, 3, 1000)
    lab = np.where(grp == 1, 2, lab)
    ref = sr.silhouette(Z, lab, grp, bars=True)
    got = silhouette_samples(Z, lab, groups=grp, return_ab=True)
    check(got, ref, "one-label group")
    assert np.array_equal(np.isnan(got[0]), grp == 1) and np.isnan(got[1][grp == 1]).all() and np.isnan(got[2][grp == 1]).all()


# ---- 4. edge values -------------------------------------------------------------------------------------------------------------------------
def test_edge_values():
    Z, lab, _ = real_case(129, 50, "two")
    lab = lab.copy()
    lab[77] = 5                                              # a singleton label
    s, a, b = silhouette_samples(Z, lab, return_ab=True)
    check((s, a, b), sr.silhouette(Z, lab, bars=True), "singleton")
    assert s[77] == 0.0 and a[77] == 0.0 and b[77] > 0
    s, a, b = silhouette_samples(np.full((100, 9), 1.25), np.arange(100) % 3, return_ab=True)      # all rows identical
    assert not s.any() and not a.any() and not b.any()
    X = Z.copy()                                             # a cell and its duplicate under different labels
    X[100], lab[100], lab[3] = X[3], 1, 0
    ref = sr.silhouette(X, lab, bars=True)
    got = silhouette_samples(X, lab, return_ab=True)
    check(got, ref, "duplicate under another label")
    assert np.isfinite(got[0]).all()


# ---- 5. input forms ---------------------------------------------------------------------------------------------------------------------------
def test_input_forms_give_identical_results():
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    Z, lab, _ = real_case(3000, 50, "four")
    X32 = np.ascontiguousarray(Z, dtype=np.float32)
    first = silhouette_samples(Z, lab, return_ab=True)
    for other in (silhouette_samples(X32, lab, return_ab=True), silhouette_samples(Z, lab, return_ab=True)):      # fp32 host; a second call
        assert all(same_bits(x, y) for x, y in zip(other, first))
    lib = _lib.load()
    h = ctypes.c_void_p(lib.hmx_create())
    dX = ctypes.c_void_p()
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    codes = np.ascontiguousarray(lab, dtype=np.int32)
    s, a, b = np.empty(3000), np.empty(3000), np.empty(3000)
    try:
        assert hip.hipMalloc(ctypes.byref(dX), X32.nbytes) == 0
        assert hip.hipMemcpy(dX, X32.ctypes.data, X32.nbytes, 1) == 0
        assert lib.hmx_silhouette(h, dX, 1, 1, 3000, 50, codes.ctypes.data_as(ip), 4, None, 0, s.ctypes.data_as(dp), a.ctypes.data_as(dp),
                                  b.ctypes.data_as(dp)) == 0, lib.hmx_last_error(h)
        assert all(same_bits(x, y) for x, y in zip((s, a, b), first))
        out = (ctypes.c_double * 1)()
        assert lib.hmx_get(h, b"timer:silhouette", out, 1) == 1 and out[0] > 0
        s2 = np.empty(3000)                                   # a and b may be NULL
        assert lib.hmx_silhouette(h, dX, 1, 1, 3000, 50, codes.ctypes.data_as(ip), 4, None, 0, s2.ctypes.data_as(dp), None, None) == 0
        assert same_bits(s2, first[0])
    finally:
        lib.hmx_destroy(h)
        if dX.value:
            hip.hipFree(dX)


# ---- 6. on a handle ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cell_lines():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines.npz"))
    pcs = fx["pcs"].astype(np.float64)
    meta = {"dataset": fx["dataset_levels"][fx["dataset"]], "cell_type": fx["cell_type_levels"][fx["cell_type"]]}
    obj = RunHarmony(pcs, meta, "dataset", return_object=True, verbose=False, seed=1)
    return pcs, meta, obj


def test_on_a_fitted_handle_and_on_a_query_handle():
    pcs, meta, obj = cell_lines()
    Zc = obj.getZcorr().T
    D = sr.distances(Zc)
    for group_col in (None, "cell_type"):
        label_col = "cell_type" if group_col is None else "dataset"
        got = obj.silhouette(meta, label_col, group_col=group_col, return_ab=True)
        ref = sr.silhouette(Zc, meta[label_col], None if group_col is None else meta[group_col], bars=True, D=D)
        check(got, ref, "handle, %s | %s" % (label_col, group_col))
        host = silhouette_samples(Zc, meta[label_col], groups=None if group_col is None else meta[group_col], return_ab=True)
        check(host, ref, "getZcorr, %s | %s" % (label_col, group_col))
        again = obj.silhouette(meta, label_col, group_col=group_col, return_ab=True)
        assert all(same_bits(x, y) for x, y in zip(again, got))
        assert same_bits(obj.silhouette(meta, label_col, group_col=group_col), got[0])
    assert np.array_equal(obj.getZcorr().T, Zc) and obj.timer("silhouette") > 0
    with pytest.raises(ValueError):
        obj.silhouette({"one": np.zeros(len(pcs), int)}, "one")
    # a query handle scores its own Z_corr
    ds = meta["dataset"]
    refsel = ds != "jurkat"
    skw, _ = prepare_setup_args(pcs[refsel], {"dataset": ds[refsel]}, "dataset", nclust=20)
    h = Harmony(seed=1)
    h.setup(**skw)
    h.init_cluster_cpp()
    harmonize(h, 10, verbose=False)
    q = map_query(pcs[ds == "jurkat"], None, h.reference_summary(), return_object=True)
    Zq = q.getZcorr().T
    qlab = np.arange(Zq.shape[0]) % 3
    check(q.silhouette({"l": qlab}, "l", return_ab=True), sr.silhouette(Zq, qlab, bars=True), "query handle")
    assert np.array_equal(q.getZcorr().T, Zq)


# ---- 7. the point of the feature ----------------------------------------------------------------------------------------------------------------
def test_harmony_mixes_the_batches_and_keeps_the_cell_types_apart_on_the_cell_lines():
    """batch ASW (dataset | cell_type) must rise from the raw PCs to Z_corr and the label ASW (cell_type) must not fall by more than 0.05
    of its [0, 1] scale: asserted on the spec's values first (a failure there is the data's), then on the GPU's, which must agree with the
    spec within the bars."""
    pcs, meta, obj = cell_lines()
    Zc = obj.getZcorr().T
    scores = {}
    for name, Z in (("raw", pcs), ("corrected", Zc)):
        D = sr.distances(Z)
        rb = sr.silhouette(Z, meta["dataset"], meta["cell_type"], bars=True, D=D)
        rl = sr.silhouette(Z, meta["cell_type"], bars=True, D=D)
        check(silhouette_samples(Z, meta["dataset"], groups=meta["cell_type"], return_ab=True), rb, "%s dataset | cell_type" % name)
        check(silhouette_samples(Z, meta["cell_type"], return_ab=True), rl, "%s cell_type" % name)
        spec_b, spec_per = sr.asw_batch(rb[0], meta["dataset"], meta["cell_type"])
        spec_l = sr.asw_label(rl[0])
        gpu_b, gpu_per = silhouette_batch(Z, meta, "dataset", "cell_type")
        gpu_l = silhouette_label(Z, meta, "cell_type")
        # a mean of |s| moves by no more than the mean bar of s
        assert abs(gpu_l - spec_l) <= np.mean(rl[5]) / 2 and set(gpu_per) == set(spec_per)
        for level in spec_per:
            assert abs(gpu_per[level] - spec_per[level]) <= np.mean(rb[5][meta["cell_type"] == level])
        assert gpu_b == pytest.approx(np.mean(list(gpu_per.values())), rel=1e-12)
        scores[name] = (spec_b, spec_l, gpu_b, gpu_l)
        print("cell lines, %s: batch ASW spec %.4f gpu %.4f, label ASW spec %.4f gpu %.4f" % (name, spec_b, gpu_b, spec_l, gpu_l))
    assert scores["corrected"][0] > scores["raw"][0] and scores["corrected"][1] > scores["raw"][1] - 0.05          # the spec
    assert scores["corrected"][2] > scores["raw"][2] and scores["corrected"][3] > scores["raw"][3] - 0.05          # the GPU
