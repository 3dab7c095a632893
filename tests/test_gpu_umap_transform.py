"""Query cells put into a fitted UMAP layout on the MI355X against their spec (tests/umap_transform_ref.py).

The weights are fp64 on both sides and differ by where the two searches stop: both within 1e-5 of the target, and every weight of a row moves
the same way with sigma, so a weight differs by at most 2e-5 plus its float rounding -- column 0, which the search leaves out, included: with
p_j = exp(-d_j / sigma) <= p_0, -p_0 ln p_0 <= sum_{j >= 1} (-p_j ln p_j) / log2 k, so column 0 moves by no more than the summed columns.
The start is an fp64 sum on both sides, in another order: one float ulp of the row's largest |yref_j|.  Which entries fire and which cells they
sample are integers and one fp64 product: "umap_transform:fired" equals the spec's count.  The terms are fp32 on the device and fp64 in the
spec, so one epoch from the same fp32 positions is held elementwise to the bound B the spec derives from the device's expression -- no tuned
tolerance.  Whole transforms are held by quality against the fp64 spec's own runs.

Sizes the kernels take another path at: k <= 16 (16 lanes per cell, four cells to a wave) | above (a wave per cell), up to 64 entries (one per
lane) | more (two); dim 2 | 3; Nq of 1, 3, 5 (groups of a wave without a cell); no negative samples | 31; b < 1, where the clip engages.

Largest |Y_gpu - Y_spec| / B measured per test: printed by `within_bound` (0.50 at most when this was written: where little moves, the
rounding of y itself, half the bound's last term, is what is left)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
sp = pytest.importorskip("scipy.sparse")

import graph_ref as gr  # noqa: E402
import metrics_ref as mr  # noqa: E402
import umap_ref as ur  # noqa: E402
import umap_transform_ref as tr  # noqa: E402
from harmony_amd import (RunHarmony, find_ab_params, knn, umap, umap_layout, umap_query_weights, umap_transform,  # noqa: E402
                         umap_transform_from_knn)
from harmony_amd._call import _Handle  # noqa: E402

ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
AB = {0.5: ur.find_ab(0.5), 0.1: ur.find_ab(0.1)}
GOLDEN = os.path.join(ROOT, "tests", "golden", "umap_layout_bits.npz")

# The fp64 spec's own 100-epoch runs at (Nr, Nq, k) = (2000, 500, 15) over seeds 0 .. 4 (test_umap_transform_cpu.spec_spread, which
# test_constants_for_the_gpu_test holds to these numbers): D = 0.903777, 0.899196, 0.907413, 0.903572, 0.895997, mean |Y - Y0| 0.4448 .. 0.4583; every vote the cell's label
SPEC_D = (0.901991, 0.011416)                              # their mean, max - min


def get(h, key):
    out = (C.c_double * 1)()
    assert h.lib.hmx_get(h.h, key, out, 1) == 1, key
    return out[0]


def library_weights(idx, dist, Nr):
    idx, dist = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float32)
    w, sigma = np.full(idx.shape, -7.0, dtype=np.float32), np.full(idx.shape[0], -7.0)
    with _Handle() as h:
        status = h.lib.hmx_umap_query_weights(h.h, idx.ctypes.data_as(ip), dist.ctypes.data_as(fp), idx.shape[0], idx.shape[1], Nr,
                                              w.ctypes.data_as(fp), sigma.ctypes.data_as(dp))
        assert status == 0, h.lib.hmx_last_error(h.h).decode()
        assert get(h, b"timer:umap_query_weights") > 0
    return w, sigma


def library(idx, w, Yref, n_epochs, epochs=None, Y0=None, a=AB[0.5][0], b=AB[0.5][1], gamma=1.0, alpha0=0.25, negative_sample_rate=5, seed=0):
    """hmx_umap_transform -> (status, the outputs and counters as a dict)"""
    idx, w = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(w, dtype=np.float32)
    Yref = np.ascontiguousarray(Yref, dtype=np.float32)
    Nq, dim = idx.shape[0], Yref.shape[1]
    begin, end = (0, n_epochs) if epochs is None else epochs
    Y0 = None if Y0 is None else np.ascontiguousarray(Y0, dtype=np.float32)
    Y, Yinit = np.full((Nq, dim), -7.0, dtype=np.float32), np.full((Nq, dim), -7.0, dtype=np.float32)
    with _Handle() as h:
        status = h.lib.hmx_umap_transform(h.h, idx.ctypes.data_as(ip), w.ctypes.data_as(fp), Nq, idx.shape[1], Yref.ctypes.data_as(fp), Yref.shape[0],
                                          dim, None if Y0 is None else Y0.ctypes.data_as(fp), n_epochs, begin, end, a, b, gamma, alpha0,
                                          negative_sample_rate, seed, Yinit.ctypes.data_as(fp), Y.ctypes.data_as(fp))
        out = {"fired": int(get(h, b"umap_transform:fired")), "epochs": int(get(h, b"umap_transform:epochs")), "timer": get(h, b"timer:umap_transform"),
               "error": h.lib.hmx_last_error(h.h).decode(), "Y": Y, "Yinit": Yinit}
    return status, out


def bits(Y):
    return np.ascontiguousarray(Y, dtype=np.float32).view(np.uint32)


# ---- the inputs: planted groups split into a reference and a query; the reference laid out once by the layout's own spec -------------------------
@functools.lru_cache(maxsize=None)
def lists(Nq, Nr, k):
    return tr.problem(Nr + Nq, Nq, 8 if Nr >= 2000 else 4, k)


@functools.lru_cache(maxsize=None)
def reference_layout(Nq, Nr, m, dim):
    """the reference of lists(Nq, Nr, .) laid out from its graph of m other cells per cell, 100 epochs, float32"""
    Xr = tr.problem(Nr + Nq, Nq, 8 if Nr >= 2000 else 4, 1)[0]
    ridx, rdist = mr.knn(Xr, m)[:2]
    g = gr.connectivities(ridx.astype(np.int32), np.sqrt(np.maximum(np.asarray(rdist, dtype=np.float64), 0.0)).astype(np.float32))
    return ur.layout(g, ur.pca_init(Xr, dim), 100, *AB[0.5])[0].astype(np.float32)


@functools.lru_cache(maxsize=None)
def spec_weights(Nq, Nr, k):
    _, _, _, _, idx, dist = lists(Nq, Nr, k)
    return tr.query_weights(idx, dist)


# ---- (a) the weights ---------------------------------------------------------------------------------------------------------------------------
WEIGHT_TOL = 2e-5 + 2.0 ** -24


@pytest.mark.parametrize("Nq,Nr,k", [(500, 2000, 15), (301, 600, 16), (203, 600, 17), (50, 300, 64), (50, 300, 65), (30, 300, 128), (7, 300, 1), (1, 300, 15)])
def test_weights(Nq, Nr, k):
    _, _, _, _, idx, dist = lists(Nq, Nr, k)
    assert np.all(np.diff(dist, axis=1) >= 0) and idx.shape == (Nq, k)
    want, sigma = spec_weights(Nq, Nr, k)
    got, gsigma = library_weights(idx, dist, Nr)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    steps, open_ = tr.search(dist)[1:]
    print("umap query weights Nq=%d Nr=%d k=%d: largest |w_gpu - w_spec| %.3g (column 0: %.3g), sigma relative difference %.3g, bisection steps "
          "at most %d, unconverged rows %d" % (Nq, Nr, k, err.max(), err[:, 0].max(), np.abs(gsigma / sigma - 1.0).max(), steps.max(), open_.sum()))
    assert np.all(got >= 0.0) and np.all(got <= 1.0) and np.all(gsigma > 0)
    assert np.all(err <= WEIGHT_TOL)
    if k == 1:
        assert np.all(gsigma == 1.0) and np.all(sigma == 1.0)      # log2 1 = 0 = the empty sum: mid stays 1, far above the floor
    again = library_weights(idx, dist, Nr)
    assert np.array_equal(bits(again[0]), bits(got)) and np.array_equal(again[1], gsigma)
    py, ps = umap_query_weights(idx, dist, Nr, return_scales=True)
    assert np.array_equal(bits(py), bits(got)) and np.array_equal(ps, gsigma) and np.array_equal(bits(umap_query_weights(idx, dist, Nr)), bits(got))


def test_weights_of_a_query_on_a_reference_cell_and_of_all_zero_distances():
    _, _, _, _, idx, dist = lists(203, 600, 17)
    dist = dist.copy()
    dist[5, 0] = 0.0                                       # the query is its nearest reference cell
    dist[9, :3] = 0.0                                      # ... or three of them at once
    got, gsigma = library_weights(idx, dist, 600)
    want, sigma = tr.query_weights(idx, dist)
    assert got[5, 0] == 1.0 and np.all(got[9, :3] == 1.0) and np.all(got[5, 1:] < 1.0)
    assert np.all(np.abs(got.astype(np.float64) - want) <= WEIGHT_TOL)
    for k, want_sigma in ((1, 1.0), (2, 1.0), (3, 2.0 ** -64), (15, 2.0 ** -64), (65, 2.0 ** -64)):
        zi = np.tile(np.arange(k, dtype=np.int32), (6, 1))
        got, gsigma = library_weights(zi, np.zeros((6, k), dtype=np.float32), 100)
        assert np.all(got == 1.0) and np.all(gsigma == want_sigma), k


# ---- (b) the start ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq,Nr,k,dim", [(500, 2000, 15, 2), (203, 600, 17, 3), (30, 300, 128, 2)])
def test_start(Nq, Nr, k, dim):
    _, _, _, _, idx, dist = lists(Nq, Nr, k)
    w = spec_weights(Nq, Nr, k)[0].copy()
    w[3] = 0.0                                             # a row whose weights all underflowed: the plain mean
    w[4, 1:] = 0.0                                         # ... and one with a single weight left: that position
    Yref = reference_layout(Nq, Nr, 14, dim)
    status, got = library(idx, w, Yref, 100, epochs=(0, 0))
    assert status == 0, got["error"]
    want = tr.init(idx, w, Yref)
    ulp = np.spacing(np.abs(Yref[idx]).max(axis=(1, 2)).astype(np.float32)).astype(np.float64)
    err = np.abs(got["Yinit"].astype(np.float64) - want)
    print("umap transform start Nq=%d k=%d dim=%d: largest error %.3g, in ulps of the row's largest |yref| %.3f" % (Nq, k, dim, err.max(), (err / ulp[:, None]).max()))
    assert np.all(err <= ulp[:, None])
    assert np.array_equal(bits(got["Y"]), bits(got["Yinit"])) and got["epochs"] == 0 and got["fired"] == 0      # an empty range returns the start
    assert np.array_equal(got["Yinit"][4], Yref[idx[4, 0]])
    assert np.allclose(got["Yinit"][3], Yref[idx[3]].astype(np.float64).mean(axis=0), rtol=0, atol=ulp[3])


# ---- (c) single epochs --------------------------------------------------------------------------------------------------------------------------
EPOCHS = (0, 1, 57, 99)
SHAPES = {(500, 15, 2): 2000, (500, 15, 3): 2000, (203, 17, 2): 600, (50, 65, 2): 300, (30, 128, 3): 300}      # (Nq, k, dim): Nr


@functools.lru_cache(maxsize=None)
def trajectory(Nq, k, dim):
    """the spec's run of the 100-epoch schedule at min_dist 0.1 from its own start: the positions epochs 0, 1, 57 and 99 start from, as fp32"""
    Nr = SHAPES[(Nq, k, dim)]
    idx = lists(Nq, Nr, k)[4]
    snap = tr.transform(idx, spec_weights(Nq, Nr, k)[0], reference_layout(Nq, Nr, 14, dim), 100, *AB[0.1], snapshots=EPOCHS)[2]
    return {n: Y.astype(np.float32) for n, Y in snap.items()}


def within_bound(idx, w, Yref, Y32, n, n_epochs, what, **kw):
    """epoch n from the fp32 positions Y32 on the library and in the spec: |Y_gpu - Y_spec| <= B elementwise, equal firings"""
    kw.setdefault("a", AB[0.1][0])
    kw.setdefault("b", AB[0.1][1])
    Y32 = np.ascontiguousarray(Y32, dtype=np.float32)
    want = tr.epoch(idx, w, Yref, Y32, n, n_epochs, **kw)
    status, got = library(idx, w, Yref, n_epochs, epochs=(n, n + 1), Y0=Y32, **kw)
    assert status == 0, got["error"]
    err = np.abs(got["Y"].astype(np.float64) - want.Y)
    ratio = float((err / np.maximum(want.B, 1e-300)).max())
    print("umap transform %s: Nq=%d k=%d dim=%d epoch %d of %d %s: fired %d, largest move %.3g, largest error %.3g, largest error / bound %.4f, "
          "%.1f ms" % (what, idx.shape[0], idx.shape[1], Yref.shape[1], n, n_epochs, kw, want.fired, np.abs(want.Y - Y32).max(), err.max(), ratio,
                       got["timer"]))
    assert np.all(np.isfinite(got["Y"])) and got["fired"] == want.fired and got["epochs"] == 1, what
    assert np.array_equal(bits(got["Yinit"]), bits(Y32))   # a start that is given is the start
    assert np.all(err <= want.B), (what, ratio)
    return got, want


@pytest.mark.parametrize("n", EPOCHS)
@pytest.mark.parametrize("Nq,k,dim", sorted(SHAPES))
def test_single_epochs(Nq, k, dim, n):
    Nr = SHAPES[(Nq, k, dim)]
    idx, w = lists(Nq, Nr, k)[4], spec_weights(Nq, Nr, k)[0]
    got, want = within_bound(idx, w, reference_layout(Nq, Nr, 14, dim), trajectory(Nq, k, dim)[n], n, 100, "lists")
    assert want.fired > 0
    if n == 99:
        assert 0.0 < ur.alpha_of(n, 100, 0.25) < 0.0026     # the last epoch still moves


def test_the_clip_engages_at_small_distances():
    """min_dist 0.1 (b < 1) with the reference and the query squeezed into a small box: many terms sit on the clip"""
    idx, w = lists(203, 600, 17)[4], spec_weights(203, 600, 17)[0]
    Yref = (reference_layout(203, 600, 14, 2) * np.float32(0.01)).astype(np.float32)
    Y = (trajectory(203, 17, 2)[57] * np.float32(0.01)).astype(np.float32)
    got, want = within_bound(idx, w, Yref, Y, 57, 100, "squeezed")
    assert np.abs(want.Y - Y).max() > 10 * 4.0 * ur.alpha_of(57, 100, 0.25)      # many clipped terms of 4 add up on a cell


# ---- (d) bit-for-bit equalities ---------------------------------------------------------------------------------------------------------------
def small():
    idx, w = lists(203, 600, 17)[4], spec_weights(203, 600, 17)[0]
    return idx, w, reference_layout(203, 600, 14, 2)


def test_entries_that_never_fire_and_cells_that_never_move():
    idx, w, Yref = small()
    w = w.copy()
    w[:, 9:] *= np.float32(0.009)                          # below wmax / 100: these entries never fire
    w[7] = np.float32(0.001)                               # a cell all of whose entries never fire
    w[0, 0] = 1.0
    r = tr.rates(w)[0]
    assert np.all(r[:, 9:] < 0.01) and np.all(r[7] < 0.01)
    status, got = library(idx, w, Yref, 100)
    want, fired, _ = tr.transform(idx, w, Yref, 100, *AB[0.5])
    assert status == 0 and got["fired"] == fired == int(np.floor(100 * r).sum()) and got["epochs"] == 100
    assert np.array_equal(bits(got["Y"][7]), bits(got["Yinit"][7])) and not np.any(got["Y"][:7] == got["Yinit"][:7])
    # ... also where the start holds a negative zero: nothing is added to it
    Y0 = got["Yinit"].copy()
    Y0[7] = [-0.0, 0.0]
    status, again = library(idx, w, Yref, 100, Y0=Y0)
    assert status == 0 and np.array_equal(bits(again["Y"][7]), bits(Y0[7])) and np.array_equal(bits(again["Y"][:7]), bits(got["Y"][:7]))
    for n in (0, 57):
        within_bound(idx, w, Yref, got["Yinit"], n, 100, "entries that never fire", a=AB[0.5][0], b=AB[0.5][1])


def test_a_query_on_a_listed_reference_position():
    idx, w, Yref = small()
    Y0 = tr.init(idx, w, Yref).astype(np.float32)
    Y0[11] = Yref[idx[11, 0]]                              # d2 = 0 to its first entry: that attraction is 0
    Y0[12] = Yref[idx[12, 16]]
    for n in (0, 3):
        within_bound(idx, w, Yref, Y0, n, 100, "on a reference position")
    one = (idx[:1, :1].copy(), np.ones((1, 1), dtype=np.float32))      # one cell, one entry, on it, no samples: nothing moves it
    status, got = library(one[0], one[1], Yref, 10, Y0=Yref[one[0][0]], negative_sample_rate=0)
    assert status == 0 and np.array_equal(bits(got["Y"]), bits(Yref[one[0][0]])) and got["fired"] == 10


def test_negative_sample_rates_gamma_and_the_other_arguments():
    idx, w, Yref = small()
    Y = trajectory(203, 17, 2)[57]
    base = within_bound(idx, w, Yref, Y, 57, 100, "5 samples")
    none = within_bound(idx, w, Yref, Y, 57, 100, "no samples", negative_sample_rate=0)
    many = within_bound(idx, w, Yref, Y, 57, 100, "31 samples", negative_sample_rate=31)
    zero = within_bound(idx, w, Yref, Y, 57, 100, "gamma 0", gamma=0.0)
    assert none[1].fired == many[1].fired == zero[1].fired == base[1].fired      # the schedule does not depend on them
    assert np.array_equal(bits(zero[0]["Y"]), bits(none[0]["Y"]))               # gamma = 0 equals no samples, in bits
    assert not np.array_equal(base[0]["Y"], none[0]["Y"]) and not np.array_equal(base[0]["Y"], many[0]["Y"])
    within_bound(idx, w, Yref, Y, 57, 100, "gamma 2.5, alpha0 1.0, seed 77", gamma=2.5, alpha0=1.0, seed=77)
    within_bound(idx, w, Yref, Y, 57, 100, "seed 2^32 - 1, min_dist 0.5", seed=2 ** 32 - 1, a=AB[0.5][0], b=AB[0.5][1])
    idx65, w65 = lists(50, 300, 65)[4], spec_weights(50, 300, 65)[0]
    within_bound(idx65, w65, reference_layout(50, 300, 14, 2), trajectory(50, 65, 2)[1], 1, 100, "31 samples, two entries per lane", negative_sample_rate=31)


@pytest.mark.parametrize("Nq", [1, 3, 5])
@pytest.mark.parametrize("k", [15, 17])
def test_partial_groups_in_a_wave(Nq, k):
    idx, w, Yref = lists(203, 600, k)[4][:Nq], spec_weights(203, 600, k)[0][:Nq].copy(), reference_layout(203, 600, 14, 2)
    w[0, 0] = 1.0
    Y0 = tr.init(idx, w, Yref).astype(np.float32)
    for n in (0, 57):
        within_bound(idx, w, Yref, Y0, n, 100, "Nq = %d" % Nq)
    status, got = library(idx, w, Yref, 100)
    status2, whole = library(lists(203, 600, k)[4][:64], np.concatenate([w, spec_weights(203, 600, k)[0][Nq:64]]), Yref, 100)
    assert status == 0 and status2 == 0 and np.array_equal(bits(got["Y"]), bits(whole["Y"][:Nq]))      # a cell does not depend on the others


def test_two_calls_give_identical_bits_and_parts_add_up():
    for (Nq, k, dim) in ((500, 15, 2), (30, 128, 3)):
        Nr = SHAPES[(Nq, k, dim)]
        idx, w, Yref = lists(Nq, Nr, k)[4], spec_weights(Nq, Nr, k)[0], reference_layout(Nq, Nr, 14, dim)
        a, b = library(idx, w, Yref, 100)[1], library(idx, w, Yref, 100)[1]
        assert np.array_equal(bits(a["Y"]), bits(b["Y"])) and np.array_equal(bits(a["Yinit"]), bits(b["Yinit"])) and a["fired"] == b["fired"] and a["epochs"] == 100
        first = library(idx, w, Yref, 100, epochs=(0, 10))[1]
        second = library(idx, w, Yref, 100, epochs=(10, 100), Y0=first["Y"])[1]
        assert np.array_equal(bits(second["Y"]), bits(a["Y"])) and first["fired"] + second["fired"] == a["fired"] and second["epochs"] == 90
        assert a["fired"] == int(np.floor(100 * tr.rates(w)[0]).sum())
        other = library(idx, w, Yref, 100, seed=1)[1]
        assert not np.array_equal(other["Y"], a["Y"]) and other["fired"] == a["fired"] and np.all(np.isfinite(a["Y"]))


def test_inputs_that_return_the_start():
    idx, w, Yref = small()
    start = library(idx, w, Yref, 100, epochs=(0, 0))[1]["Yinit"]
    for epochs in ((0, 0), (7, 7), (100, 100)):
        status, got = library(idx, w, Yref, 100, epochs=epochs)
        assert status == 0 and np.array_equal(bits(got["Y"]), bits(start)) and got["epochs"] == 0 and got["fired"] == 0
    zeros = np.zeros_like(w)                               # wmax == 0: the plain means, and no epoch runs
    status, got = library(idx, zeros, Yref, 100)
    assert status == 0 and np.array_equal(bits(got["Y"]), bits(got["Yinit"])) and got["epochs"] == 0 and got["fired"] == 0
    assert np.allclose(got["Y"], Yref[idx].astype(np.float64).mean(axis=1), rtol=0, atol=1e-5)
    Y0 = start.copy()
    Y0[6] = [-0.0, 0.0]
    status, got = library(idx, zeros, Yref, 100, Y0=Y0)
    assert status == 0 and np.array_equal(bits(got["Y"]), bits(Y0)) and np.array_equal(bits(got["Yinit"]), bits(Y0))


# ---- (e) whole transforms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_full_transforms_are_held_by_quality(seed):
    Xr, lab_r, Xq, lab_q, idx, dist = lists(500, 2000, 15)
    Yref = reference_layout(500, 2000, 14, 2)
    w = library_weights(idx, dist, 2000)[0]
    status, got = library(idx, w, Yref, 100, seed=seed)
    assert status == 0, got["error"]
    Y = got["Y"]
    D = tr.spread_to_neighbours(Y, idx, Yref)
    print("umap full transform seed %d: 500 cells into 2000, k = 15, 100 epochs, %d firings, %.1f ms: D %.6f (the spec's runs: mean %.6f, spread "
          "%.6f), mean |Y - Y0| %.4f" % (seed, got["fired"], got["timer"], D, SPEC_D[0], SPEC_D[1], np.abs(Y - got["Yinit"]).mean()))
    assert np.all(np.isfinite(Y)) and np.array_equal(tr.vote(Y, Yref, lab_r), lab_q)
    assert abs(D - SPEC_D[0]) <= 3.0 * SPEC_D[1]
    assert got["fired"] == int(np.floor(100 * tr.rates(w)[0]).sum())


# ---- (f) the composed entry points --------------------------------------------------------------------------------------------------------------------
def test_umap_transform_is_knn_then_weights_then_transform():
    Xr, lab_r, Xq, lab_q, _, _ = lists(500, 2000, 15)
    Yref = reference_layout(500, 2000, 14, 2)
    Y, Y0 = umap_transform(Xq, Xr, Yref, n_epochs=30, return_init=True)
    idx, dist = knn(Xr, 15, query=Xq)
    w = umap_query_weights(idx, dist, 2000)
    again, start = umap_transform_from_knn(idx, w, Yref, n_epochs=30, return_init=True)
    assert Y.shape == (500, 2) and Y.dtype == np.float32 and np.array_equal(bits(Y), bits(again)) and np.array_equal(bits(Y0), bits(start))
    a, b = find_ab_params(1.0, 0.5)
    status, got = library(idx, w, Yref, 30, a=a, b=b)      # learning_rate 1 is alpha0 = 1 / 4
    assert status == 0 and np.array_equal(bits(got["Y"]), bits(Y)) and np.array_equal(tr.vote(Y, Yref, lab_r), lab_q)
    part = umap_transform_from_knn(idx, w, Yref, init=umap_transform_from_knn(idx, w, Yref, n_epochs=30, epochs=(0, 12)), n_epochs=30, epochs=(12, 30))
    assert np.array_equal(bits(part), bits(Y))
    Y3 = umap_transform(Xq, Xr, reference_layout(500, 2000, 14, 3), n_neighbors=10, min_dist=0.1, learning_rate=0.5, negative_sample_rate=3, seed=4, init=np.zeros((500, 3)))
    assert Y3.shape == (500, 3) and np.all(np.isfinite(Y3)) and np.any(Y3 != 0)
    assert np.array_equal(umap_transform(Xq, Xr, Yref), umap_transform(Xq, Xr, Yref, n_epochs=100))      # 100 epochs up to 10 000 query cells


def test_harmony_umap_transform_is_umap_transform_of_z_corr():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines_small.npz"))
    meta = {"dataset": fx["dataset_levels"][fx["dataset"]]}
    obj = RunHarmony(fx["pcs"], meta, "dataset", return_object=True, verbose=False, seed=1, max_iter=2, nclust=10)
    Z = np.ascontiguousarray(np.asarray(obj.getZcorr()).T)
    Yref = obj.umap(n_epochs=40)
    a = obj.umap_transform(Z, Yref, n_epochs=30)             # the reference's own cells as the query
    b = umap_transform(Z, Z, Yref, n_epochs=30)
    assert a.shape == Yref.shape and a.dtype == np.float32 and np.array_equal(bits(a), bits(b)) and np.all(np.isfinite(a))
    c = obj.umap_transform(Z[::2], Yref[::2], n_neighbors=10, min_dist=0.1, seed=2, n_epochs=30)
    d = umap_transform(Z, Z[::2], Yref[::2], n_neighbors=10, min_dist=0.1, seed=2, n_epochs=30)
    assert np.array_equal(bits(c), bits(d))


def test_the_layout_is_unchanged_in_bits():
    """the layout's kernels share their term arithmetic with the transform's through one device header: umap_layout() and umap() on inputs of
    tests/test_gpu_umap.py give the bits recorded before the arithmetic moved there"""
    gold = np.load(GOLDEN)
    X = ur.groups(600, 4)[0]
    ridx, rdist = mr.knn(X, 29)[:2]
    g = gr.connectivities(ridx.astype(np.int32), np.sqrt(np.maximum(np.asarray(rdist, dtype=np.float64), 0.0)).astype(np.float32))
    for dim, min_dist in ((2, 0.5), (3, 0.1)):
        a, b = AB[min_dist]
        Y = umap_layout(sp.csr_matrix((g[2], g[1], g[0]), shape=(600, 600)), ur.pca_init(X, dim), n_components=dim, n_epochs=40, a=a, b=b)
        assert np.array_equal(bits(Y), gold["layout_%d" % dim])
    Y = umap(ur.groups(2000, 8)[0], n_neighbors=15, n_epochs=30)
    assert np.array_equal(bits(Y), gold["umap_2000"])
