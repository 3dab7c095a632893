"""The spec of the reference's PCA (tests/pca_ref.py) held to itself, without a GPU: the sparse identities the kernels use equal the dense definition,
the derived bars are neither violated by honest float32 nor more than ten times what it does, the subspace iteration converges on the planted
cases, and the float32 operator stays within the end-to-end bar -- before anything runs on a device (tests/test_gpu_pca.py)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pca_ref as pc  # noqa: E402
import project_ref as pr  # noqa: E402


def csr_args(c):
    return c["data"], c["indices"], c["indptr"], c["G_all"]


@functools.lru_cache(maxsize=None)
def sweep_ratios(shape):
    """worst |honest fp32 - spec| / bar of one shape: P, W (against the spec on the same fp32 P), s1, s2, var"""
    c, _ = pc.sweep_case(shape)
    A, tabs = csr_args(c), (c["slot"], c["U"], c["mean"], c["sd"])
    S = pc.dense_S(*A, c["slot"], c["mean"], c["sd"])
    P, W = pc.apply(S, c["U"])
    Ps, Ws = pc.apply_sparse(*A, *tabs)
    scale = max(np.abs(W).max(), 1e-300)
    assert np.abs(P - Ps).max() <= 1e-13 * max(np.abs(P).max(), 1.0) and np.abs(W - Ws).max() <= 1e-12 * scale      # identities: fp64 rounding
    Pf, Wf = pc.apply_fp32(*A, *tabs)
    out = {"P": float((np.abs(Pf - P) / pr.bars(**c)).max())}
    bW = pc.bars_W(*A, c["slot"], c["mean"], c["sd"], Pf)
    err = np.abs(Wf - pc.apply(S, c["U"], P=Pf)[1])
    assert np.all(err[bW == 0] == 0)                     # a column no gene maps to: exactly zero
    out["W"] = float((err[bW > 0] / bW[bW > 0]).max())
    st, sf, b = pc.gene_stats(*A), pc.gene_stats_fp32(*A), pc.gene_stats_bars(*A)
    assert np.array_equal(st["n_cells"], sf["n_cells"])
    has = st["n_cells"] > 0
    assert np.all(sf["s1"][~has] == 0) and np.all(sf["s2"][~has] == 0)
    for k in ("s1", "s2", "var"):
        out[k] = float((np.abs(sf[k] - st[k])[has] / b[k][has]).max())
    return out


@pytest.mark.parametrize("shape", pc.SHAPES)
def test_honest_fp32_stays_within_every_bar(shape):
    r = sweep_ratios(shape)
    print("pca bars %s: honest fp32 / bar = %s" % (shape, {k: round(v, 3) for k, v in r.items()}))
    assert all(v <= 1.0 for v in r.values()), r


def test_no_bar_is_looser_than_ten_times_honest_fp32():
    worst = {k: max(sweep_ratios(s)[k] for s in pc.SHAPES) for k in ("P", "W", "s1", "s2", "var")}
    print("pca bars, worst honest fp32 / bar over the sweep: %s" % {k: round(v, 3) for k, v in worst.items()})
    assert all(v >= 0.1 for v in worst.values()), worst


def test_sweep_cases_carry_their_edges():
    for shape in pc.SHAPES:
        c, special = pc.sweep_case(shape)
        ip, idx = c["indptr"], c["indices"]
        N = shape[0]
        assert all(len(set(idx[ip[i]:ip[i + 1]].tolist())) == ip[i + 1] - ip[i] for i in range(N))      # no gene twice in a row
        if N <= pc.FIRST_FREE:
            continue
        per_gene = np.bincount(idx, minlength=shape[1])
        assert list(np.diff(ip)[:6]) == [min(n, shape[1] - len(special)) for n in pc.ROWS]
        assert np.all(c["slot"][idx[ip[pc.UNKNOWN_ROW]:ip[pc.UNKNOWN_ROW + 1]]] < 0) and np.all(c["data"][ip[pc.ZERO_ROW]:ip[pc.ZERO_ROW + 1]] == 0)
        assert any(np.any(np.diff(idx[ip[i]:ip[i + 1]]) < 0) for i in range(N))
        assert per_gene[special["none"]] == 0 and per_gene[special["all"]] == N - 2 and all(c["slot"][g] >= 0 for g in special.values())
        assert all(per_gene[special[n]] == n for n in pc.COLUMN_COUNTS if n in special)
    assert {n for s in pc.SHAPES for n in pc.sweep_case(s)[1]} >= set(pc.COLUMN_COUNTS)
    tiles = {s[0] for s in pc.SHAPES}
    assert {255, 256, 257} <= tiles and max(tiles) > 3 * 256      # one below, at and one above the transposition's tile of 256 cells; four tiles


def test_clip_is_part_of_the_operator():
    shape = (257, 900, 300, 68)
    c, _ = pc.sweep_case(shape)
    A = csr_args(c)
    assert pr.clipped_entries(c["data"], c["indices"], c["indptr"], c["slot"], c["mean"], c["sd"], clip=3.0) > 0
    S = pc.dense_S(*A, c["slot"], c["mean"], c["sd"], clip=3.0)
    assert S.max() <= 3.0 and not np.array_equal(S, pc.dense_S(*A, c["slot"], c["mean"], c["sd"]))
    P, W = pc.apply(S, c["U"])
    Ps, Ws = pc.apply_sparse(*A, c["slot"], c["U"], c["mean"], c["sd"], clip=3.0)
    assert np.abs(P - Ps).max() <= 1e-12 and np.abs(W - Ws).max() <= 1e-12 * np.abs(W).max()
    Pf, Wf = pc.apply_fp32(*A, c["slot"], c["U"], c["mean"], c["sd"], clip=3.0)
    assert (np.abs(Pf - P) / pr.bars(clip=3.0, **c)).max() <= 1.0
    bW = pc.bars_W(*A, c["slot"], c["mean"], c["sd"], Pf, clip=3.0)
    assert (np.abs(Wf - pc.apply(S, c["U"], P=Pf)[1])[bW > 0] / bW[bW > 0]).max() <= 1.0


@functools.lru_cache(maxsize=None)
def planted(groups):
    """the planted counts as CSR, the spec's choice of 200 genes and their tables"""
    X, lab = pc.planted_counts(groups)
    nz = X != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    A = (X[nz], np.nonzero(nz)[1].astype(np.int32), indptr, X.shape[1])
    st = pc.gene_stats(*A)
    chosen = pc.top_variance(st["var"], st["n_cells"], 200)
    slot = np.full(X.shape[1], -1, dtype=np.int32)
    slot[chosen] = np.arange(chosen.size)
    return A, slot, st["mean"][chosen], np.sqrt(st["var"][chosen]), chosen, lab


@pytest.mark.parametrize("groups", [2, 4, 6])
def test_fit_converges_and_fp32_stays_within_the_end_to_end_bar(groups):
    A, slot, mean, sd, chosen, _ = planted(groups)
    d = groups - 1
    fb = pc.fit_bars(*A, slot, mean, sd, d)
    lam = fb["lam"]
    print("planted %d groups: sin(U_spec, E_d) = %.1e, lambda_(d+1) / lambda_d = %.2f, eta = %.1e, bar_sin = %.1e"
          % (groups, fb["sin_spec"], lam[d] / lam[d - 1], fb["eta"], fb["bar_sin"]))
    assert fb["sin_spec"] <= 1e-4
    assert np.abs(fb["ev_spec"] - lam[:d]).max() / lam[0] <= 1e-8
    top = np.abs(fb["U_spec"]).argmax(axis=0)
    assert np.all(fb["U_spec"][top, np.arange(d)] > 0)
    U, ev = pc.fit(lambda V: pc.apply_fp32(*A, slot, V, mean, sd)[1], 200, len(A[2]) - 1, d)
    s = pc.sin_theta_max(U, fb["E"])
    ev_bar = fb["bar_sin"] ** 2 + fb["eta"] / lam[0]
    ev_r = float((np.abs(ev - lam[:d]) / lam[0]).max() / ev_bar)
    print("  float32 operator: sin / bar_sin = %.4f, explained variance / bar = %.4f" % (s / fb["bar_sin"], ev_r))
    assert s <= fb["bar_sin"] and ev_r <= 1.0


def test_python_side_needs_no_device():
    """argument handling of harmony_amd.pca ahead of the library: the choice of the genes, the loop over any operator"""
    from harmony_amd import fit_loadings, gene_stats  # noqa: F401  (exported)
    from harmony_amd.pca import choose_genes, subspace_iteration
    var, n = np.array([1.0, 3.0, 3.0, 0.5, 9.0, 2.0]), np.array([5, 5, 5, 5, 1, 2])
    assert list(choose_genes(var, n, 3)) == [1, 2, 5] and list(pc.top_variance(var, n, 3)) == [1, 2, 5]      # ties by gene order; one cell: out
    A, slot, mean, sd, _, _ = planted(2)
    S = pc.dense_S(*A, slot, mean, sd)
    U = subspace_iteration(lambda V: S.T @ (S @ V), 200, S.shape[0], 1)
    assert np.array_equal(U, pc.fit(lambda V: S.T @ (S @ V), 200, S.shape[0], 1)[0])
    with pytest.raises(ValueError, match="unique"):
        fit_loadings(np.ones((3, 2)), ["a", "a"])
    with pytest.raises(ValueError, match="two cells"):
        gene_stats(np.ones((1, 2)), ["a", "b"])
