"""The fp64 spec of the silhouette widths (harmony_amd/silhouette.py): sklearn.metrics.silhouette_samples with Euclidean distance, extended by
groups, restated in NumPy.  The spec reads fp32-rounded inputs, as the device does, takes every squared distance as the direct sum of
(x - y)^2 and computes everything in float64.  It also gives the rounding bars the GPU tests hold the device to, and the two scib
aggregates (label ASW, batch ASW within labels)."""
import numpy as np

from metrics_ref import as_f32_f64, sqdist_block

U = 2.0 ** -24


def distances(X):
    """every pairwise Euclidean distance of the fp32-rounded rows, N x N float64, exact zeros on the diagonal"""
    X = as_f32_f64(X)
    D = np.sqrt(sqdist_block(X, X))
    np.fill_diagonal(D, 0.0)
    return D


def silhouette(X, labels, groups=None, bars=False, D=None):
    """(s, a, b) per cell, in the order given; with bars=True also (da, db, ds), the rounding bars of a device that forms
    d2 = |x|^2 + |y|^2 - 2 x.y in fp32 (error e = (2 d + 4) 2^-24 (|x|^2 + |y|^2)), takes one fp32 square root (<= 1 ulp) and lets a distance
    pass at most 64 fp32 additions and one conversion before an fp64 sum: per pair min(sqrt e, e / D) + 66 2^-24 D; da the mean over the
    pairs of a, db the largest such mean over the other labels, ds = 2 (da + db) / max(a, b).

    a: mean distance to the OTHER cells of the group with the cell's label (self excluded by index); b: the smallest mean distance to the
    cells of another label of the group; s = (b - a) / max(a, b), 0 where that maximum is 0; s = a = 0 for the only cell of its label in
    its group; s = a = b = NaN in a group with fewer than two labels.  D: distances(X), when the caller holds it already."""
    X = as_f32_f64(X)
    N, d = X.shape
    lab = np.unique(np.asarray(labels), return_inverse=True)[1]
    grp = np.zeros(N, dtype=np.int64) if groups is None else np.unique(np.asarray(groups), return_inverse=True)[1]
    out = [np.full(N, np.nan) for _ in range(6)]
    n2 = (X * X).sum(axis=1)
    for g in np.unique(grp):
        sel = np.nonzero(grp == g)[0]
        levels, lg = np.unique(lab[sel], return_inverse=True)
        if len(levels) < 2:
            continue
        n = len(sel)
        counts = np.bincount(lg).astype(np.float64)
        onehot = np.zeros((n, len(levels)))
        onehot[np.arange(n), lg] = 1.0
        Dg = distances(X[sel]) if D is None else D[np.ix_(sel, sel)]

        def fold(M):
            """per-label means of the pair quantity M: (own label, self excluded; the extreme over the other labels is taken by the caller)"""
            sums = M @ onehot
            own = sums[np.arange(n), lg]
            own = np.where(counts[lg] > 1, own / np.maximum(counts[lg] - 1.0, 1.0), 0.0)
            return own, sums / counts[None, :]

        a, means = fold(Dg)
        means[np.arange(n), lg] = np.inf
        b = means.min(axis=1)
        m = np.maximum(a, b)
        s = np.where(m > 0, (b - a) / np.where(m > 0, m, 1.0), 0.0)
        s[counts[lg] == 1] = 0.0
        out[0][sel], out[1][sel], out[2][sel] = s, a, b
        if bars:
            e = (2 * d + 4) * U * (n2[sel][:, None] + n2[sel][None, :])
            with np.errstate(divide="ignore", invalid="ignore"):
                delta = np.minimum(np.sqrt(e), np.where(Dg > 0, e / Dg, np.inf)) + 66 * U * Dg
            np.fill_diagonal(delta, 0.0)
            da, dmeans = fold(delta)
            dmeans[np.arange(n), lg] = -np.inf
            db = dmeans.max(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                ds = np.where(m > 0, 2 * (da + db) / m, np.inf)
            out[3][sel], out[4][sel], out[5][sel] = da, db, ds
    return tuple(out) if bars else tuple(out[:3])


def asw_label(s, rescale=True):
    """scib's label ASW: the mean width, as (mean + 1) / 2 when rescaled"""
    m = float(np.mean(s))
    return (m + 1.0) / 2.0 if rescale else m


def asw_batch(s, batch, group, rescale=True):
    """scib's batch ASW from widths over the batch computed within the groups: groups with one batch, or with as many batches as cells, are
    skipped; per cell 1 - |s| (|s| when not rescaled), the mean per group, then the mean of the group means: (score, {group: mean})"""
    batch, group = np.asarray(batch), np.asarray(group)
    per = {}
    for g in np.unique(group):
        sel = group == g
        nb = len(np.unique(batch[sel]))
        if nb == 1 or nb == int(sel.sum()):
            continue
        v = np.abs(np.asarray(s)[sel])
        per[g.item()] = float(np.mean(1.0 - v if rescale else v))
    return (float(np.mean(list(per.values()))) if per else float("nan")), per
