"""Doublet detection in the manner of Scrublet (Wolock, Lopez & Klein, Cell Systems 2019).

A doublet is a droplet that captured two cells.  Scrublet, scDblFinder and DoubletFinder all find them the same way: add the raw counts of
random pairs of observed cells, push the synthetic cells through the same normalisation and PCA as the observed ones, search the combined set
for nearest neighbours and score every cell by the share of synthetic cells among its neighbours.  Here the synthetic cells are built and
projected straight from the count matrix where it lives (hmx_simulate_doublets: the counts of the two parents are summed BEFORE the log, so
this is not project_query of a host-built matrix), the search is the library's exact kNN on the combined set followed by an integer count per
cell (hmx_doublet_neighbors), and the scores are closed forms of those counts in NumPy.  include/harmony_mi355x_doublets.h; arguments are
checked here, before the library is loaded.
"""
import ctypes as C

import numpy as np

from ._call import _Handle, _rows
from .project import MAX_D, MAX_GENES, DeviceCSR, HarmonyLoadings, _as_csr, gene_slots, project_query
from .utils import _message

MAX_K = 128
MAX_TABLE_GENES = 16128      # a wave keeps one fp32 word per reference gene in LDS (hmx_doublet_plan.h)


def _pairs(pairs, N, sim_doublet_ratio, seed):
    if pairs is None:
        if not (np.isfinite(sim_doublet_ratio) and sim_doublet_ratio > 0):
            raise ValueError("simulate_doublets: sim_doublet_ratio must be positive")
        n_sim = int(round(float(sim_doublet_ratio) * N))
        if n_sim < 1:
            raise ValueError("simulate_doublets: sim_doublet_ratio %g of %d cells leaves no synthetic cell" % (sim_doublet_ratio, N))
        return np.ascontiguousarray(np.random.default_rng(seed).integers(0, N, (n_sim, 2)), dtype=np.int64)
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError("simulate_doublets: pairs must be n_sim x 2 with n_sim >= 1")
    if not np.issubdtype(p.dtype, np.integer):
        if not np.all(np.isfinite(p)) or np.any(p != np.floor(p)):
            raise ValueError("simulate_doublets: pairs must be integers")
    if np.any(p < 0) or np.any(p >= N):
        raise ValueError("simulate_doublets: pairs must name cells in [0, %d)" % N)
    return np.ascontiguousarray(p, dtype=np.int64)


def simulate_doublets(counts, genes, loadings, pairs=None, sim_doublet_ratio=2.0, seed=0, totals=None, device=None, _handle=None):
    """Synthetic doublets in the PCs of `loadings`.  counts, genes, loadings, totals: as for project_query (every form of count matrix it
    takes).  pairs: n_sim x 2 indices of the parents (a == b is allowed), or None: round(sim_doublet_ratio N) pairs drawn with replacement by
    np.random.default_rng(seed).integers(0, N, (n_sim, 2)), as Scrublet draws them.  The draw is on the host: the library call is a pure
    function of its arguments.  Synthetic cell s is the SUM of its parents' raw counts, normalised by the sum of their library sizes, then
    log1p, the reference's scaling and the loadings.  -> (sim_pcs n_sim x d float32, pairs n_sim x 2 int64)."""
    if not isinstance(loadings, HarmonyLoadings):
        raise ValueError("simulate_doublets: loadings must be a HarmonyLoadings")
    genes = np.asarray(genes).astype(str).reshape(-1)
    G_all, G, d = int(genes.size), loadings.G, loadings.d
    if G_all < 1:
        raise ValueError("simulate_doublets: no genes")
    data, indices, indptr, N, on_device = _as_csr(counts, G_all)
    if N < 1:
        raise ValueError("simulate_doublets: no cells")
    if d > MAX_D:
        raise ValueError("simulate_doublets: the loadings have %d PCs: at most %d are supported" % (d, MAX_D))
    if G_all > MAX_GENES:
        raise ValueError("simulate_doublets: at most 2^24 genes are supported")
    if G > MAX_TABLE_GENES:
        raise ValueError("simulate_doublets: the loadings have %d genes: at most %d are supported" % (G, MAX_TABLE_GENES))
    slot = gene_slots(genes, loadings)
    if int((slot >= 0).sum()) == 0:
        raise ValueError("simulate_doublets: the matrix shares no gene with the loadings")
    if totals is not None:
        totals = np.ascontiguousarray(totals, dtype=np.float64).reshape(-1)
        if totals.size != N:
            raise ValueError("simulate_doublets: totals must hold one library size per cell")
        if not np.all(np.isfinite(totals)) or np.any(totals < 0):
            raise ValueError("simulate_doublets: totals must be non-negative and finite")
    pairs = _pairs(pairs, N, sim_doublet_ratio, seed)
    n_sim = int(pairs.shape[0])
    if isinstance(data, DeviceCSR):
        ptrs = [C.c_void_p(a.ptr) for a in (data.indptr, data.indices, data.data)]
    else:
        ptrs = [C.c_void_p(a.ctypes.data) for a in (indptr, indices, data)]
    f32 = data.dtype == np.float32
    dp = C.POINTER(C.c_double)
    out = np.empty((n_sim, d), dtype=np.float32)

    def run(h):
        st = h.lib.hmx_simulate_doublets(h.h, N, G_all, ptrs[0], ptrs[1], ptrs[2], 1 if f32 else 0, 1 if on_device else 0,
                                         slot.ctypes.data_as(C.POINTER(C.c_int32)), loadings.loadings.ctypes.data_as(dp), loadings.mean.ctypes.data_as(dp),
                                         loadings.sd.ctypes.data_as(dp), G, d, loadings.scale, 0.0 if loadings.clip is None else loadings.clip,
                                         None if totals is None else totals.ctypes.data_as(dp), n_sim, pairs.ctypes.data_as(C.POINTER(C.c_int64)),
                                         C.c_void_p(out.ctypes.data), 0)
        h.check(st, "simulate_doublets")

    if _handle is not None:
        run(_handle)
    else:
        with _Handle(device) as h:
            run(h)
    return out, pairs


def _k_adj(k_adj, N):
    k = int(k_adj)
    if k != k_adj or k < 1 or k > MAX_K:
        raise ValueError("k_adj must be an integer in 1 .. %d" % MAX_K)
    if k >= N:
        raise ValueError("k_adj = %d needs more than the %d other cells" % (k, N - 1))
    return k


def doublet_neighbors(obs_pcs, sim_pcs, k_adj, device=None, return_knn=False):
    """Of every cell's k_adj nearest other cells in the combined set (observed rows first, then synthetic), how many are synthetic.
    obs_pcs n_obs x d, sim_pcs n_sim x d (float32 or float64).  The neighbours are knn()'s: exact, self excluded, ties to the smaller index.
    -> int32 [n_obs + n_sim]; return_knn: (counts, idx, dist) with the lists as knn() returns them."""
    O, _ = _rows(obs_pcs, "obs_pcs")
    S, _ = _rows(sim_pcs, "sim_pcs")
    if O.shape[1] != S.shape[1]:
        raise ValueError("sim_pcs has %d PCs, obs_pcs %d" % (S.shape[1], O.shape[1]))
    n_obs, n_sim, d = O.shape[0], S.shape[0], O.shape[1]
    k = _k_adj(k_adj, n_obs + n_sim)
    f32 = O.dtype == np.float32 and S.dtype == np.float32
    X = np.ascontiguousarray(np.vstack([O, S]), dtype=np.float32 if f32 else np.float64)
    counts = np.empty(n_obs + n_sim, dtype=np.int32)
    idx = np.empty((n_obs + n_sim, k), dtype=np.int32) if return_knn else None
    dist = np.empty((n_obs + n_sim, k), dtype=np.float32) if return_knn else None
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    with _Handle(device) as h:
        h.check(h.lib.hmx_doublet_neighbors(h.h, C.c_void_p(X.ctypes.data), 1 if f32 else 0, 0, n_obs, n_sim, d, k, counts.ctypes.data_as(ip),
                                            None if idx is None else idx.ctypes.data_as(ip), None if dist is None else dist.ctypes.data_as(fp)),
                "doublet_neighbors")
    return (counts, idx, dist) if return_knn else counts


def doublet_scores_from_counts(n_sim_neighbors, k_adj, n_obs, n_sim, expected_doublet_rate=0.1, stdev_doublet_rate=0.02):
    """Scrublet's Bayesian doublet score from the number n of synthetic cells among a cell's k_adj neighbours, in fp64 NumPy.  With
    r = n_sim / n_obs and rho the expected doublet rate:  q = (n + 1) / (k_adj + 2),  L = q rho / r / (1 - rho - q (1 - rho - rho / r)),
    se_q = sqrt(q (1 - q) / (k_adj + 3)),  se_L = q rho / r / (1 - rho - q (1 - rho - rho / r))^2 sqrt((se_q / q (1 - rho))^2 +
    (stdev / rho (1 - q))^2).  -> (score, score_se), one per entry of n_sim_neighbors."""
    n = np.asarray(n_sim_neighbors)
    k = int(k_adj)
    if k != k_adj or k < 1:
        raise ValueError("doublet_scores_from_counts: k_adj must be a positive integer")
    if n.ndim != 1 or n.size < 1:
        raise ValueError("doublet_scores_from_counts: n_sim_neighbors must be a vector")
    if not np.issubdtype(n.dtype, np.integer):
        if not np.all(np.isfinite(n)) or np.any(n != np.floor(n)):
            raise ValueError("doublet_scores_from_counts: n_sim_neighbors must be integers")
    if np.any(n < 0) or np.any(n > k):
        raise ValueError("doublet_scores_from_counts: n_sim_neighbors must lie in 0 .. k_adj")
    if int(n_obs) < 1 or int(n_sim) < 1:
        raise ValueError("doublet_scores_from_counts: n_obs and n_sim must be positive")
    rho, sd = float(expected_doublet_rate), float(stdev_doublet_rate)
    if not (0 < rho < 1) or not np.isfinite(sd) or sd < 0:
        raise ValueError("doublet_scores_from_counts: 0 < expected_doublet_rate < 1 and stdev_doublet_rate >= 0 are required")
    r = float(n_sim) / float(n_obs)
    q = (n.astype(np.float64) + 1.0) / (k + 2.0)
    den = 1.0 - rho - q * (1.0 - rho - rho / r)
    L = q * rho / r / den
    se_q = np.sqrt(q * (1.0 - q) / (k + 3.0))
    se_L = q * rho / r / den ** 2 * np.sqrt((se_q / q * (1.0 - rho)) ** 2 + (sd / rho * (1.0 - q)) ** 2)
    return L, se_L


def doublet_threshold(sim_scores, n_bins=256):
    """The score between the two modes of the simulated doublets' scores: scikit-image's threshold_minimum, which Scrublet calls, restated in
    NumPy.  A histogram of n_bins bins over [min, max] is smoothed by a width-3 mean (edges repeated) until fewer than three local maxima
    remain -- interior bins higher than both sides, a plateau counted once at its middle, the two end bins never --; the centre of the lowest
    bin between the two.  None when exactly two modes never appear (a unimodal sample, or fewer than two distinct scores)."""
    s = np.asarray(sim_scores, dtype=np.float64).reshape(-1)
    if s.size < 1 or not np.all(np.isfinite(s)):
        raise ValueError("doublet_threshold: sim_scores must be finite and not empty")
    n_bins = int(n_bins)
    if n_bins < 3:
        raise ValueError("doublet_threshold: at least 3 bins")
    if s.min() == s.max():
        return None
    h, edges = np.histogram(s, bins=n_bins)
    h = h.astype(np.float64)
    centres = 0.5 * (edges[:-1] + edges[1:])

    def maxima(v):
        """the interior local maxima as threshold_minimum finds them: the middle bin of every plateau that is higher than the bins on both of
        its sides; the first and the last bin are never maxima"""
        out, i, last = [], 1, v.size - 1
        while i < last:
            if v[i - 1] < v[i]:
                j = i + 1
                while j < last and v[j] == v[i]:
                    j += 1
                if v[j] < v[i]:
                    out.append((i + j - 1) // 2)
                    i = j
            i += 1
        return out

    for _ in range(10000):                                       # (threshold_minimum's max_num_iter)
        p = np.concatenate([h[:1], h, h[-1:]])
        h = (p[:-2] + p[1:-1] + p[2:]) / 3.0
        m = maxima(h)
        if len(m) < 3:
            break
    if len(m) != 2:
        return None
    lo, hi = m
    return float(centres[lo + int(np.argmin(h[lo:hi + 1]))])


def default_neighbors(N, sim_doublet_ratio_actual, n_neighbors=None):
    """(n_neighbors, k_adj, capped): Scrublet's n_neighbors = round(0.5 sqrt(N)) and k_adj = round(n_neighbors (1 + r)); when k_adj would exceed
    the 128 neighbours the exact search returns, k_adj = 128 and n_neighbors is reduced to the largest value that gives k_adj <= 128"""
    r = float(sim_doublet_ratio_actual)
    if n_neighbors is None:
        n_neighbors = int(round(0.5 * np.sqrt(N)))
    n_neighbors = int(n_neighbors)
    if n_neighbors < 1:
        raise ValueError("scrub_doublets: n_neighbors must be at least 1")
    k_adj = int(round(n_neighbors * (1.0 + r)))
    if k_adj <= MAX_K:
        return n_neighbors, max(k_adj, 1), False
    n_neighbors = max(1, int(np.floor(MAX_K / (1.0 + r))))
    return n_neighbors, MAX_K, True


def scrub_doublets(counts, genes, loadings=None, n_top_genes=2000, d=30, sim_doublet_ratio=2.0, n_neighbors=None, expected_doublet_rate=0.1,
                   stdev_doublet_rate=0.02, threshold=None, seed=0, device=None, verbose=False):
    """Scrublet end to end on the GPU.  counts, genes: as for project_query.  loadings: a HarmonyLoadings, or None: fitted on the observed
    counts by fit_loadings(n_top_genes, d, seed) -- Scrublet, too, fits its PCA on the observed cells alone.  The embedding is this library's
    (log1p of CP10k, standardised by the loadings' tables, then the loadings: what scanpy's wrapper does with log_transform=True); the
    simulation (pairs with replacement, summed raw counts) and the scoring are Scrublet's.  n_neighbors defaults to round(0.5 sqrt(N)) and
    k_adj = round(n_neighbors (1 + r)) with r = n_sim / N.  The exact search returns at most 128 neighbours: when k_adj would exceed 128 it
    is CAPPED at 128 and n_neighbors reduced accordingly (said with verbose) -- the one place this differs from Scrublet's defaults; with
    r = 2 it applies above about 7 000 cells.  threshold: a score, or None: doublet_threshold of the simulated scores.
    -> dict(score, score_se (observed cells), sim_score, predicted (bool per observed cell, or None without a threshold), threshold, pairs,
    k_adj, n_neighbors)."""
    if loadings is not None and not isinstance(loadings, HarmonyLoadings):
        raise ValueError("scrub_doublets: loadings must be a HarmonyLoadings or None")
    if not (np.isfinite(sim_doublet_ratio) and sim_doublet_ratio > 0):
        raise ValueError("scrub_doublets: sim_doublet_ratio must be positive")
    rho = float(expected_doublet_rate)
    if not (0 < rho < 1) or not np.isfinite(stdev_doublet_rate) or stdev_doublet_rate < 0:
        raise ValueError("scrub_doublets: 0 < expected_doublet_rate < 1 and stdev_doublet_rate >= 0 are required")
    if threshold is not None and not np.isfinite(threshold):
        raise ValueError("scrub_doublets: threshold must be finite (None: found from the simulated scores)")
    if n_neighbors is not None and int(n_neighbors) < 1:
        raise ValueError("scrub_doublets: n_neighbors must be at least 1")
    genes = np.asarray(genes).astype(str).reshape(-1)
    if genes.size < 1:
        raise ValueError("scrub_doublets: no genes")
    csr = _as_csr(counts, int(genes.size))
    N = csr[3]
    n_sim = int(round(float(sim_doublet_ratio) * N))
    if N < 2 or n_sim < 1:
        raise ValueError("scrub_doublets: at least two cells and one synthetic cell are needed")
    n_neighbors, k_adj, capped = default_neighbors(N, n_sim / float(N), n_neighbors)
    k_adj = min(k_adj, N + n_sim - 1)
    if capped and verbose:
        _message("scrub_doublets: k_adj capped at %d (the exact search's list width); n_neighbors reduced to %d" % (MAX_K, n_neighbors))
    if loadings is None:
        from .pca import fit_loadings
        loadings, _, _ = fit_loadings(counts, genes, n_top_genes=min(int(n_top_genes), MAX_TABLE_GENES), d=d, seed=seed, device=device)
    obs = project_query(counts, genes, loadings, device=device)
    sim, pairs = simulate_doublets(counts, genes, loadings, sim_doublet_ratio=sim_doublet_ratio, seed=seed, device=device)
    n = doublet_neighbors(obs, sim, k_adj, device=device)
    score, se = doublet_scores_from_counts(n, k_adj, N, n_sim, expected_doublet_rate=rho, stdev_doublet_rate=stdev_doublet_rate)
    if threshold is None:
        threshold = doublet_threshold(score[N:])
    predicted = None if threshold is None else score[:N] > threshold
    return dict(score=score[:N], score_se=se[:N], sim_score=score[N:], predicted=predicted, threshold=threshold, pairs=pairs, k_adj=k_adj,
                n_neighbors=n_neighbors)
