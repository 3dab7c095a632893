"""gene_stats() and fit_loadings(): the reference side of the count workflow (Symphony's buildReference up to the PCA; Kang et al., Nat. Commun. 2021).

A reference arrives as a sparse cells x genes matrix of counts.  `gene_stats` gives every gene's mean and variance of the log-normalised
expression; `fit_loadings` chooses the variable genes (the largest variances, or the caller's list), standardises them and fits the leading
principal axes by subspace iteration.  The standardised matrix S is never formed: the device holds the contributing entries of the count
matrix once cell-major and once gene-major (hmx_pca_prepare) and applies S and its transpose to a tall-skinny matrix (hmx_pca_apply); the
G x k algebra -- QR, the Rayleigh-Ritz step -- is fp64 NumPy on the host.  S is defined exactly as project_query defines it, so the returned
HarmonyLoadings reproduce the returned PCs bit for bit through project_query, and counts -> fit_loadings -> RunHarmony -> reference_summary ->
map_query_counts runs in this library alone.  Seurat's vst and scanpy's binned dispersion are not implemented: call gene_stats, choose, and
pass genes_use.  All numerics of the matrix run in libharmony_mi355x.so (include/harmony_mi355x_pca.h).
"""
import ctypes as C

import numpy as np

from ._call import _Handle
from .project import MAX_D, DeviceBuffer, DeviceCSR, HarmonyLoadings, _as_csr

MAX_CHOSEN = 16384
_dp = C.POINTER(C.c_double)


def _matrix(counts, n_genes, totals, what):
    """-> (the three CSR pointers, dtype code, location code, N, totals or None, the arrays to keep alive)"""
    data, indices, indptr, N, on_device = _as_csr(counts, n_genes)
    if N < 1:
        raise ValueError("%s: no cells" % what)
    if totals is not None:
        totals = np.ascontiguousarray(totals, dtype=np.float64).reshape(-1)
        if totals.size != N:
            raise ValueError("%s: totals must hold one library size per cell" % what)
        if not np.all(np.isfinite(totals)) or np.any(totals < 0):
            raise ValueError("%s: totals must be non-negative and finite" % what)
    if isinstance(data, DeviceCSR):
        ptrs = [C.c_void_p(a.ptr) for a in (data.indptr, data.indices, data.data)]
    else:
        ptrs = [C.c_void_p(a.ctypes.data) for a in (indptr, indices, data)]
    return ptrs, (1 if data.dtype == np.float32 else 0), (1 if on_device else 0), N, totals, (data, indices, indptr)


def _with_handle(run, device, _handle):
    if _handle is not None:
        return run(_handle)
    with _Handle(device) as h:
        return run(h)


def gene_stats(counts, genes, scale=1e4, totals=None, device=None, _handle=None):
    """Per gene of a cells x genes count matrix (any form project_query accepts; len(genes) fixes the orientation): mean and variance
    (N - 1 in the denominator) of y = log1p(x scale / T) over ALL cells, zeros included, and the number of cells that store a positive count.
    -> dict(mean, var, n_cells, s1, s2, step): s1 = sum y, s2 = sum y^2 as the library returns them (fixed-point sums of the steps `step`:
    the same bits for any residence, slab size and order of the cells)."""
    genes = np.asarray(genes).astype(str).reshape(-1)
    G_all = int(genes.size)
    if G_all < 1:
        raise ValueError("gene_stats: no genes")
    if not (scale > 0) or not np.isfinite(scale):
        raise ValueError("gene_stats: scale must be positive")
    ptrs, f32, loc, N, totals, keep = _matrix(counts, G_all, totals, "gene_stats")
    if N < 2:
        raise ValueError("gene_stats: a variance needs at least two cells")
    n = np.zeros(G_all, dtype=np.int64)
    s1, s2, step = np.zeros(G_all), np.zeros(G_all), np.zeros(2)

    def run(h):
        st = h.lib.hmx_gene_stats(h.h, N, G_all, ptrs[0], ptrs[1], ptrs[2], f32, loc, float(scale),
                                  None if totals is None else totals.ctypes.data_as(_dp), n.ctypes.data_as(C.POINTER(C.c_int64)),
                                  s1.ctypes.data_as(_dp), s2.ctypes.data_as(_dp), step.ctypes.data_as(_dp))
        h.check(st, "gene_stats")

    _with_handle(run, device, _handle)
    del keep
    return dict(mean=s1 / N, var=(s2 - s1 * s1 / N) / (N - 1), n_cells=n, s1=s1, s2=s2, step=step)


class StandardisedMatrix(object):
    """S (cells x G) of the G chosen genes of a count matrix as an operator on the device: apply(V) -> (W = S^T (S V), P = S V).
    slot[g] = the column of gene g or -1; mean, sd: the G columns' centring and scaling; clip: scanpy's max_value.  close() (or leaving the
    `with` block) frees the prepared lists; apply() afterwards raises HarmonyError (status 6)."""

    def __init__(self, counts, n_genes, slot, mean, sd, scale=1e4, clip=None, totals=None, device=None, _handle=None):
        self.slot = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        self.mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        self.sd = np.ascontiguousarray(sd, dtype=np.float64).reshape(-1)
        self.G = int(self.mean.size)
        if self.slot.size != int(n_genes) or self.sd.size != self.G or self.G < 1:
            raise ValueError("StandardisedMatrix: slot (one per gene of the matrix), mean and sd (one per chosen gene) do not agree")
        if self.G > MAX_CHOSEN:
            raise ValueError("StandardisedMatrix: at most %d chosen genes are supported" % MAX_CHOSEN)
        ptrs, f32, loc, self.N, totals, keep = _matrix(counts, int(n_genes), totals, "StandardisedMatrix")
        self.device = device
        self._own = _Handle(device) if _handle is None else None
        self._h = self._own if _handle is None else _handle
        try:
            st = self._h.lib.hmx_pca_prepare(self._h.h, self.N, int(n_genes), ptrs[0], ptrs[1], ptrs[2], f32, loc,
                                             self.slot.ctypes.data_as(C.POINTER(C.c_int32)), self.mean.ctypes.data_as(_dp), self.sd.ctypes.data_as(_dp),
                                             self.G, float(scale), 0.0 if clip is None else float(clip),
                                             None if totals is None else totals.ctypes.data_as(_dp))
            self._h.check(st, "pca_prepare")
        except Exception:
            self.close()
            raise
        del keep
        out = (C.c_double * 1)()
        self._h.lib.hmx_get(self._h.h, b"pca_entries", out, 1)
        self.entries = int(out[0])

    def apply(self, V, P=None):
        """V: G x k.  -> (W, P): W = S^T (S V) (G x k float64); P = S V as cells x k float32 (P="host"), as ((k, N, float32, pointer), owner)
        in HBM (P="device"), or None."""
        if P not in (None, "host", "device"):
            raise ValueError("apply: P must be None, 'host' or 'device'")
        if self._h is None:
            raise ValueError("apply: the matrix has been closed")
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != self.G or V.shape[1] < 1:
            raise ValueError("apply: V must be G x k")
        k = int(V.shape[1])
        if k > MAX_D:
            raise ValueError("apply: at most %d columns are supported" % MAX_D)
        W = np.empty((self.G, k), dtype=np.float64)
        host = owner = None
        ptr = None
        if P == "host":
            host = np.empty((self.N, k), dtype=np.float32)
            ptr = C.c_void_p(host.ctypes.data)
        elif P == "device":
            owner = DeviceBuffer(self.N * k * 4, self.device)
            ptr = C.c_void_p(owner.ptr)
        st = self._h.lib.hmx_pca_apply(self._h.h, V.ctypes.data_as(_dp), k, W.ctypes.data_as(_dp), ptr, 1 if P == "device" else 0)
        self._h.check(st, "pca_apply")
        if P == "device":
            return W, ((k, self.N, np.float32, owner.ptr), owner)
        return W, host

    def release(self):
        """frees the prepared lists and keeps the handle: apply() then fails with the library's state error"""
        if self._h is not None:
            self._h.lib.hmx_pca_release(self._h.h)

    def close(self):
        if self._h is not None:
            self._h.lib.hmx_pca_release(self._h.h)
            if self._own is not None:
                self._own.__exit__()
            self._h = self._own = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def choose_genes(var, n_cells, n_top_genes):
    """the n_top_genes genes of largest variance among those at least two cells express, ties broken by gene order; in descending variance"""
    var, n_cells = np.asarray(var, dtype=np.float64), np.asarray(n_cells)
    ok = np.nonzero((n_cells >= 2) & (var > 0))[0]
    return ok[np.argsort(-var[ok], kind="stable")][:int(n_top_genes)]


def subspace_iteration(apply, G, N, d, oversample=10, n_iter=7, seed=0):
    """The leading d eigenvectors of C = S^T S / (N - 1) through `apply`: V -> S^T S V.  -> U (G x d, columns by descending Ritz value, each
    column's entry of largest magnitude positive)."""
    k = min(d + oversample, G)
    V = np.linalg.qr(np.random.default_rng(seed).standard_normal((G, k)))[0]
    for _ in range(int(n_iter)):
        V = np.linalg.qr(apply(V))[0]
    T = V.T @ apply(V)
    lam, Q = np.linalg.eigh((T + T.T) / (2.0 * (N - 1)))
    U = V @ Q[:, np.argsort(-lam)[:d]]
    top = np.abs(U).argmax(axis=0)
    return U * np.sign(U[top, np.arange(d)])


def fit_loadings(counts, genes, genes_use=None, n_top_genes=2000, d=20, oversample=10, n_iter=7, seed=0, scale=1e4, clip=None, totals=None,
                 out="host", device=None, _handle=None):
    """The reference's variable genes, their centring and scaling, the d leading principal axes of the standardised matrix and the cells in them.
    counts, genes, totals: as for project_query.  genes_use: the names of the genes to use, or None: the n_top_genes genes of largest variance
    of the log-normalised expression among those at least two cells express (ties by gene order).  The fit is subspace iteration on
    C = S^T S / (N - 1): a random G x min(d + oversample, G) start (default_rng(seed)), n_iter rounds of V <- qr(C V), a Rayleigh-Ritz step.
    It converges like (lambda_(d + oversample + 1) / lambda_d)^n_iter: a spectrum without a gap behind the d-th value needs more rounds or a
    wider block.  -> (HarmonyLoadings, pcs, explained_variance): pcs = S U as cells x d float32 (out="device": the buffer tuple and its owner,
    as project_query returns them), equal bit for bit to project_query(counts, genes, loadings); explained_variance = diag(U^T C U)."""
    if out not in ("host", "device"):
        raise ValueError("fit_loadings: out must be 'host' or 'device'")
    genes = np.asarray(genes).astype(str).reshape(-1)
    G_all = int(genes.size)
    if len(set(genes.tolist())) != G_all:
        raise ValueError("fit_loadings: gene names must be unique")
    d = int(d)
    if d < 1 or d > MAX_D or int(oversample) < 0 or int(n_iter) < 0:
        raise ValueError("fit_loadings: 1 <= d <= %d, oversample >= 0 and n_iter >= 0 are required" % MAX_D)
    gs = gene_stats(counts, genes, scale=scale, totals=totals, device=device, _handle=_handle)
    if genes_use is None:
        chosen = choose_genes(gs["var"], gs["n_cells"], n_top_genes)
    else:
        row = {g: i for i, g in enumerate(genes.tolist())}
        names = np.asarray(genes_use).astype(str).reshape(-1).tolist()
        if len(set(names)) != len(names) or any(g not in row for g in names):
            raise ValueError("fit_loadings: genes_use must name genes of the matrix, each once")
        chosen = np.array([row[g] for g in names], dtype=np.int64)
        if np.any(gs["var"][chosen] <= 0):
            raise ValueError("fit_loadings: a gene of genes_use has no variance")
    G = int(chosen.size)
    if G < d:
        raise ValueError("fit_loadings: %d usable genes, %d PCs asked for" % (G, d))
    if min(d + int(oversample), G) > MAX_D:
        raise ValueError("fit_loadings: d + oversample must not exceed %d" % MAX_D)
    mean, sd = gs["mean"][chosen], np.sqrt(gs["var"][chosen])
    slot = np.full(G_all, -1, dtype=np.int32)
    slot[chosen] = np.arange(G, dtype=np.int32)
    with StandardisedMatrix(counts, G_all, slot, mean, sd, scale=scale, clip=clip, totals=totals, device=device, _handle=_handle) as S:
        U = subspace_iteration(lambda V: S.apply(V)[0], G, S.N, d, oversample=oversample, n_iter=n_iter, seed=seed)
        W, pcs = S.apply(U, P=out)
        N = S.N
    ev = np.einsum("ij,ij->j", U, W) / (N - 1)
    return HarmonyLoadings(genes[chosen], U, mean, sd, scale=scale, clip=clip), pcs, ev
