"""map_query(): map new cells into the harmonised space of a fitted reference (Symphony's mapQuery, Kang et al., Nat. Commun. 2021).

The reference is summarised by three arrays taken from a fitted `Harmony` (``reference_summary()``): the cluster masses Nr[k] = sum_i R[k,i],
the R-weighted sums of the corrected embedding C[k,:] = sum_i R[k,i] Z_corr[:,i], and sigma.  The query is soft-assigned to the normalised rows
of C and corrected by one ridge regression per cluster in which the intercept carries the reference's mass (DESIGN "Query mapping").  All
numerics run in libharmony_mi355x.so (hmx_map_query).
"""
import numpy as np

from .harmony_obj import Harmony
from .options import HarmonyOptions, harmony_options
from .ui import _columns, as_factor, build_phi, lambda_vector
from .utils import _message

FORMAT = "harmony_amd.reference/1"
FORMAT_MOMENTS = "harmony_amd.reference/2"      # the same arrays plus the clusters' moments (mean, cov, space)
SPACES = ("orig", "corr")                       # HMX_SPACE_ORIG / HMX_SPACE_CORR of include/harmony_mi355x_confidence.h


class HarmonyReference(object):
    """The summary of a fitted reference: Nr (K,), C (K x d), sigma (K,); optionally the soft clusters' moments that mapping_confidence()
    measures a query against: mean (K x d), cov (K x d x d) and the space ("orig" | "corr") they were taken in."""

    def __init__(self, Nr, C, sigma, mean=None, cov=None, space=None):
        self.Nr = np.asarray(Nr, dtype=np.float64).reshape(-1)
        self.C = np.asarray(C, dtype=np.float64)
        self.sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
        K = self.Nr.size
        if self.C.ndim != 2 or self.C.shape[0] != K or self.sigma.size != K:
            raise ValueError("HarmonyReference: Nr (K), C (K x d) and sigma (K) do not agree: %s %s %s"
                             % (self.Nr.shape, self.C.shape, self.sigma.shape))
        self.mean = self.cov = self.space = None
        if mean is not None or cov is not None:
            if mean is None or cov is None:
                raise ValueError("HarmonyReference: mean and cov come together")
            self.mean = np.asarray(mean, dtype=np.float64)
            self.cov = np.asarray(cov, dtype=np.float64)
            self.space = "orig" if space is None else str(space)
            d = self.C.shape[1]
            if self.mean.shape != (K, d) or self.cov.shape != (K, d, d):
                raise ValueError("HarmonyReference: mean must be K x d = %s and cov K x d x d, got %s and %s"
                                 % ((K, d), self.mean.shape, self.cov.shape))
            if self.space not in SPACES:
                raise ValueError("HarmonyReference: space must be 'orig' or 'corr', got %r" % (space,))
        elif space is not None:
            raise ValueError("HarmonyReference: space without mean and cov")

    K = property(lambda s: int(s.Nr.size))
    d = property(lambda s: int(s.C.shape[1]))

    def save(self, path):
        """.npz of plain arrays plus a format tag"""
        with open(path, "wb") as f:
            if self.mean is None:
                np.savez(f, format=np.array(FORMAT), Nr=self.Nr, C=self.C, sigma=self.sigma)
            else:
                np.savez(f, format=np.array(FORMAT_MOMENTS), Nr=self.Nr, C=self.C, sigma=self.sigma, mean=self.mean, cov=self.cov,
                         space=np.array(self.space))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            tag = str(z["format"]) if "format" in z.files else None
            if tag not in (FORMAT, FORMAT_MOMENTS):
                raise ValueError("%s is not a saved HarmonyReference (%s or %s)" % (path, FORMAT, FORMAT_MOMENTS))
            if tag == FORMAT:
                return cls(z["Nr"], z["C"], z["sigma"])
            return cls(z["Nr"], z["C"], z["sigma"], mean=z["mean"], cov=z["cov"], space=str(z["space"]))


def prepare_query_args(data_mat, meta_data, reference, vars_use=None, lambda_=None, options=None, verbose=False):
    """Everything map_query computes before hmx_map_query: (Harmony.map_query kwargs, data_mat d x Nq)."""
    if options is None:
        options = harmony_options()
    if not isinstance(options, HarmonyOptions):
        raise ValueError("Error: .options must be created from harmony_options()!")
    data_mat = np.asarray(data_mat)
    if data_mat.ndim != 2:
        raise ValueError("data_mat must be a matrix")
    d = reference.d
    cols = None if meta_data is None else _columns(meta_data)
    if meta_data is not None and cols is None:      # a vector of batch values, as RunHarmony accepts
        meta = np.asarray(meta_data)
        if meta.ndim == 1 and meta.shape[0] in data_mat.shape:
            cols = {"batch_variable": meta}
            if vars_use is not None:
                vars_use = "batch_variable"
        else:
            raise ValueError("meta_data must be either a data.frame or a vector with batch values for each cell")
    if isinstance(vars_use, str):
        vars_use = [vars_use]
    if vars_use is not None and (cols is None or any(v not in cols for v in vars_use)):
        raise ValueError("must provide variables names (e.g. vars_use='stim')")
    # orientation (RunHarmony's rule, R/ui.R:178-183): cells x PCs or PCs x cells in
    N = len(next(iter(cols.values()))) if cols else None
    cells_first = data_mat.shape[0] == N if N is not None else (data_mat.shape[0] != d and data_mat.shape[1] == d)
    if cells_first:
        if verbose:
            _message("Transposing data matrix")
        data_mat = data_mat.T
    if N is not None and data_mat.shape[1] != N:
        raise ValueError("number of labels do not correspond to number of samples in data matrix")
    if data_mat.shape[0] != d:
        raise ValueError("the query has %d PCs, the reference %d" % (data_mat.shape[0], d))
    Nq = data_mat.shape[1]
    if vars_use is None:          # one level for all cells
        codes, n_levels = [np.zeros(Nq, dtype=np.int32)], [1]
    else:
        codes, n_levels = [], []
        for v in vars_use:
            c, lv = as_factor(cols[v])
            codes.append(c)
            n_levels.append(len(lv))
    phi = build_phi(codes, n_levels)
    B_vec = np.asarray(n_levels, dtype=np.int32)
    kwargs = dict(Zq=np.asfortranarray(data_mat, dtype=np.float64 if data_mat.dtype != np.float32 else np.float32), Phi=phi, B_vec=B_vec,
                  lambda_vec=lambda_vector(lambda_, B_vec, verbose), alpha=options["alpha"],
                  batch_proportion_cutoff=options["batch_prop_cutoff"], reference=reference)
    return kwargs, data_mat


def map_query(data_mat, meta_data, reference, vars_use=None, lambda_=None, options=None, return_object=False, device=None,
              verbose=False):
    """Map query cells (in the reference's PC space) onto a fitted reference.  `reference`: a HarmonyReference
    (``Harmony.reference_summary()`` of the fit, or ``HarmonyReference.load(path)``).  vars_use=None: one level for all cells.  lambda_:
    None = alpha * E (options["alpha"]), a scalar, or one value per covariate; the kept-level cutoff is options["batch_prop_cutoff"].
    Returns the mapped query as cells x PCs, or the Harmony object (getZcorr / getR / getZorig)."""
    kw, _ = prepare_query_args(data_mat, meta_data, reference, vars_use=vars_use, lambda_=lambda_, options=options, verbose=verbose)
    obj = Harmony(device=device)
    obj.map_query(**kw)
    if return_object:
        return obj
    return obj.getZcorr().T


def mapping_confidence(obj, reference, ridge=0.0, return_dist=False):
    """Per-cell mapping confidence of a mapped query (Symphony's calcPerCellMappingMetric): the R-weighted Mahalanobis distance of every query
    cell to the reference's soft clusters, score[i] = sum_k R[k,i] || U_k (z_i - mean_k) ||, U_k the inverse Cholesky factor of cov_k + ridge I.
    `obj`: the Harmony object of map_query(..., return_object=True); `reference`: a HarmonyReference with moments
    (``Harmony.reference_summary(moments="orig")``).  z_i is the query's Z_orig row for moments taken in "orig", its Z_corr row for "corr".
    Returns score (Nq,), or (score, dist Nq x K float32), in the order the cells were given in.  Large scores: cells the reference does not
    explain.  All numerics run in libharmony_mi355x.so (hmx_mapping_confidence)."""
    if getattr(reference, "mean", None) is None or getattr(reference, "cov", None) is None:
        raise ValueError("mapping_confidence: the reference carries no moments; build it with Harmony.reference_summary(moments='orig')")
    ridge = float(ridge)
    if not (ridge >= 0) or not np.isfinite(ridge):
        raise ValueError("mapping_confidence: ridge must be finite and non-negative")
    if not isinstance(obj, Harmony):
        raise ValueError("mapping_confidence: obj must be the Harmony object of map_query(..., return_object=True)")
    K, d = int(obj.K), int(obj.d)
    if (reference.K, reference.d) != (K, d):
        raise ValueError("mapping_confidence: the reference has K = %d, d = %d, the mapped query K = %d, d = %d" % (reference.K, reference.d, K, d))
    return obj._mapping_confidence(reference.mean, reference.cov, SPACES.index(reference.space), ridge, return_dist)
