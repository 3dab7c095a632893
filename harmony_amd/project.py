"""project_query(): raw query counts into the reference's PC space (the first three steps of Symphony's mapQuery, Kang et al., Nat. Commun. 2021).

A query arrives as a sparse cells x genes matrix of counts.  Before it can be mapped it has to be expressed in the PCs of the reference:
library-size normalise and log1p, scale every variable gene by the REFERENCE's mean and standard deviation, multiply by the reference's gene
loadings.  `HarmonyLoadings` carries those three tables with the gene names; they come from whatever produced the reference's PCs:
harmony_amd.pca.fit_loadings on the reference's own counts, or another package (scanpy: ``varm["PCs"]``, ``var["mean"]``, ``var["std"]``;
Seurat: ``Loadings``).  All numerics run in libharmony_mi355x.so (hmx_project_counts, include/harmony_mi355x_project.h); the zeros of the count
matrix are never touched, and with ``out="device"`` the PCs stay in HBM for map_query.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._call import _Handle
from .harmony_obj import HarmonyError
from .utils import _message

FORMAT = "harmony_amd.loadings/1"
MAX_D = 128
MAX_GENES = 1 << 24


class HarmonyLoadings(object):
    """The reference's gene tables: genes (G names, unique), loadings (G x d), mean (G,) >= 0, sd (G,) > 0 of the log-normalised expression,
    the normalisation's scale factor and scanpy's max_value clip (None: no clipping)."""

    def __init__(self, genes, loadings, mean, sd, scale=1e4, clip=None):
        self.genes = np.asarray(genes).astype(str).reshape(-1)
        self.loadings = np.ascontiguousarray(loadings, dtype=np.float64)
        self.mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        self.sd = np.ascontiguousarray(sd, dtype=np.float64).reshape(-1)
        self.scale = float(scale)
        self.clip = None if clip is None else float(clip)
        G = self.genes.size
        if self.loadings.ndim != 2 or self.loadings.shape[0] != G or self.mean.size != G or self.sd.size != G or G < 1 or self.loadings.shape[1] < 1:
            raise ValueError("HarmonyLoadings: genes (G), loadings (G x d), mean (G) and sd (G) do not agree: %s %s %s %s"
                             % (self.genes.shape, self.loadings.shape, self.mean.shape, self.sd.shape))
        if len(set(self.genes.tolist())) != G:
            raise ValueError("HarmonyLoadings: gene names must be unique")
        if not np.all(np.isfinite(self.loadings)):
            raise ValueError("HarmonyLoadings: the loadings must be finite")
        if not np.all(np.isfinite(self.sd)) or np.any(self.sd <= 0):
            raise ValueError("HarmonyLoadings: sd must be positive and finite")
        if not np.all(np.isfinite(self.mean)) or np.any(self.mean < 0):
            raise ValueError("HarmonyLoadings: mean must be non-negative and finite")
        if not (self.scale > 0) or not np.isfinite(self.scale):
            raise ValueError("HarmonyLoadings: scale must be positive")
        if self.clip is not None and (not (self.clip > 0) or not np.isfinite(self.clip)):
            raise ValueError("HarmonyLoadings: clip must be positive (None: no clipping)")

    G = property(lambda s: int(s.genes.size))
    d = property(lambda s: int(s.loadings.shape[1]))

    def save(self, path):
        """.npz of plain arrays plus a format tag; the gene names as a unicode array (no pickle)"""
        with open(path, "wb") as f:
            np.savez(f, format=np.array(FORMAT), genes=self.genes.astype(np.str_), loadings=self.loadings, mean=self.mean, sd=self.sd,
                     scale=np.array(self.scale), clip=np.array(np.nan if self.clip is None else self.clip))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            tag = str(z["format"]) if "format" in z.files else None
            if tag != FORMAT:
                raise ValueError("%s is not a saved HarmonyLoadings (%s)" % (path, FORMAT))
            clip = float(z["clip"])
            return cls(z["genes"], z["loadings"], z["mean"], z["sd"], scale=float(z["scale"]), clip=None if np.isnan(clip) else clip)


class DeviceBuffer(object):
    """An HBM allocation of the HIP runtime the library itself is bound to; freed when the object goes."""

    def __init__(self, nbytes, device=None):
        self._lib = _lib.load()
        self.ptr = None
        if device is not None and self._lib.hipSetDevice(C.c_int(int(device))) != 0:
            raise HarmonyError("no HIP device %r: harmony_amd has no CPU fallback" % (device,))
        p = C.c_void_p()
        if self._lib.hipMalloc(C.byref(p), C.c_size_t(max(int(nbytes), 1))) != 0 or not p.value:
            raise HarmonyError("hipMalloc of %d bytes failed (no HIP device?): harmony_amd has no CPU fallback" % nbytes)
        self.ptr = int(p.value)
        self.nbytes = int(nbytes)

    def __del__(self):
        if getattr(self, "ptr", None):
            self._lib.hipFree(C.c_void_p(self.ptr))
            self.ptr = None

    def _copy(self, dst, src, nbytes, kind):
        if nbytes > self.nbytes:
            raise ValueError("DeviceBuffer: %d bytes do not fit an allocation of %d" % (nbytes, self.nbytes))
        if nbytes and self._lib.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), C.c_int(kind)) != 0:
            raise HarmonyError("hipMemcpy failed")

    def from_host(self, a):
        a = np.ascontiguousarray(a)
        self._copy(self.ptr, a.ctypes.data, a.nbytes, 1)
        return self

    def to_host(self, a):
        """fills the C-contiguous array `a`"""
        self._copy(a.ctypes.data, self.ptr, a.nbytes, 2)
        return a


class DeviceCSR(object):
    """A cells x genes CSR matrix resident in HBM: int64 indptr, int32 indices, float32 / float64 data.  DeviceCSR(data, indices, indptr, shape)
    uploads host arrays; project_query reads it where it lives."""

    def __init__(self, data, indices, indptr, shape, device=None):
        data = np.asarray(data)
        data = np.ascontiguousarray(data, dtype=np.float32 if data.dtype == np.float32 else np.float64).reshape(-1)
        indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        indptr = np.ascontiguousarray(indptr, dtype=np.int64).reshape(-1)
        if len(shape) != 2 or indptr.size != int(shape[0]) + 1 or indices.size != data.size:
            raise ValueError("DeviceCSR: indptr must have shape[0] + 1 entries, indices and data one per stored value")
        self.shape = (int(shape[0]), int(shape[1]))
        self.dtype = data.dtype
        self.nnz = int(data.size)
        self.data = DeviceBuffer(data.nbytes, device).from_host(data)
        self.indices = DeviceBuffer(indices.nbytes, device).from_host(indices)
        self.indptr = DeviceBuffer(indptr.nbytes, device).from_host(indptr)


def gene_slots(query_genes, loadings):
    """slot[g] = the row of `loadings` query gene g corresponds to, or -1 (matched by name)"""
    query_genes = np.asarray(query_genes).astype(str).reshape(-1)
    row = {g: j for j, g in enumerate(loadings.genes.tolist())}
    slot = np.full(query_genes.size, -1, dtype=np.int32)
    seen = set()
    for g, name in enumerate(query_genes.tolist()):
        j = row.get(name)
        if j is None:
            continue
        if j in seen:
            raise ValueError("project_query: the query names gene %r twice" % name)
        seen.add(j)
        slot[g] = j
    return slot


def _as_csr(counts, n_genes):
    """-> (data, indices, indptr, Nq, on_device) of the cells x genes CSR; `n_genes` fixes the orientation"""
    if isinstance(counts, DeviceCSR):
        if counts.shape[1] != n_genes:
            raise ValueError("project_query: a DeviceCSR must be cells x genes; its shape is %s, %d genes were named" % (counts.shape, n_genes))
        return counts, counts, counts, counts.shape[0], True
    if isinstance(counts, tuple):
        if len(counts) != 4:
            raise ValueError("project_query: a CSR tuple is (data, indices, indptr, shape)")
        data, indices, indptr, shape = counts
        if len(shape) != 2 or int(shape[1]) != n_genes:
            raise ValueError("project_query: a CSR tuple must be cells x genes; its shape is %s, %d genes were named" % (tuple(shape), n_genes))
        Nq = int(shape[0])
        data = np.asarray(data)
        data = np.ascontiguousarray(data, dtype=np.float32 if data.dtype == np.float32 else np.float64).reshape(-1)
        indices = np.asarray(indices).reshape(-1)
        indptr = np.asarray(indptr).reshape(-1)
        if indptr.size != Nq + 1 or indices.size != data.size:
            raise ValueError("project_query: indptr must have Nq + 1 entries, indices and data one per stored value")
        if indptr.size and int(indptr[-1]) != data.size:
            raise ValueError("project_query: indptr ends at %d, the matrix stores %d values" % (int(indptr[-1]), data.size))
        return data, np.ascontiguousarray(indices, dtype=np.int32), np.ascontiguousarray(indptr, dtype=np.int64), Nq, False
    if hasattr(counts, "tocsr") and hasattr(counts, "format"):      # a scipy.sparse matrix / array
        X = counts
        if X.ndim != 2:
            raise ValueError("project_query: counts must be a matrix")
        if X.shape[1] != n_genes:
            if X.shape[0] != n_genes:
                raise ValueError("project_query: counts is %d x %d, %d genes were named" % (X.shape[0], X.shape[1], n_genes))
            X = X.T                                                   # (genes x cells CSC: the cells x genes CSR over the same arrays)
        if X.format != "csr":
            X = X.tocsr()
            X.sum_duplicates()
        elif not X.has_canonical_format:
            X = X.copy()
            X.sum_duplicates()
        return _as_csr((X.data, X.indices, X.indptr, X.shape), n_genes)
    X = np.asarray(counts)
    if X.ndim != 2:
        raise ValueError("project_query: counts must be a scipy.sparse matrix, a (data, indices, indptr, shape) tuple or a dense 2-D array")
    if X.shape[1] != n_genes:
        if X.shape[0] != n_genes:
            raise ValueError("project_query: counts is %d x %d, %d genes were named" % (X.shape[0], X.shape[1], n_genes))
        X = X.T
    nz = X != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1), dtype=np.int64)]).astype(np.int64)
    indices = np.nonzero(nz)[1].astype(np.int32)
    return _as_csr((X[nz], indices, indptr, X.shape), n_genes)


def project_query(counts, genes, loadings, totals=None, out="host", device=None, verbose=False, _handle=None):
    """The query's PCs from its raw counts.  counts: cells x genes as a scipy.sparse matrix (any format; genes x cells is accepted, len(genes)
    fixes the orientation the way RunHarmony uses N), a CSR tuple (data, indices, indptr, shape) of numpy arrays, a DeviceCSR (the same arrays
    resident in HBM), or a dense 2-D array; genes: the query's gene names, matched by name to `loadings` (a HarmonyLoadings).  Reference genes the query
    lacks contribute nothing (Symphony fills them with zero after scaling); query genes the reference lacks only count towards the library
    size.  totals: the cells' library sizes (default: the row sums over all query genes).
    Returns cells x d float32; out="device": ((d, Nq, float32, device_pointer), owner) -- the buffer tuple Harmony.map_query / setup accept
    and the object that keeps the allocation alive."""
    if not isinstance(loadings, HarmonyLoadings):
        raise ValueError("project_query: loadings must be a HarmonyLoadings")
    if out not in ("host", "device"):
        raise ValueError("project_query: out must be 'host' or 'device'")
    genes = np.asarray(genes).astype(str).reshape(-1)
    G_all, G, d = int(genes.size), loadings.G, loadings.d
    if G_all < 1:
        raise ValueError("project_query: no query genes")
    data, indices, indptr, Nq, on_device = _as_csr(counts, G_all)
    if Nq < 1:
        raise ValueError("project_query: no cells")
    if d > MAX_D:
        raise ValueError("project_query: the loadings have %d PCs: at most %d are supported" % (d, MAX_D))
    if G > MAX_GENES or G_all > MAX_GENES:
        raise ValueError("project_query: at most 2^24 genes are supported")
    slot = gene_slots(genes, loadings)
    shared = int((slot >= 0).sum())
    if shared == 0:
        raise ValueError("project_query: the query shares no gene with the reference's loadings")
    if verbose:
        _message("project_query: %d of the reference's %d genes are absent from the query" % (G - shared, G))
    if totals is not None:
        totals = np.ascontiguousarray(totals, dtype=np.float64).reshape(-1)
        if totals.size != Nq:
            raise ValueError("project_query: totals must hold one library size per cell")
        if not np.all(np.isfinite(totals)) or np.any(totals < 0):
            raise ValueError("project_query: totals must be non-negative and finite")
    if isinstance(data, DeviceCSR):
        ptrs = [C.c_void_p(a.ptr) for a in (data.indptr, data.indices, data.data)]
        f32 = data.dtype == np.float32
    else:
        ptrs = [C.c_void_p(a.ctypes.data) for a in (indptr, indices, data)]
        f32 = data.dtype == np.float32
    dp = C.POINTER(C.c_double)
    owner = host = None
    if out == "device":
        owner = DeviceBuffer(Nq * d * 4, device)
        optr = C.c_void_p(owner.ptr)
    else:
        host = np.empty((Nq, d), dtype=np.float32)
        optr = C.c_void_p(host.ctypes.data)

    def run(h):
        st = h.lib.hmx_project_counts(h.h, Nq, G_all, ptrs[0], ptrs[1], ptrs[2], 1 if f32 else 0, 1 if on_device else 0,
                                      slot.ctypes.data_as(C.POINTER(C.c_int32)), loadings.loadings.ctypes.data_as(dp), loadings.mean.ctypes.data_as(dp),
                                      loadings.sd.ctypes.data_as(dp), G, d, loadings.scale, 0.0 if loadings.clip is None else loadings.clip,
                                      None if totals is None else totals.ctypes.data_as(dp), optr, 1 if out == "device" else 0)
        h.check(st, "project_counts")

    if _handle is not None:
        run(_handle)
    else:
        with _Handle(device) as h:
            run(h)
    if out == "device":
        return (d, Nq, np.float32, owner.ptr), owner
    return host


class _ObjHandle(object):
    """a Harmony object's handle in the shape project_query's call takes"""

    def __init__(self, obj):
        self.lib, self.h, self.check = obj._lib, obj._h, obj._check


def map_query_counts(counts, genes, meta_data, reference, loadings, vars_use=None, totals=None, lambda_=None, options=None, return_object=False,
                     device=None, verbose=False):
    """map_query from raw counts: project_query(out="device") followed by map_query on the same handle -- the PCs never visit the host.
    Arguments as for project_query and map_query; hmx timers "project" and "map_query" of the returned object time the two steps."""
    from .harmony_obj import Harmony
    from .mapping import prepare_query_args
    obj = Harmony(device=device)
    buf, owner = project_query(counts, genes, loadings, totals=totals, out="device", device=device, verbose=verbose, _handle=_ObjHandle(obj))
    d, Nq = buf[0], buf[1]
    kw, _ = prepare_query_args(np.empty((d, Nq), dtype=np.float32, order="F"), meta_data, reference, vars_use=vars_use, lambda_=lambda_, options=options,
                               verbose=False)
    kw["Zq"] = buf
    obj.map_query(**kw)
    del owner                   # (hmx_map_query has ingested the rows into the handle's own buffers)
    if return_object:
        return obj
    return obj.getZcorr().T
