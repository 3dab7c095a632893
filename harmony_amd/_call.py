"""What every one-call wrapper of the library shares (metrics, silhouette, project): the handle that lives for one call, the cells x PCs
matrix as the library takes it, and the label columns of a meta_data as factor codes.  Arguments are checked here, before the library is
loaded."""
import ctypes as C

import numpy as np

from . import _lib
from .harmony_obj import HarmonyError
from .ui import _columns, as_factor

MAX_D = 128


class _Handle(object):
    """a handle that lives for one call: it carries the device, the stream and the error text"""

    def __init__(self, device=None):
        self.lib = _lib.load()
        self.h = C.c_void_p(self.lib.hmx_create())
        if not self.h:
            raise HarmonyError("hmx_create failed")
        if device is not None and self.lib.hmx_set_int(self.h, b"device", int(device)) != 0:
            raise HarmonyError("set device: " + self.lib.hmx_last_error(self.h).decode())

    def check(self, status, what):
        if status != 0:
            raise HarmonyError("%s failed (status %d): %s" % (what, status, self.lib.hmx_last_error(self.h).decode()))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.hmx_destroy(self.h)
        self.h = None


def _rows(X, what):
    """cells x PCs -> (C-contiguous float64 / float32 array, dtype code)"""
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("%s must be a cells x PCs matrix" % what)
    if X.shape[1] > MAX_D:
        raise ValueError("%s has %d PCs: at most %d are supported" % (what, X.shape[1], MAX_D))
    f32 = X.dtype == np.float32
    return np.ascontiguousarray(X, dtype=np.float32 if f32 else np.float64), (1 if f32 else 0)


def _factor(values, N, what, wrong_shape="%(what)s must hold one label per cell (%(N)d), got shape %(shape)s"):
    """one label per cell through ui.as_factor: (int32 codes, levels); NaN / missing labels are refused"""
    v = np.asarray(values)
    if v.ndim != 1 or v.shape[0] != N:
        raise ValueError(wrong_shape % {"what": what, "N": N, "shape": v.shape})
    if v.dtype.kind == "f" and np.any(np.isnan(v)) or v.dtype.kind == "O" and any(x is None or x != x for x in v):
        raise ValueError("%s holds NaN / missing labels" % what)
    codes, levels = as_factor(v)
    return np.ascontiguousarray(codes, dtype=np.int32), levels


def _column(meta_data, name, missing="%(name)r does not name a column of meta_data"):
    """the column `name` of meta_data (data.frame-like or a mapping of columns), or ValueError"""
    cols = _columns(meta_data)
    if cols is None:
        raise ValueError("meta_data must be a data.frame-like object or a mapping of columns")
    if not isinstance(name, str) or name not in cols:
        raise ValueError(missing % {"name": name})
    return cols[name]


def _factor_column(meta_data, name, N):
    return _factor(_column(meta_data, name), N, "column %r" % name)
