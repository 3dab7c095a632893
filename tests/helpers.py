"""Shared test helpers: drive any backend (oracle or HIP) with the reference's driver logic."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harmony_amd import harmony_options, prepare_setup_args
from harmony_amd.utils import harmonize


def run_backend(obj, data_mat, meta, vars_use, max_iter=10, Y0=None, **kw):
    """RunHarmony.default's call sequence (R/ui.R:269-283) on an already-constructed object."""
    skw, _ = prepare_setup_args(data_mat, meta, vars_use, **kw)
    obj.setup(**skw)
    obj.init_cluster_cpp(Y0) if Y0 is not None else obj.init_cluster_cpp()
    harmonize(obj, max_iter, verbose=False)
    return obj


def chi2(obj):
    O, E = obj.O, obj.E
    return float(np.sum((O - E) ** 2 / E))


from bench_data import synth  # noqa: E402,F401


# ---- the public headers against the library and the binding (the per-feature "header matches the library and the binding" tests) ------------
import ctypes as C  # noqa: E402
import re  # noqa: E402

from harmony_amd import _lib  # noqa: E402

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
# every public header and the table of harmony_amd._lib that binds its functions
PUBLIC_HEADERS = (("harmony_mi355x.h", "SIGNATURES"), ("harmony_mi355x_lab.h", "SIGNATURES"), ("harmony_mi355x_metrics.h", "METRICS_SIGNATURES"),
                  ("harmony_mi355x_silhouette.h", "SILHOUETTE_SIGNATURES"), ("harmony_mi355x_confidence.h", "CONFIDENCE_SIGNATURES"),
                  ("harmony_mi355x_project.h", "PROJECT_SIGNATURES"), ("harmony_mi355x_pca.h", "PCA_SIGNATURES"),
                  ("harmony_mi355x_groups.h", "GROUPS_SIGNATURES"), ("harmony_mi355x_ranksum.h", "RANKSUM_SIGNATURES"),
                  ("harmony_mi355x_graph.h", "GRAPH_SIGNATURES"), ("harmony_mi355x_snn.h", "SNN_SIGNATURES"))
_P = C.POINTER
# a C argument type -> the ctypes a binding may declare for it: scalars and typed pointers; a test names the pointers that its header allows to
# be host or device memory (bound as c_void_p) in `loose`
CTYPES = {"hmx_ctx*": (C.c_void_p,), "int32_t": (C.c_int32,), "int64_t": (C.c_int64,), "double": (C.c_double,), "const void*": (C.c_void_p,),
          "void*": (C.c_void_p,), "const double*": (_P(C.c_double),), "double*": (_P(C.c_double),), "const float*": (_P(C.c_float),),
          "float*": (_P(C.c_float),), "const int32_t*": (_P(C.c_int32),), "int32_t*": (_P(C.c_int32),), "const int64_t*": (_P(C.c_int64),),
          "int64_t*": (_P(C.c_int64),), "uint64_t*": (_P(C.c_uint64),)}


def header_text(header):
    """a public header without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)


def header_names(header):
    """every hmx_ function a header names, its comments included"""
    return set(re.findall(r"\b(hmx_[a-z0-9_]+)\s*\(", open(os.path.join(INCLUDE, header)).read())) - {"hmx_allreduce_fn"}


def header_functions(header):
    """[(name, [argument types])] of the int functions a header declares, in its order"""
    found = re.findall(r"int (hmx_[a-z_]+)\(([^)]*)\)", header_text(header))
    return [(n, [" ".join(a.split()[:-1]) for a in args.replace("\n", " ").split(",")]) for n, args in found]


def assert_header_stands_alone(header, mine):
    """none of the names `mine` of `header` is named by an earlier public header (comments included), declared by a later one (which may cite
    an earlier function in its comments, as the graph header cites hmx_knn), or bound by any other table of _lib"""
    own, earlier = dict(PUBLIC_HEADERS)[header], True
    for other, table in PUBLIC_HEADERS:
        if other == header:
            earlier = False
        elif earlier:
            assert not (set(mine) & header_names(other)), other
        else:
            assert not (set(mine) & set(re.findall(r"\b(hmx_[a-z0-9_]+)\s*\(", header_text(other)))), other
        if table != own:
            assert not (set(mine) & set(getattr(_lib, table))), table


def assert_binding_matches(lib, name, types, sig, loose=None):
    """the loaded function is bound as `sig`, and `sig` is the header's argument list type by type"""
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == sig, name
    assert len(types) == len(sig), name
    for t, s in zip(types, sig):
        assert any(s is o or s == o for o in (loose or {}).get(t, CTYPES[t])), (name, t, s)
