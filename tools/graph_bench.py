"""Time the neighbour graph (hmx_neighbor_graph) at 1M cells x 50 PCs for n_neighbors = 15 and 30, the neighbour search and the graph stage
separately, and the components with scib's graph connectivity on the result; writes profiles/graph_bench.json (--out) and prints it as one
JSON line.

    python tools/graph_bench.py [--cells 1000000] [--d 50] [--neighbors 15,30] [--repeats 3] [--warmup 1]

The embedding is bench_data.synth's (float32, resident on the host: the upload is part of "timer:knn", as for hmx_knn).  Every time is by the
library's own timers ("knn", "graph", "components"), medians over --repeats calls with the spread (max - min) / median.  The byte bound of
the graph stage at 6.3 TB/s: the lists in (8 B per slot, read by the search of sigma, the placement and both union passes: 4 times), w out
(8 B per slot) and gathered twice, the transposed lists written, sorted in place (read + write) and read by both union passes (8 B per entry, 5
times), the CSR out (8 B per entry).  The copy of the CSR to the host is part of "timer:graph" and not of the bound; it is reported beside it
at the measured size."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_data import synth  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.graph import _neighbor_graph, connectivity_from_components  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def timer(h, name):
    out = (C.c_double * 1)()
    h.lib.hmx_get(h.h, ("timer:" + name).encode(), out, 1)
    return float(out[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--neighbors", default="15,30")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_bench.json"))
    a = ap.parse_args()
    N, d = a.cells, a.d
    Z, meta, _ = synth(N, d=d, levels=(10,), seed=11)
    X = np.ascontiguousarray(Z, dtype=np.float32)
    levels, codes = np.unique(np.asarray(meta["cov0"]), return_inverse=True)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    res = {"what": "hmx_neighbor_graph and hmx_graph_components", "cells": N, "d": d, "repeats": a.repeats, "warmup": a.warmup, "runs": []}
    with _Handle() as h:
        for nn in [int(v) for v in a.neighbors.split(",")]:
            m = nn - 1
            ts = {"knn": [], "graph": []}
            first = None
            same = True
            for i in range(a.warmup + a.repeats):
                out = _neighbor_graph(h.lib, h.h, h.check, X, 1, N, d, m)
                print("n_neighbors %d call %d: knn %.1f ms, graph %.1f ms" % (nn, i, timer(h, "knn"), timer(h, "graph")), file=sys.stderr, flush=True)
                if i >= a.warmup:
                    ts["knn"].append(timer(h, "knn"))
                    ts["graph"].append(timer(h, "graph"))
                if first is None:
                    first = out
                else:
                    same = same and all(np.array_equal(out[k], first[k]) for k in (2, 3)) and np.array_equal(out[4].view(np.uint32), first[4].view(np.uint32))
            indptr, indices = first[2], first[3]
            nnz = int(indptr[N])
            med = {k: float(np.median(v)) for k, v in ts.items()}
            slots = float(N) * m
            bound = 8.0 * (4 * slots + 3 * slots + 5 * slots + nnz)
            r = {"n_neighbors": nn, "knn_ms": med["knn"], "knn_ms_all": ts["knn"], "graph_ms": med["graph"], "graph_ms_all": ts["graph"],
                 "graph_spread": (max(ts["graph"]) - min(ts["graph"])) / med["graph"], "graph_share_of_knn": med["graph"] / med["knn"],
                 "entries": nnz, "max_in_degree": int(np.bincount(first[0].ravel()[first[0].ravel() >= 0], minlength=1).max()),
                 "bound_ms_bytes": 1e3 * bound / HBM_BYTES_PER_S, "share_of_bound": 1e3 * bound / HBM_BYTES_PER_S / med["graph"],
                 "csr_copy_bytes": 8.0 * nnz + 8.0 * (N + 1), "same_bits_every_call": bool(same)}
            cc = []
            for i in range(a.warmup + a.repeats):
                n_all, _ = _components_timed(h, indptr, indices, N, None)
                n_lab, comp = _components_timed(h, indptr, indices, N, codes)
                if i >= a.warmup:
                    cc.append(timer(h, "components"))
            r.update({"components_within_labels_ms": float(np.median(cc)), "components": n_all, "components_within_labels": n_lab,
                      "graph_connectivity": connectivity_from_components(comp, codes, levels.size)})
            res["runs"].append(r)
            print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def _components_timed(h, indptr, indices, N, codes):
    """graph._components on the bench's own handle, so that its timer can be read"""
    comp = np.empty(N, dtype=np.int32)
    n = C.c_int64(0)
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    h.check(h.lib.hmx_graph_components(h.h, N, indptr.ctypes.data_as(lp), indices.ctypes.data_as(ip),
                                       None if codes is None else codes.ctypes.data_as(ip), comp.ctypes.data_as(ip), C.byref(n)), "components")
    return int(n.value), comp


if __name__ == "__main__":
    main()
