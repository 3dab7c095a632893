"""Time Seurat's SNN graph (hmx_snn_graph) at 1M cells x 50 PCs for k = 20, prune = 1/15, the neighbour search and the SNN stage separately;
writes profiles/snn_bench.json (--out) and prints it as one JSON line.

    python tools/snn_bench.py [--cells 1000000] [--d 50] [--k 20] [--repeats 3] [--warmup 1] [--no-cpu]

The embedding is bench_data.synth's (float32, resident on the host: the upload is part of "timer:knn", as for hmx_knn).  Every time is by the
library's own timers ("knn", "snn"), medians over --repeats calls with the spread (max - min) / median; "timer:snn" includes the copy of the
CSR to the host.  The library is called as harmony_amd.snn calls it: a first capacity of min(N^2, 6 N k) entries and, when the graph holds
more, once more with the exact count -- the timers are then those of the second call and `retried` says so, `wall_ms` is the whole Python call.
What bounds the stage is reported beside the times: sum_candidates = sum_i C_i, the candidates with multiplicity (each is one 8-byte gather
and one LDS store, then sorted), the entries written, the rows on the long path and the largest in-degree.  For comparison, on this
machine's CPU: scipy's A @ A.T on the same lists with the same pruning (`cpu_scipy_ms`), whose result must equal the library's."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_data import synth  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.snn import _snn_graph  # noqa: E402


def get(h, name):
    out = (C.c_double * 1)()
    h.lib.hmx_get(h.h, name.encode(), out, 1)
    return float(out[0])


def scipy_snn(nn, k, s_min):
    """A @ A.T with the library's pruning rule, on the CPU: (seconds, CSR of float32 weights with ascending rows)"""
    import scipy.sparse as sp
    A = sp.csr_matrix((np.ones(nn.indices.size, dtype=np.int32), nn.indices, nn.indptr), shape=nn.shape)
    t0 = time.perf_counter()
    S = (A @ A.T).tocsr()
    S.data[S.data < s_min] = 0
    S.eliminate_zeros()
    S.sort_indices()
    w = (S.data.astype(np.float64) / (2.0 * k - S.data.astype(np.float64))).astype(np.float32)
    sec = time.perf_counter() - t0
    return sec, sp.csr_matrix((w, S.indices, S.indptr), shape=S.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--prune", type=float, default=1.0 / 15.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true", help="skip scipy's A @ A.T")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snn_bench.json"))
    a = ap.parse_args()
    N, d, k = a.cells, a.d, a.k
    m = k - 1
    Z, _, _ = synth(N, d=d, levels=(10,), seed=11)
    X = np.ascontiguousarray(Z, dtype=np.float32)
    res = {"what": "hmx_snn_graph", "cells": N, "d": d, "k": k, "prune": a.prune, "repeats": a.repeats, "warmup": a.warmup}
    ts = {"knn": [], "snn": [], "wall": []}
    first, same = None, True
    with _Handle() as h:
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            nn, g = _snn_graph(h.lib, h.h, h.check, X, 1, N, d, m, a.prune)
            wall = 1e3 * (time.perf_counter() - t0)
            print("call %d: knn %.1f ms, snn %.1f ms, wall %.1f ms, %d entries" % (i, get(h, "timer:knn"), get(h, "timer:snn"), wall, g.nnz), file=sys.stderr, flush=True)
            if i >= a.warmup:
                ts["knn"].append(get(h, "timer:knn"))
                ts["snn"].append(get(h, "timer:snn"))
                ts["wall"].append(wall)
            if first is None:
                first = (nn, g)
            else:
                same = same and all(np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices)
                                    and np.array_equal(x.data.view(np.uint32), y.data.view(np.uint32)) for x, y in ((nn, first[0]), (g, first[1])))
                del nn, g
        res.update({"s_min": int(get(h, "snn:s_min")), "short_cap": int(get(h, "snn:short_cap")), "window": int(get(h, "snn:window")),
                    "long_rows": int(get(h, "snn:long_rows"))})
    nn, g = first
    med = {key: float(np.median(v)) for key, v in ts.items()}
    col = np.bincount(nn.indices, minlength=N).astype(np.int64)      # in-degree + 1: A's column sums (the diagonal is stored)
    cand = nn.astype(np.int64) @ col
    first_cap = min(N * N, 6 * N * k)
    res.update({"knn_ms": med["knn"], "knn_ms_all": ts["knn"], "snn_ms": med["snn"], "snn_ms_all": ts["snn"], "wall_ms": med["wall"],
                "snn_spread": (max(ts["snn"]) - min(ts["snn"])) / med["snn"], "snn_share_of_knn": med["snn"] / med["knn"],
                "entries": int(g.nnz), "entries_per_row": g.nnz / float(N), "first_capacity": int(first_cap), "retried": bool(g.nnz > first_cap),
                "max_in_degree": int(col.max() - 1), "sum_candidates": int(cand.sum()), "max_candidates": int(cand.max()),
                "csr_copy_bytes": 8.0 * g.nnz + 8.0 * (N + 1), "same_bits_every_call": bool(same)})
    if not a.no_cpu:
        sec, ref = scipy_snn(nn, k, res["s_min"])
        res.update({"cpu_scipy_ms": 1e3 * sec, "cpu_threads": 1, "equals_scipy": bool(np.array_equal(ref.indptr, g.indptr) and np.array_equal(ref.indices, g.indices)
                                                                                    and np.array_equal(ref.data.view(np.uint32), g.data.view(np.uint32)))})
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
