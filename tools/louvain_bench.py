"""Time the Louvain clustering (hmx_louvain) of Seurat's SNN graph at 1M cells x 50 PCs, k = 20, prune = 1/15, resolution 0.8; writes
profiles/louvain_bench.json (--out) and prints it as one JSON line.

    python tools/louvain_bench.py [--cells 1000000] [--d 50] [--k 20] [--resolution 0.8] [--repeats 3] [--warmup 1] [--no-cpu]

The embedding is bench_data.synth's; the graph is built once by harmony_amd.snn and handed to the library from the host, as Harmony.clusters
does: "timer:louvain" alone is timed, medians over --repeats calls with the spread (max - min) / median.  It includes the upload of the CSR
(`csr_bytes`), which a graph that stayed in HBM between the two calls would not pay; `upload_ms_at_50GBs` says what that is worth at the
host link's rate.  Clusters, levels, sweeps and the modularity are recorded, and whether every call gave the same labels.  For comparison, on
this machine's CPU (one thread): networkx's louvain_communities on the same graph when networkx imports and --cpu-cells allows it (it holds
the graph as Python dictionaries: above 200 000 cells it is skipped and the file says so)."""
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
from harmony_amd import snn  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.louvain import _louvain_call, _weighted_graph  # noqa: E402


def get(h, name):
    out = (C.c_double * 1)()
    h.lib.hmx_get(h.h, name.encode(), out, 1)
    return float(out[0])


def networkx_louvain(indptr, indices, weights, resolution):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(indptr.size - 1))
    src = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    up = src < indices
    G.add_weighted_edges_from(zip(src[up].tolist(), indices[up].tolist(), weights[up].tolist()))
    t0 = time.perf_counter()
    parts = nx.community.louvain_communities(G, seed=0, resolution=resolution)
    sec = time.perf_counter() - t0
    return sec, len(parts), nx.community.modularity(G, parts, resolution=resolution)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--prune", type=float, default=1.0 / 15.0)
    ap.add_argument("--resolution", type=float, default=0.8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true", help="skip networkx")
    ap.add_argument("--cpu-cells", type=int, default=200000, help="largest graph handed to networkx")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "louvain_bench.json"))
    a = ap.parse_args()
    N, d, k = a.cells, a.d, a.k
    Z, _, _ = synth(N, d=d, levels=(10,), seed=11)
    t0 = time.perf_counter()
    g = snn(np.ascontiguousarray(Z, dtype=np.float32), k=k, prune=a.prune)[1]
    snn_wall = 1e3 * (time.perf_counter() - t0)
    indptr, indices, weights, _ = _weighted_graph(g)
    res = {"what": "hmx_louvain", "cells": N, "d": d, "k": k, "prune": a.prune, "resolution": a.resolution, "repeats": a.repeats, "warmup": a.warmup,
           "entries": int(indices.size), "snn_wall_ms": snn_wall, "csr_bytes": 8.0 * indices.size + 8.0 * (N + 1)}
    res["upload_ms_at_50GBs"] = res["csr_bytes"] / 50e9 * 1e3
    ts, first, same = [], None, True
    with _Handle() as h:
        for i in range(a.warmup + a.repeats):
            r = _louvain_call(h.lib, h.h, h.check, indptr, indices, weights, N, a.resolution, 10, 32)
            ms = get(h, "timer:louvain")
            print("call %d: louvain %.1f ms, %d clusters, Q %.6f, levels %s" % (i, ms, r.n_clusters, r.modularity, r.levels), file=sys.stderr, flush=True)
            if i >= a.warmup:
                ts.append(ms)
            if first is None:
                first = r
            else:
                same = same and np.array_equal(r.labels, first.labels) and r.levels == first.levels and r.modularity == first.modularity
        res.update({"levels": int(get(h, "louvain:levels")), "best_level": int(get(h, "louvain:best_level")), "sweeps": int(get(h, "louvain:sweeps")),
                    "short_cap": int(get(h, "louvain:short_cap")), "long_rows": int(get(h, "louvain:long_rows"))})
    med = float(np.median(ts))
    res.update({"louvain_ms": med, "louvain_ms_all": ts, "louvain_spread": (max(ts) - min(ts)) / med, "clusters": first.n_clusters,
                "modularity": first.modularity, "level_clusters": [lv[0] for lv in first.levels], "level_sweeps": [lv[1] for lv in first.levels],
                "level_modularity": [lv[2] for lv in first.levels], "largest_cluster": int(np.bincount(first.labels).max()),
                "same_bits_every_call": bool(same)})
    if not a.no_cpu:
        try:
            if N > a.cpu_cells:
                res["cpu_skipped"] = "networkx holds the graph as dictionaries: not run above %d cells" % a.cpu_cells
            else:
                sec, parts, q = networkx_louvain(indptr, indices, weights, a.resolution)
                res.update({"cpu_networkx_ms": 1e3 * sec, "cpu_threads": 1, "cpu_clusters": parts, "cpu_modularity": q})
        except ImportError:
            res["cpu_skipped"] = "networkx does not import on this machine"
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
