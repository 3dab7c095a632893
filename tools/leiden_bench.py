"""Time the Leiden clustering (hmx_leiden) beside the Louvain clustering (hmx_louvain) on the same SNN graph: 1M cells x 50 PCs, k = 20,
prune = 1/15, resolution 0.8; writes profiles/leiden_bench.json (--out) and prints it as one JSON line.

    python tools/leiden_bench.py [--cells 1000000] [--d 50] [--k 20] [--resolution 0.8] [--repeats 3] [--warmup 1]

The embedding is bench_data.synth's; the graph is built once by harmony_amd.snn and handed to the library from the host, as Harmony.clusters
does.  "timer:leiden" and "timer:louvain" alone are timed, the two calls alternating on one handle, medians over --repeats calls with the
spread (max - min) / median; both include the upload of the CSR.  The phases of the Leiden call are the host's own clocks between the copies
that end them: "timer:leiden_moves" (local moves and the level's record), "timer:leiden_refine" (the refinement with its `cut` per sub-round:
the two interleave on the stream and are not separated here) and "timer:leiden_aggregate".  Clusters, levels, sweeps and the modularity of both
are recorded, whether every call gave the same labels, and the components of the Leiden clusters on the device (one per cluster when
connected)."""
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
from harmony_amd import connected_components, snn  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.leiden import _leiden_call  # noqa: E402
from harmony_amd.louvain import _louvain_call, _weighted_graph  # noqa: E402


def get(h, name):
    out = (C.c_double * 1)()
    h.lib.hmx_get(h.h, name.encode(), out, 1)
    return float(out[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--prune", type=float, default=1.0 / 15.0)
    ap.add_argument("--resolution", type=float, default=0.8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leiden_bench.json"))
    a = ap.parse_args()
    N, d, k = a.cells, a.d, a.k
    Z, _, _ = synth(N, d=d, levels=(10,), seed=11)
    t0 = time.perf_counter()
    g = snn(np.ascontiguousarray(Z, dtype=np.float32), k=k, prune=a.prune)[1]
    snn_wall = 1e3 * (time.perf_counter() - t0)
    indptr, indices, weights, _ = _weighted_graph(g)
    res = {"what": "hmx_leiden", "cells": N, "d": d, "k": k, "prune": a.prune, "resolution": a.resolution, "repeats": a.repeats, "warmup": a.warmup,
           "entries": int(indices.size), "snn_wall_ms": snn_wall, "csr_bytes": 8.0 * indices.size + 8.0 * (N + 1)}
    phases = ("leiden", "leiden_moves", "leiden_refine", "leiden_aggregate", "louvain")
    ts = {p: [] for p in phases}
    first, first_lv, same = None, None, True
    with _Handle() as h:
        for i in range(a.warmup + a.repeats):
            r = _leiden_call(h.lib, h.h, h.check, indptr, indices, weights, N, a.resolution, 20, 32)
            ms = {p: get(h, "timer:" + p) for p in phases[:4]}
            lv = _louvain_call(h.lib, h.h, h.check, indptr, indices, weights, N, a.resolution, 10, 32)
            ms["louvain"] = get(h, "timer:louvain")
            print("call %d: leiden %.1f ms (moves %.1f, refine %.1f, aggregate %.1f), %d clusters, Q %.6f, converged %s; louvain %.1f ms, %d clusters, Q %.6f"
                  % (i, ms["leiden"], ms["leiden_moves"], ms["leiden_refine"], ms["leiden_aggregate"], r.n_clusters, r.modularity, r.converged,
                     ms["louvain"], lv.n_clusters, lv.modularity), file=sys.stderr, flush=True)
            if i >= a.warmup:
                for p in phases:
                    ts[p].append(ms[p])
            if first is None:
                first, first_lv = r, lv
            else:
                same = same and np.array_equal(r.labels, first.labels) and r.levels == first.levels and r.modularity == first.modularity
        res.update({"levels": int(get(h, "leiden:levels")), "sweeps": int(get(h, "leiden:sweeps")), "refine_sweeps": int(get(h, "leiden:refine_sweeps")),
                    "short_cap": int(get(h, "louvain:short_cap")), "long_rows": int(get(h, "leiden:long_rows"))})
    for p in phases:
        med = float(np.median(ts[p]))
        res.update({p + "_ms": med, p + "_ms_all": ts[p], p + "_spread": (max(ts[p]) - min(ts[p])) / med if med else 0.0})
    keep = weights > 0                                     # the pattern of the edges, for the components inside the clusters
    rows = np.repeat(np.arange(N), np.diff(indptr))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=N))]).astype(np.int64)
    res.update({"clusters": first.n_clusters, "modularity": first.modularity, "converged": bool(first.converged),
                "level_clusters": [lv[0] for lv in first.levels], "level_nodes": [lv[1] for lv in first.levels],
                "level_sweeps": [lv[2] for lv in first.levels], "level_refine_sweeps": [lv[3] for lv in first.levels],
                "level_modularity": [lv[4] for lv in first.levels], "largest_cluster": int(np.bincount(first.labels).max()),
                "same_bits_every_call": bool(same), "cut": "recomputed per sub-round",
                "components_within_clusters": int(connected_components((ptr, indices[keep]), first.labels)[0]),
                "louvain_clusters": first_lv.n_clusters, "louvain_modularity": first_lv.modularity,
                "louvain_components_within_clusters": int(connected_components((ptr, indices[keep]), first_lv.labels)[0])})
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
