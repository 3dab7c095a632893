"""Time hmx_simulate_doublets and hmx_doublet_neighbors at 10^5 and 10^6 observed cells x 30 000 genes, 2000 reference genes, 50 PCs, r = 2
synthetic doublets per cell, about 1000 stored counts per cell, with the CSR matrix resident in HBM; writes profiles/doublets_bench.json (--out)
and prints it as one JSON line.

    python tools/doublets_bench.py [--cells 100000,1000000] [--repeats 5] [--warmup 1] [--neighbors-cells 100000]

The matrix is synthetic as in tools/project_bench.py: a block of `--block` cells is drawn (row lengths 750 .. 1250, columns distinct within a row
and unsorted, geometric counts as float32) and repeated to `cells` rows.  Timed, each the median of `repeats` calls after `warmup` untimed
ones, on the host around simulate_doublets (name matching and the draw of the pairs included) and by the library's own timer.  The byte bound
comes from the shapes: a synthetic cell reads its two parents twice (the library sizes, then the values: 8 bytes per stored entry and read),
at 6.3 TB/s if every read came from HBM -- the second read of a row is expected to hit L2 -- plus the gathered rows of the loadings (256 bytes
per contributing slot, served from L2).  The neighbour counts are timed at `--neighbors-cells` observed cells on random PCs (the exact search's
time does not depend on the values).  No time is promised in advance: DESIGN "Doublet detection" quotes what this writes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from harmony_amd import Harmony, HarmonyLoadings, simulate_doublets  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def synthetic_block(rng, cells, G_all):
    lens = rng.integers(750, 1251, cells)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.repeat(np.arange(cells), lens)
    k = np.arange(indptr[-1]) - indptr[rows]
    strides = np.array([s for s in range(7, 4000, 2) if np.gcd(s, G_all) == 1])
    start, stride = rng.integers(0, G_all, cells), strides[rng.integers(0, strides.size, cells)]
    indices = ((start[rows] + k * stride[rows]) % G_all).astype(np.int32)      # distinct within a row (stride coprime to G_all, length < G_all)
    data = rng.geometric(0.4, size=indices.size).astype(np.float32)
    return data, indices, indptr


def median_of(fn, timer, warmup, repeats):
    ts = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            ts.append((1e3 * (t1 - t0), timer()))
    a = np.array(ts)
    m = np.median(a, axis=0)
    return float(m[0]), float(m[1]), float((a[:, 1].max() - a[:, 1].min()) / m[1])


def simulate_run(cells, block, G_all, G, d, ratio, warmup, repeats):
    rng = np.random.default_rng(5)
    block = min(block, cells)
    reps = (cells + block - 1) // block
    bd, bi, bp = synthetic_block(rng, block, G_all)
    data, indices = np.tile(bd, reps), np.tile(bi, reps)
    indptr = np.concatenate([[0]] + [bp[1:] + r * bp[-1] for r in range(reps)]).astype(np.int64)
    N, nnz = block * reps, int(indptr[-1])
    genes = np.array(["g%d" % g for g in range(G_all)])
    ref = rng.permutation(G_all)[:G]
    L = HarmonyLoadings(genes[ref], rng.standard_normal((G, d)) / np.sqrt(G), rng.uniform(0, 1.5, G), rng.uniform(0.2, 1.5, G))
    pairs = rng.integers(0, N, (int(round(ratio * N)), 2))
    obj = Harmony()
    h = _ObjHandle(obj)
    dev = DeviceCSR(data, indices, indptr, (N, G_all))
    del data, indices
    out = {}
    host_ms, inner, spread = median_of(lambda: out.update(P=simulate_doublets(dev, genes, L, pairs=pairs, _handle=h)[0]),
                                       lambda: obj.timer("simulate_doublets"), warmup, repeats)
    first = out["P"]
    again = simulate_doublets(dev, genes, L, pairs=pairs, _handle=h)[0]
    n_sim = int(pairs.shape[0])
    parent_entries = float(np.diff(indptr)[pairs].sum())                 # stored entries of the two parents, over all synthetic cells
    bound_ms = 1e3 * 2 * 8.0 * parent_entries / HBM_BYTES_PER_S
    return {"cells": N, "n_sim": n_sim, "nnz": nnz, "nnz_per_cell": nnz / N, "ms_median": host_ms, "timer_ms_median": inner, "timer_spread": spread,
            "parent_entries": parent_entries, "bytes_parents_read_twice": 16.0 * parent_entries, "bound_ms_parents_twice_from_hbm": bound_ms,
            "ratio_to_bound": inner / bound_ms, "ns_per_synthetic_cell": 1e6 * inner / n_sim, "out_bytes_to_host": 4.0 * n_sim * d,
            "same_bits_every_call": bool(np.array_equal(first, again))}


def neighbors_run(cells, d, ratio, k_adj, warmup, repeats):
    import ctypes as C
    rng = np.random.default_rng(6)
    n_sim = int(round(ratio * cells))
    X = rng.standard_normal((cells + n_sim, d)).astype(np.float32)
    cnt = np.empty(cells + n_sim, dtype=np.int32)
    with _Handle() as h:
        def call():
            h.check(h.lib.hmx_doublet_neighbors(h.h, C.c_void_p(X.ctypes.data), 1, 0, cells, n_sim, d, k_adj, cnt.ctypes.data_as(C.POINTER(C.c_int32)), None, None),
                    "doublet_neighbors")

        def timer(name):
            out = (C.c_double * 1)()
            h.lib.hmx_get(h.h, name, out, 1)
            return out[0]
        host_ms, knn_ms, _ = median_of(call, lambda: timer(b"timer:knn"), warmup, repeats)
        count_ms = timer(b"timer:doublet_neighbors")
    return {"n_obs": cells, "n_sim": n_sim, "d": d, "k_adj": k_adj, "ms_median": host_ms, "knn_ms_median": knn_ms, "count_ms": count_ms,
            "mean_synthetic_neighbours": float(cnt.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="100000,1000000")
    ap.add_argument("--block", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--neighbors-cells", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "doublets_bench.json"))
    a = ap.parse_args()
    G_all, G, d, ratio = 30000, 2000, 50, 2.0
    res = {"what": "hmx_simulate_doublets, hmx_doublet_neighbors", "G_all": G_all, "G": G, "d": d, "ratio": ratio, "repeats": a.repeats, "warmup": a.warmup,
           "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "runs": [simulate_run(int(c), a.block, G_all, G, d, ratio, a.warmup, a.repeats) for c in a.cells.split(",")]}
    if a.neighbors_cells > 0:
        res["neighbors"] = neighbors_run(a.neighbors_cells, d, ratio, 128, a.warmup, a.repeats)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
