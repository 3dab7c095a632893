"""Time hmx_project_counts at 1M query cells x 30 000 genes, 2000 reference genes, 50 PCs, about 2000 stored counts per cell, with the CSR
matrix resident in HBM and on the host; writes profiles/r6_project_bench.json (--out) and prints it as one JSON line.

    python tools/project_bench.py [--cells 1000000] [--repeats 5] [--warmup 1]

The query is synthetic: a block of `--block` cells is drawn (row lengths 1500 .. 2500, columns distinct within a row and unsorted, geometric
counts as float32) and repeated to `cells` rows -- 16 GB of indices and values at the default size.  The PCs are left in HBM (out="device"),
as map_query_counts uses the call.  Timed, each the median of `repeats` calls after `warmup` untimed ones, on the host around project_query
(name matching included) and by the library's own timer.  The bounds come from the shapes: a device-resident matrix is swept twice, 8 bytes per
stored entry and sweep, at 6.3 TB/s if both sweeps came from HBM (the second one of a row is expected to hit L2); a host-resident one crosses
PCIe once.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from harmony_amd import Harmony, HarmonyLoadings, project_query  # noqa: E402
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def synthetic_block(rng, cells, G_all):
    lens = rng.integers(1500, 2501, cells)
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
    m = np.median(np.array(ts), axis=0)
    return float(m[0]), float(m[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--block", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r6_project_bench.json"))
    a = ap.parse_args()
    G_all, G, d = 30000, 2000, 50
    rng = np.random.default_rng(5)
    block = min(a.block, a.cells)
    reps = (a.cells + block - 1) // block
    bd, bi, bp = synthetic_block(rng, block, G_all)
    data, indices = np.tile(bd, reps), np.tile(bi, reps)
    indptr = np.concatenate([[0]] + [bp[1:] + r * bp[-1] for r in range(reps)]).astype(np.int64)
    N, nnz = block * reps, int(indptr[-1])
    genes = np.array(["g%d" % g for g in range(G_all)])
    ref = rng.permutation(G_all)[:G]
    L = HarmonyLoadings(genes[ref], rng.standard_normal((G, d)) / np.sqrt(G), rng.uniform(0, 1.5, G), rng.uniform(0.2, 1.5, G))
    obj = Harmony()
    h = _ObjHandle(obj)
    res = {"what": "hmx_project_counts", "cells": N, "G_all": G_all, "G": G, "d": d, "nnz": nnz, "nnz_per_cell": nnz / N, "repeats": a.repeats,
           "warmup": a.warmup, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    dev = DeviceCSR(data, indices, indptr, (N, G_all))
    host_ms, inner = median_of(lambda: project_query(dev, genes, L, out="device", _handle=h), lambda: obj.timer("project"), a.warmup, a.repeats)
    res["device_resident"] = {"ms_median": host_ms, "timer_ms_median": inner, "bound_ms_two_sweeps_from_hbm": 1e3 * 16.0 * nnz / HBM_BYTES_PER_S,
                              "bound_ms_one_sweep_from_hbm": 1e3 * 8.0 * nnz / HBM_BYTES_PER_S, "bytes_per_s_of_one_sweep": 8.0 * nnz / (1e-3 * inner)}
    (_, _, _, _), owner = project_query(dev, genes, L, out="device", _handle=h)
    first = owner.to_host(np.empty((N, d), dtype=np.float32))
    del dev, owner
    csr = (data, indices, indptr, (N, G_all))
    host_ms, inner = median_of(lambda: project_query(csr, genes, L, out="device", _handle=h), lambda: obj.timer("project"), a.warmup, a.repeats)
    res["host_resident"] = {"ms_median": host_ms, "timer_ms_median": inner, "bytes_over_pcie": 8.0 * nnz + 8.0 * (N + 1),
                            "bytes_per_s": (8.0 * nnz + 8.0 * (N + 1)) / (1e-3 * inner), "slabs": int(obj._scalar("project_slabs"))}
    (_, _, _, _), owner = project_query(csr, genes, L, out="device", _handle=h)
    res["host_equals_device_bits"] = bool(np.array_equal(first, owner.to_host(np.empty_like(first))))
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
