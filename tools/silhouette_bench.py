"""Time hmx_silhouette at N = 100k and 1M cells x 50 PCs, 10 batches x 20 cell types; writes profiles/r6_silhouette_bench.json (--out) and prints
it as one JSON line.

    python tools/silhouette_bench.py [--cells 100000,1000000] [--repeats 3] [--warmup 1]

Per N, two calls are timed, each the median of `repeats` calls on a fresh handle (fp32 rows already in HBM), on the host around the call (it
returns after a device synchronisation) and by "timer:silhouette": the label silhouette (over the cell type, ungrouped: every pair of cells)
and the batch silhouette (over the batch, grouped by cell type: the pairs within a type only).  hmx_knn with k = 89 on the same rows is the
yardstick -- the same N x N distance GEMM, with a selection in place of the sums.  The bounds come from the shapes: the GEMM's 2 P zs16 flops
over the P pairs a call forms (zs16 = d rounded up to the 16 PCs a group of four fp32 MFMAs covers) at the fp32 matrix-core peak, and one
quarter-rate v_sqrt_f32 per pair.
"""
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
from harmony_amd import _lib  # noqa: E402

CLOCK = 2.4e9
MFMA_F32_PEAK = 256 * 4 * 64 * CLOCK           # CUs x SIMDs x flop per clock of v_mfma_f32_16x16x4_f32 x 2.4 GHz
SQRT_PEAK = 256 * 4 * 4 * CLOCK                # CUs x SIMDs x quarter-rate lanes per clock


def timer(lib, h, name):
    v = (C.c_double * 1)()
    lib.hmx_get(h, name, v, 1)
    return v[0]


def silhouette_call(lib, X32, N, d, labels, n_levels, groups, n_groups, out):
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    h = C.c_void_p(lib.hmx_create())
    try:
        t0 = time.perf_counter()
        st = lib.hmx_silhouette(h, C.c_void_p(X32.data_ptr()), 1, 1, N, d, labels.ctypes.data_as(ip), n_levels,
                                None if groups is None else groups.ctypes.data_as(ip), n_groups, out.ctypes.data_as(dp), None, None)
        t1 = time.perf_counter()
        if st != 0:
            raise RuntimeError(lib.hmx_last_error(h).decode())
        return 1e3 * (t1 - t0), timer(lib, h, b"timer:silhouette")
    finally:
        lib.hmx_destroy(h)


def knn_call(lib, X32, N, d, k, idx, dist):
    h = C.c_void_p(lib.hmx_create())
    try:
        t0 = time.perf_counter()
        st = lib.hmx_knn(h, C.c_void_p(X32.data_ptr()), 1, 1, N, None, 0, 0, 0, d, k, C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()), 1)
        t1 = time.perf_counter()
        if st != 0:
            raise RuntimeError(lib.hmx_last_error(h).decode())
        return 1e3 * (t1 - t0), timer(lib, h, b"timer:knn")
    finally:
        lib.hmx_destroy(h)


def median_of(fn, warmup, repeats):
    ts = np.array([fn() for _ in range(warmup + repeats)][warmup:])
    return [float(v) for v in np.median(ts, axis=0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="100000,1000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r6_silhouette_bench.json"))
    a = ap.parse_args()
    import torch
    lib = _lib.load()
    d, k = 50, 89
    zs16 = (d + 15) // 16 * 16
    res = {"what": "hmx_silhouette", "d": d, "batches": 10, "cell_types": 20, "repeats": a.repeats, "warmup": a.warmup, "knn_k": k,
           "fp32_mfma_flops_per_s_assumed": MFMA_F32_PEAK, "sqrt_per_s_assumed": SQRT_PEAK, "sizes": []}
    for N in [int(v) for v in a.cells.split(",")]:
        Z, meta, truth = synth(N, d=d, n_types=20, levels=(10,), seed=11)
        batch = np.ascontiguousarray(np.asarray(meta["cov0"]), dtype=np.int32)
        ctype = np.ascontiguousarray(np.asarray(truth), dtype=np.int32)
        X32 = torch.from_numpy(np.ascontiguousarray(Z, dtype=np.float32)).cuda()
        idx = torch.empty((N, k), dtype=torch.int32, device="cuda")
        dist = torch.empty((N, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        out = np.empty(N)
        row = {"cells": N}
        for name, labels, nl, groups, ng, pairs in (("label", ctype, 20, None, 0, float(N) * N),
                                                     ("batch_within_label", batch, 10, ctype, 20, float(np.sum(np.bincount(ctype).astype(np.float64) ** 2)))):
            host, inner = median_of(lambda: silhouette_call(lib, X32, N, d, labels, nl, groups, ng, out), a.warmup, a.repeats)
            row[name] = {"ms_median": host, "timer_silhouette_ms_median": inner, "pairs": pairs, "mean_width": float(np.nanmean(out)),
                         "bound_ms_gemm_fp32_mfma": 1e3 * 2.0 * pairs * zs16 / MFMA_F32_PEAK, "bound_ms_sqrt": 1e3 * pairs / SQRT_PEAK}
        host, inner = median_of(lambda: knn_call(lib, X32, N, d, k, idx, dist), a.warmup, a.repeats)
        row["knn"] = {"ms_median": host, "timer_knn_ms_median": inner, "pairs": float(N) * N, "bound_ms_gemm_fp32_mfma": 1e3 * 2.0 * N * N * zs16 / MFMA_F32_PEAK}
        row["label_over_knn"] = row["label"]["ms_median"] / row["knn"]["ms_median"]
        res["sizes"].append(row)
        del X32, idx, dist
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
