"""Time compute_lisi (exact kNN + LISI) at N = 1M cells x 50 PCs, perplexity 30; writes profiles/r7_lisi_bench.json (--out) and prints it as one JSON line.

    python tools/lisi_bench.py [--cells 1000000] [--repeats 3] [--warmup 1] [--no-trace]

Each repeat is one hmx_compute_lisi call (fp32 rows already in HBM, two label columns of 10 and 30 levels) on a fresh handle, timed on the
host around the call (it returns after a device synchronisation); the split into neighbour search and LISI comes from "timer:knn" /
"timer:lisi".  Then ONE run of the same call in a child process under `rocprofv3 --kernel-trace --stats` gives the kernel table.  The bounds
come from the shapes: the distance GEMM's 2 N^2 zs flops (zs = d rounded up to the 16 PCs a group of four fp32 MFMAs covers) at the fp32
matrix-core peak, and the bytes every workgroup of 64 query rows streams (all N data rows) at the HBM rate.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_data import synth  # noqa: E402
from harmony_amd import _lib  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
MFMA_F32_PEAK = 256 * 4 * 64 * 2.4e9           # CUs x SIMDs x flop per clock of v_mfma_f32_16x16x4_f32 x 2.4 GHz


def one_call(lib, X32, N, d, codes, n_levels, perplexity, out):
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    h = C.c_void_p(lib.hmx_create())
    try:
        t0 = time.perf_counter()
        st = lib.hmx_compute_lisi(h, C.c_void_p(X32.data_ptr()), 1, 1, N, d, codes.ctypes.data_as(ip), codes.shape[0], n_levels.ctypes.data_as(ip),
                                  float(perplexity), out.ctypes.data_as(dp))
        t1 = time.perf_counter()
        if st != 0:
            raise RuntimeError(lib.hmx_last_error(h).decode())
        v = (C.c_double * 1)()
        parts = []
        for f in (b"timer:knn", b"timer:lisi"):
            lib.hmx_get(h, f, v, 1)
            parts.append(v[0])
        return 1e3 * (t1 - t0), parts
    finally:
        lib.hmx_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7_lisi_bench.json"))
    ap.add_argument("--child", action="store_true", help="one call and nothing else (the traced run)")
    a = ap.parse_args()
    import torch
    N, d, perplexity = a.cells, 50, 30
    Z, meta, truth = synth(N, d=d, levels=(10,), seed=11)
    codes = np.ascontiguousarray(np.stack([np.asarray(meta["cov0"]), np.asarray(truth) % 30]), dtype=np.int32)
    n_levels = np.array([10, 30], dtype=np.int32)
    X32 = torch.from_numpy(np.ascontiguousarray(Z, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    lib = _lib.load()
    out = np.empty((N, 2))
    if a.child:
        one_call(lib, X32, N, d, codes, n_levels, perplexity, out)
        return
    ts, parts = [], []
    for i in range(a.warmup + a.repeats):
        t, p = one_call(lib, X32, N, d, codes, n_levels, perplexity, out)
        if i >= a.warmup:
            ts.append(t)
            parts.append(p)
    p = np.median(np.array(parts), axis=0)
    zs16 = (d + 15) // 16 * 16
    flops = 2.0 * N * N * zs16
    streamed = ((N + 63) // 64) * N * ((d + 3) // 4 * 4) * 4.0
    res = {"what": "hmx_compute_lisi", "cells": N, "d": d, "perplexity": perplexity, "neighbours": 3 * perplexity - 1, "label_columns": 2,
           "repeats": a.repeats, "warmup": a.warmup, "ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)),
           "median_ms_knn": float(p[0]), "median_ms_lisi": float(p[1]),
           "gemm_flops": flops, "bound_ms_gemm_fp32_mfma": 1e3 * flops / MFMA_F32_PEAK, "fp32_mfma_flops_per_s_assumed": MFMA_F32_PEAK,
           "bytes_streamed_by_workgroups": streamed, "bound_ms_if_streamed_from_hbm": 1e3 * streamed / HBM_ACHIEVABLE,
           "bytes_compulsory": N * d * 4.0 + N * 2 * 8.0, "hbm_bytes_per_s_assumed": HBM_ACHIEVABLE,
           "median_ilisi": float(np.median(out[:, 0])), "median_clisi": float(np.median(out[:, 1]))}
    if not a.no_trace:
        import tempfile
        tdir = tempfile.mkdtemp(prefix="lisi_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "lisi", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--cells", str(N)]
        r = subprocess.run(cmd, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        import csv
        rows, seen = [], []
        for root, _, files in os.walk(tdir):
            for f in files:
                seen.append(f)
                if f.endswith("kernel_stats.csv"):
                    with open(os.path.join(root, f), newline="") as fh:
                        rows += list(csv.DictReader(fh))
        res["kernel_trace"] = [{"kernel": r_["Name"][:60], "calls": int(r_["Calls"]), "total_ms": float(r_["TotalDurationNs"]) / 1e6,
                                "percent": float(r_["Percentage"])} for r_ in rows if "k_knn" in r_["Name"] or "k_lisi" in r_["Name"]]
        if not rows:
            res["kernel_trace_error"] = "rc %d, files %s: %s" % (r.returncode, sorted(seen), (r.stderr or r.stdout)[-300:])
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
