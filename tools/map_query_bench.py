"""Time hmx_map_query at Nq = 1M cells x 50 PCs, K = 100, 10 query levels; prints one JSON line.

    python tools/map_query_bench.py [--cells 1000000] [--repeats 20] [--warmup 3]

The reference is a Harmony fit of 30000 synthetic cells (K = 100); the query is 1M cells of the same synthetic structure.  Two input forms:
fp32 already on the device (torch tensor) and fp64 on the host (the R seam, PCIe ingest included).  Each repeat is one hmx_map_query call on a
fresh handle, timed on the host around the call (the call returns after a device synchronisation), after `--warmup` untimed calls.  The byte
bound counts the HBM traffic of the device work from the shapes: ingest (read the input, write the fp32 rows), pass 1 (read the rows), pass 2
(read the rows, write Z_corr), at 6.3 TB/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_data import synth  # noqa: E402
from harmony_amd import Harmony, prepare_setup_args  # noqa: E402
from harmony_amd.ui import build_phi  # noqa: E402
from harmony_amd.utils import harmonize  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    d, K, L = 50, 100, 10
    Zr, meta, _ = synth(30000, d=d, levels=(10,), seed=11)
    skw, _ = prepare_setup_args(Zr, meta, "cov0", nclust=K)
    h = Harmony(seed=1)
    h.setup(**skw)
    h.init_cluster_cpp()
    harmonize(h, 10, verbose=False)
    ref = h.reference_summary()
    Zq, _, _ = synth(a.cells, d=d, levels=(10,), seed=11, shard=3)
    lev = (np.arange(a.cells) % L).astype(np.int32)
    phi = build_phi([lev], [L])
    B_vec = np.array([L], dtype=np.int32)
    lam = np.array([-1.0])
    host64 = np.asfortranarray(Zq.T, dtype=np.float64)
    dev32 = torch.from_numpy(np.ascontiguousarray(Zq, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    forms = {"fp32_device": (d, a.cells, np.float32, dev32.data_ptr()), "fp64_host": host64}
    out = {"what": "hmx_map_query", "cells": a.cells, "d": d, "K": K, "levels": L, "repeats": a.repeats, "warmup": a.warmup}
    for name, arg in forms.items():
        ts, parts = [], []
        for i in range(a.warmup + a.repeats):
            q = Harmony()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.map_query(arg, phi, B_vec, lam, 0.2, 1e-5, ref)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                ts.append(1e3 * (t1 - t0))
                parts.append([q.timer(p) for p in ("ingest_Z", "map_query_stats", "map_query_solve", "map_query_apply")])
            del q
        p = np.median(np.array(parts), axis=0)
        out[name] = {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)),
                     "median_ms_ingest": float(p[0]), "median_ms_stats": float(p[1]), "median_ms_solve": float(p[2]), "median_ms_apply": float(p[3])}
    zs = (d + 3) // 4 * 4
    rows = a.cells * zs * 4
    passes = 3 * rows                            # pass 1 reads the rows, pass 2 reads them and writes Z_corr
    ingest32 = a.cells * d * 4 + rows
    out["bytes_passes"] = passes
    out["bytes_with_fp32_ingest"] = passes + ingest32
    out["bound_ms_passes"] = 1e3 * passes / HBM_ACHIEVABLE
    out["bound_ms_with_fp32_ingest"] = 1e3 * (passes + ingest32) / HBM_ACHIEVABLE
    out["hbm_bytes_per_s_assumed"] = HBM_ACHIEVABLE
    print(json.dumps(out))


if __name__ == "__main__":
    main()
