"""Time hmx_reference_moments and hmx_mapping_confidence at 1M cells x 50 PCs, K = 100; writes profiles/r6_confidence_bench.json (--out) and
prints it as one JSON line.

    python tools/confidence_bench.py [--cells 1000000] [--repeats 5] [--warmup 1]

The reference is a Harmony fit (3 iterations) of `cells` synthetic cells; the query is as many cells of the same synthetic structure with 10
levels, mapped once.  Timed, each the median of `repeats` calls after `warmup` untimed ones, on the host around the call (it returns after a
device synchronisation) and by the library's own timer: the moments of the reference ("orig" space), and the confidence of the mapped query
with and without the Nq x K distance matrix (whose copy to the host is part of the call).  The bounds come from the shapes: the fp32 MFMA
flops each pass issues -- the upper triangle of 16 x 16 tiles per (cell, cluster) for the moments, the 16-column groups on and below the
diagonal for the whitening products -- at the fp32 matrix-core peak.
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
from harmony_amd import Harmony, map_query, prepare_setup_args  # noqa: E402
from harmony_amd.utils import harmonize  # noqa: E402

CLOCK = 2.4e9
MFMA_F32_PEAK = 256 * 4 * 64 * CLOCK           # CUs x SIMDs x flop per clock of v_mfma_f32_16x16x4_f32 x 2.4 GHz


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r6_confidence_bench.json"))
    a = ap.parse_args()
    d, K, L, N = 50, 100, 10, a.cells
    NG = (d + 15) // 16
    npairs = NG * (NG + 1) // 2
    Zr, meta, _ = synth(N, d=d, levels=(L,), seed=11)
    skw, _ = prepare_setup_args(Zr.astype(np.float32), meta, "cov0", nclust=K)
    h = Harmony(seed=1)
    h.setup(**skw)
    h.init_cluster_cpp()
    harmonize(h, 3, verbose=False)
    res = {"what": "hmx_reference_moments / hmx_mapping_confidence", "cells": N, "d": d, "K": K, "levels": L, "repeats": a.repeats,
           "warmup": a.warmup, "fp32_mfma_flops_per_s_assumed": MFMA_F32_PEAK}
    host, inner = median_of(lambda: h.reference_summary(moments="orig"), lambda: h.timer("reference_moments"), a.warmup, a.repeats)
    flops = 2.0 * N * K * npairs * 256
    res["reference_moments"] = {"ms_median": host, "timer_ms_median": inner, "mfma_flops": flops, "useful_flops": 2.0 * N * K * d * d,
                                "bound_ms_fp32_mfma": 1e3 * flops / MFMA_F32_PEAK}
    ref = h.reference_summary(moments="orig")
    del h
    Zq, qmeta, _ = synth(N, d=d, levels=(L,), seed=11, shard=3)
    obj = map_query(Zq.astype(np.float32), qmeta, ref, vars_use="cov0", return_object=True)
    flops = 2.0 * N * K * npairs * 256
    for name, rd in (("score_only", False), ("score_and_dist", True)):
        host, inner = median_of(lambda: obj.mapping_confidence(ref, return_dist=rd), lambda: obj.timer("mapping_confidence"), a.warmup, a.repeats)
        res["mapping_confidence_" + name] = {"ms_median": host, "timer_ms_median": inner, "mfma_flops": flops, "bound_ms_fp32_mfma": 1e3 * flops / MFMA_F32_PEAK}
    s = obj.mapping_confidence(ref)
    res["score_median"] = float(np.median(s))
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
