"""Time hmx_gene_stats, hmx_pca_prepare and one hmx_pca_apply at 1M cells x 30 000 genes, 2000 chosen genes, k = 30, about 2000 stored counts per
cell, with the CSR matrix resident in HBM and on the host; writes profiles/pca_bench.json (--out) and prints it as one JSON line.

    python tools/pca_bench.py [--cells 1000000] [--repeats 3] [--warmup 1]

The matrix is tools/project_bench.py's synthetic one.  Each figure is the median of `repeats` calls after `warmup` untimed ones, by the library's
own timers.  The bounds beside them come from the shapes, at 6.3 TB/s of HBM reads:
    gene_stats   one sweep of 8 bytes per stored entry and gene range (ceil(G_all / 7680) ranges: the LDS tables hold 7680 genes), plus the row
                 sums' sweep per range where it misses L2 -- counted here as one sweep per range;
    prepare      two sweeps of the raw matrix (count, fill) plus the transposition: the compact list (8 bytes per contributing entry) is read
                 twice and written once in each orientation;
    apply        the compact list once per orientation (8 bytes per entry) plus one 256-byte row gather per entry and orientation (V from L2,
                 P from HBM or L2).
A host-resident matrix crosses PCIe once per sweep."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from harmony_amd import Harmony, gene_stats  # noqa: E402
from harmony_amd.pca import StandardisedMatrix  # noqa: E402
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402
from project_bench import HBM_BYTES_PER_S, synthetic_block  # noqa: E402

STAT_GENES = 7680


def median_timer(fn, timer, warmup, repeats):
    ts = []
    for i in range(warmup + repeats):
        fn()
        if i >= warmup:
            ts.append(timer())
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--block", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_bench.json"))
    a = ap.parse_args()
    G_all, G, k = 30000, 2000, 30
    rng = np.random.default_rng(5)
    block = min(a.block, a.cells)
    reps = (a.cells + block - 1) // block
    bd, bi, bp = synthetic_block(rng, block, G_all)
    data, indices = np.tile(bd, reps), np.tile(bi, reps)
    indptr = np.concatenate([[0]] + [bp[1:] + r * bp[-1] for r in range(reps)]).astype(np.int64)
    N, nnz = block * reps, int(indptr[-1])
    genes = np.array(["g%d" % g for g in range(G_all)])
    slot = np.full(G_all, -1, dtype=np.int32)
    slot[rng.permutation(G_all)[:G]] = np.arange(G, dtype=np.int32)
    mean, sd = rng.uniform(0, 1.5, G), rng.uniform(0.2, 1.5, G)
    V = np.linalg.qr(rng.standard_normal((G, k)))[0]
    obj = Harmony()
    h = _ObjHandle(obj)
    ranges = (G_all + STAT_GENES - 1) // STAT_GENES
    res = {"what": "hmx_gene_stats, hmx_pca_prepare, hmx_pca_apply", "cells": N, "G_all": G_all, "G": G, "k": k, "nnz": nnz, "nnz_per_cell": nnz / N,
           "repeats": a.repeats, "warmup": a.warmup, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "gene_ranges": ranges}
    out = {}
    for where, counts in (("device_resident", lambda: DeviceCSR(data, indices, indptr, (N, G_all))), ("host_resident", lambda: (data, indices, indptr, (N, G_all)))):
        X = counts()
        r = {}
        keep = {}
        r["gene_stats_ms"] = median_timer(lambda: keep.update(gs=gene_stats(X, genes, _handle=h)), lambda: obj.timer("gene_stats"), a.warmup, a.repeats)
        S = [None]

        def prepare():
            if S[0] is not None:
                S[0].close()
            S[0] = StandardisedMatrix(X, G_all, slot, mean, sd, _handle=h)
        r["prepare_ms"] = median_timer(prepare, lambda: obj.timer("pca_prepare"), a.warmup, a.repeats)
        entries = S[0].entries
        r["apply_ms"] = median_timer(lambda: keep.update(W=S[0].apply(V)[0]), lambda: obj.timer("pca_apply"), a.warmup, a.repeats)
        t0 = time.perf_counter()
        keep.update(W=S[0].apply(V)[0])
        r["apply_ms_host_clock"] = 1e3 * (time.perf_counter() - t0)
        S[0].close()
        r["slabs"] = int(obj._scalar("project_slabs")) if where == "host_resident" else 1
        out[where] = (keep["gs"], keep["W"])
        res[where] = r
        res["pca_entries"] = entries
        del X
    res["bound_ms"] = {"gene_stats_device": 1e3 * 8.0 * nnz * ranges / HBM_BYTES_PER_S,
                       "prepare_device": 1e3 * (16.0 * nnz + 6 * 8.0 * res["pca_entries"]) / HBM_BYTES_PER_S,
                       "apply_lists": 1e3 * 2 * 8.0 * res["pca_entries"] / HBM_BYTES_PER_S,
                       "apply_row_gathers_from_hbm": 1e3 * 2 * 256.0 * res["pca_entries"] / HBM_BYTES_PER_S}
    (gd, Wd), (gh, Wh) = out["device_resident"], out["host_resident"]
    res["host_equals_device_bits"] = bool(np.array_equal(Wd, Wh) and all(np.array_equal(gd[f], gh[f]) for f in ("n_cells", "s1", "s2")))
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
