"""Time hmx_gene_stats_grouped beside hmx_gene_stats at 1M cells x 30 000 genes, about 2000 stored counts per cell, for B = 1, 8 and 200 groups,
with the CSR matrix resident in HBM and on the host; writes profiles/group_stats_bench.json (--out) and prints it as one JSON line.

    python tools/group_stats_bench.py [--cells 1000000] [--repeats 3] [--warmup 1] [--residence device,host] [--groups 1,8,200]

The matrix is tools/project_bench.py's synthetic one (tools/pca_bench.py's).  The labels are interleaved, label(i) = i mod B: the worst order for
a slab of a host-resident matrix, whose cells then spread over all groups, and for the gather of a device-resident one, whose chunks of one
group take every B-th row.  The yardstick is gene_stats itself, timed in the same process on the same matrix: the grouped pass reads the same
bytes the same way, so the figure of merit is the ratio grouped / ungrouped per B, judged against the run-to-run spread of gene_stats
((max - min) / median of all its timed calls); the two calls alternate round by round, so that both see the same machine.  Every figure is by
the library's own timers ("gene_stats", "gene_stats_grouped": the whole call, with the host's sort of the labels and the copy and conversion
of the B x G_all accumulators in it)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from harmony_amd import Harmony, gene_stats, gene_stats_by_group  # noqa: E402
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402
from project_bench import synthetic_block  # noqa: E402


def alternating(fns, warmup, repeats):
    """fns: (call, timer) pairs run one after the other, round by round -> per pair its `repeats` timer readings after `warmup` untimed rounds"""
    ts = [[] for _ in fns]
    for i in range(warmup + repeats):
        for k, (fn, timer) in enumerate(fns):
            fn()
            if i >= warmup:
                ts[k].append(float(timer()))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--block", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--residence", default="device,host")
    ap.add_argument("--groups", default="1,8,200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_stats_bench.json"))
    a = ap.parse_args()
    G_all = 30000
    rng = np.random.default_rng(5)
    block = min(a.block, a.cells)
    reps = (a.cells + block - 1) // block
    bd, bi, bp = synthetic_block(rng, block, G_all)
    data, indices = np.tile(bd, reps), np.tile(bi, reps)
    indptr = np.concatenate([[0]] + [bp[1:] + r * bp[-1] for r in range(reps)]).astype(np.int64)
    N, nnz = block * reps, int(indptr[-1])
    genes = np.array(["g%d" % g for g in range(G_all)])
    obj = Harmony()
    h = _ObjHandle(obj)
    groups = [int(b) for b in a.groups.split(",")]
    res = {"what": "hmx_gene_stats_grouped beside hmx_gene_stats", "cells": N, "G_all": G_all, "nnz": nnz, "nnz_per_cell": nnz / N, "repeats": a.repeats,
           "warmup": a.warmup, "labels": "i mod B", "groups": groups}
    for where in a.residence.split(","):
        X = DeviceCSR(data, indices, indptr, (N, G_all)) if where == "device" else (data, indices, indptr, (N, G_all))
        keep, base_all, r = {}, [], {"by_groups": {}}
        plain = (lambda: keep.update(gs=gene_stats(X, genes, _handle=h)), lambda: obj.timer("gene_stats"))
        for B in groups:      # gene_stats and the grouped call alternate, so that both see the same machine
            labels = (np.arange(N) % B).astype(np.int32)
            tp, tg = alternating([plain, (lambda: keep.update(gg=gene_stats_by_group(X, genes, labels, levels=np.arange(B), _handle=h)),
                                          lambda: obj.timer("gene_stats_grouped"))], a.warmup, a.repeats)
            base_all += tp
            gg, gs = keep["gg"], keep["gs"]
            r["by_groups"][str(B)] = {"ms": float(np.median(tg)), "ms_all": tg, "gene_stats_ms_beside": float(np.median(tp)),
                                      "ratio_to_gene_stats": float(np.median(tg)) / float(np.median(tp)),
                                      "n_cells_add_up": bool(np.array_equal(gg["n_cells"].sum(0), gs["n_cells"])),
                                      "s1_rel_diff_of_sums": float(np.abs(gg["s1"].sum(0) - gs["s1"]).max() / gs["s1"].max())}
        base = float(np.median(base_all))
        r.update({"gene_stats_ms": base, "gene_stats_ms_all": base_all, "gene_stats_spread": (max(base_all) - min(base_all)) / base,
                  "slabs": int(obj._scalar("project_slabs")) if where == "host" else 1})
        res[where + "_resident"] = r
        del X, keep
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
