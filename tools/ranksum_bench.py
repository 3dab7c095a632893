"""Time hmx_rank_sums beside hmx_gene_stats_grouped at 1M cells x 30 000 genes, about 2000 stored counts per cell, labels i mod 8, with the CSR
matrix resident in HBM and on the host; writes profiles/ranksum_bench.json (--out) and prints it as one JSON line.

    python tools/ranksum_bench.py [--cells 1000000] [--repeats 5] [--warmup 1] [--residence device,host] [--cpu-cells 60000 | 0: skip the CPU yardstick]

The matrix is tools/project_bench.py's synthetic one (tools/pca_bench.py's).  Every time is by the library's own timers: the whole call
("rank_sums") and its three stages (the count sweep, the fill sweeps, sorting and ranking), medians over --repeats calls with the spread
(max - min) / median, and the number of gene blocks.  The yardstick of the parent commit is gene_stats_by_group at B = 8, ONE sweep of the same
bytes, timed in the same process, the two calls alternating round by round.  The byte bound: entries x 8 B x (1 fill write + 2 per radix pass for
the entries on the radix path + 1 read) at 6.3 TB/s.  The CPU yardstick is the scipy spec (2 rankdata per gene summed per group) on the first
--cpu-cells cells, reported as measured, never extrapolated.  The integers of host- and device-resident calls are compared."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from harmony_amd import Harmony, gene_stats_by_group, rank_sums_by_group  # noqa: E402
from harmony_amd.project import DeviceCSR, _ObjHandle  # noqa: E402
from project_bench import synthetic_block  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def cpu_yardstick(data, indices, indptr, G_all, n, B):
    """the scipy spec on the first n cells: seconds for 2 rankdata(method="average") of every gene's dense column, summed per group"""
    try:
        from scipy.stats import rankdata
    except ImportError:
        return None
    ip = indptr[:n + 1]
    d, j = data[:ip[-1]].astype(np.float64), indices[:ip[-1]]
    rows = np.repeat(np.arange(n), np.diff(ip))
    T = np.bincount(rows, weights=d, minlength=n)
    key = (data[:ip[-1]] * (1e4 / T).astype(np.float32)[rows]).astype(np.float32)
    lab = np.arange(n) % B
    t0 = time.perf_counter()
    by = np.argsort(j, kind="stable")
    cut = np.searchsorted(j[by], np.arange(G_all + 1))
    total = 0
    for g in range(G_all):
        col = np.zeros(n, dtype=np.float32)
        col[rows[by[cut[g]:cut[g + 1]]]] = key[by[cut[g]:cut[g + 1]]]
        r2 = 2.0 * rankdata(col, method="average")
        total += int(np.bincount(lab, weights=r2, minlength=B)[0])
    return {"cells": int(n), "genes": int(G_all), "seconds": time.perf_counter() - t0, "checksum": total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--block", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--residence", default="device,host")
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--cpu-cells", type=int, default=60000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranksum_bench.json"))
    a = ap.parse_args()
    G_all, B = 30000, a.groups
    rng = np.random.default_rng(5)
    block = min(a.block, a.cells)
    reps = (a.cells + block - 1) // block
    bd, bi, bp = synthetic_block(rng, block, G_all)
    data, indices = np.tile(bd, reps), np.tile(bi, reps)
    indptr = np.concatenate([[0]] + [bp[1:] + r * bp[-1] for r in range(reps)]).astype(np.int64)
    N, nnz = block * reps, int(indptr[-1])
    genes = np.array(["g%d" % g for g in range(G_all)])
    labels = (np.arange(N) % B).astype(np.int32)
    obj = Harmony()
    h = _ObjHandle(obj)
    S = int(obj._scalar("ranksum_sort_lds"))
    res = {"what": "hmx_rank_sums beside hmx_gene_stats_grouped", "cells": N, "G_all": G_all, "nnz": nnz, "nnz_per_cell": nnz / N, "repeats": a.repeats,
           "warmup": a.warmup, "labels": "i mod %d" % B, "groups": B, "sort_lds": S, "chunk": int(obj._scalar("ranksum_chunk"))}
    timers = ("rank_sums", "rank_sums_count", "rank_sums_fill", "rank_sums_sort")
    first = None
    for where in a.residence.split(","):
        X = DeviceCSR(data, indices, indptr, (N, G_all)) if where == "device" else (data, indices, indptr, (N, G_all))
        keep = {}
        ts = {k: [] for k in timers + ("gene_stats_grouped",)}
        for i in range(a.warmup + a.repeats):      # the two calls alternate, so that both see the same machine
            keep["gg"] = gene_stats_by_group(X, genes, labels, levels=np.arange(B), _handle=h)
            tg = obj.timer("gene_stats_grouped")
            keep["rs"] = rank_sums_by_group(X, genes, labels, levels=np.arange(B), _handle=h)
            print("%s-resident call %d: rank_sums %.1f ms, gene_stats_grouped %.1f ms" % (where, i, obj.timer("rank_sums"), tg), file=sys.stderr, flush=True)
            if i >= a.warmup:
                ts["gene_stats_grouped"].append(float(tg))
                for k in timers:
                    ts[k].append(float(obj.timer(k)))
        rs = keep["rs"]
        med = {k: float(np.median(v)) for k, v in ts.items()}
        P = rs["n_pos"].sum(0)
        entries, radix = int(P.sum()), int(P[P > S].sum())
        bound_bytes = 8.0 * (entries * 2 + radix * 2 * 4)
        r = {"ms": med["rank_sums"], "ms_all": ts["rank_sums"], "spread": (max(ts["rank_sums"]) - min(ts["rank_sums"])) / med["rank_sums"],
             "count_ms": med["rank_sums_count"], "fill_ms": med["rank_sums_fill"], "sort_ms": med["rank_sums_sort"],
             "gene_blocks": int(obj._scalar("ranksum_blocks")), "slabs": int(obj._scalar("project_slabs")) if where == "host" else 1,
             "gene_stats_grouped_ms": med["gene_stats_grouped"], "gene_stats_grouped_ms_all": ts["gene_stats_grouped"],
             "gene_stats_grouped_spread": (max(ts["gene_stats_grouped"]) - min(ts["gene_stats_grouped"])) / med["gene_stats_grouped"],
             "ratio_to_gene_stats_grouped": med["rank_sums"] / med["gene_stats_grouped"],
             "entries": entries, "entries_on_the_radix_path": radix, "bound_ms_list_bytes": 1e3 * bound_bytes / HBM_BYTES_PER_S,
             "n_pos_equals_n_cells": bool(np.array_equal(rs["n_pos"], keep["gg"]["n_cells"])),
             "rank_sums_add_up": bool(np.all(rs["rank2"].sum(0) == N * (N + 1)))}
        if first is None:
            first = rs
        else:
            r["same_integers_as_the_first_residence"] = bool(all(np.array_equal(rs[k], first[k]) for k in ("n_obs", "n_pos", "rank2"))
                                                             and list(rs["tie3"]) == list(first["tie3"]))
        res[where + "_resident"] = r
        print("%s-resident: %s" % (where, json.dumps({k: v for k, v in r.items() if not k.endswith("_all")})), file=sys.stderr, flush=True)
        del X, keep
    res["cpu_scipy_spec"] = cpu_yardstick(data, indices, indptr, G_all, min(a.cpu_cells, N), B) if a.cpu_cells > 0 else None
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
