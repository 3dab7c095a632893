"""Time the UMAP layout (hmx_umap_layout) of the neighbors(n_neighbors=15) graph of 1M cells x 50 PCs, 200 epochs from the PCA start; writes
profiles/umap_bench.json (--out) and prints it as one JSON line.

    python tools/umap_bench.py [--cells 1000000] [--d 50] [--n-neighbors 15] [--epochs 200] [--repeats 3] [--warmup 1] [--sample 5000]

The embedding is bench_data.synth's; the graph is built once by harmony_amd.neighbors and handed to the library from the host, as
Harmony.umap does: "timer:umap" alone is timed, medians over --repeats calls with the spread (max - min) / median.  The timer includes the
upload of the CSR and the checks in front of the epochs: a call that asks for no epoch (epochs = (k, k)) pays exactly those, and its median is
`front_ms`.  Counted from the shapes, per epoch: the firings (`fired` / epochs), the bytes they gather (every firing reads 1 +
negative_sample_rate positions of 4 dim bytes) and the bytes every epoch streams (the CSR's indices and weights, indptr, the positions in
and out), set against the time of an epoch.  Whether every call gave the same bits, and the trustworthiness (k = 15) and the kNN purity by the planted cell
type of --sample cells drawn from the result, are recorded.  No CPU UMAP is raced against it: umap-learn is not a dependency of this project."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import umap_ref as ur  # noqa: E402
from bench_data import synth  # noqa: E402
from harmony_amd import neighbors  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.louvain import _weighted_graph  # noqa: E402
from harmony_amd.umap import _layout_call, _Params, pca_init  # noqa: E402


def get(h, name):
    out = (C.c_double * 1)()
    h.lib.hmx_get(h.h, name.encode(), out, 1)
    return float(out[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--min-dist", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=5000, help="cells the trustworthiness is taken on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umap_bench.json"))
    a = ap.parse_args()
    N, d = a.cells, a.d
    Z, _, types = synth(N, d=d, levels=(10,), seed=11)
    X = np.ascontiguousarray(Z, dtype=np.float32)
    indptr, indices, weights, _ = _weighted_graph(neighbors(X, n_neighbors=a.n_neighbors)[1])
    p = _Params(N, 2, a.epochs, a.min_dist, 1.0, None, None, 1.0, 1.0, 5, 0, None)
    Y0 = pca_init(X, 2)
    lens = np.diff(indptr)
    res = {"what": "hmx_umap_layout", "cells": N, "d": d, "n_neighbors": a.n_neighbors, "epochs": a.epochs, "min_dist": a.min_dist, "a": p.a, "b": p.b,
           "negative_sample_rate": p.negative, "repeats": a.repeats, "warmup": a.warmup, "entries": int(indices.size), "longest_row": int(lens.max()),
           "csr_bytes": 8.0 * indices.size + 8.0 * (N + 1)}
    res["upload_ms_at_50GBs"] = res["csr_bytes"] / 50e9 * 1e3
    ts, front, first, same = [], [], None, True
    with _Handle() as h:
        for i in range(a.warmup + a.repeats):
            Y = _layout_call(h.lib, h.h, h.check, indptr, indices, weights, N, Y0, p)
            ms = get(h, "timer:umap")
            fired, long_rows, cap = int(get(h, "umap:fired")), int(get(h, "umap:long_rows")), int(get(h, "umap:short_cap"))
            p.begin = p.end = 0                              # the front alone: upload, checks, the largest weight
            _layout_call(h.lib, h.h, h.check, indptr, indices, weights, N, Y0, p)
            fr = get(h, "timer:umap")
            p.begin, p.end = 0, a.epochs
            print("call %d: umap %.1f ms (front %.1f ms), %d firings" % (i, ms, fr, fired), file=sys.stderr, flush=True)
            if i >= a.warmup:
                ts.append(ms)
                front.append(fr)
            if first is None:
                first = Y
            else:
                same = same and np.array_equal(Y.view(np.uint32), first.view(np.uint32))
    med, fmed = float(np.median(ts)), float(np.median(front))
    epoch_ms = (med - fmed) / a.epochs
    gather = fired / a.epochs * (1 + p.negative) * 4.0 * p.dim
    stream = 8.0 * indices.size + 8.0 * (N + 1) + 2.0 * 4.0 * p.dim * N
    res.update({"umap_ms": med, "umap_ms_all": ts, "umap_spread": (max(ts) - min(ts)) / med, "front_ms": fmed, "front_share": fmed / med,
                "epoch_ms": epoch_ms, "epochs_per_s": 1e3 / epoch_ms, "fired": fired, "firings_per_epoch": fired / a.epochs,
                "gather_bytes_per_epoch": gather, "stream_bytes_per_epoch": stream, "gather_TBps": gather / epoch_ms / 1e9,
                "stream_TBps": stream / epoch_ms / 1e9, "positions_bytes": 4.0 * p.dim * N, "short_cap": cap, "long_rows": long_rows,
                "same_bits_every_call": bool(same), "finite": bool(np.all(np.isfinite(first)))})
    pick = np.sort(np.random.default_rng(0).choice(N, size=min(a.sample, N), replace=False))
    res.update({"sample": int(pick.size), "trustworthiness": ur.trustworthiness(X[pick], first[pick]),
                "trustworthiness_of_start": ur.trustworthiness(X[pick], Y0[pick]),
                "knn_purity": ur.knn_purity(first[pick], types[pick]), "knn_purity_of_input": ur.knn_purity(X[pick], types[pick])})
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
