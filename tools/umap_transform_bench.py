"""Time the projection of query cells into a fitted UMAP layout (hmx_umap_query_weights, hmx_umap_transform) at a reference of 1M cells x 50 PCs
with 100 000 query cells for 30 epochs and 10 000 query cells for 100 epochs, k = 15; writes profiles/umap_transform_bench.json (--out) and
prints it as one JSON line.

    python tools/umap_transform_bench.py [--reference 1000000] [--d 50] [--k 15] [--runs 100000:30,10000:100] [--repeats 15] [--warmup 2]

The embedding is bench_data.synth's, split into reference and query; the reference's layout is harmony_amd.umap's (--layout-epochs, not timed);
the lists are harmony_amd.knn's ("timer:knn").  Timed: "timer:umap_query_weights" and "timer:umap_transform", medians over --repeats calls with
the spread (max - min) / median.  The transform's timer includes the upload of the lists, the weights and the reference's positions and the
start: a call that asks for no epoch (epochs = (0, 0)) pays exactly those, and its median is `front_ms`.  The epochs are one kernel launch whose
GPU time the library takes between two events ("timer:umap_transform_epochs"): `epochs_ms`; epochs_ms / firings is the time per firing set
beside the layout's (profiles/umap_bench.json: epoch_ms / firings_per_epoch).  What bounds the kernel: the same call with the lists folded
onto the reference's first 1024 cells (idx % 1024 and a hash over 1024 cells: every gather hits a 8 KB array in cache, the arithmetic, the
firing pattern and the butterfly are unchanged) gives `cached_epochs_ms`; the share of the kernel's time that vanishes with the gathers'
misses is `gather_share`.  A call lasts a few milliseconds, most of it copies from pageable memory: hence
the many repeats.  Whether every call gave the same bits and how far the cells moved from their start are recorded."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_data import synth  # noqa: E402
from harmony_amd import knn, umap  # noqa: E402
from harmony_amd._call import _Handle  # noqa: E402
from harmony_amd.umap_transform import _params, _transform_call, _weights_call  # noqa: E402


def get(h, name):
    out = (C.c_double * 1)()
    h.lib.hmx_get(h.h, name.encode(), out, 1)
    return float(out[0])


def median_spread(ts):
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med if med > 0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--runs", default="100000:30,10000:100", help="query cells : epochs, comma separated")
    ap.add_argument("--layout-epochs", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umap_transform_bench.json"))
    a = ap.parse_args()
    runs = [tuple(int(x) for x in r.split(":")) for r in a.runs.split(",")]
    Nr, d, k = a.reference, a.d, a.k
    most = max(nq for nq, _ in runs)
    Z = np.ascontiguousarray(synth(Nr + most, d=d, levels=(10,), seed=11)[0], dtype=np.float32)
    R = Z[:Nr]
    Yref = umap(R, n_neighbors=k, n_epochs=a.layout_epochs)
    res = {"what": "hmx_umap_query_weights + hmx_umap_transform", "reference": Nr, "d": d, "k": k, "layout_epochs": a.layout_epochs,
           "repeats": a.repeats, "warmup": a.warmup, "runs": []}
    for Nq, epochs in runs:
        Q = Z[Nr:Nr + Nq]
        with _Handle() as h:
            idx = np.empty((Nq, k), dtype=np.int32)
            dist = np.empty((Nq, k), dtype=np.float32)
            h.check(h.lib.hmx_knn(h.h, C.c_void_p(R.ctypes.data), 1, 0, Nr, C.c_void_p(Q.ctypes.data), 1, 0, Nq, d, k, C.c_void_p(idx.ctypes.data),
                                  C.c_void_p(dist.ctypes.data), 0), "knn")
            knn_ms = get(h, "timer:knn")
        assert np.array_equal(idx, knn(R, k, query=Q)[0])
        p = _params(Nq, 2, epochs, 0.5, 1.0, None, None, 1.0, 1.0, 5, 0, None)
        wt, tt, ft, ct, kt, first, same, fired = [], [], [], [], [], None, True, 0
        with _Handle() as h:
            for i in range(a.warmup + a.repeats):
                w = _weights_call(h.lib, h.h, h.check, idx, dist, Nr, False)
                wms = get(h, "timer:umap_query_weights")
                Y, Y0 = _transform_call(h.lib, h.h, h.check, idx, w, Yref, None, p, True)
                ms, fired, kms = get(h, "timer:umap_transform"), int(get(h, "umap_transform:fired")), get(h, "timer:umap_transform_epochs")
                p.begin = p.end = 0                          # the front alone: the uploads and the start
                _transform_call(h.lib, h.h, h.check, idx, w, Yref, None, p, False)
                fr = get(h, "timer:umap_transform")
                p.begin, p.end = 0, epochs
                # the same arithmetic with every gather in cache: the lists and the samples folded onto 1024 reference cells
                folded, few = np.ascontiguousarray(idx % 1024), np.ascontiguousarray(Yref[:1024])
                _transform_call(h.lib, h.h, h.check, folded, w, few, Y0, p, False)
                cms = get(h, "timer:umap_transform_epochs")
                print("Nq %d call %d: weights %.2f ms, transform %.2f ms (front %.2f ms; the epochs' kernel %.3f ms, with a cached reference %.3f ms), %d firings"
                      % (Nq, i, wms, ms, fr, kms, cms, fired), file=sys.stderr, flush=True)
                if i >= a.warmup:
                    wt.append(wms); tt.append(ms); ft.append(fr); ct.append(cms); kt.append(kms)
                if first is None:
                    first, start = Y, Y0
                else:
                    same = same and np.array_equal(Y.view(np.uint32), first.view(np.uint32))
        (wmed, wsp), (tmed, tsp), (fmed, _), (cmed, _) = median_spread(wt), median_spread(tt), median_spread(ft), median_spread(ct)
        epochs_ms, ksp = median_spread(kt)
        res["runs"].append({"query": Nq, "epochs": epochs, "a": p.a, "b": p.b, "negative_sample_rate": p.negative, "knn_ms": knn_ms,
                            "weights_ms": wmed, "weights_ms_all": wt, "weights_spread": wsp, "transform_ms": tmed, "transform_ms_all": tt,
                            "transform_spread": tsp, "front_ms": fmed, "epochs_ms": epochs_ms, "epochs_spread": ksp, "cached_epochs_ms": cmed, "gather_share": 1.0 - cmed / epochs_ms, "fired": fired,
                            "ns_per_firing": epochs_ms * 1e6 / fired, "firings_per_cell_epoch": fired / (Nq * epochs),
                            "gather_bytes": fired * (p.negative) * 4.0 * 2, "gather_TBps": fired * p.negative * 8.0 / epochs_ms / 1e9,
                            "upload_bytes": 8.0 * Nq * k + 8.0 * Nr, "same_bits_every_call": bool(same), "finite": bool(np.all(np.isfinite(first))),
                            "mean_move": float(np.abs(first - start).mean())})
    try:
        lay = json.loads(open(os.path.join(ROOT, "profiles", "umap_bench.json")).read().strip().splitlines()[-1])
        res["layout_ns_per_firing"] = lay["epoch_ms"] * 1e6 / lay["firings_per_epoch"]
    except Exception:
        res["layout_ns_per_firing"] = None
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
