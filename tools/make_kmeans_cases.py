"""Search the data seeds of the CASES table of tests/test_gpu_kmeans.py on the CPU: for every wanted shape the first seed whose run of the fp64 spec
(tests/kmeans_ref.py) is clear -- every race and every Lloyd assignment at least twice its fp32 rounding bound from the next candidate -- with room to spare
(3 x, so that the handle's cells, an ulp from the oracle's, stay clear as well).  Prints the table as Python source with the launches the coverage ledger
(tests/stage_lattice.py) credits each case with."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kmeans_ref  # noqa: E402
import stage_lattice as L  # noqa: E402
import test_gpu_kmeans as T  # noqa: E402
from harmony_amd import prepare_setup_args  # noqa: E402
from oracle.oracle import OracleHarmony  # noqa: E402

F32 = {"HMX_DOT": "f32"}
# (name, PCs, clusters, levels, environment): 13 cluster-tile counts in both builds, at a full last tile, one valid lane, inside a quad; small d keeps the bounds small
WANT = [("bf_t%02d_K%d_d%d" % ((K + 15) // 16 if (K + 15) // 16 not in (9, 11, 15) else (K + 15) // 16 + 1, K, d), d, K, (2,), {}) for K, d in
        ((16, 16), (17, 8), (40, 20), (64, 32), (65, 16), (92, 24), (112, 50), (113, 17), (150, 32), (192, 20), (200, 50), (209, 16), (256, 28), (129, 12), (225, 100))]
WANT += [("f32_t%02d_K%d_d%d" % ((K + 15) // 16 if (K + 15) // 16 not in (9, 11, 15) else (K + 15) // 16 + 1, K, d), d, K, (2,), {} if 64 < d < 77 else F32) for K, d in
         ((8, 16), (32, 68), (33, 20), (49, 8), (80, 17), (81, 76), (97, 32), (128, 16), (145, 24), (177, 68), (208, 20), (224, 16), (241, 32))]
WANT += [("three_waves_t05_K65_d80", 80, 65, "own", {}), ("three_waves_t06_K96_d64", 64, 96, "own", {}), ("three_waves_t07_K112_d50", 50, 112, "own", {}),
         ("k_lloyd_K256_d64", 64, 256, (2,), {}), ("k_lloyd_K256_d128", 128, 256, (2,), {})]
ROOM = 3.0


def main():
    print("CASES = {")
    for name, d, K, levels, env in WANT:
        N = 1100 if levels == "own" else max(4 * K, 640)
        for dseed in range(1, 400):
            T.CASES[name] = (N, d, K, levels, env, dseed)
            Z, meta, var, kw, _ = T.case_data(name)
            skw, _ = prepare_setup_args(Z, meta, var, **kw)
            c = OracleHarmony(accurate=True, seed=dseed)
            c.setup(**skw)
            s = kmeans_ref.kmeans_centers(c.getZcorr().T, K, dseed)
            if min(s["race_clear"].min(), s["lloyd_clear"].min()) >= ROOM:
                break
        else:
            print("# no clear seed for", name, file=sys.stderr)
            continue
        _N, _K, shape, items = L.shape_of(skw)
        got, _p = L.launches(N, K, shape, items, env, "kmeans")
        by = {kind: v for v, kind in got.items()}
        lloyd = "k_lloyd" if by["lloyd"] == ("k_lloyd",) else (by["lloyd"][1], by["lloyd"][2], by["lloyd"][4])
        print("    %r: (%d, %d, %d, %r, %r, %d, %r, %r)," % (name, N, d, K, levels, env, dseed, (by["seed"][1], by["seed"][2]), lloyd))
        print("#", name, "seed", dseed, "race %.1f lloyd %.2f" % (s["race_clear"].min(), s["lloyd_clear"].min()), by, file=sys.stderr)
    print("}")


if __name__ == "__main__":
    main()
