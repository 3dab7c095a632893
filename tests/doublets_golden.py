"""The results tests/golden/doublets_unchanged_bits.npz records (not a test module): project_query, knn and fit_loadings on one input each of
their own GPU tests.  The file was written by `python tests/doublets_golden.py --write` on an MI355X with the library of the commit BEFORE the
doublet detection (k_project's queue then still lived in hmx_project.hip); tests/test_gpu_doublets.py holds the library to it bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "doublets_unchanged_bits.npz")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def earlier_results():
    """-> {name: array}: floats as their bit patterns"""
    import pca_ref as pc
    import test_gpu_project as tgp
    from bench_data import synth
    from harmony_amd import fit_loadings, knn, project_query
    shape = (257, 900, 300, 68)                                  # test_gpu_project.py: the case of test_clip_that_bites
    c, genes = tgp.case(shape)
    proj = project_query(tgp.csr(c), genes, tgp.loadings(c, clip=10.0))
    Z = synth(2000, d=20, levels=(4,), seed=5)[0]                # test_gpu_metrics.py: real_case(2000, 20) with k = 30
    kidx, kdist = knn(Z, 30)
    X = pc.planted_counts(4, Nq=300)[0]                          # test_gpu_pca.py: planted(4) through test_fit_loadings_on_planted_groups
    L, pcs, ev = fit_loadings(X, np.array(["gene%d" % g for g in range(X.shape[1])]), n_top_genes=200, d=3)
    return dict(project=bits(proj), knn_idx=kidx, knn_dist=bits(kdist), fit_loadings=bits(L.loadings), fit_pcs=bits(pcs), fit_ev=bits(ev))


if __name__ == "__main__":
    sys.path.append(ROOT)                                        # (behind a PYTHONPATH that names the earlier commit's package)
    import harmony_amd                                           # noqa: F401  (first: the test modules put ROOT in front)
    print("library of", os.path.dirname(harmony_amd.__file__))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    out = GOLDEN if "--write" in sys.argv else sys.argv[1]
    np.savez_compressed(out, **earlier_results())
    print("wrote", out)
