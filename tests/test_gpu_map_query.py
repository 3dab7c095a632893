"""Query mapping on the MI355X: the reference summary ("ref_Nr" / "ref_C") against fp64 sums over the same handle's R and Z_corr (one handle
and two virtual shards), hmx_map_query against the fp64 restatement of the method (tests/map_query_ref.py) on real and synthetic inputs, the
shape envelope, the input forms, reproducibility and the state rules of a query handle."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import map_query_ref as mq  # noqa: E402
from harmony_amd import Harmony, HarmonyError, HarmonyReference, harmony_options, map_query, prepare_setup_args  # noqa: E402
from harmony_amd.utils import harmonize  # noqa: E402
from helpers import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def relfro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def fit(Z, meta, var, K, seed=1, max_iter=10):
    skw, _ = prepare_setup_args(Z, meta, var, nclust=K)
    h = Harmony(seed=seed)
    h.setup(**skw)
    h.init_cluster_cpp()
    harmonize(h, max_iter, verbose=False)
    return h


def check_against_spec(obj, Zq, codes, n_levels, ref, lambda_, alpha=0.2, cutoff=1e-5):
    Zg, Rg = obj.getZcorr(), obj.getR()
    Zc, Rc = mq.map_query(Zq, codes, n_levels, ref.Nr, ref.C, ref.sigma, lambda_=lambda_, alpha=alpha, cutoff=cutoff)
    assert relfro(Zg, Zc) <= 1e-5, relfro(Zg, Zc)
    assert np.abs(Rg - Rc).max() <= 1e-4
    srt = np.sort(Rc, axis=0)
    clear = (srt[-1] - srt[-2]) >= 1e-3 if Rc.shape[0] > 1 else np.ones(Rc.shape[1], bool)
    assert np.array_equal(Rg.argmax(axis=0)[clear], Rc.argmax(axis=0)[clear])


@pytest.fixture(scope="module")
def cell_lines_fit():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines.npz"))
    ds = fx["dataset_levels"][fx["dataset"]]
    ct = fx["cell_type_levels"][fx["cell_type"]]
    ref = ds != "jurkat"
    h = fit(fx["pcs"][ref], {"dataset": ds[ref]}, "dataset", 20, seed=1)
    return h, ct[ref], fx["pcs"][ds == "jurkat"]


def test_summary_is_the_sum_over_the_handles_R_and_Zcorr(cell_lines_fit):
    h = cell_lines_fit[0]
    s = h.reference_summary()
    Nr, C = mq.reference_summary(h.getR(), h.getZcorr())
    assert relfro(s.Nr, Nr) <= 1e-6 and relfro(s.C, C) <= 1e-6
    assert np.array_equal(s.sigma, h.sigma)
    s2 = h.reference_summary()
    assert np.array_equal(s.Nr, s2.Nr) and np.array_equal(s.C, s2.C)      # fixed-order fold: bit-reproducible


def test_summary_on_two_virtual_shards():
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    Z, meta, _ = synth(30000, d=50, levels=(10,), seed=21)
    K, seed, G, N = 100, 4, 2, Z.shape[0]
    one = fit(Z, meta, "cov0", K, seed=seed, max_iter=3)
    ref1 = one.reference_summary()
    bounds = [(0, N // 2), (N // 2, N)]
    N_b = np.bincount(meta["cov0"]).astype(float)
    barrier = threading.Barrier(G)
    slots, out, errors = [None] * G, [None] * G, []

    def hook_for(rank):
        def hook(user, buf, count, dtype, stream):
            assert hip.hipDeviceSynchronize() == 0
            host = np.empty(count, dtype=np.float64 if dtype == 1 else np.int64)
            assert hip.hipMemcpy(host.ctypes.data, buf, host.nbytes, 2) == 0
            slots[rank] = host
            barrier.wait()
            st = np.stack(slots)
            red = st.min(axis=0) if dtype == 2 else st.sum(axis=0)
            barrier.wait()
            assert hip.hipMemcpy(buf, red.ctypes.data, red.nbytes, 1) == 0
            barrier.wait()
            return 0
        return hook

    def work(rank):
        try:
            lo, hi = bounds[rank]
            skw, _ = prepare_setup_args(Z[lo:hi], {k: v[lo:hi] for k, v in meta.items()}, "cov0", nclust=K, N_b=N_b,
                                        levels={"cov0": np.arange(len(N_b))})
            g = Harmony(seed=seed)
            g.set_shard(rank, G, lo, N, hook_for(rank))
            g.setup(**skw)
            g.init_cluster_cpp()
            harmonize(g, 3, verbose=False)
            out[rank] = (g.reference_summary(), g.getR(), g.getZcorr())
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(G)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    a, b = out[0][0], out[1][0]
    assert np.array_equal(a.Nr, b.Nr) and np.array_equal(a.C, b.C)
    Nr, C = mq.reference_summary(np.concatenate([o[1] for o in out], axis=1), np.concatenate([o[2] for o in out], axis=1))
    assert relfro(a.Nr, Nr) <= 1e-6 and relfro(a.C, C) <= 1e-6
    assert relfro(a.Nr, ref1.Nr) <= 1e-6 and relfro(a.C, ref1.C) <= 1e-6


@pytest.mark.parametrize("lam", [None, 1.0])
def test_cell_lines_query_matches_the_spec_and_mixes(cell_lines_fit, lam):
    h, ct_ref, Zq = cell_lines_fit
    ref = h.reference_summary()
    obj = map_query(Zq, None, ref, lambda_=lam, return_object=True)
    check_against_spec(obj, Zq.T, [np.zeros(Zq.shape[0], int)], [1], ref, None if lam is None else [lam])
    Z = h.getZcorr()
    Zr = Z[:, ct_ref == "jurkat"]
    cen = Zr.mean(axis=1, keepdims=True)
    ratio = lambda M: np.linalg.norm(M - cen, axis=0).mean() / np.linalg.norm(Zr - cen, axis=0).mean()  # noqa: E731
    assert ratio(Zq.T) >= 1.6
    assert ratio(obj.getZcorr()) <= (1.5 if lam is None else 1.35)
    out = map_query(Zq, None, ref, lambda_=lam)                # cells x PCs out
    assert np.array_equal(out, obj.getZcorr().T)


@pytest.mark.parametrize("lam", [None, 1.0])
def test_pbmc_stim_mapped_onto_ctrl(lam):
    fx = np.load(os.path.join(ROOT, "tests", "golden", "pbmc_stim_pcs.npz"))
    stim = fx["stim_levels"][fx["stim"]]
    pcs = fx["pcs"].astype(np.float64)
    ctrl = stim == "ctrl"
    h = fit(pcs[ctrl], {"half": np.arange(int(ctrl.sum())) % 2}, "half", 30, seed=2, max_iter=5)
    ref = h.reference_summary()
    obj = map_query(pcs[~ctrl], None, ref, lambda_=lam, return_object=True)
    check_against_spec(obj, pcs[~ctrl].T, [np.zeros(int((~ctrl).sum()), int)], [1], ref, None if lam is None else [lam])


@pytest.fixture(scope="module")
def synth_reference():
    Z, meta, _ = synth(30000, d=50, levels=(10,), seed=31)
    h = fit(Z, meta, "cov0", 100, seed=3, max_iter=3)
    return h.reference_summary()


@pytest.mark.parametrize("lam", [None, "per_covariate"])
def test_synthetic_two_covariate_query(synth_reference, lam):
    ref = synth_reference
    Zq, _, _ = synth(200000, d=50, levels=(10,), seed=31, shard=5)
    rng = np.random.default_rng(7)
    c0 = rng.integers(0, 7, Zq.shape[0])
    c0[np.argsort(Zq[:, 0])[-64:]] = 7                # a small level in one corner: below the cutoff in the clusters far from it
    c1 = rng.integers(0, 3, Zq.shape[0])
    meta = {"q0": c0, "q1": c1}
    lam_arg = None if lam is None else [1.0, 2.0]
    obj = map_query(Zq, meta, ref, vars_use=["q0", "q1"], lambda_=lam_arg, return_object=True)
    lam_ref = None if lam is None else np.concatenate([np.full(8, 1.0), np.full(3, 2.0)])
    check_against_spec(obj, Zq.T, [c0, c1], [8, 3], ref, lam_ref)


@pytest.mark.parametrize("K", [1, 17, 100, 200, 256])
@pytest.mark.parametrize("d", [20, 50, 128])
def test_shape_sweep(K, d):
    rng = np.random.default_rng(K * 1000 + d)
    ref = HarmonyReference(rng.random(K) * 100 + 1, rng.standard_normal((K, d)), np.full(K, 0.1) * (1 + rng.random(K)))
    for Nq in (1, 5, 1000):
        Zq = rng.standard_normal((d, Nq))
        lev = rng.integers(0, 2, Nq)
        obj = map_query(Zq, {"b": lev}, ref, vars_use="b", lambda_=1.0, return_object=True)
        nl = len(np.unique(lev))
        codes = np.unique(lev, return_inverse=True)[1]
        check_against_spec(obj, Zq, [codes], [nl], ref, [1.0] * nl)


def test_input_forms_agree_and_mapping_is_bit_reproducible(synth_reference):
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    ref = synth_reference
    Zq, _, _ = synth(20000, d=50, levels=(10,), seed=31, shard=6)
    lev = np.arange(Zq.shape[0]) % 3
    B_vec = np.array([3], dtype=np.int32)
    from harmony_amd.ui import build_phi
    phi = build_phi([lev.astype(np.int32)], [3])
    lam = np.array([-1.0])
    outs = []
    for form in ("f64", "f64", "f32", "dev32", "dev64"):
        h = Harmony()
        Zt = np.asfortranarray(Zq.T)
        if form == "f64":
            arg = Zt
        elif form == "f32":
            arg = Zt.astype(np.float32)
        else:
            host = np.ascontiguousarray(Zq, dtype=np.float32 if form == "dev32" else np.float64)   # cells x PCs row-major == d x N column-major
            dptr = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(dptr), host.nbytes) == 0
            assert hip.hipMemcpy(dptr, host.ctypes.data, host.nbytes, 1) == 0
            arg = (50, Zq.shape[0], host.dtype, dptr.value)
        h.map_query(arg, phi, B_vec, lam, 0.2, 1e-5, ref)
        if form.startswith("dev"):
            hip.hipFree(dptr)
        outs.append((h.getZcorr(), h.getR()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    for z, _r in outs[2:]:
        assert relfro(z, outs[0][0]) <= 1e-6
    np.testing.assert_array_equal(outs[4][0], outs[0][0])          # fp64 from the device = fp64 from the host
    g = Harmony()
    g.map_query(np.asfortranarray(Zq.T), phi, B_vec, lam, 0.2, 1e-5, ref)
    assert g.timer("map_query") > 0
    z32 = g.get_matrix("Z_corr", dtype=np.float32)
    assert relfro(z32.astype(np.float64), outs[0][0]) <= 1e-7
    assert np.array_equal(g.getZorig(), np.asfortranarray(Zq.T).astype(np.float32).astype(np.float64))


def test_query_handle_state_rules(synth_reference):
    ref = synth_reference
    rng = np.random.default_rng(0)
    Zq = rng.standard_normal((50, 10))
    obj = map_query(Zq, None, ref, return_object=True)
    assert obj.N == 10 and obj.d == 50 and obj.K == 100 and obj.B == 1
    for call in (obj.init_cluster_cpp, obj.cluster_cpp, obj.moe_correct_ridge_cpp, obj.compute_objective, obj.restart,
                 obj.kmeans_centers, obj.reference_summary, lambda: obj.check_convergence(1)):
        with pytest.raises(HarmonyError):
            call()
    with pytest.raises(HarmonyError):                      # a second mapping on the same handle
        from harmony_amd.mapping import prepare_query_args
        kw, _ = prepare_query_args(Zq, None, ref)
        obj.map_query(**kw)
    Z, meta, _ = synth(2000, d=50, levels=(2,), seed=1)
    skw, _ = prepare_setup_args(Z, meta, "cov0", nclust=10)
    with pytest.raises(HarmonyError):                      # and no fit on it either
        obj.setup(**skw)
    h = Harmony()                                          # a fitted handle cannot map
    h.setup(**skw)
    kw, _ = prepare_query_args(Zq, None, ref)
    with pytest.raises(HarmonyError):
        h.map_query(**kw)
