"""Query mapping on the CPU: the fp64 restatement of the method (tests/map_query_ref.py) on the oracle's fit, the Python argument
preparation, the saved reference format, and the checks hmx_map_query makes before it touches a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import map_query_ref as mq  # noqa: E402
from harmony_amd import HarmonyReference, harmony_options, _lib  # noqa: E402
from harmony_amd.mapping import prepare_query_args  # noqa: E402

HMX_ERR_ARG, HMX_ERR_PHI, HMX_ERR_STATE, HMX_ERR_LIMIT = 1, 3, 6, 7


def _cell_lines():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cell_lines.npz"))
    ds = fx["dataset_levels"][fx["dataset"]]
    ct = fx["cell_type_levels"][fx["cell_type"]]
    return fx["pcs"], ds, ct


def jurkat_ratio(Zref, ct_ref, Zx):
    """mean distance of the columns of Zx to the reference's jurkat centroid / the reference jurkat cells' own mean distance to it"""
    Zr = Zref[:, ct_ref == "jurkat"]
    cen = Zr.mean(axis=1, keepdims=True)
    return np.linalg.norm(Zx - cen, axis=0).mean() / np.linalg.norm(Zr - cen, axis=0).mean()


@pytest.fixture(scope="module")
def oracle_fit():
    from helpers import run_backend
    from oracle.oracle import OracleHarmony
    pcs, ds, ct = _cell_lines()
    ref = ds != "jurkat"
    c = OracleHarmony(accurate=True, seed=1)
    run_backend(c, pcs[ref], {"dataset": ds[ref]}, "dataset", nclust=20, max_iter=10)
    return c.getR(), c.getZcorr(), ct[ref], pcs[ds == "jurkat"].T


def test_spec_maps_jurkat_onto_the_reference_jurkat_cells(oracle_fit):
    R, Z, ct_ref, Zq = oracle_fit
    Nr, Cr = mq.reference_summary(R, Z)
    sigma = np.full(R.shape[0], 0.1)
    one = [np.zeros(Zq.shape[1], dtype=int)]
    before = jurkat_ratio(Z, ct_ref, Zq)
    fixed, _ = mq.map_query(Zq, one, [1], Nr, Cr, sigma, lambda_=[1.0])
    auto, Rq = mq.map_query(Zq, one, [1], Nr, Cr, sigma, lambda_=None)
    assert before >= 1.6
    assert jurkat_ratio(Z, ct_ref, fixed) <= 1.35
    assert jurkat_ratio(Z, ct_ref, auto) <= 1.5
    assert np.allclose(Rq.sum(axis=0), 1.0)


def test_spec_closes_the_gap_between_two_shifted_query_levels(oracle_fit):
    R, Z, _, Zq = oracle_fit
    Nr, Cr = mq.reference_summary(R, Z)
    sigma = np.full(R.shape[0], 0.1)
    rng = np.random.default_rng(3)
    lev = (rng.random(Zq.shape[1]) < 0.5).astype(int)
    shift = rng.standard_normal(Zq.shape[0])
    shift *= 0.04 / np.linalg.norm(shift)
    Zs = Zq + np.outer(shift, lev)
    gap = lambda M: np.linalg.norm(M[:, lev == 1].mean(axis=1) - M[:, lev == 0].mean(axis=1))  # noqa: E731
    out, _ = mq.map_query(Zs, [lev], [2], Nr, Cr, sigma, lambda_=[1.0, 1.0])
    assert gap(out) * 5 <= gap(Zs)


def _ref(K=4, d=3):
    rng = np.random.default_rng(0)
    return HarmonyReference(rng.random(K) * 10, rng.standard_normal((K, d)), np.full(K, 0.1))


def test_query_arguments_orientation_vars_and_lambda():
    ref = _ref(K=4, d=3)
    rng = np.random.default_rng(1)
    Z = rng.standard_normal((10, 3))              # cells x PCs
    meta = {"batch": np.array(list("aabbccaabb")), "other": np.arange(10) % 2}
    kw, dm = prepare_query_args(Z, meta, ref)
    assert dm.shape == (3, 10) and kw["Zq"].shape == (3, 10)
    assert list(kw["B_vec"]) == [1] and list(kw["lambda_vec"]) == [-1.0]                     # vars_use=None: one level for all cells
    assert np.array_equal(kw["Phi"][0], np.zeros(10, dtype=np.int32))
    kw2, dm2 = prepare_query_args(Z.T, meta, ref, vars_use="batch", lambda_=2.0)            # PCs x cells in
    assert dm2.shape == (3, 10) and list(kw2["B_vec"]) == [3]
    assert list(kw2["lambda_vec"]) == [0.0, 2.0, 2.0, 2.0]
    kw3, _ = prepare_query_args(Z, meta, ref, vars_use=["batch", "other"], lambda_=[1.0, 3.0],
                                options=harmony_options(alpha=0.5, batch_prop_cutoff=0.01))
    assert list(kw3["B_vec"]) == [3, 2] and list(kw3["lambda_vec"]) == [0.0, 1.0, 1.0, 1.0, 3.0, 3.0]
    assert kw3["alpha"] == 0.5 and kw3["batch_proportion_cutoff"] == 0.01
    kw4, _ = prepare_query_args(Z, None, ref)                                                 # no metadata at all
    assert kw4["Zq"].shape == (3, 10)
    with pytest.raises(ValueError):
        prepare_query_args(Z, meta, ref, vars_use="nope")
    with pytest.raises(ValueError):
        prepare_query_args(Z, meta, ref, vars_use="batch", lambda_=[1.0, 2.0])
    with pytest.raises(ValueError):
        prepare_query_args(rng.standard_normal((10, 4)), meta, ref)                           # PCs do not match the reference


def test_reference_save_load_round_trip(tmp_path):
    ref = _ref(K=5, d=7)
    p = str(tmp_path / "ref.npz")
    ref.save(p)
    back = HarmonyReference.load(p)
    assert np.array_equal(back.Nr, ref.Nr) and np.array_equal(back.C, ref.C) and np.array_equal(back.sigma, ref.sigma)
    np.savez(str(tmp_path / "other.npz"), Nr=ref.Nr)
    with pytest.raises(ValueError):
        HarmonyReference.load(str(tmp_path / "other.npz"))


def _call(lib, h, Zq, d, Nq, phi_i, phi_p, B, B_vec, lam, Nr, Cr, sig, K, C_=1):
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    return lib.hmx_map_query(h, Zq.ctypes.data_as(C.c_void_p), 0, 0, Nq, d, phi_i.ctypes.data_as(ip), phi_p.ctypes.data_as(ip), B,
                             B_vec.ctypes.data_as(ip), C_, lam.ctypes.data_as(dp), lam.size, 0.2, 1e-5, Nr.ctypes.data_as(dp),
                             Cr.ctypes.data_as(dp), sig.ctypes.data_as(dp), K)


def test_abi_summary_fields_and_argument_checks_before_the_device():
    lib = _lib.load()
    assert hasattr(lib, "hmx_map_query")
    h = C.c_void_p(lib.hmx_create())
    try:
        out = np.zeros(8)
        for f in (b"ref_Nr", b"ref_C"):
            assert lib.hmx_get(h, f, None, 0) == -1
            assert lib.hmx_get(h, f, out.ctypes.data_as(C.POINTER(C.c_double)), 8) == -1
        d, Nq, K = 3, 4, 2
        Zq = np.zeros((d, Nq))
        phi_i = np.zeros(Nq, dtype=np.int32)
        phi_p = np.arange(Nq + 1, dtype=np.int32)
        B_vec = np.array([1], dtype=np.int32)
        lam = np.array([-1.0])
        Nr, Cr, sig = np.ones(K), np.ones((K, d)), np.full(K, 0.1)
        assert _call(lib, h, Zq, d, 0, phi_i, phi_p, 1, B_vec, lam, Nr, Cr, sig, K) == HMX_ERR_ARG           # no cells
        assert _call(lib, h, Zq, d, Nq, phi_i, phi_p, 2, B_vec, lam, Nr, Cr, sig, K) == HMX_ERR_ARG          # sum(B_vec) != B
        assert _call(lib, h, Zq, d, Nq, phi_i, phi_p, 1, B_vec, np.array([0.0, 1.0, 1.0]), Nr, Cr, sig, K) == HMX_ERR_ARG   # lambda length
        assert _call(lib, h, Zq, d, Nq, phi_i, phi_p, 1, B_vec, lam, Nr, Cr, np.zeros(K), K) == HMX_ERR_ARG  # sigma
        assert _call(lib, h, np.zeros((129, Nq)), 129, Nq, phi_i, phi_p, 1, B_vec, lam, Nr, np.ones((K, 129)), sig, K) == HMX_ERR_LIMIT
        assert _call(lib, h, Zq, d, Nq, phi_i, phi_p, 1, B_vec, lam, np.ones(257), np.ones((257, d)), np.full(257, 0.1), 257) == HMX_ERR_LIMIT
        assert _call(lib, h, Zq, d, Nq, phi_i, np.array([0, 1, 2, 2, 4], dtype=np.int32), 1, B_vec, lam, Nr, Cr, sig, K) == HMX_ERR_PHI
        assert _call(lib, h, Zq, d, Nq, np.array([0, 1, 0, 0], dtype=np.int32), phi_p, 1, B_vec, lam, Nr, Cr, sig, K) == HMX_ERR_PHI
        assert "Phi" in lib.hmx_last_error(h).decode()
    finally:
        lib.hmx_destroy(h)
    h = C.c_void_p(lib.hmx_create())                # a query handle is single-GPU
    try:
        hook = _lib.ALLREDUCE_FN(lambda *a: 0)
        assert lib.hmx_set_shard(h, 0, 2, 0, 8, C.cast(hook, C.c_void_p), None) == 0
        assert _call(lib, h, np.zeros((3, 4)), 3, 4, np.zeros(4, dtype=np.int32), np.arange(5, dtype=np.int32), 1, np.array([1], dtype=np.int32),
                     np.array([-1.0]), np.ones(2), np.ones((2, 3)), np.full(2, 0.1), 2) == HMX_ERR_ARG
    finally:
        lib.hmx_destroy(h)
