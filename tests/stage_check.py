"""Drive a handle (harmony_amd.Harmony or the CPU oracle) stage by stage and measure each stage against the fp64 spec (tests/stage_ref.py):
before a stage the handle's own state is read through its getters, the spec applies the stage to it, and the result is compared with the
handle's state after the stage (run_stages); run_ladder does the same for the rounds of one clustering call.  Not a test module."""
import numpy as np
import scipy.sparse as sp

import stage_ref as ref


def phi_matrix(Phi):
    """(i, p, x, B) CSC of the setup arguments -> B x N scipy matrix"""
    phi_i, phi_p, _x, B = Phi
    N = len(phi_p) - 1
    return sp.csc_matrix((np.ones(len(phi_i)), np.asarray(phi_i), np.asarray(phi_p)), shape=(int(B), N))


def relfro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _count(h, name):
    v = getattr(h, name, None)
    return int(v) if v is not None else int(h._scalar(name))


def _objective_terms(h):
    return np.array([h.objective_kmeans_dist[-1], h.objective_kmeans_entropy[-1], h.objective_kmeans_cross[-1]])


def _obj_err(h, spec):
    got = _objective_terms(h)
    spec = np.asarray(spec)
    return float(np.max(np.abs(got - spec)) / np.sum(np.abs(spec)))


def _argmax_clear(Rg, Rs, margin=1e-5):
    """number of cells whose argmax differs where the spec's top-two margin is at least `margin`"""
    srt = np.sort(Rs, axis=0)
    clear = (srt[-1] - srt[-2]) >= margin
    return int(np.count_nonzero((Rg.argmax(axis=0) != Rs.argmax(axis=0)) & clear))


def _table_errs(h, R, Phi, Pr_b, tag, out):
    """O and E of the handle against fp64 sums over the handle's own R"""
    O = np.asarray((Phi @ R.T).T)
    E = R.sum(axis=1)[:, None] * Pr_b[None, :]
    out[tag + "_O"] = relfro(h.O, O)
    out[tag + "_E"] = relfro(h.E, E)


def run_stages(h, skw, Y0, order_of_round, stale_objective=True):
    """init -> one clustering round -> ridge correction -> (stand-alone objective) -> the next call's cold start and round.
    order_of_round(r): the update order of round r (pushing it into the handle first if the case injects its orders).
    Returns (errors, info): the measured errors by name, and what the stages did (counts, block partition, keep margin)."""
    Phi = phi_matrix(skw["Phi"])
    sigma = np.asarray(skw["sigma"], dtype=np.float64)
    theta = np.asarray(skw["theta"], dtype=np.float64)
    B_vec = np.asarray(skw["B_vec"])
    lam = np.asarray(skw["lambda_vec"], dtype=np.float64)
    lam = None if lam[0] < 0 else lam
    N = Phi.shape[1]
    nb, cpb, _ = ref.block_partition(N, skw["block_size"])
    err, info = {}, {"n_blocks": nb, "cells_per_block": cpb}
    Pr_b = np.asarray(h.Pr_b)

    # 1. init_cluster_cpp (src/harmony.cpp:135-155)
    Zc0 = h.getZcorr()
    h.init_cluster_cpp(Y0)
    Y = h.Y
    R0 = h.R
    Rs, dist0, _, _ = ref.head(Y, Zc0, sigma, Phi, Pr_b)
    err["init_R"] = float(np.abs(R0 - Rs).max())
    err["init_argmax"] = _argmax_clear(R0, Rs)
    _table_errs(h, R0, Phi, Pr_b, "init", err)
    err["init_obj"] = _obj_err(h, ref.objective(R0, dist0, h.O, h.E, Phi, sigma, theta, N))
    del Rs

    # 2. one round of the first cluster_cpp (:230-262 with max_iter_kmeans = 1)
    h.max_iter_kmeans = 1
    order = order_of_round(0)
    assert h.cluster_cpp() == 0
    R1 = h.R
    Rs = ref.update_round(R0, R1, Y, Zc0, Phi, Pr_b, sigma, theta, order, nb, cpb)
    err["round_R"] = float(np.abs(R1 - Rs).max())
    err["round_argmax"] = _argmax_clear(R1, Rs)
    del R0, Rs
    _table_errs(h, R1, Phi, Pr_b, "round", err)
    O1, E1 = h.O, h.E
    obj1 = ref.objective(R1, dist0, O1, E1, Phi, sigma, theta, N)
    err["round_obj"] = _obj_err(h, obj1)

    # 3. moe_correct_ridge_cpp (:345-633)
    info["keep_margin"] = ref.cutoff_margin(O1, np.asarray(Phi.sum(axis=1)).ravel(), skw["batch_proportion_cutoff"])
    Y_prev = h.Y
    Zo = h.getZorig()
    h.moe_correct_ridge_cpp()
    s = ref.moe_correct_ridge(R1, Zo, O1, E1, Phi, B_vec, lam, skw["alpha"], skw["batch_proportion_cutoff"], Y_prev)
    Zc = h.getZcorr()
    err["Z_rel"] = relfro(Zc, s["Z_corr"])
    err["Z_maxabs"] = float(np.abs(Zc - s["Z_corr"]).max() / np.abs(Zo).max())
    Yh = h.Y
    cond = np.where(np.isnan(s["cond"]), 1.0, np.maximum(s["cond"], 1.0))
    err["Y"] = float(np.max(np.abs(Yh - s["Y"]).max(axis=0) / cond))
    info["subset"], info["skipped"] = int(s["subset"].sum()), int(s["skipped"].sum())
    info["subset_h"], info["skipped_h"] = _count(h, "subset_clusters"), _count(h, "skipped_clusters")
    info["max_cond"] = float(np.nanmax(s["cond"])) if not s["skipped"].all() else 1.0
    info["max_kept"] = max(len(k) for k in s["kept"])
    if s["W"] is not None:
        last = int(np.where(~s["skipped"])[0][-1])
        W = h.W
        info["W_shape"] = (W.shape, s["W"].shape)
        if W.shape == s["W"].shape:
            err["W"] = float(np.abs(W - s["W"]).max(axis=1).max() / (cond[last] * np.linalg.norm(s["W"])))
        else:
            err["W"] = np.inf
    L = h.getLambda()
    L_spec = np.concatenate([np.zeros((h.K, 1)), skw["alpha"] * E1], axis=1) if lam is None else np.tile(lam, (h.K, 1))
    err["Lambda"] = float(np.max(np.abs(L - L_spec) / np.maximum(np.abs(L_spec), 1e-30)))

    # 4. a stand-alone compute_objective after the correction: the distances of the last head (the reference's stored dist_mat, :160)
    if stale_objective:
        h.compute_objective()
        err["stale_obj"] = _obj_err(h, obj1)
    del dist0

    # 5. the next cluster_cpp: its cold start (:214-228) and one round
    order = order_of_round(1)
    assert h.cluster_cpp() == 0
    R2 = h.R
    Rh, dist2, _, _ = ref.head(Yh, Zc, sigma, Phi, Pr_b, cold=True)
    Rs = ref.update_round(Rh, R2, Yh, ref.normalise_cols(Zc), Phi, Pr_b, sigma, theta, order, nb, cpb)
    del Rh
    err["cold_R"] = float(np.abs(R2 - Rs).max())
    err["cold_argmax"] = _argmax_clear(R2, Rs)
    del Rs
    _table_errs(h, R2, Phi, Pr_b, "cold", err)
    err["cold_obj"] = _obj_err(h, ref.objective(R2, dist2, h.O, h.E, Phi, sigma, theta, N))
    return err, info


def run_ladder(make_handle, skw, Y0, order_of_round, rounds=5, probe=None):
    """What a round hands to the next one.  For m = 1..rounds a fresh handle H_m (make_handle(): the same setup and seed every time) runs
    init_cluster_cpp(Y0) and ONE cluster_cpp of m rounds (the caller's options keep the windowed check from ending it: kmeans_rounds[-1] == m
    is asserted); R_0 is the R after init, R_j the R H_j ends on.  Rung m is the spec of round m - 1, teacher-forced from R_{m-1} to H_m's own
    R_m: H_m's first m - 1 rounds are judged through the state they left for its last one -- wrong carried sums, a row read that was never
    stored or a wrong sort set of round m - 1 move R_m off the spec.  (H_m's unstored R_{m-1} is H_{m-1}'s stored one if the library repeats
    itself from run to run: the caller compares rung["first"] between the rungs.)
    order_of_round(h, r): the update order of round r (pushing it into the handle first if the orders are injected; called for every round
    of the call before cluster_cpp).  probe(h): counters of the handle, kept as rung["probe"].
    Returns the rungs: {"m", "R", "argmax", "O", "E", "obj" (the worst of H_m's m round entries against the spec terms on R_1 .. R_m, the
    distances those of the head, the tables those of H_j), "first" (H_m's first round entry: total and the three terms), "probe"}."""
    Phi = phi_matrix(skw["Phi"])
    sigma = np.asarray(skw["sigma"], dtype=np.float64)
    theta = np.asarray(skw["theta"], dtype=np.float64)
    N = Phi.shape[1]
    nb, cpb, _ = ref.block_partition(N, skw["block_size"])
    rungs, obj_spec = [], []
    R_prev = Y = Zc0 = dist0 = Pr_b = None
    for m in range(1, rounds + 1):
        h = make_handle()
        if m == 1:
            Pr_b = np.asarray(h.Pr_b)
            Zc0 = h.getZcorr()
        h.init_cluster_cpp(Y0)
        if m == 1:
            Y = h.Y
            R_prev = h.R
            dist0 = ref.head(Y, Zc0, sigma, Phi, Pr_b)[1]
        h.max_iter_kmeans = m
        orders = [order_of_round(h, r) for r in range(m)]
        assert h.cluster_cpp() == 0
        assert int(h.kmeans_rounds[-1]) == m, (m, h.kmeans_rounds)
        R_m = h.R
        Rs = ref.update_round(R_prev, R_m, Y, Zc0, Phi, Pr_b, sigma, theta, orders[m - 1], nb, cpb)
        rung = {"m": m, "R": float(np.abs(R_m - Rs).max()), "argmax": _argmax_clear(R_m, Rs)}
        del Rs, orders
        _table_errs(h, R_m, Phi, Pr_b, "tab", rung)
        rung["O"], rung["E"] = rung.pop("tab_O"), rung.pop("tab_E")
        obj_spec.append(np.asarray(ref.objective(R_m, dist0, h.O, h.E, Phi, sigma, theta, N)))
        got = np.stack([h.objective_kmeans_dist, h.objective_kmeans_entropy, h.objective_kmeans_cross], axis=1)
        assert got.shape[0] == m + 1, got.shape            # the head's entry and one per round
        rung["obj"] = max(float(np.max(np.abs(got[1 + j] - obj_spec[j])) / np.sum(np.abs(obj_spec[j]))) for j in range(m))
        rung["first"] = [float(h.objective_kmeans[1])] + [float(v) for v in got[1]]
        rung["probe"] = probe(h) if probe else None
        rungs.append(rung)
        R_prev = R_m
        del h
    return rungs
