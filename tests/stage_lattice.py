"""The coverage ledger of the stage-spec and k-means cases: which kernel instantiations a case's handle launches, computed on the CPU from the
plan probe (tests/cpp/plan_probe.cpp over harmony_amd/csrc/hmx_plan.h) and the round probe (hmx_round.h) for the case's own B, C, Q, tile
counts and block partition -- and which instantiations the plan reaches at all across an envelope of small shapes.  Not a test module.

An instantiation is a tuple:
  ("k_tile", bf, nct, mode, wps, usig)   k_tile<nct, mode, wps, usig> of the split-bf16 (bf = 1) or the fp32 build; mode 0 update, 1 head, 2 Lloyd,
                                         3 seeding race, 4 chain, 5 chain without R stores, 6 wave-pair chain
  ("k_lloyd",)                           Lloyd where the K x d sum table does not fit LDS beside the centroid image
  ("stats" | "apply", mfma, p0, p1)      k_moe_stats_q<p0, p1> / k_moe_stats<p0> and k_moe_apply_mfma<p0> / k_moe_apply<p0, p1>"""
import contextlib
import os

import numpy as np

import stage_ref as ref
from stage_check import phi_matrix
from test_plan_cpu import plan, ridge_launch, tile_launch
from test_round_cpu import cluster, init_cluster, rounds, run

ENVELOPE_D = (1, 3, 16, 17, 32, 48, 50, 63, 64, 65, 68, 76, 80, 96, 100, 116, 128)      # (116: the only rows of seven 16-PC groups, NT4 = 7)
ENVELOPE_N = (4000, 6000)
ENVELOPE_LEVELS = {1: (4,), 2: (3, 2)}          # one and two covariates; every combination of levels is present
# as the plan decides, off the chain, and -- the carry never pays by itself below 100 000 cells -- two rounds with the carry forced on (the first stores no R)
ENVELOPE_ENVS = (({}, "stages"), ({"HMX_CHAIN": "0"}, "stages"), ({"HMX_SOLD_CARRY": "1"}, ("ladder", 2)))


_active = [None]      # the switches in force (the round rows are cached by them)


@contextlib.contextmanager
def switches(env):
    """the HMX_* switches of a case and no others, for the probes (they read the environment like the library)"""
    saved = {k: v for k, v in os.environ.items() if k.startswith("HMX_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    _active.append(tuple(sorted(env.items())))
    try:
        yield
    finally:
        _active.pop()
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def shape_of(skw):
    """the plan's shape of a setup at 256 CUs, and the static work lists of its ridge correction: as hmx_setup derives them"""
    Phi = phi_matrix(skw["Phi"])
    q_of, levels = ref._combinations(Phi, skw["B_vec"])
    counts = np.bincount(q_of)
    d, N = skw["Z"].shape
    nb, cpb, _ = ref.block_partition(N, skw["block_size"])
    shape = dict(d=d, B=Phi.shape[0], C_=len(skw["B_vec"]), Q=levels.shape[0], nb=nb, cells_per_block=cpb, usig=int(np.ptp(skw["sigma"]) == 0),
                 ntitems=int(((counts + 15) // 16).sum()))
    items = dict(nitems=int(((counts + 255) // 256).sum()), naitems=int(((counts + 1023) // 1024).sum()))
    return N, int(skw["K"]), shape, items


def even_shape(N, d, C_, usig):
    """the shape of N cells spread evenly over the envelope's levels (the envelope sweep has no data)"""
    lv = ENVELOPE_LEVELS[C_]
    Q = int(np.prod(lv))
    counts = np.full(Q, N // Q) + (np.arange(Q) < N % Q)
    nb, cpb, _ = ref.block_partition(N, 0.05)
    shape = dict(d=d, B=int(sum(lv)), C_=C_, Q=Q, nb=nb, cells_per_block=cpb, usig=usig, ntitems=int(((counts + 15) // 16).sum()))
    return shape, dict(nitems=int(((counts + 255) // 256).sum()), naitems=int(((counts + 1023) // 1024).sum()))


def _tile(t):
    assert t["valid"] == 1, t
    return ("k_tile", int(t["bf"]), int(t["nct"]), int(t["mode"]), int(t["wps"]), int(t["usig"]))


_rows_cache = {}


def _round_rows(p, N, K, shape, calls):
    """the rounds of `calls` clustering calls behind one init_cluster: [(rounds, max_iter_kmeans)]; the first follows init_cluster directly"""
    key = (_active[-1], shape["B"], K, shape["nb"],
           tuple(p[f] for f in ("nrep", "fused_ok", "chain_ok", "chain_pair", "carry_ok", "shuf_inv", "r_store_always", "NT4", "NCT", "upd_wps")), tuple(calls))
    if key not in _rows_cache:
        _rows_cache[key] = _round_rows_uncached(p, K, shape, calls)
    return _rows_cache[key]


def _round_rows_uncached(p, K, shape, calls):
    cfg = dict(B=shape["B"], K=K, nb=shape["nb"], nrep=p["nrep"], fused_ok=p["fused_ok"], chain_ok=p["chain_ok"], chain_pair=p["chain_pair"], carry_ok=p["carry_ok"],
               shuf_inv=p["shuf_inv"], r_store_always=p["r_store_always"], seed=1, NT4=p["NT4"], NCT=p["NCT"], upd_wps=p["upd_wps"])
    out = []
    for max_iter in sorted({mi for _m, mi in calls}):       # (max_iter_kmeans is one value per script: one script per value)
        ops = init_cluster()
        for i, (m, mi) in enumerate(calls):
            if mi == max_iter:
                ops = ops + cluster(m, i == 0, max_iter=mi)
        out += rounds(run(ops, max_iter_kmeans=max_iter, **cfg))
    return out


def launches(N, K, shape, items, env, script):
    """{instantiation: launch kind} of a handle on this shape under `env` (HMX_* switches).  script: "kmeans" (kmeans_centers alone), "stages" (run_stages: kmeans_centers,
    init_cluster, a call of one round, the correction, a second call of one round) or ("ladder", rounds) (run_ladder: for m = 1 .. rounds, one call of m rounds).
    Also returns the plan.  {} and the plan's limit where the plan refuses the shape."""
    with switches(env):
        return _launches(N, K, shape, items, script)


def _launches(N, K, shape, items, script):
    """launches() under the switches already in force"""
    p = plan(N, K, **shape)
    if "limit" in p:
        return {}, p
    got = {}
    seed, lloyd = tile_launch("seed", N, K, **shape), tile_launch("lloyd", N, K, **shape)
    got[_tile(seed)] = "seed"
    got[_tile(lloyd) if lloyd["ran"] else ("k_lloyd",)] = "lloyd"
    if script == "kmeans":
        return got, p
    got[_tile(tile_launch("head", N, K, **shape))] = "head"
    if script == "stages":      # two calls of one round each behind one init_cluster
        rows = _round_rows(p, N, K, shape, [(1, 1), (1, 1)])
    else:                       # a fresh handle per rung: one call of m rounds
        rows = [r for m in range(1, script[1] + 1) for r in _round_rows(p, N, K, shape, [(m, m)])]
    for r in rows:
        kind = "chain" if r["path"] == 0 else "update"
        t = tile_launch(kind, N, K, r_store=int(r["r_store"]), **shape)
        assert t["ran"] == 1, (kind, t)
        got[_tile(t)] = kind
    if script == "stages":
        for kind in ("stats", "apply"):
            t = ridge_launch(kind, N, K, **items, **shape)
            assert t["valid"] == 1, (kind, t)
            got[(kind, int(t["mfma"]), int(t["p0"]), int(t["p1"]))] = kind
    return got, p


def loop_bounds(got, p):
    """the d loop bounds a case exercises, per build of its tile launches: {(bf, "NT4" | "tail" | "NS2", value)}"""
    return {(v[1], f, int(p[f])) for v in got if v[0] == "k_tile" for f in ("NT4", "tail", "NS2")}


def admitted_loop_bounds():
    """the loop bounds the plan admits in each build for d = 1 .. 128, by itself or under HMX_DOT=f32: what the cases must exercise"""
    want = set()
    for env in ({}, {"HMX_DOT": "f32"}):
        for d in range(1, 129):
            shape, items = even_shape(4000, d, 1, 1)
            want |= loop_bounds(*launches(4000, 32, shape, items, env, "stages"))
    return want


def envelope(K_range=range(1, 257)):
    """every instantiation the plan reaches across the envelope, with one shape that reaches it: {instantiation: (K, d, usig, C, N, env)}; and the loop bounds"""
    reach, bounds = {}, set()
    for env, script in ENVELOPE_ENVS:
        with switches(env):
            for N in ENVELOPE_N:
                for d in ENVELOPE_D:
                    for C_ in (1, 2):
                        for usig in (1, 0):
                            shape, items = even_shape(N, d, C_, usig)
                            for K in K_range:
                                got, p = _launches(N, K, shape, items, script)
                                bounds |= loop_bounds(got, p)
                                for v in got:
                                    reach.setdefault(v, (K, d, usig, C_, N, env))
    return reach, bounds
