"""The launch diet's decisions as pure functions, checked without a GPU (tests/cpp/launch_path_probe.cpp drives a RoundLedger the way hmx_init_cluster,
hmx_cluster and hmx_restart drive the handle's): which of the head's four clears plan_head still asks for, when the head leaves no objective partials,
and where plan_ridge_launch puts the device solve's systems.

What the expected values follow from (harmony_amd/csrc/hmx_round.h):
  O              k_fold behind the head overwrites it (fold mode 3): cleared only where every clear is kept
  replica set    the head's own buffer; k_fold re-zeroes what it sums, the launch-per-step rounds ping-pong through it: cleared unless the last user was a head
  objective slots every launch that sums them zeroes what it read: cleared only where every clear is kept
  old table      (clear_first, unchanged) a stale table the head files into
  every clear is kept by the first head after setup / hmx_restart, with a host order, a poll, HMX_R_STORE=1, on sharded and reference-arithmetic handles
  skip_obj       cluster_cpp's head (normalise) with at least one round behind it, where not every clear is kept"""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP_CFG = ("sharded", "B", "K", "nb", "nrep", "fused_ok", "chain_ok", "chain_pair", "carry_ok", "poll", "r_store_always", "obj_arith", "max_iter_kmeans")
HEAD_FIELDS = ("clear_O", "clear_set", "clear_objpart", "clear_first", "skip_obj", "r_store", "files")
HEAD, ROUND, RESTART = range(3)
CHAIN, FOLD_PROLOGUE, STEP_LOOP = range(3)
ALL = dict(clear_O=1, clear_set=1, clear_objpart=1, skip_obj=0)
NONE = dict(clear_O=0, clear_set=0, clear_objpart=0, clear_first=0, skip_obj=1)
_probe = []


def probe():
    if not _probe:
        import tempfile
        so = os.path.join(tempfile.mkdtemp(prefix="launch_path_probe_"), "launch_path_probe.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "launch_path_probe.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.probe_launch_path.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_longlong)]
        lib.probe_launch_path.restype = None
        lib.probe_solve_lds.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_longlong)]
        lib.probe_solve_lds.restype = None
        _probe.append(lib)
    return _probe[0]


def run(ops, **kw):
    """the heads of a script as dicts of HEAD_FIELDS, the rounds as (path, close, clear_sets).  Defaults: the flagship's shape on one GPU (chain, carry)"""
    c = dict(sharded=0, B=10, K=100, nb=20, nrep=4, fused_ok=1, chain_ok=1, chain_pair=0, carry_ok=1, poll=0, r_store_always=0, obj_arith=0, max_iter_kmeans=4)
    assert not set(kw) - set(c), kw
    c.update(kw)
    flat = [int(v) for op in ops for v in (tuple(op) + (0, 0, 0))[:4]]
    out = (C.c_longlong * (8 * len(ops)))()
    probe().probe_launch_path((C.c_longlong * len(LP_CFG))(*[int(c[k]) for k in LP_CFG]), (C.c_longlong * len(flat))(*flat), len(ops), out)
    rows = []
    for i, op in enumerate(ops):
        rows.append(dict(zip(HEAD_FIELDS, out[8 * i:8 * i + 7])) if op[0] == HEAD else tuple(out[8 * i:8 * i + 3]) if op[0] == ROUND else None)
    return rows


def call(m=4, head=True, host_order=0):
    """hmx_cluster with m = max_iter_kmeans rounds (window 3): the head unless it is the first call after init_cluster"""
    return ([(HEAD, 1, host_order)] if head else []) + [(ROUND, int(it == m - 1), int(it == m - 1 or it > 3), 0) for it in range(m)]


def has(row, want):
    return {k: row[k] for k in want} == want


def heads(rows):
    return [r for r in rows if isinstance(r, dict)]


def test_flagship_sequence_init_call_correction_call():
    """init_cluster's head is the first after setup: every clear, partial sums kept (its snapshot reads them).  The first call has no head.  The correction touches
    no table.  The head of every later call: nothing to clear -- no launch --, no partial sums, and its R rows stay in registers as before"""
    rows = run([(HEAD, 0, 0)] + call(head=False) + call() + call())
    h = heads(rows)
    assert has(h[0], ALL) and h[0]["r_store"] == 1
    assert has(h[1], NONE) and has(h[2], NONE) and h[1]["r_store"] == 0 and h[1]["files"] == 1
    assert all(r[0] == CHAIN for r in rows if isinstance(r, tuple))


def test_first_head_after_restart_keeps_every_clear():
    rows = run([(HEAD, 0, 0)] + call(head=False) + call() + [(RESTART,), (HEAD, 0, 0)] + call(head=False) + call())
    h = heads(rows)
    assert has(h[1], NONE)
    assert has(h[2], ALL)              # init_cluster's head behind hmx_restart
    assert has(h[3], NONE)
    # ... and a handle that is restarted and goes straight into a head of cluster_cpp's kind keeps them too
    h = heads(run([(HEAD, 0, 0)] + call(head=False) + [(RESTART,)] + call()))
    assert has(h[1], ALL)


def test_host_order_poll_and_r_store_always_keep_every_clear():
    base = [(HEAD, 0, 0)] + call(head=False)
    assert has(heads(run(base + call(host_order=1)))[1], ALL)
    assert has(heads(run(base + call(), poll=1))[1], ALL)
    assert has(heads(run(base + call(), r_store_always=1))[1], ALL)
    assert has(heads(run(base + call(), sharded=1))[1], ALL)
    assert has(heads(run(base + call(), obj_arith=1))[1], ALL)
    # a host order for ONE head only: the next call's head is on the diet again
    h = heads(run(base + call(host_order=1) + call()))
    assert has(h[1], ALL) and h[2]["clear_O"] == 0 and h[2]["clear_set"] == 0 and h[2]["clear_objpart"] == 0 and h[2]["skip_obj"] == 1


def test_step_loop_rounds_dirty_the_heads_replica_set():
    """launch-per-step rounds (no fold in the prologue, no chain) ping-pong through the head's replica buffer: the next head clears it -- and only it"""
    rows = run([(HEAD, 0, 0)] + call(head=False) + call(), fused_ok=0, chain_ok=0, carry_ok=0)
    assert all(r[0] == STEP_LOOP for r in rows if isinstance(r, tuple))
    h = heads(rows)[1]
    assert (h["clear_O"], h["clear_set"], h["clear_objpart"], h["skip_obj"]) == (0, 1, 0, 1)
    # fold in the prologue: the rounds use the three sets, the head's buffer stays zero
    rows = run([(HEAD, 0, 0)] + call(head=False) + call(), chain_ok=0)
    assert all(r[0] == FOLD_PROLOGUE for r in rows if isinstance(r, tuple))
    assert has(heads(rows)[1], dict(clear_O=0, clear_set=0, clear_objpart=0, skip_obj=1))


def test_head_keeps_its_objective_without_a_round_behind_it():
    h = heads(run([(HEAD, 0, 0), (HEAD, 1, 0)], max_iter_kmeans=0))
    assert h[1]["skip_obj"] == 0 and h[1]["clear_O"] == 0
    # init_cluster's kind of head (no normalise) never skips: its caller takes a snapshot
    h = heads(run([(HEAD, 0, 0)] + call(head=False) + [(HEAD, 0, 0)]))
    assert h[1]["skip_obj"] == 0


def solve(K, d, B, C_=1, lds=1):
    out = (C.c_longlong * 3)()
    probe().probe_solve_lds(K, d, B, C_, lds, out)
    return dict(zip(("lds", "lds_sys_off", "lds_total"), out))


def test_solve_keeps_its_systems_in_lds_where_they_fit():
    """11 rows at 10 levels: cov 11 x 11 + rhs 50 x 11 doubles = 5368 bytes behind the form's 4584 (tests/test_plan_cpu.py), which keep their meaning"""
    t = solve(100, 50, 10)
    assert t == dict(lds=184 + 4400, lds_sys_off=4584, lds_total=4584 + 11 * 61 * 8)
    assert solve(100, 50, 10, lds=0) == dict(lds=4584, lds_sys_off=0, lds_total=4584)
    # 200 levels in three covariates: 201 x 251 doubles = 403608 bytes do not fit: global scratch
    t = solve(200, 50, 200, C_=3)
    assert t["lds_sys_off"] == 0 and t["lds_total"] == t["lds"]
    # the largest design whose systems fit behind the form within SOLVE_LDS_BYTES (158 KB), and the first that does not
    fits = [B for B in range(1, 300) if solve(100, 50, B)["lds_sys_off"]]
    assert fits == list(range(1, fits[-1] + 1))
    B = fits[-1]
    assert solve(100, 50, B)["lds_total"] <= 158 * 1024 < ((solve(100, 50, B + 1)["lds"] + 7) & ~7) + (B + 2) * (B + 2 + 50) * 8
