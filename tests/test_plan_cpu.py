"""The launch plan of hmx_setup (harmony_amd/csrc/hmx_plan.h) as a pure function: which path a shape takes, checked without a GPU.
Every expected value below is derived from the expressions of the setup code the plan was lifted out of, with the derivation beside it."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SHAPE = ("N", "N_global", "d", "K", "B", "C", "Q", "nb", "cells_per_block", "world", "sharded", "cus", "usig", "ridge_arith", "oe_arith",
              "obj_arith", "solve_arith", "tun_wps", "tun_tpw", "grid", "ntitems")
PLAN_FIELDS = ("KP", "zs", "NCT", "NQ", "NT4", "tail", "NS", "NS2", "wNQ", "wNT4", "wtail", "wNS", "moe_mfma", "dot_bf", "usig", "rvec", "pen_lds",
               "upd_wps", "upd_threads", "upd_maxblocks", "upd_tpw", "static_maxblocks", "oldsum_stream", "need_lorder", "nwmax", "objslots",
               "r_store_always", "carry_ok", "qmask", "nkeys", "npad", "shuf_inv", "solve_on_device", "st_KH", "st_halves", "st_dma", "st_cpw", "st_nwg",
               "fused_ok", "chain_ok", "chain_wgs", "chain_pair", "KH", "chain_folders", "chain_kw", "nrep", "upd_contig")
_probe = []


def plan_probe():
    """tests/cpp/plan_probe.cpp built once per session with the host compiler (the header needs no HIP)"""
    if not _probe:
        import tempfile
        so = os.path.join(tempfile.mkdtemp(prefix="plan_probe_"), "plan_probe.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "plan_probe.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.probe_plan.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_char_p, C.c_int]
        _probe.append(lib)
    return _probe[0]


def plan(N, K, d=50, B=20, C_=1, Q=None, nb=20, **kw):
    """the plan of one shape (the HMX_* switches come from the environment); a dict of PLAN_FIELDS, or {"limit": message}"""
    s = dict(N=N, N_global=N, d=d, K=K, B=B, C=C_, Q=B if Q is None else Q, nb=nb, cells_per_block=max(1, N // nb), world=1, sharded=0, cus=256, usig=1,
             ridge_arith=0, oe_arith=0, obj_arith=0, solve_arith=0, tun_wps=-1, tun_tpw=-1, grid=2048, ntitems=(N + 15) // 16)
    assert not set(kw) - set(s), kw
    s.update(kw)
    out = (C.c_int * len(PLAN_FIELDS))()
    msg = C.create_string_buffer(256)
    if plan_probe().probe_plan((C.c_longlong * len(PLAN_SHAPE))(*[int(s[k]) for k in PLAN_SHAPE]), out, msg, 256):
        return {"limit": msg.value.decode()}
    return dict(zip(PLAN_FIELDS, out))


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in [k for k in os.environ if k.startswith("HMX_")]:
        monkeypatch.delenv(k)


def diff(a, b):
    return {k for k in a if a[k] != b[k]}


# K = 100, 20 blocks, 256 CUs: the chain runs while N / 20 / 16 / (8 * 255) <= 20 tiles per resident wave, i.e. N <= 20 * 20 * 16 * 2040 = 13 056 000
# (the quotient is exactly 20.0 there); one more tile per block is 20 * 16 = 320 more cells.
CHAIN_N = 20 * 20 * 16 * 8 * 255
# K = 200, B = 200, C = 3: KH = 100, folders of kw = ((200 + 11) / 12 + 3) & ~3 = 20 clusters -> F = 10; the pair chain runs while
# N / 20 / 16 / (4 * (256 - 10)) <= 12 tiles per pair and block, i.e. N <= 12 * 984 * 16 * 20 = 3 778 560
PAIR_N = 12 * 4 * (256 - 10) * 16 * 20
C4 = dict(K=200, B=200, C_=3, Q=200)


def test_chain_threshold_and_replicas(monkeypatch):
    on, off = plan(CHAIN_N, 100), plan(CHAIN_N + 320, 100)
    assert CHAIN_N == 13056000
    assert (on["chain_ok"], on["fused_ok"], on["chain_pair"], on["chain_wgs"]) == (1, 1, 0, 256)
    assert (off["chain_ok"], off["fused_ok"], off["chain_pair"]) == (0, 1, 0)
    # replicas: 8 (8 * 20 * 100 entries are far below 2^20), 4 on the chain; contiguous tile ranges off the chain from 4 tiles per wave
    assert (on["nrep"], off["nrep"], on["upd_contig"], off["upd_contig"]) == (4, 8, 0, 1)
    assert diff(on, off) == {"chain_ok", "nrep", "upd_contig", "npad"}
    monkeypatch.setenv("HMX_NREP", "8")
    assert plan(CHAIN_N, 100)["nrep"] == 8 and plan(PAIR_N, **C4)["nrep"] == 8
    monkeypatch.setenv("HMX_NREP", "2")
    assert plan(CHAIN_N, 100)["nrep"] == 2 and plan(CHAIN_N + 320, 100)["nrep"] == 2


def test_configs4_shape_takes_the_pair_chain_up_to_12_tiles():
    on, off = plan(PAIR_N, **C4), plan(PAIR_N + 320, **C4)
    assert PAIR_N == 3778560
    # NCT = 13 > 7 cluster tiles: never the single-wave chain; 200 * 200 * 12 bytes of tables: no fold in the prologue either
    assert (on["NCT"], on["chain_ok"], on["fused_ok"], off["chain_ok"], off["fused_ok"]) == (13, 0, 0, 0, 0)
    assert (on["chain_pair"], on["KH"], on["chain_kw"], on["chain_folders"], on["nrep"], on["upd_contig"]) == (1, 100, 20, 10, 1, 0)
    assert (off["chain_pair"], off["nrep"], off["upd_contig"]) == (0, 8, 1)          # (5.8 tiles per wave: contiguous ranges)
    assert plan(5000000, **C4)["chain_pair"] == 0 and plan(1000000, **C4)["chain_pair"] == 1      # BASELINE configs[4] at 5M / 1M cells


def test_carry_upd_wps_and_moe_mfma():
    # carry: on iff nb^2 * Q * 64 <= N (nb <= 63, N + nb^2 * Q * 16 within int32, oe_arith off): 20^2 * 20 * 64 = 512 000
    on, off = plan(512000, 100), plan(511999, 100)
    assert (on["carry_ok"], on["qmask"], on["nkeys"], on["npad"]) == (1, 0x7FFFF, 400, 512000 + 400 * 20 * 16)
    assert (off["carry_ok"], off["qmask"], off["nkeys"], off["npad"]) == (0, 0x7FFFFFFF, 20, 511999 + 20 * 20 * 16)
    assert plan(512000, 100, oe_arith=1)["carry_ok"] == 0 and plan(64 * 64 * 64 * 20, 100, nb=64)["carry_ok"] == 0
    assert (on["shuf_inv"], off["shuf_inv"], plan(512000, 100, world=2, sharded=1)["shuf_inv"]) == (1, 0, 0)
    # four waves per SIMD iff uniform sigma and at most 4 cluster tiles (K <= 64)
    for K, usig, wps in ((64, 1, 4), (50, 1, 4), (64, 0, 2), (80, 1, 2), (100, 1, 2)):
        p = plan(100000, K, usig=usig)
        assert (p["upd_wps"], p["upd_threads"], p["usig"]) == (wps, 1024 if wps == 4 else 512, usig), (K, usig)
    # MFMA ridge kernels need K % 4 == 0 and d <= 64
    assert [plan(100000, K, d=d)["moe_mfma"] for K, d in ((100, 50), (100, 64), (50, 50), (99, 50), (100, 68), (100, 100))] == [1, 1, 0, 0, 0, 0]
    # split-bf16 distance GEMM: (NT4 > 4 or NS2 <= 2) and NS2 <= 4 -- rows of <= 64 PCs (two 32-PC steps) or of more than four 16-PC groups
    # (d = 68: zs = 68, NT4 = 4, NS2 = 3 -> off; d = 80: NT4 = 5 -> on)
    assert [plan(100000, 100, d=d)["dot_bf"] for d in (20, 50, 64, 68, 80, 100, 128)] == [1, 1, 1, 0, 1, 1, 1]


def test_limits():
    # centroid image: 4 quads x 50 PC steps x 1 KB at d = 200, K = 256 (beyond the envelope hmx_setup admits: its check comes first)
    assert "centroid image" in plan(100000, 256, d=200)["limit"]
    # padded order: 2e9 cells + 20 blocks x 500 000 combinations x 16 slots > 2 147 483 000 (no carry: 400 keys would not fit either)
    assert "padded block order" in plan(2000000000, 100, Q=500000)["limit"]
    assert plan(2000000000, 100, Q=20)["npad"] == 2000000000 + 400 * 20 * 16


@pytest.mark.parametrize("env,shape,flips", [
    ({"HMX_CHAIN": "0"}, dict(N=1000000, K=100), {"chain_ok": (1, 0), "nrep": (4, 8)}),
    ({"HMX_CHAIN": "1"}, dict(N=CHAIN_N + 320, K=100), {"chain_ok": (0, 1), "nrep": (8, 4), "upd_contig": (1, 0)}),
    ({"HMX_CHAIN": "1"}, dict(N=5000000, **C4), {"chain_pair": (0, 1), "nrep": (8, 1), "upd_contig": (1, 0)}),
    ({"HMX_CHAIN": "0"}, dict(N=2500000, **C4), {"chain_pair": (1, 0), "nrep": (1, 8)}),
    ({"HMX_CHAIN_PAIR": "0"}, dict(N=2500000, **C4), {"chain_pair": (1, 0), "nrep": (1, 8)}),
    ({"HMX_CHAIN_PAIR": "1"}, dict(N=5000000, **C4), {"chain_pair": (0, 1), "nrep": (8, 1), "upd_contig": (1, 0)}),
    ({"HMX_CHAIN_PAIR": "1"}, dict(N=1000000, K=100), {}),
    ({"HMX_SOLD_CARRY": "0"}, dict(N=1000000, K=100), {"carry_ok": (1, 0), "qmask": (0x7FFFF, 0x7FFFFFFF), "nkeys": (400, 20), "npad": (1128000, 1006400), "shuf_inv": (1, 0)}),
    ({"HMX_SOLD_CARRY": "1"}, dict(N=100000, K=100), {"carry_ok": (0, 1), "qmask": (0x7FFFFFFF, 0x7FFFF), "nkeys": (20, 400), "npad": (106400, 228000), "shuf_inv": (0, 1)}),
    ({"HMX_DOT": "f32"}, dict(N=1000000, K=100), {"dot_bf": (1, 0)}),
    ({"HMX_DOT": "f32"}, dict(N=1000000, **C4), {"dot_bf": (1, 0), "chain_pair": (1, 0), "nrep": (1, 8)}),      # (the pair chain exists in the split-bf16 build only)
    ({"HMX_USIG": "0"}, dict(N=1000000, K=100), {"usig": (1, 0)}),
    ({"HMX_USIG": "0"}, dict(N=1000000, K=64), {"usig": (1, 0), "upd_wps": (4, 2), "upd_threads": (1024, 512)}),
    ({"HMX_MOE_STATS": "atomic"}, dict(N=1000000, K=100), {}),      # (retired with the fp64-atomic statistics kernel: the slot form -- 62 500 tiles over 512 workgroups, 123 each -- stays)
    ({"HMX_MOE_SOLVE": "host"}, dict(N=1000000, K=100), {"solve_on_device": (1, 0)}),
    ({"HMX_SHUFFLE_INV": "0"}, dict(N=1000000, K=100), {"shuf_inv": (1, 0)}),
    ({"HMX_SHUFFLE_INV": "2"}, dict(N=1000000, K=100), {}),
    ({"HMX_SHUFFLE_INV": "2"}, dict(N=1000000, K=100, world=2, sharded=1), {"shuf_inv": (0, 1)}),
    ({"HMX_FUSED_FOLD": "0"}, dict(N=CHAIN_N + 320, K=100), {"fused_ok": (1, 0)}),
    ({"HMX_FUSED_FOLD": "0"}, dict(N=1000000, K=100), {"fused_ok": (1, 0), "chain_ok": (1, 0), "nrep": (4, 8)}),      # (the chain folds in its prologue)
])
def test_forcing_switch_flips_the_decision_it_documents(monkeypatch, env, shape, flips):
    base = plan(**shape)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    forced = plan(**shape)
    assert {k: (base[k], forced[k]) for k in diff(base, forced)} == flips
    if "HMX_MOE_STATS" in env:
        assert (forced["st_dma"], forced["st_cpw"], forced["st_nwg"]) == (1, 123, 509)


# ---- one k_tile launch (plan_tile_launch): which instantiation, of which build, on what grid, with how much LDS -------------------------------
KINDS = {"update": 0, "head": 1, "lloyd": 2, "seed": 3, "chain": 4}
LAUNCH_FIELDS = ("valid", "bf", "nct", "mode", "wps", "usig", "threads", "blocks", "lds")
KB = 1024


def shape_vector(N, K, d=50, B=20, C_=1, Q=None, nb=20, **kw):
    s = dict(N=N, N_global=N, d=d, K=K, B=B, C=C_, Q=B if Q is None else Q, nb=nb, cells_per_block=max(1, N // nb), world=1, sharded=0, cus=256, usig=1,
             ridge_arith=0, oe_arith=0, obj_arith=0, solve_arith=0, tun_wps=-1, tun_tpw=-1, grid=2048, ntitems=(N + 15) // 16)
    assert not set(kw) - set(s), kw
    s.update(kw)
    return (C.c_longlong * len(PLAN_SHAPE))(*[int(s[k]) for k in PLAN_SHAPE])


def tile_launch(kind, N, K, workgroups=256, r_store=1, fused_fold=-1, **kw):
    """the launch of one kind for a shape, as a dict of LAUNCH_FIELDS + "ran" (0: the library makes no such launch for the shape); None: plan limit.
    fused_fold -1: as the unsharded plan's path says (the chain folds, the update does off the chain where the tables fit)"""
    lib = plan_probe()
    lib.probe_tile_launch.argtypes = [C.POINTER(C.c_longlong), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 10)()
    if lib.probe_tile_launch(shape_vector(N, K, **kw), KINDS[kind], workgroups, r_store, fused_fold, out):
        return None
    return dict(zip(("ran",) + LAUNCH_FIELDS, out))


def launch(bf, nct, mode, wps, usig, threads, blocks, lds, ran=1):
    return dict(ran=ran, valid=1, bf=bf, nct=nct, mode=mode, wps=wps, usig=usig, threads=threads, blocks=blocks, lds=lds)


def test_headline_shape_launches():
    """K = 100, d = 50, 20 batches, 1M cells: NCT = 7 cluster tiles, rows of zs = 52 floats -> NS2 = 2 steps of 32 PCs: split image 7 * 2 * 3 KB = 42 KB"""
    img = 7 * 2 * 3 * KB
    # chain: O' int64 [20][100] + penalties fp32 [2000] + levels [20][1]; image + tables + 64 <= 150 KB and one workgroup per CU: split-bf16 build,
    # one workgroup of 512 threads per CU; rounds whose R rows nobody reads run MODE 5
    fold = 20 * 100 * 8 + (2000 + 20 * 1) * 4
    assert tile_launch("chain", 1000000, 100, r_store=0) == launch(1, 7, 5, 2, 1, 512, 256, img + fold)
    assert tile_launch("chain", 1000000, 100, r_store=1) == launch(1, 7, 4, 2, 1, 512, 256, img + fold)
    # static tiles: 62 500 tiles / 4 waves = 15 625 workgroups, capped at nwmax / 4 = 2048 and at static_maxblocks = 512 (NCT >= 5): two per CU, 2 * 42 KB fit
    assert tile_launch("head", 1000000, 100) == launch(1, 7, 1, 2, 1, 256, 512, img)
    assert tile_launch("seed", 1000000, 100) == launch(1, 7, 3, 2, 0, 256, 512, img)
    # Lloyd: int64 sums [100][50] + counts [100]; two workgroups per CU would need 2 * (42 KB + 40 800) > 160 KB, one fits: one of 512 threads on half
    # the grid -- and, for 5 .. 7 cluster tiles, three waves per SIMD: 768 threads
    sums = (100 * 50 + 100) * 8
    assert 2 * (img + sums) > 160 * KB >= img + sums
    assert tile_launch("lloyd", 1000000, 100) == launch(1, 7, 2, 3, 0, 768, 256, img + sums)


def test_update_launches_K64_and_configs4():
    # K = 64: NCT = 4, split image 4 * 2 * 3 KB; block of 50 000 cells: 3125 tiles + 20 combinations + 1 = 3146; fold in the prologue (fused_fold = 1):
    # O' [20][64] int64 + penalties [1280] + levels [20]
    img, fold = 4 * 2 * 3 * KB, 20 * 64 * 8 + (1280 + 20) * 4
    # uniform sigma: four waves per SIMD, 1024 threads = 16 waves per workgroup: ceil(3146 / 16) = 197 workgroups (< 256 resident, < nwmax / 16 = 512)
    assert tile_launch("update", 1000000, 64, fused_fold=1) == launch(1, 4, 0, 4, 1, 1024, 197, img + fold)
    # vector sigma: two waves per SIMD, 512 threads = 8 waves: ceil(3146 / 8) = 394, capped at upd_maxblocks = 256
    assert tile_launch("update", 1000000, 64, fused_fold=1, usig=0) == launch(1, 4, 0, 2, 0, 512, 256, img + fold)
    # K = 200, B = 200, three covariates, 200 combinations at 1M cells: the wave-pair chain, halves of KH = 100 clusters = 7 cluster tiles each.
    # workers: both halves' images 2 * 7 * 2 * 3 KB + levels [200][3] + exchange slots 4 * 2 * 2 * 16 * 8 + log2 penalties [8][4][16][7] fp32;
    # folders (20 clusters each): O slice + deltas [2][200][20] + masses [20], int64
    lds_w, lds_f = 2 * 7 * 2 * 3 * KB + 600 * 4 + 4 * 2 * 2 * 16 * 8 + 8 * 4 * 16 * 7 * 4, (2 * 200 * 20 + 20) * 8
    assert (lds_w, lds_f) == (104800, 64160) and plan(1000000, **C4)["KH"] == 100
    assert tile_launch("chain", 1000000, r_store=0, **C4) == launch(1, 7, 6, 2, 1, 512, 256, max(lds_w, lds_f))
    # the same at 5M cells: launch per step, NCT = 13, no table in LDS (200 * 200 * 4 > 24 KB: pen_lds = 0; no fold in the prologue): the image alone;
    # 15 625 tiles + 201 over 8 waves -> capped at 256
    t = tile_launch("update", 5000000, **C4)
    assert t == launch(1, 13, 0, 2, 1, 512, 256, 13 * 2 * 3 * KB) and tile_launch("chain", 5000000, **C4)["ran"] == 0


def test_fp32_build_where_the_split_form_is_not_offered(monkeypatch):
    fold, sums = 20 * 100 * 8 + (2000 + 20) * 4, (100 * 50 + 100) * 8
    # d = 68: zs = 68 -> NT4 = 4, NS2 = 3: dot_bf = 0; fp32 image [NQ = 2][NS = 17] KB; the chain has no variant without R stores there
    img = 2 * 17 * KB
    assert tile_launch("chain", 1000000, 100, d=68, r_store=0) == launch(0, 7, 4, 2, 1, 512, 256, img + fold)
    assert tile_launch("head", 1000000, 100, d=68) == launch(0, 7, 1, 2, 1, 256, 512, img)
    # HMX_DOT=f32 at d = 50: fp32 image [2][13] KB; Lloyd keeps two 256-thread workgroups per CU
    monkeypatch.setenv("HMX_DOT", "f32")
    img = 2 * 13 * KB
    assert tile_launch("chain", 1000000, 100, r_store=0) == launch(0, 7, 4, 2, 1, 512, 256, img + fold)
    assert tile_launch("lloyd", 1000000, 100) == launch(0, 7, 2, 2, 0, 256, 512, img + sums)
    assert tile_launch("update", 1000000, 64, fused_fold=1) == launch(0, 4, 0, 4, 1, 1024, 197, 1 * 13 * KB + 20 * 64 * 8 + (1280 + 20) * 4)


def resource_table_k_tile():
    """{(bf, nct, mode, wps, usig)} of the k_tile rows of profiles/r6_kernel_resources.txt: bf build in hmx_tile_bf, fp32 build in hmx_kernels"""
    import re
    rows = set()
    for line in open(os.path.join(ROOT, "profiles", "r6_kernel_resources.txt")):
        m = re.match(r"(hmx_\w+)\s.*\sk_tile<(\d+), (\d+), (\d+), (true|false), (true|false)>$", line.rstrip())
        if m:
            bf = int(m.group(6) == "true")
            assert m.group(1) == ("hmx_tile_bf" if bf else "hmx_kernels"), line
            rows.add((bf, int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5) == "true")))
    return rows


def test_every_planned_launch_of_the_envelope_is_a_kernel_of_the_build(monkeypatch):
    """Every launch the plan makes across the envelope is valid, within a CU's LDS, of a workgroup size the kernels are built for, and names an
    instantiation that the build has (profiles/r6_kernel_resources.txt) in the object of its build.  No allowance."""
    import numpy as np
    lib = plan_probe()
    lib.probe_tile_sweep.argtypes = [C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_longlong)]
    table = resource_table_k_tile()
    assert len(table) == 214
    key = lambda bf, nct, mode, wps, usig: (((bf * 32 + nct) * 8 + mode) * 8 + wps) * 2 + usig      # noqa: E731
    known = np.array(sorted(key(*r) for r in table))
    reached, n, buf = set(), 0, (C.c_longlong * (256 * 5 * 10))()
    for dot in (None, "f32"):
        if dot:
            monkeypatch.setenv("HMX_DOT", dot)
        for d in (1, 16, 50, 64, 68, 76, 100, 128):
            for B, C_, Q in ((2, 1, 2), (20, 1, 20), (200, 3, 200)):
                for nb in (1, 20, 64):
                    for usig in (0, 1):
                        for N in (2000, 1000000, 20000000):
                            for r_store in (0, 1):
                                lib.probe_tile_sweep(shape_vector(N, 1, d=d, B=B, C_=C_, Q=Q, nb=nb, usig=usig), r_store, buf)      # every K in 1 .. 256, all five kinds
                                a = np.frombuffer(buf, dtype=np.int64).reshape(256 * 5, 10)
                                a = a[a[:, 0] == 1]                                       # launches the library makes (plan admitted, kind on the shape's path)
                                ran, valid, bf, nct, mode, wps, us, threads, blocks, lds = a.T
                                k = key(bf, nct, mode, wps, us)
                                ok = (valid == 1) & (lds <= 160 * KB) & np.isin(threads, (256, 512, 768, 1024)) & (blocks >= 1) & np.isin(k, known)
                                assert ok.all(), (dot, d, B, nb, usig, N, r_store, a[~ok][:5])
                                n += len(a)
                                reached.update(np.unique(k).tolist())
    unreached = sorted(r for r in table if key(*r) not in reached)
    print("planned launches checked: %d; k_tile rows of the table no swept shape reaches (%d of %d):" % (n, len(unreached), len(table)))
    for bf, nct, mode, wps, usig in unreached:
        print("  %s k_tile<%d, %d, %d, %s, %s>" % ("hmx_tile_bf" if bf else "hmx_kernels", nct, mode, wps, str(bool(usig)).lower(), str(bool(bf)).lower()))
    assert n > 1000000


# ---- one launch of the ridge correction (plan_ridge_launch): which kernel of which form, on what grid, with how much LDS ------------------------------------
RIDGE_KINDS = {"stats": 0, "solve": 1, "apply": 2}
RIDGE_GEOM = ("K", "KP", "d", "B", "C", "Q", "NCT", "moe_mfma", "st_dma", "st_halves", "st_KH", "st_nwg", "wNQ", "wNS", "nitems", "naitems", "grid")
RIDGE_FIELDS = ("valid", "mfma", "p0", "p1", "gx", "gy", "gz", "threads", "lds", "lds_b_bytes", "lds_body_bytes", "lds_mask_off", "rgx", "rgy")


def ridge_launch(kind, N, K, nitems=None, naitems=None, forge=None, **kw):
    """the correction's launch of one kind for a shape, as a dict of RIDGE_FIELDS + "solve_on_device" (the plan's); None: plan limit.  nitems / naitems: the static
    work lists of <= 256 / <= 1024 cells (default: one combination's); forge: geometry fields overwritten after the plan (shapes hmx_setup never produces)"""
    lib = plan_probe()
    lib.probe_ridge_geom.argtypes = [C.POINTER(C.c_longlong), C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lib.probe_ridge_launch.argtypes = [C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_longlong)]
    lib.probe_ridge_launch.restype = None
    geom, sod, out = (C.c_longlong * len(RIDGE_GEOM))(), C.c_int(0), (C.c_longlong * len(RIDGE_FIELDS))()
    if lib.probe_ridge_geom(shape_vector(N, K, **kw), (N + 255) // 256 if nitems is None else nitems, (N + 1023) // 1024 if naitems is None else naitems, geom, C.byref(sod)):
        return None
    for k, v in (forge or {}).items():
        geom[RIDGE_GEOM.index(k)] = v
    lib.probe_ridge_launch(geom, RIDGE_KINDS[kind], out)
    return dict(zip(RIDGE_FIELDS, out), solve_on_device=sod.value)


def ridge(mfma, p0, p1, grid, threads, lds, solve=(0, 0, 0), reduce=(0, 0), valid=1):
    gx, gy, gz = grid
    return dict(valid=valid, mfma=mfma, p0=p0, p1=p1, gx=gx, gy=gy, gz=gz, threads=threads, lds=lds, lds_b_bytes=solve[0], lds_body_bytes=solve[1], lds_mask_off=solve[2],
                rgx=reduce[0], rgy=reduce[1], solve_on_device=1)


def test_ridge_solve_lds_terms():
    """l_moe_solve's expressions: index words ((4B + 6 + C) & ~1) * 4, panel (B + 1) * 16 * 8, right-hand sides (B + 1) * d * 8 -- in LDS while index words + them are within
    150 KB --, body = the larger; masks (B + 1) * ceil((B + 1) / 64) * 8 behind the body rounded up to 8, for C > 1 within 159 KB; 1024 threads from 49 rows on; one workgroup per cluster"""
    # B = 10, C = 1, d = 50: (46 & ~1) * 4 = 184; panel 11 * 128 = 1408 < right-hand sides 11 * 400 = 4400; no masks
    assert ridge_launch("solve", 100000, 100, B=10) == ridge(1, 0, 0, (100, 1, 1), 256, 184 + 4400, solve=(4400, 4400, 0))
    # B = 200, C = 3, d = 50: (809 & ~1) * 4 = 3232; right-hand sides 201 * 400 = 80400 > panel 25728; masks 201 * 4 * 8 = 6432 at (3232 + 80400 + 7) & ~7 = 83632
    assert ridge_launch("solve", 1000000, **C4) == ridge(1, 0, 0, (200, 1, 1), 1024, 83632 + 6432, solve=(80400, 80400, 83632))
    assert 83632 + 6432 == 90064
    # B = 1100, C = 1, d = 30: (4407 & ~1) * 4 = 17624; right-hand sides 1101 * 240 = 264240: not in LDS; body = panel 1101 * 128 = 140928
    assert ridge_launch("solve", 60000, 40, d=30, B=1100) == ridge(1, 0, 0, (40, 1, 1), 1024, 17624 + 140928, solve=(0, 140928, 0))
    assert 17624 + 140928 == 158552
    # d = 16, B = 1100: right-hand sides 1101 * 128 = the panel's bytes: beyond 150 KB beside the index words, but they fit the panel's space and stay in LDS
    assert ridge_launch("solve", 60000, 40, d=16, B=1100) == ridge(1, 0, 0, (40, 1, 1), 1024, 17624 + 140928, solve=(140928, 140928, 0))
    # threads: B + 1 > 48
    assert [ridge_launch("solve", 100000, 100, B=B)["threads"] for B in (47, 48)] == [256, 1024]
    # the envelope (plan_shape: (4B + 8 + C) * 4 + (B + 1) * 128 <= 158 KB = 161792): B = 1122 -> 17956 + 4 + 143744 = 161704 + 4C; B = 1123: 17972 + 4C + 143872 > 161792
    for C_ in (1, 2, 3, 4):
        last, first = ridge_launch("solve", 100000, 100, B=1122, C_=C_), ridge_launch("solve", 100000, 100, B=1123, C_=C_)
        assert (last["solve_on_device"], last["valid"], first["solve_on_device"], first["valid"]) == (1, 1, 0, 0), C_
    assert ridge_launch("solve", 100000, 100, B=1122)["lds"] == (4495 & ~1) * 4 + 1123 * 128 == 161720
    assert plan(100000, 100, B=1122)["solve_on_device"] == 1 and plan(100000, 100, B=1123)["solve_on_device"] == 0


def test_ridge_statistics_forms():
    # slot form, l_moe_stats_mfma's st_dma branch: grid (st_nwg, st_halves), a wave per PC tile incl. the ones column: 64 * ((d + 16) / 16) threads; fp64 shadows
    # [waves][nct * 4][64] doubles in LDS while two workgroups' fit 150 KB; reduce launch (Q, ceil((K d + K) / 256)).  1M cells: 62 500 tiles / 512 -> 123 per workgroup, 509 workgroups
    assert ridge_launch("stats", 1000000, 100) == ridge(1, 7, 1, (509, 1, 1), 256, 4 * 7 * 2048, reduce=(20, (100 * 50 + 100 + 255) // 256))
    # K > 128: two halves, st_KH = ((K + 1) / 2 + 3) & ~3 = 100 at K = 200 -> 7 cluster tiles per half, grid.y = 2
    assert ridge_launch("stats", 1000000, **C4) == ridge(1, 7, 1, (509, 2, 1), 256, 4 * 7 * 2048, reduce=(200, (200 * 50 + 200 + 255) // 256))
    for K in range(132, 257, 4):
        t, p = ridge_launch("stats", 100000, K), plan(100000, K)
        assert (t["valid"], t["gy"], t["p0"]) == (1, 2, (p["st_KH"] + 15) // 16) and p["st_halves"] == 2 and t["p0"] <= 8, K
    # d = 64: five waves; with 8 cluster tiles 2 * 5 * 8 * 2048 = 163 840 > 153 600: no LDS shadows -- K in 116 .. 128 (whole) and 228 .. 256 (halves of 116 .. 128); 7 tiles: 143 360 fit
    without = [K for K in range(4, 257, 4) if not ridge_launch("stats", 100000, K, d=64)["p1"]]
    assert without == list(range(116, 129, 4)) + list(range(228, 257, 4))
    assert all(ridge_launch("stats", 100000, K, d=64) == dict(ridge_launch("stats", 100000, K, d=64), valid=1, threads=320, lds=0, p0=8) for K in without)
    assert all(ridge_launch("stats", 100000, K, d=63)["p1"] == 1 and ridge_launch("stats", 100000, K, d=63)["threads"] == 256 for K in range(4, 257, 4))
    assert ridge_launch("stats", 100000, 128, d=63)["lds"] == 4 * 8 * 2048 and ridge_launch("stats", 100000, 112, d=64)["lds"] == 5 * 7 * 2048
    # every shape with the MFMA kernels takes the slot form, on an instantiation that exists (1 .. 8 cluster tiles)
    for K in range(4, 257, 4):
        for d in (1, 16, 50, 64):
            t, p = ridge_launch("stats", 100000, K, d=d), plan(100000, K, d=d)
            assert (p["moe_mfma"], p["st_dma"], t["valid"], t["mfma"]) == (1, 1, 1, 1) and 1 <= t["p0"] <= 8, (K, d)
    # first generation (l_moe_stats), K = 50 (K % 4 != 0), d = 50: zch = 2 chunks of ceil(50 / 2) = 25 -> DP = 28, grid.z = ceil(50 / 28) = 2; 128 clusters per grid.y;
    # 100 000 cells: 391 items of 256 cells, four per workgroup -> 98
    assert ridge_launch("stats", 100000, 50) == ridge(0, 28, 0, (98, 1, 2), 256, 0)
    assert ridge_launch("stats", 100000, 130, d=128) == ridge(0, 32, 0, (98, 2, 4), 256, 0)      # (d = 128: four chunks of 32)
    assert ridge_launch("stats", 100000000, 50)["gx"] == 2048                                   # (capped at the streaming grid)
    # forged geometries: 9 cluster tiles in one half have no instantiation; the MFMA form without its slots (st_dma = 0) has no kernel any more
    assert ridge_launch("stats", 100000, 100, forge={"NCT": 9})["valid"] == 0
    assert ridge_launch("stats", 100000, 100, forge={"st_dma": 0})["valid"] == 0


def test_ridge_apply_forms():
    # MFMA form (l_moe_apply_mfma), K = 100: NPT = ceil(d / 16); the image of one combination [wNQ = 1][wNS = 4 * 6 + 1 = 25] KB; 98 apply items of 1024 cells, one workgroup each
    for d, npt in ((16, 1), (17, 2), (64, 4)):
        assert ridge_launch("apply", 100000, 100, d=d) == ridge(1, npt, 0, (98, 1, 1), 256, 25 * KB), d
    # d = 65: the plan takes the first generation (l_moe_apply): KPL = KP / 64 = 2, DPL = 2 (d > 64), K * 64 * DPL floats of LDS
    assert ridge_launch("apply", 100000, 100, d=65) == ridge(0, 2, 2, (98, 1, 1), 256, 100 * 64 * 2 * 4)
    assert ridge_launch("apply", 100000, 100, d=65, forge={"moe_mfma": 1})["valid"] == 0      # (NPT = 5: no instantiation)
    # first generation at K = 50 (KP = 64): DPL = 1 up to d = 64
    for d, dpl in ((16, 1), (17, 1), (64, 1), (65, 2)):
        assert ridge_launch("apply", 100000, 50, d=d) == ridge(0, 1, dpl, (98, 1, 1), 256, 50 * 64 * dpl * 4), d
    assert ridge_launch("apply", 100000000, 100)["gx"] == 4 * 2048 and ridge_launch("apply", 100000, 50, forge={"KP": 320})["valid"] == 0


def test_every_planned_ridge_launch_is_a_kernel_of_the_build():
    """Across K = 1 .. 256 and a spread of d, every statistics / apply launch the plan makes names an instantiation of profiles/r6_kernel_resources.txt"""
    import re
    names = set()
    for line in open(os.path.join(ROOT, "profiles", "r6_kernel_resources.txt")):
        m = re.match(r"hmx_kernels\s.*\s(k_moe_\w+<[^>]*>)$", line.rstrip())
        if m:
            names.add(m.group(1))
    assert len(names) == 8 + 16 + 8 + 4 and not any(n.startswith("k_moe_stats_mfma") for n in names), sorted(names)
    for K in range(1, 257):
        for d in (1, 16, 17, 50, 63, 64, 65, 100, 128):
            st, ap = ridge_launch("stats", 100000, K, d=d), ridge_launch("apply", 100000, K, d=d)
            assert st["valid"] and ap["valid"] and ridge_launch("solve", 100000, K, d=d)["valid"], (K, d)
            want = ("k_moe_stats_q<%d, %s>" % (st["p0"], "true" if st["p1"] else "false") if st["mfma"] else "k_moe_stats<%d>" % st["p0"],
                    "k_moe_apply_mfma<%d>" % ap["p0"] if ap["mfma"] else "k_moe_apply<%d, %d>" % (ap["p0"], ap["p1"]))
            assert set(want) <= names, (K, d, want)
