"""CPU-side checks of the product: the C-ABI library loads and exports every symbol that
include/harmony_mi355x.h declares, the documented generators agree with the oracle's independent
implementation, host-side argument handling mirrors R/ui.R, and the library refuses to run
without a GPU (no CPU fallback).  No compute calls."""
import os
import re

import numpy as np
import pytest

import harmony_amd
from harmony_amd import _lib
from oracle.oracle import load as load_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    # the reference's interface (harmony_mi355x.h) and the laboratory equipment (harmony_mi355x_lab.h: probes, tuning) -- together everything the library exports
    pub = set(re.findall(r"\b(hmx_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "harmony_mi355x.h")).read())) - {"hmx_allreduce_fn"}
    lab = set(re.findall(r"\b(hmx_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "harmony_mi355x_lab.h")).read())) - {"hmx_allreduce_fn", "hmx_setup", "hmx_get_matrix", "hmx_set_int", "hmx_compute_objective"}
    assert not (pub & lab) and not [n for n in pub if "debug" in n], (pub & lab)
    assert len(pub) <= 32, sorted(pub)             # (the module's methods and fields, randomness, multi-GPU: no probes)
    declared = pub | lab
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), "missing export: " + name
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))


def test_generators_match_oracle_spec():
    lib, orc = _lib.load(), load_oracle()
    for seed, rnd, N in [(1, 0, 300), (7, 3, 2370), (123456789, 17, 1000003), (5, 2, 6), (9, 1, 64), (9, 1, 65)]:
        gs = np.unique(np.concatenate([np.arange(min(N, 50)), np.random.default_rng(0).integers(0, N, 50)]))
        for g in gs:
            assert lib.hmx_feistel_pos(seed, rnd, N, int(g)) == orc.orc_feistel_pos(seed, rnd, N, int(g))
    for args in [(1, 0, 0), (1, 1, 5), (99, 101, 123456789), (2**40 + 3, 7, 2**33)]:
        assert lib.hmx_u01(*args) == orc.orc_u01(*args)
        assert 0.0 < lib.hmx_u01(*args) < 1.0


def test_r_compatible_stream_known_answers():
    """the R-compatible generator (product: harmony_amd/csrc/hmx_rrng.h; oracle: its own restatement) against
    MT19937's published known-answer vector and R's documented `set.seed(s); runif(n)` streams; the two independent
    implementations must also produce the same arma::shuffle order (ties included: same std::sort)."""
    import ctypes as C
    from oracle import oracle as orc
    lib = _lib.load()
    key = (C.c_uint32 * 4)(0x123, 0x234, 0x345, 0x456)
    out = (C.c_uint32 * 5)()
    lib.hmx_mt19937_by_array(key, 4, 5, out)                       # mt19937ar.c's test output (Matsumoto & Nishimura)
    assert list(out) == [1067595299, 955945823, 477289528, 4107218783, 4228976476]
    known = {1: [0.2655087, 0.3721239, 0.5728534], 42: [0.9148060, 0.9370754, 0.2861395], 123: [0.2875775, 0.7883051, 0.4089769]}
    for seed, vals in known.items():
        u = np.empty(3)
        lib.hmx_r_runif(seed, 3, u.ctypes.data_as(C.POINTER(C.c_double)))
        np.testing.assert_allclose(u, vals, atol=5e-8)
        np.testing.assert_array_equal(u, orc.r_runif(seed, 3))     # bit-identical across the two implementations
    for seed, N in [(1, 10), (7, 2370), (99, 200003)]:
        a = np.empty(N, dtype=np.int64)
        lib.hmx_r_shuffle(seed, N, a.ctypes.data_as(C.POINTER(C.c_int64)))
        assert np.array_equal(np.sort(a), np.arange(N))
        assert np.array_equal(a, orc.r_shuffle(seed, N))


def test_feistel_inverse():
    """hmx_feistel_cell is the inverse of hmx_feistel_pos (the sort-free shuffle enumerates a block's cells with it): for domains with
    little and with heavy cycle walking, and it lists every block's cells exactly once."""
    lib = _lib.load()
    for seed, rnd, N in [(1, 0, 300), (7, 3, 2370), (123456789, 17, 1000003), (5, 2, 6), (9, 1, 64), (9, 1, 65), (3, 4, 70001)]:
        gs = np.unique(np.concatenate([np.arange(min(N, 40)), np.random.default_rng(1).integers(0, N, 60)]))
        for g in gs:
            p = lib.hmx_feistel_pos(seed, rnd, N, int(g))
            assert 0 <= p < N and lib.hmx_feistel_cell(seed, rnd, N, p) == int(g)
    N, nb = 1000, 20
    cpb = N // nb
    cells = [lib.hmx_feistel_cell(11, 2, N, p) for p in range(N)]
    assert sorted(cells) == list(range(N))
    for b in range(nb):
        assert all(min(lib.hmx_feistel_pos(11, 2, N, c) // cpb, nb - 1) == b for c in cells[b * cpb:(b + 1) * cpb])


def test_feistel_is_a_permutation():
    lib = _lib.load()
    for N in (6, 40, 300, 1000, 4097):
        pos = np.array([lib.hmx_feistel_pos(11, 2, N, g) for g in range(N)])
        assert np.array_equal(np.sort(pos), np.arange(N))
    a = np.array([lib.hmx_feistel_pos(11, 2, 1000, g) for g in range(1000)])
    b = np.array([lib.hmx_feistel_pos(11, 3, 1000, g) for g in range(1000)])
    assert (a != b).mean() > 0.9  # a fresh shuffle every round
    blocks = a // 50
    assert np.array_equal(np.bincount(blocks), np.full(20, 50))  # balanced blocks (src/harmony.cpp:280-300)


def test_prepare_setup_args_mirrors_ui_R():
    rng = np.random.default_rng(0)
    Z = rng.normal(size=(90, 5))
    meta = {"a": np.array(list("xyz") * 30), "b": np.repeat([2, 1], 45)}
    kw, dm = harmony_amd.prepare_setup_args(Z, meta, ["a", "b"])
    assert dm.shape == (5, 90)                                   # transposed (R/ui.R:178-183)
    assert kw["K"] == 3                                          # min(round(N/30), 100)
    assert list(kw["B_vec"]) == [3, 2] and kw["Phi"][3] == 5
    assert np.array_equal(kw["theta"], np.full(5, 2.0))          # theta=2 per covariate, expanded per level
    assert np.array_equal(kw["lambda_vec"], [-1.0])              # automatic lambda
    assert np.array_equal(kw["sigma"], np.full(3, 0.1))
    i, p = kw["Phi"][0], kw["Phi"][1]
    assert np.array_equal(p, np.arange(91) * 2)
    assert set(i[0::2]) == {0, 1, 2} and set(i[1::2]) == {3, 4}
    assert i[1] == 3 + 1  # level "2" sorts after "1" (as.factor)
    kw, _ = harmony_amd.prepare_setup_args(Z, meta, ["a", "b"], lambda_=[1.0, 3.0], theta=[1, 0.5], nclust=7, sigma=0.2,
                                           options=harmony_amd.harmony_options(tau=5))
    assert np.array_equal(kw["lambda_vec"], [0, 1, 1, 1, 3, 3])
    N_b = np.array([30, 30, 30, 45, 45.0])
    np.testing.assert_allclose(kw["theta"], np.array([1, 1, 1, .5, .5]) * (1 - np.exp(-(N_b / (7 * 5)) ** 2)))
    kw, _ = harmony_amd.prepare_setup_args(Z, np.repeat([0, 1, 2], 30), None)   # bare vector (R/ui.R:158-162)
    assert kw["Phi"][3] == 3
    kw, _ = harmony_amd.prepare_setup_args(Z, meta, "a", early_stop=False)
    assert kw["epsilon_harmony"] == -np.inf
    for bad in (dict(vars_use="nope"), dict(vars_use="a", lambda_=[1, 2]), dict(vars_use="a", theta=[1, 2]),
                dict(vars_use="a", lambda_=-1.0)):
        with pytest.raises(ValueError):
            harmony_amd.prepare_setup_args(Z, meta, **bad)
    with pytest.raises(ValueError):
        harmony_amd.harmony_options(block_size=0)
    with pytest.raises(TypeError):
        harmony_amd.RunHarmony(Z, meta, "a", max_iter_harmony=3)     # legacy args hard-error (R/harmony_option.R:67-81)


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="a GPU is present")
def test_no_cpu_fallback():
    with pytest.raises(harmony_amd.HarmonyError, match="no HIP device"):
        harmony_amd.RunHarmony(np.random.randn(300, 20), np.repeat([0, 1, 2], 100), verbose=False)


def test_r_glue_type_checks_against_the_c_abi():
    """r/harmony_mi355x_glue.c (the .Call wrappers INTEGRATION.md describes) cannot be built here -- R is not installed --
    but it must at least agree with include/harmony_mi355x.h: compile it (syntax + types only) against a minimal stand-in
    for R's C API (tests/stubs/), with implicit declarations and pointer/int mismatches as errors."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found"
    p = subprocess.run([gcc, "-std=c11", "-fsyntax-only", "-Wall", "-Werror=implicit-function-declaration",
                        "-Werror=incompatible-pointer-types", "-Werror=int-conversion", "-Wno-cast-function-type",
                        "-I" + os.path.join(root, "tests", "stubs"), "-I" + os.path.join(root, "include"),
                        os.path.join(root, "r", "harmony_mi355x_glue.c")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_r_glue_runs_against_an_emulated_r_api_and_fails_the_r_way():
    """The same glue, EXECUTED: linked with tests/stubs/r_emul.c (an emulation of the R C API calls it makes) and driven like
    r/harmony_mi355x.R drives it -- .Call names resolved through the table R_init_harmony registers, R-typed arguments.  Without a GPU
    every path ends in an R error: the library's no-fallback message arrives through Rf_error, wrong argument counts and unknown
    routines are refused like .Call refuses them, a finalized object is detected.  (The whole sequence: tests/test_gpu_parity2.py.)"""
    import numpy as np
    import r_emul
    from harmony_amd import prepare_setup_args
    g = r_emul.GlueHarmony(seed=5)
    assert g.get("N")[0] == 0 and g.get("objective_kmeans").size == 0
    rng = np.random.default_rng(0)
    skw, _ = prepare_setup_args(rng.normal(size=(200, 6)), {"b": np.arange(200) % 3}, "b", nclust=4)
    with pytest.raises(r_emul.RError, match="setup: no HIP device available: libharmony_mi355x has no CPU fallback"):
        g.setup(**skw)
    with pytest.raises(r_emul.RError, match="setup: no HIP device"):
        g.setup(single=True, **skw)
    with pytest.raises(r_emul.RError, match="expected the integer bit matrix of a float32 object"):
        r_emul.dot_call("C_hmx_setup_f32", g.ptr, r_emul.numeric(skw["Z"]), *[r_emul.numeric([0.0])] * 16)
    with pytest.raises(r_emul.RError, match="unknown field 'nope'"):
        g.get("nope")
    with pytest.raises(r_emul.RError, match="expecting 2 for 'C_hmx_get'"):
        r_emul.dot_call("C_hmx_get", g.ptr)
    with pytest.raises(r_emul.RError, match="not in the registration table"):
        r_emul.dot_call("C_hmx_nope", g.ptr)
    g.release()                                       # the finalizer destroys the handle and clears the pointer ...
    with pytest.raises(r_emul.RError, match="harmony object has been destroyed"):
        g.get("N")
    g.release()                                       # ... and running it again is harmless


def test_plain_c_host_links_and_fails_loudly_without_gpu(tmp_path):
    """examples/host_example.c drives the library from C exactly like R/ui.R drives the Rcpp module.  It must compile and
    link against the C ABI alone (no Python, no torch); on this GPU-less box hmx_setup must fail with the no-fallback error."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found"
    exe = str(tmp_path / "host_example")
    libdir = os.path.join(root, "harmony_amd", "lib")
    p = subprocess.run([gcc, "-std=c11", "-Wall", "-Werror=implicit-function-declaration", "-I" + os.path.join(root, "include"),
                        os.path.join(root, "examples", "host_example.c"), "-L" + libdir, "-lharmony_mi355x",
                        "-Wl,-rpath," + libdir, "-lm", "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the example would run to completion (covered by the gpu tests)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr, (r.stdout, r.stderr)


def test_cluster_to_column_mapping_is_a_bijection():
    """kcol (hmx_internal.h): for every instantiated cluster-tile count the 16 x nct MFMA columns hold each cluster index exactly
    once, a lane's columns ascend with the tile index (arg-min ties -> smallest k), the four columns of a full quad of tiles are
    four CONSECUTIVE clusters (16-byte R stores) and the r = nct % 4 remaining tiles r consecutive ones; inverse and forward map agree."""
    lib = _lib.load()
    for nct in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16):
        seen = set()
        for c in range(16):
            ks = [lib.hmx_cluster_of_column(nct, ct, c) for ct in range(nct)]
            assert all(k >= 0 for k in ks), (nct, c, ks)
            assert ks == sorted(ks)
            nfull, r = nct // 4, nct % 4
            for q in range(nfull):
                assert ks[4 * q:4 * q + 4] == [64 * q + 4 * c + j for j in range(4)]
            assert ks[4 * nfull:] == [64 * nfull + r * c + j for j in range(r)]
            seen.update(ks)
        assert seen == set(range(16 * nct))
    assert lib.hmx_cluster_of_column(7, 7, 0) == -1 and lib.hmx_cluster_of_column(0, 0, 0) == -1


def test_split_bf16_helpers(tmp_path):
    """the three-way bf16 split the tile kernels and the host image builder share (hmx_internal.h: bf3_split, bfimg_index):
    hi + mid + lo reproduces every fp32 number EXACTLY, every part is a bf16 number, the six products the kernels keep reproduce a product
    to 2^-21 of |x||y| at worst (2^-24 in the median), and the image index is a bijection of (PC, cluster, part) onto the 16-byte-per-lane B-operand layout."""
    import ctypes as C
    import subprocess
    so = tmp_path / "bf3_probe.so"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "bf3_probe.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.probe_bf3_split.argtypes = [C.c_float, C.POINTER(C.c_uint16)]
    lib.probe_bfimg_index.restype = C.c_longlong
    lib.probe_bfimg_index.argtypes = [C.c_int] * 5
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.normal(size=2000).astype(np.float32), (rng.normal(size=2000) * np.exp(rng.normal(size=2000) * 8)).astype(np.float32),
                         np.array([0.0, -0.0, 1.0, -1.0, 1 - 2.0**-24, 2.0**-24, 3.4e38, -3.4e38, 1.17549435e-38, 0.1, 1.0 / 3], np.float32)])

    def parts(x):
        p = (C.c_uint16 * 3)()
        lib.probe_bf3_split(C.c_float(float(x)), p)
        return [np.array([int(v) << 16], np.uint32).view(np.float32)[0] for v in p]       # a bf16 number IS the upper half of an fp32 one
    split = np.array([parts(x) for x in xs], np.float64)                                  # (fp64 holds sums of three fp32 numbers exactly)
    assert np.array_equal(split.sum(axis=1), xs.astype(np.float64))
    assert np.all(np.abs(split[:, 1]) <= np.abs(xs) * 2.0**-7 + 1e-45) and np.all(np.abs(split[:, 2]) <= np.abs(xs) * 2.0**-15 + 1e-45)
    a, b = split[:2000], split[2000:4000]
    six = a[:, 0] * b[:, 0] + a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 0] * b[:, 2] + a[:, 2] * b[:, 0]
    exact = xs[:2000].astype(np.float64) * xs[2000:4000].astype(np.float64)
    # dropped: mid lo + lo mid + lo lo < 2 * 2^-7 * 2^-15 |x||y| = 2^-21 |x||y| in the worst case of the truncating split (typically 2^-23):
    # the size of the rounding error a 50-term fp32 fmaf chain accumulates anyway (test_gpu_dots.py measures both against fp64)
    rel = np.abs(six - exact) / np.maximum(np.abs(exact), 1e-300)
    assert rel.max() <= 2.0**-21 and np.median(rel) <= 2.0**-24, (rel.max(), np.median(rel))
    for nct, ns2, K, d in ((7, 2, 100, 50), (13, 2, 200, 50), (4, 4, 60, 100), (1, 1, 12, 20)):
        seen = set()
        for k in range(K):
            for j in range(d):
                for part in range(3):
                    i = lib.probe_bfimg_index(nct, ns2, j, k, part)
                    assert 0 <= i < nct * ns2 * 3 * 512 and i not in seen
                    seen.add(i)
                    lane, slot = (i // 8) % 64, i % 8
                    assert slot == j % 8 and lane // 16 == (j % 32) // 8 and ((i // 8) // 64) % 3 == part
                    ct = (i // 8) // 64 // 3 // ns2
                    assert lib.probe_kcol(nct, ct, lane % 16) == k and ((i // 8) // 64 // 3) % ns2 == j // 32


def test_writable_fields_validate_their_values():
    """hmx_set_int needs no device: the settings of the restarted sums (round 5) and the arithmetic switches accept their documented ranges and refuse
    the rest with HMX_ERR_ARG and a message -- a typo must not silently select a default."""
    import ctypes as C
    from harmony_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    try:
        ok = {"seq_passes": 2, "seq_warm_passes": 2, "seq_tol_ppb": 10000, "seq_strict": 1, "seq_stats": 1, "seq_max_passes": 64, "ref_arith": 1, "rng": 1,
              "max_iter_kmeans": 7, "seed": 42}
        for f, v in ok.items():
            assert lib.hmx_set_int(h, f.encode(), v) == 0, (f, lib.hmx_last_error(h))
        bad = {"seq_passes": 1, "seq_warm_passes": 0, "seq_tol_ppb": -1, "seq_max_passes": 1000, "ref_arith": 3, "rng": 3, "no_such_field": 1}
        for f, v in bad.items():
            assert lib.hmx_set_int(h, f.encode(), v) != 0, f
            assert len(lib.hmx_last_error(h)) > 0
        # getters of scalar settings that need no device
        out = (C.c_double * 1)()
        assert lib.hmx_get(h, b"max_iter_kmeans", out, 1) == 1 and out[0] == 7.0
    finally:
        lib.hmx_destroy(h)


def test_documented_switches_and_writable_fields_are_the_ones_in_the_code():
    """INTEGRATION.md's table of environment switches and the header's list of writable fields against the library's sources, both ways:
    every getenv("HMX_...") of the library is documented, every documented switch is still read, every writable field the header names
    is a key the library knows (the round-4 verdict counted the switches; this keeps the documentation of what is left honest)."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "harmony_amd", "csrc")
    code = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)))
    envs = set(re.findall(r'getenv\("(HMX_[A-Z0-9_]+)"\)', code))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    sec = integ[integ.index("## Environment switches"):]
    live, removed = sec.split("*removed in round 5*")
    doc = set(re.findall(r"`(HMX_[A-Z0-9_]+)", live)) | set(re.findall(r"`(HMX_[A-Z0-9_]+)", removed[removed.index("|\n") + 1:]))
    assert envs == doc, (sorted(envs - doc), sorted(doc - envs))
    gone = set(re.findall(r"`(HMX_[A-Z0-9_]+)", removed[:removed.index("|\n")]))
    assert gone and not (gone & envs)                   # what the table calls removed really is
    hdr = open(os.path.join(root, "include", "harmony_mi355x.h")).read()
    w = hdr[hdr.index("/* writable fields:"):hdr.index("int hmx_set_int")]
    lab = open(os.path.join(root, "include", "harmony_mi355x_lab.h")).read()
    w += lab[lab.index("writable fields:"):lab.index("environment, read by hmx_setup")]
    keys = set(re.findall(r'"([a-z_:]+)"', w)) - {"randomness", "measurement", "arithmetic", "reference arithmetic"}
    assert len(keys) > 15
    assert not [k for k in keys if '"%s"' % k not in code]


def test_r_companion_package_assembles_and_registers_under_its_own_name(tmp_path):
    """The recommended binding: r/make_companion_package.sh assembles the R package `harmonymi355x` from the repository's
    single sources.  No R here -- so: the tree has what R CMD INSTALL needs (DESCRIPTION, NAMESPACE with useDynLib + the export, R/, src/ with
    Makevars pointing at this checkout), and the glue compiled with the package's own flags defines R_init_harmonymi355x (the name R looks
    for when it loads harmonymi355x.so), not R_init_harmony -- the reference package keeps its own DLL and registration."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "harmonymi355x"
    p = subprocess.run(["bash", os.path.join(root, "r", "make_companion_package.sh"), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "R/ui.R:269" in p.stdout
    have = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert have == ["DESCRIPTION", "NAMESPACE", "R/harmony_mi355x.R", "src/Makevars", "src/harmony_mi355x_glue.c"]
    ns = (out / "NAMESPACE").read_text()
    assert "useDynLib(harmonymi355x, .registration = TRUE)" in ns and "export(new_harmony_mi355x)" in ns
    assert "Package: harmonymi355x" in (out / "DESCRIPTION").read_text()
    mk = (out / "src" / "Makevars").read_text()
    assert "HMX_ROOT = " + root in mk and "-lharmony_mi355x" in mk and "@HMX_ROOT@" not in mk
    flags = re.search(r"PKG_CPPFLAGS = (.*)", mk).group(1).replace("$(HMX_ROOT)", root).split()
    assert "-DHMX_R_PACKAGE=harmonymi355x" in flags
    obj = tmp_path / "glue.o"
    p = subprocess.run([shutil.which("gcc"), "-std=c11", "-c", "-fPIC", "-I" + os.path.join(root, "tests", "stubs")] + flags +
                       [str(out / "src" / "harmony_mi355x_glue.c"), "-o", str(obj)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    syms = subprocess.run(["nm", "--defined-only", str(obj)], capture_output=True, text=True).stdout
    assert " T R_init_harmonymi355x" in syms and "R_init_harmony\n" not in syms.replace("R_init_harmonymi355x", "")
    # every routine the R file calls is in the table the glue registers
    rsrc = (out / "R" / "harmony_mi355x.R").read_text()
    csrc = (out / "src" / "harmony_mi355x_glue.c").read_text()
    called = set(re.findall(r'"(C_hmx_[a-z0-9_]+)"', rsrc))
    registered = set(re.findall(r'\{"(C_hmx_[a-z0-9_]+)", \(DL_FUNC\)', csrc))
    assert called and called <= registered, sorted(called - registered)


REF_PACKAGE_FACTS = os.path.join(ROOT, "tests", "golden", "ref_package_facts.json")


def ref_package_facts(pkg):
    """What the test below needs to know of the reference package at `pkg`, as data and without its text: length and SHA-256 of every line
    of R/ui.R, the routines src/RcppExports.cpp registers, and which of them R/utils.R calls (tools/make_ref_package_facts.py writes
    tests/golden/ref_package_facts.json from it)."""
    import hashlib
    ui = open(os.path.join(pkg, "R", "ui.R")).read().split("\n")
    routines = sorted(set(re.findall(r'\{"(_harmony_\w+)", \(DL_FUNC\)', open(os.path.join(pkg, "src", "RcppExports.cpp")).read())))
    utils = open(os.path.join(pkg, "R", "utils.R")).read()
    return {"ui_R_line_length": [len(l) for l in ui], "ui_R_line_sha256": [hashlib.sha256(l.encode()).hexdigest() for l in ui],
            "registered_routines": routines,
            "utils_R_calls": sorted(r[len("_harmony_"):] for r in routines if re.search(r"\b%s\(" % r[len("_harmony_"):], utils))}


def test_the_one_line_edit_applies_to_the_reference_package(tmp_path):
    """INTEGRATION.md's claim, checked against the reference's own file: r/ui_R_269.sed changes exactly ONE line of R/ui.R -- line 269,
    `harmonyObj <- new(harmony)` -- and leaves the reference's engine as the fallback.  And the reason the companion package is the
    recommended route: the reference's DLL registers three more routines than the module (src/RcppExports.cpp:60-62), one of which
    (scaleRows_dgc) its own R code calls (R/utils.R:93) -- a glue that REPLACED that DLL's registration would break them.
    The package is read through tests/golden/ref_package_facts.json (line lengths and digests, no text); where the package itself is on disk,
    the fixture must still describe it.  The sed pattern matches exactly the lines `<spaces>harmonyObj <- new(harmony)<spaces>`: every such
    line of each recorded length is tried against the digests, so no other line of the file can be one."""
    import hashlib
    import json
    import subprocess
    from oracle import ref as oref
    facts = json.load(open(REF_PACKAGE_FACTS))
    pkg = os.path.dirname(oref._REF_SRC)
    if os.path.exists(os.path.join(pkg, "R", "ui.R")):
        assert ref_package_facts(pkg) == facts
    stmt = "harmonyObj <- new(harmony)"
    found = {}
    for i, (n, h) in enumerate(zip(facts["ui_R_line_length"], facts["ui_R_line_sha256"])):
        for lead in range(n - len(stmt) + 1):
            line = " " * lead + stmt + " " * (n - len(stmt) - lead)
            if hashlib.sha256(line.encode()).hexdigest() == h:
                found[i + 1] = line
    assert list(found) == [269], sorted(found)
    old = [found[269], "harmonyObj$setup(", "    " + stmt + "  # not alone on its line"]
    work = tmp_path / "ui.R"
    work.write_text("\n".join(old))
    assert subprocess.run(["sed", "-i", "-f", os.path.join(ROOT, "r", "ui_R_269.sed"), str(work)]).returncode == 0
    new = work.read_text().split("\n")
    assert len(new) == len(old) and new[1:] == old[1:] and new[0] != old[0]
    assert new[0].startswith(found[269][:len(found[269]) - len(found[269].lstrip())] + "harmonyObj <- if (")
    assert "harmonymi355x::new_harmony_mi355x()" in new[0] and new[0].rstrip().endswith("else new(harmony)")
    assert {"_harmony_" + f for f in ("kmeans_centers", "scaleRows_dgc", "find_lambda_cpp")} <= set(facts["registered_routines"])
    assert "scaleRows_dgc" in facts["utils_R_calls"]


def test_methods_called_out_of_order_fail_cleanly():
    """The module object's methods are callable in any order after construction (the reference keeps ran_setup / ran_init
    flags but does not enforce them -- an early cluster_cpp reads empty matrices).  The C ABI enforces them: every entry point called on a
    fresh or a NULL handle returns a status (HMX_ERR_STATE = 6 / HMX_ERR_ARG = 1 / -1 for the sizing getters) and a message, never a
    crash -- no device is touched, so this runs without a GPU."""
    import ctypes as C
    lib = _lib.load()
    h = C.c_void_p(lib.hmx_create())
    buf, i64, u8 = (C.c_double * 16)(), (C.c_int64 * 16)(), (C.c_uint8 * 1024)()
    err = lambda: lib.hmx_last_error(h).decode()
    try:
        for call, msg in ((lambda: lib.hmx_init_cluster(h, None), "setup first"), (lambda: lib.hmx_kmeans_centers(h, buf), "setup first"),
                          (lambda: lib.hmx_cluster(h), "init_cluster first"), (lambda: lib.hmx_moe_correct_ridge(h), "init_cluster first"),
                          (lambda: lib.hmx_compute_objective(h), "init_cluster first"), (lambda: lib.hmx_push_update_order(h, i64), "setup first"),
                          (lambda: lib.hmx_restart(h), "setup first"), (lambda: lib.hmx_p2p_connect(h, 0, 2, u8), "hmx_p2p_export first"),
                          (lambda: lib.hmx_p2p_selftest(h), "hmx_p2p_connect first"), (lambda: lib.hmx_p2p_enable(h, 1), "hmx_p2p_connect first"),
                          (lambda: lib.hmx_comm_allreduce_host(h, buf, 1, 0), "hmx_comm_init first")):
            assert call() == 6 and msg in err(), err()
        for t in (0, 1):
            assert lib.hmx_check_convergence(h, t) < 0 and "not enough objective values" in err()
        assert lib.hmx_get_matrix(h, b"Z_corr", buf, 0, 0, 16) == -1
        assert lib.hmx_get(h, b"R", buf, 16) == -1 and lib.hmx_get(h, b"Lambda", buf, 16) == -1
        assert lib.hmx_get(h, b"N", buf, 16) == 1 and buf[0] == 0          # scalar fields of an empty object: zero, like new(harmony)'s
        assert lib.hmx_cluster(None) == 1 and lib.hmx_get(None, b"R", buf, 16) == -1 and lib.hmx_set_int(None, b"seed", 1) == 1
        assert lib.hmx_last_error(None) == b"null handle"
    finally:
        lib.hmx_destroy(h)
    lib.hmx_destroy(None)                                                       # harmless
