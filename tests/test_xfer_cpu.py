"""The host threads of the host matrix seam (harmony_amd/csrc/hmx_xfer_pool.h) without a GPU: tests/cpp/xfer_pool_probe.cpp drives one XferPool
the way a transfer through the page-locked ring does -- one copy after the other on the same pool -- and compares every copy with memcpy's."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_probe = []


def xfer_probe():
    if not _probe:
        import tempfile
        so = os.path.join(tempfile.mkdtemp(prefix="xfer_pool_probe_"), "xfer_pool_probe.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread",
                               os.path.join(ROOT, "tests", "cpp", "xfer_pool_probe.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.probe_xfer_chunk.restype = C.c_longlong
        lib.probe_xfer_copy.argtypes = [C.c_int, C.c_longlong, C.c_int]
        lib.probe_xfer_copy.restype = C.c_int
        _probe.append(lib)
    return _probe[0]


@pytest.mark.parametrize("threads", [0, 3])
def test_pool_copy_reproduces_memcpy(threads):
    """below 4 * CHUNK the caller copies alone; from there on the helpers take chunks.  20 copies on one pool: every generation hands out
    its own chunks, none of the last one's"""
    lib = xfer_probe()
    chunk = lib.probe_xfer_chunk()
    assert chunk == 1 << 20
    for nbytes in (0, 1, 4097, 4 * chunk - 1, 4 * chunk, (4 * chunk + 1) | 1):
        assert lib.probe_xfer_copy(threads, nbytes, 20) == 0, (threads, nbytes)
