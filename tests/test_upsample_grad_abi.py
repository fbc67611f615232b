"""CPU-side checks of the convex upsampling's backward in the C ABI (ecorr_upsample_flow_backward,
ecorr_upsample_backward_workspace_size; added within ABI 17): the symbols exist, the version is
unchanged, and argument validation returns before any launch (dummy non-null pointers, no device)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def ea():
    lib = os.path.join(ROOT, "e-raft_amd", "libecorr.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "e-raft_amd", "csrc")], check=True)
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _size(ea, N, H, W):
    from eraft_amd import _lib
    n = ctypes.c_int64(-7)
    st = ea.lib().ecorr_upsample_backward_workspace_size(N, H, W, ctypes.byref(n))
    return st, n.value


def test_symbols_within_abi_17(ea):
    from eraft_amd import _lib
    L = ea.lib()
    assert L.ecorr_abi_version() == 17 == _lib.ABI_VERSION
    for name in ("ecorr_upsample_backward_workspace_size", "ecorr_upsample_flow_backward"):
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
    header = open(os.path.join(ROOT, "include", "ecorr.h")).read()
    assert "#define ECORR_ABI_VERSION 17" in header
    assert "int ecorr_upsample_backward_workspace_size(int N, int H, int W, int64_t* bytes);" in header
    assert "int ecorr_upsample_flow_backward(" in header
    assert "Replaces: autograd of eraft.py:74-85" in header


def test_workspace_size(ea):
    from eraft_amd import _lib
    EINVAL = _lib.ECORR_EINVAL
    assert ea.lib().ecorr_upsample_backward_workspace_size(1, 4, 4, None) == EINVAL   # NULL bytes
    for N, H, W in [(0, 4, 4), (65536, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, 8193, 8192), (1, 1 << 26, 2)]:
        assert _size(ea, N, H, W)[0] == EINVAL, (N, H, W)
    # the geometry limits themselves are accepted
    for N, H, W in [(1, 1, 1), (65535, 1, 1), (1, 8192, 8192), (1, 1, 1 << 26), (65535, 8192, 8192)]:
        st, n = _size(ea, N, H, W)
        assert st == _lib.ECORR_OK and n > 0, (N, H, W)
    # monotone in N and in H * W
    sizes = [_size(ea, N, 60, 80)[1] for N in (1, 2, 3, 4, 16, 17, 1000)]
    assert sizes == sorted(sizes)
    sizes = [_size(ea, 3, H, W)[1] for H, W in [(1, 1), (6, 1), (1, 7), (3, 5), (17, 20), (60, 80), (61, 80), (480, 640)]]
    assert sizes == sorted(sizes)


def test_backward_validation(ea):
    from eraft_amd import _lib
    EINVAL = _lib.ECORR_EINVAL
    # (grad_out, flow, mask, N, H, W, grad_flow, grad_mask, workspace, stream)
    F = ea.lib().ecorr_upsample_flow_backward
    assert F(None, 8, 8, 1, 4, 4, 8, 8, 8, None) == EINVAL
    assert F(16, None, 8, 1, 4, 4, 8, 8, 8, None) == EINVAL
    assert F(16, 8, None, 1, 4, 4, 8, 8, 8, None) == EINVAL
    assert F(16, 8, 8, 1, 4, 4, None, None, 8, None) == EINVAL      # both gradients NULL
    assert F(16, 8, 8, 0, 4, 4, 8, 8, 8, None) == EINVAL
    assert F(16, 8, 8, 65536, 4, 4, 8, 8, 8, None) == EINVAL
    assert F(16, 8, 8, 1, 0, 4, 8, 8, 8, None) == EINVAL
    assert F(16, 8, 8, 1, 4, 0, 8, 8, 8, None) == EINVAL
    assert F(16, 8, 8, 1, 8193, 8192, 8, 8, 8, None) == EINVAL      # H * W > 2^26
    # NULL workspace where the size query is positive, whichever gradients are asked for
    assert _size(ea, 1, 4, 4)[1] > 0
    assert F(16, 8, 8, 1, 4, 4, 8, 8, None, None) == EINVAL
    assert F(16, 8, 8, 1, 4, 4, 8, None, None, None) == EINVAL
    assert F(16, 8, 8, 1, 4, 4, None, 8, None, None) == EINVAL
    # the same codes as the forward for the same geometry
    U = ea.lib().ecorr_upsample_flow   # (flow, mask, N, H, W, out, stream)
    for N, H, W in [(0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 8193, 8192)]:
        assert U(8, 8, N, H, W, 16, None) == F(16, 8, 8, N, H, W, 8, 8, 8, None) == EINVAL
