"""CPU-side checks of the convc1 backward in the C ABI (ecorr_conv1x1_relu_backward,
ecorr_conv1x1_relu_backward_workspace_size; added within ABI 17): the symbols exist, the version is
unchanged, the workspace size is positive and monotone, and argument validation returns before any
launch (dummy non-null pointers, no device)."""
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


def _size(ea, B, C, Q, O):
    n = ctypes.c_int64(-7)
    st = ea.lib().ecorr_conv1x1_relu_backward_workspace_size(B, C, Q, O, ctypes.byref(n))
    return st, n.value


def test_symbols_within_abi_17(ea):
    from eraft_amd import _lib
    L = ea.lib()
    assert L.ecorr_abi_version() == 17 == _lib.ABI_VERSION
    for name in ("ecorr_conv1x1_relu_backward_workspace_size", "ecorr_conv1x1_relu_backward"):
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
    header = open(os.path.join(ROOT, "include", "ecorr.h")).read()
    assert "#define ECORR_ABI_VERSION 17" in header
    assert "int ecorr_conv1x1_relu_backward_workspace_size(int B, int C, int Q, int O, int64_t* bytes);" in header
    assert "int ecorr_conv1x1_relu_backward(const float* grad_out, const float* out, const float* in, " \
           "const void* packed_t," in header
    assert "Replaces: autograd of update.py:67,74" in header


def test_workspace_size(ea):
    from eraft_amd import _lib
    EINVAL = _lib.ECORR_EINVAL
    assert ea.lib().ecorr_conv1x1_relu_backward_workspace_size(1, 324, 64, 256, None) == EINVAL   # NULL bytes
    for g in [(0, 324, 64, 256), (65536, 324, 64, 256), (-1, 324, 64, 256), (1, 0, 64, 256), (1, 324, 0, 256),
              (1, 324, 64, 0), (1, -3, 64, 256)]:
        assert _size(ea, *g)[0] == EINVAL, g
    for g in [(1, 1, 1, 1), (65535, 1, 1, 1), (16, 324, 4800, 256), (2, 324, 2500, 256), (1, 81, 70, 300)]:
        st, n = _size(ea, *g)
        assert st == _lib.ECORR_OK and n > 0, g
    # it holds at least the masked gradient and one slab of weight partials per batch item
    assert _size(ea, 2, 324, 2500, 256)[1] >= 4 * (2 * 256 * 2500 + 2 * 3 * 256 * 324)
    # monotone in each of B, Q, O, C
    for axis, values in ((0, (1, 2, 3, 16, 17, 1000)), (1, (1, 20, 81, 243, 324, 325, 1000)),
                         (2, (1, 63, 64, 65, 1024, 1025, 2500, 4800, 5000)), (3, (1, 20, 64, 96, 256, 257, 300))):
        sizes = []
        for v in values:
            g = [2, 324, 2500, 256]
            g[axis] = v
            st, n = _size(ea, *g)
            assert st == _lib.ECORR_OK
            sizes.append(n)
        assert sizes == sorted(sizes), (axis, sizes)


def test_backward_validation(ea):
    from eraft_amd import _lib
    EINVAL = _lib.ECORR_EINVAL
    # (grad_out, out, in, packed_t, B, C, Q, O, grad_in, grad_weight, grad_bias, workspace, stream)
    F = ea.lib().ecorr_conv1x1_relu_backward
    g = (1, 324, 64, 256)
    assert F(None, 8, 8, 8, *g, 16, 24, 32, 40, None) == EINVAL         # grad_out
    assert F(8, None, 8, 8, *g, 16, 24, 32, 40, None) == EINVAL         # out
    assert F(8, 8, 8, 8, *g, 16, 24, 32, None, None) == EINVAL          # workspace, always required
    assert F(8, 8, 8, 8, *g, None, None, 32, None, None) == EINVAL      # ... also for grad_bias alone
    assert F(8, 8, 8, 8, *g, None, None, None, 40, None) == EINVAL      # all three outputs NULL
    assert F(8, 8, None, 8, *g, None, 24, None, 40, None) == EINVAL     # in: needed for grad_weight
    assert F(8, 8, 8, None, *g, 16, None, None, 40, None) == EINVAL     # packed_t: needed for grad_in
    # grad_in must not be grad_out, out or in
    assert F(16, 8, 48, 8, *g, 16, 24, 32, 40, None) == EINVAL
    assert F(8, 16, 48, 8, *g, 16, 24, 32, 40, None) == EINVAL
    assert F(8, 48, 16, 8, *g, 16, 24, 32, 40, None) == EINVAL
    # geometry: the same status as the size query
    big_q = 1 << 22   # (2 O + 64) Q 4 bytes pass 2^31: the conv kernel's offset limit with C and O swapped
    for geo in [(0, 324, 64, 256), (65536, 324, 64, 256), (1, 0, 64, 256), (1, 324, 0, 256), (1, 324, 64, 0),
                (1, 324, big_q, 256), (1, 20, 1 << 20, 1 << 10), (1, 1 << 10, 1 << 20, 20)]:
        st = _size(ea, *geo)[0]
        assert st == EINVAL, geo
        assert F(8, 8, 8, 8, *geo, 16, 24, 32, 40, None) == st, geo
    # C and O swapped: (2 O + 64) Q 4 < 2^31 binds on O, (C + 256 ceil(C / 256)) Q 4 < 2^31 on C
    assert _size(ea, 1, 20, 1 << 19, 1 << 9)[0] == EINVAL      # 1088 Q 4 > 2^31
    assert _size(ea, 1, 20, 1 << 19, (1 << 9) - 40)[0] == _lib.ECORR_OK
    assert _size(ea, 1, 1 << 9, 1 << 19, 20)[0] == EINVAL      # 1024 Q 4 = 2^31
    assert _size(ea, 1, (1 << 9) - 40, 1 << 19, 20)[0] == _lib.ECORR_OK
