"""CPU-side checks of the alignment contract of the convex upsampling in the C ABI (include/ecorr.h):
`out` of ecorr_upsample_flow and `grad_out` of ecorr_upsample_flow_backward are accessed as 16-byte
vectors, so a misaligned one is ECORR_EINVAL before any launch.  Dummy non-null pointers, no device:
no call here gets past validation, so an aligned address shows only in that the geometry still
decides (a call with everything valid would launch on the dummy pointers)."""
import os
import subprocess

import pytest

from conftest import ROOT

ALIGNED = (16, 32)
MISALIGNED = (4, 8, 20)
BAD_GEOMETRY = [(0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 8193, 8192)]


@pytest.fixture(scope="module")
def ea():
    lib = os.path.join(ROOT, "e-raft_amd", "libecorr.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "e-raft_amd", "csrc")], check=True)
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def test_header_states_the_alignment(ea):
    from eraft_amd import _lib
    assert ea.lib().ecorr_abi_version() == 17 == _lib.ABI_VERSION
    header = " ".join(open(os.path.join(ROOT, "include", "ecorr.h")).read().split())
    assert "#define ECORR_ABI_VERSION 17" in header
    assert "out must be 16-byte aligned" in header
    assert "grad_out must be 16-byte aligned" in header
    assert "A misaligned out is ECORR_EINVAL" in header and "a misaligned grad_out is ECORR_EINVAL" in header


def test_forward_out_alignment(ea):
    from eraft_amd import _lib
    U = ea.lib().ecorr_upsample_flow   # (flow, mask, N, H, W, out, stream)
    for out in MISALIGNED:
        for N, H, W in [(1, 4, 4), (1, 1, 1), (2, 5, 53)]:   # everything else valid
            assert U(16, 16, N, H, W, out, None) == _lib.ECORR_EINVAL, (out, N, H, W)
        assert U(4, 4, 1, 4, 4, out, None) == _lib.ECORR_EINVAL   # flow and mask need no more than a float's
    for out in ALIGNED:   # aligned: the geometry still decides
        for N, H, W in BAD_GEOMETRY:
            assert U(16, 16, N, H, W, out, None) == _lib.ECORR_EINVAL, (out, N, H, W)
        assert U(None, 16, 1, 4, 4, out, None) == _lib.ECORR_EINVAL
        assert U(16, None, 1, 4, 4, out, None) == _lib.ECORR_EINVAL
    assert U(16, 16, 1, 4, 4, None, None) == _lib.ECORR_EINVAL


def test_backward_grad_out_alignment(ea):
    from eraft_amd import _lib
    F = ea.lib().ecorr_upsample_flow_backward   # (grad_out, flow, mask, N, H, W, grad_flow, grad_mask, workspace, stream)
    for go in MISALIGNED:
        for N, H, W in [(1, 4, 4), (1, 1, 1), (2, 5, 53)]:
            for gf, gm in ((16, 16), (16, None), (None, 16)):   # whichever gradients are asked for
                assert F(go, 16, 16, N, H, W, gf, gm, 16, None) == _lib.ECORR_EINVAL, (go, N, H, W, gf, gm)
        # the other buffers are accessed by element: 4-byte addresses for them do not change the answer
        assert F(go, 4, 4, 1, 4, 4, 4, 4, 4, None) == _lib.ECORR_EINVAL
    for go in ALIGNED:
        for N, H, W in BAD_GEOMETRY:
            assert F(go, 16, 16, N, H, W, 16, 16, 16, None) == _lib.ECORR_EINVAL, (go, N, H, W)
        assert F(go, 16, 16, 1, 4, 4, None, None, 16, None) == _lib.ECORR_EINVAL
        assert F(go, 16, 16, 1, 4, 4, 16, 16, None, None) == _lib.ECORR_EINVAL
    assert F(None, 16, 16, 1, 4, 4, 16, 16, 16, None) == _lib.ECORR_EINVAL
