"""CPU-side checks of the backward's C ABI (ecorr_lookup_backward, ecorr_build_backward; ABI 17):
argument validation before any launch, and the store rule of DESIGN §3.1 for csrc/grad.hip."""
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


def test_abi_version_17(ea):
    from eraft_amd import _lib
    assert ea.lib().ecorr_abi_version() == 17 == _lib.ABI_VERSION
    assert "#define ECORR_ABI_VERSION 17" in open(os.path.join(ROOT, "include", "ecorr.h")).read()


def test_lookup_backward_validation(ea):
    from eraft_amd import _lib
    F = ea.lib().ecorr_lookup_backward   # (grad_out, coords, B, H, W, q_count, levels, radius, grad_pyramid, stream)
    assert F(None, 8, 1, 8, 8, 64, 3, 4, 8, None) == _lib.ECORR_EINVAL
    assert F(8, None, 1, 8, 8, 64, 3, 4, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 1, 8, 8, 64, 3, 4, None, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 0, 8, 8, 64, 3, 4, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 1, 8, 8, 65, 3, 4, 8, None) == _lib.ECORR_EINVAL    # q_count outside [1, H*W]
    assert F(8, 8, 1, 8, 8, 0, 3, 4, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 1, 8, 8, 64, 3, 33, 8, None) == _lib.ECORR_ERADIUS
    assert F(8, 8, 1, 8, 8, 64, 3, -1, 8, None) == _lib.ECORR_ERADIUS
    assert F(8, 8, 1, 8, 8, 64, 0, 4, 8, None) == _lib.ECORR_ELEVELS
    assert F(8, 8, 1, 8, 8, 64, 17, 4, 8, None) == _lib.ECORR_ELEVELS
    assert F(8, 8, 1, 4, 4, 16, 4, 4, 8, None) == _lib.ECORR_ESHAPE


def test_build_backward_validation(ea):
    from eraft_amd import _lib
    # (grad_pyramid, fmap1, fmap2, B, D, H, W, q_count, levels, grad_fmap1, grad_fmap2, stream)
    F = ea.lib().ecorr_build_backward
    assert F(None, 8, 8, 1, 256, 8, 8, 64, 3, 8, 8, None) == _lib.ECORR_EINVAL
    assert F(8, None, 8, 1, 256, 8, 8, 64, 3, 8, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, None, 1, 256, 8, 8, 64, 3, 8, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 8, 0, 256, 8, 8, 64, 3, 8, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 8, 1, 0, 8, 8, 64, 3, 8, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 8, 1, 256, 8, 8, 65, 3, 8, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 8, 1, 256, 8, 8, 0, 3, 8, 8, None) == _lib.ECORR_EINVAL
    assert F(8, 8, 8, 1, 256, 8, 8, 64, 0, 8, 8, None) == _lib.ECORR_ELEVELS
    assert F(8, 8, 8, 1, 256, 4, 4, 16, 4, 8, 8, None) == _lib.ECORR_ESHAPE


def test_grad_hip_store_rule():
    """grad.hip compiled for gfx950 has no wide buffer store whose soffset is an SGPR (the detector of
    tests/test_isa_store_hazard.py)."""
    from test_isa_store_hazard import _ins, scan
    from test_isa_waits import listing
    ins = _ins(listing("grad.hip"))
    assert any(l.startswith("v_mfma_f32_32x32x2") for l in ins), "the backward GEMM should run on the fp32 matrix cores"
    sgpr, hazards = scan(ins)
    assert not sgpr, f"grad.hip: wide buffer stores with an SGPR soffset: {sgpr[:3]}"
