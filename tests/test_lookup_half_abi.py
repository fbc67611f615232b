"""CPU-side checks of the 16-bit lookup output in the C ABI (ecorr_lookup_as; added within ABI 17): the
symbol exists, the version is unchanged, the header declares the three element formats and the
rounding contract, and argument validation returns before any launch (dummy non-null pointers, no
device): ecorr_lookup's codes, plus ECORR_EINVAL for an unknown format."""
import os
import re
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


def test_symbol_within_abi_17(ea):
    from eraft_amd import _lib
    L = ea.lib()
    assert L.ecorr_abi_version() == 17 == _lib.ABI_VERSION
    assert "ecorr_lookup_as" in _lib.SYMBOLS
    assert L.ecorr_lookup_as.argtypes == _lib.SYMBOLS["ecorr_lookup_as"][1]
    header = open(os.path.join(ROOT, "include", "ecorr.h")).read()
    assert "#define ECORR_ABI_VERSION 17" in header
    for name, value in (("ECORR_OUT_F32", 0), ("ECORR_OUT_F16", 1), ("ECORR_OUT_BF16", 2)):
        assert re.search(rf"^#define {name} {value}$", header, re.M), name
        assert getattr(_lib, name) == value
    assert "int ecorr_lookup_as(const float* pyramid, const float* coords, int B, int H, int W, int q_count," in header
    assert "int levels, int radius, int out_format, void* out, void* stream);" in header
    assert "rounded ONCE to nearest-even" in header   # the rounding contract


def test_out_formats_per_dtype(ea):
    import torch
    from eraft_amd import _lib
    assert _lib.OUT_FORMATS == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    assert _lib.lookup_out_dtype(None) is torch.float32
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert _lib.lookup_out_dtype(dt) is dt
    for bad in (torch.float64, torch.int16, "float16", 1):
        with pytest.raises(TypeError, match="out_dtype"):
            _lib.lookup_out_dtype(bad)


def test_validation_before_launch(ea):
    from eraft_amd import _lib
    F = ea.lib().ecorr_lookup_as   # (pyramid, coords, B, H, W, q_count, levels, radius, out_format, out, stream)
    E = _lib.ECORR_EINVAL
    for fmt in (0, 1, 2):   # ecorr_lookup's validation and codes, for every format
        assert F(None, 8, 1, 8, 8, 64, 1, 4, fmt, 8, None) == E
        assert F(8, None, 1, 8, 8, 64, 1, 4, fmt, 8, None) == E
        assert F(8, 8, 1, 8, 8, 64, 1, 4, fmt, None, None) == E
        assert F(8, 8, 0, 8, 8, 64, 1, 4, fmt, 8, None) == E
        assert F(8, 8, 1, 8, 8, 65, 1, 4, fmt, 8, None) == E          # q_count outside [1, H*W]
        assert F(8, 8, 1, 8, 8, 64, 4, 33, fmt, 8, None) == _lib.ECORR_ERADIUS
        assert F(8, 8, 1, 8, 8, 64, 0, 4, fmt, 8, None) == _lib.ECORR_ELEVELS
        assert F(8, 8, 1, 4, 4, 16, 4, 4, fmt, 8, None) == _lib.ECORR_ESHAPE
        assert F(8, 8, 1, 3, 715827882, 1, 1, 4, fmt, 8, None) == E     # level-0 image past 31 bits
    for fmt in (-1, 3, 16, 1 << 20):   # an unknown format, after ecorr_lookup's own checks
        assert F(8, 8, 1, 8, 8, 64, 1, 4, fmt, 8, None) == E
        assert F(8, 8, 1, 8, 8, 64, 4, 33, fmt, 8, None) == _lib.ECORR_ERADIUS
    with pytest.raises(ValueError):
        _lib.check(E, "lookup")


def test_python_interface_signatures():
    """out_dtype on CorrBlock.__call__ and RowShardedCorrBlock.__call__; the ERAFT switches and
    their defaults (every existing call keeps its path)."""
    import inspect
    import torch
    import eraft_amd
    from eraft_amd import network, rowshard
    assert inspect.signature(eraft_amd.CorrBlock.__call__).parameters["out_dtype"].default is None
    assert inspect.signature(rowshard.RowShardedCorrBlock.__call__).parameters["out_dtype"].default is None
    p = inspect.signature(network.ERAFT.__init__).parameters
    assert p["mixed_precision"].default is False
    assert p["amp_dtype"].default is torch.float16
    assert p["_native_half_lookup"].default is True
    net = network.ERAFT({"subtype": "standard"}, n_first_channels=3)
    assert not net.mixed_precision
    with pytest.raises(TypeError, match="amp_dtype"):
        network.ERAFT({"subtype": "standard"}, n_first_channels=3, mixed_precision=True, amp_dtype=torch.float32)


def test_rowsharded_block_refuses_out_dtype():
    """RowShardedCorrBlock keeps fp32 lookups: a 16-bit out_dtype raises before anything else is looked
    at, another dtype is a TypeError as for CorrBlock, None / float32 go on to the fp32 call."""
    import torch
    from eraft_amd.rowshard import RowShardedCorrBlock
    blk = RowShardedCorrBlock.__new__(RowShardedCorrBlock)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="out_dtype"):
            blk(None, out_dtype=dt)
    with pytest.raises(TypeError, match="out_dtype"):
        blk(None, out_dtype=torch.float64)
    for dt in (None, torch.float32):   # past the dtype check: the bare object has no shape yet
        with pytest.raises(AttributeError):
            blk(None, out_dtype=dt)
