"""CPU-side checks of 16-bit fmaps in / 16-bit convc1 out in the C ABI (ecorr_build_split_pack_as,
ecorr_build_split_as, ecorr_conv1x1_relu_split_as, ecorr_lookup_conv1x1_relu_packed_as; added within
ABI 17): the symbols exist, the version is unchanged, the header declares the ECORR_ELEM_* codes and the
bitwise contracts, and argument validation returns before any launch (dummy non-null pointers, no
device): each entry gives its fp32 sibling's codes, plus ECORR_EINVAL for an unknown format after those."""
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

NEW = ("ecorr_build_split_pack_as", "ecorr_build_split_as", "ecorr_conv1x1_relu_split_as",
       "ecorr_lookup_conv1x1_relu_packed_as")
P = 256   # a dummy non-null pointer, 256-byte aligned (the workspace's alignment is validated)
BAD_FORMATS = (-1, 3, 16, 1 << 20)


@pytest.fixture(scope="module")
def ea():
    lib = os.path.join(ROOT, "e-raft_amd", "libecorr.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "e-raft_amd", "csrc")], check=True)
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def test_symbols_within_abi_17(ea):
    from eraft_amd import _lib
    L = ea.lib()
    assert L.ecorr_abi_version() == 17 == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ecorr.h")).read()
    assert "#define ECORR_ABI_VERSION 17" in header
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
        assert re.search(rf"^int {name}\(", header, re.M), name
    for name, alias, value in (("ECORR_ELEM_F32", "ECORR_OUT_F32", 0), ("ECORR_ELEM_F16", "ECORR_OUT_F16", 1),
                               ("ECORR_ELEM_BF16", "ECORR_OUT_BF16", 2)):
        assert re.search(rf"^#define {name} {alias}$", header, re.M), name
        assert re.search(rf"^#define {alias} {value}$", header, re.M), alias
        assert getattr(_lib, name) == value
    # the bitwise contracts
    assert "bitwise\n * those of ecorr_build_split_pack on the fmaps converted to fp32" in header
    assert "bitwise a cast of the fp32 entry's output" in header
    assert "rounded ONCE to nearest-even" in header
    import torch
    assert _lib.ELEM_FORMATS == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def test_pack_as_validation_before_launch(ea):
    from eraft_amd import _lib
    L = ea.lib()
    E = _lib.ECORR_EINVAL
    F32 = L.ecorr_build_split_pack      # (fmap1, fmap2, B, D, H, W, q_count, workspace, stream)
    AS = L.ecorr_build_split_pack_as    # (fmap1, fmap2, fmap_format, B, D, H, W, q_count, workspace, stream)
    bad = [((None, P), (1, 8, 8, 8, 64), P), ((P, None), (1, 8, 8, 8, 64), P), ((P, P), (1, 8, 8, 8, 64), None),
           ((P, P), (0, 8, 8, 8, 64), P), ((P, P), (1, 0, 8, 8, 64), P), ((P, P), (1, 8, 8, 8, 65), P),
           ((P, P), (1, 8, 8, 8, 0), P), ((P, P), (1, 8, 0, 8, 64), P), ((P, P), (65536, 8, 8, 8, 64), P),
           ((P, P), (1, 8, 8, 8, 64), P + 8)]                         # workspace not 256-byte aligned
    for fm, dims, ws in bad:
        want = F32(*fm, *dims, ws, None)
        assert want == E
        for fmt in (0, 1, 2) + BAD_FORMATS:
            assert AS(*fm, fmt, *dims, ws, None) == want, (fm, dims, ws, fmt)
    for fmt in BAD_FORMATS:   # an unknown format alone: after every other check, before the launch
        assert AS(P, P, fmt, 1, 8, 8, 8, 64, P, None) == E


def test_build_split_as_validation_before_launch(ea):
    from eraft_amd import _lib
    L = ea.lib()
    E = _lib.ECORR_EINVAL
    F32 = L.ecorr_build_split   # (fmap1, fmap2, B, D, H, W, q_count, levels, pyramid, workspace, stream)
    AS = L.ecorr_build_split_as   # (fmap1, fmap2, fmap_format, B, D, H, W, q_count, levels, pyramid, workspace, stream)
    bad = [((None, P), (1, 8, 8, 8, 64, 1), P, P, E), ((P, P), (1, 8, 8, 8, 64, 1), None, P, E),
           ((P, P), (1, 8, 8, 8, 64, 1), P, None, E), ((P, P), (1, 8, 8, 8, 65, 1), P, P, E),
           ((P, P), (1, 8, 8, 8, 64, 0), P, P, _lib.ECORR_ELEVELS), ((P, P), (1, 8, 8, 8, 64, 17), P, P, _lib.ECORR_ELEVELS),
           ((P, P), (1, 8, 4, 4, 16, 4), P, P, _lib.ECORR_ESHAPE),
           ((P, P), (1, 8, 8, 8, 64, 1), P + 8, P, E)]                # pyramid not 16-byte aligned
    for fm, dims, pyr, ws, code in bad:
        assert F32(*fm, *dims, pyr, ws, None) == code
        for fmt in (0, 1, 2) + BAD_FORMATS:
            assert AS(*fm, fmt, *dims, pyr, ws, None) == code, (fm, dims, fmt)
    for fmt in BAD_FORMATS:
        assert AS(P, P, fmt, 1, 8, 8, 8, 64, 1, P, P, None) == E


def test_conv_split_as_validation_before_launch(ea):
    from eraft_amd import _lib
    L = ea.lib()
    E = _lib.ECORR_EINVAL
    F32 = L.ecorr_conv1x1_relu_split      # (in, B, C, Q, qmax, G, packed, bias, O, out, stream)
    AS = L.ecorr_conv1x1_relu_split_as    # (in, B, C, Q, qmax, G, packed, bias, O, out_format, out, stream)
    Q2 = 0x7fffffff // (4 * (64 + 256)) + 1   # the fp32 store offsets pass 31 bits, the 16-bit ones do not
    bad = [(None, 1, 81, 64, None, 0, P, None, 64, 2 * P), (P, 1, 81, 64, None, 0, None, None, 64, 2 * P),
           (P, 1, 81, 64, None, 0, P, None, 64, None), (P, 0, 81, 64, None, 0, P, None, 64, 2 * P),
           (P, 1, 0, 64, None, 0, P, None, 64, 2 * P), (P, 1, 81, 0, None, 0, P, None, 64, 2 * P),
           (P, 1, 81, 64, None, 0, P, None, 0, 2 * P), (P, 65536, 81, 64, None, 0, P, None, 64, 2 * P),
           (P, 1, 81, 64, P, 0, P, None, 64, 2 * P),                  # qmax without G
           (P, 1, 81, 64, None, 0, P, None, 64, P),                   # in == out
           (P, 1, 1 << 22, 1 << 10, None, 0, P, None, 64, 2 * P)]     # the input offsets pass 31 bits
    for a in bad:
        assert F32(*a, None) == E
        for fmt in (0, 1, 2) + BAD_FORMATS:
            assert AS(*a[:9], fmt, a[9], None) == E, (a, fmt)
    # the 32-bit offset guard of the stores uses the element size
    a = (P, 1, 1, Q2, None, 0, P, None, 64)
    assert F32(*a, 2 * P, None) == E and AS(*a, 0, 2 * P, None) == E
    for fmt in BAD_FORMATS:   # (an unknown format has no element size: the fp32 guard, then its own refusal)
        assert AS(*a, fmt, 2 * P, None) == E
        assert AS(P, 1, 81, 64, None, 0, P, None, 64, fmt, 2 * P, None) == E


def test_fused_as_validation_before_launch(ea):
    from eraft_amd import _lib
    L = ea.lib()
    E = _lib.ECORR_EINVAL
    # (pyramid, coords, B, H, W, q_count, levels, radius, packed, bias, O, out, stream)
    F32 = L.ecorr_lookup_conv1x1_relu_packed
    AS = L.ecorr_lookup_conv1x1_relu_packed_as   # ... O, out_format, out, stream)
    bad = [((None, P, 1, 8, 8, 64, 1, 4, P, None, 64), P, E), ((P, None, 1, 8, 8, 64, 1, 4, P, None, 64), P, E),
           ((P, P, 1, 8, 8, 64, 1, 4, None, None, 64), P, E), ((P, P, 1, 8, 8, 64, 1, 4, P, None, 64), None, E),
           ((P, P, 0, 8, 8, 64, 1, 4, P, None, 64), P, E), ((P, P, 1, 8, 8, 65, 1, 4, P, None, 64), P, E),
           ((P, P, 1, 8, 8, 64, 1, 3, P, None, 64), P, _lib.ECORR_ERADIUS),
           ((P, P, 1, 8, 8, 64, 1, 33, P, None, 64), P, _lib.ECORR_ERADIUS),
           ((P, P, 1, 64, 64, 4096, 5, 4, P, None, 64), P, _lib.ECORR_ELEVELS),
           ((P, P, 1, 8, 8, 64, 0, 4, P, None, 64), P, _lib.ECORR_ELEVELS),
           ((P, P, 1, 4, 4, 16, 4, 4, P, None, 64), P, _lib.ECORR_ESHAPE),
           ((P, P, 1, 8, 8, 64, 1, 4, P, None, 96), P, E), ((P, P, 1, 8, 8, 64, 1, 4, P, None, 0), P, E)]
    for a, out, code in bad:
        assert F32(*a, out, None) == code, a
        for fmt in (0, 1, 2) + BAD_FORMATS:
            assert AS(*a, fmt, out, None) == code, (a, fmt)
    for fmt in BAD_FORMATS:
        assert AS(P, P, 1, 8, 8, 64, 1, 4, P, None, 64, fmt, P, None) == E


def test_python_interface_defaults():
    """fmap_dtype on CorrBlock and out_dtype on lookup_conv1x1_relu default to None: every existing call
    keeps its path; the dtype arguments are validated like out_dtype."""
    import torch
    import eraft_amd
    from eraft_amd import _lib, rowshard
    p = inspect.signature(eraft_amd.CorrBlock.__init__).parameters
    assert p["fmap_dtype"].default is None and p["fmap_dtype"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["differentiable"].default is False
    assert inspect.signature(eraft_amd.CorrBlock.lookup_conv1x1_relu).parameters["out_dtype"].default is None
    assert "fmap_dtype" not in inspect.signature(rowshard.RowShardedCorrBlock.__init__).parameters   # fp32 at both ends
    assert _lib.fmap_dtype_of(None) is torch.float32
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert _lib.fmap_dtype_of(dt) is dt
    for bad in (torch.float64, torch.int16, "float16", 1):
        with pytest.raises(TypeError, match="fmap_dtype"):
            _lib.fmap_dtype_of(bad)
