"""Every dispatch branch of the splat (csrc/splat.hip) through the C ABI, under guards and dirty scratch:
the cases of tests/splat_cases.py, whose mirror of launch_splat names the branches each case is for
(asserted on the CPU by tests/test_dispatch_mirrors.py, and again here).

Per case:
  - ecorr_splat_workspace_size, then ecorr_forward_interpolate or ecorr_grid_sample_values; the workspace
    has exactly the reported size between guards (gpu_guard.Workspace; zero bytes = NULL), the outputs
    (the splatted flow, or values and valid) lie between guard bands prefilled with a pattern no result
    has: the guards must be intact and every element written;
  - three runs, the workspace prefilled 0x00, 0xff and 0x7b: a count or key the kernel reads before
    writing it changes the result; the three outputs must be the same bits;
  - the result is the serial CPU oracle's bit for bit (oracle.same_bits; valid by equality);
  - the input is bitwise unchanged.
One line per case (pytest -s): `splat_dispatch: name [what] workspace N bytes`.
"""
import ctypes

import numpy as np
import pytest
import torch

import gpu_guard
import oracle
import splat_cases as sc

pytestmark = pytest.mark.gpu
WS_FILLS = (0x00, 0xff, 0x7b)


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _workspace_bytes(B, n, h, w, what):
    from eraft_amd import _lib
    nb = ctypes.c_int64(-1)
    _lib.check(_lib.lib().ecorr_splat_workspace_size(B, n, h, w, ctypes.byref(nb)), what)
    assert (nb.value > 0) == sc.workspace_needed(n), f"{what}: workspace of {nb.value} bytes"
    return nb.value


def _splat(flow, dev, B, n, h, w, fill, what):
    """One call on the device input (flow [B, 2, h, w] or points [3, n]) with the workspace prefilled
    `fill` -> (values as numpy [B, nz, h, w], valid as numpy uint8 [h, w] or None)."""
    from eraft_amd import _lib
    L = _lib.lib()
    nz = 2 if flow else 1
    ws = gpu_guard.Workspace(_workspace_bytes(B, n, h, w, what), fill)
    vbuf, values = gpu_guard.guarded(B * nz * h * w)
    st = _lib.stream_of(values)
    if flow:
        mbuf = None
        _lib.check(L.ecorr_forward_interpolate(dev.data_ptr(), B, h, w, values.data_ptr(), ws.ptr, st), what)
    else:
        mbuf, valid = gpu_guard.guarded_u8(h * w)
        _lib.check(L.ecorr_grid_sample_values(dev.data_ptr() if n else None, n, h, w, values.data_ptr(),
                                              valid.data_ptr(), ws.ptr, st), what)
    torch.cuda.synchronize()
    ws.check(f"{what}, workspace prefilled {fill:#04x}")
    got = gpu_guard.check_guarded(vbuf, f"{what}: values").reshape(B, nz, h, w)
    return got, None if mbuf is None else gpu_guard.check_guarded_u8(mbuf, f"{what}: valid").reshape(h, w)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_splat_dispatch_case(ea, name):
    c = sc.CASES[name]
    flow, B, n, h, w = c["mode"] == "flow", c["B"], c["n"], c["h"], c["w"]
    what = f"{name} [{sc.describe(name)}]"
    assert c["expect"] <= sc.tags(name), what
    print(f"splat_dispatch: {what} workspace {_workspace_bytes(B, n, h, w, what)} bytes")
    host = sc.inputs(name)
    dev = torch.from_numpy(host.copy()).cuda()
    assert dev.data_ptr() % 16 == 0   # the staging arms of splat_cases.staging assume it
    runs = [_splat(flow, dev, B, n, h, w, fill, what) for fill in WS_FILLS]
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), host.view(np.uint32)), f"{what}: the input changed"
    for fill, (v, m) in zip(WS_FILLS[1:], runs[1:]):
        assert np.array_equal(v.view(np.uint32), runs[0][0].view(np.uint32)), \
            f"{what}: values differ between workspaces prefilled 0x00 and {fill:#04x}"
        assert flow or np.array_equal(m, runs[0][1]), f"{what}: valid differs between workspaces prefilled 0x00 and {fill:#04x}"
    got, valid = runs[0]
    if flow:
        bad = gpu_guard.mismatch(got, oracle.forward_interpolate(host))
        assert bad is None, f"{what}: {bad}"
    else:
        ref_v, ref_m = oracle.grid_sample_values(host, h, w)
        bad = gpu_guard.mismatch(got, ref_v[None])
        assert bad is None, f"{what}: {bad}"
        assert set(np.unique(valid)) <= {0, 1} and np.array_equal(valid.astype(bool), ref_m[0]), f"{what}: valid"
        if n == 0:
            assert not got.any() and not valid.any()
    if "alone" in c:   # a batch stride of the workspace: item b equals item b splatted alone
        b = c["alone"]
        one = torch.from_numpy(host[b:b + 1].copy()).cuda()
        v1, _ = _splat(flow, one, 1, n, h, w, WS_FILLS[2], f"{what}, item {b} alone")
        bad = gpu_guard.mismatch(got[b:b + 1], v1)
        assert bad is None, f"{what}: item {b} of the batch differs from item {b} alone: {bad}"
