"""Every dispatch branch of the event -> voxel grid (csrc/voxel.hip) through the C ABI, under guards and
dirty scratch: the cases of tests/voxel_dispatch.py, whose mirror of launch_voxel / vtile_geom names
the pipeline each case takes (asserted on the CPU by tests/test_dispatch_mirrors.py, and again here).

Per case, with normalize 0 and 1:
  - ecorr_voxel_workspace_size, then ecorr_voxel_grid_dsec / ecorr_voxel_grid_mvsec; the workspace has
    exactly the reported size between guards (gpu_guard.Workspace), the grid lies between guard bands
    prefilled with a pattern no result has: the guards must be intact (norm_apply's tail included) and
    every cell written;
  - three runs, the workspace prefilled 0x00, 0xff and 0x7b: the pipelines zero little of it on the
    host (the key-range one its counts, the tiled one nothing), so a counter read before it is written
    changes the grid; the three grids must be the same bits, the normalized ones too;
  - normalize = 0: the serial CPU oracle's grid bit for bit; normalize = 1: within NORM_TOL of it;
  - MVSEC: the bad-index flag, zeroed by the test, stays 0.
One line per case (pytest -s): `voxel_dispatch: name [what] workspace N bytes`.
"""
import ctypes

import numpy as np
import pytest
import torch

import gpu_guard
import oracle
import voxel_dispatch as vd

pytestmark = pytest.mark.gpu
WS_FILLS = (0x00, 0xff, 0x7b)
NORM_TOL = 1e-6   # rtol and atol on the normalized grid (tests/test_voxel_gpu.py)


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _workspace_bytes(dsec, n, C, H, W, what):
    from eraft_amd import _lib
    nb = ctypes.c_int64(-1)
    _lib.check(_lib.lib().ecorr_voxel_workspace_size(int(dsec), n, C, H, W, ctypes.byref(nb)), what)
    assert nb.value > 0, what
    return nb.value


def _grid(dsec, dev, n, C, H, W, normalize, fill, what):
    """One call on the device events with the workspace prefilled `fill` -> the grid as numpy [C, H, W]."""
    from eraft_amd import _lib
    L = _lib.lib()
    what = f"{what}, normalize={normalize}, workspace prefilled {fill:#04x}"
    ws = gpu_guard.Workspace(_workspace_bytes(dsec, n, C, H, W, what), fill)
    gbuf, grid = gpu_guard.guarded(C * H * W)
    st = _lib.stream_of(grid)
    if dsec:
        p, t, x, y = dev
        _lib.check(L.ecorr_voxel_grid_dsec(p.data_ptr(), t.data_ptr(), x.data_ptr(), y.data_ptr(), n, C, H, W,
                                           normalize, grid.data_ptr(), ws.ptr, st), what)
    else:
        bad = torch.zeros((1,), dtype=torch.int32, device="cuda")
        _lib.check(L.ecorr_voxel_grid_mvsec(dev.data_ptr(), n, C, H, W, normalize, grid.data_ptr(), bad.data_ptr(),
                                            ws.ptr, st), what)
    torch.cuda.synchronize()
    ws.check(what)
    if not dsec:
        assert int(bad.item()) == 0, f"{what}: the bad-index flag was set"
    return gpu_guard.check_guarded(gbuf, f"{what}: grid").reshape(C, H, W)


@pytest.mark.parametrize("name", list(vd.CASES))
def test_voxel_dispatch_case(ea, name):
    dsec, n, C, H, W = vd.CASES[name]["shape"]
    what = f"{name} [{vd.describe(name)}]"
    assert vd.CASES[name]["expect"] <= vd.tags(name), what
    print(f"voxel_dispatch: {what} workspace {_workspace_bytes(dsec, n, C, H, W, what)} bytes")
    ev = vd.events(name)
    if dsec:
        dev = tuple(torch.from_numpy(v.copy()).cuda() for v in ev)
    else:
        dev = torch.from_numpy(ev.copy()).cuda()
    for normalize in (0, 1):
        grids = [_grid(dsec, dev, n, C, H, W, normalize, fill, what) for fill in WS_FILLS]
        for fill, g in zip(WS_FILLS[1:], grids[1:]):
            assert np.array_equal(g.view(np.uint32), grids[0].view(np.uint32)), \
                f"{what}: normalize={normalize}: the grid differs between workspaces prefilled 0x00 and {fill:#04x}"
        if dsec:
            ref = oracle.voxel_dsec(*ev, C, H, W, bool(normalize))
        else:
            ref, bad = oracle.voxel_mvsec(ev, C, H, W, bool(normalize))
            assert not bad
        if normalize:
            np.testing.assert_allclose(grids[0], ref, rtol=NORM_TOL, atol=NORM_TOL, err_msg=what)
        else:
            bad = gpu_guard.mismatch(grids[0][None], ref[None])
            assert bad is None, f"{what}: {bad}"
    for got, want in zip(dev if dsec else (dev,), ev if dsec else (ev,)):
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8)), f"{what}: the events changed"
