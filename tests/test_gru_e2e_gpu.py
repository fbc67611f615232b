"""End-to-end parity with the HIP SepConvGRU: ERAFT(hip_gru=True) against the reference goldens
(tests/golden/e2e_*.npz, PRNG weights from tests/e2e_weights.py), the bar of tests/test_e2e_gpu.py: final flow
within 1e-3 px EPE of the reference, low-resolution and 8x-upsampled -- alone, and with the fused lookup +
convc1 and the HIP upsampling on the same path.  The EPE of hip_gru=True against hip_gru=False on the same
GPU (the GRU's own share of the difference) is printed; no bar beyond the two above is set on it.
"""
import glob
import os

import numpy as np
import pytest
import torch

import prng
from conftest import GOLDEN
from e2e_weights import make_state_dict

pytestmark = pytest.mark.gpu

CASES = sorted(glob.glob(os.path.join(GOLDEN, "e2e_*.npz")))
EPE_TOL = 1e-3


def epe(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.mean(np.sqrt(np.sum(d * d, axis=1))))


def _run(z, **flags):
    import eraft_amd.network as nw
    H, W, bins, seed = int(z["H"]), int(z["W"]), int(z["bins"]), int(z["seed"])
    net = nw.ERAFT({"subtype": str(z["subtype"])}, n_first_channels=bins, **flags)
    net.load_state_dict(make_state_dict(net.state_dict()))
    net = net.eval().cuda()
    im1 = torch.from_numpy(prng.normal(seed, (1, bins, H, W))).cuda()
    im2 = torch.from_numpy(prng.normal(seed + 1, (1, bins, H, W))).cuda()
    flow_init = torch.from_numpy(z["flow_init"]).cuda() if bool(z["warm"]) else None
    with torch.no_grad():
        low, ups = net(im1, im2, iters=12, flow_init=flow_init)
    st = int(z["up_stride"])
    return low.cpu().numpy(), ups[-1].cpu().numpy()[:, :, ::st, ::st]


@pytest.mark.parametrize("native", [False, True], ids=["gru", "gru+convc1+upsample"])
@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_e2e_hip_gru(path, native):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    z = np.load(path)
    flags = {"fuse_motion_corr": True, "hip_upsample": True} if native else {}
    low, up = _run(z, hip_gru=True, **flags)
    base_low, base_up = _run(z, **flags)
    e_low, e_up = epe(low, z["flow_low"]), epe(up, z["flow_up"])
    print(f"{os.path.basename(path)} hip_gru{' all-native' if native else ''}: EPE vs reference low {e_low:.3g} px, "
          f"up {e_up:.3g} px | vs hip_gru=False (same GPU) low {epe(low, base_low):.3g} up {epe(up, base_up):.3g} | "
          f"hip_gru=False vs reference low {epe(base_low, z['flow_low']):.3g} up {epe(base_up, z['flow_up']):.3g}")
    assert np.isfinite(low).all() and np.isfinite(up).all()
    assert e_low <= EPE_TOL
    assert e_up <= EPE_TOL


def test_constructor_refusals():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd.network as nw
    cfg = {"subtype": "standard"}
    for kw in ({"mixed_precision": True}, {"differentiable_corr": True}, {"train_motion_corr": True},
               {"train_alternate_corr": True}):
        with pytest.raises(ValueError, match="hip_gru"):
            nw.ERAFT(cfg, 3, hip_gru=True, **kw)
    for kw in ({}, {"fuse_motion_corr": True}, {"hip_upsample": True}, {"alternate_corr": True}):
        assert nw.ERAFT(cfg, 3, hip_gru=True, **kw).update_block.hip_gru


def test_hip_gru_with_alternate_corr():
    """The flag composes with the volume-free lookup: the same flow as alternate_corr alone, within the bar."""
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    z = np.load(os.path.join(GOLDEN, "e2e_small_standard.npz"))
    low, up = _run(z, hip_gru=True, alternate_corr=True)
    e_low, e_up = epe(low, z["flow_low"]), epe(up, z["flow_up"])
    print(f"hip_gru + alternate_corr: EPE vs reference low {e_low:.3g} px, up {e_up:.3g} px")
    assert e_low <= EPE_TOL
    assert e_up <= EPE_TOL
