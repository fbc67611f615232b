"""End-to-end parity with the HIP motion encoder: ERAFT(hip_motion_encoder=True) against the reference goldens
(tests/golden/e2e_*.npz, PRNG weights from tests/e2e_weights.py), the bar of tests/test_e2e_gpu.py: final flow
within 1e-3 px EPE of the reference, low-resolution and 8x-upsampled -- alone, and with the fused lookup + convc1,
the HIP upsampling and the HIP SepConvGRU on the same path (then the whole update block in front of the flow and
mask heads is native).  The EPE against the same flags without hip_motion_encoder on the same GPU (the encoder's
own share of the difference) is printed; no bar beyond the two above is set on it.
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


def _tf32_off():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False


@pytest.mark.parametrize("native", [False, True], ids=["encoder", "encoder+convc1+upsample+gru"])
@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_e2e_hip_motion_encoder(path, native):
    _tf32_off()
    z = np.load(path)
    flags = {"fuse_motion_corr": True, "hip_upsample": True, "hip_gru": True} if native else {}
    low, up = _run(z, hip_motion_encoder=True, **flags)
    base_low, base_up = _run(z, **flags)
    e_low, e_up = epe(low, z["flow_low"]), epe(up, z["flow_up"])
    print(f"{os.path.basename(path)} hip_motion_encoder{' all-native' if native else ''}: EPE vs reference low "
          f"{e_low:.3g} px, up {e_up:.3g} px | vs hip_motion_encoder=False (same GPU) low {epe(low, base_low):.3g} "
          f"up {epe(up, base_up):.3g} | hip_motion_encoder=False vs reference low "
          f"{epe(base_low, z['flow_low']):.3g} up {epe(base_up, z['flow_up']):.3g}")
    assert np.isfinite(low).all() and np.isfinite(up).all()
    assert e_low <= EPE_TOL
    assert e_up <= EPE_TOL


def test_hip_motion_encoder_with_alternate_corr():
    """The flag composes with the volume-free lookup (torch's convc1 in front of the kernels), within the bar."""
    _tf32_off()
    z = np.load(os.path.join(GOLDEN, "e2e_small_standard.npz"))
    low, up = _run(z, hip_motion_encoder=True, alternate_corr=True)
    e_low, e_up = epe(low, z["flow_low"]), epe(up, z["flow_up"])
    print(f"hip_motion_encoder + alternate_corr: EPE vs reference low {e_low:.3g} px, up {e_up:.3g} px")
    assert e_low <= EPE_TOL
    assert e_up <= EPE_TOL


def test_constructor_refusals():
    import eraft_amd.network as nw
    cfg = {"subtype": "standard"}
    for kw in ({"mixed_precision": True}, {"differentiable_corr": True}, {"train_motion_corr": True},
               {"train_alternate_corr": True}, {"train_gru": True}):
        with pytest.raises(ValueError, match="hip_motion_encoder"):
            nw.ERAFT(cfg, 3, hip_motion_encoder=True, **kw)
