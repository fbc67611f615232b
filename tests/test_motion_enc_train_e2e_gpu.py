"""Training E-RAFT through the HIP motion encoder: ERAFT(train_motion_encoder=True) on the GPU.

Set-up of tests/test_gru_train_e2e_gpu.py: image 1 x 15 x 128 x 160, iters = 3, train mode with frozen BN, loss = sum
of mean |prediction|, tests/e2e_weights.py weights.  Per flag set three arms: train_motion_encoder=True, the stock
fp32 encoder (MIOpen + autograd) with the same other flags, and an encoder evaluated in fp64 on the CPU inside the
network (tensors carried over and back).  Bar: the pooled relative distance of ours to the fp64 arm over all
parameters <= 4 x the stock fp32 arm's -- two independent fp32 roundings of the same sums amplified by the same
network, the margin of test_gru_train_e2e_gpu.  Flag sets: train_motion_corr + train_gru + hip_upsample (native at
both ends, in the GRU and now in between), and differentiable_corr alone (torch's convc1 in front, the stock GRU
behind).  Under no_grad the predictions are bitwise hip_motion_encoder=True's, and the e2e goldens hold within the
1e-3 px EPE bar of tests/test_e2e_gpu.py.
"""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = sorted(glob.glob(os.path.join(GOLDEN, "e2e_*.npz")))
EPE_TOL = 1e-3


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return eraft_amd


def _enc64_cls():
    import eraft_amd.network as nw

    class Enc64(nw.BasicMotionEncoder):
        """The same parameters (fp32, on the device), the arithmetic in fp64 on the CPU."""

        def forward(self, flow, corr, corr_is_convc1=False):
            def conv(c, t):
                return F.conv2d(t, c.weight.double().cpu(), c.bias.double().cpu(), padding=c.padding)
            flow64, corr64 = flow.double().cpu(), corr.double().cpu()
            c = F.relu(conv(self.convc2, corr64 if corr_is_convc1 else F.relu(conv(self.convc1, corr64))))
            f = F.relu(conv(self.convf2, F.relu(conv(self.convf1, flow64))))
            out = F.relu(conv(self.conv, torch.cat([c, f], dim=1)))
            return torch.cat([out, flow64], dim=1).to(flow.device).float()

    return Enc64


def _net_grads(enc_cls, **kw):
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    saved = nw.BasicMotionEncoder
    if enc_cls is not None:
        nw.BasicMotionEncoder = enc_cls
    try:
        net = nw.ERAFT({"subtype": "standard"}, n_first_channels=15, **kw)
    finally:
        nw.BasicMotionEncoder = saved
    net.load_state_dict(make_state_dict(net.state_dict()))
    net = net.cuda().train()
    net.freeze_bn()
    im1 = torch.from_numpy(prng.normal(3000, (1, 15, 128, 160))).cuda()
    im2 = torch.from_numpy(prng.normal(3001, (1, 15, 128, 160))).cuda()
    _, preds = net(im1, im2, iters=3)
    loss = sum(p.abs().mean() for p in preds)
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().double().cpu().numpy() for n, p in net.named_parameters() if p.grad is not None}


FLAGS = {"all-native": {"train_motion_corr": True, "train_gru": True, "hip_upsample": True},
         "differentiable_corr": {"differentiable_corr": True}}


@pytest.mark.parametrize("which", list(FLAGS))
def test_eraft_train_motion_encoder(ea, which):
    kw = FLAGS[which]
    ours = _net_grads(None, train_motion_encoder=True, **kw)
    g32 = _net_grads(None, **kw)
    g64 = _net_grads(_enc64_cls(), **kw)
    enc = [n for n in g32 if n.startswith("update_block.encoder.")]
    fnet = [n for n in g32 if n.startswith("fnet.")]
    assert len(enc) == 10 and fnet   # convc1 among them
    for n in g32:   # every parameter the stock arm trains
        assert n in ours, n
        assert np.isfinite(ours[n]).all(), n
        assert np.any(ours[n] != 0), n
    assert set(g64) == set(g32)

    def dist(a, names):
        num = sum(float(np.sum((a[n] - g64[n]) ** 2)) for n in names)
        den = sum(float(np.sum(g64[n] ** 2)) for n in names)
        return (num / den) ** 0.5

    every = list(g32)
    floor, mine = dist(g32, every), dist(ours, every)
    efloor, emine = dist(g32, enc), dist(ours, enc)
    print(f"{which}: gradients vs the fp64-encoder network, pooled: all parameters stock fp32 {floor:.3g} (the "
          f"floor), train_motion_encoder {mine:.3g} (ratio {mine / floor:.2f}); the encoder's ten: {efloor:.3g} / "
          f"{emine:.3g} (ratio {emine / efloor:.2f})")
    assert mine <= 4 * floor


def test_eraft_no_grad_bitwise_hip_motion_encoder(ea):
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    im1 = torch.from_numpy(prng.normal(3000, (1, 15, 128, 160))).cuda()
    im2 = torch.from_numpy(prng.normal(3001, (1, 15, 128, 160))).cuda()
    for other in ({}, {"fuse_motion_corr": True, "hip_upsample": True}):
        nets = []
        for kw in ({"hip_motion_encoder": True}, {"train_motion_encoder": True}):
            net = nw.ERAFT({"subtype": "standard"}, n_first_channels=15, **kw, **other)
            net.load_state_dict(make_state_dict(net.state_dict()))
            nets.append(net.cuda().eval())
        # the comparison is about the encoder path: the stock convolutions around it are asked for their
        # deterministic algorithms, and the hip_motion_encoder network is run twice to show they are
        saved = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            with torch.no_grad():
                assert not nets[1](im1, im2, iters=1)[1][0].requires_grad   # (also the first call of these shapes)
                hip, train, again = (nets[i](im1, im2, iters=3)[1] for i in (0, 1, 0))
        finally:
            torch.backends.cudnn.deterministic = saved
        for a, b, c in zip(hip, train, again):
            assert torch.equal(a, c), "the yardstick itself is not reproducible"
            assert torch.equal(a, b)


def epe(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.mean(np.sqrt(np.sum(d * d, axis=1))))


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_e2e_goldens_with_train_motion_encoder(ea, path):
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    z = np.load(path)
    H, W, bins, seed = int(z["H"]), int(z["W"]), int(z["bins"]), int(z["seed"])
    net = nw.ERAFT({"subtype": str(z["subtype"])}, n_first_channels=bins, train_motion_encoder=True)
    net.load_state_dict(make_state_dict(net.state_dict()))
    net = net.eval().cuda()
    im1 = torch.from_numpy(prng.normal(seed, (1, bins, H, W))).cuda()
    im2 = torch.from_numpy(prng.normal(seed + 1, (1, bins, H, W))).cuda()
    flow_init = torch.from_numpy(z["flow_init"]).cuda() if bool(z["warm"]) else None
    with torch.no_grad():
        low, ups = net(im1, im2, iters=12, flow_init=flow_init)
    st = int(z["up_stride"])
    low, up = low.cpu().numpy(), ups[-1].cpu().numpy()[:, :, ::st, ::st]
    e_low, e_up = epe(low, z["flow_low"]), epe(up, z["flow_up"])
    print(f"{os.path.basename(path)} train_motion_encoder: EPE vs reference low {e_low:.3g} px, up {e_up:.3g} px")
    assert np.isfinite(low).all() and np.isfinite(up).all()
    assert e_low <= EPE_TOL
    assert e_up <= EPE_TOL
