"""Training E-RAFT through the HIP SepConvGRU: ERAFT(train_gru=True) on the GPU.

Set-up of tests/test_motion_grad_gpu.py's _net_grads: image 1 x 15 x 128 x 160, iters = 3, train mode with frozen
BN, loss = sum of mean |prediction|.  Three arms of ERAFT(differentiable_corr=True, hip_upsample=True):
train_gru=True, the stock fp32 GRU (MIOpen + autograd), and a GRU evaluated in fp64 on the CPU inside the network
(tensors carried over and back, as torch_ref.TorchCpuCorrBlock does for the correlation).  Bar: the pooled
relative distance of ours to the fp64 arm <= 4 x the stock fp32 arm's -- two independent fp32 roundings of the same
sums amplified by the same network, the bar and reason of test_grad_gpu.test_eraft_fnet_grads.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return eraft_amd


def _gru64_cls():
    import eraft_amd.network as nw

    class Gru64(nw.SepConvGRU):
        """The same parameters (fp32, on the device), the arithmetic in fp64 on the CPU."""

        @staticmethod
        def _half(h, x, cz, cr, cq):
            def conv(c, t):
                return F.conv2d(t, c.weight.double().cpu(), c.bias.double().cpu(), padding=c.padding)
            hx = torch.cat([h, x], dim=1)
            z = torch.sigmoid(conv(cz, hx))
            r = torch.sigmoid(conv(cr, hx))
            q = torch.tanh(conv(cq, torch.cat([r * h, x], dim=1)))
            return (1 - z) * h + z * q

        def forward(self, h, x):
            out = super().forward(h.double().cpu(), x.double().cpu())
            return out.to(h.device).float()

    return Gru64


def _net_grads(gru_cls, **kw):
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    saved = nw.SepConvGRU
    if gru_cls is not None:
        nw.SepConvGRU = gru_cls
    try:
        net = nw.ERAFT({"subtype": "standard"}, n_first_channels=15, differentiable_corr=True, hip_upsample=True, **kw)
    finally:
        nw.SepConvGRU = saved
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


def test_eraft_train_gru(ea):
    ours = _net_grads(None, train_gru=True)
    g32 = _net_grads(None)
    g64 = _net_grads(_gru64_cls())
    gru = [n for n in g32 if n.startswith("update_block.gru.")]
    fnet = [n for n in g32 if n.startswith("fnet.")]
    assert len(gru) == 12 and fnet
    for n in g32:   # every parameter the stock arm trains, all twelve GRU tensors and fnet among them
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
    gfloor, gmine = dist(g32, gru), dist(ours, gru)
    print(f"gradients vs the fp64-GRU network, pooled: all parameters stock fp32 {floor:.3g} (the floor), train_gru "
          f"{mine:.3g} (ratio {mine / floor:.2f}); the GRU's twelve: {gfloor:.3g} / {gmine:.3g} "
          f"(ratio {gmine / gfloor:.2f})")
    assert mine <= 4 * floor
    assert gmine <= 4 * gfloor


def test_eraft_no_grad_bitwise_hip_gru(ea):
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    im1 = torch.from_numpy(prng.normal(3000, (1, 15, 128, 160))).cuda()
    im2 = torch.from_numpy(prng.normal(3001, (1, 15, 128, 160))).cuda()
    nets = []
    for kw in ({"hip_gru": True}, {"train_gru": True}):
        net = nw.ERAFT({"subtype": "standard"}, n_first_channels=15, **kw)
        net.load_state_dict(make_state_dict(net.state_dict()))
        nets.append(net.cuda().eval())
    # the comparison is about the GRU path: the stock convolutions around it are asked for their deterministic
    # algorithms, and the hip_gru network is run twice to show they are
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            assert not nets[1](im1, im2, iters=1)[1][0].requires_grad   # (also the first call of these conv shapes)
            hip, train, again = (nets[i](im1, im2, iters=3)[1] for i in (0, 1, 0))
    finally:
        torch.backends.cudnn.deterministic = saved
    for a, b, c in zip(hip, train, again):
        assert torch.equal(a, c), "the yardstick itself is not reproducible"
        assert torch.equal(a, b)
