"""Training through CorrBlock.lookup_conv1x1_relu (differentiable=True) and ERAFT(train_motion_corr=True)
on the GPU.

Loss of the block tests, over the lookups of tests/backward_cases.py in order:
    loss = sum_i (blk.lookup_conv1x1_relu(coords_i, w, b) * go_i).sum(),  go_i = prng.normal(seed_i, out.shape)
Reference: the existing differentiable block's blk(coords_i) feeding a torch fp64 conv whose ReLU mask
is taken from OUR forward's out.  It has to be: a split-conv output within rounding of zero may have
the other sign in fp64, and one flipped mask element changes a whole grad_corr column by far more
than 1e-5 -- with its own mask the reference itself would miss the bar.
Bars: grad_fmap1 / grad_fmap2 1e-5 normwise (oracle.normwise_err, as tests/test_grad_gpu.py); weight and
bias max(1e-5, 2 x the distance of ATen's fp32 conv backward, same mask, TF32 off) as
tests/test_conv_grad_gpu.py.  Every test prints its figures.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_cases as bc
import prng

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = ("t16x24", "b2_17x20")


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return eraft_amd


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _params(case, O, bias=True):
    L, r, seed = bc.CASES[case][4:]
    C = L * (2 * r + 1) ** 2
    w = _cuda(prng.normal(seed + 300, (O, C, 1, 1)) * np.float32(0.05))
    b = _cuda(prng.normal(seed + 301, (O,)) * np.float32(0.1)) if bias else None
    return w, b


def _upstream(case, gseed, O):
    B, _, H, W = bc.CASES[case][:4]
    return _cuda(prng.normal(gseed + 50, (B, O, H, W)))


def _ours(ea, case, mode, O, live=True, train_w=True):
    """(outs, grad_fmap1, grad_fmap2, grad_w, grad_b, block) of the loss through the new path."""
    L, r = bc.CASES[case][4:6]
    f1, f2 = (_cuda(f).requires_grad_(live) for f in bc.fmaps(case))
    w, b = _params(case, O)
    w.requires_grad_(train_w)
    b.requires_grad_(train_w)
    blk = ea.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    loss, outs = 0.0, []
    for _, coords, gseed in bc.lookups(case):
        out = blk.lookup_conv1x1_relu(_cuda(coords), w, b, mode=mode)
        outs.append(out.detach().clone())
        loss = loss + (out * _upstream(case, gseed, O)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return outs, f1.grad, f2.grad, w.grad, b.grad, blk


def _reference(ea, case, O, outs, dtype):
    """The same loss through blk(coords) + a torch conv in `dtype` with the ReLU mask of `outs`."""
    L, r = bc.CASES[case][4:6]
    f1, f2 = (_cuda(f).requires_grad_(True) for f in bc.fmaps(case))
    w, b = _params(case, O)
    w, b = w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    blk = ea.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    loss = 0.0
    for (_, coords, gseed), out in zip(bc.lookups(case), outs):
        y = F.conv2d(blk(_cuda(coords)).to(dtype), w, b)
        loss = loss + (y * (out > 0).to(dtype) * _upstream(case, gseed, O).to(dtype)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return f1.grad, f2.grad, w.grad, b.grad


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode,O", [("split", 256), ("fused", 256), ("fused", 64), ("presplit", 256)])
def test_forward_bitwise_plain(ea, case, mode, O):
    L, r = bc.CASES[case][4:6]
    outs = _ours(ea, case, mode, O)[0]
    w, b = _params(case, O)
    with torch.no_grad():
        f1, f2 = (_cuda(f) for f in bc.fmaps(case))   # kept alive: presplit reads its column scales from them
        plain = ea.CorrBlock(f1, f2, num_levels=L, radius=r)
        for (_, coords, _), out in zip(bc.lookups(case), outs):
            assert torch.equal(plain.lookup_conv1x1_relu(_cuda(coords), w, b, mode=mode), out)
        assert (plain._colscale is not None) == (mode == "presplit")


@pytest.mark.parametrize("case,mode,O", [("t16x24", "split", 256), ("b2_17x20", "split", 256),
                                         ("t16x24", "fused", 64), ("b2_17x20", "presplit", 256)])
def test_grads_vs_fp64_chain(ea, case, mode, O):
    import oracle
    outs, g1, g2, gw, gb, _ = _ours(ea, case, mode, O)
    r1, r2, rw, rb = _reference(ea, case, O, outs, torch.float64)
    _, _, aw, ab = _reference(ea, case, O, outs, torch.float32)

    def err(a, ref):
        return oracle.normwise_err(a.double().cpu().numpy(), ref.double().cpu().numpy())
    e1, e2, ew, eb = err(g1, r1), err(g2, r2), err(gw, rw), err(gb, rb)
    fw, fb = err(aw, rw), err(ab, rb)
    print(f"{case} [{mode}, O = {O}]: normwise vs the fp64 chain grad_fmap1 {e1:.3g}, grad_fmap2 {e2:.3g}, "
          f"grad_weight {ew:.3g} (ATen fp32 {fw:.3g}), grad_bias {eb:.3g} (ATen fp32 {fb:.3g})")
    assert e1 <= 1e-5
    assert e2 <= 1e-5
    assert ew <= max(1e-5, 2 * fw)
    assert eb <= max(1e-5, 2 * fb)


def test_frozen_fmaps_train_weight_only(ea):
    """Frozen fmaps, weight and bias requiring grad: their gradients only (bitwise the live block's),
    no gradient pyramid, and more than one backward is allowed (nothing of the block is consumed)."""
    case = "b2_17x20"
    _, g1, g2, gw, gb, blk = _ours(ea, case, "split", 256, live=False)
    assert g1 is None and g2 is None and blk._grad is None and blk._handle is None
    _, _, _, lw, lb, live = _ours(ea, case, "split", 256, live=True)
    assert torch.equal(gw, lw) and torch.equal(gb, lb)
    assert live._grad.buf is None   # the build backward freed the block's one gradient pyramid
    # live block, frozen weight: fmap gradients only
    _, f1g, f2g, nw_, nb_, _ = _ours(ea, case, "split", 256, live=True, train_w=False)
    assert nw_ is None and nb_ is None and f1g is not None and f2g is not None


def test_reproducible_and_refusals(ea):
    case = "b2_17x20"
    L, r = bc.CASES[case][4:6]
    a = _ours(ea, case, "split", 256)
    b = _ours(ea, case, "split", 256)
    for x, y in zip(a[1:5], b[1:5]):
        assert torch.equal(x, y)

    f1, f2 = (_cuda(f).requires_grad_(True) for f in bc.fmaps(case))
    w, bias = _params(case, 256)
    w.requires_grad_(True)
    coords = _cuda(bc.coord_sets(case)["s0p5"])
    # a second backward through a consumed block
    blk = ea.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    loss = blk.lookup_conv1x1_relu(coords, w, bias).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    # coordinates that require grad
    blk = ea.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    with pytest.raises(RuntimeError, match="coords requires grad"):
        blk.lookup_conv1x1_relu(coords.clone().requires_grad_(True), w, bias)
    # an in-place change of a saved tensor (the coordinates; the output) is caught by autograd's version check
    c2 = coords.clone()
    out = blk.lookup_conv1x1_relu(c2, w, bias)
    c2.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    blk = ea.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    out = blk.lookup_conv1x1_relu(coords, w, bias)
    s = out.sum()
    out.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        s.backward()
    # under no_grad the differentiable block's call is the plain forward
    with torch.no_grad():
        nb = ea.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
        assert not nb.lookup_conv1x1_relu(coords, w, bias).requires_grad
    # a plain block keeps its refusal
    with torch.no_grad():
        plain = ea.CorrBlock(f1, f2, num_levels=L, radius=r)
    with pytest.raises(RuntimeError, match="forward-only"):
        plain.lookup_conv1x1_relu(coords, w, bias)


def _net_grads(corr_cls, **kw):
    """Parameter gradients of mean |prediction| over 3 iterations, train() mode with frozen BN: the set-up
    of tests/test_grad_gpu.py's _fnet_grads."""
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    saved = nw.CorrBlock
    if corr_cls is not None:
        nw.CorrBlock = corr_cls
    try:
        net = nw.ERAFT({"subtype": "standard"}, n_first_channels=15, **kw)
        net.load_state_dict(make_state_dict(net.state_dict()))
        net = net.cuda().train()
        net.freeze_bn()
        im1 = torch.from_numpy(prng.normal(3000, (1, 15, 128, 160))).cuda()
        im2 = torch.from_numpy(prng.normal(3001, (1, 15, 128, 160))).cuda()
        _, preds = net(im1, im2, iters=3)
        loss = sum(p.abs().mean() for p in preds)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        nw.CorrBlock = saved
    return {n: p.grad.detach().double().cpu().numpy() for n, p in net.named_parameters() if p.grad is not None}


def test_eraft_train_motion_corr(ea):
    """Gradients reach every fnet parameter and convc1 through the HIP backward, as close to the fp64
    correlation's as the reference's own fp32 op sequence is (within 4x: two independent fp32 roundings
    amplified by the same GRU -- the bar and reason of test_grad_gpu.test_eraft_fnet_grads)."""
    from torch_ref import TorchCpuCorrBlock

    class Corr64(TorchCpuCorrBlock):   # the reference's op sequence with the volume in fp64
        def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
            super().__init__(fmap1.double(), fmap2.double(), num_levels, radius)

        def __call__(self, coords):
            return super().__call__(coords.double())

    ours = _net_grads(None, train_motion_corr=True)
    g64 = _net_grads(Corr64)
    g32 = _net_grads(TorchCpuCorrBlock)
    fnet = [n for n in g64 if n.startswith("fnet.")]
    convc1 = ["update_block.encoder.convc1.weight", "update_block.encoder.convc1.bias"]
    assert fnet
    for n in fnet + convc1:
        assert np.isfinite(ours[n]).all(), n
        assert np.any(ours[n] != 0), n

    def dist(a, names):
        num = sum(float(np.sum((a[n] - g64[n]) ** 2)) for n in names)
        den = sum(float(np.sum(g64[n] ** 2)) for n in names)
        return (num / den) ** 0.5

    floor, mine = dist(g32, fnet), dist(ours, fnet)
    cfloor, cmine = dist(g32, convc1), dist(ours, convc1)
    print(f"fnet gradients vs fp64-correlation network: reference ops in fp32 {floor:.3g} (the floor), "
          f"train_motion_corr {mine:.3g} (ratio {mine / floor:.2f}); convc1 gradients: {cfloor:.3g} / {cmine:.3g} "
          f"(ratio {cmine / cfloor:.2f})")
    assert mine <= 4 * floor


def test_eraft_no_grad_bitwise_fuse_motion_corr(ea):
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    im1 = torch.from_numpy(prng.normal(3000, (1, 15, 128, 160))).cuda()
    im2 = torch.from_numpy(prng.normal(3001, (1, 15, 128, 160))).cuda()
    nets = []
    for kw in ({"fuse_motion_corr": True}, {"train_motion_corr": True}):
        net = nw.ERAFT({"subtype": "standard"}, n_first_channels=15, **kw)
        net.load_state_dict(make_state_dict(net.state_dict()))
        nets.append(net.cuda().eval())
    # the comparison is about the CorrBlock path: the stock convolutions around it are asked for their
    # deterministic algorithms, and the fuse_motion_corr network is run twice to show they are
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            assert not nets[1](im1, im2, iters=1)[1][0].requires_grad   # (also the first call of these conv shapes)
            fuse, train, again = (nets[i](im1, im2, iters=3)[1] for i in (0, 1, 0))
    finally:
        torch.backends.cudnn.deterministic = saved
    same = [float((a - b).abs().max()) for a, b in zip(fuse, again)]
    diff = [float((a - b).abs().max()) for a, b in zip(fuse, train)]
    print(f"max |d| of the predictions: fuse_motion_corr twice {same}, train_motion_corr vs fuse_motion_corr {diff}")
    for a, b, c in zip(fuse, train, again):
        assert torch.equal(a, c), "the yardstick itself is not reproducible"
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="fuse_motion_corr"):
        nw.ERAFT({"subtype": "standard"}, 15, fuse_motion_corr=True, differentiable_corr=True)
