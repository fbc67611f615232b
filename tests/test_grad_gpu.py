"""The differentiable CorrBlock (CorrBlock(..., differentiable=True); csrc/grad.hip) on the GPU.

Expected values are the reference CorrBlock's own gradients (tests/golden/backward_*.npz, captured
on the CPU by tests/golden/make_golden_backward.py in fp64; tests/backward_cases.py holds the cases,
inputs and the loss).  Bars: 1e-5 normwise (oracle.normwise_err, max |d| / rms: the project's bar
for the GEMM against fp64) for gradients; exact equality for which pyramid pixels receive gradient;
bitwise reproducibility.  The reference's own fp32 error against fp64 is printed beside ours.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import backward_cases as bc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-5
DEV = torch.device("cuda:0")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _golden(case):
    z = dict(np.load(os.path.join(GOLDEN, f"backward_{case}.npz")))
    z["grad_fmap2"] = np.load(os.path.join(GOLDEN, f"backward_{case}_g2.npz"))["grad_fmap2"]
    return z


def _forward_backward(case, keep_outs=False):
    """Our gradients of the case's loss through the Python API: (grad_fmap1, grad_fmap2, outs)."""
    import eraft_amd
    _, _, _, _, L, r, _ = bc.CASES[case]
    f1, f2 = (_cuda(f).requires_grad_(True) for f in bc.fmaps(case))
    blk = eraft_amd.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    loss, outs = 0.0, []
    for _, coords, gseed in bc.lookups(case):
        out = blk(_cuda(coords))
        if keep_outs:
            outs.append(out.detach().clone())
        loss = loss + (out * _cuda(bc.upstream(case, gseed))).sum()
    loss.backward()
    torch.cuda.synchronize()
    return f1.grad, f2.grad, outs


@pytest.mark.parametrize("mode", ["split", "fp32"])
@pytest.mark.parametrize("case", list(bc.CASES))
def test_fmap_grads_vs_reference(case, mode):
    """T1: both fmap gradients within 1e-5 normwise of the reference's fp64 gradients, in both build
    modes (the backward itself reads only the fmaps and the upstream gradients)."""
    _need_gpu()
    import oracle
    from eraft_amd import _lib
    z = _golden(case)
    ref_err = json.load(open(os.path.join(GOLDEN, "backward_errors.json")))[case]
    saved = _lib.build_mode()
    _lib.set_build_mode(mode)
    try:
        g1, g2, _ = _forward_backward(case)
    finally:
        _lib.set_build_mode(saved)
    e1 = oracle.normwise_err(g1.cpu().numpy(), z["grad_fmap1"])
    e2 = oracle.normwise_err(g2.cpu().numpy(), z["grad_fmap2"])
    print(f"{case} [{mode}]: normwise vs fp64 grad_fmap1 {e1:.3g} (reference fp32 {ref_err['grad_fmap1']:.3g}), "
          f"grad_fmap2 {e2:.3g} (reference fp32 {ref_err['grad_fmap2']:.3g})")
    assert e1 <= TOL
    assert e2 <= TOL


def _lookup_backward(case, names):
    """ecorr_lookup_backward alone (C ABI) for the named lookups -> reference-layout levels of G."""
    from eraft_amd import _lib
    from eraft_amd.layout import levels_of
    B, _, H, W, L, r, _ = bc.CASES[case]
    _, _, off = _lib.layout(B * H * W, H, W, L)
    G = torch.zeros(off[-1], dtype=torch.float32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for name, coords, gseed in bc.lookups(case):
        if name not in names:
            continue
        go, c = _cuda(bc.upstream(case, gseed)), _cuda(coords)
        _lib.check(_lib.lib().ecorr_lookup_backward(go.data_ptr(), c.data_ptr(), B, H, W, H * W, L, r,
                                                    G.data_ptr(), st), "lookup backward")
    torch.cuda.synchronize()
    return [lv[:, 0].cpu().numpy() for lv in levels_of(G, B * H * W, H, W, L)]


@pytest.mark.parametrize("case", list(bc.PYRAMID_CASES))
def test_pyramid_grad_support_and_values(case):
    """T2: the gradient pyramid of the lookups alone.  Per level the pixels that receive gradient are
    exactly the reference's (the forward's floor flips and zero padding, incl. the integer and
    near-integer coordinates of the edge case) and the values agree within 1e-5 normwise."""
    _need_gpu()
    import oracle
    z = _golden(case)
    L = bc.CASES[case][4]
    names = [n for n, _, _ in bc.lookups(case)]
    if case == bc.EDGE_CASE:
        assert "int" in names and "nearint" in names
    ours = _lookup_backward(case, names)
    for i in range(L):
        ref = z[f"pyr_all_l{i}"]
        assert ours[i].shape == ref.shape
        diff = int(((ours[i] != 0) != (ref != 0)).sum())
        err = oracle.normwise_err(ours[i], ref)
        print(f"{case} level {i}: support mismatches {diff} of {ref.size} ({int((ref != 0).sum())} nonzero), "
              f"normwise {err:.3g}")
        assert diff == 0
        assert err <= TOL
    far = _lookup_backward(case, ["s40"])   # mostly out of range: zero padding
    for i in range(L):
        ref = z[f"pyr_s40_l{i}"]
        assert not (far[i][ref == 0] != 0).any(), f"level {i}: gradient where the reference has none"
        assert ((far[i] != 0) == (ref != 0)).all()


def test_build_backward_slabs():
    """T3 (C ABI): row slabs 0..8 and 9..16 of the 17 x 20 case.  The slabs' grad_fmap1 concatenate to
    the whole one, their grad_fmap2 partials sum to it; NULL for either output is accepted."""
    _need_gpu()
    import oracle
    from eraft_amd import _lib
    case = "b2_17x20"
    B, D, H, W, L, r, _ = bc.CASES[case]
    L_ = _lib.lib()
    f1n, f2n = bc.fmaps(case)
    f2 = _cuda(f2n)
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    looks = bc.lookups(case)

    def run(y0, y1, want1=True, want2=True):
        q = (y1 - y0) * W
        f1 = _cuda(f1n[:, :, y0:y1])                       # [B][D][q]: contiguous rows
        _, _, off = _lib.layout(B * q, H, W, L)
        G = torch.zeros(off[-1], dtype=torch.float32, device=DEV)
        for _, coords, gseed in looks:
            go = _cuda(bc.upstream(case, gseed)[:, :, y0:y1])
            c = _cuda(coords[:, :, y0:y1])
            _lib.check(L_.ecorr_lookup_backward(go.data_ptr(), c.data_ptr(), B, H, W, q, L, r, G.data_ptr(), st),
                       "lookup backward")
        g1 = torch.full((B, D, y1 - y0, W), float("nan"), device=DEV) if want1 else None
        g2 = torch.full((B, D, H, W), float("nan"), device=DEV) if want2 else None
        _lib.check(L_.ecorr_build_backward(G.data_ptr(), f1.data_ptr(), f2.data_ptr(), B, D, H, W, q, L,
                                           None if g1 is None else g1.data_ptr(),
                                           None if g2 is None else g2.data_ptr(), st), "build backward")
        torch.cuda.synchronize()
        return g1, g2

    full1, full2 = run(0, H)
    a1, a2 = run(0, 9)
    b1, b2 = run(9, H)
    e1 = oracle.normwise_err(torch.cat([a1, b1], dim=2).cpu().numpy(), full1.cpu().numpy())
    e2 = oracle.normwise_err((a2 + b2).cpu().numpy(), full2.cpu().numpy())
    print(f"slabs: grad_fmap1 concat vs whole {e1:.3g}, grad_fmap2 sum vs whole {e2:.3g}")
    assert e1 <= TOL
    assert e2 <= TOL
    z = _golden(case)
    assert oracle.normwise_err(full1.cpu().numpy(), z["grad_fmap1"]) <= TOL
    assert oracle.normwise_err(full2.cpu().numpy(), z["grad_fmap2"]) <= TOL
    only1, none2 = run(0, 9, want2=False)
    none1, only2 = run(0, 9, want1=False)
    assert none1 is None and none2 is None
    assert torch.equal(only1, a1) and torch.equal(only2, a2)


def test_reproducible_and_forward_unchanged():
    """T4: bitwise equal gradients from two runs; forward values bitwise the plain block's; the
    refusals of the differentiable block and the unchanged refusal of the plain one."""
    _need_gpu()
    import eraft_amd
    case = "b2_17x20"
    _, _, _, _, L, r, _ = bc.CASES[case]
    g1a, g2a, outs = _forward_backward(case, keep_outs=True)
    g1b, g2b, _ = _forward_backward(case)
    assert torch.equal(g1a, g1b) and torch.equal(g2a, g2b)
    with torch.no_grad():
        plain = eraft_amd.CorrBlock(*(_cuda(f) for f in bc.fmaps(case)), num_levels=L, radius=r)
        for (_, coords, _), out in zip(bc.lookups(case), outs):
            assert torch.equal(plain(_cuda(coords)), out)

    g = torch.zeros(1, 16, 8, 8, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        eraft_amd.CorrBlock(g, g)
    with pytest.raises(RuntimeError, match="forward-only"):
        eraft_amd.CorrBlock(g, g, 4, 4, differentiable=False)

    # a second backward through a consumed block
    f1, f2 = (_cuda(f).requires_grad_(True) for f in bc.fmaps("d3_l3r1"))
    blk = eraft_amd.CorrBlock(f1, f2, num_levels=3, radius=1, differentiable=True)
    coords = _cuda(bc.coord_sets("d3_l3r1")["s0p5"])
    loss = blk(coords).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    # coordinates that require grad
    blk = eraft_amd.CorrBlock(f1, f2, num_levels=3, radius=1, differentiable=True)
    with pytest.raises(RuntimeError, match="coords requires grad"):
        blk(coords.clone().requires_grad_(True))
    # an in-place change of the saved coordinates is caught by autograd's version check
    c2 = coords.clone()
    out = blk(c2)
    c2.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    # under no_grad the differentiable block is the plain block
    with torch.no_grad():
        nb = eraft_amd.CorrBlock(f1, f2, num_levels=3, radius=1, differentiable=True)
        assert not nb(coords).requires_grad
    # level 3 of an 8 x 12 map is 1 x 1: refused when differentiable, accepted by the plain block
    h1, h2 = (torch.randn(1, 16, 8, 12, device=DEV).requires_grad_(True) for _ in range(2))
    with pytest.raises(RuntimeError, match="at least 2 x 2"):
        eraft_amd.CorrBlock(h1, h2, num_levels=4, radius=4, differentiable=True)
    with torch.no_grad():
        eraft_amd.CorrBlock(h1, h2, num_levels=4, radius=4)
    import eraft_amd.network as nw
    with pytest.raises(ValueError, match="fuse_motion_corr"):
        nw.ERAFT({"subtype": "standard"}, 15, fuse_motion_corr=True, differentiable_corr=True)


def _fnet_grads(corr_cls, differentiable):
    """fnet parameter gradients of mean |prediction| over 3 iterations, train() mode with frozen BN."""
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    import prng
    saved = nw.CorrBlock
    if corr_cls is not None:
        nw.CorrBlock = corr_cls
    try:
        net = nw.ERAFT({"subtype": "standard"}, n_first_channels=15, differentiable_corr=differentiable)
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
    return {n: p.grad.detach().double().cpu().numpy() for n, p in net.fnet.named_parameters()}


def test_eraft_fnet_grads():
    """T5: gradients reach every fnet parameter through the HIP backward, and they are as close to
    the fp64 correlation's gradients as the reference's own fp32 op sequence is (within 4x: two
    independent fp32 roundings amplified by the same GRU)."""
    _need_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    from torch_ref import TorchCpuCorrBlock

    class Corr64(TorchCpuCorrBlock):   # the reference's op sequence with the volume in fp64
        def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
            super().__init__(fmap1.double(), fmap2.double(), num_levels, radius)

        def __call__(self, coords):
            return super().__call__(coords.double())

    ours = _fnet_grads(None, True)
    g64 = _fnet_grads(Corr64, False)
    g32 = _fnet_grads(TorchCpuCorrBlock, False)
    for n, g in ours.items():
        assert np.isfinite(g).all(), n
        assert np.any(g != 0), n

    def dist(a):   # normwise over all fnet parameters
        num = sum(float(np.sum((a[n] - g64[n]) ** 2)) for n in g64)
        den = sum(float(np.sum(g64[n] ** 2)) for n in g64)
        return (num / den) ** 0.5

    floor, mine = dist(g32), dist(ours)
    print(f"fnet gradients vs fp64-correlation network: reference ops in fp32 {floor:.3g} (the floor), ours {mine:.3g} "
          f"(ratio {mine / floor:.2f})")
    assert mine <= 4 * floor
