"""The trainable AlternateCorrBlock (AlternateCorrBlock(..., trainable=True); csrc/alt_grad.hip) on the GPU.

The block is the same mathematical function as CorrBlock, so the references are CorrBlock's: the fp64
gradients of the reference (tests/golden/backward_*.npz, tests/backward_cases.py) and the plain fp64
references of tests/grad_ref.py (validated on the CPU by tests/test_grad_ref.py).  Bars: 1e-5 normwise
(oracle.normwise_err) against the goldens; max(1e-5, 2 e_aten) against grad_ref, e_aten being the distance
of ATen's fp32 autograd from the same reference (tests/test_grad_edges_gpu.py's rule); bitwise equality
wherever two runs, two dtypes or two workspaces must give the same gradients.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import alt_corr_cases as ac
import backward_cases as bc
import gpu_guard as gg
import grad_ref as gr
import prng
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-5
DEV = torch.device("cuda:0")
H1_CASE = "a4_8x32_h1_d8"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _bar(e_aten):
    return max(TOL, 2.0 * e_aten)


def _run(f1n, f2n, L, r, lookups, keep_outs=False, **kw):
    """Gradients of sum_i (blk(coords_i) * go_i).sum() over lookups = [(coords, go)] through the Python
    API: (grad_fmap1, grad_fmap2, outs)."""
    import eraft_amd
    f1, f2 = _cuda(f1n).requires_grad_(True), _cuda(f2n).requires_grad_(True)
    blk = eraft_amd.AlternateCorrBlock(f1, f2, num_levels=L, radius=r, trainable=True, **kw)
    loss, outs = 0.0, []
    for coords, go in lookups:
        out = blk(_cuda(coords))
        if keep_outs:
            outs.append(out.detach().clone())
        loss = loss + (out * _cuda(go)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return f1.grad, f2.grad, outs


def _golden_lookups(case):
    return [(coords, bc.upstream(case, gseed)) for _, coords, gseed in bc.lookups(case)]


# ---------------------------------------------------------------------------------------------
# 1. the reference's fp64 gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(bc.CASES))
def test_fmap_grads_vs_golden(case):
    _need_gpu()
    import oracle
    _, _, _, _, L, r, _ = bc.CASES[case]
    z1 = np.load(os.path.join(GOLDEN, f"backward_{case}.npz"))["grad_fmap1"]
    z2 = np.load(os.path.join(GOLDEN, f"backward_{case}_g2.npz"))["grad_fmap2"]
    ref_err = json.load(open(os.path.join(GOLDEN, "backward_errors.json")))[case]
    g1, g2, _ = _run(*bc.fmaps(case), L, r, _golden_lookups(case))
    e1 = oracle.normwise_err(g1.cpu().numpy(), z1)
    e2 = oracle.normwise_err(g2.cpu().numpy(), z2)
    print(f"{case}: normwise vs fp64 grad_fmap1 {e1:.3g} (reference fp32 {ref_err['grad_fmap1']:.3g}), "
          f"grad_fmap2 {e2:.3g} (reference fp32 {ref_err['grad_fmap2']:.3g})")
    assert e1 <= TOL
    assert e2 <= TOL


# ---------------------------------------------------------------------------------------------
# 2. dispatch and shape cases against grad_ref
# ---------------------------------------------------------------------------------------------
def _case_lookups(name):
    """The nine coordinate sets as nine lookups, each with its own upstream."""
    s = ac.seed_of(name)
    _, B, _, H, W, _ = ac.CASES[name]
    return [(c, prng.normal(s + 20 + i, (B, ac.channels(name), H, W))) for i, c in enumerate(ac.coord_sets(name).values())]


@pytest.mark.parametrize("name", [n for n in ac.CASES if n != H1_CASE])
def test_fmap_grads_vs_grad_ref(name):
    """D = 37 padded to 40, D = 320 over two channel passes, r = 0, 1, 4, 5, 8, a window wider than the image,
    odd sides, B = 2; NaN / inf / huge, border, integer and near-integer coordinates among the lookups."""
    _need_gpu()
    import oracle
    r, B, D, H, W, L = ac.CASES[name]
    f1n, f2n = ac.fmaps(name)
    looks = _case_lookups(name)
    assert len(looks) == 9
    hs, ws = gr.level_sizes(H, W, L)
    G = [np.zeros((B * H * W, h, w)) for h, w in zip(hs, ws)]
    Ga = [np.zeros((B * H * W, h, w), dtype=np.float32) for h, w in zip(hs, ws)]
    for c, go in looks:
        gq, cq = go.reshape(B, -1, H * W), c.reshape(B, 2, H * W)
        for acc, lv in zip(G, gr.lookup_backward_ref(gq, cq, hs, ws, r)):
            acc += lv
        for acc, lv in zip(Ga, gr.aten_lookup_backward(gq, cq, hs, ws, r)):
            acc += lv
    r1, r2 = gr.build_backward_ref(G, f1n.reshape(B, D, -1), f2n)
    a1, a2 = gr.aten_build_backward(Ga, f1n.reshape(B, D, -1), f2n)
    g1, g2, _ = _run(f1n, f2n, L, r, looks)
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    for what, ours, ref, aten in (("grad_fmap1", g1, r1.reshape(f1n.shape), a1.reshape(f1n.shape)),
                                  ("grad_fmap2", g2, r2, a2)):
        e_aten = oracle.normwise_err(aten, ref)
        e = oracle.normwise_err(ours.cpu().numpy(), ref)
        print(f"{name} {what}: normwise ours {e:.3g}, ATen fp32 {e_aten:.3g}, bar {_bar(e_aten):.3g}")
        assert e <= _bar(e_aten), what


def test_one_pixel_level_refused():
    _need_gpu()
    import eraft_amd
    r, B, D, H, W, L = ac.CASES[H1_CASE]
    f1, f2 = (_cuda(f) for f in ac.fmaps(H1_CASE))
    with pytest.raises(RuntimeError, match="at least 2 x 2"):
        eraft_amd.AlternateCorrBlock(f1.clone().requires_grad_(True), f2, num_levels=L, radius=r, trainable=True)
    with pytest.raises(RuntimeError, match="at least 2 x 2"):
        eraft_amd.AlternateCorrBlock(f1, f2.clone().requires_grad_(True), num_levels=L, radius=r, trainable=True)
    eraft_amd.AlternateCorrBlock(f1, f2, num_levels=L, radius=r, trainable=True)   # not live: the plain block


# ---------------------------------------------------------------------------------------------
# 3. nothing in range
# ---------------------------------------------------------------------------------------------
def test_nothing_in_range():
    """Every coordinate one of grad_ref.SERIAL (NaN, +-inf, huge): both gradients are exactly zero, and
    such a lookup beside a finite one changes no bit of the finite one's gradients."""
    _need_gpu()
    name = "a4_17x21_d37"
    r, B, D, H, W, L = ac.CASES[name]
    f1n, f2n = ac.fmaps(name)
    pick = prng.uniform(4242, (B, 2, H, W), 0.0, float(gr.SERIAL.size)).astype(np.int64).clip(0, gr.SERIAL.size - 1)
    dead = gr.SERIAL[pick]
    assert np.isnan(dead).any() and np.isinf(dead).any()
    go_dead = prng.normal(4243, (B, ac.channels(name), H, W))
    fine = ac.coord_sets(name)["smooth"]
    go_fine = prng.normal(4244, (B, ac.channels(name), H, W))

    def run(looks):   # torch.autograd.backward: the NaN samples of the forward never enter a loss
        import eraft_amd
        f1, f2 = _cuda(f1n).requires_grad_(True), _cuda(f2n).requires_grad_(True)
        blk = eraft_amd.AlternateCorrBlock(f1, f2, num_levels=L, radius=r, trainable=True)
        outs = [blk(_cuda(c)) for c, _ in looks]
        torch.autograd.backward(outs, [_cuda(g) for _, g in looks])
        torch.cuda.synchronize()
        return f1.grad, f2.grad

    z1, z2 = run([(dead, go_dead)])
    for z in (z1, z2):
        assert torch.isfinite(z).all()
        assert int(torch.count_nonzero(z)) == 0
    a1, a2 = run([(fine, go_fine)])
    assert int(torch.count_nonzero(a1)) > 0 and int(torch.count_nonzero(a2)) > 0
    for order in ([(fine, go_fine), (dead, go_dead)], [(dead, go_dead), (fine, go_fine)]):
        b1, b2 = run(order)
        assert torch.equal(a1, b1) and torch.equal(a2, b2)


# ---------------------------------------------------------------------------------------------
# 4. reproducible, forward unchanged
# ---------------------------------------------------------------------------------------------
def test_reproducible_and_forward_unchanged():
    _need_gpu()
    import eraft_amd
    case = "b2_17x20"
    _, _, _, _, L, r, _ = bc.CASES[case]
    looks = _golden_lookups(case)
    g1a, g2a, outs = _run(*bc.fmaps(case), L, r, looks, keep_outs=True)
    g1b, g2b, _ = _run(*bc.fmaps(case), L, r, looks)
    assert torch.equal(g1a, g1b) and torch.equal(g2a, g2b)
    f1, f2 = (_cuda(f) for f in bc.fmaps(case))
    with torch.no_grad():
        plain = eraft_amd.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)
        for (coords, _), out in zip(looks, outs):
            assert torch.equal(plain(_cuda(coords)), out)
        # under no_grad a trainable block is the plain block
        nb = eraft_amd.AlternateCorrBlock(f1.clone().requires_grad_(True), f2, num_levels=L, radius=r, trainable=True)
        assert nb._grad is None and nb._handle is None
        out = nb(_cuda(looks[0][0]))
        assert not out.requires_grad and torch.equal(out, outs[0])
    # frozen fmaps: the plain block too, also with grad mode on
    fb = eraft_amd.AlternateCorrBlock(f1, f2, num_levels=L, radius=r, trainable=True)
    assert fb._grad is None and not fb(_cuda(looks[0][0])).requires_grad


# ---------------------------------------------------------------------------------------------
# 5. the C ABI between guards
# ---------------------------------------------------------------------------------------------
def test_abi_guards_workspace_and_null_outputs():
    _need_gpu()
    import eraft_amd
    from eraft_amd import _lib
    name = "a4_17x21_d37"
    r, B, D, H, W, L = ac.CASES[name]
    f1, f2 = (_cuda(f) for f in ac.fmaps(name))
    with torch.no_grad():
        feat = eraft_amd.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)._feat
    n = ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_alt_size(B, D, H, W, L, ctypes.byref(n)), "size")
    assert n.value == feat.numel()
    nb = ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_alt_backward_workspace_size(B, H, W, L, r, ctypes.byref(nb)), "workspace size")
    sets = ac.coord_sets(name)
    looks = [(_cuda(sets[k]), _cuda(prng.normal(4300 + i, (B, ac.channels(name), H, W))))
             for i, k in enumerate(("smooth", "special", "edge"))]

    def lookups(fill):
        gbuf, gfeat = gg.guarded(n.value)
        gfeat.zero_()
        ws = gg.Workspace(nb.value, fill)
        for c, go in looks:
            _lib.check(_lib.lib().ecorr_alt_lookup_backward(
                feat.data_ptr(), c.data_ptr(), go.data_ptr(), B, D, H, W, L, r, gfeat.data_ptr(), ws.ptr, _stream()),
                "lookup backward")
        torch.cuda.synchronize()
        ws.check(f"workspace filled with {fill:#x}")
        gg.check_guarded(gbuf, "grad_feat")
        return gbuf

    def pack(gbuf, want1=True, want2=True):
        gbuf = gbuf.clone()   # the pack backward consumes grad_feat
        gfeat = gbuf[gg.GUARD:gg.GUARD + n.value].view(torch.float32)
        (b1, g1), (b2, g2) = gg.guarded(B * D * H * W), gg.guarded(B * D * H * W)
        _lib.check(_lib.lib().ecorr_alt_pack_backward(
            gfeat.data_ptr(), B, D, H, W, L, g1.data_ptr() if want1 else None, g2.data_ptr() if want2 else None,
            _stream()), "pack backward")
        torch.cuda.synchronize()
        gg.check_guarded(gbuf, "grad_feat after the pack backward")
        o1 = gg.check_guarded(b1, "grad_fmap1") if want1 else None
        o2 = gg.check_guarded(b2, "grad_fmap2") if want2 else None
        if not want1:
            assert bool((b1 == gg.FILL).all())
        if not want2:
            assert bool((b2 == gg.FILL).all())
        return o1, o2

    zeroed, dirty = lookups(0), lookups(gg.BYTE_FILL)
    assert torch.equal(zeroed, dirty), "the workspace's earlier contents changed grad_feat"
    g1, g2 = pack(zeroed)
    assert np.isfinite(g1).all() and np.isfinite(g2).all() and g1.any() and g2.any()
    only1, none2 = pack(zeroed, want2=False)
    none1, only2 = pack(zeroed, want1=False)
    assert none1 is None and none2 is None
    assert gg.mismatch(only1.reshape(B, D, -1), g1.reshape(B, D, -1)) is None
    assert gg.mismatch(only2.reshape(B, D, -1), g2.reshape(B, D, -1)) is None
    # and the Python API gives the same bits: autograd runs the lookups' backwards last lookup first, so the
    # block whose lookups are these in reverse adds them into grad_feat in the order of the calls above
    p1, p2, _ = _run(*ac.fmaps(name), L, r, [(c.cpu().numpy(), go.cpu().numpy()) for c, go in reversed(looks)])
    assert gg.mismatch(p1.cpu().numpy().reshape(B, D, -1), g1.reshape(B, D, -1)) is None
    assert gg.mismatch(p2.cpu().numpy().reshape(B, D, -1), g2.reshape(B, D, -1)) is None


# ---------------------------------------------------------------------------------------------
# 6. 16-bit at both ends
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_sixteen_bit(dtype):
    _need_gpu()
    import eraft_amd
    case = "l3r2_d64"
    _, _, _, _, L, r, _ = bc.CASES[case]
    looks = [(_cuda(c), _cuda(go)) for c, go in _golden_lookups(case)]
    h1, h2 = (_cuda(f).to(dtype) for f in bc.fmaps(case))

    def grads(a, b, upstream, **kw):
        a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        blk = eraft_amd.AlternateCorrBlock(a, b, num_levels=L, radius=r, trainable=True,
                                           **({"fmap_dtype": a.dtype} if a.dtype != torch.float32 else {}))
        outs = [blk(c, **kw) for c, _ in looks]
        torch.autograd.backward(outs, upstream)
        torch.cuda.synchronize()
        return a.grad, b.grad, outs

    up32 = [go for _, go in looks]
    w1, w2, _ = grads(h1.float(), h2.float(), up32)
    assert w1.dtype == w2.dtype == torch.float32
    # 16-bit fmaps: gradients in the fmaps' dtype, the fp32 block's on fmap.float() cast once
    s1, s2, _ = grads(h1, h2, up32)
    assert s1.dtype == s2.dtype == dtype
    assert torch.equal(s1, w1.to(dtype)) and torch.equal(s2, w2.to(dtype))
    # a 16-bit output: the fp32 backward on the upstream's exact values
    up16 = [go.to(dtype) for go in up32]
    o1, o2, outs = grads(h1.float(), h2.float(), up16, out_dtype=dtype)
    assert all(o.dtype == dtype for o in outs)
    x1, x2, _ = grads(h1.float(), h2.float(), [g.float() for g in up16])
    assert torch.equal(o1, x1) and torch.equal(o2, x2)


# ---------------------------------------------------------------------------------------------
# 7. contract
# ---------------------------------------------------------------------------------------------
def test_contract():
    _need_gpu()
    import eraft_amd
    case = "d3_l3r1"
    f1, f2 = (_cuda(f).requires_grad_(True) for f in bc.fmaps(case))
    coords = _cuda(bc.coord_sets(case)["s0p5"])
    blk = eraft_amd.AlternateCorrBlock(f1, f2, num_levels=3, radius=1, trainable=True)
    loss = blk(coords).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    blk = eraft_amd.AlternateCorrBlock(f1, f2, num_levels=3, radius=1, trainable=True)
    with pytest.raises(RuntimeError, match="coords requires grad"):
        blk(coords.clone().requires_grad_(True))
    c2 = coords.clone()
    out = blk(c2)
    c2.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    # an in-place change of an fmap after construction neither raises nor changes the gradients: the
    # backward reads the block's own copy of the features
    a1, a2 = (_cuda(f).requires_grad_(True) for f in bc.fmaps(case))
    ref = eraft_amd.AlternateCorrBlock(a1, a2, num_levels=3, radius=1, trainable=True)
    ref(coords).sum().backward()
    b1, b2 = (_cuda(f).requires_grad_(True) for f in bc.fmaps(case))
    chg = eraft_amd.AlternateCorrBlock(b1, b2, num_levels=3, radius=1, trainable=True)
    out = chg(coords)
    with torch.no_grad():
        b1.mul_(2.0)
    out.sum().backward()
    assert torch.equal(a1.grad, b1.grad) and torch.equal(a2.grad, b2.grad)
    # no lookup receives a gradient: zeros through the handle
    z1, z2 = (_cuda(f).requires_grad_(True) for f in bc.fmaps(case))
    zb = eraft_amd.AlternateCorrBlock(z1, z2, num_levels=3, radius=1, trainable=True)
    zb(coords)
    zb._handle.sum().backward()
    assert zb._grad.consumed and zb._grad.buf is None
    assert int(torch.count_nonzero(z1.grad)) == 0 and int(torch.count_nonzero(z2.grad)) == 0
    # what stays refused
    with pytest.raises(RuntimeError, match="forward-only"):
        eraft_amd.AlternateCorrBlock(f1, f2, num_levels=3, radius=1)
    with pytest.raises(NotImplementedError, match="differentiable"):
        eraft_amd.AlternateCorrBlock(f1, f2, num_levels=3, radius=1, differentiable=True)
    with pytest.raises(NotImplementedError, match="differentiable"):
        eraft_amd.AlternateCorrBlock(f1, f2, num_levels=3, radius=1, differentiable=True, trainable=True)
    with pytest.raises(NotImplementedError, match="corr_pyramid"):
        blk.corr_pyramid
    with pytest.raises(NotImplementedError, match="lookup_conv1x1_relu"):
        blk.lookup_conv1x1_relu(coords, torch.zeros(8, 27, device=DEV))


# ---------------------------------------------------------------------------------------------
# 8. memory
# ---------------------------------------------------------------------------------------------
def test_peak_memory():
    """Peak allocation of construction + 3 lookups + loss + backward at 48 x 64, B = 1, D = 64: at most what
    the size entries add up to, and below the same step's with CorrBlock(differentiable=True)."""
    _need_gpu()
    import eraft_amd
    from eraft_amd import _lib
    B, D, H, W, L, r = 1, 64, 48, 64, 4, 4
    C = _lib.corr_channels(L, r)
    f1n, f2n = prng.normal(4400, (B, D, H, W)), prng.normal(4401, (B, D, H, W))
    cs = [_cuda(prng.coords_with_flow(4402 + i, B, H, W, 3.0)) for i in range(3)]
    gos = [_cuda(prng.normal(4410 + i, (B, C, H, W))) for i in range(3)]

    def step(make):
        f1, f2 = _cuda(f1n).requires_grad_(True), _cuda(f2n).requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        blk = make(f1, f2)
        loss, outs = 0.0, []
        for c, go in zip(cs, gos):
            outs.append(blk(c))   # kept alive through the backward, as a training step's per-iteration outputs are
            loss = loss + (outs[-1] * go).sum()
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(DEV) - base
        assert f1.grad is not None and f2.grad is not None and len(outs) == 3
        return peak

    alt = step(lambda a, b: eraft_amd.AlternateCorrBlock(a, b, num_levels=L, radius=r, trainable=True))
    vol = step(lambda a, b: eraft_amd.CorrBlock(a, b, num_levels=L, radius=r, differentiable=True))
    n, nb = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_alt_size(B, D, H, W, L, ctypes.byref(n)), "size")
    _lib.check(_lib.lib().ecorr_alt_backward_workspace_size(B, H, W, L, r, ctypes.byref(nb)), "workspace size")
    out_bytes = 4 * B * C * H * W
    terms = {
        "features + gradient features (2 x ecorr_alt_size)": 2 * 4 * n.value,
        "backward workspace": nb.value,
        "3 lookup outputs": 3 * out_bytes,
        "one out * go product (forward) or upstream gradient (backward) in flight": out_bytes,
        "fmap gradients": 2 * 4 * B * D * H * W,
        "slack": 1 << 20,
    }
    # (the coords and the loss weights go_i exist before the step and are not part of its peak)
    bound = sum(terms.values())
    print(f"peak {alt / 2**20:.2f} MB, bound {bound / 2**20:.2f} MB "
          f"({', '.join(f'{k} {v / 2**20:.2f}' for k, v in terms.items())}); CorrBlock(differentiable=True) "
          f"{vol / 2**20:.2f} MB, ratio {alt / vol:.3f}")
    assert alt <= bound
    assert alt < vol


# ---------------------------------------------------------------------------------------------
# 9. the network
# ---------------------------------------------------------------------------------------------
def _fnet_grads_alt():
    """test_grad_gpu._fnet_grads' inputs, loss and mode with ERAFT(train_alternate_corr=True)."""
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict
    net = nw.ERAFT({"subtype": "standard"}, n_first_channels=15, train_alternate_corr=True)
    net.load_state_dict(make_state_dict(net.state_dict()))
    net = net.cuda().train()
    net.freeze_bn()
    im1 = torch.from_numpy(prng.normal(3000, (1, 15, 128, 160))).cuda()
    im2 = torch.from_numpy(prng.normal(3001, (1, 15, 128, 160))).cuda()
    _, preds = net(im1, im2, iters=3)
    loss = sum(p.abs().mean() for p in preds)
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().double().cpu().numpy() for n, p in net.fnet.named_parameters()}


def test_eraft_fnet_grads():
    """fnet's gradients through the volume-free backward are as close to the fp64-correlation network's
    as the reference's own fp32 op sequence is, within 4x (test_grad_gpu.test_eraft_fnet_grads' bar and
    reasoning: two independent fp32 roundings amplified by the same GRU)."""
    _need_gpu()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    from test_grad_gpu import _fnet_grads
    from torch_ref import TorchCpuCorrBlock

    class Corr64(TorchCpuCorrBlock):   # the reference's op sequence with the volume in fp64
        def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
            super().__init__(fmap1.double(), fmap2.double(), num_levels, radius)

        def __call__(self, coords):
            return super().__call__(coords.double())

    ours = _fnet_grads_alt()
    g64 = _fnet_grads(Corr64, False)
    g32 = _fnet_grads(TorchCpuCorrBlock, False)
    assert set(ours) == set(g64)
    for n, g in ours.items():
        assert np.isfinite(g).all(), n
        assert np.any(g != 0), n

    def dist(a):   # normwise over all fnet parameters
        num = sum(float(np.sum((a[n] - g64[n]) ** 2)) for n in g64)
        den = sum(float(np.sum(g64[n] ** 2)) for n in g64)
        return (num / den) ** 0.5

    floor, mine = dist(g32), dist(ours)
    print(f"fnet gradients vs fp64-correlation network: reference ops in fp32 {floor:.3g} (the floor), "
          f"train_alternate_corr {mine:.3g} (ratio {mine / floor:.2f})")
    assert mine <= 4 * floor
