"""The backward of the convex upsampling (ecorr_upsample_flow_backward, csrc/upsample.hip; the
differentiable eraft_amd.upsample_flow) on the GPU.

Expected values: the reference expression (the body of ERAFT.upsample_flow) under autograd in fp64 on
the CPU, on tests/prng.py inputs, computed once per case.  Statistic: oracle.normwise_err, max |d| / rms.

Bars.  For grad_flow and grad_mask the test measures three distances to the fp64 gradients: ours,
ATen's fp32 autograd of the same expression on this GPU, and the forward kernel's own distance to the
fp64 forward (the gradient is built from the forward's __expf weights, so it cannot be better than
they are).  ours <= 2 max(ATen's, the forward's): two independent fp32 evaluations, the rule of
test_grad_edges_gpu.py, with a floor from code the backward shares with the forward.  At mask scale
<= 1 additionally ours <= 1e-5, the project's bar (ATen's own distance there: 1e-6 .. 2e-6 for
grad_mask, 1e-7 .. 5e-7 for grad_flow).  At the large-logit cases ATen's own grad_mask distance is
about 1.6e-5 in this statistic, so only the relative rule and finiteness apply.  The forward's own
distance, being a floor of those bars, is itself asserted: <= max(UPSAMPLE_TOL, 2 x ATen's fp32 forward).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import prng
from flow_cases import UPSAMPLE_TOL

pytestmark = pytest.mark.gpu

TOL = 1e-5
DEV = torch.device("cuda:0")
SENTINEL = 0x5A5AA5A5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # a copy: the cached cases are read-only


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _expr(flow, mask):
    from eraft_amd.network import ERAFT
    return ERAFT.upsample_flow(flow, mask)


# (N, H, W, mask scale); scale 45: the construction of test_flow_gpu.test_upsample_large_logits at spread 90
CASES = [(1, 1, 1, 1.0), (1, 1, 7, 1.0), (1, 6, 1, 1.0), (2, 3, 5, 1.0), (2, 17, 20, 0.5), (1, 60, 80, 0.5),
         (3, 7, 9, 20.0), (2, 12, 20, 45.0)]


def _mask(N, H, W, ms):
    seed = 7100 + 13 * H + W
    mask = prng.normal(seed, (N, 576, H, W), ms)
    if ms >= 45.0:   # per sub-pixel one tap near the max, the others ~ 2 ms lower, on the upper half of the map
        spread = 2.0 * ms
        m = mask.reshape(N, 9, 64, H, W)
        hot = prng.normal(seed + 1, (N, 1, 64, H, W), 1.0)
        pick = (np.abs(prng.normal(seed + 2, (N, 1, 64, H, W), 1.0)) * 9).astype(np.int64) % 9
        m[:, :, :, :H // 2] = np.where(np.arange(9)[None, :, None, None, None] == pick,
                                       hot, hot - spread + prng.normal(seed + 3, (N, 9, 64, H, W), 5.0))[:, :, :, :H // 2]
        mask = np.ascontiguousarray(m.reshape(N, 576, H, W).astype(np.float32))
    return mask


@functools.lru_cache(maxsize=None)
def _case(N, H, W, ms):
    """Inputs (fp32, read-only) and the fp64 CPU reference: (flow, mask, g, out64, gflow64, gmask64)."""
    flow = prng.normal(7000 + 13 * H + W, (N, 2, H, W), 3.0)
    mask = _mask(N, H, W, ms)
    g = prng.normal(7200 + 13 * H + W, (N, 2, 8 * H, 8 * W))
    f64 = torch.from_numpy(flow).double().requires_grad_(True)
    m64 = torch.from_numpy(mask).double().requires_grad_(True)
    out = _expr(f64, m64)
    out.backward(torch.from_numpy(g).double())
    arrs = (flow, mask, g, out.detach().numpy(), f64.grad.numpy(), m64.grad.numpy())
    for a in arrs:
        a.setflags(write=False)
    return arrs


def _backward_abi(g, flow, mask, want_flow=True, want_mask=True):
    """ecorr_upsample_flow_backward on device tensors -> (grad_flow, grad_mask) (None where not asked for)."""
    from eraft_amd import _lib
    N, _, H, W = flow.shape
    n = ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_upsample_backward_workspace_size(N, H, W, ctypes.byref(n)), "size")
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    gf = torch.empty_like(flow) if want_flow else None
    gm = torch.empty_like(mask) if want_mask else None
    _lib.check(_lib.lib().ecorr_upsample_flow_backward(
        g.data_ptr(), flow.data_ptr(), mask.data_ptr(), N, H, W, None if gf is None else gf.data_ptr(),
        None if gm is None else gm.data_ptr(), ws.data_ptr(), _stream()), "upsample backward")
    torch.cuda.synchronize()
    return gf, gm


@pytest.mark.parametrize("N,H,W,ms", CASES)
def test_values(N, H, W, ms):
    """1: both gradients against fp64, beside ATen's fp32 autograd and the forward kernel's own error."""
    import eraft_amd
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    flow, mask, g, out64, gf64, gm64 = _case(N, H, W, ms)
    f, m, go = _cuda(flow), _cuda(mask), _cuda(g)
    gf, gm = _backward_abi(go, f, m)
    fa, ma = f.clone().requires_grad_(True), m.clone().requires_grad_(True)
    out_aten = _expr(fa, ma)
    out_aten.backward(go)
    with torch.no_grad():
        e_fwd = oracle.normwise_err(eraft_amd.upsample_flow(f, m).cpu().numpy(), out64)
    # the forward is a floor of the bars below, so it is held to its own: the project's bar for the kernel,
    # or twice ATen's fp32 forward on the same inputs where that is further from fp64
    e_fwd_aten = oracle.normwise_err(out_aten.detach().cpu().numpy(), out64)
    print(f"upsample forward ({N},{H},{W}) mask scale {ms:g}: normwise vs fp64 ours {e_fwd:.3g}, ATen fp32 {e_fwd_aten:.3g}")
    assert e_fwd <= max(UPSAMPLE_TOL, 2.0 * e_fwd_aten), "forward"
    for name, ours, aten, ref in (("grad_flow", gf, fa.grad, gf64), ("grad_mask", gm, ma.grad, gm64)):
        ours = ours.cpu().numpy()
        e_ours = oracle.normwise_err(ours, ref)
        e_aten = oracle.normwise_err(aten.cpu().numpy(), ref)
        print(f"upsample backward ({N},{H},{W}) mask scale {ms:g} {name}: normwise vs fp64 ours {e_ours:.3g}, "
              f"ATen fp32 {e_aten:.3g}, forward kernel {e_fwd:.3g}")
        assert np.isfinite(ours).all(), name
        assert e_ours <= 2.0 * max(e_aten, e_fwd), name
        if ms <= 1.0:
            assert e_ours <= TOL, name


def test_through_autograd():
    """2: the Python API: same value bits, the C ABI's gradient bits, one-sided gradients, a sliced
    upstream, the version check, no double backward, no graph under no_grad."""
    import eraft_amd
    N, H, W, ms = 2, 17, 20, 0.5
    flow, mask, g, *_ = _case(N, H, W, ms)
    f, m, go = _cuda(flow), _cuda(mask), _cuda(g)
    plain = eraft_amd.upsample_flow(f, m)
    assert not plain.requires_grad
    want_f, want_m = _backward_abi(go, f, m)

    fr, mr = f.clone().requires_grad_(True), m.clone().requires_grad_(True)
    out = eraft_amd.upsample_flow(fr, mr)
    assert out.requires_grad
    assert torch.equal(out.detach().view(torch.int32), plain.view(torch.int32))
    out.backward(go)
    assert torch.equal(fr.grad.view(torch.int32), want_f.view(torch.int32))
    assert torch.equal(mr.grad.view(torch.int32), want_m.view(torch.int32))

    # one input requires grad: the other's .grad stays None, the computed one has the same bits
    fr, mr = f.clone().requires_grad_(True), m.clone()
    eraft_amd.upsample_flow(fr, mr).backward(go)
    assert mr.grad is None and torch.equal(fr.grad.view(torch.int32), want_f.view(torch.int32))
    fr, mr = f.clone(), m.clone().requires_grad_(True)
    eraft_amd.upsample_flow(fr, mr).backward(go)
    assert fr.grad is None and torch.equal(mr.grad.view(torch.int32), want_m.view(torch.int32))

    # a non-contiguous upstream: the loss on a slice (ImagePadder.unpad) = the upstream zero outside it
    gs = torch.zeros_like(go)
    gs[..., 3:, 5:] = go[..., 3:, 5:]
    sf, sm = _backward_abi(gs, f, m)
    fr, mr = f.clone().requires_grad_(True), m.clone().requires_grad_(True)
    (eraft_amd.upsample_flow(fr, mr)[..., 3:, 5:] * go[..., 3:, 5:]).sum().backward()
    assert torch.equal(fr.grad.view(torch.int32), sf.view(torch.int32))
    assert torch.equal(mr.grad.view(torch.int32), sm.view(torch.int32))

    # an in-place change of a saved input before backward
    fr, mr = f.clone().requires_grad_(True), m.clone()
    out = eraft_amd.upsample_flow(fr, mr)
    mr.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward(go)

    # first order only
    fr, mr = f.clone().requires_grad_(True), m.clone().requires_grad_(True)
    out = eraft_amd.upsample_flow(fr, mr)
    (gfl,) = torch.autograd.grad(out, fr, go.clone().requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError):
        gfl.sum().backward()
    # a second backward through the same graph
    out = eraft_amd.upsample_flow(fr, mr)
    out.backward(go)
    with pytest.raises(RuntimeError):
        out.backward(go)

    with torch.no_grad():
        assert not eraft_amd.upsample_flow(fr, mr).requires_grad


def _padded(numel, pad, dtype=torch.float32):
    """A sentinel-filled buffer of pad + numel + pad elements and the pointer to its middle."""
    buf = torch.full((numel + 2 * pad,), SENTINEL, dtype=torch.int32, device=DEV).view(dtype)
    return buf, buf.data_ptr() + pad * buf.element_size()


@pytest.mark.parametrize("N,H,W", [(2, 17, 20), (1, 1, 1)])
def test_reproducible_and_in_place(N, H, W):
    """3: equal inputs give equal bits; nothing outside the exact extents of grad_flow, grad_mask and
    the workspace is written; a zero upstream gives zero gradients."""
    from eraft_amd import _lib
    flow, mask, g, *_ = _case(N, H, W, 0.5 if H > 1 else 1.0)
    f, m, go = _cuda(flow), _cuda(mask), _cuda(g)
    a_f, a_m = _backward_abi(go, f, m)
    b_f, b_m = _backward_abi(go, f, m)
    assert torch.equal(a_f.view(torch.int32), b_f.view(torch.int32))
    assert torch.equal(a_m.view(torch.int32), b_m.view(torch.int32))

    PAD = 1024
    n = ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_upsample_backward_workspace_size(N, H, W, ctypes.byref(n)), "size")
    assert n.value % 4 == 0
    bf, pf = _padded(f.numel(), PAD)
    bm, pm = _padded(m.numel(), PAD)
    bw, pw = _padded(n.value // 4, PAD)
    _lib.check(_lib.lib().ecorr_upsample_flow_backward(go.data_ptr(), f.data_ptr(), m.data_ptr(), N, H, W, pf, pm,
                                                       ctypes.c_void_p(pw), _stream()), "upsample backward")
    torch.cuda.synchronize()
    for buf, numel, want in ((bf, f.numel(), a_f), (bm, m.numel(), a_m), (bw, n.value // 4, None)):
        bits = buf.view(torch.int32)
        assert bool((bits[:PAD] == SENTINEL).all()) and bool((bits[PAD + numel:] == SENTINEL).all())
        if want is not None:   # and the extents themselves hold the gradients
            assert torch.equal(bits[PAD:PAD + numel], want.view(torch.int32).flatten())

    z_f, z_m = _backward_abi(torch.zeros_like(go), f, m)
    assert bool((z_f == 0).all()) and bool((z_m == 0).all())


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_logit_stays_local(bad):
    """4: one non-finite logit reaches the 9 taps of its sub-pixel in grad_mask and the 3 x 3
    neighbourhood of its pixel in grad_flow; every other element keeps the clean run's bits."""
    N, H, W = 1, 7, 9
    flow, mask, g, *_ = _case(3, H, W, 20.0)
    flow, mask, g = flow[:1], mask[:1] / 20.0, g[:1]
    k, i, j, h, w = 4, 3, 5, 2, 6
    f, m, go = _cuda(flow), _cuda(mask), _cuda(g)
    c_f, c_m = _backward_abi(go, f, m)
    assert bool(torch.isfinite(c_f).all()) and bool(torch.isfinite(c_m).all())
    m2 = m.clone()
    m2[0, k * 64 + i * 8 + j, h, w] = bad
    d_f, d_m = _backward_abi(go, f, m2)
    may_m = torch.zeros((N, 9, 8, 8, H, W), dtype=torch.bool, device=DEV)
    may_m[0, :, i, j, h, w] = True
    may_m = may_m.view(N, 576, H, W)
    may_f = torch.zeros((N, 2, H, W), dtype=torch.bool, device=DEV)
    may_f[:, :, h - 1:h + 2, w - 1:w + 2] = True
    for name, clean, dirty, may in (("grad_mask", c_m, d_m, may_m), ("grad_flow", c_f, d_f, may_f)):
        assert bool(torch.isfinite(dirty)[~may].all()), name
        assert torch.equal(dirty.view(torch.int32)[~may], clean.view(torch.int32)[~may]), name


def _net_grads(hip_upsample, upsample64):
    """Parameter gradients of sum mean |prediction| over 3 iterations, train() with frozen BN."""
    import eraft_amd.network as nw
    from e2e_weights import make_state_dict

    class Net(nw.ERAFT):
        if upsample64:   # the reference expression in fp64, cast back
            @staticmethod
            def upsample_flow(flow, mask):
                return nw.ERAFT.upsample_flow(flow.double(), mask.double()).float()

    net = Net({"subtype": "standard"}, 15, hip_upsample=hip_upsample, differentiable_corr=True)
    net.load_state_dict(make_state_dict(net.state_dict()))
    net = net.cuda().train()
    net.freeze_bn()
    im1 = torch.from_numpy(prng.normal(3000, (1, 15, 128, 160))).cuda()
    im2 = torch.from_numpy(prng.normal(3001, (1, 15, 128, 160))).cuda()
    _, preds = net(im1, im2, iters=3)
    loss = sum(p.abs().mean() for p in preds)
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().double().cpu().numpy() for n, p in net.named_parameters()
            if n.startswith(("fnet.", "cnet.", "update_block.")) and p.grad is not None}


def test_through_the_network():
    """5: ERAFT(hip_upsample=True, differentiable_corr=True) trains: its parameter gradients are as
    close to those of the network with the fp64 upsampling as the fp32 torch expression's are (within
    4x: two independent fp32 roundings amplified by the same GRU; test_eraft_fnet_grads' bar)."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    ours = _net_grads(True, False)
    g32 = _net_grads(False, False)
    g64 = _net_grads(False, True)
    assert set(ours) == set(g64) == set(g32)
    for prefix in ("fnet.", "cnet.", "update_block."):
        assert any(n.startswith(prefix) for n in ours), prefix
    for n, gr in ours.items():
        assert np.isfinite(gr).all(), n
    assert any(np.any(gr != 0) for n, gr in ours.items() if n.startswith("update_block.mask."))
    assert any(np.any(gr != 0) for n, gr in ours.items() if n.startswith("fnet."))

    def dist(a):   # normwise over all parameters
        num = sum(float(np.sum((a[n] - g64[n]) ** 2)) for n in g64)
        den = sum(float(np.sum(g64[n] ** 2)) for n in g64)
        return (num / den) ** 0.5

    floor, mine = dist(g32), dist(ours)
    print(f"parameter gradients vs the fp64-upsampling network: torch expression in fp32 {floor:.3g} (the floor), "
          f"ours {mine:.3g} (ratio {mine / floor:.2f})")
    assert mine <= 4 * floor
