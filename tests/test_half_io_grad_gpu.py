"""Gradients with 16-bit fmaps in and a 16-bit convc1 output out (CorrBlock(..., differentiable=True,
fmap_dtype=...), lookup_conv1x1_relu(..., out_dtype=...)).  No 16-bit backward kernel exists: both run
the fp32 backward on exact conversions, so every comparison here is bitwise.

Shape 16 x 20, B = 1, D = 256, 4 levels, radius 4, 2 lookups per block.
  fmap gradients  16-bit leaf fmaps through the 16-bit block against the same leaves through
                  CorrBlock(f.float(), g.float(), differentiable=True), where autograd's own .float() node
                  casts the fp32 gradient to the leaf's dtype: equal bits, dtype of the leaf.
  convc1          lookup_conv1x1_relu(out_dtype=dt) in training against the fp32-output call under
                  grad_out values exactly representable in dt.  The 16-bit call masks with its saved
                  16-bit output, so the two agree bitwise unless a positive fp32 output rounds to 0 in
                  16 bits -- asserted absent, not skipped."""
import pytest
import torch

import prng

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
B, D, H, W, L, R, O = 1, 256, 16, 20, 4, 4, 64
NLOOK = 2


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _cuda(a):
    return torch.from_numpy(a).to(DEV)


def _coords(i):
    return _cuda(prng.coords_with_flow(1210 + i, B, H, W, 2.0))


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    ia = a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32)
    assert bool(torch.isfinite(a.float()).all()) and bool((a != 0).any()), f"{what}: not finite or all zero"
    bad = int((ia != ib).sum())
    assert bad == 0, f"{what}: {bad} of {ia.numel()} elements differ"


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_fmap_grads_equal_the_float_blocks(ea, dt):
    f0 = _cuda(prng.normal(1201, (B, D, H, W))).to(dt)
    g0 = _cuda(prng.normal(1202, (B, D, H, W))).to(dt)
    gos = [_cuda(prng.normal(1220 + i, (B, L * (2 * R + 1) ** 2, H, W), 0.01)) for i in range(NLOOK)]

    def run(half):
        f, g = f0.clone().requires_grad_(True), g0.clone().requires_grad_(True)
        if half:
            blk = ea.CorrBlock(f, g, num_levels=L, radius=R, differentiable=True, fmap_dtype=dt)
        else:
            blk = ea.CorrBlock(f.float(), g.float(), num_levels=L, radius=R, differentiable=True)
        outs = [blk(_coords(i)) for i in range(NLOOK)]
        sum((o * go).sum() for o, go in zip(outs, gos)).backward()
        torch.cuda.synchronize()
        return f.grad, g.grad, outs

    f16, g16, o16 = run(True)
    f32, g32, o32 = run(False)
    for a, b in zip(o16, o32):   # the forward: the same pyramid, the same lookups
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert f16.dtype == dt and g16.dtype == dt
    _same_bits(f16, f32, "fmap1.grad")
    _same_bits(g16, g32, "fmap2.grad")


@pytest.mark.parametrize("mode", ["split", "fused"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_convc1_training_grads_equal_the_fp32_output_calls(ea, dt, mode):
    f0 = _cuda(prng.normal(1231, (B, D, H, W)))
    g0 = _cuda(prng.normal(1232, (B, D, H, W)))
    w0 = _cuda(prng.normal(1233, (O, L * (2 * R + 1) ** 2, 1, 1), 0.05))
    b0 = _cuda(prng.normal(1234, (O,), 0.5))
    # grad_out exactly representable in dt
    gos = [_cuda(prng.normal(1240 + i, (B, O, H, W), 0.01)).to(dt).float() for i in range(NLOOK)]

    def run(out_dtype):
        f, g = f0.clone().requires_grad_(True), g0.clone().requires_grad_(True)
        w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        blk = ea.CorrBlock(f, g, num_levels=L, radius=R, differentiable=True)
        kw = {} if out_dtype is None else {"out_dtype": out_dtype}
        outs = [blk.lookup_conv1x1_relu(_coords(i), w, b, mode=mode, **kw) for i in range(NLOOK)]
        sum((o.float() * go).sum() for o, go in zip(outs, gos)).backward()
        torch.cuda.synchronize()
        return (f.grad, g.grad, w.grad, b.grad), outs

    g16, o16 = run(dt)
    g32, o32 = run(None)
    for a, b in zip(o16, o32):
        assert a.dtype == dt and a.requires_grad and b.dtype == torch.float32
        # the precondition of bitwise equal masks: no positive fp32 output rounds to 0
        assert not bool(((b > 0) & (b.to(dt) == 0)).any()), "a positive fp32 output rounds to 0: choose other values"
        assert torch.equal(a.detach().view(torch.int16), b.detach().to(dt).view(torch.int16))
        assert bool((b == 0).any()) and bool((b > 0).any())   # the mask has both values
    for name, a, b in zip(("fmap1.grad", "fmap2.grad", "weight.grad", "bias.grad"), g16, g32):
        assert a.dtype == torch.float32
        _same_bits(a, b, f"{mode} {name}")
