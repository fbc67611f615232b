"""A differentiable CorrBlock with a 16-bit lookup output: the forward is the same launch with the
16-bit store, the backward converts the incoming gradient with .float() and runs the fp32 backward
(ecorr_lookup_backward, ecorr_build_backward).  So the fmap gradients of `corr_fn(c, out_dtype=dt)`
under a 16-bit gradient g must be bitwise those of an identical block called in fp32 under g.float():
both feed the same fp32 values to the same deterministic kernels."""
import pytest
import torch

import prng

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, D, H, W = 2, 8, 18, 16   # 288 queries: 4.5 query blocks, every level width even


def _leaves():
    f1 = torch.from_numpy(prng.normal(841, (B, D, H, W))).to(DEV).requires_grad_(True)
    f2 = torch.from_numpy(prng.normal(842, (B, D, H, W))).to(DEV).requires_grad_(True)
    return f1, f2


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_half_lookup_gradients_are_the_fp32_blocks(dt):
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    coords = torch.from_numpy(prng.coords_with_flow(843, B, H, W, 2.0)).to(DEV)
    g = torch.from_numpy(prng.normal(844, (B, 324, H, W))).to(DEV).to(dt)   # a 16-bit gradient

    f1, f2 = _leaves()
    out = eraft_amd.CorrBlock(f1, f2, differentiable=True)(coords, out_dtype=dt)
    assert out.dtype == dt and out.requires_grad
    out.backward(g)

    r1, r2 = _leaves()
    ref = eraft_amd.CorrBlock(r1, r2, differentiable=True)(coords)
    assert ref.dtype == torch.float32
    ref.backward(g.float())

    assert torch.equal(out.detach().view(torch.int16), ref.detach().to(dt).view(torch.int16))
    for name, a, b in (("fmap1", f1.grad, r1.grad), ("fmap2", f2.grad, r2.grad)):
        assert a is not None and a.dtype == torch.float32
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name} gradient differs from the fp32 block's"
