"""The motion encoder's integer-exact set (tests/menc_exact.py), checked on the CPU.

tests/test_motion_enc_grad_gpu.py compares the HIP forward and backward with the fp64 reference cast to fp32, bit
for bit, on this set.  That rests on three claims, each shown here without a GPU, at the shapes the GPU test uses:
  - the certificate holds: in each of the 16 stages the absolute values of an element's terms sum to less than 2^24;
  - an independent fp32 summation order gives the reference's bits: fp32 ATen autograd on the CPU equals fp64
    autograd bitwise in the forward and in all ten gradients;
  - the comparison is not vacuous: every reference gradient is nonzero, about half of every ReLU layer is alive, and
    a reference whose conv weight gradient lost the last pixel of every item is rejected.
"""
import numpy as np
import pytest
import torch

import menc_exact as mx
from gpu_guard import mismatch
from grad_slab_rule import SLAB_SHAPES, assert_slab_shapes

SHAPES = SLAB_SHAPES + [(3, 9, 15), (2, 40, 50)]


def test_value_ranges():
    flow, c1, go = mx.inputs((3, 9, 15))
    assert set(np.unique(c1.numpy())) == {0.0, 1.0} and 0.45 < float(c1.mean()) < 0.55
    assert set(np.unique(flow.numpy())) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(np.unique(go.numpy())) == {-1.0, 0.0, 1.0} and go.shape[1] == 128
    from eraft_amd import network
    mod = mx.exact_module(network.BasicMotionEncoder())
    for name in mx.CONVS:
        w, b = getattr(mod, name).weight.detach().numpy(), getattr(mod, name).bias.detach().numpy()
        assert set(np.unique(w)) == {-1.0, 0.0, 1.0} and set(np.unique(b)) == {-1.0, 0.0, 1.0}, name
        want = 1.0 / mx.ONE_IN[name]
        assert 0.8 * want < float((w != 0).mean()) < 1.2 * want, name
        assert 0.5 < float((b != 0).mean()) < 0.8, name
    assert_slab_shapes()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_certificate_and_fp32_equals_fp64(shape):
    ref = mx.reference(shape)
    print(f"menc exact set {shape}: certificate worst {ref.worst:.4g} ({max(ref.cert, key=ref.cert.get)}) of 2^24 = "
          f"{mx.LIMIT:.4g}; alive {', '.join(f'{n} {a:.2f}' for n, a in ref.alive.items())}; nonzero grad_flow "
          f"{np.mean(ref.grads[0] != 0):.3f}, grad_c1 {np.mean(ref.grads[1] != 0):.3f}")
    assert len(ref.cert) == 16 and ref.worst < mx.LIMIT
    for n, a in ref.alive.items():
        assert 0.25 < a < 0.75, f"{n}: {a:.3f} of the layer is alive"
    for n, g in zip(mx.NAMES, ref.grads):
        assert np.any(g != 0), f"{n}: the reference gradient is identically zero"
    if shape[1] * shape[2] >= 1000:
        assert np.mean(ref.grads[0] != 0) > 0.9 and np.mean(ref.grads[1] != 0) > 0.9
    out32, grads32 = mx.autograd(ref.mod, ref.flow, ref.c1, ref.go, torch.float32)
    d = mismatch(out32.astype(np.float32), ref.out.astype(np.float32))
    assert d is None, f"forward, fp32 ATen against fp64: {d}"
    for n, a, r in zip(mx.NAMES, grads32, ref.grads):
        assert a.shape == r.shape
        d = mismatch(a.astype(np.float32).reshape(1, 1, -1), r.astype(np.float32).reshape(1, 1, -1))
        assert d is None, f"{n}, fp32 ATen against fp64: {d}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_comparison_rejects_a_dropped_pixel(shape):
    ref = mx.reference(shape)
    k = mx.NAMES.index("conv.weight")
    clean, wrong = ref.grads[k].astype(np.float32), ref.dropped.astype(np.float32)
    assert mismatch(clean.reshape(1, 1, -1), clean.reshape(1, 1, -1)) is None
    d = mismatch(wrong.reshape(1, 1, -1), clean.reshape(1, 1, -1))
    assert d is not None, "the bitwise comparison accepts a weight gradient without every item's last pixel"
    # only the four taps that see the bottom-right pixel from inside the image can change
    diff = (wrong != clean)
    assert diff[:, :, :2, :2].any() and not diff[:, :, 2, :].any() and not diff[:, :, :, 2].any()
