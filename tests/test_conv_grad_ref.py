"""The fp64 references of tests/conv_grad_ref.py against torch fp64 autograd of relu(conv1x1), on
inputs where no pre-activation is within 1e-3 of zero (there the mask from out and autograd's mask
from the pre-activation are the same set, so the two must agree to fp64 rounding)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as cg
import prng


@pytest.mark.parametrize("shape", [(2, 20, 37, 12), (1, 81, 70, 30), (3, 7, 1, 5)], ids=lambda s: "b%d_c%d_q%d_o%d" % s)
def test_refs_match_fp64_autograd(shape):
    B, C, Q, O = shape
    x = prng.normal(701, (B, C, Q)).astype(np.float64)
    w = (prng.normal(702, (O, C)) * np.float32(0.05)).astype(np.float64)
    b = (prng.normal(703, (O,)) * np.float32(0.1)).astype(np.float64)
    go = prng.normal(704, (B, O, Q)).astype(np.float64)
    # a query column with a pre-activation within 1e-3 of zero is nudged (channel 0) until it has none
    for _ in range(50):
        pre = np.einsum("oc,bcq->boq", w, x) + b[None, :, None]
        near = (np.abs(pre) < 1e-3).any(axis=1)   # [B, Q]
        if not near.any():
            break
        x[:, 0, :][near] += 0.37
    assert not (np.abs(pre) < 1e-3).any()
    out = np.maximum(pre, 0.0)
    assert (out > 0).any() and (out == 0).any()

    xt = torch.from_numpy(x).requires_grad_(True)
    wt = torch.from_numpy(w.reshape(O, C, 1)).requires_grad_(True)
    bt = torch.from_numpy(b).requires_grad_(True)
    y = F.relu(F.conv1d(xt, wt, bt))
    assert np.array_equal(y.detach().numpy() > 0, out > 0)
    y.backward(torch.from_numpy(go))

    gi, gw, gb = cg.grads(go, out, x, w)
    assert cg.normwise(gi, xt.grad.numpy()) <= 1e-12
    assert cg.normwise(gw, wt.grad.numpy().reshape(O, C)) <= 1e-12
    assert cg.normwise(gb, bt.grad.numpy()) <= 1e-12


def test_mask_rule_is_threshold_backward():
    """out <= 0 blocks (also -0.0 and negative values of a given out), a NaN out passes the gradient."""
    out = np.array([[[1.0, 0.0, -0.0, -2.0, np.nan]]])
    go = np.array([[[3.0, 4.0, 5.0, 6.0, 7.0]]])
    assert np.array_equal(cg.masked(go, out)[0, 0], [3.0, 0.0, 0.0, 0.0, 7.0])
    t = torch.ops.aten.threshold_backward(torch.from_numpy(go), torch.from_numpy(out), 0.0)
    assert np.array_equal(t.numpy(), cg.masked(go, out))


def test_aten_fp32_yardstick_is_close_to_fp64():
    B, C, Q, O = 2, 20, 300, 12
    x = prng.normal(711, (B, C, Q))
    w = prng.normal(712, (O, C)) * np.float32(0.05)
    go = prng.normal(713, (B, O, Q))
    out = np.maximum(prng.normal(714, (B, O, Q)), 0.0)
    _, gw, gb = cg.grads(go, out, x, w)
    aw, ab = cg.aten_fp32_grads(go, out, x, w)
    assert cg.normwise(aw, gw) <= 1e-5 and cg.normwise(ab, gb) <= 1e-5
