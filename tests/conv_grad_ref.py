"""fp64 references of ecorr_conv1x1_relu_backward (test infrastructure, numpy only).

For out = relu(bias[o] + sum_c W[o][c] in[b][c][p]) and an upstream gradient grad_out, with the mask
taken from the GIVEN out (the ABI's rule, ATen's threshold_backward: out <= 0 blocks, a NaN passes):
    gm          = where(out <= 0, 0, grad_out)
    grad_in     = einsum(oc,boq->bcq)(W, gm)
    grad_weight = einsum(boq,bcq->oc)(gm, in)
    grad_bias   = gm.sum over (b, q)
"""
import numpy as np


def masked(grad_out, out):
    return np.where(np.asarray(out) <= 0, 0.0, np.asarray(grad_out, dtype=np.float64))


def grads(grad_out, out, x, weight):
    """(grad_in [B, C, Q], grad_weight [O, C], grad_bias [O]) in fp64; x may be None (no grad_weight)."""
    gm = masked(grad_out, out)
    w = np.asarray(weight, dtype=np.float64).reshape(gm.shape[1], -1)
    gi = np.einsum("oc,boq->bcq", w, gm, optimize=True)
    gw = None if x is None else np.einsum("boq,bcq->oc", gm, np.asarray(x, dtype=np.float64), optimize=True)
    return gi, gw, gm.sum(axis=(0, 2))


def normwise(got, ref):
    """max |got - ref| / rms(ref): the project's normwise statistic (tests/test_conv_split_gpu.py)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / np.sqrt(np.mean(ref * ref)))


def aten_fp32_grads(grad_out, out, x, weight, device="cpu"):
    """ATen's own fp32 backward of conv1x1 for the same masked gradient (mask from the given out as
    above) on `device`: the yardstick of the grad_weight / grad_bias bars, max(1e-5, 2 x its distance
    to fp64).  The caller turns TF32 off on a GPU."""
    import torch
    import torch.nn.functional as F
    gm = torch.from_numpy(masked(grad_out, out).astype(np.float32)).to(device)
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    O = gm.shape[1]
    w = torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32).reshape(O, -1, 1)).to(device).requires_grad_(True)
    b = torch.zeros(O, dtype=torch.float32, device=device, requires_grad=True)
    y = F.conv1d(xt, w, b)
    y.backward(gm)
    return w.grad.reshape(O, -1).cpu().numpy(), b.grad.cpu().numpy()
