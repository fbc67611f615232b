"""Flow output side on MI355X: convex upsampling and the DSEC 16-bit PNG codec.

    up = upsample_flow(flow, mask)           # ERAFT.upsample_flow, model/eraft.py:74-85
    png = flow_to_png16(flow)                # the array visualize_flow_submission writes,
                                             #   utils/visualization.py:75-93
    flow, valid = flow_16bit_to_float(png)   # utils/dsec_utils.py:66-83

One HIP launch each (upsample.hip).  upsample_flow agrees with the reference within a few ulp
(device expf) and is differentiable (two more launches in its backward); the codec is bit-exact.
No CPU path: inputs must be HIP tensors.
"""
import torch

from . import _lib
from ._lib import require_device


def _aligned16(t):
    """t (contiguous) at a 16-byte aligned address: itself, or a copy where it is a view at a storage
    offset that is no multiple of 4 floats.  The kernels access out and grad_out as 16-byte vectors and
    the C ABI refuses a misaligned one (ECORR_EINVAL).  The forward's out is allocated here, so aligned;
    a caller-visible output, if one is ever passed in, needs the same treatment."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _upsample(flow, mask):
    """The ecorr_upsample_flow launch on contiguous flow [N, 2, H, W] and mask (N * 576 * H * W elements)."""
    N, _, H, W = flow.shape
    with _lib.on_device(flow.device):
        out = torch.empty((N, 2, 8 * H, 8 * W), dtype=torch.float32, device=flow.device)   # the allocator aligns it
        _lib.check(_lib.lib().ecorr_upsample_flow(flow.data_ptr(), mask.data_ptr(), N, H, W, out.data_ptr(),
                                                  _lib.stream_of(flow)), "upsample_flow")
    return out


class _UpsampleFn(torch.autograd.Function):
    """upsample_flow with gradients for flow and mask (ecorr_upsample_flow_backward): the forward is
    the plain launch; the backward recomputes the softmax from the saved inputs."""

    @staticmethod
    def forward(ctx, flow, mask):
        ctx.save_for_backward(flow, mask)   # versioned: an in-place change before backward raises
        return _upsample(flow.contiguous(), mask.contiguous())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        flow, mask = ctx.saved_tensors
        N, _, H, W = flow.shape
        go = _aligned16(grad_out.contiguous())   # ImagePadder.unpad: the gradient of a slice
        fc, mc = flow.contiguous(), mask.contiguous()
        need_flow, need_mask = ctx.needs_input_grad
        with _lib.on_device(fc.device):
            ws = _lib.scratch("ecorr_upsample_backward_workspace_size", N, H, W, device=fc.device,
                              what="upsample_flow backward")
            g_flow = torch.empty((N, 2, H, W), dtype=torch.float32, device=fc.device) if need_flow else None
            g_mask = torch.empty(mask.shape, dtype=torch.float32, device=fc.device) if need_mask else None
            _lib.check(_lib.lib().ecorr_upsample_flow_backward(
                go.data_ptr(), fc.data_ptr(), mc.data_ptr(), N, H, W, _lib.ptr(g_flow), _lib.ptr(g_mask),
                _lib.ptr(ws), _lib.stream_of(fc)), "upsample_flow backward")
        return g_flow, g_mask


def upsample_flow(flow, mask):
    """eraft.py:74-85: flow [N, 2, H, W], mask [N, 576, H, W] -> [N, 2, 8H, 8W].  Differentiable in
    both inputs (ecorr_upsample_flow_backward; deterministic, first order only); with grad mode off, or
    when neither input requires grad, it is the plain launch.  Either way the values are the same bits."""
    require_device("flow", flow)
    require_device("mask", mask)
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise RuntimeError(f"flow must be [N, 2, H, W], got {tuple(flow.shape)}")
    N, _, H, W = flow.shape
    if mask.numel() != N * 576 * H * W:   # the reference's mask.view(N, 1, 9, 8, 8, H, W)
        raise RuntimeError(f"shape '[{N}, 1, 9, 8, 8, {H}, {W}]' is invalid for input of size {mask.numel()}")
    if torch.is_grad_enabled() and (flow.requires_grad or mask.requires_grad):
        return _UpsampleFn.apply(flow, mask)
    return _upsample(flow.contiguous(), mask.contiguous())


def flow_to_png16(flow):
    """visualization.py:81-84: flow [2, h, w] (or [B, 2, h, w]) -> uint16 [h, w, 3] ([B, h, w, 3]):
    rint(flow * 128 + 2^15) cast like numpy's astype(uint16), channel 2 = 0."""
    require_device("flow", flow)
    single = flow.dim() == 3
    f = flow.unsqueeze(0) if single else flow
    if f.dim() != 4 or f.shape[1] != 2:
        raise RuntimeError(f"flow must be [2, h, w] or [B, 2, h, w], got {tuple(flow.shape)}")
    f = f.contiguous()
    B, _, h, w = f.shape
    with _lib.on_device(f.device):
        out = torch.empty((B, h, w, 3), dtype=torch.uint16, device=f.device)
        _lib.check(_lib.lib().ecorr_flow_to_png16(f.data_ptr(), B, h, w, out.data_ptr(), _lib.stream_of(f)),
                   "flow_to_png16")
    return out[0] if single else out


def flow_16bit_to_float(flow_16bit):
    """dsec_utils.py:66-83: uint16 [h, w, 3] -> (flow [h, w, 2] float32, valid [h, w] bool).
    The reference returns float64; every value (v - 2^15) / 128 is exact in float32.  Raises
    AssertionError where the reference asserts (dtype, shape, channel 2 outside {0, 1}).  Not capturable
    (the channel-2 flag is read on the host): under a graph capture it raises RuntimeError."""
    _lib.refuse_capture("flow_16bit_to_float")
    if not isinstance(flow_16bit, torch.Tensor):
        raise TypeError("flow_16bit must be a torch.Tensor")
    assert flow_16bit.dtype == torch.uint16
    assert flow_16bit.dim() == 3
    h, w, c = flow_16bit.shape
    assert c == 3
    require_device("flow_16bit", flow_16bit, torch.uint16)
    src = flow_16bit.contiguous()
    dev = src.device
    with _lib.on_device(dev):
        flow = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
        valid = torch.empty((h, w), dtype=torch.bool, device=dev)
        bad = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().ecorr_png16_to_flow(src.data_ptr(), 1, h, w, flow.data_ptr(), valid.data_ptr(),
                                                  bad.data_ptr(), _lib.stream_of(src)), "flow_16bit_to_float")
        assert int(bad.item()) == 0, "flow_16bit: invalid pixels must have channel 2 == 0"
    return flow, valid
