"""The motion encoder behind convc1 on MI355X (csrc/motion_enc.hip): BasicMotionEncoder's convc2, convf1, convf2
and conv with both concatenations, model/update.py:68-81.

    m = motion_encoder(flow, c1, enc)                  # c1 = relu(enc.convc1(corr)); m [B, 128, H, W]
    motion_encoder(flow, c1, enc, out=x[:, 128:])      # written into the upper half of the GRU's x [B, 256, H, W]
    m = motion_encoder_train(flow, c1, enc)            # the same forward, differentiable in flow, c1 and the 8 parameters

Four HIP launches: convf1 (7x7) on the VALU, convc2, convf2 and conv (3x3) on the fp32 matrix instruction reading
their shifted taps in place; channels 126 and 127 of the result are flow, bit for bit.  fp32.  motion_encoder is
forward only; motion_encoder_train adds the HIP backward (csrc/motion_enc_grad.hip, ecorr_motion_encoder_backward),
which keeps flow and c1 and recomputes the intermediates.  No CPU path: inputs must be HIP tensors.
"""
import ctypes
import weakref

import torch

from . import _lib
from ._lib import require_device

CONVS = ("convc2", "convf1", "convf2", "conv")   # the order of ecorr_motion_encoder_pack
SHAPES = {"convc2": (192, 256, 3, 3), "convf1": (128, 2, 7, 7), "convf2": (64, 128, 3, 3), "conv": (126, 256, 3, 3)}
C1, OUT = 256, 128

# encoder module -> (the 8 parameter tensors, their (data_ptr, version) pairs, packed, the event recorded after
# the pack launch, the pack's stream): gru.packed_weights' cache, for this pack
_packs = weakref.WeakKeyDictionary()
_packs_t = weakref.WeakKeyDictionary()   # the backward's transposed pack: a second entry under the same stamp


def _params(enc):
    ts = []
    for name in CONVS:
        conv = getattr(enc, name)
        if conv.bias is None:
            raise RuntimeError(f"motion_encoder: {name} has no bias")
        ts.append(conv.weight)
    return ts + [getattr(enc, name).bias for name in CONVS]


def packed_weights(enc, st, transposed=False):
    """The packed weights of `enc` for the current stream st (ecorr_motion_encoder_pack), cached on the module
    per weight version as gru.packed_weights does: an optimizer step, load_state_dict or .to() repacks.
    transposed: the backward's pack (ecorr_motion_encoder_backward_pack), cached beside it."""
    ts = _params(enc)
    cache = _packs_t if transposed else _packs
    stamp = [(t.data_ptr(), _lib.tensor_version(t)) for t in ts]
    ent = cache.get(enc)
    if ent is not None and all(a is b for a, b in zip(ent[0], ts)) and ent[1] == stamp:
        # packed on another stream: this one runs after the pack and keeps the buffer from an early reuse (not
        # under a capture: torch synchronizes the device before one begins, so the pack is complete by then)
        if ent[4] != st.value and not torch.cuda.is_current_stream_capturing():
            cur = torch.cuda.current_stream(ent[2].device)
            cur.wait_event(ent[3])
            ent[2].record_stream(cur)
        return ent[2]
    dev = ts[0].device
    for name, wt, bs in zip(CONVS, ts[:4], ts[4:]):
        require_device(f"{name}.weight", wt)
        require_device(f"{name}.bias", bs)
        if wt.device != dev or bs.device != dev:
            raise RuntimeError("motion_encoder: the encoder's parameters are on different devices")
        if tuple(wt.shape) != SHAPES[name] or bs.numel() != SHAPES[name][0]:
            raise RuntimeError(f"motion_encoder: {name}.weight is {tuple(wt.shape)}, expected {SHAPES[name]} "
                               f"with {SHAPES[name][0]} biases")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("motion_encoder: the encoder's weights are not packed yet (or have changed) and a graph "
                           "capture is under way: call motion_encoder once outside the captured region first")
    keep = [t.detach().contiguous() for t in ts]   # alive until the pack is enqueued (stream-ordered release)
    wp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in keep[:4]])
    if transposed:
        packed = _lib.scratch("ecorr_motion_encoder_backward_packed_size", device=dev,
                              what="motion_encoder transposed weight pack")
        _lib.check(_lib.lib().ecorr_motion_encoder_backward_pack(wp, packed.data_ptr(), st),
                   "motion_encoder transposed weight pack")
    else:
        bp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in keep[4:]])
        packed = _lib.scratch("ecorr_motion_encoder_packed_size", device=dev, what="motion_encoder weight pack")
        _lib.check(_lib.lib().ecorr_motion_encoder_pack(wp, bp, packed.data_ptr(), st), "motion_encoder weight pack")
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    cache[enc] = (ts, stamp, packed, done, st.value)
    return packed


def motion_encoder(flow, c1, enc, out=None):
    """update.py:75-81 behind convc1: flow [B, 2, H, W] and c1 = relu(enc.convc1(corr)) [B, 256, H, W]
    (contiguous fp32 HIP tensors) -> [B, 128, H, W]: relu(conv([relu(convc2(c1)), relu(convf2(relu(convf1(flow))))]))
    in channels 0-125, flow in 126-127.  enc: a network.BasicMotionEncoder (or the reference's class); only its
    parameters are read, packed once and repacked when they change.
    out: None (a fresh contiguous tensor is returned) or an fp32 [B, 128, H, W] view on the same device whose
    strides are (S, H W, W, 1) with S >= 128 H W -- e.g. x[:, 128:] of a contiguous [B, 256, H, W], the GRU's
    input; the result is written there and `out` returned.  Any other stride pattern raises ValueError; so does
    an `out` that overlaps an input.
    Forward only: with grad mode on, an input or weight that requires grad raises RuntimeError.  Streams and graph
    capture: as sepconv_gru (the current stream; call it once outside a capture first)."""
    ts = _checked(flow, c1, enc)
    _lib.no_grad_inputs(flow, c1, *ts, what="motion_encoder (ERAFT hip_motion_encoder=True)")
    return _forward(flow, c1, enc, ts, out)


def _checked(flow, c1, enc):
    """The argument checks of both entries -> the 8 parameters."""
    require_device("flow", flow)
    require_device("c1", c1)
    if (flow.dim() != 4 or c1.dim() != 4 or flow.shape[1] != 2 or c1.shape[1] != C1 or flow.shape[0] != c1.shape[0]
            or flow.shape[2:] != c1.shape[2:]):
        raise RuntimeError(f"motion_encoder: flow {tuple(flow.shape)} and c1 {tuple(c1.shape)} are not [B, 2, H, W] "
                           f"and [B, {C1}, H, W] of one batch and image size")
    if flow.device != c1.device:
        raise RuntimeError("motion_encoder: flow and c1 are on different devices")
    if not flow.is_contiguous() or not c1.is_contiguous():
        raise RuntimeError("motion_encoder: flow and c1 must be contiguous")
    return _params(enc)


def _forward(flow, c1, enc, ts, out=None):
    if ts[0].device != c1.device:
        raise RuntimeError("motion_encoder: the encoder's parameters are on a different device than c1")
    B, _, H, W = c1.shape
    if out is not None:
        require_device("out", out)
        if out.device != c1.device:
            raise RuntimeError("motion_encoder: out is on a different device than c1")
        if tuple(out.shape) != (B, OUT, H, W):
            raise ValueError(f"motion_encoder: out is {tuple(out.shape)}, expected {(B, OUT, H, W)}")
        S = out.stride(0) if B > 1 else OUT * H * W   # one item: its batch stride addresses nothing
        if not out[0].is_contiguous() or S < OUT * H * W:   # (a dimension of size 1 may carry any stride)
            raise ValueError(f"motion_encoder: out has strides {tuple(out.stride())}; expected (S, {H * W}, {W}, 1) "
                             f"with S >= {OUT * H * W}")
    with _lib.on_device(c1.device):
        st = _lib.stream_of(c1)
        packed = packed_weights(enc, st)
        ws = _lib.scratch("ecorr_motion_encoder_workspace_size", B, H, W, device=c1.device, what="motion_encoder")
        if out is None:
            out = torch.empty((B, OUT, H, W), dtype=torch.float32, device=c1.device)
            S = OUT * H * W
        _lib.check(_lib.lib().ecorr_motion_encoder(c1.data_ptr(), flow.data_ptr(), B, H, W, packed.data_ptr(),
                                                   out.data_ptr(), S, _lib.ptr(ws), st), "motion_encoder")
    return out


class _MencFn(torch.autograd.Function):
    """(flow, c1, the 8 parameters) -> out; the forward is motion_encoder's, the backward
    ecorr_motion_encoder_backward."""

    @staticmethod
    def forward(ctx, flow, c1, enc, *ts):
        ctx.enc = enc
        ctx.save_for_backward(flow, c1, *ts)   # versioned: an in-place change before backward raises
        return _forward(flow, c1, enc, ts)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        flow, c1, *ts = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_w = any(need[3:])   # the library computes the eight or none
        B, _, H, W = c1.shape
        dev = c1.device
        go = grad_out
        # (S, H W, W, 1) with S >= 128 H W goes as it is: the upper half of the GRU's grad_x, no copy
        S = go.stride(0) if B > 1 else OUT * H * W
        if go.dtype != torch.float32 or not go[0].is_contiguous() or S < OUT * H * W:
            go = go.float().contiguous()
            S = OUT * H * W
        with _lib.on_device(dev):
            st = _lib.stream_of(c1)
            packed = packed_weights(ctx.enc, st)
            packed_t = packed_weights(ctx.enc, st, transposed=True)
            ws = _lib.scratch("ecorr_motion_encoder_backward_workspace_size", B, H, W, device=dev,
                              what="motion_encoder backward")
            gf = torch.empty_like(flow) if need[0] else None
            gc = torch.empty_like(c1) if need[1] else None
            gs = [torch.empty(t.shape, dtype=torch.float32, device=dev) for t in ts] if want_w else None
            gw = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in gs[:4]]) if want_w else None
            gb = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in gs[4:]]) if want_w else None
            _lib.check(_lib.lib().ecorr_motion_encoder_backward(
                c1.data_ptr(), flow.data_ptr(), go.data_ptr(), S, B, H, W, packed.data_ptr(), packed_t.data_ptr(),
                _lib.ptr(gc), _lib.ptr(gf), gw, gb, _lib.ptr(ws), st), "motion_encoder backward")
        grads = [g if n else None for g, n in zip(gs, need[3:])] if want_w else [None] * 8
        return (gf, gc, None, *grads)


def motion_encoder_train(flow, c1, enc):
    """motion_encoder with a gradient: the same checks and the same four forward launches (bitwise the same result),
    and, with grad mode on and flow, c1 or a parameter of enc requiring grad, a node whose backward is the HIP backward
    (csrc/motion_enc_grad.hip; first order).  Under torch.no_grad(), or when nothing requires grad, it is the plain
    forward and builds no node.
    It always returns a fresh contiguous [B, 128, H, W] tensor and has no out=: writing into a reused x (as
    ERAFT(hip_motion_encoder=True) does) would overwrite what the GRU's node saved of the previous iteration for
    its backward.
    The node keeps flow, c1 and the parameters (all inputs: no copy) and recomputes f1, cor and flo in its backward;
    an in-place change of one of them before backward raises, as in autograd.  The gradients of the eight parameters
    are computed together or, for a frozen encoder, not at all.  A grad_out whose strides are (S, H W, W, 1) with
    S >= 128 H W -- the upper half of the GRU's grad_x -- is read in place."""
    ts = _checked(flow, c1, enc)
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in (flow, c1, *ts))):
        return _forward(flow, c1, enc, ts)
    return _MencFn.apply(flow, c1, enc, *ts)
