"""SepConvGRU on MI355X (csrc/gru.hip): the update block's separable ConvGRU, model/update.py:33-60.

    h = sepconv_gru(h, x, gru)      # gru: any module with convz1 convr1 convq1 convz2 convr2 convq2
    h = sepconv_gru_train(h, x, gru)    # the same forward, differentiable in h, x and the twelve parameters

Four HIP launches (z|r and q of the 1x5 half-step, then of the 5x1 half-step) on the fp32 matrix
instruction, reading h and x in place; the gate activations and the blend run in the kernels'
epilogues.  fp32, hidden 128 / input 256.  sepconv_gru is forward only; sepconv_gru_train adds the HIP backward
(csrc/gru_grad.hip, ecorr_sepconv_gru_backward), which keeps h and x and recomputes the gates.  No CPU path:
inputs must be HIP tensors.
"""
import ctypes
import weakref

import torch

from . import _lib
from ._lib import require_device

CONVS = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")   # the order of ecorr_sepconv_gru_pack

# gru module -> (the 12 parameter tensors, (hidden, input) and their (data_ptr, version) pairs, packed, the
# event recorded after the pack launch, the pack's stream).  As _lib.packed_conv1x1_weight: the key holds each
# tensor's identity, storage pointer and version counter, so an optimizer step, load_state_dict or .to()
# repacks; a change through .data that keeps all three is not seen.  Unlike that cache this one outlives a
# forward, so a call on another stream than the pack's first waits for the pack's event, and a pack is
# refused under a graph capture (its buffer would belong to the graph's private pool).
_packs = weakref.WeakKeyDictionary()
_packs_t = weakref.WeakKeyDictionary()   # the backward's transposed pack: a second entry under the same stamp


def _params(gru):
    ts = []
    for name in CONVS:
        conv = getattr(gru, name)
        if conv.bias is None:
            raise RuntimeError(f"sepconv_gru: {name} has no bias")
        ts.append(conv.weight)
    return ts + [getattr(gru, name).bias for name in CONVS]


def packed_weights(gru, hidden, inp, st, transposed=False):
    """The packed weights of `gru` for the current stream st (ecorr_sepconv_gru_pack), cached on the module;
    transposed: the backward's pack (ecorr_sepconv_gru_backward_pack), cached beside it.
    (hidden, inp) must be sizes the library supports (sepconv_gru checks them first)."""
    ts = _params(gru)
    cache = _packs_t if transposed else _packs
    stamp = [(hidden, inp)] + [(t.data_ptr(), _lib.tensor_version(t)) for t in ts]
    ent = cache.get(gru)
    if ent is not None and all(a is b for a, b in zip(ent[0], ts)) and ent[1] == stamp:
        # packed on another stream: this one runs after the pack and keeps the buffer from an early reuse
        # (not under a capture, which may not wait for outside work: torch synchronizes the device before a
        # capture begins, so the pack is complete by then)
        if ent[4] != st.value and not torch.cuda.is_current_stream_capturing():
            cur = torch.cuda.current_stream(ent[2].device)
            cur.wait_event(ent[3])
            ent[2].record_stream(cur)
        return ent[2]
    dev = ts[0].device
    cin = hidden + inp
    for name, wt, bs in zip(CONVS, ts[:6], ts[6:]):
        require_device(f"{name}.weight", wt)
        require_device(f"{name}.bias", bs)
        if wt.device != dev or bs.device != dev:
            raise RuntimeError("sepconv_gru: the gru's parameters are on different devices")
        taps = (1, 5) if name.endswith("1") else (5, 1)
        if tuple(wt.shape) != (hidden, cin) + taps or bs.numel() != hidden:
            raise RuntimeError(f"sepconv_gru: {name}.weight is {tuple(wt.shape)}, expected {(hidden, cin) + taps} "
                               f"with {hidden} biases")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("sepconv_gru: the gru's weights are not packed yet (or have changed) and a graph capture "
                           "is under way: call sepconv_gru once outside the captured region first")
    keep = [t.detach().contiguous() for t in ts]   # alive until the pack is enqueued (stream-ordered release)
    wp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in keep[:6]])
    if transposed:
        packed = _lib.scratch("ecorr_sepconv_gru_backward_packed_size", hidden, inp, device=dev,
                              what="sepconv_gru transposed weight pack")
        _lib.check(_lib.lib().ecorr_sepconv_gru_backward_pack(wp, hidden, inp, packed.data_ptr(), st),
                   "sepconv_gru transposed weight pack")
    else:
        packed = _lib.scratch("ecorr_sepconv_gru_packed_size", hidden, inp, device=dev, what="sepconv_gru weight pack")
        bp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in keep[6:]])
        _lib.check(_lib.lib().ecorr_sepconv_gru_pack(wp, bp, hidden, inp, packed.data_ptr(), st),
                   "sepconv_gru weight pack")
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    cache[gru] = (ts, stamp, packed, done, st.value)
    return packed


def sepconv_gru(h, x, gru):
    """update.py:47-60: h [B, 128, H, W], x [B, 256, H, W] (contiguous fp32 HIP tensors) -> the new h, a
    fresh fp32 tensor.  gru: a module with the reference's six convolutions (network.SepConvGRU, or the
    reference's own class); its weights are packed once and repacked when they change.  Other (hidden, input)
    sizes raise ValueError, before the weights are looked at.  Forward only: with grad mode on, an input or
    weight that requires grad raises RuntimeError.  Streams: everything runs on the current stream; the cached
    pack is ordered for a later call on another stream by an event.  Graph capture: call it once outside the
    capture first (a pack under capture raises); a replay keeps the pack it was captured with."""
    hidden, inp, ts = _checked(h, x, gru)
    _lib.no_grad_inputs(h, x, *ts, what="sepconv_gru (ERAFT hip_gru=True)")
    return _forward(h, x, gru, hidden, inp, ts)


def _checked(h, x, gru):
    """The argument checks of both entries, up to the sizes (ValueError before the weights are looked at)
    -> (hidden, input, the 12 parameters)."""
    require_device("h", h)
    require_device("x", x)
    if h.dim() != 4 or x.dim() != 4 or h.shape[0] != x.shape[0] or h.shape[2:] != x.shape[2:]:
        raise RuntimeError(f"sepconv_gru: h {tuple(h.shape)} and x {tuple(x.shape)} are not [B, hidden, H, W] and "
                           "[B, input, H, W] of one batch and image size")
    if h.device != x.device:
        raise RuntimeError("sepconv_gru: h and x are on different devices")
    if not h.is_contiguous() or not x.is_contiguous():
        raise RuntimeError("sepconv_gru: h and x must be contiguous")
    hidden, inp = h.shape[1], x.shape[1]
    size = ctypes.c_int64()   # the sizes the kernels are built for: ECORR_EINVAL -> ValueError, whatever gru holds
    _lib.check(_lib.lib().ecorr_sepconv_gru_packed_size(hidden, inp, ctypes.byref(size)),
               f"sepconv_gru: hidden {hidden}, input {inp}")
    return hidden, inp, _params(gru)


def _forward(h, x, gru, hidden, inp, ts):
    if ts[0].device != h.device:
        raise RuntimeError("sepconv_gru: the gru's parameters are on a different device than h")
    B, _, H, W = h.shape
    with _lib.on_device(h.device):
        st = _lib.stream_of(h)
        packed = packed_weights(gru, hidden, inp, st)
        ws = _lib.scratch("ecorr_sepconv_gru_workspace_size", B, hidden, inp, H, W, device=h.device,
                          what="sepconv_gru")
        out = torch.empty_like(h)
        _lib.check(_lib.lib().ecorr_sepconv_gru(h.data_ptr(), x.data_ptr(), B, hidden, inp, H, W, packed.data_ptr(),
                                                out.data_ptr(), _lib.ptr(ws), st), "sepconv_gru")
    return out


class _GruFn(torch.autograd.Function):
    """(h, x, the 12 parameters) -> h'; the forward is sepconv_gru's, the backward ecorr_sepconv_gru_backward."""

    @staticmethod
    def forward(ctx, h, x, gru, *ts):
        ctx.gru = gru
        ctx.save_for_backward(h, x, *ts)   # versioned: an in-place change before backward raises
        return _forward(h, x, gru, h.shape[1], x.shape[1], ts)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        h, x, *ts = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_w = any(need[3:])   # the library computes the twelve or none
        go = grad_out.float().contiguous()
        B, hidden, H, W = h.shape
        inp = x.shape[1]
        dev = h.device
        with _lib.on_device(dev):
            st = _lib.stream_of(h)
            packed = packed_weights(ctx.gru, hidden, inp, st)
            packed_t = packed_weights(ctx.gru, hidden, inp, st, transposed=True)
            ws = _lib.scratch("ecorr_sepconv_gru_backward_workspace_size", B, hidden, inp, H, W, device=dev,
                              what="sepconv_gru backward")
            gh = torch.empty_like(h) if need[0] else None
            gx = torch.empty_like(x) if need[1] else None
            gs = [torch.empty(t.shape, dtype=torch.float32, device=dev) for t in ts] if want_w else None
            gw = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in gs[:6]]) if want_w else None
            gb = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in gs[6:]]) if want_w else None
            _lib.check(_lib.lib().ecorr_sepconv_gru_backward(
                h.data_ptr(), x.data_ptr(), go.data_ptr(), B, hidden, inp, H, W, packed.data_ptr(),
                packed_t.data_ptr(), _lib.ptr(gh), _lib.ptr(gx), gw, gb, _lib.ptr(ws), st), "sepconv_gru backward")
        grads = [g if n else None for g, n in zip(gs, need[3:])] if want_w else [None] * 12
        return (gh, gx, None, *grads)


def sepconv_gru_train(h, x, gru):
    """sepconv_gru with a gradient: the same arguments, checks and forward launches (bitwise the same h'), and,
    with grad mode on and h, x or a parameter of gru requiring grad, a node whose backward is the HIP backward
    (csrc/gru_grad.hip; first order).  Under torch.no_grad(), or when nothing requires grad, it is sepconv_gru.
    The node keeps h, x and the parameters (all inputs: no copy) and recomputes the gates in its backward; an
    in-place change of one of them before backward raises, as in autograd.  The gradients of the twelve
    parameters are computed together or, for a frozen gru, not at all."""
    hidden, inp, ts = _checked(h, x, gru)
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in (h, x, *ts))):
        return _forward(h, x, gru, hidden, inp, ts)
    return _GruFn.apply(h, x, gru, *ts)
