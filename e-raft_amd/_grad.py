"""The autograd scaffold of CorrBlock(differentiable=True) and AlternateCorrBlock(trainable=True), once.

Autograd never carries a block-sized tensor: the block's construction is a Function of the fmaps
returning a one-element handle (HandleFn), each lookup a Function of (handle, coords) (LookupFn) whose
backward adds its contribution into the block's one gradient buffer and returns a zero for the
handle; the handle's backward then runs once, after all of them, turns the buffer into the two fmap
gradients and frees it.  What they share is a GradState.  It references neither the block nor the
handle nor the pyramid (an argument of LookupFn.forward, never stored): the autograd graph holds no
cycle and keeps no pyramid alive.
"""
import torch

from . import _lib


class GradState:
    """Geometry, the gradient buffer `buf` of numel floats (allocated and zeroed by the first lookup
    backward, freed by the handle's) and the consumed flag of one live block.  Subclasses define:
        CONSUMED                          the message of a second backward
        lookup(source, coords, out_dtype) the forward lookup of contiguous coords in the block's `source`
        lookup_backward(grad, coords)     buf += the lookup's contribution, on the current stream
        saved(fmap1, fmap2)               the tensors the handle saves for fmap_backward (default: none)
        fmap_backward(buf, saved, g1, g2) buf -> the fp32 fmap gradients g1 / g2 (None: not needed)
    """

    def __init__(self, shape, levels, radius, device, numel):
        self.shape, self.levels, self.radius, self.device, self.numel = shape, levels, radius, device, numel
        self.buf = None
        self.consumed = False

    def saved(self, fmap1, fmap2):
        return ()

    def require_unconsumed(self):
        if self.consumed:
            raise RuntimeError(self.CONSUMED)

    def take(self):
        """The handle's backward: consumes the state; -> the buffer (None: no lookup received a gradient)."""
        self.require_unconsumed()
        self.consumed = True
        buf, self.buf = self.buf, None
        return buf

    def add_lookup_grad(self, grad, coords):
        """The one place a lookup's gradient enters the buffer: grad (contiguous fp32 [B, C, H, W]) at
        contiguous coords, on grad's current stream.  The caller holds the device (on_device) and returns
        the handle's gradient, a zero, itself: the lookup Functions make it at different points."""
        if self.buf is None:
            self.buf = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.lookup_backward(grad, coords)


class HandleFn(torch.autograd.Function):
    """(fmap1, fmap2) -> one-element handle; what the lookups read is a buffer of the block."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, state):
        ctx.state = state
        ctx.dtype = fmap1.dtype
        ctx.save_for_backward(*state.saved(fmap1, fmap2))
        return torch.zeros(1, dtype=torch.float32, device=state.device)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _grad_handle):
        st = ctx.state
        buf = st.take()
        saved = ctx.saved_tensors   # versioned: an in-place change of a saved fmap raises here
        needs = ctx.needs_input_grad[:2]
        with _lib.on_device(st.device):
            if buf is None:   # no lookup received a gradient
                z = [torch.zeros(st.shape, dtype=ctx.dtype, device=st.device) if n else None for n in needs]
                return z[0], z[1], None
            # the backward is fp32; 16-bit fmaps get the result cast once to their dtype, as autograd's
            # own .float() node would hand it back
            g1, g2 = (torch.empty(st.shape, dtype=torch.float32, device=st.device) if n else None for n in needs)
            st.fmap_backward(buf, saved, g1, g2)
            if ctx.dtype != torch.float32:
                g1 = None if g1 is None else g1.to(ctx.dtype)
                g2 = None if g2 is None else g2.to(ctx.dtype)
        return g1, g2, None


class LookupFn(torch.autograd.Function):
    """(handle, coords) -> the lookup; backward adds into the block's gradient buffer."""

    @staticmethod
    def forward(ctx, handle, coords, state, source, out_dtype):
        ctx.state = state
        ctx.save_for_backward(coords)   # versioned: an in-place change before backward raises
        return state.lookup(source, coords.contiguous(), out_dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        st = ctx.state
        st.require_unconsumed()
        (coords,) = ctx.saved_tensors
        go = grad_out.float().contiguous()   # a 16-bit lookup's gradient: the fp32 backward on its exact values
        cc = coords.contiguous()
        with _lib.on_device(st.device):
            st.add_lookup_grad(go, cc)
            return torch.zeros(1, dtype=torch.float32, device=st.device), None, None, None, None
