"""AlternateCorrBlock: CorrBlock's lookup without the all-pairs volume (RAFT's `alternate_corr`).

    corr_fn = AlternateCorrBlock(fmap1, fmap2, num_levels=4, radius=4)
    corr    = corr_fn(coords1)                               # [B, num_levels * (2r+1)^2, H, W]
    corr    = corr_fn(coords1, out_dtype=torch.float16)      # the same lookup, 16-bit elements
    corr_fn = AlternateCorrBlock(fmap1, fmap2, trainable=True)   # ... with gradients for the fmaps

The same function as CorrBlock(fmap1, fmap2, num_levels, radius)(coords) -- shape, channel order
(2r+1)^2 i + (2r+1) a + b, zeros padding and the align_corners=True round trip -- computed without the
volume: the block keeps only the feature maps (fmap1 and the pooled levels of fmap2, channel-last fp32,
ecorr_alt_pack_as) and every lookup computes the correlation values its samples need
(ecorr_alt_lookup_as, csrc/alt.hip).  avg_pool2d over the target axes is linear, so
level i of the volume is fmap1^T pool^i(fmap2) / sqrt(D); sample positions, NaN samples, exact zeros and
contributing corners are the volume lookup's by construction (the same device functions), the corner
values are fp32 dot products in another order: equal up to rounding, not bit for bit.  Memory grows
with Q = H W instead of Q^2 (DSEC, B = 16: 183 MB of features against a 1.96 GB pyramid); a lookup costs
far more time than the volume lookup's gather (README.md), so CorrBlock stays the right
choice wherever its pyramid fits.

The checks and messages are CorrBlock's.  By default the block is forward-only: fmaps or coords that
require grad while grad mode is on raise, and so do differentiable=True (CorrBlock's keyword: the
opt-in here is trainable=True), corr_pyramid (there is no volume) and lookup_conv1x1_relu (no fused
convc1).  D = 0 and empty shapes raise: there is no volume to be NaN.
fmap_dtype / out_dtype: as CorrBlock's (16-bit fmaps are read as they are, exactly; a 16-bit output is
the fp32 sample rounded once, bitwise corr_fn(coords).to(out_dtype)).  Deterministic (no atomics).

Training (opt-in): AlternateCorrBlock(fmap1, fmap2, num_levels, radius, trainable=True) accepts fmaps
that require grad and gives them gradients through every `corr_fn(coords)` lookup without a gradient
pyramid (csrc/alt_grad.hip): where a differentiable CorrBlock holds the pyramid and
one more pyramid-sized gradient buffer, this block holds the features, one feature-sized gradient
buffer and, during a lookup's backward, a workspace of the queries' window gradients.  The live rule
is CorrBlock's: the gradient path is live when trainable is set, grad mode is on and an fmap requires
grad; otherwise the block is the plain block (and without trainable, fmaps that require grad still
raise "forward-only").  The forward of a live block runs the same launches, so its values are bitwise
the plain block's.  Autograd structure as CorrBlock's (the handle mechanism of _grad.py), with the
gradient feature buffer in the gradient pyramid's place and each lookup saving only coords.  The
backward reads the block's own fp32 copy of the features, so no fmap is saved and an in-place change of an fmap after construction does
not affect (or invalidate) the backward: the gradients are those of the values the block was built
from.  Deterministic (no atomics).  Contract of the live block, as the differentiable CorrBlock's:
coords are detached (coords.requires_grad raises; there is no coordinate gradient), every level is at
least 2 x 2, one backward per block (a second one raises), first order only, single GPU.  With a
16-bit fmap_dtype the gradients are the fp32 result cast once to the fmaps' dtype; with a 16-bit
out_dtype the backward runs on grad_out.float().
"""
import torch

from . import _lib
from ._grad import GradState, HandleFn, LookupFn
from ._lib import check_coords


class _AltGradState(GradState):
    """The shared state of one trainable block (_grad.py): buf is the gradient feature buffer, laid out
    as the block's feature buffer feat, which the state keeps (the backward reads it; no fmap is saved)."""

    CONSUMED = ("eraft_amd AlternateCorrBlock: backward through a block whose gradient was already "
                "consumed (one backward per trainable block)")

    def __init__(self, shape, levels, radius, feat, device):
        super().__init__(shape, levels, radius, device, feat.numel())
        self.feat = feat

    def lookup(self, feat, coords, out_dtype):
        return _alt_lookup(feat, coords, self.shape, self.levels, self.radius, out_dtype)

    def lookup_backward(self, grad, coords):
        B, D, H, W = self.shape
        what = "AlternateCorrBlock lookup backward"
        ws = _lib.scratch("ecorr_alt_backward_workspace_size", B, H, W, self.levels, self.radius, device=self.device,
                          what=what)
        _lib.check(_lib.lib().ecorr_alt_lookup_backward(
            self.feat.data_ptr(), coords.data_ptr(), grad.data_ptr(), B, D, H, W, self.levels, self.radius,
            self.buf.data_ptr(), ws.data_ptr(), _lib.stream_of(grad)), what)

    def fmap_backward(self, gf, saved, g1, g2):
        B, D, H, W = self.shape
        _lib.check(_lib.lib().ecorr_alt_pack_backward(
            gf.data_ptr(), B, D, H, W, self.levels, _lib.ptr(g1), _lib.ptr(g2), _lib.stream_of(gf)),
            "AlternateCorrBlock pack backward")


def _alt_lookup(feat, coords, shape, levels, radius, out_dtype):
    """The ecorr_alt_lookup_as launch of the plain call and of the live block's LookupFn: contiguous, checked coords."""
    B, D, H, W = shape
    with _lib.on_device(feat.device):
        out = torch.empty((B, _lib.corr_channels(levels, radius), H, W), dtype=out_dtype, device=feat.device)
        _lib.check(_lib.lib().ecorr_alt_lookup_as(
            feat.data_ptr(), coords.data_ptr(), B, D, H, W, levels, radius, out.data_ptr(),
            _lib.OUT_FORMATS[out_dtype], _lib.stream_of(out)), "AlternateCorrBlock lookup")
    return out


class AlternateCorrBlock:
    """Volume-free correlation lookup (module docstring); the interface of CorrBlock's forward.
    trainable=True (keyword only): gradients for fmap1 / fmap2 through the lookups (module docstring)."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, *, fmap_dtype=None, differentiable=False,
                 trainable=False):
        if differentiable:
            raise NotImplementedError("AlternateCorrBlock: differentiable=True is CorrBlock's keyword (a gradient "
                                      "pyramid, which this block does not have); pass trainable=True for the "
                                      "backward of the on-the-fly lookup")
        self.num_levels = num_levels
        self.radius = radius
        self._fmap_dtype = _lib.fmap_dtype_of(fmap_dtype)
        live = _lib.require_fmap_pair(fmap1, fmap2, bool(trainable), self._fmap_dtype)
        if not (fmap1.is_contiguous() and fmap2.is_contiguous()):
            raise RuntimeError("fmap1/fmap2 must be contiguous (reference: view size is not "
                               "compatible with input tensor's size and stride)")
        B, D, H, W = fmap1.shape
        if B == 0 or D == 0 or H == 0 or W == 0:
            raise RuntimeError(f"AlternateCorrBlock: empty fmaps {tuple(fmap1.shape)} (B, D, H and W must be at "
                               "least 1: there is no volume to be NaN)")
        if live and ((H >> (num_levels - 1)) < 2 or (W >> (num_levels - 1)) < 2):
            raise RuntimeError(f"trainable AlternateCorrBlock: level {num_levels - 1} is "
                               f"{H >> (num_levels - 1)} x {W >> (num_levels - 1)}; every level must be at least 2 x 2 "
                               "(the reference's samples of a 1-pixel axis are NaN: division by size - 1 = 0)")
        self._shape = (B, D, H, W)
        self._device = fmap1.device
        what = "AlternateCorrBlock pack"
        with _lib.on_device(self._device):
            self._feat = _lib.scratch("ecorr_alt_size", B, D, H, W, num_levels, device=self._device, what=what,
                                      dtype=torch.float32)
            _lib.check(_lib.lib().ecorr_alt_pack_as(
                fmap1.data_ptr(), fmap2.data_ptr(), _lib.ELEM_FORMATS[self._fmap_dtype], B, D, H, W, num_levels,
                self._feat.data_ptr(), _lib.stream_of(self._feat)), what)
        self._grad = self._handle = None
        if live:
            self._grad = _AltGradState(self._shape, num_levels, radius, self._feat, self._device)
            self._handle = HandleFn.apply(fmap1, fmap2, self._grad)

    @property
    def corr_pyramid(self):
        raise NotImplementedError("AlternateCorrBlock has no corr_pyramid: the all-pairs volume is never "
                                  "materialized (use CorrBlock to inspect it)")

    def lookup_conv1x1_relu(self, *args, **kwargs):
        raise NotImplementedError("AlternateCorrBlock has no lookup_conv1x1_relu: a convc1 fused with the "
                                  "on-the-fly lookup is not built (apply convc1 to corr_fn(coords), or use CorrBlock)")

    def __call__(self, coords, out_dtype=None):
        """The lookup [B, num_levels * (2r+1)^2, H, W]; out_dtype as CorrBlock.__call__'s."""
        out_dtype = _lib.lookup_out_dtype(out_dtype)
        B, D, H, W = self._shape
        check_coords(coords, (B, 2, H, W), self._device, self._grad is not None, "trainable AlternateCorrBlock")
        if self._grad is not None:
            return LookupFn.apply(self._handle, coords, self._grad, self._feat, out_dtype)
        return _alt_lookup(self._feat, coords.contiguous(), self._shape, self.num_levels, self.radius, out_dtype)
