"""AlternateCorrBlock: CorrBlock's lookup without the all-pairs volume (RAFT's `alternate_corr`).

    corr_fn = AlternateCorrBlock(fmap1, fmap2, num_levels=4, radius=4)
    corr    = corr_fn(coords1)                               # [B, num_levels * (2r+1)^2, H, W]
    corr    = corr_fn(coords1, out_dtype=torch.float16)      # the same lookup, 16-bit elements

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

The checks and messages are CorrBlock's.  The block is forward-only: fmaps or coords that require grad
while grad mode is on raise, and so do differentiable=True, corr_pyramid (there is no volume) and
lookup_conv1x1_relu (no fused convc1).  D = 0 and empty shapes raise: there is no volume to be NaN.
fmap_dtype / out_dtype: as CorrBlock's (16-bit fmaps are read as they are, exactly; a 16-bit output is
the fp32 sample rounded once, bitwise corr_fn(coords).to(out_dtype)).  Deterministic (no atomics).
"""
import torch

from . import _lib
from ._lib import no_grad_inputs, require_device


class AlternateCorrBlock:
    """Volume-free correlation lookup (module docstring); the interface of CorrBlock's forward."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, *, fmap_dtype=None, differentiable=False):
        if differentiable:
            raise NotImplementedError("AlternateCorrBlock is forward-only: differentiable=True needs a backward of "
                                      "the on-the-fly lookup, which is not built (use CorrBlock)")
        self.num_levels = num_levels
        self.radius = radius
        self._fmap_dtype = _lib.fmap_dtype_of(fmap_dtype)
        _lib.require_fmap_pair(fmap1, fmap2, False, self._fmap_dtype)
        if not (fmap1.is_contiguous() and fmap2.is_contiguous()):
            raise RuntimeError("fmap1/fmap2 must be contiguous (reference: view size is not "
                               "compatible with input tensor's size and stride)")
        B, D, H, W = fmap1.shape
        if B == 0 or D == 0 or H == 0 or W == 0:
            raise RuntimeError(f"AlternateCorrBlock: empty fmaps {tuple(fmap1.shape)} (B, D, H and W must be at "
                               "least 1: there is no volume to be NaN)")
        self._shape = (B, D, H, W)
        self._device = fmap1.device
        what = "AlternateCorrBlock pack"
        with _lib.on_device(self._device):
            self._feat = _lib.scratch("ecorr_alt_size", B, D, H, W, num_levels, device=self._device, what=what,
                                      dtype=torch.float32)
            _lib.check(_lib.lib().ecorr_alt_pack_as(
                fmap1.data_ptr(), fmap2.data_ptr(), _lib.ELEM_FORMATS[self._fmap_dtype], B, D, H, W, num_levels,
                self._feat.data_ptr(), _lib.stream_of(self._feat)), what)

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
        require_device("coords", coords)
        no_grad_inputs(coords)
        if tuple(coords.shape) != (B, 2, H, W):
            raise RuntimeError(f"coords shape {tuple(coords.shape)} != {(B, 2, H, W)} of the pyramid")
        if coords.device != self._device:
            raise RuntimeError("coords is on a different device than the pyramid")
        coords = coords.contiguous()
        with _lib.on_device(self._device):
            out = torch.empty((B, _lib.corr_channels(self.num_levels, self.radius), H, W), dtype=out_dtype,
                              device=self._device)
            _lib.check(_lib.lib().ecorr_alt_lookup_as(
                self._feat.data_ptr(), coords.data_ptr(), B, D, H, W, self.num_levels, self.radius, out.data_ptr(),
                _lib.OUT_FORMATS[out_dtype], _lib.stream_of(out)), "AlternateCorrBlock lookup")
        return out
