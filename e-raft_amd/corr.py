"""Drop-in CorrBlock for E-RAFT on MI355X (mirrors /root/reference/model/corr.py).

Same constructor and call signatures as the reference:
    corr_fn = CorrBlock(fmap1, fmap2, num_levels=4, radius=4)      # corr.py:13  (eraft.py:107)
    corr    = corr_fn(coords1)                                       # corr.py:29  (eraft.py:128)
    corr    = corr_fn(coords1, out_dtype=torch.float16)              # the same lookup, 16-bit elements
    CorrBlock.corr(fmap1, fmap2) -> [B, H, W, 1, H, W]               # corr.py:52
    corr_fn.corr_pyramid[i] : [B*H*W, 1, h_i, w_i]                   # corr.py:16,24,27
The work happens in libecorr.so (hand-written gfx950 HIP kernels, C ABI include/ecorr.h): one
MFMA GEMM launch builds all 4 pyramid levels, one gather launch serves each lookup.  No ATen
compute op runs on the hot path and there is no CPU fallback.  The pyramid lives in a tiled,
gather-friendly layout (layout.py); corr_pyramid materializes the reference-layout levels on
first access (nothing on the E-RAFT path reads it).

Contract differences, all loud: inputs must be fp32 HIP tensors (the reference path is fp32,
eraft.py:104-105); by default the block is forward-only (E-RAFT only ever calls it under
torch.no_grad(), test.py:80) and refuses inputs that require grad while grad mode is on; coords
must match the build's (B, 2, H, W) exactly.

Mixed precision: `corr_fn(coords, out_dtype=torch.float16 | torch.bfloat16)` returns the lookup in
that dtype (ecorr_lookup_as, csrc/lookup_half.hip): each element is the fp32 sample
rounded once to nearest-even, bitwise `corr_fn(coords).to(dtype)`, stored by the lookup kernel itself
-- half the output bytes and no cast kernel in front of an autocast convc1 (eraft.py:131-132).
out_dtype None or torch.float32 is the fp32 call exactly; any other dtype raises TypeError.  On a
differentiable block the 16-bit lookup is differentiable too: its backward converts the incoming
gradient with .float() and runs the fp32 backward.

16-bit at both ends: `CorrBlock(f1, f2, ..., fmap_dtype=torch.float16 | torch.bfloat16)`
takes both fmaps in that dtype, as fnet returns them under autocast, and the split build's operand pass
reads them itself (ecorr_build_split_pack_as): the 16-bit -> fp32 conversion is exact, so the pyramid is
bitwise that of `CorrBlock(f1.float(), f2.float(), ...)` with two cast kernels and half the pack's read
bytes less.  fmap_dtype None / torch.float32 is the fp32 check and path exactly (a 16-bit fmap without
the keyword still raises); another dtype, or fmaps of different dtypes, raise TypeError.  With
ECORR_BUILD_MODE=fp32 (no 16-bit input there) the block converts with .float() and builds as before.
The presplit convc1 mode needs fp32 fmaps for its column scale, so on a 16-bit block it takes its
documented fallback, "split".  A differentiable block saves the 16-bit fmaps; its backward converts
them with .float() as temporaries, runs ecorr_build_backward and returns the gradients cast to the
fmaps' dtype -- what autograd's own .float() node would hand back, so fmap.grad is bitwise that of the
fp32 block on fmap.float().
`corr_fn.lookup_conv1x1_relu(coords, weight, bias, out_dtype=...)` returns relu(convc1(corr)) in that
dtype from the conv's own epilogue (ecorr_conv1x1_relu_split_as / ecorr_lookup_conv1x1_relu_packed_as):
bitwise the fp32 call's result cast once, with no cast kernel in front of an autocast convc2.

Training (opt-in): CorrBlock(fmap1, fmap2, num_levels, radius, differentiable=True) accepts fmaps
that require grad and gives them gradients through the build and every `corr_fn(coords)` lookup
(the two backward entries of csrc/grad.hip).  The forward runs
the same launches, so its values are bitwise the plain block's; under torch.no_grad(), or when no
fmap requires grad, the block is the plain block.  Autograd never carries a pyramid-sized tensor
(the handle mechanism of _grad.py: the lookups' backwards add into the block's single gradient
pyramid, the build's backward runs once after all of them).  Deterministic (no atomics).
Contract of the differentiable block: coords are detached
(coords.requires_grad raises; eraft.py:127 detaches them; there is no coordinate gradient), every
pyramid level is at least 2 x 2 (the reference's samples of a 1-pixel axis are NaN), D >= 1, one
backward per block (a second one raises), single GPU; bilinear_sampler and RowShardedCorrBlock stay
forward-only.

Training through convc1 (the same opt-in): on a differentiable block,
`corr_fn.lookup_conv1x1_relu(coords, weight, bias)` is a Function of (handle, coords, weight, bias)
whenever grad mode is on and the block is live or weight / bias require grad.  Its forward is the
plain call's launch sequence in the requested mode (bitwise the same values) and saves only coords,
weight, bias and its own output; the backward (ecorr_conv1x1_relu_backward, csrc/conv_grad.hip;
DESIGN.md §3.3.1) masks the incoming gradient with the saved output, recomputes the lookup for the
weight gradient instead of keeping it alive (99.5 MB per iteration at DSEC B = 16), runs grad_corr on
the f16 matrix cores (the split conv with the transposed weight, packed once per block) and feeds it
to the lookup backward when the block is live.  With frozen fmaps only weight and bias receive
gradients and no gradient pyramid is allocated.  Deterministic (no atomics).

Numerics: the default build sums each product as f16 lo*hi + hi*lo + hi*hi of per-pixel-scaled
operands: within 1e-5 normwise of the reference and closer to fp64 than its fp32
GEMM, pooling and lookup bit-exact given level 0.  One semantic difference: an fmap pixel holding
+-inf yields NaN (not +-inf) in its level-0 row/column, because the lo half of an infinite value
is NaN; NaN inputs give NaN in both.  ECORR_BUILD_MODE=fp32 (read once at import) selects the
fp32-MFMA build, which keeps the reference's inf semantics.

corr_pyramid is a materialized COPY in the reference layout: 4 levels of B*H*W query images
(1.96 GB at DSEC B=16, the whole pyramid again), made on first access and cached on the block.
Nothing on the E-RAFT path reads it; access it only for inspection or tests.
"""
import weakref

import torch

from . import _lib
from ._grad import GradState, HandleFn, LookupFn
from ._lib import check_coords, require_device
from .layout import levels_of


class _GradState(GradState):
    """The shared state of one differentiable block (_grad.py): buf is the gradient pyramid G."""

    CONSUMED = ("eraft_amd CorrBlock: backward through a block whose gradient was already "
                "consumed (one backward per differentiable block)")

    def lookup(self, pyramid, coords, out_dtype):
        B, _, H, W = self.shape
        out = torch.empty((B, _lib.corr_channels(self.levels, self.radius), H, W), dtype=out_dtype,
                          device=self.device)
        return _lib.lookup(pyramid, coords, (B, H, W), H * W, self.levels, self.radius, out, "CorrBlock")

    def lookup_backward(self, grad, coords):
        B, _, H, W = self.shape
        _lib.check(_lib.lib().ecorr_lookup_backward(
            grad.data_ptr(), coords.data_ptr(), B, H, W, H * W, self.levels, self.radius, self.buf.data_ptr(),
            _lib.stream_of(grad)), "CorrBlock lookup backward")

    def saved(self, fmap1, fmap2):
        return fmap1, fmap2   # as given: 16-bit fmaps (fmap_dtype) are saved as 16-bit

    def fmap_backward(self, G, saved, g1, g2):
        B, D, H, W = self.shape
        f1, f2 = (f.float() for f in saved)   # 16-bit fmaps as fp32 temporaries (exact)
        _lib.check(_lib.lib().ecorr_build_backward(
            G.data_ptr(), f1.data_ptr(), f2.data_ptr(), B, D, H, W, H * W, self.levels,
            _lib.ptr(g1), _lib.ptr(g2), _lib.stream_of(f1)), "CorrBlock build backward")


class _LookupConvFn(torch.autograd.Function):
    """(handle, coords, weight, bias) -> relu(conv1x1(lookup(coords))).  handle is None when the block
    is not live (frozen fmaps): then only weight and bias get gradients.  corr is not saved: the
    backward recomputes it (ecorr_lookup) when the weight needs its gradient."""

    @staticmethod
    def forward(ctx, handle, coords, weight, bias, blk, mode, out_dtype=torch.float32):
        out = blk._lookup_conv(coords, weight, bias, mode, out_dtype)
        # what the backward reads of the block, not the block: the pyramid, the geometry, the shared
        # gradient state (None: not live) and the packed-weight cache
        ctx.pyramid, ctx.state, ctx.wcache = blk._pyramid, blk._grad, blk._wcache
        ctx.geom = (blk._shape, blk.num_levels, blk.radius)
        ctx.save_for_backward(coords, out, weight, bias)   # versioned: an in-place change raises in backward
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        st = ctx.state
        if st is not None:
            st.require_unconsumed()
        coords, out, weight, bias = ctx.saved_tensors
        (B, _, H, W), levels, radius = ctx.geom
        want_in = st is not None and ctx.needs_input_grad[0]
        want_w = ctx.needs_input_grad[2]
        want_b = bias is not None and ctx.needs_input_grad[3]
        dev = out.device
        cc = coords.contiguous()
        with _lib.on_device(dev):
            handle_grad = None if st is None else torch.zeros(1, dtype=torch.float32, device=dev)
            if not (want_in or want_w or want_b):
                return handle_grad, None, None, None, None, None, None
            # a 16-bit output: the fp32 backward on its exact values -- the ReLU mask is the saved 16-bit
            # output's, as autocast's own ReLU would take it
            go = grad_out.float().contiguous()
            out = out.float()
            corr = None
            if want_w:   # the conv's input again (44 us at DSEC B = 16) instead of 99.5 MB saved per call
                corr = torch.empty((B, _lib.corr_channels(levels, radius), H, W), dtype=torch.float32, device=dev)
                _lib.lookup(ctx.pyramid, cc, (B, H, W), H * W, levels, radius, corr, "CorrBlock")
            gi, gw, gb = _lib.conv1x1_relu_backward(go, out, corr, weight, ctx.wcache, want_in, want_w, want_b,
                                                    "CorrBlock lookup+conv1x1+relu backward")
            del corr
            if want_in:
                st.add_lookup_grad(gi, cc)
        return handle_grad, None, gw, gb, None, None, None


class CorrBlock:
    """All-pairs correlation pyramid + radius-r lookup (reference: model/corr.py:12-60).
    differentiable=True (keyword only): gradients for fmap1 / fmap2, and through
    lookup_conv1x1_relu for its weight and bias too (module docstring).
    fmap_dtype (keyword only): None / torch.float32 = fp32 fmaps (the reference's); torch.float16 /
    torch.bfloat16 = both fmaps in that dtype, read by the split build as they are (module docstring)."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, *, differentiable=False, fmap_dtype=None):
        self.num_levels = num_levels
        self.radius = radius
        self._differentiable = bool(differentiable)   # lookup_conv1x1_relu: weight / bias gradients without live fmaps
        # the gradient path is live only when asked for and needed; otherwise: the plain block
        self._fmap_dtype = _lib.fmap_dtype_of(fmap_dtype)
        live = _lib.require_fmap_pair(fmap1, fmap2, self._differentiable, self._fmap_dtype)
        if not (fmap1.is_contiguous() and fmap2.is_contiguous()):
            # the reference .view()s them (corr.py:55-56), which raises on these strides
            raise RuntimeError("fmap1/fmap2 must be contiguous (reference: view size is not "
                               "compatible with input tensor's size and stride)")
        B, D, H, W = fmap1.shape
        # degenerate shapes as the reference (tests/golden/degenerate.npz): an empty batch or map
        # raises where its reshape / avg_pool2d do (corr.py:16-24); D = 0 feature channels give
        # 0 / sqrt(0) = NaN volumes, which its lookup samples like any other values
        if B == 0:
            raise RuntimeError(f"cannot reshape tensor of 0 elements into shape [0, {H}, {W}, -1] "
                               "(empty batch: the reference's CorrBlock.corr reshape)")
        if H == 0 or W == 0:
            raise RuntimeError(f"Expected 3D or 4D (batch mode) tensor with optional 0 dim batch size for "
                               f"input, but got:[{B * H * W}, 1, {H}, {W}] (empty map: the reference's avg_pool2d)")
        self._shape = (B, D, H, W)
        self._device = fmap1.device
        Q = H * W
        self._h, self._w, self._off = _lib.layout(B * Q, H, W, num_levels)
        if live:
            if D == 0:
                raise RuntimeError("differentiable CorrBlock: D = 0 feature channels (the volume is 0 / sqrt(0) = NaN)")
            if self._h[-1] < 2 or self._w[-1] < 2:
                raise RuntimeError(f"differentiable CorrBlock: pyramid level {num_levels - 1} is "
                                   f"{self._h[-1]} x {self._w[-1]}; every level must be at least 2 x 2 (the "
                                   "reference's samples of a 1-pixel axis are NaN: division by size - 1 = 0)")
        with _lib.on_device(self._device):
            if D == 0:
                self._pyramid = torch.full((self._off[-1],), float("nan"), dtype=torch.float32, device=self._device)
            else:
                self._pyramid = _lib.build_pyramid(fmap1, fmap2, B, D, H, W, Q, num_levels, self._off,
                                                   "CorrBlock build")
        self._rows = B * Q
        self._levels_cache = None
        self._wcache = {}   # packed convc1 weights of this block (_lib.packed_conv1x1_weight)
        # presplit convc1: the column scales come from the fmaps (ecorr_split_column_scale), computed
        # on the first presplit call; weak references and version counters, so the block neither
        # keeps the fmaps alive nor trusts them after an in-place change (then: the split mode)
        self._fmap_refs = (weakref.ref(fmap1), weakref.ref(fmap2),
                           _lib.tensor_version(fmap1), _lib.tensor_version(fmap2))
        self._colscale = None
        self._grad = self._handle = None
        if live:
            self._grad = _GradState(self._shape, num_levels, radius, self._device, self._off[-1])
            self._handle = HandleFn.apply(fmap1, fmap2, self._grad)

    @property
    def corr_pyramid(self):
        """Reference-layout levels [B*H*W, 1, h_i, w_i] (corr.py:16-27), materialized on demand."""
        if self._levels_cache is None:
            self._levels_cache = levels_of(self._pyramid, self._rows, self._shape[2], self._shape[3], self.num_levels)
        return self._levels_cache

    def __call__(self, coords, out_dtype=None):
        """The lookup [B, num_levels * (2r+1)^2, H, W] (corr.py:29-50).  out_dtype: None / torch.float32
        (the fp32 call), torch.float16 or torch.bfloat16 (the same launch storing each fp32 sample
        rounded once to nearest-even: bitwise self(coords).to(out_dtype)); anything else: TypeError."""
        out_dtype = _lib.lookup_out_dtype(out_dtype)
        B, _, H, W = self._shape
        check_coords(coords, (B, 2, H, W), self._device, self._grad is not None, "differentiable CorrBlock")
        if self._grad is not None:
            return LookupFn.apply(self._handle, coords, self._grad, self._pyramid, out_dtype)
        coords = coords.contiguous()   # the reference accepts any strides (permute + reshape)
        out = torch.empty((B, _lib.corr_channels(self.num_levels, self.radius), H, W), dtype=out_dtype,
                          device=self._device)
        return _lib.lookup(self._pyramid, coords, (B, H, W), H * W, self.num_levels, self.radius, out, "CorrBlock")

    def lookup_conv1x1_relu(self, coords, weight, bias=None, mode=None, out_dtype=None):
        """F.relu(conv1x1(self(coords), weight, bias)): the lookup followed by
        BasicMotionEncoder.convc1 + ReLU (update.py:67,74).
        weight: [O, C, 1, 1] (or [O, C]) fp32 with C = num_levels * (2r+1)^2; bias: [O] or None.
        Returns [B, O, H, W] in out_dtype: None / torch.float32, or torch.float16 / torch.bfloat16 -- each
        element the fp32 call's value (after bias and ReLU) rounded once to nearest-even by the conv's own
        epilogue, bitwise self.lookup_conv1x1_relu(...).to(out_dtype), in modes "split" and "fused"
        ("presplit" with a 16-bit out_dtype runs as "split"); weight and bias stay fp32; anything else:
        TypeError.  mode (default: env ECORR_CONVC1, else "split"):
          "split"  ecorr_lookup_qmax into a temporary [B, C, H, W] (+ per-query maxima), then
                   ecorr_conv1x1_relu_split (f16 matrix cores, split operands: normwise within 1e-5
                   of the fp32 conv);
          "presplit" (ABI 16, radius 4, <= 4 levels) ecorr_lookup_presplit writes corr already split
                   (f16 hi + lo under a per-query bound scale from the fmaps, ecorr_split_column_scale,
                   once per block) and ecorr_conv1x1_relu_presplit loads it whole: normwise within 1e-5;
                   falls back to "split" when the fmaps are gone or changed in place since the build;
                   measured no faster than "split" (DESIGN.md §3.3);
          "fused"  ecorr_lookup_conv1x1_relu_packed: one kernel, the lookup tile never leaves the
                   CU, an exact c-ordered fp32 MFMA sum (radius 4, num_levels <= 4, O a multiple of 64).
        A block built with differentiable=True trains through this call (grad mode on, and the block
        live or weight / bias requiring grad): the same launches in the forward (bitwise the plain
        block's values), and in the backward ecorr_conv1x1_relu_backward on the recomputed lookup, then
        the lookup backward into the block's gradient pyramid when the block is live (module
        docstring).  coords that require grad raise, as in corr_fn(coords).  With a 16-bit
        out_dtype the saved output is the 16-bit one and the backward runs the fp32 backward on
        out.float() and grad_out.float(): the ReLU mask is taken from the 16-bit output, as autocast's own
        ReLU would take it, so the gradients differ from the fp32-output call's only where a positive
        fp32 output rounds to 0 in 16 bits."""
        mode = _lib.convc1_mode(mode, presplit=True)
        out_dtype = _lib.lookup_out_dtype(out_dtype)
        train = self._differentiable and torch.is_grad_enabled() and (
            self._grad is not None or (isinstance(weight, torch.Tensor) and weight.requires_grad)
            or (isinstance(bias, torch.Tensor) and bias.requires_grad))
        B, _, H, W = self._shape
        check_coords(coords, (B, 2, H, W), self._device, train, "differentiable CorrBlock")
        if train:
            require_device("weight", weight)
            return _LookupConvFn.apply(self._handle, coords, weight, bias, self, mode, out_dtype)
        return self._lookup_conv(coords, weight, bias, mode, out_dtype)

    def _lookup_conv(self, coords, weight, bias, mode, out_dtype=torch.float32):
        """The launches of lookup_conv1x1_relu on checked coords (its plain call and _LookupConvFn.forward)."""
        B, _, H, W = self._shape
        return _lib.lookup_conv1x1_relu(
            self._pyramid, coords.contiguous(), (B, H, W), H * W, self.num_levels, self.radius, weight, bias, mode,
            lambda O: torch.empty((B, O, H, W), dtype=out_dtype, device=self._device), self._wcache, "CorrBlock",
            column_scale=self._column_scale)

    def _column_scale(self, st):
        """int[B*H*W + B]: the presplit column exponents (ecorr_split_column_scale), once per block;
        None when the fmaps are gone or were changed in place since the build, or are 16-bit (the
        scale kernel reads fp32)."""
        if self._fmap_dtype != torch.float32:
            return None
        if self._colscale is None:
            r1, r2, v1, v2 = self._fmap_refs
            f1, f2 = r1(), r2()
            if f1 is None or f2 is None or _lib.tensor_version(f1) != v1 or _lib.tensor_version(f2) != v2:
                return None
            B, D, H, W = self._shape
            sc = torch.empty(B * H * W + B, dtype=torch.int32, device=self._device)
            _lib.check(_lib.lib().ecorr_split_column_scale(f1.data_ptr(), f2.data_ptr(), B, D, H, W, sc.data_ptr(),
                                                           st), "CorrBlock presplit column scale")
            self._colscale = sc
            self._fmap_refs = None
        return self._colscale

    @staticmethod
    def corr(fmap1, fmap2):
        """Level-0 volume fmap1^T fmap2 / sqrt(D) as [B, H, W, 1, H, W] (corr.py:52-60)."""
        blk = CorrBlock(fmap1, fmap2, num_levels=1, radius=0)
        B, _, H, W = fmap1.shape
        return blk.corr_pyramid[0].view(B, H, W, 1, H, W)
