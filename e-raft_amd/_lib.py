"""ctypes binding of libecorr.so (C ABI: include/ecorr.h).

torch is imported first on purpose: torch ships its own libamdhip64.so (SONAME libamdhip64.so.7);
loading libecorr.so afterwards makes the dynamic linker reuse that already-loaded runtime, so the
kernels run in torch's HIP context on torch's streams and caching-allocator pointers.

There is no fallback: if libecorr.so is missing or was built for another target, every entry point
raises.  Build it with `make -C e-raft_amd/csrc` or `python -c "import __graft_entry__ as g; g.build()"`.

What every wrapper in the package is made of, each defined here once: require_device (the argument
check), ptr (an optional tensor as a pointer), scratch (size entry -> temporary), on_device (the
device context of a launch), stream_of, check, corr_channels.
"""
import contextlib
import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load, see above)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libecorr.so")
ABI_VERSION = 17
MAX_LEVELS = 16

ECORR_OK = 0
ECORR_EINVAL = -1
ECORR_ESHAPE = -2
ECORR_ERADIUS = -3
ECORR_ELEVELS = -4

# ecorr_lookup_as's out_format (include/ecorr.h) per output dtype
ECORR_OUT_F32 = 0
ECORR_OUT_F16 = 1
ECORR_OUT_BF16 = 2
OUT_FORMATS = {torch.float32: ECORR_OUT_F32, torch.float16: ECORR_OUT_F16, torch.bfloat16: ECORR_OUT_BF16}
# the same codes as an input format (ECORR_ELEM_*: ecorr_build_split_pack_as's fmap_format)
ECORR_ELEM_F32, ECORR_ELEM_F16, ECORR_ELEM_BF16 = ECORR_OUT_F32, ECORR_OUT_F16, ECORR_OUT_BF16
ELEM_FORMATS = OUT_FORMATS

_lib = None

_i = ctypes.c_int
_i64 = ctypes.c_int64
_p = ctypes.c_void_p

SYMBOLS = {
    # name: (restype, argtypes)
    "ecorr_abi_version": (_i, []),
    "ecorr_strerror": (ctypes.c_char_p, [_i]),
    "ecorr_pyramid_layout": (_i, [_i64, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i),
                                  ctypes.POINTER(_i64)]),
    # (fmap1, fmap2, B, D, H, W, q_count, levels, pyramid, stream)
    "ecorr_build": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    # (B, D, H, W, q_count, bytes*)
    "ecorr_build_split_workspace_size": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_i64)]),
    # (fmap1, fmap2, B, D, H, W, q_count, levels, pyramid, workspace, stream)
    "ecorr_build_split": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    # (fmap1, fmap2, B, D, H, W, q_count, workspace, stream)
    "ecorr_build_split_pack": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p]),
    # 16-bit (or fp32) fmaps in (added within ABI 17):
    # (fmap1, fmap2, fmap_format, B, D, H, W, q_count, workspace, stream) /
    # (fmap1, fmap2, fmap_format, B, D, H, W, q_count, levels, pyramid, workspace, stream)
    "ecorr_build_split_pack_as": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    "ecorr_build_split_as": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    # (B, D, H, W, q_count, levels, pyramid, workspace, stream)
    "ecorr_build_split_gemm": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p]),
    # the hi-only split build (added within ABI 17): the size entry, pack_as, gemm and as with a hi
    # workspace (256 bytes of flag block in front of the split workspace)
    "ecorr_build_split_hi_workspace_size": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_build_split_pack_hi_as": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    "ecorr_build_split_gemm_hi": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "ecorr_build_split_hi_as": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    # (pyramid, coords, B, H, W, q_count, levels, radius, out, stream)
    "ecorr_lookup": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    # a 16-bit (or fp32) output element (added within ABI 17):
    # (pyramid, coords, B, H, W, q_count, levels, radius, out_format, out, stream)
    "ecorr_lookup_as": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p]),
    # volume-free correlation (added within ABI 17): (B, D, H, W, levels, floats*) /
    # (fmap1, fmap2, fmap_format, B, D, H, W, levels, feat, stream) /
    # (feat, coords, B, D, H, W, levels, radius, out, out_format, stream)
    "ecorr_alt_size": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_alt_pack_as": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    "ecorr_alt_lookup_as": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _i, _p]),
    # its backward (added within ABI 17): (B, H, W, levels, radius, bytes*) /
    # (feat, coords, grad_out, B, D, H, W, levels, radius, grad_feat, workspace, stream) /
    # (grad_feat, B, D, H, W, levels, grad_fmap1, grad_fmap2, stream)
    "ecorr_alt_backward_workspace_size": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_alt_lookup_backward": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "ecorr_alt_pack_backward": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p]),
    # the backward (ABI 17): (grad_out, coords, B, H, W, q_count, levels, radius, grad_pyramid, stream)
    "ecorr_lookup_backward": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    # (grad_pyramid, fmap1, fmap2, B, D, H, W, q_count, levels, grad_fmap1, grad_fmap2, stream)
    "ecorr_build_backward": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    # (pyramid, coords, B, H, W, q_count, levels, radius, weight[O][C], bias, O, out, stream)
    "ecorr_lookup_conv1x1_relu": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p, _p]),
    # (O, C, floats*) / (weight[O][C], O, C, packed, stream) / as ecorr_lookup_conv1x1_relu, packed weight
    "ecorr_conv1x1_packed_size": (_i, [_i, _i, ctypes.POINTER(_i64)]),
    "ecorr_conv1x1_pack": (_i, [_p, _i, _i, _p, _p]),
    "ecorr_lookup_conv1x1_relu_packed": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p, _p]),
    # a 16-bit (or fp32) convc1 output (added within ABI 17): as the packed entry, out_format before out
    "ecorr_lookup_conv1x1_relu_packed_as": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _i, _p, _p]),
    # (O, C, bytes*) / (weight[O][C], O, C, packed, stream) /
    # (in[B][C][Q], B, C, Q, qmax, G, packed, bias, O, out, stream): split-f16 convc1 + ReLU (ABI 15)
    "ecorr_conv1x1_split_size": (_i, [_i, _i, ctypes.POINTER(_i64)]),
    "ecorr_conv1x1_split_pack": (_i, [_p, _i, _i, _p, _p]),
    "ecorr_conv1x1_relu_split": (_i, [_p, _i, _i, _i, _p, _i, _p, _p, _i, _p, _p]),
    # (in[B][C][Q], B, C, Q, qmax, G, packed, bias, O, out_format, out, stream) (added within ABI 17)
    "ecorr_conv1x1_relu_split_as": (_i, [_p, _i, _i, _i, _p, _i, _p, _p, _i, _i, _p, _p]),
    # its backward (added within ABI 17): (B, C, Q, O, bytes*) /
    # (grad_out, out, in, packed_t, B, C, Q, O, grad_in, grad_weight, grad_bias, workspace, stream)
    "ecorr_conv1x1_relu_backward_workspace_size": (_i, [_i, _i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_conv1x1_relu_backward": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    # as ecorr_lookup + qmax[B][3*levels][q_count] (before stream)
    "ecorr_lookup_qmax": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    # presplit convc1 (ABI 16): (fmap1, fmap2, B, D, H, W, scale[B*H*W + B], stream)
    "ecorr_split_column_scale": (_i, [_p, _p, _i, _i, _i, _i, _p, _p]),
    "ecorr_presplit_size": (_i, [_i, _i, _i, ctypes.POINTER(_i64)]),
    # (pyramid, coords, B, H, W, q_count, levels, radius, scale, out, stream)
    "ecorr_lookup_presplit": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "ecorr_conv1x1_presplit_size": (_i, [_i, _i, ctypes.POINTER(_i64)]),
    "ecorr_conv1x1_split_pack_presplit": (_i, [_p, _i, _i, _p, _p]),
    # (in, B, levels, Q, scale, packed, bias, O, out, stream)
    "ecorr_conv1x1_relu_presplit": (_i, [_p, _i, _i, _i, _p, _p, _p, _i, _p, _p]),
    # SepConvGRU (added within ABI 17): (hidden, input, bytes*) /
    # (weight[6], bias[6], hidden, input, packed, stream) / (B, hidden, input, H, W, bytes*) /
    # (h, x, B, hidden, input, H, W, packed, h_out, workspace, stream)
    "ecorr_sepconv_gru_packed_size": (_i, [_i, _i, ctypes.POINTER(_i64)]),
    "ecorr_sepconv_gru_pack": (_i, [ctypes.POINTER(_p), ctypes.POINTER(_p), _i, _i, _p, _p]),
    "ecorr_sepconv_gru_workspace_size": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_sepconv_gru": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    # its backward (added within ABI 17): (hidden, input, bytes*) / (weight[6], hidden, input, packed_t, stream) /
    # (B, hidden, input, H, W, bytes*) / (h, x, grad_out, B, hidden, input, H, W, packed, packed_t, grad_h, grad_x,
    # grad_weight[6], grad_bias[6], workspace, stream)
    "ecorr_sepconv_gru_backward_packed_size": (_i, [_i, _i, ctypes.POINTER(_i64)]),
    "ecorr_sepconv_gru_backward_pack": (_i, [ctypes.POINTER(_p), _i, _i, _p, _p]),
    "ecorr_sepconv_gru_backward_workspace_size": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_sepconv_gru_backward": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, ctypes.POINTER(_p),
                                        ctypes.POINTER(_p), _p, _p]),
    # the motion encoder behind convc1 (added within ABI 17): (bytes*) / (weight[4], bias[4], packed, stream) /
    # (B, H, W, bytes*) / (c1, flow, B, H, W, packed, out, out_batch_stride, workspace, stream)
    "ecorr_motion_encoder_packed_size": (_i, [ctypes.POINTER(_i64)]),
    "ecorr_motion_encoder_pack": (_i, [ctypes.POINTER(_p), ctypes.POINTER(_p), _p, _p]),
    "ecorr_motion_encoder_workspace_size": (_i, [_i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_motion_encoder": (_i, [_p, _p, _i, _i, _i, _p, _p, _i64, _p, _p]),
    # its backward (added within ABI 17): (bytes*) / (weight[4], packed_t, stream) / (B, H, W, bytes*) / (c1, flow,
    # grad_out, grad_out_batch_stride, B, H, W, packed, packed_t, grad_c1, grad_flow, grad_weight[4], grad_bias[4],
    # workspace, stream)
    "ecorr_motion_encoder_backward_packed_size": (_i, [ctypes.POINTER(_i64)]),
    "ecorr_motion_encoder_backward_pack": (_i, [ctypes.POINTER(_p), _p, _p]),
    "ecorr_motion_encoder_backward_workspace_size": (_i, [_i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_motion_encoder_backward": (_i, [_p, _p, _p, _i64, _i, _i, _i, _p, _p, _p, _p, ctypes.POINTER(_p),
                                           ctypes.POINTER(_p), _p, _p]),
    "ecorr_bilinear_sampler": (_i, [_p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p]),
    "ecorr_coords_grid": (_i, [_i, _i, _i, _p, _p]),
    # (chunks, chunk, world, B, C, H, W, out, stream)
    "ecorr_rows_assemble": (_i, [_p, _i64, _i, _i, _i, _i, _i, _p, _p]),
    "ecorr_pyramid_tile": (_i, [ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    # (H, W, levels, ntx[levels])
    "ecorr_pyramid_formats": (_i, [_i, _i, _i, ctypes.POINTER(_i)]),
    # (B, n, h, w, bytes*)
    "ecorr_splat_workspace_size": (_i, [_i, _i64, _i, _i, ctypes.POINTER(_i64)]),
    # (flow, B, h, w, out, workspace, stream)
    "ecorr_forward_interpolate": (_i, [_p, _i, _i, _i, _p, _p, _p]),
    # (pts, n, h, w, values, valid, workspace, stream)
    "ecorr_grid_sample_values": (_i, [_p, _i64, _i, _i, _p, _p, _p, _p]),
    # (flow, mask, N, H, W, out, stream)
    "ecorr_upsample_flow": (_i, [_p, _p, _i, _i, _i, _p, _p]),
    # its backward (added within ABI 17): (N, H, W, bytes*) /
    # (grad_out, flow, mask, N, H, W, grad_flow, grad_mask, workspace, stream)
    "ecorr_upsample_backward_workspace_size": (_i, [_i, _i, _i, ctypes.POINTER(_i64)]),
    "ecorr_upsample_flow_backward": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    # (flow, B, h, w, out_u16, stream)
    "ecorr_flow_to_png16": (_i, [_p, _i, _i, _i, _p, _p]),
    # (in_u16, B, h, w, flow, valid, bad, stream)
    "ecorr_png16_to_flow": (_i, [_p, _i, _i, _i, _p, _p, _p, _p]),
    # (dsec, n, C, H, W, bytes*)
    "ecorr_voxel_workspace_size": (_i, [_i, _i64, _i, _i, _i, ctypes.POINTER(_i64)]),
    # (p, t, x, y, n, C, H, W, normalize, voxel, workspace, stream)
    "ecorr_voxel_grid_dsec": (_i, [_p, _p, _p, _p, _i64, _i, _i, _i, _i, _p, _p, _p]),
    # (events, n, C, H, W, normalize, voxel, bad_index, workspace, stream)
    "ecorr_voxel_grid_mvsec": (_i, [_p, _i64, _i, _i, _i, _i, _p, _p, _p, _p]),
}


def lib():
    """The loaded libecorr.so (raises if it is absent: no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"eraft_amd: {LIB_PATH} is not built; run `make -C e-raft_amd/csrc` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        v = L.ecorr_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"eraft_amd: libecorr ABI {v} != expected {ABI_VERSION}")
        _lib = L
    return _lib


def source_digest() -> str:
    """sha256 (16 hex) of the kernel sources, their Makefile (flags) and the C header: ties a committed PMC summary
    (profiles/latest_pmc.json, tools/pmc_summary.py) to the code it measured."""
    import hashlib
    root = os.path.dirname(os.path.abspath(__file__))
    files = sorted(os.path.join(root, "csrc", f) for f in os.listdir(os.path.join(root, "csrc"))
                   if f.endswith((".hip", ".h")) or f == "Makefile")   # the Makefile: compile flags
    files.append(os.path.join(root, "..", "include", "ecorr.h"))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def strerror(status: int) -> str:
    return lib().ecorr_strerror(status).decode()


def check(status: int, what: str):
    if status == ECORR_OK:
        return
    msg = f"{what}: {strerror(status)}"
    if status in (ECORR_EINVAL, ECORR_ERADIUS, ECORR_ELEVELS):
        raise ValueError(msg)
    raise RuntimeError(msg)


def require_device(name, t, dtype=torch.float32):
    """The argument check of every entry that takes tensors: a HIP tensor of `dtype`."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} is on {t.device}: eraft_amd runs only on HIP devices (no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {str(dtype).removeprefix('torch.')} (got {t.dtype})")


def no_grad_inputs(*ts, what="CorrBlock"):
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise RuntimeError(f"eraft_amd {what} is forward-only; call it under torch.no_grad() "
                           "(as the reference harness does, test.py:80)")


def check_coords(coords, shape, device, train=False, who=None, rows=False):
    """The coords check of every block's lookup: a float32 HIP tensor of `shape` on the pyramid's `device`.
    train: the call goes through autograd (coords that require grad are refused in the name of `who`, before
    the shape is looked at), else it is forward-only.  rows: the shape text of RowShardedCorrBlock's slab."""
    require_device("coords", coords)
    if train:
        if torch.is_grad_enabled() and coords.requires_grad:
            raise RuntimeError(f"{who}: coords requires grad; detach it (as eraft.py:127 does), "
                               "there is no gradient with respect to the coordinates")
    else:
        no_grad_inputs(coords)
    if tuple(coords.shape) != shape:
        raise RuntimeError(f"coords rows {tuple(coords.shape)} != {shape}" if rows else
                           f"coords shape {tuple(coords.shape)} != {shape} of the pyramid")
    if coords.device != device:
        raise RuntimeError("coords is on a different device than the pyramid")


def fmap_dtype_of(fmap_dtype):
    """The dtype both fmaps must have for the fmap_dtype argument of CorrBlock: None = float32."""
    if fmap_dtype is None:
        return torch.float32
    if fmap_dtype not in ELEM_FORMATS:
        raise TypeError(f"fmap_dtype must be None, torch.float32, torch.float16 or torch.bfloat16 (got {fmap_dtype!r})")
    return fmap_dtype


def require_fmap_pair(fmap1, fmap2, differentiable=False, dtype=torch.float32):
    """The fmap checks of CorrBlock and RowShardedCorrBlock (both fmaps of `dtype`).  Returns whether the
    gradient path is live: asked for (differentiable) and needed; otherwise fmaps that require grad raise."""
    require_device("fmap1", fmap1, dtype)
    require_device("fmap2", fmap2, dtype)
    live = differentiable and torch.is_grad_enabled() and (fmap1.requires_grad or fmap2.requires_grad)
    if not live:
        no_grad_inputs(fmap1, fmap2)
    if fmap1.dim() != 4 or fmap1.shape != fmap2.shape:
        raise RuntimeError(f"fmap shapes {tuple(fmap1.shape)} / {tuple(fmap2.shape)} differ "
                           "or are not [B, D, H, W]")
    if fmap1.device != fmap2.device:
        raise RuntimeError("fmap1 and fmap2 are on different devices")
    return live


def ptr(t):
    """An optional tensor as a pointer argument: None (NULL) for None."""
    return None if t is None else t.data_ptr()


def corr_channels(levels: int, radius: int) -> int:
    """Channels of a lookup: levels * (2r+1)^2."""
    return levels * (2 * radius + 1) ** 2


def layout(rows: int, H: int, W: int, levels: int):
    """(h[], w[], off[]) of the pyramid; raises like avg_pool2d on a 0-pixel level."""
    h = (_i * levels)()
    w = (_i * levels)()
    off = (_i64 * (levels + 1))()
    check(lib().ecorr_pyramid_layout(rows, H, W, levels, h, w, off), "CorrBlock pyramid")
    return list(h), list(w), list(off)


def stream_of(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def refuse_capture(what: str):
    """For the entry points that read an error flag on the host: they cannot be part of a HIP graph and
    say so themselves, before anything is launched."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what} reads an error flag on the host and cannot be captured into a HIP graph "
                           "(torch.cuda.graph): call it outside the captured region")


def tensor_version(t: torch.Tensor) -> int:
    """t's version counter, -1 for an inference tensor: it has none (in-place updates, legal under
    inference_mode, are then not seen)."""
    try:
        return t._version
    except RuntimeError:
        return -1


_same_device = contextlib.nullcontext()


def on_device(dev: torch.device):
    """The device context of every launch in the package, entered only when dev is not already current:
    the launches then go to dev's context, and the per-call host cost stays off the lookup path
    (12 calls per pair)."""
    return _same_device if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


_scratch_sizes = {}   # (size entry, dims) -> what it answered: the size entries are pure functions of their integers


def scratch(entry, *dims, device, what, dtype=torch.uint8, min_bytes=0):
    """A temporary from the caching allocator (released stream-ordered after its last launch) of the
    size that the library's size entry `entry` gives for the integers `dims`: bytes as uint8, or
    elements of `dtype` where the entry counts those.  None when that is 0 (ptr() makes it NULL);
    min_bytes=1 for an entry whose kernel wants a pointer anyway.  what: the text of a failure."""
    n = _scratch_sizes.get((entry, dims))
    if n is None:
        size = _i64()
        check(getattr(lib(), entry)(*dims, ctypes.byref(size)), what)
        if len(_scratch_sizes) >= 4096:   # event counts differ from call to call (voxel grids): stay bounded
            _scratch_sizes.clear()
        n = _scratch_sizes[(entry, dims)] = size.value
    n = max(n, min_bytes)
    return torch.empty(n, dtype=dtype, device=device) if n > 0 else None


# Which GEMM builds level 0 (include/ecorr.h): "split" = ecorr_build_split (f16 matrix cores on
# per-pixel-scaled hi/lo halves of every fp32 operand; error vs fp64 below the fp32 path's),
# "fp32" = ecorr_build (fp32 MFMA, an exact k-ordered fmaf chain per element).  Both meet the
# north star's 1e-5 bar against the reference's fp32 GEMM; ECORR_BUILD_MODE overrides.
BUILD_MODES = ("split", "fp32")
_build_mode = os.environ.get("ECORR_BUILD_MODE", "split")
if _build_mode not in BUILD_MODES:
    raise ValueError(f"ECORR_BUILD_MODE={_build_mode!r} not in {BUILD_MODES}")


# Timing hook (bench.py): when a list, every split build appends its (start, after the operand
# pass, after the GEMM) HIP events, recorded on the launch stream (start is None unless
# stage_event_start: bench.py times the operand pass outside its timed region, one event fewer per
# step -- each costs ~5 us of idle GPU).  Never changes a result.
stage_events = None
stage_event = None   # bench.py: the timing-event class for stage_events (default torch.cuda.Event)
stage_event_start = True


# Whether the split build of float16 / bfloat16 fmaps takes the hi-only entries
# (ecorr_build_split_pack_hi_as / ecorr_build_split_gemm_hi: one MFMA per product while every lo half is
# +-0, which finite 16-bit fmaps guarantee; bitwise the pyramid of the plain entries either way).
# On by default: at DSEC size the build is 14-16% shorter at B = 16 and 10-14% at B = 4, beyond the
# plain arm's spread in every run of profiles/hi_build/bench_hi_build.json.  ECORR_BUILD_HI = 0 | 1 overrides the default;
# fp32 fmaps never take the hi entries.
BUILD_HI_DEFAULT = "1"
_build_hi = os.environ.get("ECORR_BUILD_HI", BUILD_HI_DEFAULT)
if _build_hi not in ("0", "1"):
    raise ValueError(f"ECORR_BUILD_HI={_build_hi!r} not in ('0', '1')")
_build_hi = _build_hi == "1"


def set_build_hi(on: bool):
    global _build_hi
    if not isinstance(on, (bool, int)) or on not in (0, 1):
        raise ValueError(f"build_hi {on!r}: expected a bool")
    _build_hi = bool(on)


def build_hi() -> bool:
    return _build_hi


def set_build_mode(mode: str):
    global _build_mode
    if mode not in BUILD_MODES:
        raise ValueError(f"build mode {mode!r} not in {BUILD_MODES}")
    _build_mode = mode


def build_mode() -> str:
    return _build_mode


def build_pyramid(fmap1, fmap2, B, D, H, W, q_count, levels, off, what, mode=None):
    """Allocate the pyramid (levels at off[i]) on fmap2's device and build it on the current
    stream.  The split build's workspace (exponents + packed f16 operand panels, about the fmaps'
    size) is a temporary from the caching allocator, released stream-ordered after the launch.
    float16 / bfloat16 fmaps (both of one dtype, checked by the caller): the split build's operand pass
    reads them as they are (ecorr_build_split_pack_as: bitwise the pack of their .float()); the fp32
    build has no 16-bit input and gets .float() temporaries.  With build_hi() they take the hi-only
    entries instead: the same pyramid bit for bit, the GEMM on one MFMA per product."""
    mode = mode or _build_mode
    if mode not in BUILD_MODES:
        raise ValueError(f"build mode {mode!r} not in {BUILD_MODES}")
    pyr = torch.empty(off[-1], dtype=torch.float32, device=fmap2.device)
    st = stream_of(fmap2)
    if mode == "split":
        hi = _build_hi and fmap1.dtype != torch.float32
        ws = scratch("ecorr_build_split_hi_workspace_size" if hi else "ecorr_build_split_workspace_size",
                     B, D, H, W, q_count, device=fmap2.device, what=what)
        tm = stage_events
        if tm is not None:   # bench.py: HIP events on this stream around the two stages
            mk = stage_event or (lambda: torch.cuda.Event(enable_timing=True))
            ev = [mk() if stage_event_start else None, mk(), mk()]
            if ev[0] is not None:
                ev[0].record()
        if fmap1.dtype == torch.float32:
            check(lib().ecorr_build_split_pack(fmap1.data_ptr(), fmap2.data_ptr(), B, D, H, W, q_count,
                                               ws.data_ptr(), st), what)
        else:
            pack = lib().ecorr_build_split_pack_hi_as if hi else lib().ecorr_build_split_pack_as
            check(pack(fmap1.data_ptr(), fmap2.data_ptr(), ELEM_FORMATS[fmap1.dtype], B, D, H, W, q_count,
                       ws.data_ptr(), st), what)
        if tm is not None:
            ev[1].record()
        gemm = lib().ecorr_build_split_gemm_hi if hi else lib().ecorr_build_split_gemm
        check(gemm(B, D, H, W, q_count, levels, pyr.data_ptr(), ws.data_ptr(), st), what)
        if tm is not None:
            ev[2].record()
            tm.append(ev)
        del ws
    else:
        f1, f2 = fmap1.float(), fmap2.float()   # (fp32 fmaps: themselves)
        check(lib().ecorr_build(f1.data_ptr(), f2.data_ptr(), B, D, H, W, q_count, levels,
                                pyr.data_ptr(), st), what)
    return pyr


# Packed convc1 weights.  kind "fused": ecorr_conv1x1_pack (the fused lookup + convc1 kernel's fp32
# MFMA fragment order); "split": ecorr_conv1x1_split_pack (hi/lo f16 fragments + row exponents for
# ecorr_conv1x1_relu_split); "split_t": the same pack of the transposed weight (the backward's
# grad_in, ecorr_conv1x1_relu_backward).  ERAFT.forward builds one CorrBlock per forward and calls convc1 `iters`
# times with the same weight, so the caller passes a cache it owns (the CorrBlock instance's): the
# weight is re-laid once per block.  The key holds the tensor identity, its storage pointer and its
# version counter; a change through .data that keeps all three (w.data.mul_(...)) between two calls
# of ONE block is not seen -- weights are fixed during a forward.  The pack runs on the consumer's
# stream `st`, so the lookups that read it are ordered after it.
# kind: (size entry, pack entry, their two integers from (O, C), the weight transposed, the pack's element, label);
# the fused pack is sized in floats, the others in bytes; the presplit pack's columns are in the
# presplit corr's channel order (C = 81 * levels) and it takes the levels
_PACKS = {
    "fused": ("ecorr_conv1x1_packed_size", "ecorr_conv1x1_pack", lambda O, C: (O, C), False, torch.float32,
              "convc1 weight pack"),
    "split": ("ecorr_conv1x1_split_size", "ecorr_conv1x1_split_pack", lambda O, C: (O, C), False, torch.uint8,
              "convc1 split weight pack"),
    "split_t": ("ecorr_conv1x1_split_size", "ecorr_conv1x1_split_pack", lambda O, C: (C, O), True, torch.uint8,
                "convc1 transposed weight pack"),
    "presplit": ("ecorr_conv1x1_presplit_size", "ecorr_conv1x1_split_pack_presplit", lambda O, C: (O, C // 81), False,
                 torch.uint8, "convc1 presplit weight pack"),
}


def packed_conv1x1_weight(weight, O, C, kind, st, cache):
    version = tensor_version(weight)
    key = (kind, O, C)
    ent = cache.get(key)
    if ent is not None and ent[0] is weight and ent[1] == (weight.data_ptr(), version):
        return ent[2]
    size_entry, pack_entry, dims, transposed, dtype, label = _PACKS[kind]
    wt = weight.reshape(O, C).contiguous()
    if transposed:
        wt = wt.t().contiguous()
    packed = scratch(size_entry, *dims(O, C), device=weight.device, what=label, dtype=dtype)
    check(getattr(lib(), pack_entry)(wt.data_ptr(), *dims(O, C), packed.data_ptr(), st), label)
    cache[key] = (weight, (weight.data_ptr(), version), packed)
    return packed


def lookup(pyramid, coords, shape, q_count, levels, radius, out, what):
    """The ecorr_lookup launch of every block: the q_count queries of contiguous coords
    [B][2][q_count] into out ([B][C][q_count] fp32, returned), on the current stream of the pyramid's
    device.  shape = (B, H, W) of the build; what: the class name for error texts.  A float16 /
    bfloat16 out takes ecorr_lookup_as: the same launch with the 16-bit store."""
    B, H, W = shape
    with on_device(pyramid.device):
        if out.dtype == torch.float32:
            check(lib().ecorr_lookup(pyramid.data_ptr(), coords.data_ptr(), B, H, W, q_count, levels, radius,
                                     out.data_ptr(), stream_of(out)), f"{what} lookup")
        else:
            check(lib().ecorr_lookup_as(pyramid.data_ptr(), coords.data_ptr(), B, H, W, q_count, levels, radius,
                                        OUT_FORMATS[out.dtype], out.data_ptr(), stream_of(out)), f"{what} lookup")
    return out


def lookup_out_dtype(out_dtype):
    """The dtype of a lookup output for the out_dtype argument of CorrBlock.__call__: None = float32."""
    if out_dtype is None:
        return torch.float32
    if out_dtype not in OUT_FORMATS:
        raise TypeError(f"out_dtype must be None, torch.float32, torch.float16 or torch.bfloat16 (got {out_dtype!r})")
    return out_dtype


def convc1_mode(mode, presplit):
    """The convc1 mode of a lookup_conv1x1_relu call: `mode`, else env ECORR_CONVC1, else "split";
    presplit: whether the block has that mode."""
    mode = mode or os.environ.get("ECORR_CONVC1", "split")
    if mode not in ("split", "fused") and (mode != "presplit" or not presplit):
        raise ValueError(f"mode {mode!r}: expected 'split'" + (", 'presplit'" if presplit else "") + " or 'fused'")
    return mode


def lookup_conv1x1_relu(pyramid, coords, shape, q_count, levels, radius, weight, bias, mode, alloc_out, cache, what,
                        column_scale=None):
    """relu(conv1x1(lookup(coords), weight, bias)) for the q_count queries of one block (CorrBlock: all
    H * W; RowShardedCorrBlock: its rows): the body of both classes' lookup_conv1x1_relu.
    coords: contiguous [B][2][q_count], checked by the caller; shape = (B, H, W) of the build;
    alloc_out(O) -> the tensor of B * O * q_count elements to write (returned): fp32, or float16 /
    bfloat16 for the 16-bit output (the *_as entries of modes "split" and "fused"; "presplit" has no
    16-bit form and then runs as "split"); cache: the
    block's packed-weight cache; what: the class name for error texts.
    mode: what convc1_mode returned (the callers resolve it before their coords checks).
    column_scale (mode "presplit"): stream -> the presplit column exponents, or None when the block
    cannot give them (then, as for another radius or more levels: "split")."""
    B, H, W = shape
    dev = pyramid.device
    require_device("weight", weight)
    no_grad_inputs(weight, *(() if bias is None else (bias,)))
    if weight.device != dev or (bias is not None and bias.device != dev):
        raise RuntimeError("weight / bias are on a different device than the pyramid")
    C = corr_channels(levels, radius)
    O = weight.shape[0]
    if weight.numel() != O * C:
        raise RuntimeError(f"weight {tuple(weight.shape)} does not map {C} correlation channels")
    if bias is not None:
        require_device("bias", bias)
        if bias.numel() != O:
            raise RuntimeError(f"bias has {bias.numel()} elements, expected {O}")
        bias = bias.contiguous()
    if mode == "fused" and (O <= 0 or O % 64 != 0):
        raise RuntimeError(f"{O} output channels: the fused kernel needs a positive multiple of 64")
    bptr = ptr(bias)
    with on_device(dev):
        out = alloc_out(O)
        st = stream_of(out)
        fmt = OUT_FORMATS[out.dtype]
        if mode == "presplit" and fmt != ECORR_OUT_F32:
            mode = "split"
        if mode == "presplit":
            scale = column_scale(st) if radius == 4 and levels <= 4 else None
            if scale is None:
                mode = "split"
        wt = packed_conv1x1_weight(weight, O, C, mode, st, cache)   # once per block
        if mode == "presplit":
            corr = scratch("ecorr_presplit_size", B, levels, q_count, device=dev, what=f"{what} presplit size")
            check(lib().ecorr_lookup_presplit(
                pyramid.data_ptr(), coords.data_ptr(), B, H, W, q_count, levels, radius, scale.data_ptr(),
                corr.data_ptr(), st), f"{what} lookup (presplit convc1)")
            check(lib().ecorr_conv1x1_relu_presplit(
                corr.data_ptr(), B, levels, q_count, scale.data_ptr(), wt.data_ptr(), bptr, O, out.data_ptr(), st),
                f"{what} lookup+conv1x1+relu (presplit)")
        elif mode == "split":
            G = 3 * levels
            corr = torch.empty((B, C, q_count), dtype=torch.float32, device=dev)
            qmax = torch.empty((B, G, q_count), dtype=torch.float32, device=dev)
            check(lib().ecorr_lookup_qmax(
                pyramid.data_ptr(), coords.data_ptr(), B, H, W, q_count, levels, radius, corr.data_ptr(),
                qmax.data_ptr(), st), f"{what} lookup (split convc1)")
            if fmt == ECORR_OUT_F32:
                check(lib().ecorr_conv1x1_relu_split(
                    corr.data_ptr(), B, C, q_count, qmax.data_ptr(), G, wt.data_ptr(), bptr, O, out.data_ptr(), st),
                    f"{what} lookup+conv1x1+relu (split)")
            else:
                check(lib().ecorr_conv1x1_relu_split_as(
                    corr.data_ptr(), B, C, q_count, qmax.data_ptr(), G, wt.data_ptr(), bptr, O, fmt, out.data_ptr(),
                    st), f"{what} lookup+conv1x1+relu (split)")
        elif fmt == ECORR_OUT_F32:
            check(lib().ecorr_lookup_conv1x1_relu_packed(
                pyramid.data_ptr(), coords.data_ptr(), B, H, W, q_count, levels, radius, wt.data_ptr(), bptr, O,
                out.data_ptr(), st), f"{what} lookup+conv1x1+relu")
        else:
            check(lib().ecorr_lookup_conv1x1_relu_packed_as(
                pyramid.data_ptr(), coords.data_ptr(), B, H, W, q_count, levels, radius, wt.data_ptr(), bptr, O, fmt,
                out.data_ptr(), st), f"{what} lookup+conv1x1+relu")
    return out


def conv1x1_relu_backward(grad_out, out, corr, weight, cache, want_in, want_weight, want_bias, what):
    """ecorr_conv1x1_relu_backward for out = relu(conv1x1(corr, weight, bias)): (grad_in, grad_weight,
    grad_bias) on grad_out's current stream, None where not wanted.  grad_out, out: contiguous
    [B, O, ...]; corr: the conv's contiguous input [B, C, ...] (needed for want_weight only, else
    None); cache: the block's packed-weight cache (the transposed pack, kind "split_t", once per
    block, on this stream).  The workspace is a temporary from the caching allocator."""
    B, O = out.shape[0], out.shape[1]
    C = weight.numel() // O
    Q = out.numel() // (B * O)
    dev = out.device
    with on_device(dev):
        st = stream_of(out)
        ws = scratch("ecorr_conv1x1_relu_backward_workspace_size", B, C, Q, O, device=dev, what=what)
        pk = packed_conv1x1_weight(weight, O, C, "split_t", st, cache) if want_in else None
        gi = torch.empty((B, C) + tuple(out.shape[2:]), dtype=torch.float32, device=dev) if want_in else None
        gw = torch.empty(weight.shape, dtype=torch.float32, device=dev) if want_weight else None
        gb = torch.empty(O, dtype=torch.float32, device=dev) if want_bias else None
        check(lib().ecorr_conv1x1_relu_backward(
            grad_out.data_ptr(), out.data_ptr(), ptr(corr) if want_weight else None, ptr(pk), B, C, Q, O,
            ptr(gi), ptr(gw), ptr(gb), ptr(ws), st), what)
    return gi, gw, gb
