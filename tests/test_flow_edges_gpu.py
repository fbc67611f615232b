"""The flow side's forward (csrc/upsample.hip: upsample_kernel and the DSEC PNG codec) on the GPU at its
edges: the shapes of tests/flow_cases.py against the fp64 reference (pinned on the CPU by
tests/test_flow_ref.py), one-hot masks and power-of-two scalings bit for bit, non-finite inputs against
the CPU module's footprint, outputs between guard bands through the raw C ABI, the codec's second
grid-stride pass, B > 1 and the exact count in *bad, and a gradient arriving at an unaligned address.

Bar of the value test: per batch item, oracle.normwise_err(ours, fp64) <= max(UPSAMPLE_TOL, 2 x ATen's),
ATen's being the fp32 ERAFT.upsample_flow on the same GPU and inputs with TF32 off: the project's rule
of two independent fp32 evaluations (test_grad_edges_gpu.py, test_upsample_grad_gpu.py), with the
kernel's existing bar as the floor.  Everything else here is compared without a tolerance.
"""
import ctypes

import numpy as np
import pytest
import torch

import flow_cases as fc
import oracle
from gpu_guard import check_guarded, check_guarded_u8, check_guarded_u16, guarded, guarded_u8, guarded_u16, mismatch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
UPSAMPLE_TOL = fc.UPSAMPLE_TOL


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import eraft_amd
    eraft_amd.lib()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return eraft_amd


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # a copy: the cached cases are read-only


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _module(flow, mask):
    """ERAFT.upsample_flow on whatever device and dtype the tensors have."""
    from eraft_amd.network import ERAFT
    with torch.no_grad():
        return ERAFT.upsample_flow(flow, mask)


def _cpu_module(flow, mask):
    return _module(torch.from_numpy(np.array(flow)), torch.from_numpy(np.array(mask))).numpy()


def _ours(ea, flow, mask):
    return ea.upsample_flow(_dev(flow), _dev(mask)).cpu().numpy()


def _within_bar(ea, flow, mask, ref, what):
    """The value bar, per batch item; prints ours and ATen's."""
    f, m = _dev(flow), _dev(mask)
    got, aten = ea.upsample_flow(f, m).cpu().numpy(), _module(f, m).cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    for n in range(got.shape[0]):
        e_ours, e_aten = oracle.normwise_err(got[n], ref[n]), oracle.normwise_err(aten[n], ref[n])
        print(f"upsample forward {what} item {n}: normwise vs fp64 ours {e_ours:.3g}, ATen fp32 {e_aten:.3g}")
        assert e_ours <= max(UPSAMPLE_TOL, 2.0 * e_aten), (what, n, e_ours, e_aten)


# ---- a: values against fp64 ---------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,W,ms", fc.CASES)
def test_values_vs_fp64(ea, N, H, W, ms):
    flow, mask, out64 = fc.case(N, H, W, ms)
    _within_bar(ea, flow, mask, out64, f"({N},{H},{W}) mask scale {ms:g}")


# ---- b: one-hot masks, bit for bit --------------------------------------------------------------------

@pytest.mark.parametrize("low", [-np.inf, -120.0])
@pytest.mark.parametrize("N,H,W", list(fc.SHAPES))
def test_onehot_bitwise(ea, N, H, W, low):
    """Pins the tap order k = 3 ky + kx, the (i, j) layout of the mask, the 8x interleave of the output,
    both borders and the batch stride: every element is 8 * flow of the one selected neighbour."""
    flow, mask, want, _ = fc.onehot(N, H, W, low)
    assert mismatch(_cpu_module(flow, mask), want) is None, "the fp32 module itself"   # the expectation is the reference's
    bad = mismatch(_ours(ea, flow, mask), want)
    assert bad is None, bad


# ---- c: power-of-two scaling, bit for bit -------------------------------------------------------------

@pytest.mark.parametrize("N,H,W", [(3, 5, 53), (1, 1, 7)])
def test_power_of_two_scaling_bitwise(ea, N, H, W):
    """Everything after the softmax is a rounded multiply or add, so scaling flow by 2^e scales every
    output by 2^e exactly (mask scale 1: weights >= ~1e-6, outputs ~ 1e1, nothing near overflow or the
    subnormal range at e = -20, 20)."""
    flow, mask = fc.inputs(N, H, W, 1.0)
    base = _ours(ea, flow, mask)
    assert np.isfinite(base).all() and np.abs(base[base != 0]).min() > 1e-12 and np.abs(base).max() < 1e3
    for e in (-20, 20):
        s = np.float32(2.0 ** e)
        bad = mismatch(_ours(ea, flow * s, mask), base * s)
        assert bad is None, (e, bad)


# ---- d: non-finite values keep the reference's footprint ----------------------------------------------

def _blocks(shape, n, c, y, x):
    """The 8 x 8 output blocks of channel c of the 3 x 3 pixels around (y, x), clipped to the map."""
    N, H, W = shape
    hit = np.zeros((N, 2, 8 * H, 8 * W), dtype=bool)
    hit[n, c, 8 * max(y - 1, 0):8 * min(y + 2, H), 8 * max(x - 1, 0):8 * min(x + 2, W)] = True
    return hit


@pytest.mark.parametrize("where", ["interior", "corner"])
def test_nan_in_flow_stays_on_its_blocks(ea, where):
    N, H, W = 3, 5, 53
    flow, mask = fc.inputs(N, H, W, 1.0)
    n, c, y, x = (1, 1, 2, 30) if where == "interior" else (2, 0, H - 1, W - 1)
    clean = _ours(ea, flow, mask)
    assert np.isfinite(clean).all()
    dirty_in = flow.copy()
    dirty_in[n, c, y, x] = np.nan
    hit = _blocks((N, H, W), n, c, y, x)
    assert int(hit.sum()) == (9 if where == "interior" else 4) * 64
    assert np.array_equal(np.isnan(_cpu_module(dirty_in, mask)), hit)   # the reference's own footprint
    got = _ours(ea, dirty_in, mask)
    assert np.array_equal(np.isnan(got), hit)
    assert np.array_equal(got.view(np.uint32)[~hit], clean.view(np.uint32)[~hit])


def test_inf_in_flow_follows_the_reference(ea):
    """Mask scale 1: every weight is a normal number (no 0 * inf), so +-inf times a weight is +-inf and
    NaN appears only where +inf and -inf meet in one window.  The CPU module decides the pattern."""
    N, H, W = 3, 5, 53
    flow, mask = fc.inputs(N, H, W, 1.0)
    clean = _ours(ea, flow, mask)
    dirty_in = flow.copy()
    dirty_in[0, 0, 2, 10] = np.inf
    dirty_in[0, 0, 2, 12] = -np.inf     # the windows of column 11 hold both
    dirty_in[1, 1, 0, 0] = -np.inf      # a corner, alone
    dirty_in[2, 0, 4, 52] = np.inf      # the last pixel of the last item
    ref = _cpu_module(dirty_in, mask)
    touched = (_blocks((N, H, W), 0, 0, 2, 10) | _blocks((N, H, W), 0, 0, 2, 12) | _blocks((N, H, W), 1, 1, 0, 0)
               | _blocks((N, H, W), 2, 0, 4, 52))
    assert np.array_equal(~np.isfinite(ref), touched)                   # the reference's own footprint
    assert np.isnan(ref).any() and (ref == np.inf).any() and (ref == -np.inf).any()
    assert np.array_equal(np.isnan(ref), _blocks((N, H, W), 0, 0, 2, 10) & _blocks((N, H, W), 0, 0, 2, 12))
    got = _ours(ea, dirty_in, mask)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got == np.inf, ref == np.inf) and np.array_equal(got == -np.inf, ref == -np.inf)
    assert np.array_equal(got.view(np.uint32)[~touched], clean.view(np.uint32)[~touched])


SUBPIXEL = (0, 4, 6, 2, 3)   # (n, i, j, h, w) on the 5 x 6 map


def _logits(kind):
    """The nine logits of SUBPIXEL for `kind`, from the clean ones."""
    N, H, W = 1, 5, 6
    flow = fc.inputs(3, 5, 53, 1.0)[0][:1, :, :, :W].copy()
    mask = fc.inputs(3, 5, 53, 1.0)[1][:1, :, :, :W].copy()
    n, i, j, h, w = SUBPIXEL
    taps = mask.reshape(N, 9, 8, 8, H, W)[n, :, i, j, h, w]   # a view
    if kind == "all -inf":
        taps[:] = -np.inf
    elif kind == "one +inf":
        taps[7] = np.inf
    elif kind == "one nan":
        taps[2] = np.nan
    elif kind == "one -inf":
        taps[5] = -np.inf
    return flow, mask


@pytest.mark.parametrize("kind", ["all -inf", "one +inf", "one nan"])
def test_non_finite_logits_stay_in_their_sub_pixel(ea, kind):
    """softmax9 takes its maximum with fmaxf, which drops a NaN where ATen's max propagates it; the NaN
    comes back through the sum.  Exactly the sub-pixel's two elements (c = 0, 1) are NaN."""
    N, H, W = 1, 5, 6
    flow, clean_mask = _logits("clean")
    flow, mask = _logits(kind)
    n, i, j, h, w = SUBPIXEL
    hit = np.zeros((N, 2, 8 * H, 8 * W), dtype=bool)
    hit[n, :, 8 * h + i, 8 * w + j] = True
    assert int((mask != clean_mask).sum()) == (9 if kind == "all -inf" else 1)
    ref_clean, ref = _cpu_module(flow, clean_mask), _cpu_module(flow, mask)
    assert np.array_equal(np.isnan(ref), hit) and int(hit.sum()) == 2   # the reference's own footprint
    assert np.array_equal(ref.view(np.uint32)[~hit], ref_clean.view(np.uint32)[~hit])
    clean, got = _ours(ea, flow, clean_mask), _ours(ea, flow, mask)
    assert np.array_equal(np.isnan(got), hit)
    assert np.array_equal(got.view(np.uint32)[~hit], clean.view(np.uint32)[~hit])


def test_one_minus_inf_logit_is_a_zero_weight(ea):
    flow, mask = _logits("one -inf")
    assert int(np.isinf(mask).sum()) == 1
    ref = fc.reference(flow, mask)
    assert np.isfinite(ref).all() and np.isfinite(_cpu_module(flow, mask)).all()
    _within_bar(ea, flow, mask, ref, "(1,5,6) one -inf logit")   # asserts finiteness of ours too


# ---- e: guards, through the raw C ABI -----------------------------------------------------------------

@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 1, 300), (3, 5, 53)])
def test_out_between_guards(ea, N, H, W):
    """ecorr_upsample_flow itself, on ordinary logits and on the one-hot mask: both guards intact, every
    element written, the bits of eraft_amd.upsample_flow -- and, one-hot, the expectation's, so what
    the raw entry writes between the guards is also the right value in the right place."""
    from eraft_amd import _lib
    for flow, mask, expect in (fc.inputs(N, H, W, 1.0) + (None,), fc.onehot(N, H, W, -np.inf)[:3]):
        f, m = _dev(flow), _dev(mask)
        want = ea.upsample_flow(f, m).cpu().numpy()
        buf, out = guarded(N * 2 * 64 * H * W)
        assert out.data_ptr() % 16 == 0
        _lib.check(_lib.lib().ecorr_upsample_flow(f.data_ptr(), m.data_ptr(), N, H, W, out.data_ptr(), _stream()),
                   "upsample")
        torch.cuda.synchronize()
        got = check_guarded(buf, f"out ({N},{H},{W})").reshape(want.shape)
        for bad in (mismatch(got, want), None if expect is None else mismatch(got, expect)):
            assert bad is None, bad


# ---- f: the codec: second grid-stride pass, B > 1, guards, the exact *bad ------------------------------

def _encode_guarded(flow):
    from eraft_amd import _lib
    B, _, h, w = flow.shape
    f = _dev(flow)
    buf, out = guarded_u16(B * h * w * 3)
    _lib.check(_lib.lib().ecorr_flow_to_png16(f.data_ptr(), B, h, w, out.data_ptr(), _stream()), "encode")
    torch.cuda.synchronize()
    return check_guarded_u16(buf, f"png ({B},{h},{w})").reshape(B, h, w, 3)


def test_encode_small_batch_between_guards(ea):
    flow = fc.inputs(3, 5, 53, 1.0)[0][:, :, :, :7] * np.float32(10.0)
    want = oracle.flow_to_png16(flow)
    assert want.shape == (3, 5, 7, 3)
    assert np.array_equal(_encode_guarded(flow), want)


def test_encode_second_pass(ea):
    """h * w one row past what a single pass of the capped grid covers: the loop's second pass encodes
    the tail, the special values among it."""
    flow = fc.codec_flow_large()
    _, _, h, w = flow.shape
    assert h * w > fc.CODEC_PASS >= h * w - w
    want = oracle.flow_to_png16(flow)
    assert len(np.unique(want[0, -1, -100:, :2])) > 16      # the tail is not one value
    got = _encode_guarded(flow)
    diff = np.flatnonzero((got != want).reshape(-1, 3).any(axis=1))
    assert diff.size == 0, f"{diff.size} pixels differ, first at {diff[0]} (one pass covers {fc.CODEC_PASS})"


def _decode_guarded(png, calls=1):
    """ecorr_png16_to_flow on uint16 [B, h, w, 3] -> (flow [B, h, w, 2], valid [B, h, w], *bad after
    `calls` calls that started from *bad = 0)."""
    from eraft_amd import _lib
    B, h, w, _ = png.shape
    src = _dev(png.view(np.int16)).view(torch.uint16)
    fbuf, flow = guarded(B * h * w * 2)
    vbuf, valid = guarded_u8(B * h * w)
    bad = torch.zeros((1,), dtype=torch.int32, device=DEV)
    for _ in range(calls):
        _lib.check(_lib.lib().ecorr_png16_to_flow(src.data_ptr(), B, h, w, flow.data_ptr(), valid.data_ptr(),
                                                  bad.data_ptr(), _stream()), "decode")
    torch.cuda.synchronize()
    return (check_guarded(fbuf, f"flow ({B},{h},{w})").reshape(B, h, w, 2),
            check_guarded_u8(vbuf, f"valid ({B},{h},{w})").reshape(B, h, w), int(bad.item()))


def _check_decode(png, bad_at):
    B, h, w, _ = png.shape
    n_bad = int((png[..., 2] > 1).sum())
    assert n_bad == len(bad_at) and (png.reshape(-1, 3)[list(bad_at), 2] > 1).all()
    flow, valid, bad = _decode_guarded(png)
    for b in range(B):
        want_flow, want_valid, want_bad = oracle.flow_16bit_to_float(png[b])
        assert want_bad == int((png[b, ..., 2] > 1).sum())
        assert np.array_equal(valid[b], want_valid.astype(np.uint8)), b
        d = np.flatnonzero((flow[b].view(np.uint32) != want_flow.view(np.uint32)).reshape(-1, 2).any(axis=1))
        assert d.size == 0, f"item {b}: {d.size} pixels differ, first at {d[0]}"
    assert bad == n_bad, f"*bad = {bad}, {n_bad} pixels have channel 2 above 1"
    return n_bad


def test_decode_small_batch(ea):
    """B = 3 (the Python wrapper always passes 1); channel 2 above 1 at the first pixel, in item 2 and at
    the last pixel; *bad is their exact number, and a call on a non-zero *bad adds to it."""
    bad_at = (0, 2 * 35 + 3, 3 * 35 - 1)
    png = fc.codec_png(3, 5, 7, bad_at)
    assert png[0, 0, 0, 2] == 2          # the smallest value above 1 is among them
    n_bad = _check_decode(png, bad_at)
    assert _decode_guarded(png, calls=2)[2] == 2 * n_bad


def test_decode_second_pass(ea):
    h, w = fc.CODEC_LARGE_H, fc.CODEC_LARGE_W
    bad_at = (0, fc.CODEC_PASS - 1, fc.CODEC_PASS, h * w - 1)
    _check_decode(fc.codec_png(1, h, w, bad_at), bad_at)


# ---- alignment: an offset view from Python ------------------------------------------------------------

def test_gradient_at_an_unaligned_address(ea):
    """A contiguous gradient one float into its storage is legal in Python; the C ABI refuses it
    (tests/test_flow_abi.py), so the wrapper copies it: the bits are the aligned call's."""
    N, H, W = 2, 3, 5
    flow, mask = fc.inputs(3, 5, 53, 1.0)
    f, m = _dev(flow[:N, :, :H, :W]), _dev(mask[:N, :, :H, :W])
    g = torch.from_numpy(np.array(fc.inputs(2, 16, 16, 1.0)[1].reshape(-1)[:N * 2 * 64 * H * W])).to(DEV)
    buf = torch.zeros(g.numel() + 1, dtype=torch.float32, device=DEV)
    buf[1:] = g
    view = buf[1:].view(N, 2, 8 * H, 8 * W)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 0
    grads = []
    for go in (g.view(N, 2, 8 * H, 8 * W), view):
        fr, mr = f.clone().requires_grad_(True), m.clone().requires_grad_(True)
        ea.upsample_flow(fr, mr).backward(go)
        grads.append((fr.grad, mr.grad))
    assert bool(torch.isfinite(grads[0][0]).all()) and bool((grads[0][1] != 0).any())
    assert torch.equal(grads[0][0].view(torch.int32), grads[1][0].view(torch.int32))
    assert torch.equal(grads[0][1].view(torch.int32), grads[1][1].view(torch.int32))
