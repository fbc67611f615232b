"""GPU checks of ecorr_conv1x1_relu_backward (csrc/conv_grad.hip) through the raw C ABI, against the
fp64 references of tests/conv_grad_ref.py.

Inputs from tests/prng.py (weights x 0.05 as tests/test_conv_split_gpu.py); `out` is our own forward's
(ecorr_conv1x1_relu_split), and the references take their mask from that same out.  Bars (statistic:
max |d| / rms(ref), the project's normwise one):
    grad_in                  <= 1e-5 against fp64 (the split conv's bar);
    grad_weight, grad_bias   <= max(1e-5, 2 x ATen fp32's own distance to fp64) -- ATen's fp32 conv
                             backward on the same device and masked gradient, TF32 off.
Each test prints its distances.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_grad_ref as cg
import prng

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, C, Q, O): ragged Q with a 5000-term weight reduction over several slabs and the batch boundary;
# one whole tile; odd everything; grad_in's K loop with a remainder chunk and O past one 256 block;
# two remainder steps; Q = 1
SHAPES = [(2, 324, 2500, 256), (1, 324, 64, 256), (3, 243, 130, 96), (1, 81, 70, 300), (2, 100, 200, 20),
          (2, 20, 1, 64)]


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import eraft_amd
    eraft_amd.lib()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return eraft_amd


def _forward(x, w, bias):
    from eraft_amd import _lib
    B, C, Q = x.shape
    O = w.shape[0]
    pk = _lib.packed_conv1x1_weight(w, O, C, "split", _lib.stream_of(w), {})
    out = torch.empty((B, O, Q), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().ecorr_conv1x1_relu_split(
        x.data_ptr(), B, C, Q, None, 0, pk.data_ptr(), None if bias is None else bias.data_ptr(), O, out.data_ptr(),
        _lib.stream_of(x)), "split conv")
    torch.cuda.synchronize()
    return out


def _backward(go, out, x, w, want="iwb", fill=0.0):
    """The raw call; outputs and workspace pre-filled with `fill`.  -> {"i": grad_in, "w": .., "b": ..}."""
    from eraft_amd import _lib
    B, O, Q = out.shape
    C = w.shape[1]
    L = _lib.lib()
    n = ctypes.c_int64()
    _lib.check(L.ecorr_conv1x1_relu_backward_workspace_size(B, C, Q, O, ctypes.byref(n)), "size")
    ws = torch.full((n.value // 4,), fill, dtype=torch.float32, device=DEV)
    st = _lib.stream_of(out)
    pk = _lib.packed_conv1x1_weight(w, O, C, "split_t", st, {})
    res = {}
    if "i" in want:
        res["i"] = torch.full((B, C, Q), fill, dtype=torch.float32, device=DEV)
    if "w" in want:
        res["w"] = torch.full((O, C), fill, dtype=torch.float32, device=DEV)
    if "b" in want:
        res["b"] = torch.full((O,), fill, dtype=torch.float32, device=DEV)

    def ptr(k):
        return res[k].data_ptr() if k in res else None
    _lib.check(L.ecorr_conv1x1_relu_backward(go.data_ptr(), out.data_ptr(), x.data_ptr() if "w" in want else None,
                                             pk.data_ptr() if "i" in want else None, B, C, Q, O, ptr("i"), ptr("w"),
                                             ptr("b"), ws.data_ptr(), st), "conv backward")
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, our forward's out, our three gradients and the fp64 references of one shape, computed once."""
    B, C, Q, O = shape
    x = prng.normal(801, (B, C, Q))
    w = (prng.normal(802, (O, C)) * np.float32(0.05)).astype(np.float32)
    bias = (prng.normal(803, (O,)) * np.float32(0.1)).astype(np.float32)
    go = prng.normal(804, (B, O, Q))
    t = {k: torch.from_numpy(v).to(DEV) for k, v in (("x", x), ("w", w), ("bias", bias), ("go", go))}
    t["out"] = _forward(t["x"], t["w"], t["bias"])
    out = t["out"].cpu().numpy()
    got = _backward(t["go"], t["out"], t["x"], t["w"])
    ref = dict(zip("iwb", cg.grads(go, out, x, w)))
    return t, {"x": x, "w": w, "go": go, "out": out}, got, ref


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d_c%d_q%d_o%d" % s)
def test_grads_vs_fp64(ea, shape):
    _, n, got, ref = _case(shape)
    aw, ab = cg.aten_fp32_grads(n["go"], n["out"], n["x"], n["w"], device=DEV)
    ei = cg.normwise(got["i"].cpu().numpy(), ref["i"])
    ew, eb = cg.normwise(got["w"].cpu().numpy(), ref["w"]), cg.normwise(got["b"].cpu().numpy(), ref["b"])
    fw, fb = cg.normwise(aw, ref["w"]), cg.normwise(ab, ref["b"])
    print(f"{shape}: normwise vs fp64 grad_in {ei:.3g}; grad_weight {ew:.3g} (ATen fp32 {fw:.3g}); "
          f"grad_bias {eb:.3g} (ATen fp32 {fb:.3g})")
    assert (n["out"] > 0).any() and (n["out"] == 0).any()
    assert ei <= 1e-5
    assert ew <= max(1e-5, 2 * fw)
    assert eb <= max(1e-5, 2 * fb)


def test_zero_column_and_dead_channel(ea):
    """A query whose out column is all zero gets an exactly zero grad_in column; a channel a large
    negative bias keeps non-positive everywhere gets an exactly zero grad_weight row and grad_bias entry."""
    B, C, Q, O = 2, 100, 200, 20
    x = prng.normal(811, (B, C, Q))
    x[:, :, 5] = 0.0
    x[1, :, 199] = 0.0
    w = (prng.normal(812, (O, C)) * np.float32(0.05)).astype(np.float32)
    bias = np.zeros(O, np.float32)
    bias[3] = -1.0e3
    go = prng.normal(813, (B, O, Q))
    xt, wt, bt, got_ = (torch.from_numpy(a).to(DEV) for a in (x, w, bias, go))
    out = _forward(xt, wt, bt)
    o = out.cpu().numpy()
    assert not o[:, :, 5].any() and not o[1, :, 199].any() and not o[:, 3, :].any() and (o > 0).any()
    r = _backward(got_, out, xt, wt, fill=float("nan"))
    gi, gw, gb = (r[k].cpu().numpy() for k in "iwb")
    assert np.all(gi[:, :, 5] == 0.0) and np.all(gi[1, :, 199] == 0.0)
    assert np.all(gw[3] == 0.0) and gb[3] == 0.0
    ri, rw, rb = cg.grads(go, o, x, w)
    assert cg.normwise(gi, ri) <= 1e-5 and cg.normwise(gw, rw) <= 1e-5 and cg.normwise(gb, rb) <= 1e-5


def test_grad_out_scales(ea):
    """Per-query grad_out scales 2^-40 .. 2^40: every query column of the masked gradient gets its own
    exponent, so each grad_in element keeps the split's relative error of its own products (the
    per-element bar of test_conv_split_gpu.test_scales_and_zero_columns)."""
    B, C, Q, O = 2, 324, 700, 256
    x = prng.normal(821, (B, C, Q))
    w = (prng.normal(822, (O, C)) * np.float32(0.05)).astype(np.float32)
    go = prng.normal(823, (B, O, Q))
    go = (go * np.exp2(np.linspace(-40, 40, Q)).astype(np.float32)[None, None, :]).astype(np.float32)
    xt, wt, got_ = (torch.from_numpy(a).to(DEV) for a in (x, w, go))
    out = _forward(xt, wt, None)
    gi = _backward(got_, out, xt, wt, want="i")["i"].cpu().numpy().astype(np.float64)
    o = out.cpu().numpy()
    ref, _, _ = cg.grads(go, o, None, w)
    own = np.einsum("oc,boq->bcq", np.abs(w.astype(np.float64)), np.abs(cg.masked(go, o)), optimize=True)
    rel = np.abs(gi - ref) / np.maximum(own, 1e-300)
    print(f"grad_out scales 2^-40..2^40: max per-element relative error {rel.max():.3g}")
    assert rel.max() <= 1e-5, rel.max()


@pytest.mark.parametrize("shape", [(3, 243, 130, 96), (1, 81, 70, 300), (2, 324, 2500, 256)],
                         ids=lambda s: "b%d_c%d_q%d_o%d" % s)
def test_bitwise_properties(ea, shape):
    """NaN-filled outputs and workspace give the bits of clean buffers (every element overwritten,
    nothing read before it is written); each output computed alone is bitwise the all-three call;
    two calls give equal bits."""
    t, _, got, _ = _case(shape)
    args = (t["go"], t["out"], t["x"], t["w"])
    nan = _backward(*args, fill=float("nan"))
    for k in "iwb":
        assert torch.equal(nan[k].view(torch.int32), got[k].view(torch.int32)), k
    for k in "iwb":
        alone = _backward(*args, want=k, fill=float("nan"))
        assert list(alone) == [k]
        assert torch.equal(alone[k].view(torch.int32), got[k].view(torch.int32)), k
    again = _backward(*args)
    for k in "iwb":
        assert torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)), k


def test_nan_in_out_passes_and_poisons_its_query(ea):
    """The documented non-finite contract: a NaN in out passes the gradient (threshold_backward); a
    non-finite masked gradient makes that query's whole grad_in column NaN and no other."""
    t, n, got, _ = _case((1, 324, 64, 256))
    go = t["go"].clone()
    go[0, 7, 33] = float("inf")
    out = t["out"].clone()
    out[0, 7, 33] = float("nan")   # passes the inf through
    gi = _backward(go, out, t["x"], t["w"], want="i")["i"].cpu().numpy()
    assert np.all(np.isnan(gi[0, :, 33]))
    keep = np.ones(64, bool)
    keep[33] = False
    assert np.array_equal(gi[0][:, keep], got["i"].cpu().numpy()[0][:, keep])
