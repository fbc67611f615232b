"""The fp64 reference of tests/test_flow_edges_gpu.py (flow_cases.reference), checked on the CPU.

  * Against ERAFT.upsample_flow evaluated in fp64 on the CPU, on every case: both are fp64 evaluations of
    one expression in different orders (ATen's softmax and sum against the in-order loops), so they agree
    to fp64 rounding.  The bound is per element, 2 * 2^-53 * A with A the element's error scale
    (flow_cases.reference: sum_k s_k (20 + d_k) |8 flow_k|), one 2^-53 * A for each side.
  * Against the committed goldens (tests/golden/next_flow.npz, keys up_*): those are the reference
    project's fp32 outputs, so here the other side's unit roundoff is 2^-24 and the bound per element is
    2^-24 * A (+ 2^-140 per tap for weights in fp32's subnormal range); the fp64 side adds nothing visible.
    Both hold with the same A, the one derived in flow_cases.reference; it is not fitted to either result.
  * The one-hot expectation of the GPU test, from the fp32 module itself: its bits are 8 * flow of the
    drawn neighbour.  And what keeps the GPU comparison from passing on nothing: every tap index is drawn,
    padding is selected and so is an inside neighbour, on every shape.
"""
import os

import numpy as np
import pytest
import torch

import flow_cases as fc
import oracle
from conftest import GOLDEN
from gpu_guard import mismatch


def _expr(flow, mask):
    from eraft_amd.network import ERAFT
    with torch.no_grad():
        return ERAFT.upsample_flow(torch.from_numpy(np.array(flow)), torch.from_numpy(np.array(mask))).numpy()


@pytest.mark.parametrize("N,H,W,ms", fc.CASES)
def test_reference_is_the_module_in_fp64(N, H, W, ms):
    flow, mask = fc.inputs(N, H, W, ms)
    ref, A = fc.reference(flow, mask, with_scale=True)
    assert np.array_equal(ref, fc.case(N, H, W, ms)[2])
    got = _expr(flow.astype(np.float64), mask.astype(np.float64))
    assert got.dtype == np.float64 and got.shape == ref.shape == (N, 2, 8 * H, 8 * W)
    assert np.isfinite(ref).all() and np.sqrt(np.mean(ref * ref)) > 1.0
    d = np.abs(got - ref)
    print(f"({N},{H},{W}) mask scale {ms:g}: normwise {oracle.normwise_err(got, ref):.3g}, "
          f"max |d| / (2^-53 A) {float(np.max(d / (2.0 ** -53 * A))):.3g}")
    assert (d <= 2.0 * 2.0 ** -53 * A).all()


def test_reference_reproduces_the_goldens():
    from test_oracle_next import upsample_inputs
    z = np.load(os.path.join(GOLDEN, "next_flow.npz"))
    names = sorted(k.split("/")[0] for k in z.files if k.startswith("up_") and k.endswith("/out"))
    assert len(names) >= 4
    for k in names:
        flow, mask = upsample_inputs(z, k)
        ref, A = fc.reference(flow, mask, with_scale=True)
        want = z[f"{k}/out"]
        assert want.dtype == np.float32 and want.shape == ref.shape
        d = np.abs(want.astype(np.float64) - ref)
        bound = 2.0 ** -24 * A + 9 * 2.0 ** -140 * 8.0 * float(np.abs(flow).max())
        print(f"{k}: normwise {oracle.normwise_err(want, ref):.3g}, max |d| / bound {float(np.max(d / bound)):.3g}")
        assert (d <= bound).all(), k


@pytest.mark.parametrize("low", [-np.inf, -120.0])
@pytest.mark.parametrize("N,H,W", list(fc.SHAPES))
def test_onehot_expectation_is_the_modules_bits(N, H, W, low):
    flow, mask, want, pick = fc.onehot(N, H, W, low)
    assert (np.float32(np.exp(np.float64(-120.0))) == 0.0) and np.exp(np.float32(-120.0)) == 0.0
    m = mask.reshape(N, 9, 64, H, W)
    assert ((m == 0).sum(axis=1) == 1).all() and ((m == np.float32(low)).sum(axis=1) == 8).all()
    assert mismatch(_expr(flow, mask), want) is None
    assert not np.signbit(want[want == 0]).any()
    assert np.array_equal(fc.reference(flow, mask).astype(np.float32), want)   # and the fp64 loops agree
    # the draw reaches every tap, padding and (but for the 1 x 1 map's off-centre taps) inside neighbours
    assert set(np.unique(pick)) == set(range(9))
    hh, ww = np.arange(H)[:, None], np.arange(W)[None, :]
    y, x = hh + pick // 3 - 1, ww + pick % 3 - 1
    inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    assert (~inside).any() and inside.any()
    if H > 1 or W > 1:
        assert (inside & (pick != 4)).any()


def test_shapes_reach_what_they_claim():
    hw = {s: s[1] * s[2] for s in fc.SHAPES}
    assert hw[(3, 5, 53)] == fc.NTU + 9 and fc.NTU % 53 != 0            # a 9-thread tail, the boundary mid-row
    assert hw[(2, 16, 16)] == fc.NTU                                    # one full block
    assert fc.NTU < hw[(2, 1, 300)] == hw[(2, 300, 1)] < 2 * fc.NTU     # a boundary inside the map, N > 1
    assert hw[(1, 17, 31)] == 2 * fc.NTU + 15
    src = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "e-raft_amd", "csrc", "upsample.hip")).read()
    assert "constexpr int NTU = 256;" in src and fc.NTU == 256
    assert "g < 16384 ? (g > 0 ? g : 1) : 16384" in src and fc.CODEC_PASS == 16384 * 256
    assert fc.CODEC_LARGE_H * fc.CODEC_LARGE_W - fc.CODEC_PASS == fc.CODEC_LARGE_W
