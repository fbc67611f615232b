"""The 16-bit convc1 output (ecorr_conv1x1_relu_split_as, ecorr_lookup_conv1x1_relu_packed_as,
CorrBlock.lookup_conv1x1_relu(..., out_dtype=...)) on the GPU.

Contract (include/ecorr.h): each element is the fp32 value the fp32 entry writes, after bias and ReLU,
rounded once to nearest-even.  So for both dtypes and both modes the 16-bit output, read as int16 bit
patterns, must equal the fp32 call's output converted by torch.Tensor.to(dtype) wherever that is not
NaN, and be NaN exactly where it is.  No tolerance anywhere.

Shapes: 23 x 40 with B = 2 (Q = 920 = 14.4 query blocks of the split conv, 28.75 of the fused kernel), 4
levels and 1 level, O = 64 (both modes) and O = 96 (split: a partial output block; the fused kernel
takes multiples of 64); and a 5 x 7 map, 1 level: Q = 35 odd, so output rows start on 2-byte boundaries
only.  Coordinates carry one NaN query per batch item, so NaN outputs occur."""
import numpy as np
import pytest
import torch

import prng

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]

# name: (B, D, H, W, levels, O, modes)
CASES = {
    "23x40_l4_o64": (2, 8, 23, 40, 4, 64, ("split", "fused")),
    "23x40_l1_o64": (2, 8, 23, 40, 1, 64, ("split", "fused")),
    "23x40_l4_o96": (2, 8, 23, 40, 4, 96, ("split",)),
    "23x40_l1_o96": (2, 8, 23, 40, 1, 96, ("split",)),
    "odd_q_5x7_l1_o64": (2, 8, 5, 7, 1, 64, ("split", "fused")),
}
RUNS = [(n, m) for n in sorted(CASES) for m in CASES[n][6]]


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_bits(out16, out32, dt, what):
    """out16 == out32.to(dt) as bit patterns off the NaNs, NaN exactly where out32 is."""
    assert out16.dtype == dt and out16.shape == out32.shape
    nan32 = torch.isnan(out32)
    assert torch.equal(torch.isnan(out16), nan32), f"{what}: NaN positions differ"
    want = out32.to(dt)
    same = (_bits(out16) == _bits(want)) | nan32
    bad = int((~same).sum())
    if bad:
        i = int(torch.nonzero(~same.reshape(-1))[0])
        pytest.fail(f"{what}: {bad} of {same.numel()} elements differ; first at flat index {i}: fp32 "
                    f"{out32.reshape(-1)[i].item()!r} -> {out16.reshape(-1)[i].item()!r}, expected "
                    f"{want.reshape(-1)[i].item()!r}")


@pytest.fixture(scope="module")
def fp32_runs(ea):
    """case -> (block, coords, weight, bias, {mode: fp32 output}): once, shared by both dtypes, never written."""
    cache = {}

    def get(name):
        if name not in cache:
            B, D, H, W, L, O, modes = CASES[name]
            seed = 1100 + 10 * sorted(CASES).index(name)
            f1 = torch.from_numpy(prng.normal(seed, (B, D, H, W))).to(DEV)
            f2 = torch.from_numpy(prng.normal(seed + 1, (B, D, H, W))).to(DEV)
            blk = ea.CorrBlock(f1, f2, num_levels=L, radius=4)
            c = prng.coords_with_flow(seed + 2, B, H, W, 2.0)
            c[:, :, H // 2, W // 2] = np.nan                       # one NaN query per batch item
            coords = torch.from_numpy(c).to(DEV)
            wt = torch.from_numpy(prng.normal(seed + 3, (O, 81 * L, 1, 1), 0.1)).to(DEV)
            bias = torch.from_numpy(prng.normal(seed + 4, (O,), 0.5)).to(DEV)
            outs = {m: blk.lookup_conv1x1_relu(coords, wt, bias, mode=m) for m in modes}
            torch.cuda.synchronize()
            cache[name] = (blk, coords, wt, bias, outs)
        return cache[name]
    return get


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name,mode", RUNS)
def test_half_output_is_the_rounded_fp32_output(ea, fp32_runs, name, mode, dt):
    blk, coords, wt, bias, outs = fp32_runs(name)
    out32 = outs[mode]
    assert out32.dtype == torch.float32
    assert bool(torch.isnan(out32).any()) and bool((out32 == 0).any()) and bool((out32 > 0).any())
    out16 = blk.lookup_conv1x1_relu(coords, wt, bias, mode=mode, out_dtype=dt)
    torch.cuda.synchronize()
    _check_bits(out16, out32, dt, f"{name} / {mode}")
    # None and float32 are the fp32 call
    for same in (None, torch.float32):
        o = blk.lookup_conv1x1_relu(coords, wt, bias, mode=mode, out_dtype=same)
        assert o.dtype == torch.float32
        assert torch.equal(o.view(torch.int32), out32.view(torch.int32))


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_no_bias_and_presplit_runs_as_split(ea, fp32_runs, dt):
    blk, coords, wt, bias, outs = fp32_runs("23x40_l4_o64")
    want = blk.lookup_conv1x1_relu(coords, wt, bias, mode="split", out_dtype=dt)
    got = blk.lookup_conv1x1_relu(coords, wt, bias, mode="presplit", out_dtype=dt)
    assert got.dtype == dt
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert bool(((_bits(got) == _bits(want)) | torch.isnan(want)).all()), "presplit + 16-bit is not split + 16-bit"
    for mode in ("split", "fused"):
        o32 = blk.lookup_conv1x1_relu(coords, wt, None, mode=mode)
        _check_bits(blk.lookup_conv1x1_relu(coords, wt, None, mode=mode, out_dtype=dt), o32, dt, f"no bias / {mode}")
    for bad in (torch.float64, torch.int16, "float16"):
        with pytest.raises(TypeError, match="out_dtype"):
            blk.lookup_conv1x1_relu(coords, wt, bias, out_dtype=bad)


def _rounding_values():
    """fp32 values whose rounding to 16 bits is decided by a tie, an overflow or a subnormal; each has
    at most 13 significant bits, so the split conv's hi + lo halves hold it exactly."""
    v = [0.0, -0.0, 1.0, -1.0]
    # f16: 10 fraction bits -- ties above 1 at odd multiples of 2^-11 (both parities of the kept bit),
    # below 1 at odd multiples of 2^-12
    v += [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 - 2.0 ** -12, 1 - 3 * 2.0 ** -12, 1 + 5 * 2.0 ** -11, 1 + 7 * 2.0 ** -11]
    # bf16: 7 fraction bits -- ties above 1 at odd multiples of 2^-8, below 1 at odd multiples of 2^-9
    v += [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 - 2.0 ** -9, 1 - 3 * 2.0 ** -9, 1 + 5 * 2.0 ** -8, 1 + 7 * 2.0 ** -8]
    # past f16's largest finite value 65504: below, at and above the tie 65520 with +inf
    v += [65504.0, 65512.0, 65520.0, 65528.0, 65536.0, 131072.0, 2.0 ** 127]
    # below f16's smallest normal 2^-14: exact subnormals, ties (2^-25 -> 0, 3 * 2^-25 -> 2^-23), below half the smallest
    v += [2.0 ** -15, 3 * 2.0 ** -16, 1023 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, 5 * 2.0 ** -26,
          3 * 2.0 ** -27, 2.0 ** -40]
    # negative values: the ReLU clips them to +0
    v += [-(1 + 2.0 ** -11), -65520.0, -(2.0 ** -25), -(2.0 ** 127)]
    v += [float("nan")]   # a NaN query
    assert len(v) <= 64
    return np.array(v + [1.0] * (64 - len(v)), dtype=np.float32)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_rounding_ties_overflow_subnormals(ea, dt):
    """ecorr_conv1x1_relu_split_as at the ABI level: C = 1, O = 1, weight 1.0, no bias, so query p's output
    is relu(v_p).  The column scale makes v_p's hi half its upper 11 bits and the lo half the rest, and
    the weight is a power of two: the product is exact.  First the fp32 entry must return the table bit
    for bit (+0 where the ReLU clips), then the 16-bit entry its cast."""
    from eraft_amd import _lib
    B, C, Q, O = 1, 1, 64, 1
    vals = _rounding_values()
    x = torch.from_numpy(vals).view(B, C, Q).to(DEV)
    wt = torch.ones((O, C), dtype=torch.float32, device=DEV)
    st = _lib.stream_of(x)
    pk = _lib.packed_conv1x1_weight(wt, O, C, "split", st, {})
    out32 = torch.full((B, O, Q), 7.0, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().ecorr_conv1x1_relu_split(x.data_ptr(), B, C, Q, None, 0, pk.data_ptr(), None, O,
                                                   out32.data_ptr(), st), "conv split")
    torch.cuda.synchronize()
    want32 = np.where(vals > 0, vals, np.float32(0.0)).astype(np.float32)
    want32[np.isnan(vals)] = np.nan
    got32 = out32.cpu().numpy().reshape(-1)
    fin = ~np.isnan(vals)
    assert np.array_equal(np.isnan(got32), np.isnan(vals))
    assert np.array_equal(got32.view(np.uint32)[fin], want32.view(np.uint32)[fin]), \
        "the fp32 conv does not return the value table bit for bit"
    out16 = torch.zeros((B, O, Q), dtype=torch.int16, device=DEV).fill_(0x7b7b).view(dt)
    _lib.check(_lib.lib().ecorr_conv1x1_relu_split_as(x.data_ptr(), B, C, Q, None, 0, pk.data_ptr(), None, O,
                                                      _lib.OUT_FORMATS[dt], out16.data_ptr(), st), "conv split_as")
    torch.cuda.synchronize()
    got = out16.cpu().view(torch.int16).numpy().reshape(-1).view(np.uint16)
    want = torch.from_numpy(want32).to(dt).view(torch.int16).numpy().view(np.uint16)   # the host's conversion
    for i in range(Q):
        print(f"{vals[i]!r:>16} -> {got[i]:#06x} (host conversion {want[i]:#06x})")
    _check_bits(out16, out32, dt, "rounding table")
    assert np.array_equal(got[fin], want[fin]), "the device result differs from the host's round-to-nearest-even"
    tab = dict(zip(vals.tolist(), got.tolist()))
    if dt == torch.float16:   # spot checks of the contract, independent of torch
        assert tab[65520.0] == 0x7c00 and tab[65512.0] == 0x7bff and tab[-65520.0] == 0x0000
        assert tab[float(np.float32(2.0 ** -24))] == 0x0001 and tab[float(np.float32(2.0 ** -25))] == 0x0000
        assert tab[float(np.float32(3 * 2.0 ** -25))] == 0x0002
        assert tab[float(np.float32(1 + 2.0 ** -11))] == 0x3c00 and tab[float(np.float32(1 + 3 * 2.0 ** -11))] == 0x3c02
    else:
        assert tab[float(np.float32(1 + 2.0 ** -8))] == 0x3f80 and tab[float(np.float32(1 + 3 * 2.0 ** -8))] == 0x3f82
        assert tab[float(np.float32(1 - 2.0 ** -9))] == 0x3f80 and tab[65520.0] == 0x4780
    # the fp32 format through the _as entry: the same launch, the same bits
    again = torch.full_like(out32, 7.0)
    _lib.check(_lib.lib().ecorr_conv1x1_relu_split_as(x.data_ptr(), B, C, Q, None, 0, pk.data_ptr(), None, O,
                                                      _lib.ECORR_OUT_F32, again.data_ptr(), st), "conv split_as f32")
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.uint32)[0, 0][fin], got32.view(np.uint32)[fin])
    for fmt in (-1, 3):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().ecorr_conv1x1_relu_split_as(x.data_ptr(), B, C, Q, None, 0, pk.data_ptr(), None, O,
                                                              fmt, out16.data_ptr(), st), "conv split_as")
