"""The 16-bit lookup output (ecorr_lookup_as, CorrBlock.__call__(coords, out_dtype=...)) on the GPU.

Contract (include/ecorr.h): each element is the fp32 sample ecorr_lookup computes, rounded once to
nearest-even.  So for both dtypes the 16-bit output, read as int16 bit patterns, must equal
ecorr_lookup's fp32 output converted by torch.Tensor.to(dtype) on the same device wherever the fp32
value is not NaN, and be NaN exactly where the fp32 value is.  No tolerance anywhere.

Cases are the smallest shapes that reach each kernel path (D = 8, B = 2):
  lookup_cols_reg<4, PAIR>   18 x 16: level widths 16 / 8 / 4 / 2 all even, Q = 288 = 4.5 query blocks;
  lookup_cols_reg<4, !PAIR>  17 x 21: Q = 357 odd, so channel rows start on 2-byte boundaries only;
  a query-row slab           17 x 20, q_count = 5 rows from row 3 (inside an interleave group);
  lookup_cols_reg<1>         both staging forms;  lookup_staged<0 | 2 | 3>;  lookup_direct (radius 5);
  1 and 5 levels at 64 x 64  (level 4 = 4 x 4: the formats of levels >= 4).
lookup_staged<1 | 4> run only when a batch item's output passes 2^31 bytes, which no pyramid that
fits a device reaches (Q queries need Q * H * W floats of level 0); they share lookup_staged<R>'s code.

Each case runs four coordinate sets -- smooth (prng.coords_with_flow), grad_ref.special_coords (NaN,
+-inf, huge: whole and half blocks on the direct-gather mode), grad_ref.edge_coords (windows over all
four borders) and i.i.d. large flows -- so all three modes of the radius-4 kernel occur: window
(md 0), direct gather (md 1: the special queries) and past the range (md 2: the lanes of the tail
block).  From the fp32 output, which no new code produced, each case asserts that NaN, exact zero
(taps outside the image) and non-zero finite values are all present.  That fp32 reference is itself
checked against the oracle, bit for bit: at radius 4 by tests/test_corr_gpu.py, at radii 0, 1, 2, 3
and 5 (these shapes among others) by tests/test_lookup_radius_gpu.py.
"""
import numpy as np
import pytest
import torch

import grad_ref as gr
import prng

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]

# (B, D, H, W, levels, radius, q_begin, q_count)
CASES = {
    "pair_tail_18x16": (2, 8, 18, 16, 4, 4, 0, 288),
    "odd_q_17x21": (2, 8, 17, 21, 4, 4, 0, 357),
    "slab_17x20_5rows": (2, 8, 17, 20, 4, 4, 60, 100),
    "r1_pair_18x16": (2, 8, 18, 16, 4, 1, 0, 288),
    "r1_17x21": (2, 8, 17, 21, 4, 1, 0, 357),
    "r0_17x21": (2, 8, 17, 21, 4, 0, 0, 357),
    "r2_17x21": (2, 8, 17, 21, 4, 2, 0, 357),
    "r3_17x21": (2, 8, 17, 21, 4, 3, 0, 357),
    "r5_direct_17x21": (2, 8, 17, 21, 4, 5, 0, 357),
    "levels1_64x64": (2, 8, 64, 64, 1, 4, 0, 4096),
    "levels5_64x64": (2, 8, 64, 64, 5, 4, 0, 4096),
}


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


def _coord_sets(B, H, W, q_begin, q):
    sets = {"smooth": prng.coords_with_flow(811, B, H, W, 2.0), "special": gr.special_coords(812, B, H, W),
            "edge": gr.edge_coords(B, H, W), "iid_large": prng.coords_with_flow(813, B, H, W, 40.0)}
    return {k: torch.from_numpy(np.ascontiguousarray(v.reshape(B, 2, H * W)[:, :, q_begin:q_begin + q])).to(DEV)
            for k, v in sets.items()}


@pytest.fixture(scope="module")
def fp32_runs(ea):
    """case -> (pyramid, {set: (coords, fp32 output)}): built once, shared by both dtypes, never written."""
    from eraft_amd import _lib
    cache = {}

    def get(name):
        if name not in cache:
            B, D, H, W, L, r, q_begin, q = CASES[name]
            f1 = prng.normal(801, (B, D, H, W)).reshape(B, D, H * W)[:, :, q_begin:q_begin + q]
            d1 = torch.from_numpy(np.ascontiguousarray(f1)).to(DEV)
            d2 = torch.from_numpy(prng.normal(802, (B, D, H, W))).to(DEV)
            _, _, off = _lib.layout(B * q, H, W, L)
            pyr = _lib.build_pyramid(d1, d2, B, D, H, W, q, L, off, "test build")
            C = L * (2 * r + 1) ** 2
            runs = {}
            for sname, c in _coord_sets(B, H, W, q_begin, q).items():
                out = torch.full((B, C, q), float("nan"), dtype=torch.float32, device=DEV)
                _lib.check(_lib.lib().ecorr_lookup(pyr.data_ptr(), c.data_ptr(), B, H, W, q, L, r, out.data_ptr(),
                                                   _lib.stream_of(out)), "lookup")
                runs[sname] = (c, out)
            torch.cuda.synchronize()
            cache[name] = (pyr, runs)
        return cache[name]
    return get


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_half_output_is_the_rounded_fp32_output(ea, fp32_runs, name, dt):
    from eraft_amd import _lib
    B, D, H, W, L, r, q_begin, q = CASES[name]
    pyr, runs = fp32_runs(name)
    C = L * (2 * r + 1) ** 2
    # every class of value occurs in this case's fp32 outputs
    allv = torch.cat([o.reshape(-1) for _, o in runs.values()])
    assert bool(torch.isnan(allv).any()), "no NaN sample"
    assert bool((allv == 0).any()), "no zero (out-of-image) sample"
    assert bool((torch.isfinite(allv) & (allv != 0)).any()), "no non-zero finite sample"
    assert bool(torch.isnan(runs["special"][1]).any()) and not bool(torch.isnan(runs["smooth"][1]).any())
    for sname, (c, out32) in runs.items():
        # 0x7b7b: a finite pattern in both formats, so an element the kernel skipped would show
        out16 = torch.full((B, C, q), 0, dtype=torch.int16, device=DEV).fill_(0x7b7b).view(dt)
        _lib.check(_lib.lib().ecorr_lookup_as(pyr.data_ptr(), c.data_ptr(), B, H, W, q, L, r, _lib.OUT_FORMATS[dt],
                                              out16.data_ptr(), _lib.stream_of(out16)), "lookup_as")
        torch.cuda.synchronize()
        _check_bits(out16, out32, dt, f"{name} / {sname}")


def _rounding_values():
    """fp32 values whose rounding to 16 bits is decided by a tie, an overflow or a subnormal."""
    v = [0.0, -0.0, 1.0, -1.0]
    for s in (1.0, -1.0):
        # f16: 10 fraction bits -- ties above 1 at odd multiples of 2^-11, below 1 at odd multiples of 2^-12
        v += [s * (1 + 2.0 ** -11), s * (1 - 2.0 ** -11), s * (1 + 3 * 2.0 ** -11), s * (1 - 3 * 2.0 ** -11),
              s * (1 - 2.0 ** -12), s * (1 - 3 * 2.0 ** -12)]
        # bf16: 7 fraction bits -- ties above 1 at odd multiples of 2^-8, below 1 at odd multiples of 2^-9
        v += [s * (1 + 2.0 ** -8), s * (1 - 2.0 ** -8), s * (1 + 3 * 2.0 ** -8), s * (1 - 3 * 2.0 ** -8),
              s * (1 - 2.0 ** -9), s * (1 - 3 * 2.0 ** -9)]
        # past f16's largest finite value 65504: below, at and above the tie 65520 with +-inf
        v += [s * 65504.0, s * 65512.0, s * 65520.0, s * 65536.0, s * 131072.0, s * 3.0e38]
        # below f16's smallest normal 2^-14: exact subnormals, ties (2^-25 -> 0, 3 * 2^-25 -> 2^-23), underflow
        v += [s * 2.0 ** -15, s * 3 * 2.0 ** -16, s * 1023 * 2.0 ** -24, s * 2.0 ** -24, s * 2.0 ** -25,
              s * 3 * 2.0 ** -25, s * 2.0 ** -26, s * 5 * 2.0 ** -26]
    assert len(v) <= 64
    return np.array(v + [1.0] * (64 - len(v)), dtype=np.float32)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_rounding_ties_overflow_subnormals_zeros(ea, dt):
    """Radius 0, one level, integer coordinates: the output is the pyramid pixel itself.  Query p's
    whole 8 x 8 level-0 image holds the value v_p, written into the pyramid's storage directly: a GEMM
    cannot deliver -0 (its accumulator starts at +0), and a constant image keeps it through the blend
    (-0 * 1 + -0 * 0 + ... = -0).  The test first asserts that the fp32 lookup returns exactly these
    bit patterns, then compares the 16-bit outputs with torch's conversion of them."""
    from eraft_amd import _lib
    from eraft_amd.layout import formats, tile
    B, H, W, L, r = 1, 8, 8, 1, 0
    Q = H * W
    vals = _rounding_values()
    level0 = torch.from_numpy(vals).view(Q, 1, 1).expand(Q, H, W).contiguous()
    pyr = tile(level0, ntx=formats(H, W, L)[0]).to(DEV)
    _, _, off = _lib.layout(B * Q, H, W, L)
    assert pyr.numel() == off[-1] and pyr.dtype == torch.float32
    coords = torch.from_numpy(prng.coords_with_flow(0, B, H, W, 0.0)).to(DEV)
    out32 = torch.full((B, 1, Q), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().ecorr_lookup(pyr.data_ptr(), coords.data_ptr(), B, H, W, Q, L, r, out32.data_ptr(),
                                       _lib.stream_of(out32)), "lookup")
    torch.cuda.synchronize()
    assert np.array_equal(out32.cpu().numpy().reshape(-1).view(np.uint32), vals.view(np.uint32)), \
        "the fp32 lookup does not return the value table bit for bit"
    out16 = torch.zeros((B, 1, Q), dtype=torch.int16, device=DEV).fill_(0x7b7b).view(dt)
    _lib.check(_lib.lib().ecorr_lookup_as(pyr.data_ptr(), coords.data_ptr(), B, H, W, Q, L, r, _lib.OUT_FORMATS[dt],
                                          out16.data_ptr(), _lib.stream_of(out16)), "lookup_as")
    torch.cuda.synchronize()
    got = out16.cpu().view(torch.int16).numpy().reshape(-1).view(np.uint16)
    want = torch.from_numpy(vals).to(dt).view(torch.int16).numpy().view(np.uint16)   # the host's conversion
    for i in range(Q):
        print(f"{vals[i]!r:>16} -> {got[i]:#06x} (host conversion {want[i]:#06x})")
    _check_bits(out16, out32, dt, "rounding table")
    assert np.array_equal(got, want), "the device result differs from the host's round-to-nearest-even"
    if dt == torch.float16:   # spot checks of the contract, independent of torch
        tab = dict(zip(vals.tolist(), got.tolist()))
        assert tab[65520.0] == 0x7c00 and tab[-65520.0] == 0xfc00 and tab[65512.0] == 0x7bff   # overflow -> +-inf
        assert tab[float(np.float32(2.0 ** -24))] == 0x0001 and tab[float(np.float32(2.0 ** -25))] == 0x0000
        assert tab[float(np.float32(3 * 2.0 ** -25))] == 0x0002                                # subnormal tie -> even
        assert got[1] == 0x8000 and got[0] == 0x0000                                           # -0, +0
        assert tab[float(np.float32(1 + 2.0 ** -11))] == 0x3c00 and tab[float(np.float32(1 + 3 * 2.0 ** -11))] == 0x3c02
    else:
        tab = dict(zip(vals.tolist(), got.tolist()))
        assert tab[float(np.float32(1 + 2.0 ** -8))] == 0x3f80 and tab[float(np.float32(1 + 3 * 2.0 ** -8))] == 0x3f82
        assert tab[float(np.float32(1 - 2.0 ** -9))] == 0x3f80 and got[1] == 0x8000


def test_f32_format_is_ecorr_lookup(ea, fp32_runs):
    """ECORR_OUT_F32 through ecorr_lookup_as: the same launch, the same bits."""
    from eraft_amd import _lib
    for name in ("pair_tail_18x16", "r2_17x21", "r5_direct_17x21"):
        B, D, H, W, L, r, q_begin, q = CASES[name]
        pyr, runs = fp32_runs(name)
        for sname, (c, out32) in runs.items():
            out = torch.full_like(out32, 7.0)
            _lib.check(_lib.lib().ecorr_lookup_as(pyr.data_ptr(), c.data_ptr(), B, H, W, q, L, r, _lib.ECORR_OUT_F32,
                                                  out.data_ptr(), _lib.stream_of(out)), "lookup_as")
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), out32.view(torch.int32)), f"{name} / {sname}"


def test_bad_format_and_dtype(ea):
    from eraft_amd import _lib
    B, D, H, W = 1, 8, 18, 16
    f1 = torch.from_numpy(prng.normal(821, (B, D, H, W))).to(DEV)
    f2 = torch.from_numpy(prng.normal(822, (B, D, H, W))).to(DEV)
    blk = ea.CorrBlock(f1, f2)
    coords = torch.from_numpy(prng.coords_with_flow(823, B, H, W, 2.0)).to(DEV)
    out = torch.empty((B, 324, H, W), dtype=torch.float32, device=DEV)
    for fmt in (-1, 3):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().ecorr_lookup_as(blk._pyramid.data_ptr(), coords.data_ptr(), B, H, W, H * W, 4, 4, fmt,
                                                  out.data_ptr(), _lib.stream_of(out)), "lookup_as")
    for bad in (torch.float64, torch.int16, "float16"):
        with pytest.raises(TypeError, match="out_dtype"):
            blk(coords, out_dtype=bad)
    # the accepted values, through the class: None and float32 are the fp32 call, the others its rounding
    ref = blk(coords)
    assert ref.dtype == torch.float32 and torch.equal(blk(coords, out_dtype=torch.float32), ref)
    assert torch.equal(blk(coords, out_dtype=None), ref)
    for dt in DTYPES:
        got = blk(coords, out_dtype=dt)
        assert got.dtype == dt and got.shape == ref.shape
        _check_bits(got, ref, dt, f"CorrBlock {dt}")
