"""16-bit feature maps into the split build (ecorr_build_split_pack_as, CorrBlock(..., fmap_dtype=...)).

Contract (include/ecorr.h): the operand pass converts each 16-bit element to fp32 on load, which is
exact, and runs the fp32 pass on it.  So for both dtypes the WHOLE workspace (exponents and hi/lo
panels) after ecorr_build_split_pack_as(x16) must equal, byte for byte, the workspace after
ecorr_build_split_pack(x16.float()); both are prefilled with one byte pattern, so bytes no kernel
writes compare too.  The pyramids of the gemm that follows are then equal as int32 patterns off the NaNs
with identical NaN positions.  No tolerance anywhere.

Geometries (B, D, H x W, levels), the smallest that reach each path of pack_body:
  L16 layout, ragged both ways   2, 256, 23 x 40, 4   (23 = 16 + 7: a padded regular tile row; 40 = 2.5 n-tiles)
  chunk panels, k >= D zeros     1,  40, 16 x 20, 4
  dc = 17: the re-read path      1, 272,  8 x  8, 1
  the smallest D                 1,   1,  8 x  8, 1
  fmap1 as a query slab          2, 256, 23 x 40, 4, q_count = 3 * 40 (rows 5 .. 7 as [B][D][q_count])
  4 x 32 band tiles              1, 256, 12 x 40, 2 and 1, 24, 12 x 40, 2   (12 = 8 + 4; both panel layouts)
Values: PRNG normals rounded to the dtype, with planted pixels: +-0 beside ordinary values, a pixel of
+-(the smallest subnormal) only, the largest finite value, an all-zero pixel, one +inf and one NaN pixel."""
import ctypes

import numpy as np
import pytest
import torch

import prng

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
FILL = 0xA5

# name: (B, D, H, W, levels, q_begin, q_count)
GEOMS = {
    "l16_23x40": (2, 256, 23, 40, 4, 0, 23 * 40),
    "chunks_d40_16x20": (1, 40, 16, 20, 4, 0, 16 * 20),
    "reread_d272_8x8": (1, 272, 8, 8, 1, 0, 64),
    "d1_8x8": (1, 1, 8, 8, 1, 0, 64),
    "slab_l16_23x40": (2, 256, 23, 40, 4, 5 * 40, 3 * 40),
    "band_l16_12x40": (1, 256, 12, 40, 2, 0, 12 * 40),
    "band_chunks_d24_12x40": (1, 24, 12, 40, 2, 0, 12 * 40),
}


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _plant(x, dt, first):
    """x: float32 array [B][D][N], already rounded to dt.  Plants the special pixels from pixel `first`."""
    fi = torch.finfo(dt)
    B, D, N = x.shape
    tiny = float(fi.smallest_normal) * float(fi.eps)   # the smallest subnormal
    p = first
    x[:, 0, p] = 0.0                      # +-0 beside ordinary values
    x[:, D - 1, p] = -0.0
    x[:, :, p + 1] = tiny * np.where(np.arange(D) % 2 == 0, 1.0, -1.0)[None, :]   # a subnormal-only pixel
    x[:, 0, p + 2] = float(fi.max)        # the largest finite value
    if D > 1:
        x[:, D // 2, p + 2] = -float(fi.max)
    x[:, :, p + 3] = 0.0                  # an all-zero pixel
    x[0, 0, p + 4] = float("inf")         # one pixel with +inf, one with NaN (batch item 0 only)
    x[0, D - 1, p + 5] = float("nan")
    return x


def _fmaps(name, dt):
    """(fmap1 slab [B][D][q], fmap2 [B][D][H*W]) as dt tensors on the device."""
    B, D, H, W, L, q_begin, q = GEOMS[name]
    seed = 900 + 10 * sorted(GEOMS).index(name)
    a = torch.from_numpy(prng.normal(seed, (B, D, H * W))).to(dt).float().numpy()
    b = torch.from_numpy(prng.normal(seed + 1, (B, D, H * W))).to(dt).float().numpy()
    a = np.ascontiguousarray(a[:, :, q_begin:q_begin + q])
    _plant(a, dt, 3)          # query pixels 3 .. 8 of the slab
    _plant(b, dt, H * W - 7)  # target pixels in the last row (a ragged tile)
    f1 = torch.from_numpy(a).to(dt).to(DEV)
    f2 = torch.from_numpy(b).to(dt).to(DEV)
    # the planted values survived the conversion
    fi = torch.finfo(dt)
    assert float(f1[0, 0, 5].float()) == float(fi.max) and bool(torch.isinf(f1[0, 0, 7])) and bool(torch.isnan(f1[0, D - 1, 8]))
    assert float(f1[0, 0, 4].float()) == float(fi.smallest_normal) * float(fi.eps) > 0
    assert f1.view(torch.int16)[0, D - 1, 3].item() == -32768 or D == 1   # -0 kept (D = 1: the same cell as +0)
    return f1, f2


def _ws_bytes(_lib, B, D, H, W, q):
    n = ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_build_split_workspace_size(B, D, H, W, q, ctypes.byref(n)), "ws size")
    return n.value


def _pack(_lib, f1_ptr, f2_ptr, fmt, geom, anchor):
    """The prefilled workspace after the operand pass: fmt None = ecorr_build_split_pack."""
    B, D, H, W, L, q_begin, q = geom
    ws = torch.full((_ws_bytes(_lib, B, D, H, W, q),), FILL, dtype=torch.uint8, device=DEV)
    st = _lib.stream_of(anchor)
    if fmt is None:
        _lib.check(_lib.lib().ecorr_build_split_pack(f1_ptr, f2_ptr, B, D, H, W, q, ws.data_ptr(), st), "pack")
    else:
        _lib.check(_lib.lib().ecorr_build_split_pack_as(f1_ptr, f2_ptr, fmt, B, D, H, W, q, ws.data_ptr(), st), "pack_as")
    torch.cuda.synchronize()
    return ws


def _gemm(_lib, ws, geom):
    B, D, H, W, L, q_begin, q = geom
    _, _, off = _lib.layout(B * q, H, W, L)
    pyr = torch.full((off[-1],), 0, dtype=torch.int32, device=DEV).fill_(0x5a5a5a5a).view(torch.float32)
    _lib.check(_lib.lib().ecorr_build_split_gemm(B, D, H, W, q, L, pyr.data_ptr(), ws.data_ptr(), _lib.stream_of(pyr)),
               "gemm")
    torch.cuda.synchronize()
    return pyr


def _same_off_nans(a, b, what):
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: NaN positions differ"
    same = (a.view(torch.int32) == b.view(torch.int32)) | na
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ"


@pytest.fixture(scope="module")
def fp32_packs(ea):
    """(geometry, dtype) -> (f1, f2, workspace and pyramid of the fp32 entry on their .float()): once, never written."""
    from eraft_amd import _lib
    cache = {}

    def get(name, dt):
        if (name, dt) not in cache:
            f1, f2 = _fmaps(name, dt)
            g1, g2 = f1.float(), f2.float()
            ws = _pack(_lib, g1.data_ptr(), g2.data_ptr(), None, GEOMS[name], g1)
            cache[(name, dt)] = (f1, f2, ws, _gemm(_lib, ws, GEOMS[name]))
        return cache[(name, dt)]
    return get


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_pack_as_workspace_and_pyramid_bitwise(ea, fp32_packs, name, dt):
    from eraft_amd import _lib
    f1, f2, ws32, pyr32 = fp32_packs(name, dt)
    assert bool((ws32 != FILL).any())
    ws16 = _pack(_lib, f1.data_ptr(), f2.data_ptr(), _lib.ELEM_FORMATS[dt], GEOMS[name], f1)
    diff = int((ws16 != ws32).sum())
    assert diff == 0, f"{name}: {diff} of {ws32.numel()} workspace bytes differ"
    pyr16 = _gemm(_lib, ws16, GEOMS[name])
    assert bool(torch.isnan(pyr32).any()) and bool(torch.isfinite(pyr32).any())   # the inf / NaN pixels reached it
    _same_off_nans(pyr16, pyr32, name)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["l16_23x40", "chunks_d40_16x20", "slab_l16_23x40"])
def test_pointers_two_byte_aligned_only(ea, fp32_packs, name, dt):
    """Both fmaps one element into their allocations: 2-byte aligned, not 4."""
    from eraft_amd import _lib
    f1, f2, ws32, _ = fp32_packs(name, dt)
    b1 = torch.zeros(f1.numel() + 1, dtype=dt, device=DEV)
    b2 = torch.zeros(f2.numel() + 1, dtype=dt, device=DEV)
    b1[1:].copy_(f1.reshape(-1))
    b2[1:].copy_(f2.reshape(-1))
    p1, p2 = b1.data_ptr() + 2, b2.data_ptr() + 2
    assert p1 % 4 == 2 and p2 % 4 == 2
    ws16 = _pack(_lib, p1, p2, _lib.ELEM_FORMATS[dt], GEOMS[name], b1)
    assert torch.equal(ws16, ws32), name


def test_f32_format_is_the_existing_entry(ea, fp32_packs):
    from eraft_amd import _lib
    for name in ("l16_23x40", "chunks_d40_16x20", "reread_d272_8x8"):
        f1, f2, ws32, _ = fp32_packs(name, torch.bfloat16)
        g1, g2 = f1.float(), f2.float()
        ws = _pack(_lib, g1.data_ptr(), g2.data_ptr(), _lib.ECORR_ELEM_F32, GEOMS[name], g1)
        assert torch.equal(ws, ws32), name
    B, D, H, W, L, _, q = GEOMS["d1_8x8"]
    f1, f2, _, _ = fp32_packs("d1_8x8", torch.float16)
    ws = torch.empty(_ws_bytes(_lib, B, D, H, W, q), dtype=torch.uint8, device=DEV)
    for fmt in (-1, 3):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().ecorr_build_split_pack_as(f1.data_ptr(), f2.data_ptr(), fmt, B, D, H, W, q,
                                                            ws.data_ptr(), _lib.stream_of(ws)), "pack_as")


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["l16_23x40", "chunks_d40_16x20", "reread_d272_8x8", "d1_8x8"])
def test_corrblock_fmap_dtype_equals_float_block(ea, fp32_packs, name, dt):
    """Through the class: the reference-layout levels of CorrBlock(x16, fmap_dtype=dt) and of
    CorrBlock(x16.float()), and ecorr_build_split_as beside them."""
    from eraft_amd import _lib
    B, D, H, W, L, _, q = GEOMS[name]
    f1, f2, ws32, pyr32 = fp32_packs(name, dt)
    f1, f2 = f1.view(B, D, H, W), f2.view(B, D, H, W)
    blk16 = ea.CorrBlock(f1, f2, num_levels=L, radius=4, fmap_dtype=dt)
    blk32 = ea.CorrBlock(f1.float(), f2.float(), num_levels=L, radius=4)
    for i, (a, b) in enumerate(zip(blk16.corr_pyramid, blk32.corr_pyramid)):
        assert a.dtype == torch.float32 and a.shape == b.shape
        _same_off_nans(a, b, f"{name} level {i}")
    # one call: pack_as then gemm
    ws = torch.full_like(ws32, FILL)
    pyr = torch.full_like(pyr32.view(torch.int32), 0x5a5a5a5a).view(torch.float32)
    _lib.check(_lib.lib().ecorr_build_split_as(f1.data_ptr(), f2.data_ptr(), _lib.ELEM_FORMATS[dt], B, D, H, W, q, L,
                                               pyr.data_ptr(), ws.data_ptr(), _lib.stream_of(pyr)), "build_split_as")
    torch.cuda.synchronize()
    assert torch.equal(ws, ws32)
    _same_off_nans(pyr, pyr32, f"{name} ecorr_build_split_as")


def test_dtype_checks(ea):
    B, D, H, W = 1, 8, 16, 20
    h1 = torch.from_numpy(prng.normal(981, (B, D, H, W))).to(DEV).half()
    h2 = torch.from_numpy(prng.normal(982, (B, D, H, W))).to(DEV).half()
    with pytest.raises(TypeError, match=r"fmap1 must be float32 \(got torch.float16\)"):
        ea.CorrBlock(h1, h2)                                  # without the keyword: the pinned refusal
    with pytest.raises(TypeError, match=r"fmap1 must be float32 \(got torch.float16\)"):
        ea.CorrBlock(h1, h2, fmap_dtype=torch.float32)
    with pytest.raises(TypeError, match=r"fmap2 must be float16 \(got torch.bfloat16\)"):
        ea.CorrBlock(h1, h2.bfloat16(), fmap_dtype=torch.float16)     # mixed dtypes
    with pytest.raises(TypeError, match=r"fmap1 must be float16 \(got torch.float32\)"):
        ea.CorrBlock(h1.float(), h2, fmap_dtype=torch.float16)
    with pytest.raises(TypeError, match=r"fmap1 must be bfloat16 \(got torch.float16\)"):
        ea.CorrBlock(h1, h2, fmap_dtype=torch.bfloat16)
    for bad in (torch.float64, torch.int16, "float16"):
        with pytest.raises(TypeError, match="fmap_dtype"):
            ea.CorrBlock(h1, h2, fmap_dtype=bad)
    blk = ea.CorrBlock(h1, h2, fmap_dtype=torch.float16)
    assert blk._column_scale(None) is None   # presplit needs fp32 fmaps: its documented split fallback


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_fp32_build_mode_converts(ea, dt):
    """ECORR_BUILD_MODE=fp32 has no 16-bit input: the block converts with .float() and builds as before."""
    from eraft_amd import _lib
    B, D, H, W = 2, 24, 16, 20
    f1 = torch.from_numpy(prng.normal(991, (B, D, H, W))).to(DEV).to(dt)
    f2 = torch.from_numpy(prng.normal(992, (B, D, H, W))).to(DEV).to(dt)
    before = _lib.build_mode()
    _lib.set_build_mode("fp32")
    try:
        a = ea.CorrBlock(f1, f2, fmap_dtype=dt).corr_pyramid
        b = ea.CorrBlock(f1.float(), f2.float()).corr_pyramid
    finally:
        _lib.set_build_mode(before)
    assert _lib.build_mode() == before
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
