"""The hi-only split build (ecorr_build_split_pack_hi_as / _gemm_hi / _hi_as, ECORR_BUILD_HI).

Contract (include/ecorr.h): the pyramid is bitwise that of ecorr_build_split_as on the same inputs,
whichever of the two K loops ran; the workspace from byte 256 on is bitwise ecorr_build_split_pack_as's;
int32 word 0 is 1 exactly when a lo half of a panel has a magnitude bit -- for 16-bit fmaps: when an
element is not finite (tests/test_hi_split_ref.py).  No tolerance anywhere: every workspace is prefilled
with 0xA5 bytes and every pyramid with 0x5a5a5a5a words, whole buffers are compared (padding included),
equality is int32 equality off the NaNs with identical NaN positions.

Geometries (B, D, H x W, levels):
  l16_23x40       2, 256, 23 x 40, 4   ragged both ways, several query tiles
  slab_l16_23x40  the same with fmap1 as the slab of rows 5 .. 7
  full_16x16      1, 256, 16 x 16, 4   one FULL 256-query tile, level 3 is 2 x 2
  band_12x40      1, 256, 12 x 40, 2   4 x 32 band tiles
  div_d250_16x24  1, 250, 16 x 24, 4   the MUL = false kernels (sqrt(250) is no power of two)
  d40_16x20       1,  40, 16 x 20, 4   not routed to the split16 kernels: the entries must still work
Values: PRNG normals rounded to the dtype, with planted pixels: +-0 beside ordinary values, a pixel of
+-(the smallest subnormal) only, +-the largest finite value, an all-zero pixel and, for bfloat16, a pixel
that spans 2^60 inside itself.  (bfloat16: the product of the two largest-value pixels overflows to +inf
in level 0, as it does in the plain build; nothing is NaN.)"""
import ctypes

import numpy as np
import pytest
import torch

import prng

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
FILL = 0xA5
FLAG_BYTES = 256

# name: (B, D, H, W, levels, q_begin, q_count)
GEOMS = {
    "l16_23x40": (2, 256, 23, 40, 4, 0, 23 * 40),
    "slab_l16_23x40": (2, 256, 23, 40, 4, 5 * 40, 3 * 40),
    "full_16x16": (1, 256, 16, 16, 4, 0, 256),
    "band_12x40": (1, 256, 12, 40, 2, 0, 12 * 40),
    "div_d250_16x24": (1, 250, 16, 24, 4, 0, 16 * 24),
    "d40_16x20": (1, 40, 16, 20, 4, 0, 16 * 20),
}
ROUTED = [n for n in sorted(GEOMS) if (GEOMS[n][1] + 15) // 16 == 16]   # D = 241 .. 256: the split16 kernels


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _plant(x, dt, first):
    """x: float32 array [B][D][N], already rounded to dt.  Plants the special (finite) pixels from pixel `first`."""
    fi = torch.finfo(dt)
    B, D, N = x.shape
    tiny = float(fi.smallest_normal) * float(fi.eps)   # the smallest subnormal
    p = first
    x[:, 0, p] = 0.0                      # +-0 beside ordinary values
    x[:, D - 1, p] = -0.0
    x[:, :, p + 1] = tiny * np.where(np.arange(D) % 2 == 0, 1.0, -1.0)[None, :]   # a subnormal-only pixel
    x[:, 0, p + 2] = float(fi.max)        # +-the largest finite value
    x[:, D // 2, p + 2] = -float(fi.max)
    x[:, :, p + 3] = 0.0                  # an all-zero pixel
    if dt == torch.bfloat16:              # a pixel that spans 2^60 inside itself
        x[:, :, p + 4] = np.ldexp(1.0, -(np.arange(D) % 61)).astype(np.float32)[None, :] * 2.0 ** 30
        x[:, 1, p + 4] *= -1.0
    return x


def _fmaps(name, dt, nonfinite=False):
    """(fmap1 slab [B][D][q], fmap2 [B][D][H*W]) as dt tensors on the device; nonfinite: one +inf pixel in
    fmap1 and one NaN pixel in fmap2 (batch item 0) beside the finite planted ones."""
    B, D, H, W, L, q_begin, q = GEOMS[name]
    seed = 1500 + 10 * sorted(GEOMS).index(name)
    a = torch.from_numpy(prng.normal(seed, (B, D, H * W))).to(dt).float().numpy()
    b = torch.from_numpy(prng.normal(seed + 1, (B, D, H * W))).to(dt).float().numpy()
    # the two channels that carry +-the largest finite value in the planted pixels: 2^-6 of the normals (exact),
    # so that value times the other map's entries stays finite in bfloat16 too and no inf - inf = NaN is pooled
    for m in (a, b):
        m[:, [0, D // 2], :] *= 2.0 ** -6
    a = np.ascontiguousarray(a[:, :, q_begin:q_begin + q])
    _plant(a, dt, 3)          # query pixels 3 .. 7 of the slab
    _plant(b, dt, H * W - 7)  # target pixels in the last row (a ragged tile)
    if nonfinite:
        a[0, 0, 9] = float("inf")
        b[0, D - 1, H * W - 9] = float("nan")
    f1 = torch.from_numpy(a).to(dt).to(DEV)
    f2 = torch.from_numpy(b).to(dt).to(DEV)
    fi = torch.finfo(dt)
    assert float(f1[0, 0, 5].float()) == float(fi.max) and float(f1[0, D // 2, 5].float()) == -float(fi.max)
    assert float(f1[0, 0, 4].float()) == float(fi.smallest_normal) * float(fi.eps) > 0
    assert f1.view(torch.int16)[0, D - 1, 3].item() == -32768   # -0 kept
    assert bool(torch.isfinite(f1.float()).all()) != nonfinite and bool(torch.isfinite(f2.float()).all()) != nonfinite
    return f1, f2


def _size(_lib, entry, geom):
    B, D, H, W, L, q_begin, q = geom
    n = ctypes.c_int64()
    _lib.check(getattr(_lib.lib(), entry)(B, D, H, W, q, ctypes.byref(n)), entry)
    return n.value


def _new_pyr(_lib, geom):
    B, D, H, W, L, q_begin, q = geom
    _, _, off = _lib.layout(B * q, H, W, L)
    return torch.full((off[-1],), 0x5a5a5a5a, dtype=torch.int32, device=DEV).view(torch.float32)


def _plain(_lib, f1, f2, geom):
    """(workspace, pyramid) of ecorr_build_split_pack_as + ecorr_build_split_gemm: the reference."""
    B, D, H, W, L, q_begin, q = geom
    ws = torch.full((_size(_lib, "ecorr_build_split_workspace_size", geom),), FILL, dtype=torch.uint8, device=DEV)
    pyr = _new_pyr(_lib, geom)
    st = _lib.stream_of(ws)
    _lib.check(_lib.lib().ecorr_build_split_pack_as(f1.data_ptr(), f2.data_ptr(), _lib.ELEM_FORMATS[f1.dtype], B, D, H, W,
                                                    q, ws.data_ptr(), st), "pack_as")
    _lib.check(_lib.lib().ecorr_build_split_gemm(B, D, H, W, q, L, pyr.data_ptr(), ws.data_ptr(), st), "gemm")
    torch.cuda.synchronize()
    return ws, pyr


def _pack_hi(_lib, f1, f2, geom):
    B, D, H, W, L, q_begin, q = geom
    n = _size(_lib, "ecorr_build_split_hi_workspace_size", geom)
    assert n == _size(_lib, "ecorr_build_split_workspace_size", geom) + FLAG_BYTES
    ws = torch.full((n,), FILL, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().ecorr_build_split_pack_hi_as(f1.data_ptr(), f2.data_ptr(), _lib.ELEM_FORMATS[f1.dtype], B, D, H,
                                                       W, q, ws.data_ptr(), _lib.stream_of(ws)), "pack_hi_as")
    torch.cuda.synchronize()
    return ws


def _gemm_hi(_lib, ws, geom):
    B, D, H, W, L, q_begin, q = geom
    pyr = _new_pyr(_lib, geom)
    _lib.check(_lib.lib().ecorr_build_split_gemm_hi(B, D, H, W, q, L, pyr.data_ptr(), ws.data_ptr(), _lib.stream_of(pyr)),
               "gemm_hi")
    torch.cuda.synchronize()
    return pyr


def _flag(ws):
    return int(ws[:4].view(torch.int32).item())


def _set_flag(ws, v):
    ws[:4].view(torch.int32).fill_(v)


def _check_hi_ws(ws_hi, ws_plain, flag, what):
    assert _flag(ws_hi) == flag, f"{what}: flag word {_flag(ws_hi)}"
    assert bool((ws_hi[4:FLAG_BYTES] == FILL).all()), f"{what}: the reserved bytes of the flag block were written"
    diff = int((ws_hi[FLAG_BYTES:] != ws_plain).sum())
    assert diff == 0, f"{what}: {diff} of {ws_plain.numel()} workspace bytes differ"
    assert bool((ws_plain != FILL).any())


def _same_off_nans(a, b, what):
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: NaN positions differ"
    same = (a.view(torch.int32) == b.view(torch.int32)) | na
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ"


@pytest.fixture(scope="module")
def plain(ea):
    """(geometry, dtype, nonfinite) -> (f1, f2, workspace, pyramid) of the plain entries: once, never written."""
    from eraft_amd import _lib
    cache = {}

    def get(name, dt, nonfinite=False):
        key = (name, dt, nonfinite)
        if key not in cache:
            f1, f2 = _fmaps(name, dt, nonfinite)
            cache[key] = (f1, f2) + _plain(_lib, f1, f2, GEOMS[name])
        return cache[key]
    return get


# ---- 1. finite 16-bit fmaps: flag 0, the workspace and the pyramid of the plain entries, no NaN
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_finite_16bit_fmaps_flag_clear_and_bitwise(ea, plain, name, dt):
    from eraft_amd import _lib
    f1, f2, ws0, pyr0 = plain(name, dt)
    ws = _pack_hi(_lib, f1, f2, GEOMS[name])
    _check_hi_ws(ws, ws0, 0, name)
    pyr = _gemm_hi(_lib, ws, GEOMS[name])
    assert not bool(torch.isnan(pyr0).any()) and not bool(torch.isnan(pyr).any())
    assert bool((pyr0.view(torch.int32) != 0x5a5a5a5a).any())
    assert torch.equal(pyr.view(torch.int32), pyr0.view(torch.int32)), \
        f"{name}: {int((pyr.view(torch.int32) != pyr0.view(torch.int32)).sum())} of {pyr.numel()} elements differ"
    # one call: pack_hi_as then gemm_hi
    B, D, H, W, L, q_begin, q = GEOMS[name]
    ws1 = torch.full_like(ws, FILL)
    pyr1 = _new_pyr(_lib, GEOMS[name])
    _lib.check(_lib.lib().ecorr_build_split_hi_as(f1.data_ptr(), f2.data_ptr(), _lib.ELEM_FORMATS[dt], B, D, H, W, q, L,
                                                  pyr1.data_ptr(), ws1.data_ptr(), _lib.stream_of(pyr1)), "hi_as")
    torch.cuda.synchronize()
    assert torch.equal(ws1, ws) and torch.equal(pyr1.view(torch.int32), pyr0.view(torch.int32)), name


# ---- 2. one +inf pixel and one NaN pixel: flag 1, equal pyramids
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_nonfinite_pixels_raise_the_flag(ea, plain, name, dt):
    from eraft_amd import _lib
    f1, f2, ws0, pyr0 = plain(name, dt, True)
    ws = _pack_hi(_lib, f1, f2, GEOMS[name])
    _check_hi_ws(ws, ws0, 1, name)
    pyr = _gemm_hi(_lib, ws, GEOMS[name])
    assert bool(torch.isnan(pyr0).any()) and bool(torch.isfinite(pyr0).any())   # the pixels reached it
    _same_off_nans(pyr, pyr0, name)
    # each alone raises it too
    for which in (0, 1):
        g1, g2 = _fmaps(name, dt, False)
        (g1 if which == 0 else g2).copy_((f1 if which == 0 else f2))
        assert _flag(_pack_hi(_lib, g1, g2, GEOMS[name])) == 1, (name, which)


# ---- 3. both loops on one workspace
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_both_loops_give_one_pyramid(ea, plain, name, dt):
    """After the pass on finite 16-bit fmaps (flag 0: the one-term loop), the flag set by hand runs the
    three-term loop on the same panels: the same pyramid bit for bit.  Fails if either loop is wrong."""
    from eraft_amd import _lib
    f1, f2, ws0, pyr0 = plain(name, dt)
    ws = _pack_hi(_lib, f1, f2, GEOMS[name])
    assert _flag(ws) == 0
    one = _gemm_hi(_lib, ws, GEOMS[name])
    _set_flag(ws, 1)
    three = _gemm_hi(_lib, ws, GEOMS[name])
    assert _flag(ws) == 1   # the gemm only reads it
    assert torch.equal(three.view(torch.int32), one.view(torch.int32)), name
    assert torch.equal(three.view(torch.int32), pyr0.view(torch.int32)), name


# ---- 4. the one-term loop really drops lo
def _f32_fmaps(name):
    B, D, H, W, L, q_begin, q = GEOMS[name]
    seed = 1700 + 10 * sorted(GEOMS).index(name)
    a = prng.normal(seed, (B, D, H * W))[:, :, q_begin:q_begin + q]
    b = prng.normal(seed + 1, (B, D, H * W))
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV), torch.from_numpy(b).to(DEV)


def _plain_f32(_lib, f1, f2, geom):
    B, D, H, W, L, q_begin, q = geom
    ws = torch.full((_size(_lib, "ecorr_build_split_workspace_size", geom),), FILL, dtype=torch.uint8, device=DEV)
    pyr = _new_pyr(_lib, geom)
    _lib.check(_lib.lib().ecorr_build_split(f1.data_ptr(), f2.data_ptr(), B, D, H, W, q, L, pyr.data_ptr(), ws.data_ptr(),
                                            _lib.stream_of(pyr)), "build_split")
    torch.cuda.synchronize()
    return ws, pyr


@pytest.mark.parametrize("name", ROUTED)
def test_one_term_loop_drops_lo(ea, name):
    from eraft_amd import _lib
    geom = GEOMS[name]
    B, D, H, W, L, q_begin, q = geom
    f1, f2 = _f32_fmaps(name)   # full 24-bit significands
    ws0, pyr0 = _plain_f32(_lib, f1, f2, geom)
    ws = _pack_hi(_lib, f1, f2, geom)
    _check_hi_ws(ws, ws0, 1, name)
    _same_off_nans(_gemm_hi(_lib, ws, geom), pyr0, f"{name} flag 1")
    _set_flag(ws, 0)
    one = _gemm_hi(_lib, ws, geom)
    assert not torch.equal(one.view(torch.int32), pyr0.view(torch.int32)), "the one-term loop summed the lo terms"
    # ... and is the three-term build of the fmaps rounded to their hi halves, x' = f16(x 2^e) 2^-e,
    # with e the workspace's per-pixel exponents (fmap1's [B][q], then fmap2's [B][H * W])
    ex = ws[FLAG_BYTES:FLAG_BYTES + 4 * B * (q + H * W)].view(torch.int32)
    e1 = ex[:B * q].view(B, 1, q)
    e2 = ex[B * q:].view(B, 1, H * W)
    h1 = torch.ldexp(torch.ldexp(f1, e1).half().float(), -e1)
    h2 = torch.ldexp(torch.ldexp(f2, e2).half().float(), -e2)
    assert not torch.equal(h1, f1) and bool(torch.isfinite(h1).all()) and bool(torch.isfinite(h2).all())
    _, pyr_h = _plain_f32(_lib, h1.contiguous(), h2.contiguous(), geom)
    assert torch.equal(one.view(torch.int32), pyr_h.view(torch.int32)), \
        f"{name}: {int((one.view(torch.int32) != pyr_h.view(torch.int32)).sum())} of {one.numel()} elements differ"


# ---- 5. fp32 fmaps that are f16-representable take the one-term loop too
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_fp32_fmaps_of_f16_values(ea, name):
    from eraft_amd import _lib
    geom = GEOMS[name]
    a, b = _f32_fmaps(name)
    f1, f2 = a.half().float(), b.half().float()
    ws0, pyr0 = _plain_f32(_lib, f1, f2, geom)
    ws = _pack_hi(_lib, f1, f2, geom)
    _check_hi_ws(ws, ws0, 0, name)
    pyr = _gemm_hi(_lib, ws, geom)
    assert not bool(torch.isnan(pyr).any())
    assert torch.equal(pyr.view(torch.int32), pyr0.view(torch.int32)), name


# ---- 6. through the class
class _Spy:
    """lib() with every entry's calls recorded by name."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("ecorr_"):
            return fn

        def call(*a):
            self._calls.append(name)
            return fn(*a)
        return call


def _with_switch(_lib, on, fn):
    before = _lib.build_hi()
    _lib.set_build_hi(on)
    try:
        return fn()
    finally:
        _lib.set_build_hi(before)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["l16_23x40", "div_d250_16x24", "d40_16x20"])
def test_corrblock_switch_on_equals_off(ea, plain, monkeypatch, name, dt):
    from eraft_amd import _lib
    B, D, H, W, L, _, q = GEOMS[name]
    f1, f2, _, _ = plain(name, dt)
    f1, f2 = f1.view(B, D, H, W), f2.view(B, D, H, W)
    coords = torch.from_numpy(prng.coords_with_flow(1801, B, H, W, 2.0)).to(DEV)
    real = _lib.lib()

    def run(on):
        calls = []
        monkeypatch.setattr(_lib, "lib", lambda: _Spy(real, calls))
        try:
            with torch.no_grad():
                blk = _with_switch(_lib, on, lambda: ea.CorrBlock(f1, f2, num_levels=L, radius=4, fmap_dtype=dt))
                outs = [blk(coords), blk(coords, out_dtype=dt)]
                levels = list(blk.corr_pyramid)
        finally:
            monkeypatch.setattr(_lib, "lib", lambda: real)
        torch.cuda.synchronize()
        return calls, levels, outs

    c_on, l_on, o_on = run(True)
    c_off, l_off, o_off = run(False)
    builds = [c for c in c_on if c.startswith("ecorr_build")]
    assert builds == ["ecorr_build_split_hi_workspace_size", "ecorr_build_split_pack_hi_as", "ecorr_build_split_gemm_hi"] or \
        builds == ["ecorr_build_split_pack_hi_as", "ecorr_build_split_gemm_hi"], builds   # (the size entry is cached)
    builds = [c for c in c_off if c.startswith("ecorr_build")]
    assert builds[-2:] == ["ecorr_build_split_pack_as", "ecorr_build_split_gemm"] and not any("_hi" in c for c in c_off), c_off
    for i, (a, b) in enumerate(zip(l_on, l_off)):
        _same_off_nans(a, b, f"{name} level {i}")
    assert o_on[0].dtype == torch.float32 and o_on[1].dtype == dt
    _same_off_nans(o_on[0], o_off[0], f"{name} lookup")
    _same_off_nans(o_on[1].float(), o_off[1].float(), f"{name} 16-bit lookup")
    assert torch.equal(o_on[1].view(torch.int16)[~torch.isnan(o_on[1])], o_off[1].view(torch.int16)[~torch.isnan(o_off[1])])


def test_fp32_fmaps_never_take_the_hi_entries(ea, monkeypatch):
    from eraft_amd import _lib
    a, b = _f32_fmaps("full_16x16")
    real, calls = _lib.lib(), []
    monkeypatch.setattr(_lib, "lib", lambda: _Spy(real, calls))
    try:
        with torch.no_grad():
            _with_switch(_lib, True, lambda: ea.CorrBlock(a.view(1, 256, 16, 16), b.view(1, 256, 16, 16)))
    finally:
        monkeypatch.setattr(_lib, "lib", lambda: real)
    torch.cuda.synchronize()
    assert "ecorr_build_split_pack" in calls and "ecorr_build_split_gemm" in calls and not any("_hi" in c for c in calls)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_fmap_gradients_switch_on_equals_off(ea, dt):
    from eraft_amd import _lib
    B, D, H, W, L, R = 1, 256, 16, 20, 4, 4
    f0 = torch.from_numpy(prng.normal(1811, (B, D, H, W))).to(DEV).to(dt)
    g0 = torch.from_numpy(prng.normal(1812, (B, D, H, W))).to(DEV).to(dt)
    coords = torch.from_numpy(prng.coords_with_flow(1813, B, H, W, 2.0)).to(DEV)

    def run():
        f, g = f0.clone().requires_grad_(True), g0.clone().requires_grad_(True)
        blk = ea.CorrBlock(f, g, num_levels=L, radius=R, differentiable=True, fmap_dtype=dt)
        out = blk(coords)
        out.sum().backward()
        torch.cuda.synchronize()
        return f.grad, g.grad, out.detach()

    on = _with_switch(_lib, True, run)
    off = _with_switch(_lib, False, run)
    assert torch.equal(on[2].view(torch.int32), off[2].view(torch.int32))
    for what, a, b in (("fmap1.grad", on[0], off[0]), ("fmap2.grad", on[1], off[1])):
        assert a.dtype == dt and bool(torch.isfinite(a.float()).all()) and bool((a != 0).any()), what
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), what


# ---- 7. the network
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_eraft_mixed_precision_flow_switch_on_equals_off(ea, dt):
    import os
    from conftest import GOLDEN
    from e2e_weights import make_state_dict
    import eraft_amd.network as nw
    from eraft_amd import _lib
    z = np.load(os.path.join(GOLDEN, "e2e_small_standard.npz"))   # 128 x 160 events -> a 16 x 20 flow
    H, W, bins, seed = int(z["H"]), int(z["W"]), int(z["bins"]), int(z["seed"])
    im1 = torch.from_numpy(prng.normal(seed, (1, bins, H, W))).cuda()
    im2 = torch.from_numpy(prng.normal(seed + 1, (1, bins, H, W))).cuda()
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True   # MIOpen's deterministic algorithm choice, as tests/test_mixed_precision_io_gpu.py
    try:
        def run():
            net = nw.ERAFT({"subtype": str(z["subtype"])}, n_first_channels=bins, mixed_precision=True, amp_dtype=dt,
                           fuse_motion_corr=True)
            net.load_state_dict(make_state_dict(net.state_dict()))
            net = net.cuda().eval()
            with torch.no_grad():
                low, ups = net(im1, im2, iters=2)
            torch.cuda.synchronize()
            return [low] + list(ups)
        on = _with_switch(_lib, True, run)
        off = _with_switch(_lib, False, run)
    finally:
        torch.backends.cudnn.deterministic = saved
    assert len(on) == len(off) == 3
    for a, b in zip(on, off):
        assert a.dtype == torch.float32 and bool(torch.isfinite(a).all())
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 8. one graph capture (a single stream): the memset node
def test_graph_capture_replays_the_hi_build(ea):
    from eraft_amd import _lib
    dt = torch.float16
    B, D, H, W, L = 1, 256, 16, 24, 4
    dev = torch.device("cuda", 0)
    sets = [(torch.from_numpy(prng.normal(1830 + 2 * i, (B, D, H, W))).to(dev).to(dt),
             torch.from_numpy(prng.normal(1831 + 2 * i, (B, D, H, W))).to(dev).to(dt)) for i in range(3)]
    sets[2][1][0, 7, 3, 5] = float("nan")   # the second replay flips the flag the first replay left clear
    f1, f2 = sets[0][0].clone(), sets[0][1].clone()
    out = []

    def step():
        out.clear()
        out.append(ea.CorrBlock(f1, f2, num_levels=L, radius=4, fmap_dtype=dt)._pyramid)

    def eager(a, b):
        return _with_switch(_lib, False, lambda: ea.CorrBlock(a, b, num_levels=L, radius=4, fmap_dtype=dt)._pyramid.clone())

    before = _lib.build_hi()
    _lib.set_build_hi(True)
    try:
        with torch.no_grad():
            s = torch.cuda.Stream(dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                step()   # warm-up on a side stream, as torch.cuda.graphs recommends
            torch.cuda.current_stream(dev).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            for a, b in sets[1:]:
                f1.copy_(a)
                f2.copy_(b)
                g.replay()
                torch.cuda.synchronize()
                _same_off_nans(out[0], eager(a, b), "replay")
            assert bool(torch.isnan(out[0]).any())   # the NaN pixel reached the last replay
    finally:
        _lib.set_build_hi(before)
