"""The volume-free lookup (ecorr_alt_pack_as / ecorr_alt_lookup_as, AlternateCorrBlock) on the GPU.

It computes CorrBlock's function with the arithmetic reordered, so it is compared with the fp64
reference of tests/alt_corr_ref.py (tests/test_alt_corr_ref.py checks that reference on the CPU) on the
cases and the nine coordinate sets of tests/alt_corr_cases.py:
  * NaN mask: the output's NaN positions are the reference's; where the reference is exactly 0 (every
    contributing corner outside the image) the output is exactly 0 -- both hold by construction, the
    kernels take positions and in-image tests from the volume lookup's own device functions.
  * Normwise: per (case, level), over the nine sets together and all non-NaN elements,
    max|got - ref| / rms(ref) <= 1e-5, the project's bar for the GEMM the volume block is held to.
  * Elementwise: |got - ref| <= (D + 32) 2^-24 S for every non-NaN element, S the same lookup of
    |f1|, |f2| -- the fp32 dot-product bound gamma_D on sum |a_i b_i|, the remaining <= 20 roundings for
    the pooling, scale, blend and the reference's own fp32 steps; it catches a single wrong query.
  * A second call is bitwise the first; 16-bit outputs are bitwise fp32_result.to(dtype); 16-bit fmaps
    give bitwise the block on fmap.float(); the class returns the C ABI's bits.
  * Memory: construction plus one lookup at B = 1, D = 64, 48 x 64 stays within the feature buffer +
    output + coords + 1 MB, below the 37.7 MB of the level-0 volume alone.
  * The forward-only contract raises, and ERAFT(alternate_corr=True) gives the default network's flow
    within the project's end-to-end bar of 1e-3 px, in fp32 and with mixed_precision=True.
Every C ABI output (the feature buffer included) lies between guard bands in a buffer filled with a bit
pattern no result can equal: a store outside it or an element never written shows.
"""
import ctypes

import numpy as np
import pytest
import torch

import alt_corr_cases as ac
import alt_corr_ref as ar
import oracle
import prng
from e2e_weights import make_state_dict
from gpu_guard import FILL, GUARD, check_guarded, guarded, mismatch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF = {torch.float16: 1, torch.bfloat16: 2}


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _pack(name, f1, f2):
    """ecorr_alt_pack_as of device fmaps (fp32 / f16 / bf16) into a guarded feature buffer -> (buf, feat)."""
    from eraft_amd import _lib
    _, B, D, H, W, L = ac.CASES[name]
    n = ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_alt_size(B, D, H, W, L, ctypes.byref(n)), "alt size")
    buf, feat = guarded(n.value)
    _lib.check(_lib.lib().ecorr_alt_pack_as(f1.data_ptr(), f2.data_ptr(), _lib.ELEM_FORMATS[f1.dtype], B, D, H, W, L,
                                            feat.data_ptr(), _lib.stream_of(feat)), "alt pack")
    torch.cuda.synchronize()
    check_guarded(buf, f"{name}: feature buffer")
    return buf, feat


def _lookup(feat, c, name, fmt=0):
    """ecorr_alt_lookup_as into a guarded buffer (2-byte formats: two elements per guarded float)."""
    from eraft_amd import _lib
    r, B, D, H, W, L = ac.CASES[name]
    n = B * ac.channels(name) * H * W
    assert fmt == 0 or n % 2 == 0
    buf, out = guarded(n if fmt == 0 else n // 2)
    _lib.check(_lib.lib().ecorr_alt_lookup_as(feat.data_ptr(), c.data_ptr(), B, D, H, W, L, r, out.data_ptr(), fmt,
                                              _lib.stream_of(out)), "alt lookup")
    torch.cuda.synchronize()
    return buf


@pytest.fixture(scope="module")
def runs(ea):
    """case -> (feat, block, {set: (device coords, guarded output buffer, output [B, C, H, W] numpy)}): each
    case packed and looked up once through the C ABI, shared by the tests, never written."""
    cache = {}

    def get(name):
        if name not in cache:
            r, B, D, H, W, L = ac.CASES[name]
            f1, f2 = (torch.from_numpy(f).to(DEV) for f in ac.fmaps(name))
            _, feat = _pack(name, f1, f2)
            with torch.no_grad():
                blk = ea.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)
            outs = {}
            for s, (cs, _, _) in ar.reference(name).items():
                c = torch.tensor(cs, device=DEV)   # (the reference's arrays are read-only)
                buf = _lookup(feat, c, name)
                got = check_guarded(buf, f"{name} / {s}").reshape(B, ac.channels(name), H, W)
                outs[s] = (c, buf, got)
            cache[name] = (feat, blk, outs)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_nan_mask_and_exact_zeros_are_the_references(runs, name):
    _, _, outs = runs(name)
    bad = []
    for s, (_, ref, _) in ar.reference(name).items():
        got = outs[s][2]
        if not np.array_equal(np.isnan(got), np.isnan(ref)):
            bad.append(f"{s}: {int((np.isnan(got) != np.isnan(ref)).sum())} NaN positions differ")
        zero = ref == 0
        if not (got[zero] == 0).all():
            bad.append(f"{s}: {int((got[zero] != 0).sum())} of {int(zero.sum())} exact zeros are not zero")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_normwise_error_per_level(runs, name):
    L = ac.CASES[name][5]
    _, _, outs = runs(name)
    ref = ar.reference(name)
    for i in range(L):
        ch = ar.level_channels(name, i)
        g = np.concatenate([outs[s][2][:, ch].reshape(-1) for s in ac.SETS])
        w = np.concatenate([ref[s][1][:, ch].reshape(-1) for s in ac.SETS])
        ok = ~np.isnan(w)
        if i == ac.h1_level(name):
            assert not ok.any()
            continue
        err = oracle.normwise_err(g[ok], w[ok])
        print(f"{name} level {i} ({ac.kernel_of(name)}): normwise {err:.3g} over {int(ok.sum())} elements")
        assert err <= 1e-5, f"level {i}: normwise error {err}"


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_elementwise_error_bound(runs, name):
    D = ac.CASES[name][2]
    _, _, outs = runs(name)
    worst = 0.0
    for s, (_, ref, S) in ar.reference(name).items():
        got = outs[s][2]
        ok = ~np.isnan(ref) & ~np.isnan(got)
        d = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64))
        bound = (D + 32) * 2.0 ** -24 * S[ok].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, d / bound, 0.0), initial=0.0)))
        n = int((d > bound).sum())
        assert n == 0, (f"{name} / {s}: {n} elements beyond (D + 32) 2^-24 S; first: got {got[ok][d > bound][0]!r}, "
                        f"reference {ref[ok][d > bound][0]!r}, S {S[ok][d > bound][0]!r}")
    print(f"{name}: largest |got - ref| / bound = {worst:.3g}")


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_second_call_and_class_are_bitwise_the_first(runs, name):
    r, B, D, H, W, L = ac.CASES[name]
    feat, blk, outs = runs(name)
    for s, (c, buf, _) in outs.items():
        again = _lookup(feat, c, name)
        assert torch.equal(again, buf), f"{name} / {s}: a second call differs"
        with torch.no_grad():
            o = blk(c)
        assert tuple(o.shape) == (B, ac.channels(name), H, W) and o.dtype == torch.float32
        assert torch.equal(o.reshape(-1).view(torch.int32), buf[GUARD:-GUARD]), f"{name} / {s}: the class differs"


@pytest.mark.parametrize("dt", list(HALF), ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["a4_17x21_d37", "a1_17x21_d8", "a5_17x21_d8"])
def test_16bit_output_is_the_fp32_result_rounded_once(runs, name, dt):
    feat, blk, outs = runs(name)
    for s in ("smooth", "special", "edge"):
        c, buf, _ = outs[s]
        want = buf[GUARD:-GUARD].view(torch.float32).to(dt).view(torch.int16)
        hbuf = _lookup(feat, c, name, HALF[dt])
        host = hbuf.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), f"{name} / {s}: a guard band was written"
        got = hbuf[GUARD:-GUARD].view(torch.int16)
        # every element written: the fill pattern as two halves is 0x7b7b, a value the fp32 result would
        # have to round to in both halves of one word
        assert int((hbuf[GUARD:-GUARD] == FILL).sum()) == 0, f"{name} / {s}: elements never written"
        nan = torch.isnan(want.view(dt))
        assert torch.equal(torch.isnan(got.view(dt)), nan)
        assert torch.equal(got[~nan], want[~nan]), f"{name} / {s} {dt}: not fp32.to(dtype)"
        with torch.no_grad():
            o = blk(c, out_dtype=dt)
        assert o.dtype == dt and torch.equal(o.reshape(-1).view(torch.int16), got), f"{name} / {s}: the class differs"


@pytest.mark.parametrize("dt", list(HALF), ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["a4_17x21_d37", "a5_17x21_d8"])
def test_16bit_fmaps_are_the_block_on_their_float(ea, name, dt):
    r, B, D, H, W, L = ac.CASES[name]
    h1, h2 = (torch.from_numpy(f).to(DEV).to(dt) for f in ac.fmaps(name))
    _, feat16 = _pack(name, h1, h2)
    _, feat32 = _pack(name, h1.float(), h2.float())
    assert torch.equal(feat16.view(torch.int32), feat32.view(torch.int32)), "the packs differ"
    c = torch.from_numpy(ac.coord_sets(name)["smooth"]).to(DEV)
    with torch.no_grad():
        a = ea.AlternateCorrBlock(h1, h2, num_levels=L, radius=r, fmap_dtype=dt)(c)
        b = ea.AlternateCorrBlock(h1.float(), h2.float(), num_levels=L, radius=r)(c)
    assert not torch.isnan(a).any() and torch.equal(a, b)
    with pytest.raises(TypeError):   # a 16-bit fmap without the keyword still raises, as CorrBlock's
        ea.AlternateCorrBlock(h1, h2, num_levels=L, radius=r)


def test_memory_grows_with_q_not_q_squared(ea):
    from eraft_amd import _lib
    B, D, H, W, L, r = 1, 64, 48, 64, 4, 4
    f1 = torch.from_numpy(prng.normal(71, (B, D, H, W))).to(DEV)
    f2 = torch.from_numpy(prng.normal(72, (B, D, H, W))).to(DEV)
    c = torch.from_numpy(prng.coords_with_flow(73, B, H, W, 2.0)).to(DEV)
    n = ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_alt_size(B, D, H, W, L, ctypes.byref(n)), "alt size")
    allowed = n.value * 4 + B * _lib.corr_channels(L, r) * H * W * 4 + c.numel() * 4 + (1 << 20)
    assert allowed < (H * W) ** 2 * 4 == 37748736   # the level-0 volume alone
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = ea.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)(c)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - base
    print(f"construction + one lookup: {used} bytes, allowed {allowed}, level-0 volume {(H * W) ** 2 * 4}")
    assert bool(torch.isfinite(out).all())
    assert used <= allowed


def test_forward_only_contract(ea):
    import eraft_amd.network as nw
    name = "a1_17x21_d8"
    r, B, D, H, W, L = ac.CASES[name]
    f1, f2 = (torch.from_numpy(f).to(DEV) for f in ac.fmaps(name))
    c = torch.from_numpy(ac.coord_sets(name)["smooth"]).to(DEV)
    with pytest.raises(RuntimeError, match="forward-only"):   # inputs that require grad while grad mode is on
        ea.AlternateCorrBlock(f1.clone().requires_grad_(True), f2, num_levels=L, radius=r)
    with torch.no_grad():                                       # ... and not under no_grad
        blk = ea.AlternateCorrBlock(f1.clone().requires_grad_(True), f2, num_levels=L, radius=r)
    with pytest.raises(RuntimeError, match="forward-only"):
        blk(c.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="differentiable"):
        ea.AlternateCorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    with pytest.raises(NotImplementedError, match="corr_pyramid"):
        blk.corr_pyramid
    with pytest.raises(NotImplementedError, match="lookup_conv1x1_relu"):
        blk.lookup_conv1x1_relu(c, torch.zeros(8, ac.channels(name), device=DEV))
    for shape in ((0, D, H, W), (B, 0, H, W), (B, D, 0, W), (B, D, H, 0)):   # D = 0 and empty shapes
        e = torch.zeros(shape, device=DEV)
        with pytest.raises(RuntimeError, match="empty"):
            ea.AlternateCorrBlock(e, e, num_levels=1, radius=r)
    with pytest.raises(RuntimeError, match="contiguous"):
        ea.AlternateCorrBlock(f1.transpose(2, 3).contiguous().transpose(2, 3), f2, num_levels=L, radius=r)
    with pytest.raises(RuntimeError, match="coords shape"):
        blk(c[:, :, :-1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        blk(c.cpu())
    with pytest.raises(TypeError, match="out_dtype"):
        blk(c, out_dtype=torch.float64)
    with pytest.raises(TypeError, match="fmap_dtype"):
        ea.AlternateCorrBlock(f1, f2, fmap_dtype=torch.float64)
    with pytest.raises(ValueError):   # a level that pools to 0 pixels
        ea.AlternateCorrBlock(f1, f2, num_levels=6, radius=r)
    with pytest.raises(ValueError, match="alternate_corr"):
        nw.ERAFT({"subtype": "standard"}, n_first_channels=5, alternate_corr=True, fuse_motion_corr=True)


def _epe(a, b):
    d = a.double() - b.double()
    return float(d.pow(2).sum(dim=1).sqrt().mean())


def _flow(calls, **kw):
    """The final full-resolution flow of ERAFT(**kw) with the PRNG weights: 128 x 128, 5 bins, B = 1, 3 iterations."""
    import eraft_amd.alt_corr as alt
    import eraft_amd.network as nw
    net = nw.ERAFT({"subtype": "standard"}, n_first_channels=5, **kw)
    net.load_state_dict(make_state_dict(net.state_dict()))
    net = net.cuda().eval()
    im1 = torch.from_numpy(prng.normal(9101, (1, 5, 128, 128))).cuda()
    im2 = torch.from_numpy(prng.normal(9102, (1, 5, 128, 128))).cuda()
    orig = alt.AlternateCorrBlock.__call__

    def call(self, coords, out_dtype=None):
        calls.append(out_dtype)
        return orig(self, coords, out_dtype=out_dtype)
    alt.AlternateCorrBlock.__call__ = call
    try:
        with torch.no_grad():
            _, ups = net(im1, im2, iters=3)
    finally:
        alt.AlternateCorrBlock.__call__ = orig
    assert ups[-1].dtype == torch.float32 and bool(torch.isfinite(ups[-1]).all())
    return ups[-1]


@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "mixed_precision"])
def test_eraft_alternate_corr_end_to_end(ea, mixed):
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True   # MIOpen's deterministic algorithm choice for both arms
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    try:
        kw = {"mixed_precision": True} if mixed else {}
        base_calls, alt_calls = [], []
        base = _flow(base_calls, **kw)
        got = _flow(alt_calls, alternate_corr=True, **kw)
    finally:
        torch.backends.cudnn.deterministic = saved
    assert base_calls == [] and alt_calls == [torch.float16 if mixed else None] * 3
    e = _epe(got, base)
    print(f"mixed_precision={mixed}: EPE(alternate_corr, default) = {e:.3g} px (|flow| mean {float(base.abs().mean()):.3g} px)")
    assert e <= 1e-3, f"EPE {e} px"
