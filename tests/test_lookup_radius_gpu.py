"""ecorr_lookup at every radius against the oracle, bit for bit, on the GPU.

Which kernel serves a plain lookup depends on the radius (launch_lookup_plain, csrc/lookup_kernels.h);
tests/lookup_radius_cases.py lists the cases of each kernel (KERNEL) and asserts the list against the
dispatch rule restated from the radius and the level widths:
    lookup_cols_reg<1, PAIR>    r1_pair_18x16, r1_8x32_h1, r1_pair_slab_64x64_l5
    lookup_cols_reg<1, !PAIR>   r1_17x21, r1_slab_17x20, r1_23x40, r1_slab_64x120_l6
    lookup_staged<0>            r0_17x21, r0_8x32_h1
    lookup_staged<2>            r2_17x21, r2_8x32_h1
    lookup_staged<3>            r3_17x21, r3_slab_17x20, r3_23x40, r3_64x64_l5, r3_8x32_h1
    lookup_direct               r5_17x21, r5_slab_17x20, r5_8x32_h1, r5_slab_64x120_l6, r8_16x16, r32_16x16
(radius 4, lookup_cols_reg<4, ...>: tests/test_corr_gpu.py).  r32_16x16 has more outputs than
lookup_direct's 8192 x 256 threads, so its grid-stride loop wraps; the _h1 cases have a level 1 pixel
tall, which the reference makes NaN throughout (it divides by h - 1 = 0); the _l6 slabs read a tiled
level 4 and a compact level 5 (single-column staging at radius 1: their widths turn odd), and
r1_pair_slab_64x64_l5 is the column-pair staging on a slab that starts inside an interleave group,
with a (compact) level 4.

Every case runs the nine coordinate sets of the table -- smooth and large flows, NaN / +-inf / huge
coordinates (the direct-gather mode of the windowed kernels), windows over all four borders, the
integer grid, half pixels, and the integers moved by one ulp and by 1e-4 (the floor flips that the
staged window's slack row and column absorb).  The pyramid is built once per case (C ABI, slab
cases on their query rows only) and the reference is oracle.lookup on the levels read back from it:
tests/test_lookup_radius_ref.py pins that oracle, in this call shape, to ATen's grid_sample, and
asserts from ATen's result alone that NaN, exact-zero and ordinary samples all occur.  The output
lies between two guard bands in a buffer filled with a bit pattern no sample can equal, so a store
outside the output or an element never written shows.  No tolerance anywhere.
"""
import numpy as np
import pytest
import torch

import lookup_radius_cases as lc
import oracle
from gpu_guard import GUARD, check_guarded, guarded, mismatch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


@pytest.fixture(scope="module")
def pyramids(ea):
    """case -> (pyramid, its levels [B q, h_i, w_i] read back, {set: coords [B, 2, 1, q] numpy}): built
    once per case, never written."""
    from eraft_amd import _lib
    from eraft_amd.layout import levels_of
    cache = {}

    def get(name):
        if name not in cache:
            r, B, H, W, L, q_begin, q = lc.CASES[name]
            if name.endswith("_l6"):
                lc.assert_l6_formats()
            f1, f2 = lc.fmaps(name)
            d1 = torch.from_numpy(lc.slab(f1, name)).to(DEV)
            d2 = torch.from_numpy(f2).to(DEV)
            _, _, off = _lib.layout(B * q, H, W, L)
            pyr = _lib.build_pyramid(d1, d2, B, lc.D, H, W, q, L, off, "test build")
            if lc.kernel_of(name).endswith("<1, PAIR>"):   # PAIR's other condition: every level 8-byte aligned
                assert pyr.data_ptr() % 8 == 0 and all(o % 2 == 0 for o in off[:L]), f"{name}: levels at {off}"
            torch.cuda.synchronize()
            levels = [lv[:, 0].cpu().numpy() for lv in levels_of(pyr, B * q, H, W, L)]
            coords = {s: lc.slab(c, name).reshape(B, 2, 1, q) for s, c in lc.coord_sets(name).items()}
            cache.clear()   # one case at a time: the largest level 0 is 64 MB
            cache[name] = (pyr, levels, coords)
        return cache[name]
    return get


def _lookup(pyr, c, name, qmax=None):
    """ecorr_lookup (ecorr_lookup_qmax with qmax) of coords c on the device into a guarded buffer."""
    from eraft_amd import _lib
    r, B, H, W, L, _, q = lc.CASES[name]
    buf, out = guarded(lc.outputs(name))
    if qmax is None:
        st = _lib.lib().ecorr_lookup(pyr.data_ptr(), c.data_ptr(), B, H, W, q, L, r, out.data_ptr(), _lib.stream_of(out))
    else:
        st = _lib.lib().ecorr_lookup_qmax(pyr.data_ptr(), c.data_ptr(), B, H, W, q, L, r, out.data_ptr(),
                                          qmax.data_ptr(), _lib.stream_of(out))
    _lib.check(st, "lookup")
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_lookup_is_the_oracle_bit_for_bit(ea, pyramids, name):
    r, B, H, W, L, _, q = lc.CASES[name]
    C = lc.channels(name)
    pyr, levels, coords = pyramids(name)
    blk = None
    if not lc.is_slab(name):   # the same lookups through the class: its channel count and reshape at K != 9
        f1, f2 = lc.fmaps(name)
        with torch.no_grad():
            blk = ea.CorrBlock(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    bad = []   # every set runs, so a failure names all the sets that differ
    for s, cs in coords.items():
        what = f"{name} / {s}"
        c = torch.from_numpy(cs).to(DEV)
        buf = _lookup(pyr, c, name)
        got = check_guarded(buf, what).reshape(B, C, 1, q)
        want = oracle.lookup(levels, cs, r)
        if not oracle.same_bits(got, want):
            bad.append(f"{what}: {mismatch(got, want)}")
        again = _lookup(pyr, c, name)   # a fresh buffer: deterministic to the bit, NaN payloads too
        assert torch.equal(again, buf), f"{what}: a second call differs"
        if blk is not None:
            with torch.no_grad():
                o = blk(c.view(B, 2, H, W))
            assert tuple(o.shape) == (B, C, H, W) and o.dtype == torch.float32
            assert torch.equal(o.reshape(-1).view(torch.int32), buf[GUARD:-GUARD]), f"{what}: CorrBlock differs"
    assert not bad, "; ".join(bad)


# qmax_kernel is the only writer of the maxima at radii other than 4
@pytest.mark.parametrize("name", ["r0_17x21", "r1_17x21", "r2_17x21", "r8_16x16"])
def test_lookup_qmax_is_the_oracle_and_its_maxima(ea, pyramids, name):
    r, B, H, W, L, _, q = lc.CASES[name]
    C, G = lc.channels(name), 3 * L
    pyr, levels, coords = pyramids(name)
    for s, cs in coords.items():
        what = f"{name} / {s}"
        c = torch.from_numpy(cs).to(DEV)
        qbuf, qmax = guarded(B * G * q)
        got = check_guarded(_lookup(pyr, c, name, qmax=qmax), what).reshape(B, C, 1, q)
        want = oracle.lookup(levels, cs, r)
        assert oracle.same_bits(got, want), f"{what}: {mismatch(got, want)}"
        m = check_guarded(qbuf, what + " qmax").reshape(B, G, q)
        assert not np.isnan(m).any(), f"{what}: NaN maxima"
        # max over the 3 * levels partial maxima = max_c |out| with NaN ignored (fmaxf from 0)
        wmax = np.fmax.reduce(np.abs(want.reshape(B, C, q)), axis=1, initial=np.float32(0.0))
        assert oracle.same_bits(m.max(axis=1), wmax), f"{what}: {mismatch(m.max(axis=1)[:, None], wmax[:, None])}"
