"""The references of tests/test_lookup_radius_gpu.py and tests/test_sampler_gpu.py, pinned on the CPU.

The GPU tests compare the kernels with the C oracle (oracle/ecorr_oracle.c) bit for bit.  Here the
oracle itself is compared, bit for bit and NaN positions included, with an independent
implementation that issues the real ATen grid_sample:
  * oracle.lookup against oracle/torch_ref.TorchCpuCorrBlock at every radius, shape and coordinate
    set of tests/lookup_radius_cases.py (the levels are the ones TorchCpuCorrBlock built); for the
    slab cases in the call shape the GPU test uses -- [B, 2, 1, q] coordinates on the slab's rows of
    the levels -- against the slab's columns of the whole-map result;
  * oracle.bilinear_sampler (with its mask) and oracle.coords_grid against the reference's
    definition (model/utils.py:7-27), written out below, on the inputs of tests/sampler_cases.py.
It also carries the preconditions that keep the GPU test from passing on nothing, computed from the
ATen result alone: NaN outputs where they must be and nowhere else, exact zeros (taps outside the
image), and enough ordinary samples.  No tolerance anywhere.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lookup_radius_cases as lc
import oracle
import sampler_cases as sc
from gpu_guard import mismatch
from torch_ref import TorchCpuCorrBlock

_cache = {}


def reference(name):
    """case -> (levels of the case's query rows [B q, h_i, w_i], {set: (coords [B, 2, 1 | H, q | W],
    ATen's output in the same shape)}): computed once, shared by the tests below, never written."""
    if name not in _cache:
        r, B, H, W, L, q_begin, q = lc.CASES[name]
        f1, f2 = lc.fmaps(name)
        sets = lc.coord_sets(name)
        with torch.no_grad():
            blk = TorchCpuCorrBlock(torch.from_numpy(f1), torch.from_numpy(f2), L, r)
            outs = {s: blk(torch.from_numpy(c)).numpy() for s, c in sets.items()}
        levels = [lv[:, 0].numpy() for lv in blk.corr_pyramid]
        if lc.is_slab(name):
            levels = [np.ascontiguousarray(lv.reshape(B, H * W, *lv.shape[1:])[:, q_begin:q_begin + q]
                                           .reshape(B * q, *lv.shape[1:])) for lv in levels]
            runs = {s: (lc.slab(sets[s], name).reshape(B, 2, 1, q), lc.slab(outs[s], name).reshape(B, -1, 1, q))
                    for s in lc.SETS}
        else:
            runs = {s: (sets[s], outs[s]) for s in lc.SETS}
        _cache[name] = (levels, runs)
    return _cache[name]


def test_l6_cases_reach_a_tiled_level_4_and_a_compact_level_5():
    lc.assert_l6_formats()


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_oracle_lookup_is_aten_grid_sample(name):
    r = lc.CASES[name][0]
    levels, runs = reference(name)
    for s, (coords, want) in runs.items():
        got = oracle.lookup(levels, coords, r)
        assert oracle.same_bits(got, want), f"{name} / {s}: {mismatch(got, want)}"


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_reference_outputs_hold_every_class_of_value(name):
    r, B, H, W, L, _, q = lc.CASES[name]
    KK = (2 * r + 1) ** 2
    _, runs = reference(name)
    assert np.isnan(runs["special"][1]).any(), "special: no NaN output"
    smooth = runs["smooth"][1].reshape(B, L * KK, q)
    nan = np.isnan(smooth)
    h1 = lc.h1_level(name)
    if h1 is None:
        assert not nan.any(), "smooth: NaN outputs"
    else:   # the 1-pixel-tall level is NaN everywhere, no other level anywhere
        want = np.zeros_like(nan)
        want[:, h1 * KK:(h1 + 1) * KK] = True
        assert np.array_equal(nan, want), "smooth: NaN outputs are not exactly the level-%d channels" % h1
    allv = np.concatenate([o.reshape(-1) for _, o in runs.values()])
    assert (allv == 0).any(), "no exact zero (a tap outside the image)"
    ordinary = int((np.isfinite(smooth) & (smooth != 0)).sum())
    print(f"{name}: smooth has {ordinary} non-zero finite samples")
    assert ordinary >= 500, f"smooth: only {ordinary} non-zero finite samples"


def _aten_sampler(img, coords):
    """model/utils.py:7-21 with mask=True: the definition."""
    H, W = img.shape[-2:]
    xgrid, ygrid = coords.split([1, 1], dim=-1)
    xgrid = 2 * xgrid / (W - 1) - 1
    ygrid = 2 * ygrid / (H - 1) - 1
    out = F.grid_sample(img, torch.cat([xgrid, ygrid], dim=-1), align_corners=True)
    mask = (xgrid > -1) & (ygrid > -1) & (xgrid < 1) & (ygrid < 1)
    return out, mask.float()


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_oracle_sampler_is_aten_grid_sample(case):
    img, grid = sc.inputs(case)
    with torch.no_grad():
        want, wmask = _aten_sampler(torch.from_numpy(img), torch.from_numpy(grid))
    got, gmask = oracle.bilinear_sampler(img, grid, mask=True)
    assert oracle.same_bits(got, want.numpy()), mismatch(got, want.numpy())
    assert oracle.same_bits(gmask, wmask.numpy()), mismatch(gmask, wmask.numpy())
    assert oracle.same_bits(oracle.bilinear_sampler(img, grid), want.numpy())
    # the inputs decide something: both mask values occur, and unless an image side is 1 pixel (then
    # every sample is NaN) so do NaN, zero and ordinary samples
    assert (gmask == 0).any() and ((gmask == 1).any() or 1 in case[2:4])
    if 1 not in case[2:4]:
        assert np.isnan(got).any() and (got == 0).any() and (np.isfinite(got) & (got != 0)).any()
    else:
        assert np.isnan(got).all()


@pytest.mark.parametrize("shape", sc.GRID_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_oracle_coords_grid_is_the_meshgrid(shape):
    B, H, W = shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")   # utils.py:24-27
    want = torch.stack([xs, ys], dim=0).float()[None].repeat(B, 1, 1, 1).numpy()
    assert oracle.same_bits(oracle.coords_grid(B, H, W), want)
