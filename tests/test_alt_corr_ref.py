"""The reference of tests/test_alt_corr_gpu.py (tests/alt_corr_ref.py), checked on the CPU.

  * In fp64, pooling the features and then correlating equals correlating and then pooling the volume
    (avg_pool2d over the target axes is linear): 1e-12 normwise on every case and level.  This is the
    identity the volume-free lookup rests on.
  * The reference (fp64 volume, pooled in fp64, rounded once to fp32, sampled by oracle.lookup)
    reproduces the committed reference lookups of tests/golden/corr_*.npz within the GEMM's 1e-5
    normwise, with the same NaN positions.
  * The preconditions that keep the GPU comparison from passing on nothing, from the reference alone:
    per case NaN, exact-zero and ordinary samples all occur, and per (case, level) other than a
    1-pixel-tall level the reference norm over the nine coordinate sets is non-zero.  With these the GPU
    comparison leaves nothing out except NaN positions, and those are compared as a mask.
"""
import glob
import os

import numpy as np
import pytest

import alt_corr_cases as ac
import alt_corr_ref as ar
import oracle
import prng
from conftest import GOLDEN

CORR_CASES = sorted(glob.glob(os.path.join(GOLDEN, "corr_*.npz")))


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_pool_then_correlate_is_correlate_then_pool(name):
    _, _, _, _, _, L = ac.CASES[name]
    f1, f2 = ac.fmaps(name)
    a, b = ar.volume_levels64(f1, f2, L), ar.pooled_feature_levels64(f1, f2, L)
    assert [x.shape for x in a] == [x.shape for x in b]
    assert [x.shape[1:] for x in a] == ac.level_sizes(name)
    for i in range(L):
        err = oracle.normwise_err(b[i], a[i])
        print(f"{name} level {i}: {err:.3g}")
        assert err <= 1e-12, f"level {i}: {err}"


@pytest.mark.parametrize("path", CORR_CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_reference_reproduces_the_golden_lookups(path):
    """The statistic is the GPU test's: per (case, level), max|d| / rms over the case's coordinate sets
    together and over all non-NaN elements.  (A single set is not its domain: in the sigma-40 set 95-99%
    of the samples are exact zeros in both results, which deflates the rms alone -- 1.3e-5 there from the
    golden fp32 GEMM's own 2e-6; the per-set figures are printed.)"""
    z = np.load(path)
    B, D, H, W, seed, L, r = (int(z[k]) for k in ("B", "D", "H", "W", "seed", "L", "r"))
    KK = (2 * r + 1) ** 2
    f1, f2 = prng.normal(seed, (B, D, H, W)), prng.normal(seed + 1, (B, D, H, W))
    lv = ar.levels32(f1, f2, L)
    sets = [k[len("coords_"):] for k in z.files if k.startswith("coords_")]
    assert sets
    got = {s: oracle.lookup(lv, z[f"coords_{s}"], r) for s in sets}
    for s in sets:
        want = z[f"out_{s}"]
        assert got[s].shape == want.shape
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[s]), nan), f"{s}: NaN positions differ"
        if (~nan).any():
            print(f"{os.path.basename(path)} / {s}: {oracle.normwise_err(got[s][~nan], want[~nan]):.3g}")
    for i in range(L):
        g = np.concatenate([got[s][:, i * KK:(i + 1) * KK].reshape(-1) for s in sets])
        w = np.concatenate([z[f"out_{s}"][:, i * KK:(i + 1) * KK].reshape(-1) for s in sets])
        ok = ~np.isnan(w)
        if not ok.any():
            assert min(H >> i, W >> i) == 1, f"level {i}: NaN throughout"   # a 1-pixel side: the reference's NaN level
            continue
        err = oracle.normwise_err(g[ok], w[ok])
        print(f"{os.path.basename(path)} level {i}: {err:.3g}")
        assert err <= 1e-5, f"level {i}: {err}"


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_reference_holds_every_class_of_value(name):
    runs = ar.reference(name)
    assert tuple(runs) == ac.SETS
    allv = np.concatenate([ref.reshape(-1) for _, ref, _ in runs.values()])
    assert np.isnan(allv).any(), "no NaN sample"
    assert np.isnan(runs["special"][1]).any(), "special: no NaN sample"
    assert (allv == 0).any(), "no exact zero (a tap outside the image)"
    assert int((np.isfinite(allv) & (allv != 0)).sum()) >= 500, "too few ordinary samples"
    # the bound scale is defined wherever the reference is, and bounds it
    for s, (_, ref, S) in runs.items():
        assert np.array_equal(np.isnan(ref), np.isnan(S)), s
        ok = ~np.isnan(ref)
        assert (np.abs(ref[ok]) <= S[ok] * (1 + 1e-5)).all(), s


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_reference_norm_is_nonzero_on_every_level(name):
    L = ac.CASES[name][5]
    runs = ar.reference(name)
    for i in range(L):
        v = np.concatenate([ref[:, ar.level_channels(name, i)].reshape(-1) for _, ref, _ in runs.values()])
        if i == ac.h1_level(name):
            assert np.isnan(v).all(), f"level {i}: a 1-pixel-tall level is NaN throughout"
            continue
        v = v[~np.isnan(v)]
        assert v.size and np.sqrt(np.mean(v.astype(np.float64) ** 2)) > 0.01, f"level {i}: the reference norm vanishes"
