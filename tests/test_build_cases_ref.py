"""The forward build sweep's references and comparisons, checked on the CPU (tests/build_cases.py).

tests/test_build_sweep_gpu.py compares every GEMM kernel of csrc/build.hip with the oracle: bit for
bit on the exact input set, within GEMM_TOL normwise on the normal set.  Here, without a GPU:
  - the oracle itself is pinned on the exact set: oracle.corr_level0 must be float32(S) / sqrtf(D)
    with the sums S taken in int64 by numpy, and max |S| = 49 D < 2^24 (the +-7 pixels' dot product);
  - both comparisons are shown to reject what a subtly wrong build would write -- channel D - 1
    dropped, one target pixel's column taken from its neighbour, the last K chunk summed twice --
    and to pass the clean result, so a kernel with such an error cannot pass the GPU test;
  - the case table reaches every cell of the kernel x D class x geometry matrix (asserted at the
    import of build_cases too: here it is a test of its own, with the cells in its message).
"""
import numpy as np
import pytest

import build_cases as bc
import oracle


def test_matrix_coverage():
    bc.assert_coverage()
    cov = bc.coverage()
    assert len(cov) == sum(len(ts) for ts in bc.REQUIRED.values())
    assert all(cov.values()), [cell for cell, names in cov.items() if not names]
    # every instantiation launch_build can reach (build_f32_kernel<false> is unreachable: D == 256 implies MUL)
    assert {bc.kernel_of(n) for n in bc.CASES} == {
        "build_split_kernel<MUL>", "build_split_kernel<!MUL>", "build_split16_kernel<MUL>",
        "build_split16_kernel<!MUL>", "build_f32_kernel<MUL>", "build_kernel<true, true>",
        "build_kernel<true, false>", "build_kernel<false, false>"}
    assert {bc.CASES[n][2] for n in bc.CASES if bc.kernel_of(n) == "build_split16_kernel<!MUL>"} == {241, 250, 255}


def test_scale_rule_matches_libm():
    """scale_is_mul restates frexpf(sqrtf(D)) == 0.5: true at the powers of 4 only (D up to 4096)."""
    assert [D for D in range(1, 4097) if bc.scale_is_mul(D)] == [1, 4, 16, 64, 256, 1024, 4096]


@pytest.mark.parametrize("name", bc.HOST_CASES)
def test_oracle_pinned_on_exact_set(name):
    _, B, D, H, W, L, q_begin, q, _ = bc.CASES[name]
    f1, f2 = bc.fmaps(name, "exact")
    for f in (f1, f2):
        assert np.array_equal(f, np.rint(f)) and np.abs(f).max() == 7.0, "exact set: integers in [-7, 7]"
        px = f.reshape(B, D, H * W)
        assert (np.abs(px) == 7.0).all(axis=1).any(axis=1).all(), "a pixel of all +-7 in every batch item"
    qz, q7, tz, t7 = bc.planted(name)
    if tz is not None:
        assert not f2.reshape(B, D, H * W)[:, :, tz].any() and t7 == tz + 1
        assert W < 2 or t7 // W == tz // W, "the +-7 target pixel is the zero pixel's right-hand neighbour"
    if qz is not None:
        assert not f1.reshape(B, D, H * W)[:, :, qz].any()
    a = bc.slab(f1, name).astype(np.int64)                         # [B, D, q]
    b = f2.reshape(B, D, H * W).astype(np.int64)
    S = np.matmul(a.transpose(0, 2, 1), b)                         # [B, q, H * W] int64
    assert S.dtype == np.int64 and np.abs(S).max() == 49 * D < 2 ** 24
    want = (S.astype(np.float32) / np.sqrt(np.float32(D))).reshape(B * q, H, W)
    got = bc.reference(name, "exact")[0]
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert bc.check_exact([got], [want]) is None, bc.check_exact([got], [want])


def _sgemm_level0(name, kind):
    """A stand-in for a correct fp32 build: numpy's float32 GEMM, / sqrtf(D)."""
    _, B, D, H, W, _, _, q, _ = bc.CASES[name]
    f1, f2 = bc.fmaps(name, kind)
    S = np.matmul(bc.slab(f1, name).transpose(0, 2, 1), f2.reshape(B, D, H * W))
    assert S.dtype == np.float32
    return (S / np.sqrt(np.float32(D))).reshape(B * q, H, W)


@pytest.mark.parametrize("name", bc.HOST_CASES)
def test_comparisons_reject_corrupted_builds(name):
    _, B, D, H, W, L, q_begin, q, _ = bc.CASES[name]
    one_pixel = H * W == 1
    for kind in bc.SETS:
        clean = bc.reference(name, kind)
        if kind == "exact":
            assert bc.check_exact(list(clean), list(clean)) is None
            # any correct summation is exact here: numpy's float32 GEMM equals the oracle too
            lv0 = _sgemm_level0(name, kind)
            assert bc.check_exact(oracle.pyramid_from_level0(lv0, L), list(clean)) is None
        else:
            err, bad = bc.check_normal(oracle.pyramid_from_level0(_sgemm_level0(name, kind), L), clean[0])
            assert bad is None and err <= bc.GEMM_TOL, (err, bad)
        for how in bc.CORRUPTIONS:
            wrong = bc.corrupted_levels(name, kind, how)
            if wrong is None:
                assert how == "pixel_from_neighbour" and one_pixel
                continue
            if kind == "exact":
                _, q7, _, t7 = bc.planted(name)
                d = wrong[0].reshape(B, q, H * W)[:, q7 - q_begin, t7 if how != "pixel_from_neighbour" else t7 - 1] \
                    - clean[0].reshape(B, q, H * W)[:, q7 - q_begin, t7 if how != "pixel_from_neighbour" else t7 - 1]
                assert (d != 0).all(), f"{how}: the corrupted channel is zero at the planted pixels"
                assert bc.check_exact(wrong, list(clean)) is not None, f"exact set accepts {how}"
            else:
                err, bad = bc.check_normal(wrong, clean[0])
                assert bad is not None and err > bc.GEMM_TOL, f"normal set accepts {how} (normwise {err:.3e})"
