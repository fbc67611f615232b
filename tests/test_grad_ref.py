"""The plain backward references (tests/grad_ref.py) validated on the CPU: against ATen's fp32 autograd of
the reference's op sequence, against the reference's recorded per-level gradients, against the C
oracle's forward through the adjoint identity, and (the build) against fp64 autograd.  No GPU.
"""
import os

import numpy as np
import pytest

import backward_cases as bc
import grad_ref as gr
import oracle
import prng
from conftest import GOLDEN

TOL = 1e-5


def _support_and_err(ref, got, what):
    """Per level: support mismatches must be 0, normwise distance of `got` from `ref` is returned."""
    errs = []
    for i, (r, g) in enumerate(zip(ref, got)):
        assert r.shape == g.shape
        diff = int(((r != 0) != (g != 0)).sum())
        e = oracle.normwise_err(g, r)
        print(f"{what} level {i}: support mismatches {diff} of {r.size} ({int((r != 0).sum())} nonzero), normwise {e:.3g}")
        assert diff == 0, f"{what} level {i}"
        errs.append(e)
    return errs


def _slab(a):
    return a.reshape(a.shape[0], a.shape[1], -1)


@pytest.mark.parametrize("case", list(bc.CASES))
def test_lookup_ref_vs_aten_fp32(case):
    """Every lookup of the five backward cases: the support is ATen's, the values within 1e-5."""
    B, _, H, W, L, r, _ = bc.CASES[case]
    hs, ws = gr.level_sizes(H, W, L)
    for name, coords, gseed in bc.lookups(case):
        go = _slab(bc.upstream(case, gseed))
        ref = gr.lookup_backward_ref(go, _slab(coords), hs, ws, r)
        aten = gr.aten_lookup_backward(go, _slab(coords), hs, ws, r)
        assert all(lv.dtype == np.float64 for lv in ref)
        errs = _support_and_err(ref, aten, f"{case}/{name}")
        assert max(errs) <= TOL


@pytest.mark.parametrize("shape", [(1, 16, 24, 4, 4), (2, 17, 20, 4, 4), (1, 8, 12, 2, 1), (1, 6, 10, 1, 0)],
                         ids=lambda s: "b%d_%dx%d_l%dr%d" % s)
def test_lookup_ref_special_coords(shape):
    """NaN, +-inf, huge, border and half-integer coordinates: the same two assertions, and the queries
    whose coordinate is non-finite or huge add nothing."""
    B, H, W, L, r = shape
    hs, ws = gr.level_sizes(H, W, L)
    K = 2 * r + 1
    go = prng.normal(401, (B, L * K * K, H * W))
    sets = {"edge": gr.edge_coords(B, H, W), "half": prng.coords_with_flow(0, B, H, W, 0.0) + np.float32(0.5)}
    if H * W >= 256:
        sets["special"] = gr.special_coords(402, B, H, W)
    else:   # too small for the blocks: the specials one by one, both channels
        c = prng.coords_with_flow(403, B, H, W, 3.0).reshape(B, 2, -1)
        sp = gr.specials(H, W)
        c[:, 0, :sp.size] = sp
        c[:, 1, sp.size:2 * sp.size] = sp
        sets["special"] = c.reshape(B, 2, H, W)
    for name, coords in sets.items():
        ref = gr.lookup_backward_ref(go, _slab(coords), hs, ws, r)
        aten = gr.aten_lookup_backward(go, _slab(coords), hs, ws, r)
        errs = _support_and_err(ref, aten, f"{name}")
        assert max(errs) <= TOL
        dead = gr.special_rows(coords).reshape(-1)
        if name == "special":
            assert dead.sum() >= 10
        for lv in ref:
            assert not lv[dead].any()


@pytest.mark.parametrize("case", list(bc.PYRAMID_CASES))
def test_lookup_ref_vs_recorded_reference(case):
    """The reference CorrBlock's own recorded fp32 per-level gradients of the whole loss."""
    B, _, H, W, L, r, _ = bc.CASES[case]
    hs, ws = gr.level_sizes(H, W, L)
    z = np.load(os.path.join(GOLDEN, f"backward_{case}.npz"))
    ref = [np.zeros((B * H * W, h, w)) for h, w in zip(hs, ws)]
    for _, coords, gseed in bc.lookups(case):
        for acc, lv in zip(ref, gr.lookup_backward_ref(_slab(bc.upstream(case, gseed)), _slab(coords), hs, ws, r)):
            acc += lv
    errs = _support_and_err(ref, [z[f"pyr_all_l{i}"] for i in range(L)], f"{case} recorded")
    assert max(errs) <= TOL


@pytest.mark.parametrize("shape", [(2, 17, 20, 4, 4), (1, 12, 16, 3, 2), (1, 64, 120, 6, 4)],
                         ids=lambda s: "b%d_%dx%d_l%dr%d" % s)
def test_adjoint_identity_vs_oracle_forward(shape):
    """<lookup(P, coords), go> = sum_i <G_i, P_i> for a random pyramid P, the left side from the C oracle's
    bit-exact forward (summed in fp64): they differ only by the forward's fp32 blend rounding."""
    B, H, W, L, r = shape
    hs, ws = gr.level_sizes(H, W, L)
    K = 2 * r + 1
    rows = H if H * W <= 1024 else 2          # the oracle takes whole maps: a short map of the same width
    P = [prng.normal(500 + i, (B * rows * W, h, w)) for i, (h, w) in enumerate(zip(hs, ws))]
    go = prng.normal(510, (B, L * K * K, rows * W))
    for name, coords in {"s3": prng.coords_with_flow(511, B, H, W, 3.0), "s40": prng.coords_with_flow(512, B, H, W, 40.0),
                         "edge": gr.edge_coords(B, H, W),
                         "half": prng.coords_with_flow(0, B, H, W, 0.0) + np.float32(0.5)}.items():
        c = np.ascontiguousarray(coords[:, :, :rows])
        out = oracle.lookup(P, c, r).astype(np.float64)
        lhs = float((out.reshape(go.shape) * go.astype(np.float64)).sum())
        G = gr.lookup_backward_ref(go, _slab(c), hs, ws, r)
        rhs = float(sum((g * p.astype(np.float64)).sum() for g, p in zip(G, P)))
        rel = abs(lhs - rhs) / abs(rhs)
        print(f"adjoint {shape} {name}: forward {lhs:.9g}, reference {rhs:.9g}, relative {rel:.3g}")
        assert rel <= TOL


BUILD_SHAPES = [(2, 7, 10, 20, 2, 50), (1, 5, 11, 21, 3, 231), (2, 3, 11, 21, 3, 40), (1, 4, 10, 20, 1, 50),
                (1, 2, 64, 120, 6, 7)]


@pytest.mark.parametrize("shape", BUILD_SHAPES, ids=lambda s: "b%d_d%d_%dx%d_l%d_q%d" % s)
def test_build_ref_vs_fp64_autograd(shape):
    """bmm / sqrt(D) then avg_pool2d differentiated by torch in fp64: 1e-12, incl. the odd chain
    11 x 21 -> 5 x 10 -> 2 x 5 (row 10 and column 20 get no pooled term) and query slabs."""
    import torch
    B, D, H, W, L, q = shape
    hs, ws = gr.level_sizes(H, W, L)
    G = [prng.normal(600 + i, (B * q, h, w)).astype(np.float64) for i, (h, w) in enumerate(zip(hs, ws))]
    f1 = prng.normal(610, (B, D, q))
    f2 = prng.normal(611, (B, D, H, W))
    g1, g2 = gr.build_backward_ref(G, f1, f2)
    a1, a2 = gr.aten_build_backward(G, f1, f2, dtype=torch.float64)
    e1, e2 = oracle.normwise_err(g1, a1), oracle.normwise_err(g2, a2)
    print(f"build ref {shape}: grad_fmap1 {e1:.3g}, grad_fmap2 {e2:.3g}")
    assert g1.dtype == g2.dtype == np.float64
    assert e1 <= 1e-12 and e2 <= 1e-12
    if L > 1 and H % 2:   # the dropped row / column carries level 0's own gradient alone
        T = gr.fold_ref(G)
        assert np.array_equal(T[:, H - 1], G[0][:, H - 1]) and np.array_equal(T[:, :, W - 1], G[0][:, :, W - 1])
