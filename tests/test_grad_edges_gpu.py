"""csrc/grad.hip at its edges, through the C ABI and the Python API, against the plain fp64 references
of tests/grad_ref.py (validated on the CPU by tests/test_grad_ref.py; nothing here needs a recorded
fixture): the serial path of the lookup backward (NaN, +-inf, huge coordinates), fewer than 64 queries
per workgroup (radius 5 .. 32) and radius 0 / 1, tiled and compact levels >= 4, memory outside the
valid pixels, the build backward alone (D > 256: several d passes; odd level sizes; 6 levels) and the
Python-side branches of the build's backward.

Bars.  Lookup backward: the pixels that receive gradient are exactly the reference's; values normwise
(oracle.normwise_err) within max(1e-5, 2 e_aten), 1e-5 being the project's bar and e_aten the normwise
distance of ATen's fp32 autograd from the same reference on the same inputs (computed here on the
CPU): two independent fp32 summation orders.  Ours and e_aten are printed for every level.
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_ref as gr
import oracle
import prng

pytestmark = pytest.mark.gpu

TOL = 1e-5
DEV = torch.device("cuda:0")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _bar(e_aten):
    return max(TOL, 2.0 * e_aten)


def _lookup_backward(go, coords, H, W, L, r, G=None):
    """ecorr_lookup_backward of go [B][C][q], coords [B][2][q] -> the flat gradient pyramid (device)."""
    from eraft_amd import _lib
    B, _, q = go.shape
    if G is None:
        G = torch.zeros(_lib.layout(B * q, H, W, L)[2][-1], dtype=torch.float32, device=DEV)
    g, c = _cuda(go), _cuda(coords)
    _lib.check(_lib.lib().ecorr_lookup_backward(g.data_ptr(), c.data_ptr(), B, H, W, q, L, r, G.data_ptr(), _stream()),
               "lookup backward")
    torch.cuda.synchronize()
    return G


def _levels(G, rows, H, W, L):
    from eraft_amd.layout import levels_of
    return [lv[:, 0].cpu().numpy() for lv in levels_of(G, rows, H, W, L)]


def _check_lookup(what, go, coords, H, W, L, r):
    """Support exactly the reference's, values within the bar, per level; returns (ours, reference)."""
    B, _, q = go.shape
    hs, ws = gr.level_sizes(H, W, L)
    ref = gr.lookup_backward_ref(go, coords, hs, ws, r)
    aten = gr.aten_lookup_backward(go, coords, hs, ws, r)
    ours = _levels(_lookup_backward(go, coords, H, W, L, r), B * q, H, W, L)
    fails = []
    for i in range(L):
        assert ours[i].shape == ref[i].shape
        diff = int(((ours[i] != 0) != (ref[i] != 0)).sum())
        e_aten = oracle.normwise_err(aten[i], ref[i])
        e = oracle.normwise_err(ours[i], ref[i])
        print(f"{what} level {i} ({hs[i]} x {ws[i]}): support mismatches {diff} of {ref[i].size} "
              f"({int((ref[i] != 0).sum())} nonzero), normwise ours {e:.3g}, ATen fp32 {e_aten:.3g}, bar {_bar(e_aten):.3g}")
        if diff != 0 or not e <= _bar(e_aten):
            fails.append((i, diff, e))
    assert not fails, f"{what}: (level, support mismatches, normwise) {fails}"
    return ours, ref


def _slab(a, q_begin, q):
    """[B, C, H, W] -> the contiguous query slab [B, C, q]."""
    return np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1)[:, :, q_begin:q_begin + q])


# ---------------------------------------------------------------------------------------------
# special coordinates: the serial path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 16, 24), (2, 17, 20)], ids=["b1_16x24_even", "b2_17x20_odd"])
def test_lookup_backward_special_coords(shape):
    """r = 4, L = 4.  A whole 64-query block of NaN / +-inf / huge / border coordinates, a block mixing
    them with normal queries, a block with one special axis; windows over all four edges; int + 0.5."""
    _need_gpu()
    B, H, W = shape
    L, r = 4, 4
    go = prng.normal(701, (B, L * 81, H * W))
    sets = {"special": gr.special_coords(702, B, H, W), "edge": gr.edge_coords(B, H, W),
            "half": prng.coords_with_flow(0, B, H, W, 0.0) + np.float32(0.5)}
    for name, coords in sets.items():
        c = _slab(coords, 0, H * W)
        ours, ref = _check_lookup(f"{shape} {name}", go, c, H, W, L, r)
        if name != "special":
            continue
        dead = gr.special_rows(coords).reshape(-1)
        assert dead.sum() >= 64 * B
        for i in range(L):
            zero_rows = ~ref[i].reshape(ref[i].shape[0], -1).any(axis=1)
            assert zero_rows[dead].all()          # NaN, +-inf and huge coordinates add nothing (the reference)
            assert not ours[i][zero_rows].any(), f"level {i}: gradient in a row the reference leaves all-zero"


# ---------------------------------------------------------------------------------------------
# radius sweep: queries per workgroup 64 (r <= 4), 32 (r = 5), 16 (r = 8), 1 (r = 32); K = 1 at r = 0
# ---------------------------------------------------------------------------------------------
RADII = [(0, 1, 6, 10, 1, 60), (1, 2, 8, 8, 3, 64), (5, 2, 12, 16, 3, 100), (8, 1, 12, 16, 2, 70), (32, 2, 8, 12, 2, 40)]


@pytest.mark.parametrize("cfg", RADII, ids=lambda c: "r%d_b%d_%dx%d_l%d_q%d" % c)
def test_lookup_backward_radius_sweep(cfg):
    _need_gpu()
    r, B, H, W, L, q = cfg
    K = 2 * r + 1
    go = prng.normal(710 + r, (B, L * K * K, q))
    q_begin = (H * W - q) // 2
    coords = _slab(prng.coords_with_flow(711 + r, B, H, W, 3.0), q_begin, q)
    _check_lookup(f"r{r}", go, coords, H, W, L, r)


# ---------------------------------------------------------------------------------------------
# level formats: tiled and compact levels >= 4
# ---------------------------------------------------------------------------------------------
# (B, H, W, L, q_begin, q, {level: format}): ntx > 0 tiled with ntx tiles per tile row, 0 compact
FORMATS = [(2, 64, 120, 6, 32 * 120, 120, {0: 15, 4: 1, 5: 0}),
           (1, 64, 272, 5, 30 * 272 + 50, 100, {0: 34, 4: 3}),
           (1, 32, 40, 5, 0, 1280, {0: 5, 4: 0})]


def _assert_formats(H, W, L, want):
    from eraft_amd.layout import formats
    got = formats(H, W, L)
    for lv, ntx in want.items():
        assert got[lv] == ntx, f"{H} x {W}: level {lv} has format {got[lv]}, this test was written for {ntx}"
    assert all(n < 0 for n in got[1:4])


@pytest.mark.parametrize("sigma", [3.0, 40.0], ids=["s3", "s40"])
@pytest.mark.parametrize("cfg", FORMATS, ids=lambda c: "b%d_%dx%d_l%d_q%d" % (c[0], c[1], c[2], c[3], c[5]))
def test_lookup_backward_level_formats(cfg, sigma):
    _need_gpu()
    B, H, W, L, q_begin, q, want = cfg
    _assert_formats(H, W, L, want)
    go = prng.normal(720, (B, L * 81, q))
    coords = _slab(prng.coords_with_flow(721, B, H, W, sigma), q_begin, q)
    _check_lookup(f"{H}x{W} L{L} s{sigma:g}", go, coords, H, W, L, 4)


# ---------------------------------------------------------------------------------------------
# nothing outside the valid pixels is written
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(2, 17, 20, 4, 100), (2, 64, 120, 6, 120)], ids=["17x20_l4_q100", "64x120_l6_q120"])
def test_lookup_backward_writes_only_valid_pixels(cfg):
    """Tile padding, interleave block padding, the pad rows of a 64-row group, the gaps between levels
    and 4096 floats past the pyramid keep a sentinel bit for bit through lookup backwards of in-range,
    far and special coordinates."""
    _need_gpu()
    from eraft_amd import _lib
    from eraft_amd.layout import pack
    B, H, W, L, q = cfg
    TAIL = 4096
    hs, ws, off = _lib.layout(B * q, H, W, L)
    valid = pack([torch.ones(B * q, h, w) for h, w in zip(hs, ws)], H, W) != 0
    assert valid.numel() == off[-1] and int(valid.sum()) == B * q * sum(h * w for h, w in zip(hs, ws))
    assert int((~valid).sum()) > 0
    sentinel = torch.tensor(-1234.5678, dtype=torch.float32)
    host = torch.full((off[-1] + TAIL,), float(sentinel), dtype=torch.float32)
    host[:off[-1]][valid] = 0.0
    G = host.to(DEV)
    go = prng.normal(730, (B, L * 81, q))
    q_begin = (H // 2) * W
    fields = [prng.coords_with_flow(731, B, H, W, 3.0), prng.coords_with_flow(732, B, H, W, 40.0),
              gr.edge_coords(B, H, W), gr.special_coords(733, B, H, W)]
    for i, f in enumerate(fields):
        _lookup_backward(go, _slab(f, q_begin if i < 3 else 0, q), H, W, L, 4, G=G)
    after = G.cpu()
    outside = torch.cat([~valid, torch.ones(TAIL, dtype=torch.bool)])
    changed = after.view(torch.int32)[outside] != host.view(torch.int32)[outside]
    print(f"{H} x {W} L{L}: {int(outside.sum())} cells outside the valid pixels, {int(changed.sum())} changed")
    assert not changed.any(), f"first changed float offsets: {torch.nonzero(outside)[changed][:8, 0].tolist()} (levels at {off})"
    assert after[:off[-1]][valid].abs().sum() > 0   # the launches did write


# ---------------------------------------------------------------------------------------------
# ecorr_build_backward alone
# ---------------------------------------------------------------------------------------------
# (B, D, H, W, L, q)
BUILDS = [(2, D, 10, 20, 2, 50) for D in (1, 31, 257, 300, 513)] + \
         [(2, 31, 10, 20, 1, 50), (1, 64, 11, 21, 3, 231), (2, 16, 64, 120, 6, 120)]


@pytest.mark.parametrize("cfg", BUILDS, ids=lambda c: "b%d_d%d_%dx%d_l%d_q%d" % c)
def test_build_backward_alone(cfg):
    """Dense random G on the valid pixels of every level (no lookup involved).  D > 256 runs the second
    and third d pass; 11 x 21 folds odd sizes at two levels; 64 x 120 folds tiled and compact levels
    >= 4.  NaN-prefilled outputs come back finite; NULL for either output leaves the other bitwise."""
    _need_gpu()
    from eraft_amd import _lib
    from eraft_amd.layout import pack
    B, D, H, W, L, q = cfg
    hs, ws = gr.level_sizes(H, W, L)
    Gl = [prng.normal(740 + i, (B * q, h, w)) for i, (h, w) in enumerate(zip(hs, ws))]
    q_begin = (H * W - q) // 2
    f1 = _slab(prng.normal(750, (B, D, H, W)), q_begin, q)
    f2 = prng.normal(751, (B, D, H, W))
    r1, r2 = gr.build_backward_ref(Gl, f1, f2)
    a1, a2 = gr.aten_build_backward(Gl, f1, f2)
    Gflat = pack([torch.from_numpy(g) for g in Gl], H, W).to(DEV)
    d1, d2 = _cuda(f1), _cuda(f2)

    def run(want1=True, want2=True):
        G = Gflat.clone()   # the build backward consumes it
        g1 = torch.full((B, D, q), float("nan"), device=DEV) if want1 else None
        g2 = torch.full((B, D, H, W), float("nan"), device=DEV) if want2 else None
        _lib.check(_lib.lib().ecorr_build_backward(G.data_ptr(), d1.data_ptr(), d2.data_ptr(), B, D, H, W, q, L,
                                                   None if g1 is None else g1.data_ptr(),
                                                   None if g2 is None else g2.data_ptr(), _stream()), "build backward")
        torch.cuda.synchronize()
        return g1, g2

    g1, g2 = run()
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    for name, ours, ref, aten in (("grad_fmap1", g1, r1, a1), ("grad_fmap2", g2, r2, a2)):
        e_aten = oracle.normwise_err(aten, ref)
        e = oracle.normwise_err(ours.cpu().numpy(), ref)
        print(f"build backward {cfg} {name}: normwise ours {e:.3g}, ATen fp32 {e_aten:.3g}, bar {_bar(e_aten):.3g}")
        assert e <= _bar(e_aten), name
    only1, none2 = run(want2=False)
    none1, only2 = run(want1=False)
    assert none1 is None and none2 is None
    assert torch.equal(only1, g1) and torch.equal(only2, g2)
    if L > 1 and H % 2:   # 11 x 21: row 10 / column 20 of level 0 take no pooled term (the reference asserts it too)
        T = gr.fold_ref(Gl)
        assert np.array_equal(T[:, H - 1], Gl[0][:, H - 1].astype(np.float64))


# ---------------------------------------------------------------------------------------------
# the Python API: branches of _BuildFn.backward
# ---------------------------------------------------------------------------------------------
API = (3, 32, 10, 14, 3, 2)   # B, D, H, W, L, r


def _api_inputs():
    B, D, H, W, L, r = API
    C = L * (2 * r + 1) ** 2
    f1, f2 = prng.normal(760, (B, D, H, W)), prng.normal(761, (B, D, H, W))
    coords = [prng.coords_with_flow(762 + i, B, H, W, s) for i, s in enumerate((0.5, 6.0, 3.0))]
    wgt = [prng.normal(766 + i, (B, H, W, C)) for i in range(2)]   # channels last: the loss permutes the lookup
    return f1, f2, coords, wgt


def _api_run(req1, req2):
    """Gradients of sum_i (blk(coords_i).permute(0, 2, 3, 1) * wgt_i).sum() over the first two of three
    lookups (the third is made and ignored)."""
    import eraft_amd
    B, D, H, W, L, r = API
    f1n, f2n, coords, wgt = _api_inputs()
    f1, f2 = _cuda(f1n).requires_grad_(req1), _cuda(f2n).requires_grad_(req2)
    blk = eraft_amd.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    outs = [blk(_cuda(c)) for c in coords]
    seen = []
    for o in outs[:2]:
        o.register_hook(lambda g: seen.append(g.is_contiguous()))
    loss = sum((o.permute(0, 2, 3, 1) * _cuda(w)).sum() for o, w in zip(outs[:2], wgt))
    loss.backward()
    torch.cuda.synchronize()
    assert seen == [False, False], "the upstream gradients were meant to arrive non-contiguous"
    return f1.grad, f2.grad


def test_python_api_backward_branches():
    _need_gpu()
    import eraft_amd
    B, D, H, W, L, r = API
    hs, ws = gr.level_sizes(H, W, L)
    f1n, f2n, coords, wgt = _api_inputs()
    # expected: the two references chained (and ATen fp32 chained the same way, for the bar)
    G = [np.zeros((B * H * W, h, w)) for h, w in zip(hs, ws)]
    Ga = [np.zeros((B * H * W, h, w), dtype=np.float32) for h, w in zip(hs, ws)]
    for c, w in zip(coords[:2], wgt):
        go = np.ascontiguousarray(w.transpose(0, 3, 1, 2)).reshape(B, -1, H * W)
        cc = c.reshape(B, 2, H * W)
        for acc, lv in zip(G, gr.lookup_backward_ref(go, cc, hs, ws, r)):
            acc += lv
        for acc, lv in zip(Ga, gr.aten_lookup_backward(go, cc, hs, ws, r)):
            acc += lv
    r1, r2 = gr.build_backward_ref(G, f1n.reshape(B, D, -1), f2n)
    a1, a2 = gr.aten_build_backward(Ga, f1n.reshape(B, D, -1), f2n)

    g1, g2 = _api_run(True, True)
    for name, ours, ref, aten in (("grad_fmap1", g1, r1.reshape(f1n.shape), a1.reshape(f1n.shape)), ("grad_fmap2", g2, r2, a2)):
        e_aten = oracle.normwise_err(aten, ref)
        e = oracle.normwise_err(ours.cpu().numpy(), ref)
        print(f"python API {name}: normwise ours {e:.3g}, ATen fp32 {e_aten:.3g}, bar {_bar(e_aten):.3g}")
        assert e <= _bar(e_aten), name
    # only one fmap requires grad
    o1, n2 = _api_run(True, False)
    assert n2 is None and torch.equal(o1, g1)
    n1, o2 = _api_run(False, True)
    assert n1 is None and torch.equal(o2, g2)

    # no lookup receives a gradient, but the build's node is reached through the handle: `G is None`
    f1, f2 = _cuda(f1n).requires_grad_(True), _cuda(f2n).requires_grad_(True)
    blk = eraft_amd.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    for c in coords:
        blk(_cuda(c))
    other = (f1 * f2).sum()
    (other + blk._handle.sum()).backward()
    torch.cuda.synchronize()
    assert blk._grad.consumed and blk._grad.buf is None   # _BuildFn.backward ran and no gradient pyramid ever existed
    assert torch.equal(f1.grad, f2.detach()) and torch.equal(f2.grad, f1.detach())   # other's gradient plus exact zeros
