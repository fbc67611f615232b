"""Every GEMM kernel of the forward build (csrc/build.hip) against the oracle, over D, tile
geometry, query slabs, levels and batch sizes: the cases of tests/build_cases.py, whose
kernel_of() restates launch_build's dispatch and names the kernel in every failure.

Raw C ABI calls (ecorr_build_split, ecorr_build_split_pack + ecorr_build_split_gemm, ecorr_build).
Per case and input set:
  - the pyramid lies between two guard bands of gpu_guard.FILL and is pre-filled with it: the guards
    must be intact, every valid element of every level overwritten (padding cells may be either);
  - split mode: the workspace has exactly ecorr_build_split_workspace_size bytes between
    guards (gpu_guard.Workspace), all pre-filled with 0x7E, so a panel or exponent byte the GEMM reads and the operand
    pass never wrote poisons the result (0x7E7E is an f16 NaN, 0x7E7E7E7E a scale of 2^-2e9); the
    guards must be intact; pack + gemm on a second such workspace must give the same pyramid bit
    for bit (the whole buffer, padding included);
  - both fmaps are bitwise unchanged;
  - exact set: every level bit for bit the oracle's; normal set: level 0 within GEMM_TOL normwise of
    the fp64 oracle, the pooled levels bit for bit the pools of the level 0 written
    (build_cases.check_exact / check_normal, shown to reject corrupted builds on the CPU:
    tests/test_build_cases_ref.py);
  - whole-map cases: CorrBlock in the case's build mode gives the same corr_pyramid bit for bit.
The two operand-size cases (2 GiB of fmap2 per batch item: build_kernel<true, false>, and the same
geometry through the split build) make their integers on the device; their reference is the
slab's fp64 matmul on the device, which is exact, divided on the host in float32 by sqrtf(2048).

One line per case (pytest -s): `build_sweep: name kernel normwise_err` (the normal set's level-0
error against fp64; profiles/build_sweep/errors.txt keeps a run's lines).
"""
import ctypes

import numpy as np
import pytest
import torch

import build_cases as bc
import gpu_guard
import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_FILL = 0x7E


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _to_device(a, misaligned):
    """The host array on the device, 16-byte aligned, or (misaligned) as a contiguous view that
    starts 4 bytes into its buffer."""
    t = torch.from_numpy(np.array(a, dtype=np.float32, order="C"))   # a copy: the shared inputs are read-only
    if not misaligned:
        d = t.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    d = buf[1:1 + t.numel()].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    return d


def _bits(t):
    return t.contiguous().view(torch.int32)


def _build(name, f1, f2, two_stage=False):
    """One build of the case through the C ABI -> (the whole guarded int32 buffer, its pyramid part)."""
    from eraft_amd import _lib
    mode, B, D, H, W, L, _, q, _ = bc.CASES[name]
    what = f"{name} [{bc.describe(name)}]"
    _, _, off = _lib.layout(B * q, H, W, L)
    buf, pyr = gpu_guard.guarded(off[-1], DEV)
    assert pyr.data_ptr() % 16 == 0
    st = _lib.stream_of(f2)
    L_ = _lib.lib()
    with torch.no_grad():
        if mode == "split":
            nb = ctypes.c_int64()
            _lib.check(L_.ecorr_build_split_workspace_size(B, D, H, W, q, ctypes.byref(nb)), what)
            ws = gpu_guard.Workspace(nb.value, WS_FILL, DEV)
            if two_stage:
                _lib.check(L_.ecorr_build_split_pack(f1.data_ptr(), f2.data_ptr(), B, D, H, W, q, ws.ptr, st), what)
                _lib.check(L_.ecorr_build_split_gemm(B, D, H, W, q, L, pyr.data_ptr(), ws.ptr, st), what)
            else:
                _lib.check(L_.ecorr_build_split(f1.data_ptr(), f2.data_ptr(), B, D, H, W, q, L, pyr.data_ptr(),
                                                ws.ptr, st), what)
            torch.cuda.synchronize()
            ws.check(what)
            del ws
        else:
            _lib.check(L_.ecorr_build(f1.data_ptr(), f2.data_ptr(), B, D, H, W, q, L, pyr.data_ptr(), st), what)
            torch.cuda.synchronize()
    G = gpu_guard.GUARD
    assert bool((buf[:G] == gpu_guard.FILL).all()) and bool((buf[-G:] == gpu_guard.FILL).all()), \
        f"{what}: a guard band of the pyramid was written"
    return buf, pyr


def _levels(name, pyr):
    """The pyramid's levels in the reference layout, [B * q_count, h_i, w_i] device tensors; every
    valid element must have been written."""
    from eraft_amd import _lib
    from eraft_amd.layout import formats, untile
    _, B, _, H, W, L, _, q, _ = bc.CASES[name]
    h, w, off = _lib.layout(B * q, H, W, L)
    ntx = formats(H, W, L)
    out = []
    for i in range(L):
        lv = untile(pyr[off[i]:off[i + 1]], B * q, h[i], w[i], ntx[i], i)[:, 0]
        left = int((_bits(lv) == gpu_guard.FILL).sum())
        assert left == 0, f"{name} [{bc.describe(name)}]: level {i}: {left} of {lv.numel()} elements never written"
        out.append(lv)
    return out


def _run(ea, name, f1, f2):
    """The case's builds on device fmaps (fmap1 = the query slab [B, D, q_count]) -> its levels as
    device tensors, after the checks that need no reference."""
    mode, B, D, H, W, L, q_begin, q, _ = bc.CASES[name]
    what = f"{name} [{bc.describe(name)}]"
    f1_before, f2_before = f1.clone(), f2.clone()
    buf, pyr = _build(name, f1, f2)
    levels = _levels(name, pyr)
    if mode == "split":
        buf2, _ = _build(name, f1, f2, two_stage=True)
        assert torch.equal(buf, buf2), f"{what}: pack + gemm differs from the one-call build"
        del buf2
    assert torch.equal(_bits(f1), _bits(f1_before)), f"{what}: fmap1 changed"
    assert torch.equal(_bits(f2), _bits(f2_before)), f"{what}: fmap2 changed"
    del f1_before, f2_before
    if q == H * W:   # the class path: CorrBlock in this build mode
        prev = ea._lib.build_mode()
        ea._lib.set_build_mode(mode)
        try:
            with torch.no_grad():
                blk = ea.CorrBlock(f1.view(B, D, H, W), f2, num_levels=L)
                cls = [lv[:, 0] for lv in blk.corr_pyramid]
                torch.cuda.synchronize()
        finally:
            ea._lib.set_build_mode(prev)
        for i in range(L):
            assert torch.equal(_bits(cls[i]), _bits(levels[i])), f"{what}: CorrBlock.corr_pyramid[{i}] differs from the ABI build"
    return levels


@pytest.mark.parametrize("kind", bc.SETS)
@pytest.mark.parametrize("name", bc.HOST_CASES)
def test_build_case(ea, name, kind):
    mis = bc.CASES[name][8]
    what = f"{name} [{bc.describe(name)}] {kind} set"
    f1n, f2n = bc.fmaps(name, kind)
    f1 = _to_device(bc.slab(f1n, name), mis == 1)
    f2 = _to_device(f2n, mis == 2)
    levels = [lv.cpu().numpy() for lv in _run(ea, name, f1, f2)]
    ref = bc.reference(name, kind)
    if kind == "exact":
        bad = bc.check_exact(levels, list(ref))
    else:
        err, bad = bc.check_normal(levels, ref[0])
        print(f"build_sweep: {name} {bc.kernel_of(name)} {err:.3e}")
    assert bad is None, f"{what}: {bad}"


@pytest.mark.parametrize("name", bc.ON_DEVICE)
def test_operand_size_case(ea, name):
    """fmap2 of 2 GiB per batch item: past the 31-bit buffer range of the LDS-DMA staging, so fp32
    mode takes build_kernel<true, false>; the split build's operand pass reads it through 64-bit
    offsets and writes 2 GiB of panels.  Integers in [-7, 7] made on the device; level 0 bit for
    bit the slab's fp64 matmul (exact), divided in float32 by sqrtf(D) on the host."""
    mode, B, D, H, W, L, q_begin, q, _ = bc.CASES[name]
    assert (B, L) == (1, 1) and D * H * W * 4 >= bc.OPERAND_LIMIT
    what = f"{name} [{bc.describe(name)}]"
    gen = torch.Generator(device=DEV)
    gen.manual_seed(bc.seed_of(name))
    f2 = torch.randint(-7, 8, (B, D, H, W), generator=gen, device=DEV, dtype=torch.int8).float()
    f1 = torch.randint(-7, 8, (B, D, q), generator=gen, device=DEV, dtype=torch.int8).float()
    # the planted pixels of the exact set: an all-zero and an all +-7 pixel in each map
    sg = torch.from_numpy(bc.signs7(name)).to(DEV)
    t0 = (H // 2) * W + W // 2
    f2.view(B, D, H * W)[:, :, t0] = 0.0
    f2.view(B, D, H * W)[:, :, t0 + 1] = sg[None, :]
    f1[:, :, 0] = 0.0
    f1[:, :, 1] = sg[None, :]
    assert f1.data_ptr() % 16 == 0 and f2.data_ptr() % 16 == 0
    levels = _run(ea, name, f1, f2)
    got = levels[0].cpu().numpy()
    del levels
    a = f1[0].double().t().contiguous()                      # [q, D]
    S = torch.empty((q, H * W), dtype=torch.float64, device=DEV)
    step = H * W // 8
    for c in range(0, H * W, step):                          # fp64 copies of 256 MiB of fmap2 at a time
        S[:, c:c + step] = torch.matmul(a, f2[0].view(D, H * W)[:, c:c + step].double())
    S = S.cpu().numpy()
    assert np.array_equal(S, np.rint(S)) and np.abs(S).max() == 49 * D < 2 ** 24
    want = (S.astype(np.float32) / np.sqrt(np.float32(D))).reshape(q, H, W)
    print(f"build_sweep: {name} {bc.kernel_of(name)} {oracle.normwise_err(got, want):.3e}")
    bad = bc.check_exact([got], [want])
    assert bad is None, f"{what}: {bad}"
