"""Every level-0 row at the BASELINE batch sizes (corr.py:58-60).

The other GEMM parity tests compare the whole level 0 at B <= 2 and sample rows at the full-size
configs; everything downstream (pooling, lookup) is checked against our own level 0.  Here every row
of level 0 -- C2 (DSEC 60x80, B = 16), the C4 slice (B = 32 per GPU) and C5 (1280x720 -> 92x160,
B = 4, one rank) -- is compared with an independent GEMM on the same GPU: torch.bmm (hipBLASLt /
rocBLAS fp32; TF32 off) divided by sqrt(D), as corr.py:58-60 computes it.  Both build modes; per
query row max|ours - ref| / rms(ref row) <= 1e-5 (GEMM_TOL: the reference's own fp32 GEMM orderings
differ at that level, SURVEY §7 hard part 3), and no row may be all zeros (a dropped store or load
would leave zeros or a stale row: the pyramid buffer is pre-filled with NaN here)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEMM_TOL = 1e-5


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


@pytest.mark.parametrize("mode", ["split", "fp32"])
@pytest.mark.parametrize("B,H,W", [(16, 60, 80), (32, 60, 80), (4, 92, 160)], ids=["C2_b16", "C4_b32", "C5_b4"])
def test_level0_every_row(ea, mode, B, H, W):
    from eraft_amd import _lib
    from eraft_amd.layout import formats, untile
    D, Q = 256, H * W
    torch.backends.cuda.matmul.allow_tf32 = False
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + H)
    with torch.no_grad():
        f1 = torch.randn((B, D, H, W), generator=g, device=DEV)
        f2 = torch.randn((B, D, H, W), generator=g, device=DEV)
        hs, ws, off = _lib.layout(B * Q, H, W, 4)   # the 4-level build E-RAFT runs
        empty = torch.empty

        def nan_empty(*a, **k):
            t = empty(*a, **k)
            return t.fill_(float("nan")) if t.is_floating_point() else t
        try:   # NaN-filled pyramid: an element the build does not write reads back as NaN
            torch.empty = nan_empty
            pyr = _lib.build_pyramid(f1, f2, B, D, H, W, Q, 4, off, "level-0 test", mode=mode)
        finally:
            torch.empty = empty
        lv0 = untile(pyr[off[0]:off[1]], B * Q, hs[0], ws[0], formats(H, W, 4)[0], 0).view(B, Q, Q)
        del pyr
        worst = 0.0
        for b in range(B):
            a = f1[b].reshape(D, Q)
            ref = torch.mm(a.t(), f2[b].reshape(D, Q)) / torch.sqrt(torch.tensor(float(D), device=DEV))
            got = lv0[b]
            assert not torch.isnan(got).any(), f"{mode} b={b}: unwritten elements"
            rms = ref.pow(2).mean(dim=1).sqrt()
            err = (got - ref).abs().amax(dim=1) / rms
            assert (got.abs().amax(dim=1) > 0).all(), f"{mode} b={b}: an all-zero row"
            worst = max(worst, float(err.max()))
            bad = (err > GEMM_TOL).nonzero().flatten()
            assert bad.numel() == 0, f"{mode} b={b}: rows {bad[:8].tolist()} err {err[bad[:8]].tolist()}"
        print(f"{mode} B={B} {H}x{W}: worst row err {worst:.2e}")
