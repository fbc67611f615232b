"""bilinear_sampler and coords_grid (sampler_kernel, coords_grid_kernel of csrc/lookup.hip) against
the oracle, bit for bit, on the GPU.

The inputs are those of tests/sampler_cases.py: a general image, images 1 pixel tall, wide and both
(the reference divides by size - 1 = 0), a 2 x 2 image, and a 1500 x 1400 grid whose 2.1 M points
pass the 8192 x 256 threads of one pass of the kernel's grid-stride loop; every grid leads with
coordinates exactly on, one ulp inside and one pixel outside the borders, signed zero, NaN, +-inf and
huge values -- where the mask's strict inequalities and the zero padding decide.
tests/test_lookup_radius_ref.py pins oracle.bilinear_sampler and oracle.coords_grid on the same
inputs to the reference's ATen expression.  Outputs written through the C ABI lie between guard
bands in a buffer filled with a bit pattern no result can equal.  No tolerance anywhere.
"""
import pytest
import torch

import oracle
import sampler_cases as sc
from gpu_guard import check_guarded, guarded, mismatch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_sampler_is_the_oracle_bit_for_bit(ea, case):
    from eraft_amd import _lib
    N, C, h, w, Hg, Wg = case
    img, grid = sc.inputs(case)
    want, wmask = oracle.bilinear_sampler(img, grid, mask=True)
    dimg, dgrid = torch.from_numpy(img).to(DEV), torch.from_numpy(grid).to(DEV)
    with torch.no_grad():
        out, mask = ea.bilinear_sampler(dimg, dgrid, mask=True)
        out2 = ea.bilinear_sampler(dimg, dgrid)
    assert tuple(out.shape) == (N, C, Hg, Wg) and tuple(mask.shape) == (N, Hg, Wg, 1)
    got, gmask = out.cpu().numpy(), mask.cpu().numpy()
    assert oracle.same_bits(got, want), "out: " + str(mismatch(got, want))
    assert oracle.same_bits(gmask, wmask), "mask: " + str(mismatch(gmask.reshape(N, 1, -1), wmask.reshape(N, 1, -1)))
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), "mask=False returns another output"
    # the C ABI into guarded buffers: nothing outside out and mask written, nothing inside left out
    obuf, o = guarded(N * C * Hg * Wg)
    mbuf, m = guarded(N * Hg * Wg)
    _lib.check(_lib.lib().ecorr_bilinear_sampler(dimg.data_ptr(), N, C, h, w, dgrid.data_ptr(), Hg, Wg, o.data_ptr(),
                                                 m.data_ptr(), _lib.stream_of(o)), "bilinear_sampler")
    torch.cuda.synchronize()
    assert oracle.same_bits(check_guarded(obuf, "out").reshape(want.shape), want)
    assert oracle.same_bits(check_guarded(mbuf, "mask").reshape(wmask.shape), wmask)
    obuf, o = guarded(N * C * Hg * Wg)   # no mask asked for
    _lib.check(_lib.lib().ecorr_bilinear_sampler(dimg.data_ptr(), N, C, h, w, dgrid.data_ptr(), Hg, Wg, o.data_ptr(),
                                                 None, _lib.stream_of(o)), "bilinear_sampler")
    torch.cuda.synchronize()
    assert oracle.same_bits(check_guarded(obuf, "out, no mask").reshape(want.shape), want)


@pytest.mark.parametrize("shape", sc.GRID_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_coords_grid_is_the_oracle_bit_for_bit(ea, shape):
    from eraft_amd import _lib
    B, H, W = shape
    want = oracle.coords_grid(B, H, W)
    got = ea.coords_grid(B, H, W, device=DEV)
    assert tuple(got.shape) == (B, 2, H, W) and got.dtype == torch.float32
    assert oracle.same_bits(got.cpu().numpy(), want), mismatch(got.cpu().numpy(), want)
    buf, o = guarded(B * 2 * H * W)
    _lib.check(_lib.lib().ecorr_coords_grid(B, H, W, o.data_ptr(), _lib.stream_of(o)), "coords_grid")
    torch.cuda.synchronize()
    assert oracle.same_bits(check_guarded(buf, "coords_grid").reshape(want.shape), want)
