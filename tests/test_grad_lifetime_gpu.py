"""What the autograd graph of a live block keeps alive (e-raft_amd/_grad.py): not the pyramid, and no
reference cycle.  torch.cuda.memory_allocated() counts live blocks of the caching allocator, so it
falls the moment the last reference to a tensor goes -- with the garbage collector off, only if no
cycle holds it.  B = 1, D = 8, 16 x 16, two levels, r = 1.
"""
import gc

import pytest
import torch

import prng

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, D, H, W, LEVELS, RADIUS = 1, 8, 16, 16, 2, 1


@pytest.fixture
def no_gc():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    yield
    if was:
        gc.enable()


def _inputs():
    f1 = torch.from_numpy(prng.normal(31, (B, D, H, W))).to(DEV).requires_grad_(True)
    f2 = torch.from_numpy(prng.normal(32, (B, D, H, W))).to(DEV).requires_grad_(True)
    coords = torch.from_numpy(prng.coords_with_flow(33, B, H, W, 2.0)).to(DEV)
    go = torch.from_numpy(prng.normal(34, (B, LEVELS * (2 * RADIUS + 1) ** 2, H, W))).to(DEV)
    return f1, f2, coords, go


def test_corr_block_graph_keeps_no_pyramid_and_no_cycle(no_gc):
    import eraft_amd
    torch.cuda.synchronize()
    start = torch.cuda.memory_allocated()
    f1, f2, coords, go = _inputs()
    blk = eraft_amd.CorrBlock(f1, f2, num_levels=LEVELS, radius=RADIUS, differentiable=True)
    pyramid_bytes = blk._pyramid.numel() * blk._pyramid.element_size()
    assert pyramid_bytes >= (B * H * W) * (H * W) * 4
    out = blk(coords)
    assert out.requires_grad
    held = torch.cuda.memory_allocated()
    del blk   # the lookup's output and its graph are still held
    freed = held - torch.cuda.memory_allocated()
    print(f"pyramid {pyramid_bytes} bytes; deleting the block freed {freed}")
    assert freed >= pyramid_bytes
    (out * go).sum().backward()
    torch.cuda.synchronize()
    assert f1.grad is not None and f2.grad is not None
    del out, f1, f2, coords, go
    assert torch.cuda.memory_allocated() == start


def test_alternate_block_graph_has_no_cycle(no_gc):
    import eraft_amd
    torch.cuda.synchronize()
    start = torch.cuda.memory_allocated()
    f1, f2, coords, go = _inputs()
    blk = eraft_amd.AlternateCorrBlock(f1, f2, num_levels=LEVELS, radius=RADIUS, trainable=True)
    out = blk(coords)
    assert out.requires_grad
    (out * go).sum().backward()
    torch.cuda.synchronize()
    assert f1.grad is not None and f2.grad is not None
    del blk, out, f1, f2, coords, go
    assert torch.cuda.memory_allocated() == start
