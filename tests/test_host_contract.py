"""The argument contract of every public entry that takes tensors, where no HIP device is needed: a
non-tensor and a CPU tensor each raise before any library call, with a fixed exception type and a
fixed text.  The texts are literals: a change of wording in the host layer has to change this file."""
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import eraft_amd

NOT_TENSOR = "{} must be a torch.Tensor"
ON_CPU = "{} is on cpu: eraft_amd runs only on HIP devices (no CPU path)"
VOXEL = "events['{}'] must be a float32 HIP tensor (no CPU path)"

F4 = torch.zeros(1, 4, 4, 4)             # fmap / img / flow_in with 4 channels
FLOW = torch.zeros(1, 2, 4, 4)
MASK = torch.zeros(1, 576, 4, 4)
GRID = torch.zeros(1, 4, 4, 2)
PTS = torch.zeros(3, 5)
PNG = torch.zeros(4, 4, 3, dtype=torch.uint16)
EV = torch.zeros(5)


def _events(**bad):
    ev = {k: EV for k in "ptxy"}
    ev.update(bad)
    return ev


VG = eraft_amd.VoxelGrid((3, 4, 4), normalize=True)

# (id, call, exception type, full message)
ROWS = [
    ("corrblock-fmap1-list", lambda: eraft_amd.CorrBlock([1.0], F4), TypeError, NOT_TENSOR.format("fmap1")),
    ("corrblock-fmap1-cpu", lambda: eraft_amd.CorrBlock(F4, F4), RuntimeError, ON_CPU.format("fmap1")),
    ("corrblock-corr-list", lambda: eraft_amd.CorrBlock.corr([1.0], F4), TypeError, NOT_TENSOR.format("fmap1")),
    ("corrblock-corr-cpu", lambda: eraft_amd.CorrBlock.corr(F4, F4), RuntimeError, ON_CPU.format("fmap1")),
    ("sampler-img-list", lambda: eraft_amd.bilinear_sampler([1.0], GRID), TypeError, NOT_TENSOR.format("img")),
    ("sampler-img-cpu", lambda: eraft_amd.bilinear_sampler(F4, GRID), RuntimeError, ON_CPU.format("img")),
    ("upsample-flow-none", lambda: eraft_amd.upsample_flow(None, MASK), TypeError, NOT_TENSOR.format("flow")),
    ("upsample-flow-cpu", lambda: eraft_amd.upsample_flow(FLOW, MASK), RuntimeError, ON_CPU.format("flow")),
    ("png16-flow-ndarray", lambda: eraft_amd.flow_to_png16(FLOW.numpy()), TypeError, NOT_TENSOR.format("flow")),
    ("png16-flow-cpu", lambda: eraft_amd.flow_to_png16(FLOW), RuntimeError, ON_CPU.format("flow")),
    ("from16-ndarray", lambda: eraft_amd.flow_16bit_to_float(PNG.numpy()), TypeError,
     NOT_TENSOR.format("flow_16bit")),
    ("from16-cpu", lambda: eraft_amd.flow_16bit_to_float(PNG), RuntimeError, ON_CPU.format("flow_16bit")),
    ("grid-sample-list", lambda: eraft_amd.grid_sample_values([[0.0]] * 3, 4, 4), TypeError,
     NOT_TENSOR.format("input")),
    ("grid-sample-cpu", lambda: eraft_amd.grid_sample_values(PTS, 4, 4), RuntimeError, ON_CPU.format("input")),
    ("splat-none", lambda: eraft_amd.forward_interpolate_pytorch(None), TypeError, NOT_TENSOR.format("flow_in")),
    ("splat-cpu", lambda: eraft_amd.forward_interpolate_pytorch(FLOW), RuntimeError, ON_CPU.format("flow_in")),
    ("voxel-p-ndarray", lambda: VG.convert(_events(p=EV.numpy())), RuntimeError, VOXEL.format("p")),
    ("voxel-p-cpu", lambda: VG.convert(_events()), RuntimeError, VOXEL.format("p")),
]


@pytest.mark.parametrize("call,exc,msg", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_rejected_before_any_launch(call, exc, msg):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc
    assert str(e.value) == msg


def test_from16_asserts_before_the_device_check():
    """flow_16bit_to_float asserts dtype and shape as the reference does, before it looks at the device."""
    with pytest.raises(AssertionError):
        eraft_amd.flow_16bit_to_float(torch.zeros(4, 4, 3))
    with pytest.raises(AssertionError):
        eraft_amd.flow_16bit_to_float(torch.zeros(4, 4, 2, dtype=torch.uint16))
