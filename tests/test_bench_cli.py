"""bench.py's --gpus contract, the part that runs without a GPU: a launcher whose WORLD_SIZE differs
from --gpus N is refused before any device call; the N-rank self-launch itself
is exercised on the GPU box (tests/test_batch_shard_gpu.py, launcher=bench_itself)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=120)


def test_world_size_mismatch_refused():
    r = _run(["--gpus", "2"], WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0
    assert "WORLD_SIZE=3" in r.stderr
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())


def test_zero_gpus_refused():
    r = _run(["--gpus", "0"])
    assert r.returncode != 0 and "--gpus 0" in r.stderr


def test_dump_outputs_sample_is_fixed(tmp_path):
    """--dump-outputs: an array larger than its share is sampled at the same sorted flat indices in
    every run (a seeded host generator), a smaller one is written whole; float32 files."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(1_500_000, dtype=torch.float32)   # its value is its flat index
    outs = [big, big + 0.5, torch.arange(1000, dtype=torch.float32).reshape(10, 100)]
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["lookup_00.npy", "lookup_01.npy", "lookup_02.npy"]
    a = [np.load(tmp_path / "a" / n) for n in names]
    b = [np.load(tmp_path / "b" / n) for n in names]
    for x, y in zip(a, b):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    assert a[0].shape == (1 << 20,) and np.all(np.diff(a[0]) >= 0) and a[0].max() < 1_500_000
    assert len(np.unique(a[0])) > 500_000   # spread over the array, not one corner of it
    assert np.array_equal(a[2], np.arange(1000, dtype=np.float32))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= bench.DUMP_BYTES
