"""CPU: bench.py --dump-outputs' writer -- float32 / float64 files under the 64 MB cap, the same seeded sample every time."""
import os

import numpy as np
import torch

import bench


def test_dump_writes_float32_and_float64(tmp_path):
    bench.dump_outputs(str(tmp_path), {"params": torch.arange(6, dtype=torch.float32).view(2, 3),
                                       "step": torch.tensor([7], dtype=torch.int32), "loss": np.float64(1.5)})
    p, s, l = (np.load(os.path.join(str(tmp_path), f"{n}.npy")) for n in ("params", "step", "loss"))
    assert p.dtype == np.float32 and p.shape == (2, 3) and np.array_equal(p.reshape(-1), np.arange(6))
    assert s.dtype == np.float64 and s.tolist() == [7.0]
    assert l.dtype == np.float64 and float(l) == 1.5


def test_dump_samples_the_same_elements_past_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4096)
    big = torch.randn(3000, generator=torch.Generator().manual_seed(0))
    small = torch.ones(10)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(str(tmp_path / "a" / "big.npy")), np.load(str(tmp_path / "b" / "big.npy"))
    assert a.nbytes <= 2048 and np.array_equal(a, b)
    assert np.isin(a, big.numpy()).all()
    assert np.array_equal(np.load(str(tmp_path / "a" / "small.npy")), small.numpy())
    assert sum(np.load(str(tmp_path / "a" / f)).nbytes for f in os.listdir(str(tmp_path / "a"))) <= 4096
