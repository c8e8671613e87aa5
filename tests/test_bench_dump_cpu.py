"""bench.py --dump-outputs: the file writer on host tensors (no GPU): float32 / float64 .npy files, shapes kept
below the element cap, a fixed seeded sample above it, identical files from identical outputs, and the byte
limit respected by lowering the cap."""
import os

import numpy as np
import torch

import bench


def _outputs():
    g = torch.Generator().manual_seed(3)
    big = torch.randn(300, 70, generator=g)
    strided = torch.randn(40, 16, generator=g)[:, :10]  # a padded-row view, as a slab hands out
    return {"train_loss": np.asarray([1.5], dtype=np.float64), "small": torch.randn(7, 5, generator=g),
            "strided": strided, "big": big}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_files(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP", 1000)
    outs = _outputs()
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), _outputs())
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["big", "small", "strided", "train_loss"]
    assert a["train_loss"].dtype == np.float64 and a["train_loss"][0] == 1.5
    for k in ("small", "strided"):
        assert a[k].dtype == np.float32
        assert np.array_equal(a[k], outs[k].numpy())
    # above the cap: 1000 distinct elements of the flattened array in their order, the same ones every run
    assert a["big"].dtype == np.float32 and a["big"].shape == (1000,)
    flat = outs["big"].reshape(-1).numpy()
    idx = np.sort(np.random.default_rng(20240229).choice(flat.size, 1000, replace=False))
    assert np.array_equal(a["big"], flat[idx])
    for k in a:
        assert np.array_equal(a[k], b[k])


def test_dump_outputs_byte_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP", 4096)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 3 * 4 * 1024)
    outs = {f"p{i}": torch.arange(5000, dtype=torch.float32) + i for i in range(4)}
    bench.dump_outputs(str(tmp_path), outs)
    got = _load(tmp_path)
    assert sum(v.nbytes for v in got.values()) <= 3 * 4 * 1024
    assert all(v.shape == (512,) for v in got.values())  # the cap halved until four arrays fit: 4096 -> 512
