"""CPU tests of bench.py --dump-outputs: what lands in DIR (names, dtypes, the 64 MB bound) and that a sampled array is sampled at the
same positions every time, so that two builds' dumps compare element for element."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("dwg_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_snapshot_walks_nested_outputs_and_keeps_float32_or_float64():
    b = _bench()
    loss = torch.tensor([1.5])
    render = {"image": torch.rand(1, 8, 8, 3), "radii": torch.arange(5, dtype=torch.int32), "visible": torch.tensor([True, False]),
              "note": "not an array"}
    guide = {"latents": torch.randn(2, 4, dtype=torch.float64), "gradients": None, "timestep": torch.tensor([500])}
    snap = b.snapshot_outputs(dict(zip(("loss", "render", "guidance"), (loss, [render], guide, "a prompt name"))))
    assert sorted(snap) == ["guidance.latents", "guidance.timestep", "loss", "render.0.image", "render.0.radii", "render.0.visible"]
    assert snap["loss"].dtype == np.float32 and snap["render.0.image"].shape == (1, 8, 8, 3)
    assert snap["guidance.latents"].dtype == np.float64 and snap["guidance.timestep"].dtype == np.float64
    assert snap["render.0.radii"].tolist() == [0, 1, 2, 3, 4] and snap["render.0.visible"].tolist() == [1.0, 0.0]


def test_dump_is_bounded_and_samples_at_fixed_positions(tmp_path):
    b = _bench()
    big = np.arange(3 * b.DUMP_SAMPLE, dtype=np.float32)
    arrays = {"params": big, "grads": -big, "image": np.ones((4, 4, 3), np.float32)}
    arrays.update(("view.%02d" % i, big) for i in range(16))           # 18 full-size samples would be 72 MB: the sample size is halved
    s1 = b.dump_outputs(arrays, str(tmp_path / "a"))
    s2 = b.dump_outputs(dict(arrays), str(tmp_path / "b"))
    assert s1 == dict(s2, dir=s1["dir"]) and s1["arrays"] == 19 and s1["sample_elements"] == b.DUMP_SAMPLE // 2
    assert s1["bytes"] <= b.DUMP_LIMIT_BYTES and "image" not in s1["sampled"] and len(s1["sampled"]) == 18
    files = sorted(os.listdir(tmp_path / "a"))
    assert len(files) == 19 and "params.npy" in files and files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= b.DUMP_LIMIT_BYTES + 19 * 256       # + the .npy headers
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
    p = np.load(tmp_path / "a" / "params.npy")
    assert p.size == s1["sample_elements"] and np.all(np.diff(p) > 0)          # distinct positions, in order
    assert np.array_equal(np.load(tmp_path / "a" / "grads.npy"), -p)             # same shape -> same positions
    assert np.load(tmp_path / "a" / "image.npy").shape == (4, 4, 3)             # small arrays are written whole
