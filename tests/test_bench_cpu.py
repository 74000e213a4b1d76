"""CPU: bench.py's command line and its --dump-outputs writer (handed a plan-shaped object of CPU tensors: no GPU needed)."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_options():
    p = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in p.stdout, opt


def _plan(B=64, H=200, W=200, N=53215, seed=0):
    g = torch.Generator().manual_seed(seed)
    planes = tuple(torch.rand((B, H, W, c), generator=g) for c in (1, 3, 3, 1))
    vertex = torch.rand((B, 3, N + 13), generator=g)[:, :, :N]     # (a pitched, strided view, as the plans hand it over)
    return types.SimpleNamespace(B=B, device=torch.device("cpu"), vertex_proj=vertex, outputs=lambda: planes)


def test_dump_outputs_is_a_fixed_bounded_sample(tmp_path):
    plan = _plan()
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), plan)
    bench.dump_outputs(str(b), _plan())
    names = ("depth", "texture_image", "normal", "tri_ind")
    assert sorted(os.listdir(str(a))) == sorted([n + ".npy" for n in names + ("vertex_proj", "face_index")])
    assert sum(f.stat().st_size for f in a.iterdir()) <= 64 * 10 ** 6
    faces = np.load(str(a / "face_index.npy"))
    assert faces.dtype == np.float64 and 16 <= len(faces) < plan.B and np.all(np.diff(faces) > 0)
    idx = faces.astype(np.int64)
    for name, t in zip(names + ("vertex_proj",), plan.outputs() + (plan.vertex_proj,)):
        got = np.load(str(a / (name + ".npy")))
        assert got.dtype == np.float32 and np.array_equal(got, t.numpy()[idx]), name
        assert np.array_equal(got, np.load(str(b / (name + ".npy")))), name     # same inputs, same files


def test_dump_outputs_small_batch_is_whole(tmp_path):
    plan = _plan(B=3, H=8, W=9, N=50)
    bench.dump_outputs(str(tmp_path), plan)
    assert np.array_equal(np.load(str(tmp_path / "face_index.npy")), [0, 1, 2])
    assert np.array_equal(np.load(str(tmp_path / "depth.npy")), plan.outputs()[0].numpy())
