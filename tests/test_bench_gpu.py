"""bench.py run as the driver runs it -- as a program, its ONE JSON line parsed -- on the GPU box.

The N > 1 legs walk the multi-rank control flow (partition, barrier + synchronize brackets, MAX over ranks, the parity gate
on every rank, the `dist` block) with two ranks that SHARE the one GPU of the test box over gloo: RCCL refuses two ranks on
one device, so the collective library itself is the one thing these legs cannot cover; the line says `backend: gloo`."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = ["--steps", "3", "--warmup", "1", "--repeats", "2"]
FULL = SHORT + ["--full"]   # (everything beyond the headline: legs, gates, per-kernel figures, CPU baseline)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _line(cmd):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]          # ONE line, from rank 0
    # ... and nothing else on stdout: RCCL's version banner, MIOpen's chatter etc. go to stderr (bench.py points fd 1 there)
    assert [l for l in p.stdout.splitlines() if l.strip()] == lines, p.stdout[:2000]
    return json.loads(lines[0])


def test_bench_line_one_gpu():
    d = _line([sys.executable, "bench.py"] + FULL + ["--cpu-faces", "8"])
    assert d["metric"].startswith("faces/sec") and d["unit"] == "faces/s" and d["n_gpus"] == 1 and d["steps"] == 3
    assert d["value"] > 1e4 and abs(d["value"] - 64 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None and d["higher_is_better"] is True
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] < 1
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    assert d["parity"]["ok"] and d["parity"]["faces"] == 64 and d["parity"]["mismatching_planes"] == 0
    assert d["ops_surface"]["outputs_identical_to_plan"] and d["ops_surface_faces_per_s"] > 1e4
    assert d["dist"]["world_size"] == 1 and d["config"]["faces_per_step_all_gpus"] == 64
    # the default route keeps two independent batches in flight (two plans, two streams); the serial plan is timed beside it
    assert d["route"].startswith("inflight") and {"decode", "raster_emit", "resolve_write"} <= set(d["kernels"])
    assert d["config"]["batches_in_flight"] == 2 and d["parity"]["batches_checked"] == 2 and d["parity"]["faces_checked"] == 128
    assert d["serial_plan_faces_per_s"] > 1e4 and d["serial_plan"]["timed_route_vs_serial"] > 0.8
    assert all(d["kernels"][k]["in_region_avg_ms"] > 0 for k in ("decode", "raster_emit", "resolve_write"))
    assert d["dist"]["distinct_devices"] and d["dist"]["devices"][0]["name"] and d["dist"]["devices"][0]["id"]
    assert all("avg_ms_is" in d["kernels"][k] for k in ("decode", "raster_emit", "resolve_write"))
    assert "which_side_binds" in d["kernels"]["decode"]
    # round 5: what the headline means, one batch's latency, the clock the part held, the one-batch-at-a-time figure, and the
    # same route with the Q30 decode (ten digit products), gated against ITS oracle, beside `value`
    assert d["value_route"] == "inflight" and "THROUGHPUT" in d["value_meaning"]
    assert d["per_batch_latency_ms"] > d["ms_per_step"]          # two in flight: a batch takes longer than the interval
    assert abs(d["config"]["value_one_batch_at_a_time"] - d["serial_plan_faces_per_s"]) < 1e-6 * d["value"]
    for k in ("after_timed_blocks", "after_serial_leg"):
        assert 1.0 < d["clock_GHz_held"][k]["median"] < 2.6
    assert "vector_pipe" not in d and "pipeline_hbm" not in d and "north_star_40pct_of_8TBs" not in d
    rec = d["config"]["caller_configs_recorded"]     # configs 3-5 ride along as RECORDED lines, marked as such
    assert "not measured by this run" in rec["source"] and rec["config3_fwd"]["faces_per_gpu"] == 32 and rec["config4_train_shard"]["ms_per_step"] > 100
    _check_roofline_is_self_contained(d)
    q = d["q30_inflight"]
    assert q["parity"]["ok"] and q["parity"]["mismatching_planes"] == 0 and q["parity"]["faces_checked"] == 16
    assert d["q30_inflight_faces_per_s"] > 1e4 and abs(q["vs_value"] - d["q30_inflight_faces_per_s"] / d["value"]) < 1e-9
    assert "4 digit-product levels" in q["decode_arith"] and d["config"]["decode_arith"].startswith("f32")
    # ... and the one-GPU box's contact with RCCL: a one-rank communicator on this GPU and one all-reduce through it
    st = d["dist"]["rccl_selftest"]
    assert st["ok"], st
    assert st["describe"]["backend"] == "nccl" and st["rccl_version"] and st["allreduce"]["sum_correct"] and st["allreduce"]["bytes"] == 302000000


def _check_roofline_is_self_contained(d, q30=True):
    """the driver's record keeps `config`, `roofline` and `cpu_baseline` -- every fraction the line
    claims must be recomputable from those alone."""
    r = d["roofline"]
    st = r["step"]
    per_gpu = d["value"] / d["n_gpus"]
    assert abs(st["faces_per_s_per_gpu"] - per_gpu) < 1e-6 * per_gpu and abs(st["ms_per_step"] - d["ms_per_step"]) < 1e-12
    assert abs(st["achieved_GBs"] - st["algorithmic_bytes_per_face"] * per_gpu / 1e9) < 1e-6 * st["achieved_GBs"]
    assert abs(st["frac_of_8TBs"] - st["achieved_GBs"] / 8000.0) < 1e-12 and st["peak_GBs"] == 8000.0
    assert 4.8e6 < st["algorithmic_bytes_per_face"] < 4.95e6 or d["config"]["faces_per_gpu_rank0"] != 64
    ns = st["north_star_40pct"]
    assert abs(ns["needs_faces_per_s_per_gpu"] - 0.4 * 8e12 / st["algorithmic_bytes_per_face"]) < 1.0
    assert ns["value_passes"] == (per_gpu >= ns["needs_faces_per_s_per_gpu"])
    one = st["one_batch_at_a_time"]
    if d["value_route"] == "inflight" and "serial_plan" in d:
        assert abs(one["faces_per_s_per_gpu"] * d["n_gpus"] - d["config"]["value_one_batch_at_a_time"]) < 1e-6 * d["value"]
        assert abs(one["frac_of_8TBs"] - st["algorithmic_bytes_per_face"] * one["faces_per_s_per_gpu"] / 8e12) < 1e-12
        assert ns["one_batch_at_a_time_passes"] == (one["faces_per_s_per_gpu"] >= ns["needs_faces_per_s_per_gpu"])
    assert 1.0 < r["clock_GHz_held"]["after_timed_blocks"] < 2.6
    for name in ("decode", "raster_emit", "resolve_write"):
        k = r["kernels"][name]
        assert abs(k["frac"] - k["achieved"] / k["peak"]) < 1e-12 and k["avg_ms"] > 0
        work = k.get("algorithmic_flop_per_launch") if k["unit"] == "TFLOP/s" else k["algorithmic_bytes_per_launch"]
        assert abs(k["achieved"] - work / (k["avg_ms"] * 1e-3) / (1e12 if k["unit"] == "TFLOP/s" else 1e9)) < 1e-6 * k["achieved"]
    if q30:
        q = r["q30"]
        assert q["levels"] == 4 and q["parity_ok"] is True and q["faces_checked"] == 16
        assert abs(q["frac_of_8TBs"] - st["algorithmic_bytes_per_face"] * q["faces_per_s_per_gpu"] / 8e12) < 1e-12
        assert abs(q["faces_per_s_per_gpu"] * d["n_gpus"] - d["q30_inflight_faces_per_s"]) < 1e-6 * d["value"]
        assert ns["q30_passes"] == (q["faces_per_s_per_gpu"] >= ns["needs_faces_per_s_per_gpu"])
    else:
        assert r["q30"] is None and ns["q30_passes"] is None


def test_bench_q30_leg_failure_does_not_take_the_line_down():
    """the Q30 leg is auxiliary -- an exception in it is reported inside q30_inflight / roofline.q30 and the f32
    line (already measured, still gated) is printed all the same.  FR_BENCH_Q30_FAULT makes the leg raise on purpose."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", FR_BENCH_Q30_FAULT="1")
    p = subprocess.run([sys.executable, "bench.py"] + FULL + ["--cpu-faces", "0", "--no-ops-surface", "--no-rccl-selftest", "--parity-faces", "2"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert d["parity"]["ok"] and d["value"] > 1e4
    assert "error" in d["q30_inflight"] and "q30_inflight_faces_per_s" not in d
    assert "error" in d["roofline"]["q30"] and d["roofline"]["step"]["north_star_40pct"]["q30_passes"] is None


def test_bench_line_serial_route():
    """--route serial: one plan, one stream, one batch at a time."""
    d = _line([sys.executable, "bench.py"] + FULL + ["--cpu-faces", "0", "--route", "serial", "--no-ops-surface"])
    assert d["route"].startswith("serial") and d["config"]["batches_in_flight"] == 1 and d["parity"]["ok"]
    assert "serial_plan" not in d and {"decode", "raster_emit", "resolve_write"} <= set(d["kernels"])
    _check_roofline_is_self_contained(d, q30=False)
    assert d["roofline"]["step"]["one_batch_at_a_time"]["ms_per_step"] == pytest.approx(d["ms_per_step"], rel=1e-9)


@pytest.mark.parametrize("scaling,global_faces,local_faces", [("weak", 128, 64), ("strong", 64, 32)])
def test_bench_two_ranks_walk_the_multi_rank_flow(scaling, global_faces, local_faces):
    d = _line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2", "--dist-backend", "gloo",
               "--scaling", scaling, "--cpu-faces", "4", "--no-ops-surface", "--q30-levels", "0"] + FULL)
    assert d["n_gpus"] == 2 and d["scaling"] == scaling
    assert d["dist"]["backend"] == "gloo" and d["dist"]["world_size"] == 2 and d["dist"]["ranks_reporting"] == 2
    assert len(d["dist"]["per_rank_ms_per_step"]) == 2 and all(t > 0 for t in d["dist"]["per_rank_ms_per_step"])
    assert d["config"]["faces_per_step_all_gpus"] == global_faces and d["config"]["faces_per_gpu_rank0"] == local_faces
    # value is the whole job: all ranks' faces over the slowest rank's time
    assert abs(d["value"] - global_faces * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert abs(d["ms_per_step"] - max(d["dist"]["per_rank_ms_per_step"])) < 1e-9     # MAX over ranks of the reported block
    p = d["parity"]
    assert p["ok"] and p["faces_all_ranks"] == global_faces and p["mismatching_planes_all_ranks"] == 0
    # an N > 1 line is complete -- rank 0 times the CPU baseline at every N, and the roofline object
    # carries the step per GPU
    c = d["cpu_baseline"]
    assert c is not None and c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and d["speedup_vs_cpu"]["n_gpus"] == 2
    r = d["roofline"]
    assert r is not None and 0 < r["frac"] < 1 and r["step"]["faces_per_step_per_gpu"] == local_faces
    assert abs(r["step"]["faces_per_s_per_gpu"] * 2 - d["value"]) < 1e-6 * d["value"]
    assert d["dist"]["rccl_version"] is None and d["dist"]["backend"] == "gloo"
    # which device every rank ran on (here: both on the box's one GPU, which only gloo tolerates), and the all-reduce preflight
    assert len(d["dist"]["devices"]) == 2 and d["dist"]["distinct_devices"] is False and d["dist"]["rccl_version"] is None
    ar = d["dist"]["allreduce_preflight"]
    assert ar["sum_correct"] and ar["bytes"] == 4000000 and ar["ms"] > 0
    assert ("strong_scaling_prediction" in d["dist"]) == (scaling == "strong")
    if scaling == "strong":   # (read from the committed shard timings, not literals)
        sp = d["dist"]["strong_scaling_prediction"]
        assert sp["predicted_speedup_vs_1_gpu"]["8"] > 1.5 and sp["us_per_step_at_faces_per_gpu"]["64"] > 50


def test_bench_plain_line_and_outputs(tmp_path, oracle, synth):
    """A plain run (no --full): exactly K timed steps in one block, the headline fields and nothing measured beside them, and
    --dump-outputs: the planes and vertices of the slot that ran the LAST timed step, for a seeded sample of its faces --
    the oracle rasteriser on those vertices gives those planes bit for bit, and the vertices are that slot's batch decoded."""
    out = tmp_path / "outs"
    K = 7
    d = _line([sys.executable, "bench.py", "--gpus", "1", "--steps", str(K), "--warmup", "2", "--dump-outputs", str(out)])
    assert d["metric"].startswith("faces/sec") and d["unit"] == "faces/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == K and d["warmup"] == 2 and d["warmup_steps_run"] >= 2 and d["full"] is False
    assert d["repeats"] == 1 and len(d["blocks_ms_per_step"]) == 1 and d["value_is"] == "one timed block of K steps"
    assert d["value"] > 1e4 and abs(d["value"] - 64 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert abs(d["blocks_ms_per_step"][0] - d["ms_per_step"]) < 1e-4
    for k in ("cpu_baseline", "parity", "kernels", "roofline", "serial_plan", "q30_inflight", "ops_surface", "clock_GHz_held"):
        assert k not in d, k
    assert "rccl_selftest" not in d["dist"] and d["route"].startswith("inflight")
    names = ("depth", "texture_image", "normal", "tri_ind")
    files = {f.name[:-4]: np.load(str(f)) for f in out.iterdir()}
    assert set(files) == set(names) | {"face_index", "vertex_proj"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 * 10 ** 6
    faces = files["face_index"].astype(np.int64)
    n = len(faces)
    assert 16 <= n <= 64 and np.all(np.diff(faces) > 0)
    assert files["depth"].shape == (n, 200, 200, 1) and files["texture_image"].shape == (n, 200, 200, 3)
    A = synth.make_assets()
    assert files["vertex_proj"].shape == (n, 3, A["mu"].size // 3)
    V = files["vertex_proj"][:2]
    want = oracle.render_depth(V, A["tri"], A["vertex"][None], 200, 200)
    for name, w in zip(names, want):
        assert np.array_equal(files[name][:2], w, equal_nan=True), name
    assert (files["tri_ind"] >= 0).mean() > 0.05
    # step k of the run goes to slot k mod 2 (warm-up included); slot i holds the sampler's draw seed 3456 + 1000 i
    slot = (d["warmup_steps_run"] + K - 1) % 2
    P = synth.sample_params_batch(64, im_size=200, beta=0.7, seed=3456 + 1000 * slot)[faces[:2]]
    Vo = oracle.decode_3dmm(P, A["mu"], A["pc_shape"], A["pc_exp"], 200.0, R=oracle.rotation_matrix_batch(P[:, :3]))
    assert np.allclose(V, Vo, rtol=1e-6, atol=1e-4)   # (in-kernel fp64 rotation: a few ulp, tests/test_decode_gpu.py)
