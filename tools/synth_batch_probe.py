#!/usr/bin/env python3
"""What a synthetic batch costs, in ONE process (modelled on tools/albedo_lse_probe.py): alternating rounds, device events,
medians, 32 and 64 faces of the full mesh at 200 x 200.

  'params'        = fr_synth_params
  'texture'       = fr_synth_texture
  'shade'         = fr_synth_shade on the planes of the batch's own render
  'decode_render' = DecodeRenderPlan.step() with the per-face texture (not new; for scale)
  'batch'         = the whole sequence of pipeline.SynthBatches on one stream: params, texture, decode + render, shade, clamp
  'copy'          = a device-to-device copy of 512 MiB: the copy rate of THIS run, which prices the bytes below
  'host_route'    = WALL time per batch of what the parent's loop did for its data: utils.synth.sample_params_batch, torch.rand
                    on the CPU generator, and the two copies to the device (synchronised)
  'in_flight'     = WALL time per SynthBatches.next() in a loop that does nothing else (two slots; the generation's own rate)

Beside them the bytes each new kernel must move: params writes (7 + ns + ne + 4 + K) floats per face; texture reads pc_tex and
mu_tex once (3 N (K + 1) floats; the other faces' reads come out of cache) and alpha, and writes 3 N floats per face; shade reads
tri_ind (4 B) per pixel and 24 B more per covered one, and writes 8 B per pixel.

--train-steps N (default 5; 0 = skip): also runs examples/coarse_loop.py --train --batch B with and without --synth-data as child
processes and records their ms_per_step.
--out FILE: where the JSON goes besides stdout (default profiles/synth_batch.json)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[32, 64])
ap.add_argument("--size", type=int, default=200)
ap.add_argument("--train-steps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_batch.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("synth_batch_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
pipe = importlib.import_module("3dfacerecon_amd.pipeline")
L = h.lib()
dev = torch.device("cuda:0")
S = args.size
COPY_BYTES = 512 << 20


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / calls * 1e3, 2)


def wall(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / calls * 1e6, 2)


def summary(xs):
    return {"us": xs, "median": round(statistics.median(xs), 2), "spread_max_minus_min": round(max(xs) - min(xs), 2)}


def train_step_ms(B, flag):
    if args.train_steps <= 0:
        return "unmeasured"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "coarse_loop.py"), "--train", "--batch", str(B), "--im-size", str(S),
           "--steps", str(args.train_steps), "--warmup", "2"] + flag
    try:
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        return "unmeasured (the program ran into its time limit)"
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or len(lines) != 1:
        return "unmeasured (the program ended with %d)" % p.returncode
    return round(json.loads(lines[0])["ms_per_step"], 2)


A = synth.make_assets()
src, dst = (torch.empty((COPY_BYTES,), dtype=torch.uint8, device=dev) for _ in range(2))
out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=dev)
    K, N, ns, ne = int(net.pc_tex.shape[1]), net.nvert, net.ndim_shape, net.ndim_exp
    f32 = dict(dtype=torch.float32, device=dev)
    tex = torch.empty((B, 3, N), **f32)
    plan = pipe.DecodeRenderPlan(net, B, S, S, texture=tex)
    light, alpha = torch.empty((B, 4), **f32), torch.empty((B, K), **f32)
    im, mask, depth = (torch.empty((B, S, S, 1), **f32) for _ in range(3))
    face = [0]

    def params():
        ops.synth_params(1, face[0], B, ns, ne, K, S, out=(plan.params, light, alpha))
        face[0] += B

    def texture():
        ops.synth_texture(net.mu_tex, net.pc_tex, alpha, out=tex)

    def decode_render():
        plan.step()

    def shade():
        ops.synth_shade(plan.texture_image, plan.normal, plan.tri_ind, light, out=(im, mask))

    def batch():
        params()
        texture()
        decode_render()
        shade()
        torch.clamp_min(plan.depth, 1e-6, out=depth)

    def copy():
        dst.copy_(src)

    g = torch.Generator(device="cpu").manual_seed(100)
    seed = [200]

    def host_route():
        seed[0] += 1
        i = torch.rand((B, S, S, 1), generator=g).to(dev)
        lab = torch.as_tensor(synth.sample_params_batch(B, im_size=S, n_shape=ns, n_exp=ne, beta=0.7, seed=seed[0]), device=dev)
        return i, lab

    flights = pipe.SynthBatches(net, B, 2, slots=2)
    routes = {"params": params, "texture": texture, "decode_render": decode_render, "shade": shade, "batch": batch, "copy": copy}
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    coverage = float((plan.tri_ind >= 0).float().mean())
    res = {k: [] for k in routes}
    res["host_route"], res["in_flight"] = [], []
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
        res["host_route"].append(wall(host_route, 5))
        res["in_flight"].append(wall(flights.next, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rate = 2 * COPY_BYTES / (rec["copy"]["median"] * 1e-6)
    rec["copy_rate_bytes_per_s"] = round(rate, -9)
    rec["coverage"] = round(coverage, 3)
    npix = S * S
    must = {"params": B * (7 + ns + ne + 4 + K) * 4,
            "texture": 3 * N * (K + 1) * 4 + B * K * 4 + B * 3 * N * 4,
            "shade": int(B * npix * (4 + 24 * coverage + 8) + B * 16)}
    for k, v in must.items():
        rec[k + "_vs_bytes"] = {"must_move": v, "time_at_copy_rate_us": round(v / rate * 1e6, 2),
                                "fraction_of_copy_rate": round(v / rate * 1e6 / rec[k]["median"], 3)}
    rec["host_route_over_batch"] = round(rec["host_route"]["median"] / rec["batch"]["median"], 1)
    del flights, plan
    torch.cuda.synchronize()
    rec["train_ms_per_step"] = {"parent_route": train_step_ms(B, []), "synth_data": train_step_ms(B, ["--synth-data"])}
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)
    del net

doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, full mesh, %d x %d; "
               "host_route and in_flight are WALL us per batch (synchronised; 5 and %d calls per figure); copy = a 512 MiB "
               "device-to-device copy, copy_rate = 2 x 512 MiB / its median; must_move = the bytes any scheme moves, "
               "fraction_of_copy_rate = (must_move / copy_rate) / time; train_ms_per_step = examples/coarse_loop.py --train "
               "--batch B --steps %d --warmup 2, one child process each" % (args.calls, args.rounds, S, S, args.calls,
                                                                            args.train_steps),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
