#!/usr/bin/env python3
"""What the landmark term costs beside the dense route to the same 68 points, in ONE process (modelled on tools/coverage_probe.py):
alternating rounds, device events, medians of the rounds, the full-size model (N = 53,215, 199 + 29 coefficients), K = 68, 32 and 64
faces.

  'forward'   = fr_landmark_forward with a target                       (raw C ABI: points and sse, one launch)
  'backward'  = fr_landmark_backward from grad_sse, pose_grad 1         (raw C ABI: one launch)
  'operator'  = nets/losses.py::landmark_loss(...).backward()           (the autograd node forward + backward, host time included)
  'dense'     = FaceRecNet.vertices_transform(pose_grad=True) -> index_select at the ids -> the same loss in torch -> backward
                (the dense decode over the 153 MB basis image, the packed decode backward with the pose moment)
  'dense_forward' = the forward half of that route alone
  'basis_build'   = fr_landmark_basis_build (paid once per id list, not per step)

Memory: `image_bytes` is the compact image; `dense_peak_bytes` / `operator_peak_bytes` are torch's peak allocation over one forward +
backward of each route above what was allocated before it (the dense route keeps a [B,3,N] tensor and builds its gradient).

--out FILE: where the JSON goes besides stdout (default profiles/landmark.json)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--landmarks", type=int, default=68)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("landmark_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
losses = importlib.import_module("3dfacerecon_amd.nets.losses")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
K = args.landmarks
idx = synth.landmark_ids(A, K)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / calls * 1e3, 2)


def summary(xs):
    return {"us": xs, "median": round(statistics.median(xs), 2), "spread_max_minus_min": round(max(xs) - min(xs), 2)}


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated(dev) - base)


out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    ns, ne = net.ndim_shape, net.ndim_exp
    lb = net.landmark_basis(idx)
    idx_t = torch.as_tensor(idx, device=dev)
    idx32 = idx_t.to(torch.int32)
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    with torch.no_grad():
        target = (net.landmarks(P, idx)[:, 0:2].transpose(1, 2) + torch.randn((B, K, 2), **o)).contiguous()
    weight = torch.ones((B, K), **o)
    points, sse = torch.empty((B, 3, K), **o), torch.empty((B,), dtype=torch.float64, device=dev)
    gs = torch.full((B,), 1.0 / (B * K), dtype=torch.float64, device=dev)
    gpar = torch.empty((B, 7 + ns + ne), **o)
    image2 = torch.empty_like(lb.image)

    def forward():
        return L.fr_landmark_forward(h.ptr(P), h.ptr(lb.image), lb.nbytes, None, h.ptr(target), h.ptr(weight), 1, B, K, ns, ne, 200.0,
                                     h.ptr(points), h.ptr(sse), st)

    def backward():
        return L.fr_landmark_backward(None, h.ptr(gs), h.ptr(P), h.ptr(lb.image), lb.nbytes, None, h.ptr(target), h.ptr(weight), 1, B, K,
                                      ns, ne, 200.0, h.ptr(gpar), None, 1, st)

    def basis_build():
        return L.fr_landmark_basis_build(h.ptr(net.mu), h.ptr(net.pc_shape), h.ptr(net.pc_exp), h.ptr(idx32), net.nvert, ns, ne, K,
                                         h.ptr(image2), lb.nbytes, st)

    def operator():
        p = P.detach().requires_grad_(True)
        losses.landmark_loss(net, p, idx, target, weight).backward()
        return 0

    def dense_loss(p):
        V = net.vertices_transform(p, pose_grad=True)
        xy = V[:, 0:2].index_select(2, idx_t).transpose(1, 2).double()
        return ((weight.double() * ((xy - target.double()) ** 2).sum(dim=2)).sum(dim=1) / weight.double().sum(dim=1).clamp_min(1.0)).mean()

    def dense():
        p = P.detach().requires_grad_(True)
        dense_loss(p).backward()
        return 0

    def dense_forward():
        with torch.no_grad():
            dense_loss(P)
        return 0
    routes = {"forward": forward, "backward": backward, "operator": operator, "dense": dense, "dense_forward": dense_forward,
              "basis_build": basis_build}
    for fn in routes.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rec["memory"] = {"image_bytes": lb.nbytes, "operator_peak_bytes": peak_of(operator), "dense_peak_bytes": peak_of(dense),
                     "dense_vertex_tensor_bytes": B * 3 * net.nvert * 4, "dense_basis_image_bytes": int(net._basis.image.numel())}
    rec["operator_over_dense"] = round(rec["operator"]["median"] / rec["dense"]["median"], 3)
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds (medians of the rounds; spread = max - min of "
               "the rounds), one process, full-size model (N = 53,215, 199 + 29 coefficients), K = %d landmarks; forward / backward = "
               "fr_landmark_forward (with target) / fr_landmark_backward (from grad_sse, pose_grad 1) through the raw C ABI; operator = "
               "landmark_loss(...).backward(), the autograd node both ways with its host time; dense = vertices_transform(pose_grad=True), "
               "index_select, the same loss in torch, backward; dense_forward = its forward half; basis_build = the one-time gather"
               % (args.calls, args.rounds, K),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
