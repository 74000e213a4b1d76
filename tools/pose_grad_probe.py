#!/usr/bin/env python3
"""What the pose gradients cost, in ONE process through the raw C ABI (modelled on tools/layer_step_probe.py and
tools/bwd_ab_probe.py): alternating rounds, device events, the full-size mesh.

  (a) 'packed'        = fr_decode_3dmm_backward_packed alone
      'packed_pose'   = the same followed by fr_decode_pose_backward            (dense layout: g and vertex_proj [B,3,N])
  (b) 'fused'         = fr_decode_render_backward
      'fused_pose'    = fr_decode_render_backward_pose                          (z-only layout: its z plane + the forward's hand-off)

Beside each difference: the bytes the moment kernel must move (dense 2 x B x 3 x N x 4; z-only B x pitch x 4 + B x 3 x pitch x 4),
the time those bytes take at the measured copy rate of 6.29 TB/s, and the fraction of that rate the difference represents.
Nothing is asserted: the figures are recorded.

--trace: a few calls of each route and nothing else, for a `rocprofv3 --kernel-trace --stats -- python tools/pose_grad_probe.py
--trace` run of its own (per-kernel times).  --out FILE: where the JSON goes besides stdout (default
profiles/decode_pose_backward.json)."""
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

COPY_RATE = 6.29e12   # bytes / s: the measured device-to-device copy figure of the part

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_pose_backward.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("pose_grad_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
H = W = 200
NS, NE = 199, 29


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


out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    N, ntri = net.nvert, int(net.tri.shape[1])
    pitch = L.fr_decode_render_vertex_pitch(N)
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    im = torch.rand((B, H, W, 1), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    net_in, depth_img = torch.empty((B, H, W, 7), **o), torch.empty((B, H, W, 1), **o)
    depth, tri_ind = torch.empty((B, H, W, 1), **o), torch.empty((B, H, W, 1), **o)
    nws = L.fr_render_depth_workspace_bytes(B, N, ntri, H, W)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    nh = L.fr_decode_render_vertex_bytes(B, N)
    hand = torch.empty((nh,), dtype=torch.uint8, device=dev)
    rc = L.fr_decode_rendering_layer_forward(h.ptr(P), h.ptr(net._basis.image), None, h.ptr(net.tri), h.ptr(net.vertex_code),
                                             h.ptr(im), B, N, NS, NE, ntri, H, W, 1, 200.0, h.ptr(hand), nh, h.ptr(net_in),
                                             h.ptr(depth_img), h.ptr(depth), h.ptr(tri_ind), h.ptr(ws), nws, st, 15)
    assert rc == 0, rc
    V = hand.view(torch.float32).view(B, 3, pitch)[:, :, :N].contiguous()     # the dense forward output: the same bits
    g = torch.randn((B, 3, N), **o)
    gd, gi, gn = torch.randn((B, H, W, 1), **o), torch.randn((B, H, W, 1), **o), torch.randn((B, H, W, 7), **o)
    img_t = net._basis.image_t()
    ndw = L.fr_decode_backward_workspace_bytes(B, N, NS, NE)
    dws = torch.empty((ndw,), dtype=torch.uint8, device=dev)
    npw = L.fr_decode_pose_backward_workspace_bytes(B, N)
    pws = torch.empty((npw,), dtype=torch.uint8, device=dev)
    nfw = L.fr_decode_render_backward_workspace_bytes(B, N, NS, NE, H, W)
    fws = torch.empty((nfw,), dtype=torch.uint8, device=dev)
    nqw = L.fr_decode_render_backward_pose_workspace_bytes(B, N, NS, NE, H, W)
    qws = torch.empty((nqw,), dtype=torch.uint8, device=dev)
    gp, gR = torch.empty_like(P), torch.empty((B, 3, 3), **o)

    def packed():
        return L.fr_decode_3dmm_backward_packed(h.ptr(g), h.ptr(P), h.ptr(V), h.ptr(img_t), None, B, N, NS, NE, 200.0, h.ptr(gp),
                                                h.ptr(dws), ndw, st)

    def packed_pose():
        return packed() or L.fr_decode_pose_backward(h.ptr(g), h.ptr(V), h.ptr(P), None, B, N, NS, NE, 200.0, h.ptr(gp), h.ptr(gR),
                                                     h.ptr(pws), npw, st)

    def fused():
        return L.fr_decode_render_backward(h.ptr(gd), h.ptr(gi), h.ptr(gn), h.ptr(im), h.ptr(depth), h.ptr(net.tri), h.ptr(tri_ind),
                                           h.ptr(P), h.ptr(net.mu), h.ptr(img_t), None, B, N, NS, NE, ntri, H, W, 200.0, h.ptr(gp),
                                           h.ptr(fws), nfw, st)

    def fused_pose():
        return L.fr_decode_render_backward_pose(h.ptr(gd), h.ptr(gi), h.ptr(gn), h.ptr(im), h.ptr(depth), h.ptr(net.tri),
                                                h.ptr(tri_ind), h.ptr(P), h.ptr(net.mu), h.ptr(img_t), None, B, N, NS, NE, ntri, H,
                                                W, 200.0, h.ptr(gp), h.ptr(qws), nqw, st, h.ptr(hand), nh, h.ptr(gR))
    routes = {"packed": packed, "packed_pose": packed_pose, "fused": fused, "fused_pose": fused_pose}
    for fn in routes.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    if args.trace:
        for fn in routes.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        continue
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    for name, with_, base, nbytes in (("dense", "packed_pose", "packed", 2 * B * 3 * N * 4),
                                      ("z_only", "fused_pose", "fused", B * pitch * 4 + B * 3 * pitch * 4)):
        diff = round(rec[with_]["median"] - rec[base]["median"], 2)
        copy_us = nbytes / COPY_RATE * 1e6
        rec["pose_" + name] = {"median_difference_us": diff, "margin_us": rec[base]["spread_max_minus_min"],
                               "moment_kernel_bytes": nbytes, "time_at_copy_rate_us": round(copy_us, 2),
                               "fraction_of_copy_rate": round(copy_us / diff, 3) if diff > 0 else None}
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

if not args.trace:
    doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, raw C ABI, full-size "
                   "mesh (N = 53,215); pose_dense = (fr_decode_3dmm_backward_packed + fr_decode_pose_backward) - "
                   "fr_decode_3dmm_backward_packed; pose_z_only = fr_decode_render_backward_pose - fr_decode_render_backward; "
                   "fraction_of_copy_rate = (bytes / 6.29 TB/s) / difference -- the difference holds the moment kernel, the "
                   "finish kernel and two launches" % (args.calls, args.rounds),
           "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
           "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
