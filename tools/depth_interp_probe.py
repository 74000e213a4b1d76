#!/usr/bin/env python3
"""What the interpolated depth costs, in ONE process through the raw C ABI (modelled on tools/normal_grad_probe.py): alternating
rounds, device events, medians of the rounds, the full-size mesh at 200 x 200, 32 and 64 faces.

  'forward'       = fr_depth_interp_forward                                              (the post-pass over tri_ind)
  'backward'      = fr_depth_interp_backward, accumulate 0, dense [B,H,W,1] gradient     (x, y and z rows)
  'flat_backward' = fr_render_depth_backward_ws on the same tri_ind and gradient          (the z-only backward it replaces)
  'normal_raw'    = fr_render_normal_backward, mode 0, accumulate 0, dense [B,H,W,3] gradient, dense vertex rows: the same record
                    planes through the same owners, three gradient floats per pixel instead of one
  'copy'          = a device-to-device copy of 512 MiB: the copy rate of THIS run, which prices the bytes below

Beside each direction: the bytes it must move -- forward: tri_ind read and depth written (8 B per pixel), the id gathers (12 B) and
the vertex gathers (36 B) of the covered pixels; backward: depth_grad and tri_ind read (8 B per pixel), the same gathers, three rows
written (12 B per vertex) -- the time those take at the run's copy rate, and for the backward the bytes its own scheme moves on top
(48-byte records written and read for the covered pixels, the id plane re-read by every owner of a face).  The results are also
compared with a float64 evaluation formed with torch on two faces (recorded, not asserted: the tests hold the bits).

--trace: a few calls of each route and nothing else, for a `rocprofv3 --kernel-trace --stats -- python tools/depth_interp_probe.py
--trace` run of its own (per-kernel times).  --out FILE: where the JSON goes besides stdout (default profiles/depth_interp.json)."""
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
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_interp.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("depth_interp_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
H = W = 200
COPY_BYTES = 512 << 20


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


def float64_check(depth, vg, gd, V, tri, tind, faces):
    """both directions of `faces` against a float64 evaluation with torch on the device (autograd for the backward): the largest
    |difference| over the largest |value| of each"""
    worst_f = worst_b = 0.0
    for b in faces:
        t = tind[b].reshape(-1).long()
        px = (t >= 0).nonzero().squeeze(1)
        ids = tri[:, t[px]].long()
        with torch.no_grad():   # triangles without area take the flat h: not part of this comparison
            Q = [V[b].double()[:2, ids[k]] for k in range(3)]
            e0, e1 = Q[2] - Q[0], Q[1] - Q[0]
            area = (e0 * e0).sum(0) * (e1 * e1).sum(0) - (e0 * e1).sum(0) ** 2 != 0
        px, ids = px[area], ids[:, area]
        Vb = V[b].double().clone().requires_grad_(True)
        P1, P2, P3 = (Vb[:, ids[k]] for k in range(3))
        pix = torch.stack([px % W, px // W]).double()
        v0, v1, v2 = P3[:2] - P1[:2], P2[:2] - P1[:2], pix - P1[:2]
        d00, d01, d02, d11, d12 = (v0 * v0).sum(0), (v0 * v1).sum(0), (v0 * v2).sum(0), (v1 * v1).sum(0), (v1 * v2).sum(0)
        den = d00 * d11 - d01 * d01
        u, v = (d11 * d02 - d01 * d12) / den, (d00 * d12 - d01 * d02) / den
        z = (1 - u - v) * P1[2] + v * P2[2] + u * P3[2]
        (z * gd[b].reshape(-1)[px].double()).sum().backward()
        worst_f = max(worst_f, float((depth[b].reshape(-1)[px].double() - z.detach()).abs().max() / z.detach().abs().max()))
        worst_b = max(worst_b, float((vg[b].double() - Vb.grad).abs().max() / Vb.grad.abs().max()))
    return worst_f, worst_b


out = {}
src = torch.empty((COPY_BYTES // 4,), dtype=torch.float32, device=dev).normal_()
dst = torch.empty_like(src)
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    N, ntri = net.nvert, int(net.tri.shape[1])
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    V = net.vertices_transform(P).detach().contiguous()
    tri_ind = ops.render_depth(V, net.tri, net.vertex_code, torch.zeros((B, H, W, 3), **o))[3].contiguous()
    covered = int((tri_ind >= 0).sum())
    gd, g3 = torch.randn((B, H, W, 1), **o), torch.randn((B, H, W, 3), **o)
    ndw = L.fr_render_depth_backward_workspace_bytes(B, H, W)
    dws = torch.empty((ndw,), dtype=torch.uint8, device=dev)
    nnw = L.fr_render_normal_backward_workspace_bytes(B, N, H, W)
    nws = torch.empty((nnw,), dtype=torch.uint8, device=dev)
    niw = L.fr_depth_interp_backward_workspace_bytes(B, N, H, W)
    iws = torch.empty((niw,), dtype=torch.uint8, device=dev)
    vg = torch.empty((B, 3, N), **o)
    depth = torch.empty((B, H, W, 1), **o)
    geo = (ctypes.c_int * 6)()
    L.fr_debug_depth_interp_bwd_geom(B, N, H, W, geo)

    def forward():
        return L.fr_depth_interp_forward(h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), B, N, ntri, H, W, h.ptr(depth), st)

    def backward():
        return L.fr_depth_interp_backward(h.ptr(gd), h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W, 0,
                                          h.ptr(iws), niw, st)

    def flat_backward():
        return L.fr_render_depth_backward_ws(h.ptr(gd), h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W, h.ptr(dws), ndw, st)

    def normal_raw():
        return L.fr_render_normal_backward(h.ptr(g3), 3, h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W,
                                           0, 0, h.ptr(nws), nnw, st)

    def copy():
        dst.copy_(src)
        return 0
    routes = {"forward": forward, "backward": backward, "flat_backward": flat_backward, "normal_raw": normal_raw, "copy": copy}
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
    assert forward() == 0 and backward() == 0
    torch.cuda.synchronize()
    agree_f, agree_b = float64_check(depth, vg, gd, V, net.tri, tri_ind, (0, B - 1))
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rate = 2 * COPY_BYTES / (rec["copy"]["median"] * 1e-6)
    rec["copy_rate_bytes_per_s"] = round(rate, -9)
    must_f = B * H * W * 8 + covered * (12 + 36)
    must_b = B * H * W * 8 + covered * (12 + 36) + B * 3 * N * 4
    scheme = covered * 48 + geo[0] * B * H * W * 16 + covered * 48
    for k, must in (("forward", must_f), ("backward", must_b)):
        t = rec[k]["median"]
        rec[k + "_vs_bytes"] = {"must_move": must, "time_at_copy_rate_us": round(must / rate * 1e6, 2),
                                "fraction_of_copy_rate": round(must / rate * 1e6 / t, 3)}
    rec["bytes"] = {"planes_read_or_written": B * H * W * 8, "id_gathers": covered * 12, "vertex_gathers": covered * 36,
                    "three_rows_written": B * 3 * N * 4, "backward_scheme_on_top": scheme, "records_written": covered * 48,
                    "id_plane_read_by_every_owner": geo[0] * B * H * W * 16, "term_planes_read": covered * 48}
    rec["geometry"] = dict(zip(("owners_per_face", "vertices_per_owner", "shift", "chunks", "lds_bytes", "xcd_map"), geo))
    rec["covered_pixels"] = covered
    rec["vs_float64_max_rel"] = {"forward": agree_f, "backward": agree_b}
    rec["backward_minus_normal_raw_us"] = round(rec["backward"]["median"] - rec["normal_raw"]["median"], 2)
    rec["backward_condition_holds"] = bool(rec["backward"]["median"] - rec["normal_raw"]["median"]
                                           <= max(rec["backward"]["spread_max_minus_min"], rec["normal_raw"]["spread_max_minus_min"]))
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

if not args.trace:
    doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds (medians of the rounds; spread = max - "
                   "min of the rounds), one process, raw C ABI, full-size mesh (N = 53,215, 105,840 triangles) at 200 x 200; forward / "
                   "backward = fr_depth_interp_forward / fr_depth_interp_backward (accumulate 0); flat_backward = "
                   "fr_render_depth_backward_ws and normal_raw = fr_render_normal_backward (mode 0, dense stride) on the same inputs; "
                   "copy = a 512 MiB device-to-device copy, copy_rate = 2 x 512 MiB / its median; must_move = the bytes any scheme "
                   "moves, fraction_of_copy_rate = (must_move / copy_rate) / time; backward_scheme_on_top = what the records pass and "
                   "the owners move besides (mostly L2 traffic); backward_condition_holds = backward - normal_raw <= the run's "
                   "round-to-round spread" % (args.calls, args.rounds),
           "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
