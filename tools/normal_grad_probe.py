#!/usr/bin/env python3
"""What the normal-map gradients cost, in ONE process through the raw C ABI (modelled on tools/pose_grad_probe.py): alternating
rounds, device events, medians, the full-size mesh at 200 x 200.

  'depth'         = fr_render_depth_backward_ws alone                                   (the z-only backward every caller runs)
  'normal_raw'    = fr_render_normal_backward, mode 0, accumulate 0, dense [B,H,W,3] gradient
  'normal_post'   = fr_render_normal_backward, mode 1, accumulate 1, channels 4-6 of a [B,H,W,7] gradient (what
                    rendering_layer_fused(normal_grad=True) enqueues behind 'depth')
  'depth_normal'  = 'depth' followed by 'normal_post': the backward of the flag-on node

Beside the new call: the bytes it must move -- normal_grad and tri_ind read (16 B per pixel), the id gathers (12 B) and the
vertex gathers (36 B) of the covered pixels, three rows written (12 B per vertex) -- the time those take at the measured copy
rate of 6.29 TB/s, and the bytes its own scheme moves on top (48-byte records written for the covered pixels, the id plane
re-read by every owner of a face).  The clock the part holds is read behind the timed rounds (fr_debug_clock_probe).  The
results are also compared with a float64 sum of the call's terms on two faces (recorded, not asserted).

--trace: a few calls of each route and nothing else, for a `rocprofv3 --kernel-trace --stats -- python tools/normal_grad_probe.py
--trace` run of its own (per-kernel times).  --out FILE: where the JSON goes besides stdout (default
profiles/render_normal_backward.json)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_normal_backward.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("normal_grad_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
H = W = 200


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


def clock_ghz():
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ticks = torch.zeros((cus, 2), dtype=torch.int64, device=dev)
    assert L.fr_debug_clock_probe(h.ptr(ticks), cus, int(2e-3 * 2.1e9 / (6 * 32 * 4)), st) == 0
    torch.cuda.synchronize()
    t = ticks.cpu().double()
    return round(float((0.1 * t[:, 0] / t[:, 1].clamp(min=1)).median()), 3)


def float64_check(got, g, V, tri, tind, faces):
    """the raw-mode result of `faces` against a float64 scatter of the same terms formed with torch on the device: the largest
    |difference| over the largest |value| (a transposition or a sign could not hide; the tests hold the bits to their bound)"""
    worst = 0.0
    for b in faces:
        t = tind[b].reshape(-1).long()
        px = (t >= 0).nonzero().squeeze(1)
        ids = tri[:, t[px]].long()
        P = [V[b].double()[:, ids[k]].T for k in range(3)]
        a, bb, G = (P[0] - P[1]), (P[0] - P[2]), g[b].reshape(-1, 3)[px].double()
        da, db = torch.linalg.cross(bb, G, dim=1), torch.linalg.cross(G, a, dim=1)
        want = torch.zeros((3, V.shape[2]), dtype=torch.float64, device=dev)
        for k, term in enumerate((da + db, -da, -db)):
            want.index_add_(1, ids[k], term.T.contiguous())
        worst = max(worst, float((got[b].double() - want).abs().max() / want.abs().max()))
    return worst


out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    N, ntri = net.nvert, int(net.tri.shape[1])
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    V = net.vertices_transform(P).detach().contiguous()
    tri_ind = ops.render_depth(V, net.tri, net.vertex_code, torch.zeros((B, H, W, 3), **o))[3].contiguous()
    covered = int((tri_ind >= 0).sum())
    gd, g3, g7 = torch.randn((B, H, W, 1), **o), torch.randn((B, H, W, 3), **o), torch.randn((B, H, W, 7), **o)
    ndw = L.fr_render_depth_backward_workspace_bytes(B, H, W)
    dws = torch.empty((ndw,), dtype=torch.uint8, device=dev)
    nnw = L.fr_render_normal_backward_workspace_bytes(B, N, H, W)
    nws = torch.empty((nnw,), dtype=torch.uint8, device=dev)
    vg = torch.empty((B, 3, N), **o)
    g7n = ctypes.c_void_p(g7.data_ptr() + 16)
    geo = (ctypes.c_int * 6)()
    L.fr_debug_render_normal_bwd_geom(B, N, H, W, geo)

    def depth():
        return L.fr_render_depth_backward_ws(h.ptr(gd), h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W, h.ptr(dws), ndw, st)

    def normal_raw():
        return L.fr_render_normal_backward(h.ptr(g3), 3, h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W,
                                           0, 0, h.ptr(nws), nnw, st)

    def normal_post():
        return L.fr_render_normal_backward(g7n, 7, h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W, 1, 1,
                                           h.ptr(nws), nnw, st)

    def depth_normal():
        return depth() or normal_post()
    routes = {"depth": depth, "normal_raw": normal_raw, "normal_post": normal_post, "depth_normal": depth_normal}
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
    assert normal_raw() == 0
    torch.cuda.synchronize()
    agree = float64_check(vg, g3, V, net.tri, tri_ind, (0, B - 1))
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rec["clock_GHz_held"] = clock_ghz()
    must = B * H * W * 16 + covered * (12 + 36) + B * 3 * N * 4
    scheme = covered * 48 + geo[0] * B * H * W * 16 + covered * 48
    for k in ("normal_raw", "normal_post"):
        t = rec[k]["median"]
        rec[k + "_vs_bytes"] = {"time_at_copy_rate_us": round(must / COPY_RATE * 1e6, 2),
                                "fraction_of_copy_rate": round(must / COPY_RATE * 1e6 / t, 3)}
    rec["bytes"] = {"must_move": must, "normal_grad_and_tri_ind_read": B * H * W * 16, "id_gathers": covered * 12,
                    "vertex_gathers": covered * 36, "three_rows_written": B * 3 * N * 4,
                    "scheme_on_top": scheme, "records_written": covered * 48, "id_plane_read_by_every_owner": geo[0] * B * H * W * 16,
                    "term_planes_read": covered * 48}
    rec["geometry"] = dict(zip(("owners_per_face", "vertices_per_owner", "shift", "chunks", "lds_bytes", "xcd_map"), geo))
    rec["covered_pixels"] = covered
    rec["raw_vs_float64_scatter_max_rel"] = agree
    rec["flag_on_adds_us"] = round(rec["depth_normal"]["median"] - rec["depth"]["median"], 2)
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

if not args.trace:
    doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, raw C ABI, full-size "
                   "mesh (N = 53,215, 105,840 triangles) at 200 x 200; normal_raw / normal_post = fr_render_normal_backward (mode 0 "
                   "dense gradient, accumulate 0 / mode 1 at stride 7, accumulate 1); depth = fr_render_depth_backward_ws on the same "
                   "tri_ind; flag_on_adds_us = depth_normal - depth; must_move = the bytes any scheme moves, fraction_of_copy_rate = "
                   "(must_move / 6.29 TB/s) / time; scheme_on_top = what the records pass and the owners move besides (mostly L2 "
                   "traffic: every owner of a face re-reads its id plane)" % (args.calls, args.rounds),
           "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
           "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
