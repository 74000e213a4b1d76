#!/usr/bin/env python3
"""What the soft coverage costs, in ONE process through the raw C ABI (modelled on tools/depth_interp_probe.py): alternating rounds,
device events, medians of the rounds, the full-size mesh at 200 x 200, 32 and 64 faces.

  'forward'          = fr_coverage_forward                                               (the post-pass over tri_ind)
  'backward'         = fr_coverage_backward, accumulate 0, dense [B,H,W,1] gradient      (x and y rows; z is +0)
  'dinterp_forward'  = fr_depth_interp_forward on the same inputs
  'dinterp_backward' = fr_depth_interp_backward on the same inputs: the same record planes through the same owners, with a record
                       for every covered pixel instead of the border pixels alone
  'parent_dinterp_backward' (--parent-lib FILE) = fr_depth_interp_backward of a library built from the parent commit's
                       csrc/fr_depth_interp.hip, in the same rounds: the shared owner kept its time; its bits are compared too
  'forward_background' / 'dinterp_forward_background' = the two forwards on a tri_ind plane of -1: no gather at all, so what is left
                       is each kernel's own structure (the staged tile with its halo and barrier against a plain map)
  'copy'             = a device-to-device copy of 512 MiB: the copy rate of THIS run, which prices the bytes below

Beside each direction the bytes it must move -- forward: tri_ind read and cov written (8 B per pixel), the id gathers (12 B) of the
covered pixels and the x, y gathers (24 B per triangle) of the border pixels; backward: tri_ind read (4 B per pixel), the id gathers
of the covered pixels, cov and cov_grad (8 B) and the x, y gathers on the border pixels, three rows written (12 B per vertex) -- and
the time those take at the run's copy rate.

--out FILE: where the JSON goes besides stdout (default profiles/coverage.json)."""
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
ap.add_argument("--parent-lib", default=None, help="a shared library built from the parent commit's fr_depth_interp.hip alone")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("coverage_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
PARENT = None
if args.parent_lib:
    PARENT = h.bind(ctypes.CDLL(os.path.abspath(args.parent_lib)), ["fr_depth_interp_backward"])
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
    ok = tri_ind[..., 0] >= 0
    covered = int(ok.sum())
    pad = torch.nn.functional.pad(ok[:, None].float(), (1, 1, 1, 1), mode="replicate")[:, 0] > 0
    differs = (pad[:, 1:-1, :-2] != ok) | (pad[:, 1:-1, 2:] != ok) | (pad[:, :-2, 1:-1] != ok) | (pad[:, 2:, 1:-1] != ok)
    border_ok, border_bg = int((differs & ok).sum()), int((differs & ~ok).sum())
    gd = torch.randn((B, H, W, 1), **o)
    nws = L.fr_coverage_backward_workspace_bytes(B, N, H, W)
    assert nws == L.fr_depth_interp_backward_workspace_bytes(B, N, H, W)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    vg, vg2 = torch.empty((B, 3, N), **o), torch.empty((B, 3, N), **o)
    cov, depth = torch.empty((B, H, W, 1), **o), torch.empty((B, H, W, 1), **o)
    geo = (ctypes.c_int * 6)()
    L.fr_debug_coverage_bwd_geom(B, N, H, W, geo)

    def forward():
        return L.fr_coverage_forward(h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), B, N, ntri, H, W, h.ptr(cov), st)

    def backward():
        return L.fr_coverage_backward(h.ptr(gd), h.ptr(cov), h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W,
                                      0, h.ptr(ws), nws, st)

    def dinterp_forward():
        return L.fr_depth_interp_forward(h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), B, N, ntri, H, W, h.ptr(depth), st)

    def dinterp_backward(lib=L, dstv=vg2):
        return lib.fr_depth_interp_backward(h.ptr(gd), h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), h.ptr(dstv), B, N, ntri, H, W, 0,
                                            h.ptr(ws), nws, st)

    nothing = torch.full_like(tri_ind, -1.0)

    def forward_background():
        return L.fr_coverage_forward(h.ptr(V), N, h.ptr(net.tri), h.ptr(nothing), B, N, ntri, H, W, h.ptr(depth), st)

    def dinterp_forward_background():
        return L.fr_depth_interp_forward(h.ptr(V), N, h.ptr(net.tri), h.ptr(nothing), B, N, ntri, H, W, h.ptr(depth), st)

    def copy():
        dst.copy_(src)
        return 0
    routes = {"forward": forward, "backward": backward, "dinterp_forward": dinterp_forward, "dinterp_backward": dinterp_backward,
              "forward_background": forward_background, "dinterp_forward_background": dinterp_forward_background}
    same_bits = None
    if PARENT is not None:
        vg3 = torch.empty((B, 3, N), **o)
        routes["parent_dinterp_backward"] = lambda: dinterp_backward(PARENT, vg3)
    routes["copy"] = copy
    for fn in routes.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    if PARENT is not None:
        same_bits = bool((vg2.view(torch.int32) == vg3.view(torch.int32)).all())
    soft = int(((cov > 0) & (cov < 1)).sum())
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rate = 2 * COPY_BYTES / (rec["copy"]["median"] * 1e-6)
    rec["copy_rate_bytes_per_s"] = round(rate, -9)
    must = {"forward": B * H * W * 8 + covered * 12 + (border_ok + border_bg) * 24,
            "backward": B * H * W * 4 + covered * 12 + border_ok * (24 + 16) + B * 3 * N * 4,
            "dinterp_forward": B * H * W * 8 + covered * (12 + 36),
            "dinterp_backward": B * H * W * 8 + covered * (12 + 36) + B * 3 * N * 4}
    for k, m in must.items():
        t = rec[k]["median"]
        rec[k + "_vs_bytes"] = {"must_move": m, "time_at_copy_rate_us": round(m / rate * 1e6, 2),
                                "fraction_of_copy_rate": round(m / rate * 1e6 / t, 3)}
    rec["geometry"] = dict(zip(("owners_per_face", "vertices_per_owner", "shift", "chunks", "lds_bytes", "xcd_map"), geo))
    rec["pixels"] = {"all": B * H * W, "covered": covered, "border_ok": border_ok, "border_background": border_bg, "soft": soft}
    rec["backward_scheme_on_top"] = {"records_written": B * H * W * 16 + border_ok * 32,
                                     "id_plane_read_by_every_owner": geo[0] * B * H * W * 16, "term_planes_read": border_ok * 32}
    rec["forward_below_dinterp_forward"] = bool(rec["forward"]["median"] < rec["dinterp_forward"]["median"])
    if PARENT is not None:
        rec["parent_dinterp_backward_same_bits"] = same_bits
        rec["dinterp_backward_minus_parent_us"] = round(rec["dinterp_backward"]["median"] - rec["parent_dinterp_backward"]["median"], 2)
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds (medians of the rounds; spread = max - min "
               "of the rounds), one process, raw C ABI, full-size mesh (N = 53,215, 105,840 triangles) at 200 x 200; forward / backward "
               "= fr_coverage_forward / fr_coverage_backward (accumulate 0); dinterp_* = fr_depth_interp_forward / _backward on the "
               "same inputs; *_background = the two forwards on a tri_ind of -1 everywhere (no gathers); parent_dinterp_backward = the same entry point of a library built from the parent commit's source; copy = "
               "a 512 MiB device-to-device copy, copy_rate = 2 x 512 MiB / its median; must_move = the bytes any scheme moves, "
               "fraction_of_copy_rate = (must_move / copy_rate) / time" % (args.calls, args.rounds),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
