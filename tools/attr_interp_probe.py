#!/usr/bin/env python3
"""What the smooth planes cost, in ONE process through the raw C ABI (modelled on tools/depth_interp_probe.py): alternating rounds,
device events, medians of the rounds, the full-size mesh at 200 x 200, 32 and 64 faces.

  'forward'            = fr_attr_interp_forward of a per-face [B,3,N] attribute                (the post-pass over tri_ind)
  'backward_attr'      = fr_attr_interp_backward with attr_grad alone                         (one records pass, one owner pass)
  'backward_vertex'    = ... with vertex_grad alone
  'backward_both'      = ... with both                                                        (one records pass, two owner passes)
  'normals_forward'    = fr_mesh_vertex_normals
  'normals_backward'   = fr_mesh_vertex_normals_backward: its two launches, timed as the one call they are (the first repeats the
                         forward's walk; a --trace run under rocprofv3 --kernel-trace --stats gives each kernel's own time)
  'depth_forward' / 'depth_backward' = fr_depth_interp_forward / _backward on the same vertices and tri_ind
  'torch_*'            = the same operators composed from stock torch ops in fp32 (gathers, elementwise arithmetic, index_add_;
                         the backwards by autograd: forward + backward, minus nothing)
  'copy'               = a device-to-device copy of 512 MiB: the copy rate of THIS run, which prices the bytes below

Beside each of ours: the bytes it must move -- planes read and written, the id gathers (12 B), the x and y gathers (24 B) and the
attribute gathers (36 B) of the covered pixels, the rows written (12 B per vertex and output); for the normals' backward the
vertices, the gradient, h written and read and the rows written per face, the triangle list and the adjacency once -- and the time
those take at the run's copy rate.

--parent-lib PATH: a library built from the PARENT commit's fr_depth_interp.hip (see --make-parent-lib), loaded beside ours: its
fr_depth_interp_forward / _backward on the same inputs in the same rounds -- the same bits, and the time of each beside ours.  The
weights moved from that file into csrc/fr_point_weight.h; this is the check that the move cost nothing.
--make-parent-lib REV OUT: no GPU needed -- takes csrc/ and include/ of git revision REV into a temporary directory and compiles its
fr_depth_interp.hip alone into the shared library OUT, with the package's flags.
--trace: a few calls of each route and nothing else.  --out FILE: where the JSON goes besides stdout (default
profiles/attr_interp.json)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--trace", action="store_true")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--make-parent-lib", nargs=2, metavar=("REV", "OUT"), default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_interp.json"))
args = ap.parse_args()

h = importlib.import_module("3dfacerecon_amd._lib")
DEPTH = ("fr_depth_interp_forward", "fr_depth_interp_backward_workspace_bytes", "fr_depth_interp_backward")

if args.make_parent_lib:
    rev, dest = args.make_parent_lib
    with tempfile.TemporaryDirectory() as tmp:
        for sub in ("3dfacerecon_amd/csrc", "include"):
            names = subprocess.check_output(["git", "ls-tree", "--name-only", rev, sub + "/"], cwd=ROOT, text=True).split()
            os.makedirs(os.path.join(tmp, sub))
            for n in names:
                with open(os.path.join(tmp, n), "wb") as f:
                    f.write(subprocess.check_output(["git", "show", "%s:%s" % (rev, n)], cwd=ROOT))
        os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
        subprocess.check_call([h._hipcc()] + h.HIPCC_FLAGS + ["-o", os.path.abspath(dest), "fr_depth_interp.hip"],
                              cwd=os.path.join(tmp, "3dfacerecon_amd", "csrc"))
    print("built", dest, "from", rev)
    raise SystemExit(0)

import torch  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("attr_interp_probe: needs an MI355X (a measurement path does not fall back)")

synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
PL = h.bind(ctypes.CDLL(os.path.abspath(args.parent_lib)), DEPTH) if args.parent_lib else None
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


def same_bits(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


# ---- the same operators from stock torch ops, fp32 ---------------------------------------------------------------------------------
def torch_interp(V, At, tri_l, tind):
    B = V.shape[0]
    t = tind.reshape(B, -1).long()
    cov = (t >= 0).unsqueeze(1)
    ids = tri_l[:, t.clamp_min(0)]                                            # [3,B,HW]
    P = [torch.gather(V, 2, ids[k].unsqueeze(1).expand(-1, 3, -1)) for k in range(3)]
    Q = [torch.gather(At, 2, ids[k].unsqueeze(1).expand(-1, 3, -1)) for k in range(3)]
    i = torch.arange(H * W, device=V.device)
    px, py = (i % W).float(), (i // W).float()
    v0x, v0y = P[2][:, 0] - P[0][:, 0], P[2][:, 1] - P[0][:, 1]
    v1x, v1y = P[1][:, 0] - P[0][:, 0], P[1][:, 1] - P[0][:, 1]
    v2x, v2y = px - P[0][:, 0], py - P[0][:, 1]
    d00, d01, d02 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v0x * v2x + v0y * v2y
    d11, d12 = v1x * v1x + v1y * v1y, v1x * v2x + v1y * v2y
    inv = 1 / (d00 * d11 - d01 * d01)
    u, v = ((d11 * d02 - d01 * d12) * inv).unsqueeze(1), ((d00 * d12 - d01 * d02) * inv).unsqueeze(1)
    out = (1 - u - v) * Q[0] + v * Q[1] + u * Q[2]
    return torch.where(cov, out, torch.zeros_like(out)).permute(0, 2, 1).reshape(B, H, W, 3)


def torch_normals(V, tri_l):
    P = [V[:, :, tri_l[k]] for k in range(3)]
    n = torch.linalg.cross(P[1] - P[0], P[2] - P[0], dim=1)
    N = torch.zeros_like(V)
    for k in range(3):
        N = N.index_add(2, tri_l[k], n)
    return N / N.norm(dim=1, keepdim=True).clamp_min(1e-30)


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
    At = (torch.rand((B, 3, N), **o) + 0.1).contiguous()
    g3, g1, gn = torch.randn((B, H, W, 3), **o), torch.randn((B, H, W, 1), **o), torch.randn((B, 3, N), **o)
    adj = net.adjacency()
    tri_l = net.tri.long()
    chunks = (H * W + 1023) // 1024
    rec = torch.empty((2, B, 3, H * W, 4), dtype=torch.int32, device=dev)
    part = torch.empty((2, B, chunks, 2), dtype=torch.int32, device=dev)
    hbuf = torch.empty((B, 3, N), dtype=torch.float64, device=dev)
    niw = L.fr_depth_interp_backward_workspace_bytes(B, N, H, W)
    iws = torch.empty((niw,), dtype=torch.uint8, device=dev)
    plane = torch.empty((B, H, W, 3), **o)
    depth, depth_p = torch.empty((B, H, W, 1), **o), torch.empty((B, H, W, 1), **o)
    ga, gv, vg, vg_p, nrm, gvn = (torch.empty((B, 3, N), **o) for _ in range(6))
    geo = (ctypes.c_int * 6)()
    L.fr_debug_attr_interp_bwd_geom(B, N, H, W, geo)

    def forward():
        return L.fr_attr_interp_forward(h.ptr(V), N, h.ptr(At), N, h.ptr(net.tri), h.ptr(tri_ind), B, N, ntri, H, W, h.ptr(plane), st)

    def backward(want_a, want_v):
        return lambda: L.fr_attr_interp_backward(h.ptr(g3), h.ptr(V), N, h.ptr(At), N, h.ptr(net.tri), h.ptr(tri_ind),
                                                 h.ptr(ga) if want_a else None, 0, h.ptr(gv) if want_v else None, 0, B, N, ntri, H, W,
                                                 h.ptr(rec), h.ptr(part), st)

    def normals_forward():
        return L.fr_mesh_vertex_normals(h.ptr(V), N, h.ptr(net.tri), h.ptr(adj.adj_start), h.ptr(adj.adj_tri), B, N, ntri, h.ptr(nrm), N, st)

    def normals_backward():
        return L.fr_mesh_vertex_normals_backward(h.ptr(gn), N, h.ptr(V), N, h.ptr(net.tri), h.ptr(adj.adj_start), h.ptr(adj.adj_tri), B, N,
                                                 ntri, h.ptr(hbuf), h.ptr(gvn), N, 0, st)

    def depth_calls(lib, d, g):
        return (lambda: lib.fr_depth_interp_forward(h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), B, N, ntri, H, W, h.ptr(d), st),
                lambda: lib.fr_depth_interp_backward(h.ptr(g1), h.ptr(V), N, h.ptr(net.tri), h.ptr(tri_ind), h.ptr(g), B, N, ntri, H, W, 0,
                                                     h.ptr(iws), niw, st))

    def torch_forward():
        with torch.no_grad():
            torch_interp(V, At, tri_l, tri_ind)
        return 0

    def torch_backward():
        Vr, Ar = V.clone().requires_grad_(True), At.clone().requires_grad_(True)
        (torch_interp(Vr, Ar, tri_l, tri_ind) * g3).sum().backward()
        return 0

    def torch_normals_forward():
        with torch.no_grad():
            torch_normals(V, tri_l)
        return 0

    def torch_normals_backward():
        Vr = V.clone().requires_grad_(True)
        (torch_normals(Vr, tri_l) * gn).sum().backward()
        return 0

    def copy():
        dst.copy_(src)
        return 0
    routes = {"forward": forward, "backward_attr": backward(True, False), "backward_vertex": backward(False, True),
              "backward_both": backward(True, True), "normals_forward": normals_forward, "normals_backward": normals_backward}
    routes["depth_forward"], routes["depth_backward"] = depth_calls(L, depth, vg)
    if PL is not None:
        routes["parent_depth_forward"], routes["parent_depth_backward"] = depth_calls(PL, depth_p, vg_p)
    routes.update(torch_forward=torch_forward, torch_backward=torch_backward, torch_normals_forward=torch_normals_forward,
                  torch_normals_backward=torch_normals_backward, copy=copy)
    for fn in routes.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    if args.trace:
        for k, fn in routes.items():
            if not k.startswith("torch_"):
                for _ in range(10):
                    fn()
        torch.cuda.synchronize()
        continue
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    r = {k: summary(v) for k, v in res.items()}
    rate = 2 * COPY_BYTES / (r["copy"]["median"] * 1e-6)
    r["copy_rate_bytes_per_s"] = round(rate, -9)
    px = B * H * W
    must = {"forward": px * 16 + covered * (12 + 24 + 36),
            "backward_attr": px * 16 + covered * (12 + 24) + B * 3 * N * 4,
            "backward_vertex": px * 16 + covered * (12 + 24 + 36) + B * 3 * N * 4,
            "backward_both": px * 16 + covered * (12 + 24 + 36) + 2 * B * 3 * N * 4,
            "normals_forward": B * N * (12 + 12) + ntri * 12 + 3 * ntri * 4 + (N + 1) * 4,
            "normals_backward": B * N * (12 + 12 + 24 + 24 + 12) + ntri * 12 + 3 * ntri * 4 + (N + 1) * 4}
    for k, m in must.items():
        t = r[k]["median"]
        r[k + "_vs_bytes"] = {"must_move": m, "time_at_copy_rate_us": round(m / rate * 1e6, 2),
                              "time_over_byte_floor": round(t / (m / rate * 1e6), 2)}
    r["vs_torch"] = {"forward": round(r["torch_forward"]["median"] / r["forward"]["median"], 1),
                     "backward_both": round(r["torch_backward"]["median"] / r["backward_both"]["median"], 1),
                     "normals_forward": round(r["torch_normals_forward"]["median"] / r["normals_forward"]["median"], 1),
                     "normals_backward": round(r["torch_normals_backward"]["median"] / r["normals_backward"]["median"], 1)}
    r["geometry"] = dict(zip(("owners_per_face", "vertices_per_owner", "shift", "chunks", "lds_bytes", "xcd_map"), geo))
    r["covered_pixels"] = covered
    # agreement with the torch composition (fp32 against float64-then-rounded: recorded, not asserted -- the tests hold the bits)
    assert forward() == 0 and backward(True, True)() == 0
    Vr, Ar = V.clone().requires_grad_(True), At.clone().requires_grad_(True)
    tp = torch_interp(Vr, Ar, tri_l, tri_ind)
    (tp * g3).sum().backward()
    ok = torch.isfinite(tp.detach()).all(dim=-1) & (tri_ind[..., 0] >= 0)
    r["vs_torch_fp32_max_abs"] = {"forward": float((plane - tp.detach())[ok].abs().max()), "forward_scale": float(plane[ok].abs().max()),
                                  "attr_grad": float((ga - Ar.grad).abs().max()), "attr_grad_scale": float(ga.abs().max())}
    if PL is not None:
        for fn in depth_calls(L, depth, vg) + depth_calls(PL, depth_p, vg_p):
            assert fn() == 0
        torch.cuda.synchronize()
        r["parent_depth_interp"] = {
            "forward_same_bits": same_bits(depth, depth_p), "backward_same_bits": same_bits(vg, vg_p),
            "forward_us_ours_minus_parent": round(r["depth_forward"]["median"] - r["parent_depth_forward"]["median"], 2),
            "backward_us_ours_minus_parent": round(r["depth_backward"]["median"] - r["parent_depth_backward"]["median"], 2),
            "within_spread": bool(
                abs(r["depth_forward"]["median"] - r["parent_depth_forward"]["median"])
                <= max(r["depth_forward"]["spread_max_minus_min"], r["parent_depth_forward"]["spread_max_minus_min"])
                and abs(r["depth_backward"]["median"] - r["parent_depth_backward"]["median"])
                <= max(r["depth_backward"]["spread_max_minus_min"], r["parent_depth_backward"]["spread_max_minus_min"]))}
    out["B=%d" % B] = r
    print("B=%d" % B, json.dumps(r), flush=True)

if not args.trace:
    doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds (medians of the rounds; spread = max - "
                   "min of the rounds), one process, raw C ABI, full-size mesh (N = 53,215, 105,840 triangles) at 200 x 200; the routes "
                   "are named in tools/attr_interp_probe.py; copy = a 512 MiB device-to-device copy, copy_rate = 2 x 512 MiB / its "
                   "median; must_move = the bytes any scheme moves, time_over_byte_floor = time / (must_move / copy_rate); vs_torch = "
                   "the stock-torch composition's time over ours; parent_depth_interp = fr_depth_interp_* of a library built from the "
                   "parent commit's source, in the same rounds" % (args.calls, args.rounds),
           "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
