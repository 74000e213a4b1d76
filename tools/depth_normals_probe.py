#!/usr/bin/env python3
"""What the depth-map normals cost, in ONE process (modelled on tools/sfs_probe.py): alternating rounds, device events, medians, 64
and 32 faces at 200 x 200 on the depth map and tri_ind of a real render of the synthetic full-size assets (the depth perturbed as a
fine depth map would be).

  'kernel_fwd'      = fr_depth_normals_forward through the raw C ABI
  'kernel_bwd'      = fr_depth_normals_backward through the raw C ABI
  'op_fwd_bwd'      = rendering_layer/ops.py::depth_normals + backward of a given dL / d normal (autograd node, outputs allocated per
                      call)
  'torch_fwd'       = the same operator composed from stock torch ops in fp32 (pads, slices, `where` chains, sqrt, divisions, a
                      stack), under no_grad
  'torch_fwd_bwd'   = that composition with the depth requiring grad + backward of the same dL / d normal

Beside the kernels: the bytes each direction must move -- forward 20 B per (face, pixel) (depth and mask read, three floats written),
backward 24 B (normal gradient, depth and mask read, one float written) -- and the time they take at the measured copy rate of
6.29 TB/s.  The kernel is also compared with the fp32 composition (recorded, not asserted; the tests hold the kernel to its float64
model).

--alt-lib NAME=PATH (repeatable): a shared library built from another version of csrc/fr_depth_normals.hip ALONE (hipcc
--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -o PATH fr_depth_normals.hip): its two kernels are timed in the
same rounds, and whether its bits equal this build's is recorded -- how a change to the kernels is judged.
--trace: a few calls of each route and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own.
--out FILE: where the JSON goes besides stdout (default profiles/depth_normals.json)."""
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
import torch.nn.functional as F  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s: the measured device-to-device copy figure of the part

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="kernel calls per timed figure")
ap.add_argument("--torch-calls", type=int, default=5, help="torch-route calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--alt-lib", action="append", default=[], metavar="NAME=PATH")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_normals.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("depth_normals_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
H = W = 200


ALT = {}
for spec in args.alt_lib:
    name, path = spec.split("=", 1)
    ALT[name] = h.bind(ctypes.CDLL(path), ("fr_depth_normals_forward", "fr_depth_normals_backward"))


def _sh(a, dr, dc, fill):
    """out[b, r, c] = a[b, r + dr, c + dc], `fill` outside the image ([B,H,W])"""
    p = F.pad(a, (max(-dc, 0), max(dc, 0), max(-dr, 0), max(dr, 0)), value=fill)
    return p[:, max(dr, 0):max(dr, 0) + a.shape[1], max(dc, 0):max(dc, 0) + a.shape[2]]


def torch_depth_normals(depth, mask):
    """the operator from stock torch ops, fp32: [B,H,W,1], [B,H,W,1] -> [B,H,W,3]"""
    z = depth[..., 0]
    v = mask[..., 0] >= 0
    vf = v.to(z.dtype)
    Lv, Rv, Uv, Dv = (_sh(vf, 0, -1, 0.0) > 0, _sh(vf, 0, 1, 0.0) > 0, _sh(vf, -1, 0, 0.0) > 0, _sh(vf, 1, 0, 0.0) > 0)
    zL, zR, zU, zD = _sh(z, 0, -1, 0.0), _sh(z, 0, 1, 0.0), _sh(z, -1, 0, 0.0), _sh(z, 1, 0, 0.0)
    zero = torch.zeros_like(z)
    dx = torch.where(Lv & Rv, (zR - zL) * 0.5, torch.where(Rv, zR - z, torch.where(Lv, z - zL, zero)))
    dy = torch.where(Uv & Dv, (zD - zU) * 0.5, torch.where(Dv, zD - z, torch.where(Uv, z - zU, zero)))
    dx, dy = torch.where(v, dx, zero), torch.where(v, dy, zero)
    s = torch.sqrt((dx * dx + dy * dy) + 1.0)
    n = torch.stack([-dx / s, -dy / s, 1.0 / s], -1)
    return n * vf[..., None]


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
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    with torch.no_grad():
        V = net.vertices_transform(P)
        depth, _, _, tri_ind = ops.render_depth(V, net.tri, net.vertex_code, torch.zeros((B, H, W, 3), **o))
    mask = tri_ind.contiguous()
    # a fine depth map: the coarse one plus a smooth-ish perturbation; the background's depth is left as the render wrote it
    fine = (depth + 0.05 * torch.rand((B, H, W, 1), generator=torch.Generator().manual_seed(2)).to(dev)).contiguous()
    g = torch.randn((B, H, W, 3), generator=torch.Generator().manual_seed(3)).to(dev)
    normal = torch.empty((B, H, W, 3), **o)
    gd = torch.empty((B, H, W, 1), **o)
    z_req = fine.clone().requires_grad_(True)

    def c_fwd(lib, out):
        return lambda: lib.fr_depth_normals_forward(h.ptr(fine), h.ptr(mask), B, H, W, h.ptr(out), st)

    def c_bwd(lib, out):
        return lambda: lib.fr_depth_normals_backward(h.ptr(g), h.ptr(fine), h.ptr(mask), B, H, W, h.ptr(out), st)
    k_fwd, k_bwd = c_fwd(L, normal), c_bwd(L, gd)

    def op_fwd_bwd():
        z_req.grad = None
        ops.depth_normals(z_req, mask).backward(g)

    def torch_fwd():
        with torch.no_grad():
            return torch_depth_normals(fine, mask)

    def torch_fwd_bwd():
        z_req.grad = None
        torch_depth_normals(z_req, mask).backward(g)
    routes = {"torch_fwd": (torch_fwd, args.torch_calls), "kernel_fwd": (k_fwd, args.calls),
              "torch_fwd_bwd": (torch_fwd_bwd, args.torch_calls), "op_fwd_bwd": (op_fwd_bwd, args.calls),
              "kernel_bwd": (k_bwd, args.calls)}
    assert k_fwd() == 0 and k_bwd() == 0
    bits = {}
    for name, lib in ALT.items():   # the other library's kernels on the same inputs: the same bits?
        n_alt, gd_alt = torch.full_like(normal, float("nan")), torch.full_like(gd, float("nan"))
        assert c_fwd(lib, n_alt)() == 0 and c_bwd(lib, gd_alt)() == 0
        torch.cuda.synchronize()
        bits["equals_" + name] = bool((n_alt.view(torch.int32) == normal.view(torch.int32)).all()
                                      and (gd_alt.view(torch.int32) == gd.view(torch.int32)).all())
        routes["%s_fwd" % name] = (c_fwd(lib, n_alt), args.calls)
        routes["%s_bwd" % name] = (c_bwd(lib, gd_alt), args.calls)
    for fn, _ in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if args.trace:
        for fn, _ in routes.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        continue
    # the kernel beside the fp32 composition (recorded, not asserted)
    assert k_fwd() == 0 and k_bwd() == 0
    n_t = torch_fwd()
    torch_fwd_bwd()
    diff_n = float((normal - n_t).abs().max())
    diff_g = float((gd - z_req.grad).abs().max())
    gmax = float(gd.abs().max())
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, (fn, calls) in routes.items():
            res[k].append(timed(fn, calls))
    rec = {k: summary(v) for k, v in res.items()}
    npix = H * W
    must_f, must_b = B * npix * 20, B * npix * 24
    rec["bytes"] = {"forward_must_move": must_f, "backward_must_move": must_b,
                    "forward_time_at_copy_rate_us": round(must_f / COPY_RATE * 1e6, 2),
                    "backward_time_at_copy_rate_us": round(must_b / COPY_RATE * 1e6, 2)}
    rec["kernel_fwd_over_byte_floor"] = round(rec["kernel_fwd"]["median"] / (must_f / COPY_RATE * 1e6), 2)
    rec["kernel_bwd_over_byte_floor"] = round(rec["kernel_bwd"]["median"] / (must_b / COPY_RATE * 1e6), 2)
    rec["torch_over_kernel_fwd"] = round(rec["torch_fwd"]["median"] / rec["kernel_fwd"]["median"], 2)
    rec["torch_over_op_fwd_bwd"] = round(rec["torch_fwd_bwd"]["median"] / rec["op_fwd_bwd"]["median"], 2)
    geo = (ctypes.c_int * 6)()
    L.fr_debug_depth_normals_geom(B, H, W, geo)
    rec["geometry"] = dict(zip(("tile_w", "tile_h", "threads", "tiles_across", "tiles_down", "lds_backward"), geo))
    if bits:
        rec["bits"] = bits
    rec["valid_pixels"] = int((mask >= 0).sum())
    rec["kernel_vs_torch_fp32_max_abs"] = {"normal": diff_n, "grad_depth": diff_g, "max_abs_grad_depth": gmax}
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

if not args.trace:
    doc = {"what": "us per call, device events around %d kernel / %d torch calls per figure, %d alternating rounds, one process; depth "
                   "and tri_ind from render_depth of the full-size synthetic mesh at 200 x 200, the depth perturbed by 0.05 x uniform "
                   "noise; kernel_fwd / kernel_bwd = fr_depth_normals_forward / _backward through the raw C ABI, op_fwd_bwd = the "
                   "autograd operator depth_normals + backward (it allocates its outputs per call), torch_* = the same operator "
                   "composed from stock torch ops in fp32; *_must_move = the bytes any scheme moves, *_over_byte_floor = time / "
                   "(must_move / 6.29 TB/s); <name>_fwd / <name>_bwd = the same calls from a library given as --alt-lib <name>=..., "
                   "bits.equals_<name> = whether its outputs have this build's bits" % (args.calls, args.torch_calls, args.rounds),
           "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
           "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
