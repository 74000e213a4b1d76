#!/usr/bin/env python3
"""What the per-face albedo fit costs, in ONE process (modelled on tools/depth_interp_probe.py): alternating rounds, device events,
medians, 32 and 64 faces of the full mesh at 200 x 200, the maps from the project's own render.

  'basis_build'   = fr_albedo_basis_build (load time: once per mesh)
  'moments'       = fr_sfs_moments, the streaming half the lighting needs first (not new; for scale)
  'lighting'      = fr_sfs_lighting on that one part
  'fit'           = fr_albedo_lse_forward (the tile kernel and the finish-and-solve launch)
  'torch_fit'     = the same fit from stock torch ops in float64: index gather of the basis, einsum for G and r, linalg.solve
  'copy'          = a device-to-device copy of 512 MiB: the copy rate of THIS run, which prices the bytes below

Beside them the bytes each must move: the basis build reads 9 K fp32 per triangle at worst and writes K float64; the lighting reads
72 B and writes 80 B per pixel; the fit reads per face and pixel tri_ind, a, I (4 B each) and n' (12 B), the lighting once per pixel
and face (24 B out of cache after the first face), and gathers 8 K B of the basis per covered pixel -- 48 B + 8 K B x coverage per
pixel and face -- and writes 257 doubles per tile.

--alt-lib NAME=PATH: a shared library built from ANOTHER csrc/fr_sfs.hip alone (the parent commit's: hipcc --offload-arch=gfx950 -O3
-std=c++17 -ffp-contract=off -fPIC -shared -o PATH fr_sfs.hip): its fr_sfs_intensity_forward and _backward are timed in the same
rounds beside this build's, and whether their bits are equal is recorded -- this change adds a kernel to that file.
--trace: a few calls of each new entry point and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own (the split
of 'fit' between its two launches).
--out FILE: where the JSON goes besides stdout (default profiles/albedo_lse.json)."""
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
ap.add_argument("--torch-calls", type=int, default=5)
ap.add_argument("--faces", type=int, nargs="+", default=[32, 64])
ap.add_argument("--size", type=int, default=200)
ap.add_argument("--ridge", type=float, default=1e-6)
ap.add_argument("--alt-lib", action="append", default=[], metavar="NAME=PATH")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "albedo_lse.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("albedo_lse_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
L = h.lib()
dev = torch.device("cuda:0")
S = args.size
COPY_BYTES = 512 << 20
SFS = ("fr_sfs_intensity_forward", "fr_sfs_intensity_backward")
ALT = {}
for spec in args.alt_lib:
    name, path = spec.split("=", 1)
    ALT[name] = h.bind(ctypes.CDLL(path), SFS)


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


A = synth.make_assets()
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
src, dst = (torch.empty((COPY_BYTES,), dtype=torch.uint8, device=dev) for _ in range(2))
out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=dev)
    K, T, N = net.ndim_tex, int(net.tri.shape[1]), net.nvert
    params = torch.as_tensor(synth.sample_params_batch(B, im_size=S), device=dev)
    with torch.no_grad():
        V = net.vertices_transform(params)
        a, n, tind = net.compute_abedo_image(V, net.tri, net.mu_tex, with_tri_ind=True)
    im = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    a, n, tind = a.contiguous(), n.contiguous(), tind.contiguous()
    coverage = float((tind >= 0).float().mean())
    basis = torch.empty((T, K), dtype=torch.float64, device=dev)
    nba = L.fr_albedo_basis_bytes(T, K)
    nmo, nst = L.fr_sfs_moments_bytes(S, S), L.fr_sfs_state_bytes(S, S)
    mom = torch.empty((9, S, S), dtype=torch.float64, device=dev)
    state = torch.empty((10, S, S), dtype=torch.float64, device=dev)
    nws = L.fr_albedo_lse_workspace_bytes(B, S, S, K)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    alpha = torch.empty((B, K), dtype=torch.float32, device=dev)
    moments = torch.empty((B, 16, 16), dtype=torch.float64, device=dev)
    stats = torch.empty((B, 4), dtype=torch.float64, device=dev)
    light = state[6:9]

    def basis_build():
        L.fr_albedo_basis_build(h.ptr(net.tri), h.ptr(net.pc_tex), N, T, K, h.ptr(basis), nba, st)

    def moments_part():
        L.fr_sfs_moments(h.ptr(a), h.ptr(n), h.ptr(im), B, S, S, h.ptr(mom), nmo, st)

    def lighting():
        L.fr_sfs_lighting(h.ptr(mom), 1, S, S, 1e-6, h.ptr(state), nst, st)

    def fit():
        L.fr_albedo_lse_forward(h.ptr(basis), h.ptr(tind), h.ptr(light), h.ptr(n), h.ptr(a), h.ptr(im), B, T, S, S, K, args.ridge,
                                h.ptr(alpha), h.ptr(moments), h.ptr(stats), h.ptr(ws), nws, st)

    t_idx = tind.view(B, -1).long().clamp_min(0)
    cov = (tind.view(B, -1) >= 0).double()

    def torch_fit():
        d = torch.einsum("kp,bpk->bp", light.view(3, -1), n.view(B, -1, 3).double()) * cov
        X = basis[t_idx] * d[..., None]
        rho = (im.view(B, -1).double() - a.view(B, -1).double() * d) * cov
        G = torch.einsum("bpi,bpj->bij", X, X)
        r = torch.einsum("bpi,bp->bi", X, rho)
        lam = args.ridge * torch.diagonal(G, dim1=1, dim2=2).sum(1) / K
        return torch.linalg.solve(G + lam[:, None, None] * torch.eye(K, dtype=torch.float64, device=dev), r)

    def copy():
        dst.copy_(src)

    a2 = (a * 1.1).contiguous()
    gi = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(1)).to(dev)

    def sfs_buffers():
        return (torch.empty((B, S, S, 1), device=dev), torch.empty((10, S, S), dtype=torch.float64, device=dev),
                torch.empty((B, S, S, 3), device=dev), torch.empty((B, S, S, 3), device=dev))

    def sfs_routes(lib, bufs):
        inten, stt, gn, gn2 = bufs

        def fwd():
            lib.fr_sfs_intensity_forward(h.ptr(a), h.ptr(n), h.ptr(im), h.ptr(a2), h.ptr(n), B, S, S, 1e-6, h.ptr(inten),
                                         h.ptr(stt), nst, st)

        def bwd():
            lib.fr_sfs_intensity_backward(h.ptr(gi), h.ptr(a), h.ptr(im), h.ptr(a2), h.ptr(n), h.ptr(stt), nst, B, S, S,
                                          h.ptr(gn), h.ptr(gn2), st)
        return fwd, bwd

    routes = {"basis_build": basis_build, "moments": moments_part, "lighting": lighting, "fit": fit, "torch_fit": torch_fit,
              "copy": copy}
    sfs_out = {"this": sfs_buffers()}
    routes["this_sfs_forward"], routes["this_sfs_backward"] = sfs_routes(L, sfs_out["this"])
    for name, lib in ALT.items():
        sfs_out[name] = sfs_buffers()
        routes[name + "_sfs_forward"], routes[name + "_sfs_backward"] = sfs_routes(lib, sfs_out[name])
    if args.trace:
        for fn in (basis_build, moments_part, lighting, fit):
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        continue
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.torch_calls if k == "torch_fit" else args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rate = 2 * COPY_BYTES / (rec["copy"]["median"] * 1e-6)
    rec["copy_rate_bytes_per_s"] = round(rate, -9)
    npix = S * S
    tiles = -(-npix // 256)
    must = {"basis_build": T * K * 8 + min(9 * T, 3 * N) * K * 4 + 3 * T * 4,
            "lighting": npix * (72 + 80),
            "fit": int(B * npix * (4 + 4 + 4 + 12 + 8 * K * coverage) + npix * 24 + 2 * B * tiles * 257 * 8)}
    for k, v in must.items():
        rec[k + "_vs_bytes"] = {"must_move": v, "time_at_copy_rate_us": round(v / rate * 1e6, 2),
                                "fraction_of_copy_rate": round(v / rate * 1e6 / rec[k]["median"], 3)}
    rec["torch_over_fit"] = round(rec["torch_fit"]["median"] / rec["fit"]["median"], 1)
    ref = torch_fit()
    okf = stats[:, 3] == 1.0
    rec["fit_vs_torch"] = {"faces_ok": int(okf.sum()), "coverage": round(coverage, 3),
                           "largest_relative_difference_of_alpha": float(((alpha.double() - ref)[okf].abs().max(1).values
                                                                          / ref[okf].abs().max(1).values).max()),
                           "E1_over_E0_median": float((stats[okf, 2] / stats[okf, 1]).median())}
    for name in ALT:
        same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64),
                               y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int64))
                   for x, y in zip(sfs_out["this"], sfs_out[name]))
        rec[name + "_sfs_bits_equal"] = bool(same)
        rec[name + "_sfs_time_ratio"] = {d: round(rec["this_sfs_" + d]["median"] / rec[name + "_sfs_" + d]["median"], 3)
                                         for d in ("forward", "backward")}
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)
    del net

if args.trace:
    raise SystemExit(0)
geo = (ctypes.c_int * 5)()
L.fr_debug_albedo_lse_geom(args.faces[-1], S, S, 10, geo)
doc = {"what": "us per call, device events around %d calls per figure (%d for torch_fit), %d alternating rounds, one process, full mesh, "
               "%d x %d images rendered by the project; copy = a 512 MiB device-to-device copy, copy_rate = 2 x 512 MiB / its median; "
               "must_move = the bytes any scheme moves, fraction_of_copy_rate = (must_move / copy_rate) / time; <name>_sfs_* = the "
               "one-call SfS kernels of the library given as --alt-lib <name>=... beside this build's (this_sfs_*)"
               % (args.calls, args.torch_calls, args.rounds, S, S),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "ridge": args.ridge,
       "geometry_at_%d_faces" % args.faces[-1]: dict(zip(("pixels_per_tile", "tiles_per_face", "tile_workgroups", "finish_workgroups",
                                                         "finish_lds_bytes"), geo)),
       "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
