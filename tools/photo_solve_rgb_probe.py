#!/usr/bin/env python3
"""What the colour photometric solve costs, in ONE process (modelled on tools/albedo_lse_probe.py): alternating rounds, device events,
medians, 32 and 64 faces of the full mesh at 200 x 200, the picture and its truth from pipeline.SynthBatches(colour=True), the maps
from the project's own render at the truth's geometry.

  'basis_build'   = fr_albedo_basis_rgb_build (load time: once per mesh)
  'image'         = fr_albedo_image_rgb
  'light_fit'     = fr_photo_light_lse_rgb_forward (tile kernel and finish-and-solve launch), gated by the truth's lighting
  'albedo_fit'    = fr_albedo_lse_rgb_forward
  'gray_fit'      = fr_albedo_lse_forward on the same faces (the gray, first-order fit; for scale)
  'torch_light', 'torch_albedo' = the same two solves from stock torch ops in float64 (einsum, linalg.solve)
  'copy'          = a device-to-device copy of 512 MiB: the copy rate of THIS run, which prices the bytes below

Beside them the bytes each must move per face: the image reads tri_ind (4 B) and writes 12 B per pixel and gathers the 24 (K + 1) B
basis row per covered pixel; the light fit reads tri_ind at every pixel and tex_img, normal and target (36 B) at a covered one; the
albedo fit reads tri_ind, and normal and target (24 B) plus the basis row at a covered one; each writes its tile partials.

Then ONE photo_solve_rgb(iters=8) from alpha = 0 against 100 Adam steps of examples/photo_fit.py's colour objective from the
truth perturbed (its defaults: light noise 0.2, alpha noise 0.5, lr 0.02), geometry held: wall time around a synchronise, and the
RMS errors of light and alpha against the truth at the end of each.
--out FILE: where the JSON goes besides stdout (default profiles/photo_solve_rgb.json)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--torch-calls", type=int, default=5)
ap.add_argument("--faces", type=int, nargs="+", default=[32, 64])
ap.add_argument("--size", type=int, default=200)
ap.add_argument("--adam-steps", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_solve_rgb.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("photo_solve_rgb_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
pipe = importlib.import_module("3dfacerecon_amd.pipeline")
losses = importlib.import_module("3dfacerecon_amd.nets.losses")
L = h.lib()
dev = torch.device("cuda:0")
S = args.size
COPY_BYTES = 512 << 20
f64 = dict(dtype=torch.float64, device=dev)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / calls * 1e3, 2)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 2), r


def summary(xs):
    return {"us": xs, "median": round(statistics.median(xs), 2), "spread_max_minus_min": round(max(xs) - min(xs), 2)}


def rms(a, b):
    return float((a.detach().double() - b.double()).pow(2).mean().sqrt())


A = synth.make_assets()
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
src, dst = (torch.empty((COPY_BYTES,), dtype=torch.uint8, device=dev) for _ in range(2))
out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=dev)
    K, T, N = net.ndim_tex, int(net.tri.shape[1]), net.nvert
    stream = pipe.SynthBatches(net, B, 77, slots=1, focal=1e-3 * S / 200.0, colour=True)
    b = {k: v.clone() for k, v in stream.next().items()}
    gain, offset = float(stream.gain), float(stream.offset)
    target, light_gt, alpha_gt = b["im_rgb"].contiguous(), b["light"].contiguous(), b["alpha"].contiguous()
    with torch.no_grad():
        V = net.vertices_transform(b["params"])
        _, _, normal, tind = ops.render_depth(V, net.tri, net.mu_tex[None], target)
        a_gray, n_gray, _ = net.compute_abedo_image(V, net.tri, net.mu_tex, with_tri_ind=True)
        lighting = ops.sfs_lighting(a_gray, n_gray, b["im_gray"]).contiguous()
    normal, tind, a_gray, n_gray, im_gray = (x.contiguous() for x in (normal, tind, a_gray, n_gray, b["im_gray"]))
    coverage = float((tind >= 0).float().mean())
    basis = net.albedo_basis_rgb()
    gbasis = net.albedo_basis()
    mu_flat = net.mu_tex.reshape(-1).contiguous()
    nba = L.fr_albedo_basis_rgb_bytes(T, K)
    nws = L.fr_photo_solve_rgb_workspace_bytes(B, S, S)
    ngw = L.fr_albedo_lse_workspace_bytes(B, S, S, K)
    ws = torch.empty((max(nws, ngw),), dtype=torch.uint8, device=dev)
    tex = torch.empty((B, S, S, 3), device=dev)
    light = torch.empty((B, 3, 9), device=dev)
    alpha = torch.empty((B, K), device=dev)
    mom_l, st_l = torch.empty((B, 3, 16, 16), **f64), torch.empty((B, 3, 4), **f64)
    mom_a, st_a = torch.empty((B, 16, 16), **f64), torch.empty((B, 4), **f64)
    scratch = torch.empty((T, 3, K + 1), **f64)

    def basis_build():
        L.fr_albedo_basis_rgb_build(h.ptr(net.tri), h.ptr(mu_flat), h.ptr(net.pc_tex), N, T, K, h.ptr(scratch), nba, st)

    def image():
        L.fr_albedo_image_rgb(h.ptr(basis), h.ptr(tind), h.ptr(alpha_gt), B, T, S, S, K, h.ptr(tex), st)

    def light_fit():
        L.fr_photo_light_lse_rgb_forward(h.ptr(tex), h.ptr(normal), h.ptr(tind), h.ptr(target), None, h.ptr(light_gt), B, S, S, gain,
                                         offset, 0.0, h.ptr(light), h.ptr(mom_l), h.ptr(st_l), h.ptr(ws), nws, st)

    def albedo_fit():
        L.fr_albedo_lse_rgb_forward(h.ptr(basis), h.ptr(tind), h.ptr(normal), h.ptr(light_gt), h.ptr(target), None, B, T, S, S, K, gain,
                                    offset, 0.0, h.ptr(alpha), h.ptr(mom_a), h.ptr(st_a), h.ptr(ws), nws, st)

    def gray_fit():
        L.fr_albedo_lse_forward(h.ptr(gbasis), h.ptr(tind), h.ptr(lighting), h.ptr(n_gray), h.ptr(a_gray), h.ptr(im_gray), B, T, S, S, K,
                                1e-6, h.ptr(alpha), h.ptr(mom_a), h.ptr(st_a), h.ptr(ws), ngw, st)

    t_idx = tind.view(B, -1).long().clamp(0, T - 1)
    cov = (tind.view(B, -1) >= 0)

    def shading():
        n = torch.where(normal[..., 2:3] < 0, -normal, normal).view(B, -1, 3)
        mag = (n * n).sum(-1)
        nh = (n / (torch.where(mag > 1e-6, mag, torch.ones_like(mag)).sqrt() + 1e-6)[..., None]).double()
        hx, hy, hz = nh.unbind(-1)
        return torch.stack([torch.ones_like(hx), hx, hy, hz, hx * hy, hx * hz, hy * hz, hx * hx - hy * hy, 3 * hz * hz - 1], -1)

    def torch_light():
        Hb = shading()
        a = tex.view(B, -1, 3).clamp_min(1e-6).double()
        lit = cov[..., None] & (torch.einsum("bck,bpk->bpc", light_gt.double(), Hb) > 0)
        X = (a[..., None] * Hb[:, :, None, :] * gain) * lit[..., None]                       # [B,npix,3,9]
        y = (target.view(B, -1, 3).double() - offset) * lit
        G = torch.einsum("bpci,bpcj->bcij", X, X)
        return torch.linalg.solve(G, torch.einsum("bpci,bpc->bci", X, y))

    def torch_albedo():
        Hb = shading()
        sp = torch.einsum("bck,bpk->bpc", light_gt.double(), Hb).clamp_min(0) * cov[..., None]
        rows = basis[t_idx]                                                                # [B,npix,3,K+1]
        X = rows[..., :K] * (sp * gain)[..., None]
        y = ((target.view(B, -1, 3).double() - offset) - rows[..., K] * sp * gain) * cov[..., None]
        G = torch.einsum("bpci,bpcj->bij", X, X)
        return torch.linalg.solve(G, torch.einsum("bpci,bpc->bi", X, y))

    def copy():
        dst.copy_(src)

    routes = {"basis_build": basis_build, "image": image, "light_fit": light_fit, "albedo_fit": albedo_fit, "gray_fit": gray_fit,
              "torch_light": torch_light, "torch_albedo": torch_albedo, "copy": copy}
    image()
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.torch_calls if k.startswith("torch_") else args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rate = 2 * COPY_BYTES / (rec["copy"]["median"] * 1e-6)
    rec["copy_rate_bytes_per_s"] = round(rate, -9)
    npix = S * S
    tiles = -(-npix // 256)
    row = 24 * (K + 1)
    must = {"basis_build": T * 3 * (K + 1) * 8 + 3 * N * (K + 1) * 4 + 3 * T * 4,
            "image": int(B * npix * (4 + 12 + row * coverage)),
            "light_fit": int(B * npix * (4 + 36 * coverage) + 2 * B * tiles * 3 * 257 * 8),
            "albedo_fit": int(B * npix * (4 + (24 + row) * coverage) + 2 * B * tiles * 257 * 8)}
    for k, v in must.items():
        rec[k + "_vs_bytes"] = {"must_move": v, "time_at_copy_rate_us": round(v / rate * 1e6, 2),
                                "fraction_of_copy_rate": round(v / rate * 1e6 / rec[k]["median"], 3)}
    light_fit()
    albedo_fit()
    tl, ta = torch_light(), torch_albedo()
    rec["fits_vs_torch"] = {"coverage": round(coverage, 3), "light_units_ok": int((st_l[:, :, 3] == 1).sum()),
                            "faces_ok": int((st_a[:, 3] == 1).sum()),
                            "largest_relative_difference_of_light": float(((light.double() - tl).abs().amax(2) / tl.abs().amax(2)).max()),
                            "largest_relative_difference_of_alpha": float(((alpha.double() - ta).abs().amax(1) / ta.abs().amax(1)).max()),
                            "torch_light_over_light_fit": round(rec["torch_light"]["median"] / rec["light_fit"]["median"], 1),
                            "torch_albedo_over_albedo_fit": round(rec["torch_albedo"]["median"] / rec["albedo_fit"]["median"], 1)}

    # ---- the loop against Adam -----------------------------------------------------------------------------------------------------
    def solve():
        return ops.photo_solve_rgb(basis, tind, normal, target, iters=8, gain=gain, offset=offset)
    solve()
    ms_solve, (lf, af, _, info) = wall(solve)
    g = torch.Generator().manual_seed(77)
    l_fit = (light_gt + 0.2 * torch.randn(light_gt.shape, generator=g).to(dev)).requires_grad_(True)
    a_fit = (alpha_gt + 0.5 * torch.randn(alpha_gt.shape, generator=g).to(dev)).requires_grad_(True)
    start = {"light_rms": rms(l_fit, light_gt), "alpha_rms": rms(a_fit, alpha_gt)}
    opt = torch.optim.Adam([l_fit, a_fit], lr=0.02)

    def adam():
        for _ in range(args.adam_steps):
            opt.zero_grad(set_to_none=True)
            losses.photometric_loss(net, V, target, l_fit, a_fit, gain=gain, offset=offset).backward()
            opt.step()
    ms_adam, _ = wall(adam)
    rec["solve_vs_adam"] = {"photo_solve_rgb_iters8_ms": ms_solve, "adam_%d_steps_ms" % args.adam_steps: ms_adam,
                            "solve": {"light_rms": rms(lf, light_gt), "alpha_rms": rms(af, alpha_gt), "ok": bool(info["ok"].all()),
                                      "E_first": float(info["E"][0, 0].sum()), "E_last": float(info["E"][-1, 1].sum())},
                            "adam_start": start, "adam_end": {"light_rms": rms(l_fit, light_gt), "alpha_rms": rms(a_fit, alpha_gt)}}
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)
    del net

geo = (ctypes.c_int * 6)()
L.fr_debug_photo_solve_rgb_geom(args.faces[-1], S, S, geo)
doc = {"what": "us per call, device events around %d calls per figure (%d for torch_*), %d alternating rounds, one process, full mesh, "
               "%d x %d; copy = a 512 MiB device-to-device copy, copy_rate = 2 x 512 MiB / its median; must_move = the bytes any "
               "scheme moves, fraction_of_copy_rate = (must_move / copy_rate) / time; solve_vs_adam: wall ms around a synchronise"
               % (args.calls, args.torch_calls, args.rounds, S, S),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
       "geometry_at_%d_faces" % args.faces[-1]: dict(zip(("pixels_per_tile", "tiles_per_face", "tile_workgroups",
                                                         "light_finish_workgroups", "albedo_finish_workgroups", "finish_lds_bytes"), geo)),
       "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
