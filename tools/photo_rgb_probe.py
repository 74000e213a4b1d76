#!/usr/bin/env python3
"""What the colour route costs beside the gray one, in ONE process (modelled on tools/photo_loss_probe.py): alternating rounds, device
events, medians; 32 and 64 faces of the full mesh rendered at 200 x 200 from sampled parameters (synth_params -> decode ->
synth_texture -> render_depth), the targets independent images.  Both routes run on the SAME planes.

  'shade_gray' / 'shade_rgb'       = fr_synth_shade / fr_synth_shade_rgb (im_rgb, im_gray and mask)
  'fwd_gray' / 'fwd_rgb'           = fr_photo_loss_forward / fr_photo_loss_rgb_forward through the raw C ABI (the pass and the finish launch)
  'bwd_gray' / 'bwd_rgb'           = fr_photo_loss_backward / fr_photo_loss_rgb_backward, all three gradients
  'parent_fwd_gray' / 'parent_bwd_gray' = the gray loss of a SECOND library built from the parent commit's csrc/fr_photo.hip alone
                                     (--parent-lib; left out when the file is not there): the refactor that made the tile tree and the
                                     finish kernel templates must not move a bit or a microsecond
  'torch_rgb_fwd_bwd'              = the stock-torch composition of the colour term under autograd, into tex_img, normal and light
  'copy'                           = a 512 MiB device-to-device copy; copy_rate = 2 x 512 MiB / its median

Beside them the bytes each kernel must move with the coverage as measured, their time at the copy rate of the same run, and each kernel
as a multiple of that floor.  Recorded, no threshold.

--out FILE: where the JSON goes besides stdout (default profiles/photo_rgb.json)."""
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
ap.add_argument("--faces", type=int, nargs="+", default=[32, 64])
ap.add_argument("--size", type=int, default=200)
ap.add_argument("--small", action="store_true", help="the tiny assets (a rehearsal of the program, not a measurement)")
ap.add_argument("--parent-lib", default=None, help="a shared library built from the parent commit's csrc/fr_photo.hip")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_rgb.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("photo_rgb_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
L = h.lib()
PARENT = None
if args.parent_lib and os.path.exists(args.parent_lib):
    PARENT = h.bind(ctypes.CDLL(args.parent_lib), ["fr_photo_loss_state_bytes", "fr_photo_loss_forward", "fr_photo_loss_backward"])
dev = torch.device("cuda:0")
S = args.size
GAIN, OFFSET = 1.0, 0.0


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


A = synth.make_small_assets() if args.small else synth.make_assets()
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
copy_src = torch.empty((512 << 20,), dtype=torch.uint8, device=dev)
copy_dst = torch.empty_like(copy_src)
out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=dev)
    K = int(net.pc_tex.shape[1])
    P, light4, alpha = ops.synth_params(11, 0, B, net.ndim_shape, net.ndim_exp, K, S, focal=1e-3 * S / 200.0 if args.small else 1e-3,
                                        device=dev)
    light27 = ops.synth_light_rgb(11, 0, B, device=dev)
    with torch.no_grad():
        tex = ops.synth_texture(net.mu_tex, net.pc_tex, alpha)
        _, tex_img, normal, tri_ind = ops.render_depth(net.vertices_transform(P), net.tri, tex, torch.zeros((B, S, S, 1), device=dev))
    gen = torch.Generator().manual_seed(B)
    target1 = torch.rand((B, S, S, 1), generator=gen).to(dev)
    target3 = torch.rand((B, S, S, 3), generator=gen).to(dev)
    covered = int((tri_ind >= 0).sum())
    npix = B * S * S
    f32 = dict(dtype=torch.float32, device=dev)
    g_sse = torch.full((B,), 1.0 / max(covered, 1), dtype=torch.float64, device=dev)
    gt, gn = torch.empty_like(tex_img), torch.empty_like(normal)
    im_gray, mask, im_rgb = torch.empty((B, S, S, 1), **f32), torch.empty((B, S, S, 1), **f32), torch.empty((B, S, S, 3), **f32)
    base = [h.ptr(t) for t in (tex_img, normal, tri_ind)]

    def loss_calls(lib, suffix, nsums, light, target):
        nst = getattr(lib, "fr_photo_loss%s_state_bytes" % suffix)(B, S, S)
        state = torch.empty((nst,), dtype=torch.uint8, device=dev)
        sums = torch.full((B, nsums), float("nan"), dtype=torch.float64, device=dev)
        gl = torch.empty_like(light)
        fwd_fn, bwd_fn = getattr(lib, "fr_photo_loss%s_forward" % suffix), getattr(lib, "fr_photo_loss%s_backward" % suffix)
        planes = base + [h.ptr(light), h.ptr(target)]

        def fwd():
            fwd_fn(*planes, None, B, S, S, GAIN, OFFSET, h.ptr(sums), h.ptr(state), nst, st)

        def bwd():
            bwd_fn(h.ptr(g_sse), h.ptr(sums), *planes, None, B, S, S, GAIN, OFFSET, h.ptr(gt), h.ptr(gn), h.ptr(gl), st)
        return fwd, bwd, sums, gl, (state, nst)

    fwd_gray, bwd_gray, sums_gray, gl_gray, keep1 = loss_calls(L, "", 6, light4, target1)
    fwd_rgb, bwd_rgb, sums_rgb, gl_rgb, keep2 = loss_calls(L, "_rgb", 29, light27, target3)

    def shade_gray():
        L.fr_synth_shade(*base, h.ptr(light4), None, 0, B, S, S, GAIN, OFFSET, h.ptr(im_gray), h.ptr(mask), st)

    def shade_rgb():
        L.fr_synth_shade_rgb(*base, h.ptr(light27), None, 0, B, S, S, GAIN, OFFSET, h.ptr(im_rgb), h.ptr(im_gray), h.ptr(mask), st)

    tex_l, nrm_l, light_l = (t.clone().requires_grad_(True) for t in (tex_img, normal, light27))
    cov_f = (tri_ind >= 0).float()

    def torch_rgb_loss():
        a = torch.clamp_min(tex_l, 1e-6)
        n = torch.where(nrm_l[..., 2:3] < 0, -1.0 * nrm_l, nrm_l)
        mag = (n * n).sum(-1)
        mag = torch.where(mag > 1e-6, mag, torch.ones_like(mag))
        nm = n / (torch.sqrt(mag) + 1e-6)[..., None]
        hx, hy, hz = nm[..., 0], nm[..., 1], nm[..., 2]
        Hb = torch.stack([torch.ones_like(hx), hx, hy, hz, hx * hy, hx * hz, hy * hz, hx * hx - hy * hy, 3.0 * hz * hz - 1.0], -1)
        s = torch.einsum("bck,bhwk->bhwc", light_l, Hb)
        im = a * torch.relu(s) * GAIN + OFFSET
        r = (im - target3) * cov_f
        return (r * r).sum() / (3 * cov_f.sum()).clamp_min(1)

    def torch_rgb_fwd_bwd():
        tex_l.grad = nrm_l.grad = light_l.grad = None
        torch_rgb_loss().backward()

    def copy():
        copy_dst.copy_(copy_src)

    routes = {"shade_gray": shade_gray, "shade_rgb": shade_rgb, "fwd_gray": fwd_gray, "fwd_rgb": fwd_rgb, "bwd_gray": bwd_gray,
              "bwd_rgb": bwd_rgb, "torch_rgb_fwd_bwd": torch_rgb_fwd_bwd, "copy": copy}
    parent = None
    if PARENT is not None:
        pf, pb, sums_parent, gl_parent, keep3 = loss_calls(PARENT, "", 6, light4, target1)
        routes.update(parent_fwd_gray=pf, parent_bwd_gray=pb)
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the routes beside each other on this input (recorded, not asserted; the tests hold the kernels to their model)
    fwd_gray()
    bwd_gray()
    torch.cuda.synchronize()
    if PARENT is not None:
        mine = [sums_gray.clone(), gt.clone(), gn.clone(), gl_gray.clone()]
        pf()
        pb()
        torch.cuda.synchronize()
        parent = {"same_bits": bool(all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                                        for a, b in zip(mine, (sums_parent, gt, gn, gl_parent))))}
    fwd_rgb()
    bwd_rgb()
    torch.cuda.synchronize()
    lf = float(sums_rgb[:, 0].sum() / (3 * sums_rgb[:, 1].sum()).clamp_min(1))
    grads_f = [gt.clone() * 1.0, gn.clone() * 1.0, gl_rgb.clone() * 1.0]
    torch_rgb_fwd_bwd()
    lt = float(torch_rgb_loss().detach())
    scale = float(g_sse[0]) * 3 * covered          # the kernels ran with grad_sse = 1 / covered; the torch loss is the mean over 3 covered
    grads_t = [t.grad.clone() * scale for t in (tex_l, nrm_l, light_l)]
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls if k != "copy" else max(args.calls // 4, 1)))
    rec = {k: summary(v) for k, v in res.items()}
    copy_rate = 2 * (512 << 20) / (rec["copy"]["median"] * 1e-6)
    unc = npix - covered
    must = {"shade_gray": 28 * covered + 4 * unc + 8 * npix, "shade_rgb": 28 * covered + 4 * unc + 20 * npix,
            "fwd_gray": 32 * covered + 4 * unc, "fwd_rgb": 40 * covered + 4 * unc,
            "bwd_gray": 32 * covered + 4 * unc + 24 * npix, "bwd_rgb": 40 * covered + 4 * unc + 24 * npix}
    rec["coverage"] = round(covered / npix, 4)
    rec["copy_rate_bytes_per_s"] = round(copy_rate, 0)
    rec["bytes"] = {k: {"must_move": v, "time_at_copy_rate_us": round(v / copy_rate * 1e6, 2)} for k, v in must.items()}
    rec["ratio_to_byte_floor"] = {k: round(rec[k]["median"] / rec["bytes"][k]["time_at_copy_rate_us"], 2) for k in must}
    rec["torch_over_kernels_rgb_fwd_bwd"] = round(rec["torch_rgb_fwd_bwd"]["median"] / (rec["fwd_rgb"]["median"] + rec["bwd_rgb"]["median"]), 2)
    if parent is not None:
        for d in ("fwd", "bwd"):
            a, b = rec["%s_gray" % d], rec["parent_%s_gray" % d]
            parent["%s_median_difference_us" % d] = round(a["median"] - b["median"], 2)
            parent["%s_within_the_runs_spread" % d] = bool(abs(a["median"] - b["median"]) <= max(a["spread_max_minus_min"],
                                                                                                 b["spread_max_minus_min"]))
        rec["parent_gray_loss"] = parent
    rec["losses"] = {"torch": lt, "fused": lf, "relative_difference": abs(lt - lf) / abs(lf),
                     "largest_gradient_difference_over_largest_gradient": {
                         name: float((a - b).abs().max() / b.abs().max())
                         for name, a, b in zip(("tex_img", "normal", "light"), grads_t, grads_f)}}
    rec["state_bytes"] = {"gray": int(keep1[1]), "rgb": int(keep2[1])}
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

geo = (ctypes.c_int * 4)()
L.fr_debug_photo_loss_rgb_geom(args.faces[-1], S, S, geo)
doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, %s mesh, %d x %d, both routes on "
               "the same planes; shade_* = fr_synth_shade / fr_synth_shade_rgb; fwd_* / bwd_* = fr_photo_loss[_rgb]_forward (both launches) / "
               "_backward (all three gradients) through the raw C ABI; parent_* = the gray loss of a second library built from the parent "
               "commit's fr_photo.hip; torch_rgb_fwd_bwd = the stock-torch composition of the colour term under autograd; copy = a 512 MiB "
               "device-to-device copy, copy_rate = 2 x 512 MiB / its median; must_move: forward 32 (gray) or 40 (colour) B per covered "
               "pixel and 4 per uncovered one, backward plus 24 B written per pixel; the shaders read 28 or 4 B and write 8 (gray) or 20 "
               "(colour) per pixel" % (args.calls, args.rounds, "small" if args.small else "full", S, S),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "parent_lib": bool(PARENT is not None),
       "geometry_at_%d_faces" % args.faces[-1]: dict(zip(("pixels_per_tile", "tiles_per_face", "finish_threads", "sums_per_face"), geo)),
       "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
