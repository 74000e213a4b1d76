#!/usr/bin/env python3
"""What the colour route costs beside the gray one, in ONE process (modelled on tools/photo_loss_probe.py): alternating rounds, device
events, medians; 32 and 64 faces of the full mesh rendered at 200 x 200 from sampled parameters (synth_params -> decode ->
synth_texture -> render_depth), the targets independent images.  Both routes run on the SAME planes.

  'shade_gray' / 'shade_rgb'       = fr_synth_shade / fr_synth_shade_rgb (im_rgb, im_gray and mask)
  'fwd_gray' / 'fwd_rgb'           = fr_photo_loss_forward / fr_photo_loss_rgb_forward through the raw C ABI (the pass and the finish launch)
  'bwd_gray' / 'bwd_rgb'           = fr_photo_loss_backward / fr_photo_loss_rgb_backward, all three gradients
  'parent_' + each of the six     = the same call into a SECOND library, the parent commit's whole library built with the project's
                                     flags (--parent-lib; left out when the file is not there), in the same alternating rounds.  With
                                     it the probe also compares every output of the pair's ten entry points with the parent's bit
                                     for bit (bits_against_parent) and exits with status 1 where one differs: a refactor of the
                                     shading models must not move a bit, and a microsecond only within the run's own spread
  'torch_rgb_fwd_bwd'              = the stock-torch composition of the colour term under autograd, into tex_img, normal and light
  'copy'                           = a 512 MiB device-to-device copy; copy_rate = 2 x 512 MiB / its median

Beside them the bytes each kernel must move with the coverage as measured, their time at the copy rate of the same run, and each kernel
as a multiple of that floor.  Recorded, no threshold.

--out FILE: where the JSON goes besides stdout (default profiles/photo_rgb.json)."""
import argparse
import collections
import ctypes
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[32, 64])
ap.add_argument("--size", type=int, default=200)
ap.add_argument("--small", action="store_true", help="the tiny assets (a rehearsal of the program, not a measurement)")
ap.add_argument("--parent-lib", default=None, help="the parent commit's whole library, built with the project's flags")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_rgb.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("photo_rgb_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
L = h.lib()
# the two models as the ten entry points see them: the names' suffix, the sums per face, a face's lighting, the image's channels
Model = collections.namedtuple("Model", "suffix sums light channels")
GRAY, RGB = Model("", 6, (4,), 1), Model("_rgb", 29, (3, 9), 3)
PARENT = None
if args.parent_lib and os.path.exists(args.parent_lib):
    PARENT = h.bind(ctypes.CDLL(args.parent_lib), [n % m.suffix for m in (GRAY, RGB) for n in (
        "fr_synth_shade%s", "fr_photo_loss%s_state_bytes", "fr_photo_loss%s_forward", "fr_photo_loss%s_backward", "fr_debug_photo_loss%s_geom")])
dev = torch.device("cuda:0")
S = args.size
GAIN, OFFSET = 1.0, 0.0


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def bits_against_parent():
    """Every output of the ten entry points, this library's against the parent's, bit for bit (NaN patterns included), on planes that
    reach every branch of both models (tests/ref_photo_loss.py, tests/ref_photo_rgb.py: the first seed whose planes do) at B = 3,
    17 x 33 (three tiles, the last one partial), and on B = 1, 16 x 16 (exactly one tile) and B = 1, 1 x 1 (covered): the shaders
    with no background, one for all faces and one per face; the forwards with and without weight; the backwards with each single
    gradient asked for alone and all three together.  Every output starts as the same NaN fill for both libraries.
    -> {"cases": how many outputs were compared, "differing": the labels of those with a differing bit}"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    RP, RC = importlib.import_module("ref_photo_loss"), importlib.import_module("ref_photo_rgb")
    cases, differing = 0, []

    def dev_t(a, dtype=torch.float32):
        return torch.as_tensor(a).to(device=dev, dtype=dtype).contiguous()

    def nan(shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), dtype=dtype, device=dev)

    def both(label, call, outs):
        """call(lib, tensors) on fresh NaN-filled outputs for each library"""
        nonlocal cases
        got = []
        for lib in (L, PARENT):
            ts = [nan(shape, dtype) for shape, dtype in outs]
            rc = call(lib, ts)
            torch.cuda.synchronize()
            got.append((rc, ts))
        for k, (a, b) in enumerate(zip(got[0][1], got[1][1])):
            cases += 1
            if got[0][0] != got[1][0] or not same_bits(a, b):
                differing.append("%s, output %d" % (label, k))

    reach = {}
    for B, H, W in ((3, 17, 33), (1, 16, 16), (1, 1, 1)):
        big = H >= 3 and W >= 4
        for seed in range(64 if big else 1):
            gray = RP.hand_planes(B, H, W, seed)
            rgb = RC.hand_planes_rgb(B, H, W, seed) if big else None
            if not big or (RP.reaches_every_branch(*gray[:4]) and RC.reaches_every_branch(*rgb[:4], rgb[5])):
                break
        if big:
            reach["B%d-%dx%d" % (B, H, W)] = {"seed": seed, "gray": RP.reaches_every_branch(*gray[:4]),
                                              "rgb": RC.reaches_every_branch(*rgb[:4], rgb[5])}
        else:                                    # too small for the colour planes' hand-set pixels: the gray planes, every pixel covered
            rs = np.random.RandomState(B * H * W)
            gray[2][...] = 3.0
            rgb = gray[:3] + (rs.uniform(-1, 1, (B, 3, 9)), rs.uniform(0, 1, (B, H, W, 3)), gray[5])
        g_sse = dev_t([1.0, -0.75, 0.5][:B], torch.float64)
        for name, m, planes in (("gray", GRAY, gray), ("rgb", RGB, rgb)):
            tex, nrm, ti, light, target, weight = (dev_t(x) for x in planes)
            inputs = [h.ptr(t) for t in (tex, nrm, ti, light)]
            what = "%s B%d-%dx%d" % (name, B, H, W)
            f32 = torch.float32
            shade_outs = [((B, H, W, c), f32) for c in ((3,) if m.channels == 3 else ()) + (1, 1)]
            for bgb in (0, 1, B):
                bg = None if bgb == 0 else dev_t(np.random.RandomState(bgb).uniform(0, 1, (bgb, H, W, m.channels)))
                both("%s shade, background %d" % (what, bgb), lambda lib, ts: getattr(lib, "fr_synth_shade" + m.suffix)(
                    *inputs, h.ptr(bg), bgb, B, H, W, 1.75, -0.125, *[h.ptr(t) for t in ts], st), shade_outs)
            for w in (None, weight):
                label = "%s, weight %s" % (what, "none" if w is None else "given")

                def fwd(lib, ts):
                    nst = getattr(lib, "fr_photo_loss%s_state_bytes" % m.suffix)(B, H, W)
                    state = torch.empty((nst,), dtype=torch.uint8, device=dev)
                    return getattr(lib, "fr_photo_loss%s_forward" % m.suffix)(*inputs, h.ptr(target), h.ptr(w), B, H, W, 1.75, -0.125,
                                                                              h.ptr(ts[0]), h.ptr(state), nst, st)
                both(label + " forward", fwd, [((B, m.sums), torch.float64)])
                sums = nan((B, m.sums), torch.float64)
                fwd(L, [sums])
                for wants in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                    both("%s backward, gradients %s" % (label, wants), lambda lib, ts: getattr(lib, "fr_photo_loss%s_backward" % m.suffix)(
                        h.ptr(g_sse), h.ptr(sums), *inputs, h.ptr(target), h.ptr(w), B, H, W, 1.75, -0.125,
                        *[h.ptr(t) if on else None for t, on in zip(ts, wants)], st),
                        [((B, H, W, 3), f32), ((B, H, W, 3), f32), ((B,) + m.light, f32)])
            geo = [(ctypes.c_int * 4)(), (ctypes.c_int * 4)()]
            for lib, g in zip((L, PARENT), geo):
                getattr(lib, "fr_debug_photo_loss%s_geom" % m.suffix)(B, H, W, g)
            cases += 1
            if list(geo[0]) != list(geo[1]):
                differing.append(what + " geometry")
    return {"cases": cases, "differing": differing, "planes_reach_every_branch": reach}


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

    def routes_of(lib, prefix=""):
        """one library's six calls on this input -> {figure: call}, {figure: the tensors it writes}, {model: its state's bytes}"""
        calls, writes, state_bytes = {}, {}, {}
        for name, m, light, target, planes in (("gray", GRAY, light4, target1, (im_gray, mask)),
                                               ("rgb", RGB, light27, target3, (im_rgb, im_gray, mask))):
            nst = getattr(lib, "fr_photo_loss%s_state_bytes" % m.suffix)(B, S, S)
            state = torch.empty((nst,), dtype=torch.uint8, device=dev)
            sums = torch.full((B, m.sums), float("nan"), dtype=torch.float64, device=dev)
            gl = torch.empty_like(light)
            shade_fn = getattr(lib, "fr_synth_shade" + m.suffix)
            fwd_fn, bwd_fn = getattr(lib, "fr_photo_loss%s_forward" % m.suffix), getattr(lib, "fr_photo_loss%s_backward" % m.suffix)
            inputs = base + [h.ptr(light)]

            def shade(shade_fn=shade_fn, inputs=inputs, planes=planes):
                shade_fn(*inputs, None, 0, B, S, S, GAIN, OFFSET, *[h.ptr(p) for p in planes], st)

            def fwd(fwd_fn=fwd_fn, inputs=inputs, target=target, sums=sums, state=state, nst=nst):
                fwd_fn(*inputs, h.ptr(target), None, B, S, S, GAIN, OFFSET, h.ptr(sums), h.ptr(state), nst, st)

            def bwd(bwd_fn=bwd_fn, inputs=inputs, target=target, sums=sums, gl=gl):
                bwd_fn(h.ptr(g_sse), h.ptr(sums), *inputs, h.ptr(target), None, B, S, S, GAIN, OFFSET, h.ptr(gt), h.ptr(gn), h.ptr(gl), st)
            for figure, fn, out_t in (("shade", shade, planes), ("fwd", fwd, (sums,)), ("bwd", bwd, (gt, gn, gl))):
                calls["%s%s_%s" % (prefix, figure, name)] = fn
                writes["%s_%s" % (figure, name)] = out_t
            state_bytes[name] = int(nst)
        return calls, writes, state_bytes

    def snapshot(calls, writes, prefix=""):
        """runs the six calls in order (shade, fwd, bwd per model: a backward reads its forward's sums) -> {figure: copies of what it wrote}"""
        got = {}
        for figure, tensors in writes.items():
            calls[prefix + figure]()
            torch.cuda.synchronize()
            got[figure] = [t.clone() for t in tensors]
        return got

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

    routes, writes, state_bytes = routes_of(L)
    routes.update(torch_rgb_fwd_bwd=torch_rgb_fwd_bwd, copy=copy)
    if PARENT is not None:
        parent_calls, parent_writes, _ = routes_of(PARENT, "parent_")
        routes.update(parent_calls)
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the routes beside each other on this input (recorded, not asserted; the tests hold the kernels to their model)
    parent = None
    if PARENT is not None:
        theirs = snapshot(routes, parent_writes, "parent_")
    mine = snapshot(routes, writes)              # (last: the colour backward's gradients stay in gt and gn for the comparison with torch)
    if PARENT is not None:
        parent = {"same_bits": {k: bool(all(same_bits(a, b) for a, b in zip(mine[k], theirs[k]))) for k in mine}}
    sums_rgb, gl_rgb = mine["fwd_rgb"][0], mine["bwd_rgb"][2]
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
        # the margin is this run's own spread: the larger of the two figures' max - min
        for k in must:
            a, b = rec[k], rec["parent_" + k]
            margin = max(a["spread_max_minus_min"], b["spread_max_minus_min"])
            parent[k] = {"median": a["median"], "parent_median": b["median"], "difference_us": round(a["median"] - b["median"], 2),
                         "margin_us": margin, "no_slower_within_the_margin": bool(a["median"] - b["median"] <= margin)}
        rec["against_parent"] = parent
    rec["losses"] = {"torch": lt, "fused": lf, "relative_difference": abs(lt - lf) / abs(lf),
                     "largest_gradient_difference_over_largest_gradient": {
                         name: float((a - b).abs().max() / b.abs().max())
                         for name, a, b in zip(("tex_img", "normal", "light"), grads_t, grads_f)}}
    rec["state_bytes"] = state_bytes
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

geo = (ctypes.c_int * 4)()
L.fr_debug_photo_loss_rgb_geom(args.faces[-1], S, S, geo)
doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, %s mesh, %d x %d, both routes on "
               "the same planes; shade_* = fr_synth_shade / fr_synth_shade_rgb; fwd_* / bwd_* = fr_photo_loss[_rgb]_forward (both launches) / "
               "_backward (all three gradients) through the raw C ABI; parent_* = the same call into the parent commit's library; "
               "against_parent: per figure the medians, their difference and the margin (the larger of the two spreads of this run); "
               "torch_rgb_fwd_bwd = the stock-torch composition of the colour term under autograd; copy = a 512 MiB "
               "device-to-device copy, copy_rate = 2 x 512 MiB / its median; must_move: forward 32 (gray) or 40 (colour) B per covered "
               "pixel and 4 per uncovered one, backward plus 24 B written per pixel; the shaders read 28 or 4 B and write 8 (gray) or 20 "
               "(colour) per pixel" % (args.calls, args.rounds, "small" if args.small else "full", S, S),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "parent_lib": bool(PARENT is not None),
       "geometry_at_%d_faces" % args.faces[-1]: dict(zip(("pixels_per_tile", "tiles_per_face", "finish_threads", "sums_per_face"), geo)),
       "results": out}
if PARENT is not None:
    doc["bits_against_parent"] = bits_against_parent()
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
if PARENT is not None and doc["bits_against_parent"]["differing"]:
    raise SystemExit("photo_rgb_probe: %d outputs differ from the parent library's" % len(doc["bits_against_parent"]["differing"]))
