#!/usr/bin/env python3
"""What the photometric term costs on its two routes, in ONE process (modelled on tools/fine_losses_probe.py): alternating rounds,
device events, medians; 32 and 64 faces of the full mesh rendered at 200 x 200 from sampled parameters (synth_params -> decode ->
synth_texture -> render_depth), the target an independent image.

  'kernels_fwd'        = fr_photo_loss_forward through the raw C ABI (the pass and the finish launch)
  'kernels_bwd'        = fr_photo_loss_backward through the raw C ABI, all three gradients
  'kernels_fwd_bwd'    = the three launches together
  'operator_fwd_bwd'   = ops.photo_loss(...), sse.sum() / count.sum() and its backward into tex_img, normal and light (the autograd
                         node; outputs and gradients allocated per call)
  'torch_fwd_bwd'      = the stock-torch composition of the same term: the formula of
                         tests/test_synth_batch_gpu.py::test_shade_against_the_stock_torch_composition, gain and offset, then a masked
                         mean squared error, and its backward into the same three tensors
  'texture_bwd'        = fr_synth_texture_backward (both launches);  'texture_bwd_matmul' = grad.reshape(B, -1) @ pc_tex
  'copy'               = a 512 MiB device-to-device copy; copy_rate = 2 x 512 MiB / its median

Beside them the bytes each direction must move with the coverage as measured -- forward 32 B per covered pixel (tex_img, normal,
tri_ind, target) and 4 per uncovered one; backward the same plus 24 B written per pixel -- and their time at the copy rate of the same
run.  Recorded, no threshold.

--out FILE: where the JSON goes besides stdout (default profiles/photo_loss.json)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_loss.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("photo_loss_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
L = h.lib()
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
    N = int(net.mu_tex.shape[1])
    P, light, alpha = ops.synth_params(11, 0, B, net.ndim_shape, net.ndim_exp, K, S, focal=1e-3 * S / 200.0 if args.small else 1e-3, device=dev)
    with torch.no_grad():
        tex = ops.synth_texture(net.mu_tex, net.pc_tex, alpha)
        _, tex_img, normal, tri_ind = ops.render_depth(net.vertices_transform(P), net.tri, tex, torch.zeros((B, S, S, 1), device=dev))
    target = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(B)).to(dev)
    covered = int((tri_ind >= 0).sum())
    npix = B * S * S
    nst = L.fr_photo_loss_state_bytes(B, S, S)
    state = torch.empty((nst,), dtype=torch.uint8, device=dev)
    sums = torch.empty((B, 6), dtype=torch.float64, device=dev)
    g_sse = torch.full((B,), 1.0 / max(covered, 1), dtype=torch.float64, device=dev)
    gt, gn, gl = torch.empty_like(tex_img), torch.empty_like(normal), torch.empty_like(light)
    planes = [h.ptr(t) for t in (tex_img, normal, tri_ind, light, target)]
    tex_l, nrm_l, light_l = (t.clone().requires_grad_(True) for t in (tex_img, normal, light))
    mask = (tri_ind >= 0).float()
    g_tex = torch.randn((B, 3, N), generator=torch.Generator().manual_seed(B + 1)).to(dev)
    g_alpha = torch.empty((B, K), dtype=torch.float32, device=dev)
    nws = L.fr_synth_texture_backward_workspace_bytes(B, N, K)
    ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=dev)
    pc = net.pc_tex.contiguous()

    def kernels_fwd():
        L.fr_photo_loss_forward(*planes, None, B, S, S, GAIN, OFFSET, h.ptr(sums), h.ptr(state), nst, st)

    def kernels_bwd():
        L.fr_photo_loss_backward(h.ptr(g_sse), h.ptr(sums), *planes, None, B, S, S, GAIN, OFFSET, h.ptr(gt), h.ptr(gn), h.ptr(gl), st)

    def kernels_fwd_bwd():
        kernels_fwd()
        kernels_bwd()

    def operator_fwd_bwd():
        tex_l.grad = nrm_l.grad = light_l.grad = None
        sse, cnt = ops.photo_loss(tex_l, nrm_l, tri_ind, light_l, target, None, GAIN, OFFSET)
        (sse.sum() / cnt.sum().clamp_min(1)).backward()

    def torch_loss():
        a = torch.clamp_min(tex_l, 1e-6).mean(dim=-1, keepdim=True)
        n = torch.where(nrm_l[..., 2:3] < 0, -1.0 * nrm_l, nrm_l)
        mag = (n * n).sum(-1)
        mag = torch.where(mag > 1e-6, mag, torch.ones_like(mag))
        nm = n / (torch.sqrt(mag) + 1e-6)[..., None]
        s = light_l[:, None, None, 0:1] + (light_l[:, None, None, 1:4] * nm).sum(-1, keepdim=True)
        im = a * torch.relu(s) * GAIN + OFFSET
        r = (im - target) * mask
        return (r * r).sum() / mask.sum().clamp_min(1)

    def torch_fwd_bwd():
        tex_l.grad = nrm_l.grad = light_l.grad = None
        torch_loss().backward()

    def texture_bwd():
        L.fr_synth_texture_backward(h.ptr(pc), h.ptr(g_tex), B, N, K, h.ptr(g_alpha), h.ptr(ws), nws, st)

    def texture_bwd_matmul():
        return g_tex.reshape(B, -1) @ pc

    def copy():
        copy_dst.copy_(copy_src)

    routes = {"kernels_fwd": kernels_fwd, "kernels_bwd": kernels_bwd, "kernels_fwd_bwd": kernels_fwd_bwd,
              "operator_fwd_bwd": operator_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd, "texture_bwd": texture_bwd,
              "texture_bwd_matmul": texture_bwd_matmul, "copy": copy}
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the two routes beside each other on this input (recorded, not asserted; the tests hold the kernels to their model)
    torch_fwd_bwd()
    lt = float(torch_loss().detach())
    grads_t = [t.grad.clone() for t in (tex_l, nrm_l, light_l)]
    operator_fwd_bwd()
    kernels_fwd()
    lf = float(sums[:, 0].sum() / sums[:, 1].sum().clamp_min(1))
    grads_f = [t.grad.clone() for t in (tex_l, nrm_l, light_l)]
    texture_bwd()
    ga_mm = texture_bwd_matmul()
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls if k != "copy" else max(args.calls // 4, 1)))
    rec = {k: summary(v) for k, v in res.items()}
    copy_rate = 2 * (512 << 20) / (rec["copy"]["median"] * 1e-6)
    must = {"forward": 32 * covered + 4 * (npix - covered), "backward": 32 * covered + 4 * (npix - covered) + 24 * npix}
    rec["coverage"] = round(covered / npix, 4)
    rec["copy_rate_bytes_per_s"] = round(copy_rate, 0)
    rec["bytes"] = {k: {"must_move": v, "time_at_copy_rate_us": round(v / copy_rate * 1e6, 2)} for k, v in must.items()}
    rec["ratio_to_byte_floor"] = {"forward": round(rec["kernels_fwd"]["median"] / rec["bytes"]["forward"]["time_at_copy_rate_us"], 2),
                                  "backward": round(rec["kernels_bwd"]["median"] / rec["bytes"]["backward"]["time_at_copy_rate_us"], 2)}
    rec["torch_over_kernels_fwd_bwd"] = round(rec["torch_fwd_bwd"]["median"] / rec["kernels_fwd_bwd"]["median"], 2)
    rec["torch_over_operator_fwd_bwd"] = round(rec["torch_fwd_bwd"]["median"] / rec["operator_fwd_bwd"]["median"], 2)
    rec["matmul_over_texture_bwd"] = round(rec["texture_bwd_matmul"]["median"] / rec["texture_bwd"]["median"], 2)
    rec["losses"] = {"torch": lt, "fused": lf, "relative_difference": abs(lt - lf) / abs(lf),
                     "largest_gradient_difference_over_largest_gradient": {
                         name: float((a - b).abs().max() / b.abs().max())
                         for name, a, b in zip(("tex_img", "normal", "light"), grads_t, grads_f)},
                     "texture_bwd_vs_matmul": float((ga_mm - g_alpha).abs().max() / g_alpha.abs().max())}
    rec["state_bytes"], rec["texture_bwd_workspace_bytes"] = int(nst), int(nws)
    rec["mesh"] = {"N": N, "K": K}
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

geo = (ctypes.c_int * 4)()
L.fr_debug_photo_loss_geom(args.faces[-1], S, S, geo)
doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, %s mesh, %d x %d; kernels_* = "
               "fr_photo_loss_forward (both launches) / _backward (all three gradients) through the raw C ABI; operator_fwd_bwd = "
               "ops.photo_loss, the mean and its backward (autograd node); torch_fwd_bwd = the stock-torch composition of the same term "
               "under autograd; texture_bwd = fr_synth_texture_backward beside grad.reshape(B, -1) @ pc_tex; copy = a 512 MiB "
               "device-to-device copy, copy_rate = 2 x 512 MiB / its median; must_move = 32 B per covered pixel and 4 per uncovered one "
               "forward, plus 24 B written per pixel backward" % (args.calls, args.rounds, "small" if args.small else "full", S, S),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
       "geometry_at_%d_faces" % args.faces[-1]: dict(zip(("pixels_per_tile", "tiles_per_face", "finish_threads", "sums_per_face"), geo)),
       "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
