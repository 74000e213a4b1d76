#!/usr/bin/env python3
"""What the fidelity and the smoothness term of the fine depth map cost on their two routes, in ONE process (modelled on
tools/geometry_gram_probe.py): alternating rounds, device events, medians, 32 and 64 faces of 200 x 200.

  'torch_fwd_bwd'     = the default route of get_loss for the two terms: F.mse_loss(pred, coarse), laplace_transform(pred[..., 0])
                        .abs().sum(), their weighted sum (100, 1e-5) and its backward into pred AND coarse
  'fused_fwd_bwd'     = ops.fine_depth_losses(pred, coarse), the same weighted sum and backward (the autograd node; outputs and
                        gradients allocated per call)
  'kernels_fwd'       = fr_fine_losses_forward through the raw C ABI (the pass and the finish launch)
  'kernels_bwd'       = fr_fine_losses_backward through the raw C ABI with grad_coarse;  'kernels_bwd_pred_only' without it
  'kernels_fwd_bwd'   = the three launches together

Beside them the bytes each direction must move -- forward 8 B / pixel (z and c read), backward 12 B / pixel (z and c read, grad_pred
written) or 16 with grad_coarse -- the time they take at the measured copy rate of 6.29 TB/s, and each direction's ratio to that
floor (recorded, no threshold).  The condition: 'kernels_fwd_bwd' and, on a quiet host, 'fused_fwd_bwd' below 'torch_fwd_bwd' at
both sizes.

--out FILE: where the JSON goes besides stdout (default profiles/fine_losses.json)."""
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
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[32, 64])
ap.add_argument("--size", type=int, default=200)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_losses.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("fine_losses_probe: needs an MI355X (a measurement path does not fall back)")

importlib.import_module("3dfacerecon_amd.nets.coarse_net").apply_miopen_workaround()   # the torch route runs a convolution backward
h = importlib.import_module("3dfacerecon_amd._lib")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
losses = importlib.import_module("3dfacerecon_amd.nets.losses")
L = h.lib()
dev = torch.device("cuda:0")
S = args.size
LAMBDA_F, LAMBDA_SM = losses.LAMBDA_F, losses.LAMBDA_SM


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


st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
out = {}
for B in args.faces:
    g = torch.Generator().manual_seed(B)
    coarse = (torch.rand((B, S, S, 1), generator=g) * 40.0).to(dev).requires_grad_(True)
    pred = (coarse.detach() + 0.05 * torch.rand((B, S, S, 1), generator=g).to(dev)).requires_grad_(True)
    one = torch.ones((), dtype=torch.float32, device=dev)
    gf = torch.full((), LAMBDA_F, dtype=torch.float32, device=dev)
    gs = torch.full((), LAMBDA_SM, dtype=torch.float32, device=dev)
    nst = L.fr_fine_losses_state_bytes(B, S, S)
    state = torch.empty((nst,), dtype=torch.uint8, device=dev)
    scal = torch.empty((2,), dtype=torch.float32, device=dev)
    gp, gc = torch.empty_like(pred), torch.empty_like(coarse)
    p_, c_ = pred.detach(), coarse.detach()

    def torch_fwd_bwd():
        pred.grad = coarse.grad = None
        f = F.mse_loss(pred, coarse)
        s = losses.laplace_transform(pred[..., 0]).abs().sum()
        (LAMBDA_F * f + LAMBDA_SM * s).backward(one)

    def fused_fwd_bwd():
        pred.grad = coarse.grad = None
        f, s = ops.fine_depth_losses(pred, coarse)
        (LAMBDA_F * f + LAMBDA_SM * s).backward(one)

    def kernels_fwd():
        L.fr_fine_losses_forward(h.ptr(p_), h.ptr(c_), B, S, S, h.ptr(scal[0:]), h.ptr(scal[1:]), h.ptr(state), nst, st)

    def kernels_bwd():
        L.fr_fine_losses_backward(h.ptr(gf), h.ptr(gs), h.ptr(p_), h.ptr(c_), B, S, S, h.ptr(gp), h.ptr(gc), st)

    def kernels_bwd_pred_only():
        L.fr_fine_losses_backward(h.ptr(gf), h.ptr(gs), h.ptr(p_), h.ptr(c_), B, S, S, h.ptr(gp), None, st)

    def kernels_fwd_bwd():
        kernels_fwd()
        kernels_bwd()

    routes = {"torch_fwd_bwd": torch_fwd_bwd, "fused_fwd_bwd": fused_fwd_bwd, "kernels_fwd": kernels_fwd, "kernels_bwd": kernels_bwd,
              "kernels_bwd_pred_only": kernels_bwd_pred_only, "kernels_fwd_bwd": kernels_fwd_bwd}
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the two routes beside each other on this input (recorded, not asserted; the tests hold both)
    torch_fwd_bwd()
    ft, s_t = float(F.mse_loss(p_, c_)), float(losses.laplace_transform(p_[..., 0]).abs().sum())
    gpt, gct = pred.grad.clone(), coarse.grad.clone()
    fused_fwd_bwd()
    ff, sf = (float(v) for v in ops.fine_depth_losses(p_, c_))
    gpf, gcf = pred.grad.clone(), coarse.grad.clone()
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    npix = B * S * S
    floors = {"forward": 8 * npix, "backward": 16 * npix, "backward_pred_only": 12 * npix}
    rec["bytes"] = {k: {"must_move": v, "time_at_copy_rate_us": round(v / COPY_RATE * 1e6, 2)} for k, v in floors.items()}
    rec["ratio_to_byte_floor"] = {
        "forward": round(rec["kernels_fwd"]["median"] / rec["bytes"]["forward"]["time_at_copy_rate_us"], 2),
        "backward": round(rec["kernels_bwd"]["median"] / rec["bytes"]["backward"]["time_at_copy_rate_us"], 2),
        "backward_pred_only": round(rec["kernels_bwd_pred_only"]["median"] / rec["bytes"]["backward_pred_only"]["time_at_copy_rate_us"], 2)}
    rec["torch_over_fused_fwd_bwd"] = round(rec["torch_fwd_bwd"]["median"] / rec["fused_fwd_bwd"]["median"], 2)
    rec["torch_over_kernels_fwd_bwd"] = round(rec["torch_fwd_bwd"]["median"] / rec["kernels_fwd_bwd"]["median"], 2)
    rec["condition"] = {"kernels_below_torch": bool(rec["kernels_fwd_bwd"]["median"] < rec["torch_fwd_bwd"]["median"]),
                        "operator_below_torch": bool(rec["fused_fwd_bwd"]["median"] < rec["torch_fwd_bwd"]["median"])}
    rec["losses"] = {"torch": [ft, s_t], "fused": [ff, sf],
                     "relative_difference": [abs(ft - ff) / abs(ff), abs(s_t - sf) / abs(sf)],
                     "largest_gradient_difference_over_largest_gradient": {
                         "pred": float((gpt - gpf).abs().max() / gpf.abs().max()),
                         "coarse": float((gct - gcf).abs().max() / gcf.abs().max())}}
    rec["state_bytes"] = int(nst)
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

geo = (ctypes.c_int * 7)()
L.fr_debug_fine_losses_geom(args.faces[-1], S, S, geo)
doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, %d x %d images; "
               "torch_fwd_bwd = mse_loss + laplace_transform().abs().sum(), weighted, and the backward into pred and coarse; "
               "fused_fwd_bwd = ops.fine_depth_losses the same way (autograd node); kernels_* = fr_fine_losses_forward / _backward "
               "through the raw C ABI" % (args.calls, args.rounds, S, S),
       "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
       "geometry_at_%d_faces" % args.faces[-1]: dict(zip(("tile_w", "tile_h", "threads", "tiles_across", "tiles_down",
                                                         "finish_threads", "backward_lds_bytes"), geo)),
       "condition_holds_at_every_size": {"kernels": all(r["condition"]["kernels_below_torch"] for r in out.values()),
                                         "operator": all(r["condition"]["operator_below_torch"] for r in out.values())},
       "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
