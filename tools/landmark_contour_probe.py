#!/usr/bin/env python3
"""What sliding contour landmarks cost, in ONE process (modelled on tools/landmark_solve_probe.py): alternating rounds, device events,
medians of the rounds, the full-size model (N = 53,215, 199 + 29 coefficients), 32 and 64 faces, Kf = 52 fixed landmarks and 16 lines
of 24 candidates every 4th column (utils/synth.py::contour_lines(145, 367, 8, 24, stride=4)): K = 52 + 384 = 436 landmarks of which
68 carry weight, beside a plain K = 68: the fixed ids and the 16 lines' rim vertices (every face's own winners would need an image
per face; the rim vertices give the same K and the same arithmetic per landmark).

  'select'          = fr_landmark_contour_select, nearest rule, target and weight written     (raw C ABI: one launch)
  'forward_K'       = fr_landmark_forward over the masked K = 436 under the call's target and weight
  'forward_68'      = fr_landmark_forward over K = 68 (the fixed ids and the rim vertices)
  'step_pose_K'     = fr_landmark_solve_step, the six pose columns, over the masked K
  'step_pose_68'      ... over K = 68
  'step_coef_K'     = fr_landmark_solve_step, pose and the 228 coefficients, over the masked K
  'step_coef_68'      ... over K = 68
  'fit10_slide'     = rendering_layer/ops.py::landmark_fit(iters=10, line_target=...): re-selection at every iteration (host time
                      included)
  'fit10_fixed'     = landmark_fit(iters=10) over K = 68, every contour point held to its line's rim vertex: no selection (host
                      time included)
`fit_quality` records what the two fits reach from the same start (`fit10_fixed_rim` is the rim-vertex fit), and `sel` how far the
truth's contour sits from the rim.

--out FILE: where the JSON goes besides stdout (default profiles/landmark_contour.json)."""
import argparse
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
ap.add_argument("--calls", type=int, default=20, help="calls per timed figure of a kernel")
ap.add_argument("--fit-calls", type=int, default=3, help="calls per timed figure of a whole fit")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark_contour.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("landmark_contour_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
KF, PER_SIDE, M, STRIDE = 52, 8, 24, 4
fixed = synth.landmark_ids(A, KF)
lines, line_dir = synth.contour_lines(synth.GRID_U, synth.GRID_V, PER_SIDE, M, stride=STRIDE)
C = lines.shape[0]
F64 = dict(dtype=torch.float64, device=dev)


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
    ns, ne = net.ndim_shape, net.ndim_exp
    Kt = ns + ne
    cb = net.landmark_contour_basis(fixed, lines)
    K = cb.K
    P_gt = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    ld = torch.as_tensor(line_dir, device=dev)
    with torch.no_grad():
        sel_gt, line_target, _, _ = ops.landmark_contour_select(P_gt, cb, rule="extreme", line_dir=ld)
        fixed_target = ops.landmarks(P_gt, cb)[:, 0:2, :KF].transpose(1, 2).contiguous()
    # the perturbed start: the example's units at --pose-noise 4
    g = torch.Generator(device="cpu").manual_seed(77)
    scale = torch.tensor([0.03] * 3 + [1.5, 1.5, 0.0], **o).repeat(B, 1)
    scale = torch.cat([scale, 0.03 * P_gt[:, 6:7]], dim=1)
    P0 = torch.cat([P_gt[:, :7] + (torch.rand((B, 7), generator=g) * 2 - 1).to(dev) * 4.0 * scale, P_gt[:, 7:]], dim=1).contiguous()
    ridge, center = (torch.as_tensor(t, device=dev) for t in synth.coefficient_prior(ns, ne, 0.5))
    damp = torch.full((B,), 1e-3, **F64)
    sel = torch.empty((B, C), dtype=torch.int32, device=dev)
    pts, target, weight = torch.empty((B, C, 2), **o), torch.empty((B, K, 2), **o), torch.empty((B, K), **o)
    # K = 68: the fixed ids and each face's own winners would need an image per face; the plain route takes ONE id list, so the
    # comparison uses the fixed ids and the rim vertices -- the same K, the same arithmetic per landmark
    lb68 = net.landmark_basis(np.concatenate([fixed, lines[:, 0]]))
    target68 = torch.cat([fixed_target, line_target], dim=1).contiguous()
    weight68 = torch.ones((B, KF + C), **o)
    points, points68 = torch.empty((B, 3, K), **o), torch.empty((B, 3, KF + C), **o)
    sse = torch.empty((B,), **F64)
    delta, cost, ok = torch.empty((B, 7 + Kt), **F64), torch.empty((B, 2), **F64), torch.empty((B,), dtype=torch.int32, device=dev)
    nws = L.fr_landmark_solve_workspace_bytes(B, ns, ne)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)

    def select():
        return L.fr_landmark_contour_select(h.ptr(P0), h.ptr(cb.image), cb.nbytes, None, h.ptr(fixed_target), None, 0, h.ptr(line_target),
                                            None, 0, None, 0, B, KF, C, M, ns, ne, 200.0, h.ptr(sel), h.ptr(pts), h.ptr(target),
                                            h.ptr(weight), st)

    def forward(lb, k, t, w, p):
        return L.fr_landmark_forward(h.ptr(P0), h.ptr(lb.image), lb.nbytes, None, h.ptr(t), h.ptr(w), 1, B, k, ns, ne, 200.0, h.ptr(p),
                                     h.ptr(sse), st)

    def step(lb, k, t, w, coef):
        return L.fr_landmark_solve_step(h.ptr(P0), h.ptr(lb.image), lb.nbytes, h.ptr(t), h.ptr(w), 1, h.ptr(ridge) if coef else None,
                                        h.ptr(center) if coef else None, h.ptr(damp), 0x5F, coef, B, k, ns, ne, 200.0, h.ptr(delta),
                                        h.ptr(cost), h.ptr(ok), h.ptr(ws) if coef else None, nws if coef else 0, st)

    def fit_slide():
        ops.landmark_fit(P0, cb, fixed_target, line_target=line_target, iters=10)
        return 0

    def fit_fixed():
        ops.landmark_fit(P0, lb68, target68, weight68, iters=10)
        return 0

    assert select() == 0
    torch.cuda.synchronize()
    assert int((weight != 0).sum()) == B * (KF + C)

    def err(P):
        e = (P.double() - P_gt.double()).abs()
        return {"angle_max_rad": float(e[:, 0:3].max()), "txy_max_px": float(e[:, 3:5].max())}
    fs, i_s = ops.landmark_fit(P0, cb, fixed_target, line_target=line_target, iters=10)
    ff, i_f = ops.landmark_fit(P0, lb68, target68, weight68, iters=10)
    quality = {"start": err(P0), "fit10_slide": err(fs), "fit10_fixed_rim": err(ff),
               "F_sum": {"fit10_slide": [float(i_s["cost"][0].sum()), float(i_s["cost"][-1].sum())],
                         "fit10_fixed_rim": [float(i_f["cost"][0].sum()), float(i_f["cost"][-1].sum())]},
               "sel_equals_truth": float((i_s["sel"][-1] == sel_gt).double().mean())}
    sel_stats = {"truth_mean_position": float(sel_gt.double().mean()), "truth_max_position": int(sel_gt.max()),
                 "lines_off_the_rim": float((sel_gt > 0).double().mean())}

    routes = {"select": (select, args.calls),
              "forward_K": (lambda: forward(cb, K, target, weight, points), args.calls),
              "forward_68": (lambda: forward(lb68, KF + C, target68, weight68, points68), args.calls),
              "step_pose_K": (lambda: step(cb, K, target, weight, 0), args.calls),
              "step_pose_68": (lambda: step(lb68, KF + C, target68, weight68, 0), args.calls),
              "step_coef_K": (lambda: step(cb, K, target, weight, 1), args.calls),
              "step_coef_68": (lambda: step(lb68, KF + C, target68, weight68, 1), args.calls),
              "fit10_slide": (fit_slide, args.fit_calls), "fit10_fixed": (fit_fixed, args.fit_calls)}
    for fn, _ in routes.values():
        assert fn() == 0
    torch.cuda.synchronize()
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, (fn, calls) in routes.items():
            res[k].append(timed(fn, calls))
    rec = {k: summary(v) for k, v in res.items()}
    rec["fit_quality"] = quality
    rec["sel"] = sel_stats
    rec["K_masked"], rec["K_live"], rec["image_bytes"] = int(K), int(KF + C), int(cb.nbytes)
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

doc = {"what": "us per call, device events around the calls of a figure (%d per kernel figure, %d per fit10 figure), %d alternating "
               "rounds (medians of the rounds; spread = max - min of the rounds), one process, full-size model (N = 53,215, 199 + 29 "
               "coefficients), Kf = %d fixed landmarks + %d lines x %d candidates (stride %d): K = %d masked, %d live; *_K = over the "
               "masked K under the select call's target and weight, *_68 = over the fixed ids and the rim vertices alone; fit10_slide "
               "= ops.landmark_fit(iters=10, line_target=) with re-selection, fit10_fixed = ops.landmark_fit(iters=10) over K = 68, "
               "both with their host time" % (args.calls, args.fit_calls, args.rounds, KF, C, M, STRIDE, KF + C * M, KF + C),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
