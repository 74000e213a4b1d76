#!/usr/bin/env python3
"""What a step of the landmark solver costs beside the stock-torch composition of the same step, and a whole fit beside the Adam loop
of the --landmarks-only route, in ONE process (modelled on tools/landmark_probe.py): alternating rounds, device events, medians of the
rounds, the full-size model (N = 53,215, 199 + 29 coefficients), K = 68, 32 and 64 faces.

  'step_pose'   = fr_landmark_solve_step, the six pose columns              (raw C ABI: one launch, no workspace)
  'step_coef'   = fr_landmark_solve_step, pose and the 228 coefficients     (raw C ABI: one launch, P = 234)
  'torch_pose'  = the same step in stock torch, float64: the decode and the Jacobian by einsum, J^T W J by einsum,
  'torch_coef'    linalg.cholesky and cholesky_solve of [B,P,P] through the vendor solver (its agreement with the kernel's delta, in
                  the Jacobi-scaled norm relative to the step, is recorded as `torch_agreement`)
  'fit10_pose'  = rendering_layer/ops.py::landmark_fit(iters=10), pose only  (10 steps, 11 evaluations of F, torch.where between;
  'fit10_coef'    host time included)
  'adam100'     = 100 Adam steps on nets/losses.py::landmark_loss with pose_grad, the loop of examples/photo_fit.py --fit-pose
                  --landmarks-only (host time included)
The fits start from the truth perturbed as the example perturbs it (--pose-noise 4); `fit_quality` records what each reaches.

--out FILE: where the JSON goes besides stdout (default profiles/landmark_solve.json)."""
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
ap.add_argument("--calls", type=int, default=20, help="calls per timed figure of a step")
ap.add_argument("--fit-calls", type=int, default=3, help="calls per timed figure of a whole fit")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--landmarks", type=int, default=68)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark_solve.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("landmark_solve_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
losses = importlib.import_module("3dfacerecon_amd.nets.losses")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
K = args.landmarks
idx = synth.landmark_ids(A, K)
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


def rotations(ang):
    """float64 angles [B,3] -> (R, [dR_phi, dR_gamma, dR_theta]), each [B,3,3]: the factors of tests/ref_landmark.py"""
    s, c = torch.sin(ang), torch.cos(ang)
    o, z = torch.ones_like(s[:, 0]), torch.zeros_like(s[:, 0])

    def m(*e):
        return torch.stack(e, dim=1).reshape(-1, 3, 3)
    Rp, Ry, Rr = m(o, z, z, z, c[:, 0], s[:, 0], z, -s[:, 0], c[:, 0]), m(c[:, 1], z, -s[:, 1], z, o, z, s[:, 1], z, c[:, 1]), \
        m(c[:, 2], s[:, 2], z, -s[:, 2], c[:, 2], z, z, z, o)
    dRp, dRy, dRr = m(z, z, z, z, -s[:, 0], c[:, 0], z, -c[:, 0], -s[:, 0]), m(-s[:, 1], z, -c[:, 1], z, z, z, c[:, 1], z, -s[:, 1]), \
        m(-s[:, 2], c[:, 2], z, -c[:, 2], -s[:, 2], z, z, z, z)
    return Rp @ Ry @ Rr, [dRp @ Ry @ Rr, Rp @ dRy @ Rr, Rp @ Ry @ dRr]


def torch_step(P, mean, U, target, weight, ridge, center, damp, coef, im):
    """the step of include/fr_hotpath.h ("landmark solver") in stock torch, float64 -> (delta over the unknowns, A, g)"""
    p = P.double()
    a, f = p[:, 7:], p[:, 6]
    v = mean[None] + torch.einsum("bj,kcj->bkc", a, U)
    R, dR = rotations(p[:, 0:3])
    Rv = torch.einsum("bic,bkc->bki", R, v)
    x = f[:, None] * Rv[:, :, 0] + p[:, None, 3]
    y = (im - (f[:, None] * Rv[:, :, 1] + p[:, None, 4])) - 1.0
    r = torch.stack([x - target[:, :, 0], y - target[:, :, 1]], dim=2).reshape(P.shape[0], -1)
    sign = torch.tensor([1.0, -1.0], **F64)
    cols = [f[:, None, None] * torch.einsum("bic,bkc->bki", d, v)[:, :, 0:2] * sign for d in dR]
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    cols += [torch.stack([one, zero], dim=2), torch.stack([zero, -one], dim=2), Rv[:, :, 0:2] * sign]
    J = torch.stack(cols, dim=3)                                               # [B,K,2,6]
    if coef:
        Jc = f[:, None, None, None] * torch.einsum("bic,kcj->bkij", R[:, 0:2], U) * sign[None, None, :, None]
        J = torch.cat([J, Jc], dim=3)
    J = J.reshape(P.shape[0], -1, J.shape[3])
    w = weight.double().repeat_interleave(2, dim=1)
    H = torch.einsum("brp,br,brq->bpq", J, w, J)
    g = torch.einsum("brp,br->bp", J, w * r)
    D = torch.diagonal(H, dim1=1, dim2=2).clone()
    if coef:
        H = H + torch.diag_embed(torch.cat([torch.zeros(6, **F64), ridge.double()]))[None]
        g = g + torch.cat([torch.zeros(6, **F64), ridge.double()])[None] * torch.cat([torch.zeros_like(p[:, :6]), a - center.double()], dim=1)
    Am = H + torch.diag_embed(damp[:, None] * D)
    Lc = torch.linalg.cholesky(Am)
    return torch.cholesky_solve(-g[:, :, None], Lc)[:, :, 0], Am, g


out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    ns, ne = net.ndim_shape, net.ndim_exp
    Kt = ns + ne
    lb = net.landmark_basis(idx)
    idx_t = torch.as_tensor(idx, device=dev)
    N = net.nvert
    rows = torch.stack([c * N + idx_t for c in range(3)], dim=1)                # [K,3]
    mean = net.mu.reshape(-1)[rows].double()
    U = torch.cat([net.pc_shape[rows], net.pc_exp[rows]], dim=2).double()      # [K,3,Kt]
    P_gt = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    g = torch.Generator(device="cpu").manual_seed(77)
    with torch.no_grad():
        target = (net.landmarks(P_gt, idx)[:, 0:2].transpose(1, 2) + 0.5 * torch.randn((B, K, 2), generator=g).to(dev)).contiguous()
    weight = torch.ones((B, K), **o)
    ridge, center = (torch.as_tensor(t, device=dev) for t in synth.coefficient_prior(ns, ne, 0.5))
    # the perturbed start: the example's units at --pose-noise 4, the coefficients at the prior's centre
    scale = torch.tensor([0.03] * 3 + [1.5, 1.5, 0.0], **o).repeat(B, 1)
    scale = torch.cat([scale, 0.03 * P_gt[:, 6:7]], dim=1)
    kick = (torch.rand((B, 7), generator=g) * 2 - 1).to(dev) * 4.0
    pose0 = P_gt[:, :7] + kick * scale
    P_pose = torch.cat([pose0, P_gt[:, 7:]], dim=1).contiguous()
    P_coef = torch.cat([pose0, center[None].expand(B, Kt)], dim=1).contiguous()
    damp = torch.full((B,), 1e-3, **F64)
    delta, cost, ok = torch.empty((B, 7 + Kt), **F64), torch.empty((B, 2), **F64), torch.empty((B,), dtype=torch.int32, device=dev)
    nws = L.fr_landmark_solve_workspace_bytes(B, ns, ne)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)

    def step(P, coef):
        return L.fr_landmark_solve_step(h.ptr(P), h.ptr(lb.image), lb.nbytes, h.ptr(target), h.ptr(weight), 1, h.ptr(ridge) if coef else None,
                                        h.ptr(center) if coef else None, h.ptr(damp), 0x5F, coef, B, K, ns, ne, 200.0, h.ptr(delta),
                                        h.ptr(cost), h.ptr(ok), h.ptr(ws) if coef else None, nws if coef else 0, st)

    def t_step(P, coef):
        with torch.no_grad():
            torch_step(P, mean, U, target.double(), weight, ridge, center, damp, coef, 200.0)
        return 0

    def fit10(P, coef):
        ops.landmark_fit(P, lb, target, weight, ridge=ridge if coef else None, center=center if coef else None, iters=10, fit_coef=bool(coef))
        return 0

    def adam100():
        pose = torch.zeros_like(pose0, requires_grad=True)
        unit = torch.where(scale > 0, scale, torch.ones_like(scale))
        opt = torch.optim.Adam([{"params": [pose], "lr": 0.02}])
        for _ in range(100):
            opt.zero_grad(set_to_none=True)
            p = torch.cat([pose0 + pose * unit, P_gt[:, 7:]], dim=1)
            losses.landmark_loss(net, p, idx, target, weight, pose_grad=True).backward()
            opt.step()
        return (pose0 + pose.detach() * unit)

    # agreement of the two routes to the same step, and what the fits reach
    agree = {}
    for name, P, coef in (("pose", P_pose, 0), ("coef", P_coef, 1)):
        assert step(P, coef) == 0
        with torch.no_grad():
            d_t, Am, _ = torch_step(P, mean, U, target.double(), weight, ridge, center, damp, coef, 200.0)
        torch.cuda.synchronize()
        cols = [0, 1, 2, 3, 4, 6] + (list(range(7, 7 + Kt)) if coef else [])
        s = torch.sqrt(torch.diagonal(Am, dim1=1, dim2=2))
        rel = (s * (delta[:, cols] - d_t)).norm(dim=1) / (s * d_t).norm(dim=1)
        agree[name] = {"ok_faces": int(ok.sum()), "max_relative_difference_scaled_norm": float(rel.max())}
    quality = {}

    def t3d_rms(P):
        return float((P[:, 3:5].double() - P_gt[:, 3:5].double()).pow(2).mean().sqrt())
    fp, ip = ops.landmark_fit(P_pose, lb, target, weight, iters=10)
    fc, ic = ops.landmark_fit(P_coef, lb, target, weight, ridge=ridge, center=center, iters=10, fit_coef=True)
    pa = adam100()
    quality = {"txy_rms_px": {"start": t3d_rms(P_pose), "fit10_pose": t3d_rms(fp), "fit10_coef": t3d_rms(fc), "adam100": t3d_rms(pa)},
               "F_sum": {"fit10_pose": [float(ip["cost"][0].sum()), float(ip["cost"][-1].sum())],
                         "fit10_coef": [float(ic["cost"][0].sum()), float(ic["cost"][-1].sum())]},
               "accepted": {"fit10_pose": int(ip["accepted"].sum()), "fit10_coef": int(ic["accepted"].sum())}}

    routes = {"step_pose": (lambda: step(P_pose, 0), args.calls), "step_coef": (lambda: step(P_coef, 1), args.calls),
              "torch_pose": (lambda: t_step(P_pose, 0), args.calls), "torch_coef": (lambda: t_step(P_coef, 1), args.calls),
              "fit10_pose": (lambda: fit10(P_pose, 0), args.fit_calls), "fit10_coef": (lambda: fit10(P_coef, 1), args.fit_calls),
              "adam100": (lambda: 0 if adam100() is not None else 1, 1)}
    for fn, _ in routes.values():
        assert fn() == 0
    torch.cuda.synchronize()
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, (fn, calls) in routes.items():
            res[k].append(timed(fn, calls))
    rec = {k: summary(v) for k, v in res.items()}
    rec["torch_agreement"] = agree
    rec["fit_quality"] = quality
    rec["workspace_bytes"] = int(nws)
    for k in ("pose", "coef"):
        rec["step_over_torch_" + k] = round(rec["step_" + k]["median"] / rec["torch_" + k]["median"], 3)
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

doc = {"what": "us per call, device events around the calls of a figure (%d per step figure, %d per fit10 figure, 1 per adam100 figure), %d "
               "alternating rounds (medians of the rounds; spread = max - min of the rounds), one process, full-size model (N = 53,215, "
               "199 + 29 coefficients), K = %d landmarks with 0.5 px of noise; step_* = fr_landmark_solve_step through the raw C ABI "
               "(pose: the six pose columns; coef: pose and 228 coefficients, damp 1e-3); torch_* = the same step in stock torch float64 "
               "(einsum Jacobian and normal matrix, linalg.cholesky, cholesky_solve); fit10_* = ops.landmark_fit(iters=10) with its host "
               "time; adam100 = 100 Adam steps on landmark_loss with pose_grad, the --landmarks-only loop, with its host time"
               % (args.calls, args.fit_calls, args.rounds, K),
       "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
