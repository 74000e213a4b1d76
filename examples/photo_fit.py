#!/usr/bin/env python3
"""Analysis by synthesis on one synthetic batch: fit the lighting and the albedo coefficients of every face to its picture by
descending the photometric loss (nets/losses.py::photometric_loss: synth_texture -> render_depth -> photo_loss, every link with a
HIP backward).

    python examples/photo_fit.py --small                 # tiny assets, 32 x 32, 3 faces
    python examples/photo_fit.py --batch 8 --steps 200   # the full mesh at 200 x 200
    python examples/photo_fit.py --small --fit-shape     # also fit the shape and expression coefficients (pose held at the truth)
    python examples/photo_fit.py --small --fit-pose      # also fit t3d, f and the angles, from the truth perturbed
    python examples/photo_fit.py --small --colour        # the picture in colour: RGB albedo, second-order lighting per channel
    python examples/photo_fit.py --small --colour --closed-form 8 --steps 0   # ... light and alpha by alternating least squares
    python examples/photo_fit.py --small --colour --smooth   # ... shaded from interpolated albedo and vertex normals, target included
    python examples/photo_fit.py --small --fit-pose --landmarks 68                    # ... with the landmark term beside the two
    python examples/photo_fit.py --small --fit-pose --landmarks 68 --landmarks-only   # pose from the landmarks alone: no render
    python examples/photo_fit.py --small --fit-pose --landmarks 68 --landmarks-only --landmark-init 6 --steps 0   # ... by the solver
    python examples/photo_fit.py --small --fit-pose --landmarks 20 --contour 4 --landmarks-only --landmark-init 10 --steps 0 --yaw 0.5
                                                         # ... with 4 contour points a side that slide (--contour-fixed: that do not)

A batch of pipeline.SynthBatches gives the picture and its ground truth (parameters, light, alpha).  The fit starts from the truth
perturbed (light by --light-noise, alpha by --alpha-noise; with --fit-shape the coefficients from zero) and runs Adam.  By default the
geometry is the ground truth's and stays fixed.  With --fit-pose the translation, the scale and the three angles start from the truth
perturbed (--pose-noise) and are fitted too: the decode runs with pose_grad=True, and the silhouette term
(nets/losses.py::silhouette_loss: the soft coverage of the rendered face against the batch's mask, --silhouette-lambda) stands beside
the photometric one -- it is the term that tells the fit where the face is in the picture.  With --landmarks K the batch also carries
the projections of K vertices (utils/synth.py::landmark_ids; pipeline.SynthBatches(landmarks=)) and the landmark term
(nets/losses.py::landmark_loss, --landmark-lambda) holds the fit's own projections of those vertices to them: it reads a compact image
of their basis rows, not the dense basis.  --landmarks-only fits the pose (and with --fit-shape the coefficients) to that term alone
-- the usual first stage of a fit to a real picture -- with no render and no dense decode in the loop; light and alpha then stay where
they start.  --landmark-init [ITERS] first runs the landmark solver (rendering_layer/ops.py::landmark_fit: damped Gauss-Newton
steps, scale-free, a handful of iterations) from the perturbed start, and Adam goes on from where it ends; with --fit-shape the
solver also fits the coefficients under the sampler's own prior (utils/synth.py::coefficient_prior).  --steps 0 gives the solver
alone.  --contour PER_SIDE adds PER_SIDE contour landmarks a side (utils/synth.py::contour_lines): each is a line of candidate vertices
from the rim inwards, the batch carries the face's occluding contour on every line, and the term and the solver hold each point to
the candidate that lies nearest under the current parameters -- the correspondence slides with the pose, as the jaw points of a
68-point annotation do.  --colour --closed-form [ITERS] first runs the colour photometric solve (FaceRecNet.photo_solve_rgb: the
lighting and alpha by alternating linear least squares on the render at the current geometry, from alpha = 0 and no lighting: the
perturbed start is not used) and Adam goes on from where it ends; --steps 0 gives the solve alone.  --contour-fixed keeps the rim vertex instead, for the comparison; --yaw sets the truth's yaw.  Prints ONE
JSON record: the first and last loss and the parameter errors (RMS against the ground truth) before and after.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def pkg(n):
    return importlib.import_module("3dfacerecon_amd." + n)


def rms(a, b):
    return float((a.detach().double() - b.double()).pow(2).mean().sqrt())


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="tiny synthetic assets at 32 x 32, 3 faces (smoke runs)")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--im-size", type=int, default=None)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--light-noise", type=float, default=0.2)
    ap.add_argument("--alpha-noise", type=float, default=0.5)
    ap.add_argument("--fit-shape", action="store_true", help="also fit the shape and expression coefficients, from zero")
    ap.add_argument("--fit-pose", action="store_true", help="also fit t3d, f and the angles, from the truth perturbed; adds the "
                                                           "silhouette term")
    ap.add_argument("--pose-noise", type=float, default=1.0, help="with --fit-pose: the perturbation, in units of 1.5 px of "
                                                                  "translation, 3 %% of scale and 0.03 rad")
    ap.add_argument("--silhouette-lambda", type=float, default=1.0)
    ap.add_argument("--colour", action="store_true", help="the picture in colour: per-channel albedo under a second-order lighting per "
                                                          "channel, light [B,3,9] (default: the gray first-order route)")
    ap.add_argument("--closed-form", type=int, nargs="?", const=8, default=0, metavar="ITERS",
                    help="with --colour: first fit light and alpha by ITERS alternations of the two linear least squares "
                         "(photo_solve_rgb); --steps 0 gives the solve alone")
    ap.add_argument("--smooth", action="store_true", help="shade from smooth planes (FaceRecNet.smooth_planes: the albedo and the vertex "
                                                          "normals interpolated at the pixel) in place of the render's flat ones, "
                                                          "the target picture included")
    ap.add_argument("--landmarks", type=int, default=0, help="K > 0: add the landmark term over K vertices (utils/synth.landmark_ids)")
    ap.add_argument("--landmark-lambda", type=float, default=1.0)
    ap.add_argument("--landmarks-only", action="store_true", help="fit to the landmark term alone (needs --landmarks and --fit-pose or "
                                                                  "--fit-shape): no render in the loop")
    ap.add_argument("--landmark-init", type=int, nargs="?", const=10, default=0, metavar="ITERS",
                    help="run ITERS (default 10) Levenberg-Marquardt iterations on the landmark term before the Adam loop (needs "
                         "--landmarks and --fit-pose or --fit-shape)")
    ap.add_argument("--landmark-sigma", type=float, default=0.5, help="with --landmark-init and --fit-shape: the landmark noise, in "
                                                                      "pixels, that scales the coefficients' prior")
    ap.add_argument("--contour", type=int, default=0, metavar="PER_SIDE",
                    help="PER_SIDE > 0: add PER_SIDE contour landmarks a side that slide along the silhouette (utils/synth.contour_lines; "
                         "needs --landmarks)")
    ap.add_argument("--contour-depth", type=int, default=None, metavar="M",
                    help="candidates per contour line, from the rim inwards (default 8 with --small, else 24 every 4th column)")
    ap.add_argument("--contour-fixed", action="store_true", help="hold each contour landmark to its line's rim vertex (a fixed "
                                                                 "correspondence), for the comparison")
    ap.add_argument("--yaw", type=float, default=None, help="with --landmarks-only: set the truth's yaw (radians) on every face; the "
                                                            "landmarks are then taken at that truth")
    return ap


def make_noise(seed, dev):
    """uniform noise in [-s, s] of a tensor's shape, from one seeded CPU generator: the draws follow the order of the calls"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return lambda t, s: (torch.rand(t.shape, generator=g) * 2 - 1).to(device=dev, dtype=t.dtype) * s


def pose_start(pose_gt, noise, pose_noise):
    """-> (pose0, pose_scale): the truth perturbed, and the unit of each unknown -- angles in 0.03 rad, x and y in 1.5 px, f in 3 %
    of its value; t3d's z moves no pixel and stays"""
    B, dev = pose_gt.shape[0], pose_gt.device
    pose_scale = torch.tensor([0.03] * 3 + [1.5, 1.5, 1.0], device=dev, dtype=pose_gt.dtype).repeat(B, 1)
    pose_scale = torch.cat([pose_scale, 0.03 * pose_gt[:, 6:7]], dim=1)
    kick = noise(pose_gt, pose_noise)
    kick[:, 5] = 0
    return pose_gt + kick * pose_scale, pose_scale


def descend(opt, loss_of, steps):
    """`steps` optimiser steps on loss_of() -> (the first loss, the loss after the last step)"""
    first = None
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        L = loss_of()
        L.backward()
        opt.step()
        first = float(L.detach()) if first is None else first
    with torch.no_grad():
        return first, float(loss_of())


def main():
    args = build_parser().parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    synth, netm, pipe, losses = pkg("utils.synth"), pkg("nets.network"), pkg("pipeline"), pkg("nets.losses")
    B = args.batch or (3 if args.small else 8)
    S = args.im_size or (32 if args.small else 200)
    A = synth.make_small_assets() if args.small else synth.make_assets()
    face = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=dev)
    if args.landmarks_only and not (args.landmarks > 0 and (args.fit_pose or args.fit_shape)):
        raise SystemExit("--landmarks-only needs --landmarks K and something to fit: --fit-pose or --fit-shape")
    if args.landmarks > 0 and not (args.fit_pose or args.fit_shape):
        raise SystemExit("--landmarks needs --fit-pose or --fit-shape: with the geometry fixed the term is a constant")
    if args.landmark_init and not (args.landmarks > 0 and (args.fit_pose or args.fit_shape)):
        raise SystemExit("--landmark-init needs --landmarks K and something to fit: --fit-pose or --fit-shape")
    if args.closed_form and (not args.colour or args.landmarks_only):
        raise SystemExit("--closed-form needs --colour, and a render: not --landmarks-only")
    lm_idx = synth.landmark_ids(A, args.landmarks) if args.landmarks > 0 else None
    kw = {"colour": True} if args.colour else {}
    if lm_idx is not None:
        kw["landmarks"] = lm_idx
    if args.contour > 0 and lm_idx is None:
        raise SystemExit("--contour needs --landmarks K: the contour points stand beside the fixed landmarks")
    if args.yaw is not None and not args.landmarks_only:
        raise SystemExit("--yaw needs --landmarks-only: the batch's picture shows the sampled pose")
    lines = line_dir = None
    if args.contour > 0:
        depth = args.contour_depth or (8 if args.small else 24)
        lines, line_dir = synth.contour_lines(20 if args.small else synth.GRID_U, 24 if args.small else synth.GRID_V, args.contour, depth,
                                              stride=1 if args.small else 4)
        kw["contour_lines"] = (lines, line_dir)
    stream = pipe.SynthBatches(face, B, args.seed, slots=1, focal=1e-3 * S / 200.0, **kw)
    b = {k: v.clone() for k, v in stream.next().items()}
    torch.cuda.synchronize(dev)
    if args.yaw is not None:
        ops = pkg("rendering_layer.ops")
        with torch.no_grad():
            b["params"][:, 1] = args.yaw
            b["landmarks"] = face.landmarks(b["params"], lm_idx)[:, 0:2].transpose(1, 2).contiguous()
            if lines is not None:
                b["contour_sel"], b["contour_landmarks"], _, _ = ops.landmark_contour_select(
                    b["params"], face.landmark_contour_basis(None, lines), rule="extreme",
                    line_dir=torch.as_tensor(line_dir, device=dev), im_size=S)
    # --contour-fixed: every line keeps its rim vertex alone, so the correspondence cannot slide
    fit_lines = None if lines is None else (lines[:, :1] if args.contour_fixed else lines)
    if args.smooth:
        if args.landmarks_only or args.closed_form:
            raise SystemExit("--smooth shades the render's planes: not with --landmarks-only or --closed-form")
        # the batch's picture shows flat planes: shade the same face, light and albedo again from the smooth ones
        ops = pkg("rendering_layer.ops")
        with torch.no_grad():
            tex_gt = ops.synth_texture(face.mu_tex, face.pc_tex, b["alpha"])
            planes = face.smooth_planes(face.vertices_transform(b["params"]), tex_gt, b["tri_ind"])
            if args.colour:
                b["im_rgb"], b["im_gray"], _ = ops.synth_shade_rgb(*planes, b["tri_ind"], b["light"], gain=stream.gain, offset=stream.offset)
            else:
                b["im_gray"], _ = ops.synth_shade(*planes, b["tri_ind"], b["light"], gain=stream.gain, offset=stream.offset)
    im, params, light_gt, alpha_gt = b["im_gray"], b["params"], b["light"], b["alpha"]
    noise = make_noise(args.seed, dev)
    light = (light_gt + noise(light_gt, args.light_noise)).requires_grad_(True)
    alpha = (alpha_gt + noise(alpha_gt, args.alpha_noise)).requires_grad_(True)
    groups = [{"params": [light, alpha], "lr": args.lr}]
    n0, ns = face.ndim_pose, face.ndim_shape
    coef_gt = params[:, n0:]
    coef = None
    if args.fit_shape:
        # unit-scale unknowns: the shape coefficients live on a scale of 1e4 (utils/synth.get_random_params), the expression's on 1
        scale = torch.cat([torch.full((ns,), 1e4), torch.ones(face.ndim_exp)]).to(dev)
        coef = torch.zeros_like(coef_gt, requires_grad=True)
        groups.append({"params": [coef], "lr": args.lr})
    pose = None
    if args.fit_pose:
        pose_gt = params[:, :n0]
        pose0, pose_scale = pose_start(pose_gt, noise, args.pose_noise)
        pose = torch.zeros_like(pose_gt, requires_grad=True)
        groups.append({"params": [pose], "lr": args.lr})
    opt = torch.optim.Adam(groups)

    def pose_now():
        return pose0 + pose * pose_scale

    def params_now():
        return torch.cat([params[:, :n0] if pose is None else pose_now(), params[:, n0:] if coef is None else coef * scale], dim=1)

    def vertices(p):
        if coef is None and pose is None:
            with torch.no_grad():
                return face.vertices_transform(params)
        return face.vertices_transform(p, pose_grad=True) if pose is not None else face.vertices_transform(p)

    def landmark_term(p):
        if fit_lines is not None:
            return losses.landmark_loss(face, p, lm_idx, b["landmarks"], pose_grad=pose is not None, lines=fit_lines,
                                        line_target=b["contour_landmarks"])
        return losses.landmark_loss(face, p, lm_idx, b["landmarks"], pose_grad=pose is not None)

    def loss_of():
        p = params_now()
        if args.landmarks_only:
            return args.landmark_lambda * landmark_term(p)
        ver = vertices(p)
        term = losses.photometric_loss_smooth if args.smooth else losses.photometric_loss
        L = term(face, ver, b["im_rgb"] if args.colour else im, light, alpha, gain=stream.gain, offset=stream.offset)
        if pose is not None:
            L = L + args.silhouette_lambda * losses.silhouette_loss(face, ver, b["mask"]).double()
        if lm_idx is not None:
            L = L + args.landmark_lambda * landmark_term(p)
        return L

    def pose_errors():
        p = pose_now().detach()
        return {"t3d_rms": rms(p[:, 3:6], pose_gt[:, 3:6]), "f_rel_rms": rms(p[:, 6] / pose_gt[:, 6], torch.ones_like(p[:, 6])),
                "angle_rms": rms(p[:, 0:3], pose_gt[:, 0:3])}

    before = {"light_rms": rms(light, light_gt), "alpha_rms": rms(alpha, alpha_gt)}
    if pose is not None:
        before.update(pose_errors())
    if coef is not None:
        before["coef_rms_scaled"] = rms(coef, coef_gt / scale)
    init = contour = None
    if lines is not None:
        contour = {"per_side": int(args.contour), "depth": int(lines.shape[1]), "fixed": bool(args.contour_fixed),
                   "sel_truth": b["contour_sel"].tolist(), "sel_fitted": None}
    if args.landmark_init:
        ridge = center = None
        if coef is not None:
            ridge, center = (torch.as_tensor(t, device=dev) for t in synth.coefficient_prior(ns, face.ndim_exp, args.landmark_sigma))
        with torch.no_grad():
            if fit_lines is not None:
                fitted, info = face.landmark_fit(params_now(), face.landmark_contour_basis(lm_idx, fit_lines), b["landmarks"], ridge=ridge,
                                                 center=center, iters=args.landmark_init, fit_pose=pose is not None,
                                                 fit_coef=coef is not None, line_target=b["contour_landmarks"])
                contour["sel_fitted"] = info["sel"][-1].tolist()
            else:
                fitted, info = face.landmark_fit(params_now(), lm_idx, b["landmarks"], ridge=ridge, center=center,
                                                 iters=args.landmark_init, fit_pose=pose is not None, fit_coef=coef is not None)
            if pose is not None:
                pose0 = fitted[:, :n0].clone()      # (pose stays 0: Adam goes on from the solver's pose, in the same units)
            if coef is not None:
                coef.copy_(fitted[:, n0:] / scale)
        init = {"iters": int(args.landmark_init), "cost_first": float(info["cost"][0].sum()), "cost_last": float(info["cost"][-1].sum()),
                "accepted": int(info["accepted"].sum())}
        if pose is not None:
            init.update(pose_errors())
        if coef is not None:
            init["coef_rms_scaled"] = rms(coef, coef_gt / scale)
    closed = None
    if args.closed_form:
        ops = pkg("rendering_layer.ops")
        with torch.no_grad():
            ver = vertices(params_now()).detach().float()
            _, _, normal, tri_ind = ops.render_depth(ver, face.tri, face.mu_tex[None], b["im_rgb"])
            l_fit, a_fit, _, info = face.photo_solve_rgb(tri_ind, normal, b["im_rgb"], iters=args.closed_form, gain=stream.gain,
                                                         offset=stream.offset)
            light.copy_(l_fit)
            alpha.copy_(a_fit)
        closed = {"iters": int(args.closed_form), "E_first": float(info["E"][0, 0].sum()), "E_last": float(info["E"][-1, 1].sum()),
                  "ok": bool(info["ok"].all()), "light_rms": rms(light, light_gt), "alpha_rms": rms(alpha, alpha_gt)}
        if pose is not None:
            closed.update(pose_errors())
    first, last = descend(opt, loss_of, args.steps)
    after = {"light_rms": rms(light, light_gt), "alpha_rms": rms(alpha, alpha_gt)}
    if coef is not None:
        after["coef_rms_scaled"] = rms(coef, coef_gt / scale)
    if pose is not None:
        after.update(pose_errors())
    print(json.dumps({"program": "photo_fit", "faces": B, "im_size": S, "steps": args.steps, "lr": args.lr, "fit_shape": bool(args.fit_shape),
                      "fit_pose": bool(args.fit_pose), "colour": bool(args.colour), "smooth": bool(args.smooth),
                      "landmarks": int(args.landmarks),
                      "landmarks_only": bool(args.landmarks_only), "landmark_init": init, "closed_form": closed, "contour": contour, "yaw": args.yaw,
                      "first": first, "last": last, "ratio": last / first if first else None, "errors_before": before,
                      "errors_after": after, "finite": bool(torch.isfinite(light).all() and torch.isfinite(alpha).all())}))


if __name__ == "__main__":
    main()
