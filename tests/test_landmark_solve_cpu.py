"""CPU: the landmark solver (include/fr_hotpath.h, "landmark solver") without a GPU -- the binding rows and every return code of the
header's checks (all before any HIP call), and the numpy model (tests/ref_landmark_solve.py): its Jacobian against central differences
of the landmark model's float64 forward, its Cholesky against numpy's own solve of the same system, and the convergence of the
Levenberg-Marquardt loop on the case of the --landmarks-only fit, beside that fit's own Adam loop."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
import ref_landmark as RL
import ref_landmark_solve as RS
import ref_synth_batch as RB
import test_landmark_cpu as TL      # (its helpers: the example as a module, the float64 forward under torch autograd)

ROWS = {"fr_landmark_solve_workspace_bytes": "z:iii",
        "fr_landmark_solve_step": "i:ppzppipppiiiiiifppppzp"}
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4


def _face_doubles(Kt):
    Pm = 6 + Kt
    return (Pm * (Pm + 1) + Pm + 1) // 2 * 2


def test_names_and_rows():
    host = pkg("_lib")
    for name, row in ROWS.items():
        assert name in host.EXPORTS and host.SIGNATURES[name] == row, name
    assert "fr_landmark_solve.hip" in host.SOURCES
    src = open(os.path.join(ROOT, "include", "fr_hotpath.h")).read()
    assert "---- landmark solver ----" in src
    # the prototypes, as the header spells them: the names, the argument counts and the stream parameter's name
    for name, row in ROWS.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, src)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(row.split(":")[1]), (name, args)
    assert re.search(r"fr_landmark_solve_step\([^;]*void\* stream\);", src)
    L = host.lib()
    assert L.fr_landmark_solve_workspace_bytes(1, 199, 29) == 8 * _face_doubles(228)
    assert L.fr_landmark_solve_workspace_bytes(64, 199, 29) == 64 * 8 * _face_doubles(228)
    assert L.fr_landmark_solve_workspace_bytes(3, 0, 0) == 3 * 8 * _face_doubles(0) and _face_doubles(0) == 48
    assert L.fr_landmark_solve_workspace_bytes(2, 256, 0) == 2 * 8 * _face_doubles(256)
    for bad in ((0, 9, 5), (-1, 9, 5), (3, 200, 57), (3, -1, 5), (3, 9, -1), (3, 257, 0)):
        assert L.fr_landmark_solve_workspace_bytes(*bad) == 0, bad


# ---- return codes: made-up non-NULL pointers; every case returns before any HIP call ---------------------------------------------------
def test_return_codes():
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    L = pkg("_lib").lib()
    p, q, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), None   # q: not 16-byte aligned
    K, ns, ne, B = 5, 9, 5, 3
    nb = L.fr_landmark_basis_bytes(K, ns, ne)
    nws = L.fr_landmark_solve_workspace_bytes(B, ns, ne)
    assert nws == B * 8 * _face_doubles(ns + ne)

    def step(params=p, lb=p, nbytes=nb, target=p, weight=nul, wb=0, ridge=nul, center=nul, damp=nul, mask=0x5F, coef=1, B=B, K=K, ns=ns,
             ne=ne, delta=p, cost=p, ok=p, ws=p, wsb=nws):
        return L.fr_landmark_solve_step(params, lb, nbytes, target, weight, wb, ridge, center, damp, mask, coef, B, K, ns, ne, 200.0,
                                        delta, cost, ok, ws, wsb, nul)
    assert step(B=-1) == INVALID and step(K=-1) == INVALID and step(ns=-1) == INVALID and step(ne=-1) == INVALID
    assert step(wb=2) == INVALID and step(wb=-1) == INVALID and step(coef=2) == INVALID and step(coef=-1) == INVALID
    assert step(mask=0x20) == INVALID and step(mask=0x7F) == INVALID               # tz in the mask
    assert step(mask=0x80) == INVALID and step(mask=-1) == INVALID                 # a bit above 6
    assert step(mask=0, coef=0) == INVALID and step(mask=0, coef=1, ns=0, ne=0) == INVALID     # nothing to fit
    assert step(B=0) == OK and step(K=0) == OK and step(B=0, params=nul, delta=nul, cost=nul, ok=nul) == OK
    assert step(params=nul) == INVALID and step(target=nul) == INVALID
    assert step(delta=nul) == INVALID and step(cost=nul) == INVALID and step(ok=nul) == INVALID
    assert step(K=1025) == UNSUPPORTED and step(ns=200, ne=57) == UNSUPPORTED
    assert step(lb=nul) == WORKSPACE and step(lb=q) == WORKSPACE and step(nbytes=nb - 1) == WORKSPACE
    assert step(ws=nul) == WORKSPACE and step(ws=q) == WORKSPACE and step(wsb=nws - 1) == WORKSPACE    # a short workspace
    # the order of the checks
    assert step(B=-1, params=nul) == INVALID and step(mask=0x20, B=0) == INVALID and step(mask=0, coef=0, K=0) == INVALID
    assert step(params=nul, K=1025) == INVALID and step(K=1025, lb=nul) == UNSUPPORTED and step(lb=nul, ws=nul) == WORKSPACE
    assert step(K=1025, ws=nul) == UNSUPPORTED


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _case(assets, B, K, seed, synth, noise=2.0):
    rs = np.random.RandomState(seed)
    ns, ne = assets["ndim_shape"], assets["ndim_exp"]
    idx = synth.landmark_ids(assets, K)
    mean, U = RL.split_image(RL.basis_image(assets["mu"], assets["pc_shape"], assets["pc_exp"], idx), K, ns + ne)
    P = synth.sample_params_batch(B, im_size=200, n_shape=ns, n_exp=ne, seed=seed).astype(np.float32)
    fw = RL.Forward(P, mean, U)
    target = (fw.points[:, 0:2].transpose(0, 2, 1) + rs.uniform(-noise, noise, (B, K, 2))).astype(np.float32)
    weight = rs.uniform(0.5, 2.0, (B, K)).astype(np.float32)
    weight[B - 1, K // 2] = 0.0
    return dict(mean=mean, U=U, P=P, target=target, weight=weight, ns=ns, ne=ne, rs=rs, B=B, K=K)


def test_model_jacobian_against_central_differences(small_assets, synth):
    """Every residual row's directional derivative J d (the model with exact=True: the rotation not rounded to fp32) against the
    central difference of RL.forward_f64 along d, per parameter group, within the bound tests/test_landmark_cpu.py uses for the
    gradient, taken row by row: h^2 / 6 max|x'''| + E / h with h = 2^-17; E <= (Kt + 16) 2^-53 A, A the sum of the absolute values of
    the coordinate's terms (RL.Forward.absterms); x''' = 0 along t3d, f and the coefficients (x and y are linear in each group) and
    at most X = 4 |f| sum_c |v_c| along the angles (|d|_1 = 1).  The tallest row of every direction must stand 100 bounds tall."""
    c = _case(small_assets, 3, 7, 5, synth)
    mean, U, P = c["mean"], c["U"], c["P"]
    B, K, Kt = c["B"], c["K"], c["ns"] + c["ne"]
    rs = c["rs"]
    st = RS.Step(P, mean, U, c["target"], fit_coef=True, exact=True)
    assert st.cols == [0, 1, 2, 3, 4, 6] + list(range(7, 7 + Kt)) and st.J.shape == (B, 2 * K, 6 + Kt)
    h = 2.0 ** -17
    P64 = P.astype(np.float64)
    A = st.fw.absterms                                                   # [B,3,K]
    X = 4 * np.abs(st.fw.f)[:, None] * np.abs(st.fw.v).sum(axis=2)       # [B,K]
    groups = [("angles", slice(0, 3), 1.0), ("t3d", slice(3, 5), 1.0), ("f", slice(6, 7), float(np.abs(P64[:, 6]).max())),
              ("shape", slice(7, 7 + c["ns"]), 1e3), ("expression", slice(7 + c["ns"], 7 + Kt), 0.3)]
    for name, cols, scale in groups:
        d = rs.uniform(-1, 1, (B, P64[:, cols].shape[1]))
        if name == "angles":
            d = d / np.abs(d).sum(axis=1, keepdims=True)
        dP = np.zeros_like(P64)
        dP[:, cols] = d * scale
        up = RL.forward_f64(P64 + h * dP, mean, U)
        dn = RL.forward_f64(P64 - h * dP, mean, U)
        num = ((up - dn) / (2 * h))[:, :, 0:2].reshape(B, 2 * K)         # rows 2 k (x), 2 k + 1 (y)
        want = np.einsum("brp,bp->br", st.J, dP[:, st.cols])
        bound = np.empty((B, 2 * K))
        for i in range(2):
            bound[:, i::2] = 1.01 * ((h * h / 6) * (X if name == "angles" else 0.0) + (Kt + 16) * 2.0 ** -53 * A[:, i, :] / h)
        err = np.abs(num - want)
        print("%s: max |J d| %.6g, max |difference| %.3g, max difference / bound %.3g" % (name, np.abs(want).max(), err.max(),
                                                                                          (err / bound).max()))
        assert np.abs(want).max() >= 100 * bound.max(), (name, np.abs(want).max(), bound.max())
        assert (err <= bound).all(), (name, (err / bound).max())
    # a landmark of weight 0: rows and residuals of exact +0, whatever its target
    target = c["target"].copy()
    target[2, 3] = np.nan
    weight = np.ones((B, K), np.float32)
    weight[2, 3] = 0.0
    ridge, center = synth.coefficient_prior(c["ns"], c["ne"])        # (14 rows cannot hold 20 unknowns alone)
    z = RS.Step(P, mean, U, target, weight=weight, fit_coef=True, ridge=ridge, center=center)
    assert not z.J[2, 6:8].any() and not z.r[2, 6:8].any() and np.isfinite(z.delta).all() and z.ok.all()
    # ... and the columns that are not fitted are +0
    part = RS.Step(P, mean, U, c["target"], pose_mask=RS.pose_mask(["tx", "ty", "f"]))
    assert part.cols == [3, 4, 6] and not part.delta[:, [0, 1, 2, 5]].any() and not part.delta[:, 7:].any() and part.delta[:, [3, 4, 6]].all()


def _solve_cases(small_assets, full_assets, synth):
    out = []
    s = _case(small_assets, 3, 68, 11, synth)
    rg, ce = synth.coefficient_prior(s["ns"], s["ne"], 0.5)
    out.append(("small, pose only", s, dict(), None))
    out.append(("small, pose only, damped", s, dict(weight=s["weight"]), np.array([1e-3, 0.5, 10.0])))
    out.append(("small, coefficients only", s, dict(pose_mask=0, fit_coef=True, ridge=rg, center=ce), None))
    out.append(("small, both", s, dict(fit_coef=True, ridge=rg, center=ce, weight=s["weight"]), np.array([0.0, 1e-3, 1.0])))
    f = _case(full_assets, 2, 68, 12, synth)
    rg, ce = synth.coefficient_prior(f["ns"], f["ne"], 0.5)
    out.append(("full, both", f, dict(fit_coef=True, ridge=rg, center=ce), np.array([1e-3, 1e-1])))
    return out


def test_model_solve_against_numpy(small_assets, full_assets, synth):
    """The model's delta (the right-looking Cholesky and the two substitutions, in the header's order) against numpy's own solve of
    the same (H + damp D) delta = -g, in the Jacobi-scaled norm: with S = diag(sqrt(A_ii)), |S (delta - delta_numpy)|_2 <=
    8 P kappa_2 2^-53 |S delta_numpy|_2, kappa_2 the condition number of S^-1 A S^-1 as numpy computes it -- the classical bound of a
    Cholesky solve.  kappa_2 <= 1e4 is asserted, so that the bound cannot hide a failure.  numpy is handed the scaled system
    (S^-1 A S^-1) (S delta) = -S^-1 g: its LU of the unscaled A -- condition 4e9 to 9e9 on these cases, the unknowns living on scales
    from 1e-3 to 1e4 -- is itself up to 216 units of 2^-53 off the exact rational solution in this norm where the model stays within
    1.3, so it could not referee; the scaled solve stays within 3.  The prediction is held to its formula."""
    for name, c, kw, damp in _solve_cases(small_assets, full_assets, synth):
        st = RS.Step(c["P"], c["mean"], c["U"], c["target"], damp=damp, **kw)
        assert st.ok.all(), name
        for b in range(c["B"]):
            A, g = st.A[b], st.g[b]
            assert np.array_equal(A, A.T)
            s = np.sqrt(np.diag(A))
            kappa = np.linalg.cond(A / s[:, None] / s[None, :])
            ref = np.linalg.solve(A / s[:, None] / s[None, :], -g / s) / s
            err = np.linalg.norm(s * (st.x[b] - ref))
            bound = 8 * st.Pn * kappa * 2.0 ** -53 * np.linalg.norm(s * ref)
            print("%s, face %d: P %d, kappa_2 %.4g, scaled error %.3g, bound %.3g" % (name, b, st.Pn, kappa, err, bound))
            assert kappa <= 1e4, (name, b, kappa)
            assert err <= bound, (name, b, err, bound)
            pred = st.F[b] + 2 * g @ ref + ref @ st.H[b] @ ref
            assert abs(st.cost[b, 1] - pred) <= 1e-10 * (abs(st.F[b]) + abs(pred)), (name, b)
            assert st.cost[b, 0] == st.F[b] and st.cost[b, 1] < st.cost[b, 0]
            assert np.array_equal(st.delta[b, st.cols], st.x[b])


def test_model_failure_rule(small_assets, synth):
    c = _case(small_assets, 4, 5, 13, synth)
    P = c["P"].copy()
    P[1, 6] = 0.0                                  # f = 0 with the angles fitted: their columns vanish
    P[3, 3] = np.inf                               # a non-finite parameter that is read
    weight = np.ones((4, 5), np.float32)
    weight[2] = 0.0                                # no landmark counts
    st = RS.Step(P, c["mean"], c["U"], c["target"], weight=weight)
    assert st.ok.tolist() == [1, 0, 0, 0]
    assert not st.delta[1:].any() and not np.signbit(st.delta[1:]).any()
    assert np.array_equal(st.cost[1:3, 0], st.cost[1:3, 1]) and st.cost[2, 0] == 0.0 and st.cost[0, 1] < st.cost[0, 0]
    alone = RS.Step(P[0:1], c["mean"], c["U"], c["target"][0:1], weight=weight[0:1])
    assert np.array_equal(alone.delta[0], st.delta[0]) and np.array_equal(alone.cost[0], st.cost[0])
    # f = 0 is no obstacle while only the translation is fitted
    t = RS.Step(P[0:3], c["mean"], c["U"], c["target"][0:3], pose_mask=RS.pose_mask(["tx", "ty"]))
    assert t.ok.tolist() == [1, 1, 1]


# ---- convergence -------------------------------------------------------------------------------------------------------------------------
def _fit_case(small_assets, synth, pose_noise):
    """the batch, the landmarks and the perturbed start of `photo_fit.py --small --fit-pose --landmarks-only --landmarks 68
    --pose-noise N`, as test_landmark_cpu.py::test_landmarks_only_fit_converges_in_the_model builds them"""
    ex = TL._photo_fit()
    args = ex.build_parser().parse_args(["--small", "--fit-pose", "--landmarks-only", "--landmarks", "68", "--pose-noise", str(pose_noise)])
    B, S = 3, 32
    A = small_assets
    ns, ne = A["ndim_shape"], A["ndim_exp"]
    idx = synth.landmark_ids(A, args.landmarks)
    P32 = RB.sample(args.seed, 0, B, ns, ne, 10, S, 0.7, [(0.0, 1.0)] * 4, [(-1.0, 1.0)] * 10, focal=1e-3 * S / 200.0)[0]
    mean, U = RL.split_image(RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], idx), len(idx), ns + ne)
    fw = RL.Forward(P32, mean, U, im_size=float(S))
    target64 = fw.points[:, 0:2].transpose(0, 2, 1).astype(np.float64)
    params = torch.as_tensor(P32)
    noise = ex.make_noise(args.seed, torch.device("cpu"))
    noise(torch.zeros(B, 4), args.light_noise)       # the example perturbs light and alpha first: the same draws, in the same order
    noise(torch.zeros(B, 10), args.alpha_noise)
    pose0, pose_scale = ex.pose_start(params[:, :7], noise, args.pose_noise)
    return dict(ex=ex, args=args, B=B, S=S, ns=ns, ne=ne, K=len(idx), mean=mean, U=U, P32=P32, params=params, target64=target64,
                pose0=pose0, pose_scale=pose_scale)


def test_pose_fit_converges_in_the_model(small_assets, synth):
    """Six Levenberg-Marquardt iterations on the pose, from four times the example's perturbation, noise-free targets: cost never
    increases, the final F is at most 1e-8 of the first, t3d stands within 1e-3 px of the truth, and F ends below what the example's
    own 100 Adam steps reach from the same start."""
    c = _fit_case(small_assets, synth, 4)
    ex, args, S, K = c["ex"], c["args"], c["S"], c["K"]
    target32 = c["target64"].astype(np.float32)
    assert np.array_equal(target32.astype(np.float64), c["target64"])          # (the forward's points are fp32 already)
    P0 = np.concatenate([c["pose0"].numpy(), c["P32"][:, 7:]], axis=1).astype(np.float32)
    fitted, info = RS.fit(P0, c["mean"], c["U"], target32, iters=6, im_size=float(S))
    cost = info["cost"]
    t3d = float(np.sqrt(np.mean((fitted[:, 3:6].astype(np.float64) - c["P32"][:, 3:6]) ** 2)))
    print("LM, pose only: F", " -> ".join("%.3g" % v for v in cost.sum(axis=1)), "; accepted", info["accepted"].sum(axis=1).tolist(),
          "; t3d_rms %.3g px" % t3d)
    assert np.isfinite(cost).all() and (np.diff(cost, axis=0) <= 0).all()
    assert (cost[-1] <= 1e-8 * cost[0]).all(), cost[-1] / cost[0]
    assert t3d <= 1e-3
    # the example's Adam loop on the same inputs
    pose = torch.zeros_like(c["pose0"], requires_grad=True)
    opt = torch.optim.Adam([{"params": [pose], "lr": args.lr}])
    mean_t, U_t, target_t = torch.as_tensor(c["mean"]), torch.as_tensor(c["U"]), torch.as_tensor(c["target64"])

    def sse_of():
        P = torch.cat([c["pose0"] + pose * c["pose_scale"], c["params"][:, 7:]], dim=1).double()
        return ((TL._torch_points(P, mean_t, U_t, float(S)) - target_t) ** 2).sum(dim=(1, 2))
    first, last = ex.descend(opt, lambda: args.landmark_lambda * (sse_of() / K).mean(), args.steps)
    adam = sse_of().detach().numpy()
    print("Adam, %d steps: loss %.4g -> %.4g, F %.4g against LM's %.4g" % (args.steps, first, last, adam.sum(), cost[-1].sum()))
    assert (cost[-1] < adam).all()


def test_coefficient_fit_converges_in_the_model(small_assets, synth):
    """Pose and coefficients, the coefficients from the prior's centre under the ridge of the sampler's variances, 0.5 px of landmark
    noise, five iterations: cost is non-increasing and the last two accepted values agree to 1e-3 relative."""
    c = _fit_case(small_assets, synth, 1)
    S = c["S"]
    rs = np.random.RandomState(3)
    target = (c["target64"] + 0.5 * rs.standard_normal(c["target64"].shape)).astype(np.float32)
    ridge, center = synth.coefficient_prior(c["ns"], c["ne"], 0.5)
    P0 = np.concatenate([c["pose0"].numpy(), np.broadcast_to(center, (c["B"], center.size))], axis=1).astype(np.float32)
    fitted, info = RS.fit(P0, c["mean"], c["U"], target, ridge=ridge, center=center, iters=5, fit_coef=True, im_size=float(S))
    cost, acc = info["cost"], info["accepted"]
    print("LM, pose and coefficients: F", " -> ".join("%.4g" % v for v in cost.sum(axis=1)), "; accepted", acc.sum(axis=1).tolist())
    assert np.isfinite(cost).all() and np.isfinite(fitted).all() and (np.diff(cost, axis=0) <= 0).all()
    for b in range(c["B"]):
        vals = [cost[0, b]] + [cost[i + 1, b] for i in range(acc.shape[0]) if acc[i, b]]
        assert len(vals) >= 3, (b, vals)
        assert abs(vals[-1] - vals[-2]) <= 1e-3 * vals[-2], (b, vals)
