"""numpy float64 model of the landmark solver (include/fr_hotpath.h, "landmark solver"): one damped Gauss-Newton step in the header's
order -- explicit loops over the rows, the columns of the factorisation and the substitution, never `@` or `.sum()`, so that every
product and every sum is rounded on its own and in the stated sequence -- and the Levenberg-Marquardt loop of
rendering_layer/ops.py::landmark_fit around it.  The forward (v, R, x, y, sse) is tests/ref_landmark.py's.

Where the model and the kernel may differ: the coefficient-coefficient block of J^T W J, which the kernel forms on the float64 matrix
cores (this model adds its terms one by one in row order, each product rounded before it is added); and the angle columns, whose
rotation derivatives start from the device's own double sincos.  tests/test_landmark_solve_gpu.py bounds both."""
import numpy as np

import ref_landmark as RL

POSE_NAMES = ("phi", "gamma", "theta", "tx", "ty", "f")
POSE_BITS = (0, 1, 2, 3, 4, 6)          # the parameter column (= the mask bit) of each pose slot
ALL_POSE = 0x5F


def pose_mask(names):
    m = 0
    for n in names:
        m |= 1 << POSE_BITS[POSE_NAMES.index(n)]
    return m


def _f64(x):
    return None if x is None else np.asarray(x, np.float32).astype(np.float64)


class Step:
    """One step of B faces.  P [B, 7 + Kt] fp32, mean / U of RL.split_image, target [B,K,2] fp32, weight None, [K] or [B,K] fp32, ridge
    and center None or [Kt] fp32, damp None or [B] float64, pose_mask as in the header, fit_coef.
    Fields: delta [B, 7 + Kt], cost [B,2], ok [B] int32 (the outputs); cols (the parameter column of every unknown), J [B,2K,P],
    wrow [B,2K], r [B,2K], H [B,P,P] (symmetric, with the ridge), g [B,P], D [B,P], A = H + damp D, x [B,P] (the solution before the
    failure rule), Jabs [B,2K,P] (the sum of the absolute values of the terms of every Jacobian entry: equal to |J| outside the
    angle columns).  exact=True (the central-difference test only): rotation and derivatives from the unrounded angles."""

    def __init__(self, P, mean, U, target, weight=None, ridge=None, center=None, damp=None, pose_mask=ALL_POSE, fit_coef=False,
                 im_size=200.0, exact=False):
        P = np.asarray(P, np.float32)
        B, K, Kt = P.shape[0], mean.shape[0], U.shape[2]
        coef = bool(fit_coef) and Kt > 0
        assert not (pose_mask & ~ALL_POSE) and (pose_mask or coef)
        with np.errstate(all="ignore"):
            fw = RL.Forward(P, mean, U, target=target, weight=weight, im_size=im_size, exact=exact)
            self.fw = fw
            live = fw.w != 0                                                    # [B,K]
            v, Rv, R, f = fw.v, fw.Rv, fw.R, fw.f
            dR, dRabs = RL.rotation_derivatives(P[:, 0:3])
            slots = [s for s in range(6) if (pose_mask >> POSE_BITS[s]) & 1]
            n_pose = len(slots)
            Pn = n_pose + (Kt if coef else 0)
            self.cols = [POSE_BITS[s] for s in slots] + ([7 + j for j in range(Kt)] if coef else [])
            J = np.zeros((B, 2 * K, Pn))
            Jabs = np.zeros((B, 2 * K, Pn))
            one = np.ones((B, K))
            for i, s in enumerate(slots):
                if s < 3:
                    e0 = (dR[s][:, None, 0, 0] * v[:, :, 0] + dR[s][:, None, 0, 1] * v[:, :, 1]) + dR[s][:, None, 0, 2] * v[:, :, 2]
                    e1 = (dR[s][:, None, 1, 0] * v[:, :, 0] + dR[s][:, None, 1, 1] * v[:, :, 1]) + dR[s][:, None, 1, 2] * v[:, :, 2]
                    jx, jy = f[:, None] * e0, -(f[:, None] * e1)
                    ax = np.abs(f)[:, None] * (dRabs[s][:, None, 0, :] * np.abs(v)).sum(axis=2)
                    ay = np.abs(f)[:, None] * (dRabs[s][:, None, 1, :] * np.abs(v)).sum(axis=2)
                elif s == 3:
                    jx, jy = one, 0.0 * one
                    ax, ay = np.abs(jx), np.abs(jy)
                elif s == 4:
                    jx, jy = 0.0 * one, -one
                    ax, ay = np.abs(jx), np.abs(jy)
                else:
                    jx, jy = Rv[:, :, 0], -Rv[:, :, 1]
                    ax, ay = np.abs(jx), np.abs(jy)
                J[:, 0::2, i], J[:, 1::2, i] = np.where(live, jx, 0.0), np.where(live, jy, 0.0)
                Jabs[:, 0::2, i], Jabs[:, 1::2, i] = np.where(live, ax, 0.0), np.where(live, ay, 0.0)
            if coef:
                u0 = (R[:, None, 0, 0, None] * U[None, :, 0, :] + R[:, None, 0, 1, None] * U[None, :, 1, :]) \
                    + R[:, None, 0, 2, None] * U[None, :, 2, :]                # [B,K,Kt]
                u1 = (R[:, None, 1, 0, None] * U[None, :, 0, :] + R[:, None, 1, 1, None] * U[None, :, 1, :]) \
                    + R[:, None, 1, 2, None] * U[None, :, 2, :]
                J[:, 0::2, n_pose:] = np.where(live[:, :, None], f[:, None, None] * u0, 0.0)
                J[:, 1::2, n_pose:] = np.where(live[:, :, None], -(f[:, None, None] * u1), 0.0)
                Jabs[:, :, n_pose:] = np.abs(J[:, :, n_pose:])
            r = np.zeros((B, 2 * K))
            r[:, 0::2] = np.where(live, fw.xyz[:, :, 0] - fw.target[:, :, 0], 0.0)
            r[:, 1::2] = np.where(live, fw.xyz[:, :, 1] - fw.target[:, :, 1], 0.0)
            wrow = np.repeat(fw.w, 2, axis=1)
            WJ = wrow[:, :, None] * J
            M = np.zeros((B, Pn, Pn))                                            # entry (i, j), i >= j: sum of (w J_i) J_j
            gJ = np.zeros((B, Pn))
            for row in range(2 * K):
                M = M + WJ[:, row, :, None] * J[:, row, None, :]
                gJ = gJ + WJ[:, row, :] * r[:, row, None]
            low = np.tril(np.ones((Pn, Pn), bool))
            M = np.where(low, M, M.transpose(0, 2, 1))                           # (the lower triangle mirrored)
            D = np.einsum("bii->bi", M).copy()
            g = gJ.copy()
            F = fw.sse.copy()
            rg = np.zeros(Kt) if ridge is None else _f64(ridge)
            ce = np.zeros(Kt) if center is None else _f64(center)
            H = M.copy()
            if coef:
                dj = fw.a - ce[None]
                g[:, n_pose:] = gJ[:, n_pose:] + rg[None] * dj
                prior = np.zeros(B)
                for j in range(Kt):
                    prior = prior + rg[j] * (dj[:, j] * dj[:, j])
                F = fw.sse + prior
                idx = np.arange(n_pose, Pn)
                H[:, idx, idx] = D[:, n_pose:] + rg[None]
            dm = np.zeros(B) if damp is None else np.asarray(damp, np.float64)
            A = H.copy()
            ii = np.arange(Pn)
            A[:, ii, ii] = H[:, ii, ii] + dm[:, None] * D
            # right-looking Cholesky on the triangle with -g as row Pn
            Aug = np.concatenate([A, -g[:, None, :]], axis=1)                    # [B, Pn + 1, Pn]
            okf = np.ones(B, bool)
            diag = np.ones((B, Pn))
            for c in range(Pn):
                d = Aug[:, c, c]
                okf &= (d > 0) & np.isfinite(d)
                diag[:, c] = np.sqrt(np.where(okf, d, 1.0))
                col = Aug[:, c + 1:, c] / diag[:, c, None]
                Aug[:, c + 1:, c] = col
                Aug[:, c + 1:, c + 1:] = Aug[:, c + 1:, c + 1:] - col[:, :, None] * col[:, None, :Pn - c - 1]
            y = Aug[:, Pn, :].copy()
            x = np.zeros((B, Pn))
            for c in range(Pn - 1, -1, -1):
                x[:, c] = y[:, c] / diag[:, c]
                y[:, :c] = y[:, :c] - Aug[:, c, :c] * x[:, c, None]
            q = np.zeros((B, Pn))
            for j in range(Pn):
                q = q + H[:, :, j] * x[:, j, None]
            e = x * (2.0 * g + q)
            m = np.zeros(B)
            for i in range(Pn):
                m = m + e[:, i]
            pred = F + m
            fail = ~okf | ~np.isfinite(x).all(axis=1) | ~np.isfinite(F) | ~np.isfinite(pred)
        self.J, self.Jabs, self.wrow, self.r, self.H, self.g, self.D, self.A, self.x, self.F, self.pred = J, Jabs, wrow, r, H, g, D, A, x, F, pred
        self.n_pose, self.Pn, self.slots = n_pose, Pn, slots
        self.ok = (~fail).astype(np.int32)
        self.delta = np.zeros((B, 7 + Kt))
        self.delta[:, self.cols] = np.where(fail[:, None], 0.0, x)
        self.cost = np.stack([F, np.where(fail, F, pred)], axis=1)


def objective(P, mean, U, target, weight=None, ridge=None, center=None, fit_coef=False, im_size=200.0):
    """F [B] of fp32 parameters: the forward's sse plus, with fit_coef, the prior -- as landmark_fit evaluates a candidate"""
    with np.errstate(all="ignore"):
        fw = RL.Forward(P, mean, U, target=target, weight=weight, im_size=im_size)
        F = fw.sse.copy()
        if fit_coef and ridge is not None and U.shape[2] > 0:
            d = fw.a - (0.0 if center is None else _f64(center)[None])
            F = F + (_f64(ridge)[None] * d * d).sum(axis=1)
    return F


def fit(P, mean, U, target, weight=None, ridge=None, center=None, iters=10, damp0=1e-3, pose_mask=ALL_POSE, fit_coef=False,
        im_size=200.0):
    """The loop of rendering_layer/ops.py::landmark_fit -> (params [B, 7 + Kt] fp32, dict(cost [iters + 1, B], accepted [iters, B],
    damp [B]))"""
    cur = np.asarray(P, np.float32).copy()
    B = cur.shape[0]
    damp = np.full(B, float(damp0))
    kw = dict(weight=weight, ridge=ridge, center=center, fit_coef=fit_coef, im_size=im_size)
    F = objective(cur, mean, U, target, **kw)
    costs, accepted = [F], []
    for _ in range(int(iters)):
        st = Step(cur, mean, U, target, damp=damp, pose_mask=pose_mask, **kw)
        cand = (cur.astype(np.float64) + st.delta).astype(np.float32)
        F_new = objective(cand, mean, U, target, **kw)
        with np.errstate(invalid="ignore"):
            acc = (st.ok != 0) & (F_new < F)
        cur = np.where(acc[:, None], cand, cur)
        F = np.where(acc, F_new, F)
        damp = np.where(acc, np.maximum(damp / 3.0, 1e-9), np.minimum(damp * 4.0, 1e9))
        costs.append(F)
        accepted.append(acc)
    return cur, dict(cost=np.stack(costs), accepted=np.stack(accepted) if accepted else np.zeros((0, B), bool), damp=damp)
