"""numpy float64 model of the landmark term (include/fr_hotpath.h, "landmarks"): the basis gather, the forward, the sse and every
gradient, in exactly the header's order -- explicit loops over the coefficients j and the landmarks k, never `@` or `.sum()`, so that
every product and every sum is rounded on its own and in the stated sequence.  The kernels are held to this file bit for bit
(tests/test_landmark_gpu.py); tests/test_landmark_cpu.py holds its gradients to central differences of its own forward."""
import numpy as np

U24 = 2.0 ** -24


def basis_image(mu, pc_shape, pc_exp, idx):
    """-> the compact image as one fp32 vector: part A [Kt + 1][3K] (plane 0 the mean), then part B [3K][Kt]; row r = 3 k + c.
    An id outside [0, N) gives +0 rows."""
    mu = np.asarray(mu, np.float32).reshape(-1)
    pcs, pce = np.asarray(pc_shape, np.float32), np.asarray(pc_exp, np.float32)
    N = mu.shape[0] // 3
    idx = np.asarray(idx, np.int64).reshape(-1)
    K, Kt = idx.shape[0], pcs.shape[1] + pce.shape[1]
    rows = np.zeros((3 * K, Kt + 1), np.float32)
    for k in range(K):
        if 0 <= idx[k] < N:
            for c in range(3):
                r = c * N + idx[k]
                rows[3 * k + c, 0] = mu[r]
                rows[3 * k + c, 1:1 + pcs.shape[1]] = pcs[r]
                rows[3 * k + c, 1 + pcs.shape[1]:] = pce[r]
    return np.concatenate([rows.T.reshape(-1), rows[:, 1:].reshape(-1)])


def split_image(image, K, Kt):
    """the fp32 image -> (mean [K,3], U [K,3,Kt]) float64, from part A; part B must hold the same numbers"""
    image = np.asarray(image, np.float32)
    nA = (Kt + 1) * 3 * K
    A = image[:nA].reshape(Kt + 1, 3 * K)
    Bm = image[nA:].reshape(3 * K, Kt)
    assert np.array_equal(A[1:].T.view(np.uint32), Bm.view(np.uint32))
    return A[0].reshape(K, 3).astype(np.float64), A[1:].T.reshape(K, 3, Kt).astype(np.float64)


def _mat3(A, B):
    """[.., 3, 3] x [.., 3, 3] with the 3-term dots of csrc/fr_decode_shared.h::mat3_mul: (a0 b0 + a1 b1) + a2 b2"""
    C = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for i in range(3):
        for j in range(3):
            C[..., i, j] = (A[..., i, 0] * B[..., 0, j] + A[..., i, 1] * B[..., 1, j]) + A[..., i, 2] * B[..., 2, j]
    return C


def _factors(angles):
    """float64 angles [B,3] -> the six matrices (R_pitch, R_yaw, R_roll, dR_pitch, dR_yaw, dR_roll), each [B,3,3]
    (the conventions of tests/ref_pose_backward.py::rotation_f64)"""
    a = np.asarray(angles, np.float64)
    B = a.shape[0]
    sp, cp, sy, cy, st, ct = np.sin(a[:, 0]), np.cos(a[:, 0]), np.sin(a[:, 1]), np.cos(a[:, 1]), np.sin(a[:, 2]), np.cos(a[:, 2])
    o, z = np.ones(B), np.zeros(B)

    def m(*e):
        return np.stack(e, axis=1).reshape(B, 3, 3)
    return (m(o, z, z, z, cp, sp, z, -sp, cp), m(cy, z, -sy, z, o, z, sy, z, cy), m(ct, st, z, -st, ct, z, z, z, o),
            m(z, z, z, z, -sp, cp, z, -cp, -sp), m(-sy, z, -cy, z, z, z, cy, z, -sy), m(-st, ct, z, -ct, -st, z, z, z, z))


def rotation32(angles32):
    """fp32 angles [B,3] -> the fp32 matrix the dense decode uses: (R_pitch R_yaw) R_roll in float64, rounded once"""
    Rp, Ry, Rr = _factors(np.asarray(angles32, np.float32).astype(np.float64))[:3]
    return _mat3(_mat3(Rp, Ry), Rr).astype(np.float32)


def rotation_derivatives(angles32):
    """-> (dR [3][B,3,3] float64, dRabs [3][B,3,3]: the same products over the absolute values of the factors)"""
    Rp, Ry, Rr, dRp, dRy, dRr = _factors(np.asarray(angles32, np.float32).astype(np.float64))
    trip = [(dRp, Ry, Rr), (Rp, dRy, Rr), (Rp, Ry, dRr)]
    return ([_mat3(_mat3(a, b), c) for a, b, c in trip],
            [_mat3(_mat3(np.abs(a), np.abs(b)), np.abs(c)) for a, b, c in trip])


def _weights(weight, B, K):
    if weight is None:
        return np.ones((B, K))
    w = np.asarray(weight, np.float32).astype(np.float64)
    return np.broadcast_to(w, (B, K)) if w.ndim == 1 else w


class Forward:
    """The forward of B faces.  P [B, 7 + Kt] fp32, mean [K,3] / U [K,3,Kt] float64 (split_image), R None or [B,3,3] fp32,
    target None or [B,K,2] fp32, weight None, [K] or [B,K] fp32.
    Fields: v [B,K,3] (un-projected), Rv [B,K,3], xyz [B,K,3] float64 (before the rounding), points [B,3,K] fp32, sse [B] float64 or
    None, absterms [B,3,K] (the sum of the absolute values of each coordinate's terms).
    exact=True (the central-difference test only): the rotation of the angles is NOT rounded to fp32, so that the model is the
    derivative of forward_f64 at the widened parameters."""

    def __init__(self, P, mean, U, R=None, target=None, weight=None, im_size=200.0, exact=False):
        P = np.asarray(P, np.float32)
        B, K, Kt = P.shape[0], mean.shape[0], U.shape[2]
        assert P.shape[1] == 7 + Kt
        a = P[:, 7:].astype(np.float64)
        v = np.broadcast_to(mean[None], (B, K, 3)).copy()
        va = np.abs(v)
        for j in range(Kt):
            v = v + a[:, j, None, None] * U[None, :, :, j]
            va = va + np.abs(a[:, j, None, None] * U[None, :, :, j])
        self.override = R is not None
        R32 = rotation32(P[:, 0:3]) if R is None else np.asarray(R, np.float32).reshape(B, 3, 3)
        Rm = R32.astype(np.float64)
        if exact and R is None:
            Rp, Ry, Rr = _factors(P[:, 0:3].astype(np.float64))[:3]
            Rm = _mat3(_mat3(Rp, Ry), Rr)
        f = P[:, 6].astype(np.float64)
        t = P[:, 3:6].astype(np.float64)
        Rv = np.empty((B, K, 3))
        absq = np.empty((B, K, 3))
        for i in range(3):
            Rv[:, :, i] = (Rm[:, None, i, 0] * v[:, :, 0] + Rm[:, None, i, 1] * v[:, :, 1]) + Rm[:, None, i, 2] * v[:, :, 2]
            absq[:, :, i] = np.abs(f)[:, None] * (np.abs(Rm[:, None, i, :]) * va).sum(axis=2) + np.abs(t[:, None, i])
        q = f[:, None, None] * Rv + t[:, None, :]
        xyz = q.copy()
        xyz[:, :, 1] = (float(im_size) - q[:, :, 1]) - 1.0
        absq[:, :, 1] += abs(float(im_size)) + 1.0
        self.P, self.a, self.R, self.f, self.t, self.im_size = P, a, Rm, f, t, float(im_size)
        self.v, self.Rv, self.xyz = v, Rv, xyz
        self.points = np.ascontiguousarray(xyz.transpose(0, 2, 1)).astype(np.float32)
        self.absterms = np.ascontiguousarray(absq.transpose(0, 2, 1))
        self.w = _weights(weight, B, K)
        self.target = None if target is None else np.asarray(target, np.float32).astype(np.float64).reshape(B, K, 2)
        self.sse = None
        if target is not None:
            sse = np.zeros(B)
            with np.errstate(invalid="ignore"):
                for k in range(K):
                    dx = xyz[:, k, 0] - self.target[:, k, 0]
                    dy = xyz[:, k, 1] - self.target[:, k, 1]
                    term = self.w[:, k] * (dx * dx + dy * dy)
                    sse = sse + np.where(self.w[:, k] != 0, term, 0.0)   # (adding +0 to a sum that started at +0 is skipping)
            self.sse = sse


class Backward:
    """The gradients of a Forward `fw` over the same U.  grad_points None or [B,3,K] fp32, grad_sse None or [B] float64.
    Fields: grad_params [B, 7 + Kt] fp32 (angle columns +0 unless pose_grad and no override), grad_R [B,3,3] fp32 or None (override
    with pose_grad), params64 / G64 the unrounded float64 values, angle_S [B,3] = the sum of the absolute terms of each angle's
    gradient (for the bound on the angle columns)."""

    def __init__(self, fw, U, grad_points=None, grad_sse=None, pose_grad=False):
        assert grad_points is not None or grad_sse is not None
        B, K, Kt = fw.v.shape[0], fw.v.shape[1], U.shape[2]
        g = np.zeros((B, K, 3))
        if grad_points is not None:
            g = np.asarray(grad_points, np.float32).astype(np.float64).transpose(0, 2, 1).copy()
        if grad_sse is not None:
            assert fw.target is not None
            gs = np.asarray(grad_sse, np.float64)
            with np.errstate(invalid="ignore"):
                s = gs[:, None] * (2.0 * fw.w)
                live = fw.w != 0
                g[:, :, 0] = np.where(live, g[:, :, 0] + s * (fw.xyz[:, :, 0] - fw.target[:, :, 0]), g[:, :, 0])
                g[:, :, 1] = np.where(live, g[:, :, 1] + s * (fw.xyz[:, :, 1] - fw.target[:, :, 1]), g[:, :, 1])
        dq = g.copy()
        dq[:, :, 1] = -g[:, :, 1]
        R, Rv, v, f = fw.R, fw.Rv, fw.v, fw.f
        ft = (dq[:, :, 0] * Rv[:, :, 0] + dq[:, :, 1] * Rv[:, :, 1]) + dq[:, :, 2] * Rv[:, :, 2]
        rt = np.empty((B, K, 3))
        for c in range(3):
            rt[:, :, c] = (R[:, None, 0, c] * dq[:, :, 0] + R[:, None, 1, c] * dq[:, :, 1]) + R[:, None, 2, c] * dq[:, :, 2]
        gt, gf, G, ga = np.zeros((B, 3)), np.zeros(B), np.zeros((B, 3, 3)), np.zeros((B, Kt))
        for k in range(K):
            gt = gt + dq[:, k, :]
            gf = gf + ft[:, k]
            G = G + dq[:, k, :, None] * v[:, k, None, :]
            for c in range(3):
                ga = ga + rt[:, k, c, None] * U[None, k, c, :]
        G = f[:, None, None] * G
        out = np.zeros((B, 7 + Kt))
        out[:, 3:6], out[:, 6], out[:, 7:] = gt, gf, f[:, None] * ga
        self.angle_S = np.zeros((B, 3))
        self.grad_R = None
        if pose_grad and fw.override:
            self.grad_R = G.astype(np.float32)
        elif pose_grad:
            dR, dRabs = rotation_derivatives(fw.P[:, 0:3])
            for a in range(3):
                s = np.zeros(B)
                for i in range(3):
                    for j in range(3):
                        s = s + G[:, i, j] * dR[a][:, i, j]
                        self.angle_S[:, a] += np.abs(G[:, i, j]) * dRabs[a][:, i, j]
                out[:, a] = s
        self.G64, self.params64 = G, out
        self.grad_params = out.astype(np.float32)


def forward_f64(P64, mean, U, R64=None, im_size=200.0):
    """The same forward as a smooth float64 function of float64 parameters (no fp32 rounding anywhere, the rotation of the angles
    exact): what the central differences of tests/test_landmark_cpu.py differentiate.  -> xyz [B,K,3]"""
    P64 = np.asarray(P64, np.float64)
    if R64 is None:
        Rp, Ry, Rr = _factors(P64[:, 0:3])[:3]
        R64 = _mat3(_mat3(Rp, Ry), Rr)
    v = mean[None] + np.einsum("bj,kcj->bkc", P64[:, 7:], U)
    q = P64[:, 6, None, None] * np.einsum("bic,bkc->bki", R64, v) + P64[:, None, 3:6]
    q[:, :, 1] = (float(im_size) - q[:, :, 1]) - 1.0
    return q


def landmark_loss(sse, weight, B, K):
    """the mean over faces of sse_b / max(sum_k w_k, 1) (nets/losses.py::landmark_loss), float64"""
    w = _weights(weight, B, K)
    return float(np.mean(np.asarray(sse, np.float64) / np.maximum(w.sum(axis=1), 1.0)))
