"""float64 reference of the pose gradients (fr_decode_pose_backward, fr_decode_render_backward_pose) and the magnitudes behind the
bound tests/test_pose_backward_gpu.py holds the kernels to.  numpy only; of the oracle it uses rotation_matrix_batch alone.

The forward (nets/network.py:140-171):  q = f R v + t,  out = (q_0, (im - q_1) - 1, q_2),  L = sum g . out.  With
dq = (g_x, -g_y, g_z) the gradient with respect to the nine entries of R is

    G = dL/dR = f sum_p dq_p v_p^T                                (formed here directly from the un-projected vertices v)

and, when R is the rotation of the three angles, d angle = <G, dR/d angle>.  The kernels never see v: they form the pose moment
A = sum_p dq_p (q_p - t)^T from the forward's fp32 output and G = A cof(R) / det(R); the two agree in exact arithmetic for every
invertible R.  det(R) == 0 is DEFINED as G = 0 (include/fr_hotpath.h); f == 0 gives G = 0 by itself.
tests/test_pose_backward_cpu.py holds this file to central differences of decode_f64."""
import numpy as np

U = 2.0 ** -24


def rotation_f64(angles):
    """[B,3] angles -> (R, dR/dphi, dR/dgamma, dR/dtheta), each [B,3,3] float64: R = R_pitch R_yaw R_roll (network.py:276-290)"""
    a = np.asarray(angles, np.float64)
    B = a.shape[0]
    out = np.zeros((4, B, 3, 3))
    for b in range(B):
        sp, cp, sy, cy, st, ct = np.sin(a[b, 0]), np.cos(a[b, 0]), np.sin(a[b, 1]), np.cos(a[b, 1]), np.sin(a[b, 2]), np.cos(a[b, 2])
        Rp = np.array([[1, 0, 0], [0, cp, sp], [0, -sp, cp]])
        Ry = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
        Rr = np.array([[ct, st, 0], [-st, ct, 0], [0, 0, 1]])
        dRp = np.array([[0, 0, 0], [0, -sp, cp], [0, -cp, -sp]])
        dRy = np.array([[-sy, 0, -cy], [0, 0, 0], [cy, 0, -sy]])
        dRr = np.array([[-st, ct, 0], [-ct, -st, 0], [0, 0, 0]])
        out[0, b] = Rp @ Ry @ Rr
        out[1, b] = dRp @ Ry @ Rr
        out[2, b] = Rp @ dRy @ Rr
        out[3, b] = Rp @ Ry @ dRr
    return out[0], out[1], out[2], out[3]


def decode_f64(v, R, t, f, im_size):
    """v [B,3,N], R [B,3,3], t [B,3], f [B] (float64) -> the projected, y-flipped vertices [B,3,N] in float64"""
    q = np.einsum("bij,bjp->bip", R, v) * f[:, None, None] + t[:, :, None]
    q[:, 1] = (im_size - q[:, 1]) - 1.0
    return q


def unprojected_f64(assets, P):
    """v = mu + pc_shape alpha + pc_exp beta in float64, [B,3,N] (blocked rows: element r = coordinate r / N of vertex r % N)"""
    mu = np.asarray(assets["mu"], np.float64).reshape(-1)
    pcs, pce = np.asarray(assets["pc_shape"], np.float64), np.asarray(assets["pc_exp"], np.float64)
    ns = pcs.shape[1]
    x = np.asarray(P, np.float32).astype(np.float64)[:, 7:]
    v = mu[None] + x[:, :ns] @ pcs.T + x[:, ns:] @ pce.T
    return v.reshape(P.shape[0], 3, -1)


def cofactor(R):
    """[B,3,3] -> (cof(R) [B,3,3], det(R) [B]) in float64"""
    r = np.asarray(R, np.float64)
    c = np.empty_like(r)
    for i in range(3):
        for j in range(3):
            i1, i2 = (i + 1) % 3, (i + 2) % 3
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            c[:, i, j] = r[:, i1, j1] * r[:, i2, j2] - r[:, i1, j2] * r[:, i2, j1]
    return c, (r[:, 0] * c[:, 0]).sum(1)


class PoseRef:
    """The float64 pose gradients of B faces.
        G [B,3,N] fp32 gradient of the forward output, v [B,3,N] float64 un-projected vertices, P [B, >= 7] fp32 parameters,
        R None (the rotation of the angles: oracle.rotation_matrix_batch, the fp32 matrix the forward uses) or [B,3,3] fp32.
    Fields: grad_R [B,3,3]; angles [B,3] (zeros under an override); V the exact forward output; and, for the bound,
    S [B,3,3] = sum_p |dq_i| |q_k - t_k| (the absolute terms of the pose moment), dqa = |dq|, cofa = |cof(R)| / |det(R)|,
    Rabs, dRabs [3][B,3,3] = |dR/d angle|, singular [B] (det == 0)."""

    def __init__(self, oracle, G, v, P, R=None, im_size=200.0):
        P = np.asarray(P, np.float32)
        B = P.shape[0]
        self.override = R is not None
        R32 = oracle.rotation_matrix_batch(P[:, 0:3]) if R is None else np.asarray(R, np.float32)
        Rm = R32.astype(np.float64)
        f = P[:, 6].astype(np.float64)
        t = P[:, 3:6].astype(np.float64)
        dq = np.asarray(G, np.float32).astype(np.float64).copy()
        dq[:, 1] = -dq[:, 1]
        v = np.asarray(v, np.float64)
        cof, det = cofactor(Rm)
        self.singular = det == 0
        ok = (~self.singular).astype(np.float64)[:, None, None]
        self.grad_R = f[:, None, None] * np.einsum("bip,bkp->bik", dq, v) * ok
        _, d0, d1, d2 = rotation_f64(P[:, 0:3].astype(np.float64))
        self.angles = np.zeros((B, 3))
        if not self.override:
            for k, d in enumerate((d0, d1, d2)):
                self.angles[:, k] = (self.grad_R * d).sum(axis=(1, 2))
        self.V = decode_f64(v, Rm, t, f, im_size)
        qt = np.abs(f)[:, None, None] * np.abs(np.einsum("bij,bjp->bip", Rm, v))      # |q - t|
        self.dqa = np.abs(dq)
        self.S = np.einsum("bip,bkp->bik", self.dqa, qt)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.cofa = np.where(self.singular[:, None, None], 0.0, np.abs(cof) / np.abs(det)[:, None, None])
        self.Rabs = np.abs(Rm)
        self.dRabs = [np.abs(d) for d in (d0, d1, d2)]
        self.t, self.f, self.im_size = t, f, float(im_size)

    def bound(self, Vg, depth):
        """-> (bound on grad_R [B,3,3], bound on the angles [B,3]) for a kernel that starts from the fp32 forward output Vg and
        whose longest chain of rounded fp32 additions is `depth` (the fourth value of fr_debug_pose_bwd_geom).
          * E_q = |Vg - V| + 2 u (|Vg| + |t| + im): how far the kernel's (q - t) is from the exact one -- the measured distance of
            the forward output from the exact projection plus the (im - 1) - y and - t roundings;  E1 = sum_p |dq_i| E_q,k;
          * each term has 3 roundings, the sum `depth` more, the fp32 output one:  |A~ - A| <= E1 + gamma(depth + 4) (S + E1);
          * G = A cof / det:  through |cof| / |det|;  an in-kernel rotation may differ from the host's by an ulp, which moves
            R^-T by R^-T dR^T R^-T:  + 2 u (S |cof| / |det|) |R|^T |cof| / |det|;
          * angles: through |dR / d angle|.
        A factor 1.01 covers the second-order terms and the float64 steps.  Nothing is fitted."""
        Vg = np.asarray(Vg, np.float32).astype(np.float64)
        Eq = np.abs(Vg - self.V) + 2 * U * (np.abs(Vg) + np.abs(self.t)[:, :, None] + self.im_size)
        E1 = np.einsum("bip,bkp->bik", self.dqa, Eq)
        n = depth + 4
        gamma = n * U / (1.0 - n * U)
        bA = 1.01 * (E1 + gamma * (self.S + E1))
        bG = np.einsum("bik,bkj->bij", bA, self.cofa)
        if not self.override:
            SG = np.einsum("bik,bkj->bij", self.S + E1, self.cofa)
            bG = bG + 1.01 * 2 * U * np.einsum("bik,bkj->bij", SG, np.einsum("bki,bkj->bij", self.Rabs, self.cofa))
        bang = np.zeros((Vg.shape[0], 3))
        if not self.override:
            for k in range(3):
                bang[:, k] = (bG * self.dRabs[k]).sum(axis=(1, 2)) * 1.01
        return bG, bang


# ---- the inputs of the C-level GPU cases (generated from seeds; the CPU suite checks the discrimination cap on them) ------------
NS, NE = 20, 5


def rotations(rs, B):
    """random proper rotations (QR of a Gaussian matrix in float64, rounded to fp32): not the rotation of any face's angles"""
    R = np.empty((B, 3, 3), np.float32)
    for b in range(B):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))[None, :]
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        R[b] = q
    return R


def case_list(chunk):
    """(name, seed, B, N, mode, f0): mode None = rotation evaluated from the angles, "rot" = random rotations as R_override,
    "skew" = a mildly non-orthogonal override, "sing" = face 0's override singular; f0: face B // 2 has f = 0.
    Every N of {1, 7, 15, 16, 17, 4270, chunk + 1, chunk - 1} and every B of {1, 17, 64, 65} appears."""
    return [("n1", 1, 17, 1, None, False), ("n7", 2, 1, 7, "rot", False), ("n15", 3, 17, 15, None, False),
            ("n16", 4, 65, 16, "rot", False), ("n17", 5, 64, 17, None, False), ("mesh", 6, 17, 4270, None, False),
            ("mesh_rot", 7, 1, 4270, "rot", False), ("above", 8, 17, chunk + 1, None, False),
            ("below", 9, 17, chunk - 1, "rot", False), ("b64", 10, 64, 1000 + 7, None, True),
            ("b65", 11, 65, 1000 + 7, "rot", True), ("skew", 12, 17, 4270, "skew", False),
            ("sing", 13, 17, 1000 + 7, "sing", False)]


def make_case(seed, B, N, mode, f0, im_size=200.0):
    """-> dict(P [B,32] fp32, G [B,3,N] fp32, v [B,3,N] float64, R fp32 [B,3,3] or None, Vg [B,3,N] fp32): the input scale recipe
    of tests/test_decode_backward_bounds_gpu.py (per-face gradient scale 2^U(-20, 20), per-value magnitudes standard normal times
    exp(U(-6, 6)), f in [2e-4, 1e-3]); the un-projected vertices are drawn directly (the pose gradient reads no basis), of the
    model's magnitude (1e5), and the forward output handed to the kernel is the exact projection rounded to fp32."""
    rs = np.random.RandomState(1000 + seed)
    P = np.zeros((B, 7 + NS + NE), np.float32)
    P[:, 0:3] = rs.uniform(-1.0, 1.0, (B, 3))
    P[:, 3:5] = rs.uniform(60, 140, (B, 2))
    P[:, 5] = rs.uniform(-1, 1, B)
    P[:, 6] = rs.uniform(2e-4, 1e-3, B)
    P[:, 7:7 + NS] = rs.uniform(0, 1e4, (B, NS))
    P[:, 7 + NS:] = rs.uniform(-1.5, 1.5, (B, NE))
    face = 2.0 ** rs.uniform(-20, 20, (B, 1, 1))
    G = (rs.standard_normal((B, 3, N)) * np.exp(rs.uniform(-6, 6, (B, 3, N))) * face).astype(np.float32)
    v = rs.uniform(-1e5, 1e5, (B, 3, N))
    R = None
    if mode is not None:
        R = rotations(rs, B)
        if mode == "skew":
            R = (R.astype(np.float64) @ (np.eye(3) + 0.1 * rs.uniform(-1, 1, (B, 3, 3)))).astype(np.float32)
        if mode == "sing":
            R[0, 2] = R[0, 0]
    if f0:
        P[B // 2, 6] = 0.0
    from oracle import oracle as O
    Rm = (O.rotation_matrix_batch(P[:, 0:3]) if R is None else R).astype(np.float64)
    V = decode_f64(v, Rm, P[:, 3:6].astype(np.float64), P[:, 6].astype(np.float64), im_size)
    return dict(P=P, G=G, v=v, R=R, Vg=V.astype(np.float32))
