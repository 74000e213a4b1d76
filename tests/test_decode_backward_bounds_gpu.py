"""GPU: the decode backward (fr_decode_3dmm_backward{,_packed,_packed_mu}) held to the float64 gradient by a PROVEN bound, at every
launch shape its launcher can take, plus the bit-level invariants its fixed summation order promises.

The three entry points:
  "packed" -- bwd_fused_kernel<NB, CB> + bwd_reduce_kernel, d f from the forward's output (the autograd default);
  "mu"     -- the same fused kernel with d f from mu and the coefficient gradients (`basis.backward_from_mu`);
  "ref"    -- the reference-layout path bwd_prepass_kernel + bwd_gemm_kernel<NB> + bwd_reduce_kernel (bases of more than 16
              coefficient blocks, meshes of fewer than 16 vertices).

The bound.  Every output is a sum of float64 terms t_i; the kernel forms each term with a few fp32 roundings and adds them up
along a tree whose longest path has D roundings.  With u = 2^-24 and gamma(n) = n u / (1 - n u) the standard recursive-summation
argument gives |got - want| <= gamma(D + c) * sum_i |t~_i|, where t~_i bounds the kernel's own term (below).  D is derived from
the launch geometry the launcher itself reports (fr_debug_decode_bwd_geom, under the knobs of the run), per entry point:
  * bwd_reduce_kernel over nk partials: wave w takes m <= ceil(nk / 16) of them; its sixteen- and eight-wide loops add one
    partial per eight to each of eight chains, and the m % 8 left over all go to chain 0, so the longest chain has
    floor(m / 8) + m % 8 adds; a 3-level tree joins the eight, the 16 wave sums are added in order: _red_depth(nk), the
    maximum over the 16 waves' m.
  * fused kernel, coefficients: one product + one MFMA accumulation per basis row (4 rows per k-step, each added once) over the
    48 rows (16 vertices x 3 coordinates) of each of the workgroup's groups_per_block vertex groups, then the slab sum:
    1 + 48 gpb + red(blocks).  d t3d: 4 vertices per group in each staging thread's chain (4 gpb), the 2-step DPP quad sum, then
    red(blocks).  d f (vertex_proj form): 3 roundings of the per-vertex fma chain + that chain + fl(1/f) and the product (2).
  * reference-layout path: rows_per_block rows per GEMM workgroup, one accumulation per row; the
    prepass sums 64 vertices per workgroup in a 6-level DPP tree; then red(gemm / prepass blocks).
  * mu form of d f: dv (4) + product (1) + the fp32 partial coefficient gradients (48 gpb) + the per-lane fma chain over its
    4 CB slots + the 4 x waves (wave, k-row) partials + the add to the pose partial + red(blocks) + fl(1/f) and the product (2).
c and the terms t~:
  * dv = fmaf chain of fl(f R_ic) dq_i: |dv~ - dv| <= 4 u w with w = |f| |R|^T |dq| (NOT |dv|: dv may cancel), and an in-kernel R
    may differ from the host one by an ulp (1 more): coefficient k uses c = 5 and Sw_k = |pc_k|^T w >= S_k.
  * d t3d: the terms dq are exact: S (the oracle's sum of |dq|).
  * d f from vertex_proj: the kernel's term (q_i - t_i) dq_i / f starts from the fp32 FORWARD output, whose distance from the
    exact projection E_q = |V_gpu - V_exact| + 2 u (|V_gpu| + |t| + im_size) (the (im - 1) - y and - t roundings) is measured,
    not assumed: |err| <= E1 + gamma(D_f) (S_f + E1), E1 = sum |dq| E_q / |f|.
  * d f from mu: f d f = sum_p mu_p . dv_p + alpha . d alpha + beta . d beta; its terms are bounded by
    T = (sum |mu| w + sum_k |x_k| Sw_k) / |f|.
A global factor 1.01 covers the second-order terms.  Nothing is fitted: the bound cannot flake.

The per-face bar: 2e-5 of each face's OWN block maximum (d t3d, d f, d alpha, d beta), with the floor max(|want|, 1e-2 S) for the
single-value blocks d t3d and d f.  Inputs: per-face gradient scale 2^U(-20, 20), per-value magnitudes standard normal times
exp(U(-6, 6)); f in [2e-4, 1e-3] and basis entries ~1e-2 keep the smallest terms near 1e-11 -- far from fp32 subnormals."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import net_mod

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
IM = 200.0
DEV = torch.device("cuda:0")
KINDS = ("packed", "mu", "ref")
STATS = {}


def _h():
    return pkg("_lib")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _inputs(rs, B, N, ns, ne):
    P = np.zeros((B, 7 + ns + ne), np.float32)
    P[:, 0:3] = rs.uniform(-1.0, 1.0, (B, 3))
    P[:, 3:5] = rs.uniform(60, 140, (B, 2))
    P[:, 5] = rs.uniform(-1, 1, B)
    P[:, 6] = rs.uniform(2e-4, 1e-3, B)
    P[:, 7:7 + ns] = rs.uniform(0, 1e4, (B, ns))
    P[:, 7 + ns:] = rs.uniform(-1.5, 1.5, (B, ne))
    face = 2.0 ** rs.uniform(-20, 20, (B, 1, 1))
    G = (rs.standard_normal((B, 3, N)) * np.exp(rs.uniform(-6, 6, (B, 3, N))) * face).astype(np.float32)
    return P, G


def _rotations(rs, B):
    """random proper rotations (QR of a Gaussian matrix in float64, rounded to fp32): not the rotation of any face's angles"""
    R = np.empty((B, 3, 3), np.float32)
    for b in range(B):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))[None, :]
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        R[b] = q
    return R


# ---- the float64 reference and the magnitudes behind the bound ------------------------------------------------------------------
class Ref:
    def __init__(self, oracle, A, P, G, R=None, fields=None):
        if fields is not None:
            self.__dict__.update(fields)
            return
        mu = np.asarray(A["mu"], np.float32).reshape(-1)
        pcs, pce = A["pc_shape"], A["pc_exp"]
        ns, ne = pcs.shape[1], pce.shape[1]
        B, N = P.shape[0], mu.shape[0] // 3
        self.want, self.S = oracle.decode_3dmm_backward_f64(G, P, mu, pcs, pce, R=R, abs_sum=True)
        Rm = (oracle.rotation_matrix_batch(P[:, 0:3]) if R is None else np.asarray(R, np.float32)).astype(np.float64)
        f = P[:, 6].astype(np.float64)
        dqa = np.abs(G.astype(np.float64))                                    # |dq| = |g| (the y flip is a sign)
        with np.errstate(invalid="ignore", over="ignore"):
            w = np.abs(f)[:, None, None] * np.einsum("bic,bip->bcp", np.abs(Rm), dqa)   # >= |dv| and >= the fp32 dv's terms
        w = w.reshape(B, 3 * N)
        x = P[:, 7:].astype(np.float64)
        Sw = np.zeros((B, ns + ne))
        v = np.repeat(mu.astype(np.float64)[None], B, 0)
        for r0 in range(0, 3 * N, 8192):
            r1 = min(3 * N, r0 + 8192)
            for basis, k0, xs in ((pcs, 0, x[:, :ns]), (pce, ns, x[:, ns:])):
                if basis.shape[1] == 0:
                    continue
                a = basis[r0:r1].astype(np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    Sw[:, k0:k0 + basis.shape[1]] += (np.abs(a).T @ w[:, r0:r1].T).T
                v[:, r0:r1] += (a @ xs.T).T
        v = v.reshape(B, 3, N)
        q = np.einsum("bij,bjp->bip", Rm, v) * f[:, None, None] + P[:, 3:6].astype(np.float64)[:, :, None]
        q[:, 1] = (IM - q[:, 1]) - 1.0
        self.V = q                                                            # the exact forward output
        with np.errstate(invalid="ignore", over="ignore"):
            self.T = ((np.abs(mu.astype(np.float64))[None] * w).sum(1) + (np.abs(x) * Sw).sum(1)) / np.abs(f)
        self.Sw, self.dqa, self.f, self.t = Sw, dqa, f, P[:, 3:6].astype(np.float64)
        self.ns = ns

    def take(self, idx):
        return Ref(None, None, None, None, fields={k: (v[idx] if k != "ns" else v) for k, v in self.__dict__.items()})

    def e1(self, Vg):
        """sum_p sum_i |dq_i| E_q,i / |f|: how far the fp32 forward output the vertex_proj form starts from is from exact"""
        Vg = Vg.astype(np.float64)
        Eq = np.abs(Vg - self.V) + 2 * U * (np.abs(Vg) + np.abs(self.t)[:, :, None] + IM)
        with np.errstate(invalid="ignore", over="ignore"):
            return (self.dqa * Eq).sum(axis=(1, 2)) / np.abs(self.f)


# ---- launch geometry -> the longest rounding chain --------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _red_depth(nk):
    """longest rounding chain of bwd_reduce_kernel over nk partials (see the module docstring)"""
    per = _cdiv(nk, 16)
    chain = 0
    for w in range(16):
        m = max(0, min(nk, (w + 1) * per) - w * per)
        chain = max(chain, m // 8 + m % 8)
    return chain + 3 + 16


def _geom(rig, B):
    """the launcher's own geometry for a pass of min(B, 64) faces under the current knobs (fr_debug_decode_bwd_geom)"""
    out = (ctypes.c_int * 7)()
    _h().lib().fr_debug_decode_bwd_geom(B, rig.N, rig.ns, rig.ne, out)
    return dict(gpb=out[0], blocks=out[1], cb=out[2], waves=out[3], rpb=out[4], gemm=out[5], pre=out[6])


def _depths(kind, rig, B):
    g = _geom(rig, B)
    if kind == "ref":
        red_g, red_p = _red_depth(g["gemm"]), _red_depth(g["pre"])
        pose = 6 + red_p
        return dict(coef=1 + g["rpb"] + red_g, t3d=pose, f=3 + pose + 2)
    gpb, red = g["gpb"], _red_depth(g["blocks"])
    pose = 4 * gpb + 2 + red
    d = dict(coef=1 + 48 * gpb + red, t3d=pose, f=3 + pose + 2)
    if kind == "mu":   # (passes of B > 64 faces may take different CBs: the longest of their chains)
        lanes = max(4 * q["cb"] + 4 * q["waves"] for q in (_geom(rig, min(64, B - b0)) for b0 in range(0, B, 64)))
        d["f"] = 4 + 1 + 48 * gpb + lanes + 1 + red + 2
    return d


def _gamma(n):
    return 1.01 * n * U / (1.0 - n * U)


# ---- the checker -------------------------------------------------------------------------------------------------------------------
def _check(got, ref, D, kind, Vg=None, tag="", bar=True):
    """got [B, nd] (float64 of the fp32 result) against ref (a Ref of the same faces) under the depths D of the launch"""
    B, nd = got.shape
    want, S = ref.want, ref.S
    assert np.all(got[:, 0:3] == 0), tag                              # angles: no gradient (tf.py_func), exactly
    bound = np.zeros_like(want)
    bound[:, 3:6] = _gamma(D["t3d"]) * S[:, 3:6]
    if kind == "mu":
        bound[:, 6] = _gamma(D["f"]) * ref.T
    else:
        E1 = ref.e1(Vg)
        bound[:, 6] = E1 * 1.01 + _gamma(D["f"]) * (S[:, 6] + E1)
    bound[:, 7:] = _gamma(D["coef"] + 5) * ref.Sw
    # class of every output: NaN / +Inf / -Inf as the oracle's (the mu form of d f: non-finite as the oracle's -- its algebra
    # turns one infinite dq into infinities of both signs)
    cls = np.ones(nd, bool)
    if kind == "mu":
        cls[6] = False
        assert np.array_equal(~np.isfinite(got[:, 6]), ~np.isfinite(want[:, 6])), tag
    for fn in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(fn(got[:, cls]), fn(want[:, cls])), (tag, fn.__name__, np.argwhere(fn(got[:, cls]) != fn(want[:, cls]))[:4])
    fin = np.isfinite(want) & np.isfinite(got)
    fin[:, 0:3] = False
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - want), 0.0)
    ok = err <= np.where(fin, bound, np.inf)
    if not ok.all():
        b, k = np.argwhere(~ok)[0]
        raise AssertionError("%s: output [%d, %d] got %r want %r err %.3e bound %.3e (%d outside)" %
                             (tag, b, k, got[b, k], want[b, k], err[b, k], bound[b, k], int((~ok).sum())))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(fin & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    worst_face = 0.0
    if bar:
        blocks = [slice(3, 6), slice(6, 7), slice(7, 7 + ref.ns), slice(7 + ref.ns, nd)]
        for b in range(B):
            if not np.all(np.isfinite(want[b])):
                continue
            for sl in blocks:
                if sl.stop is not None and sl.start >= sl.stop:
                    continue
                scale = np.abs(want[b, sl]).max()
                if sl.start in (3, 6):
                    scale = max(scale, 1e-2 * S[b, sl].max())
                if scale == 0:
                    continue
                e = err[b, sl].max() / scale
                assert e < 2e-5, (tag, b, sl, e)
                worst_face = max(worst_face, e)
    s = STATS.setdefault(tag, [0.0, 0.0])
    s[0] = max(s[0], float(r.max()) if r.size else 0.0)
    s[1] = max(s[1], worst_face)
    return r


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(STATS):
        print("\n[bounds] %-34s max err/bound %.3e   max per-face err/scale %.3e" % (k, STATS[k][0], STATS[k][1]), end="")


# ---- the entry points ------------------------------------------------------------------------------------------------------------
class Rig:
    """one mesh / basis on the GPU: the C entry points by ctypes, the autograd surface through FaceRecNet"""

    def __init__(self, A):
        self.A = A
        self.net = net_mod().FaceRecNet(mesh_data=A, batch_size=1, im_size=IM)
        self.N, self.ns, self.ne = self.net.nvert, self.net.ndim_shape, self.net.ndim_exp
        self.packed_ok = _h().lib().fr_decode_backward_basis_bytes(self.N, self.ns, self.ne) > 0

    def kinds(self):
        return KINDS if self.packed_ok else ("ref",)

    def forward(self, P, R=None):
        p = torch.as_tensor(P, device=DEV)
        Rt = None if R is None else torch.as_tensor(R, device=DEV)
        with torch.no_grad():
            return self.net.vertices_transform(p, R=Rt).detach()

    def call(self, kind, P, G, V, R=None, ws=None):
        h = _h()
        L = h.lib()
        B = P.shape[0]
        p = torch.as_tensor(P, device=DEV)
        g = torch.as_tensor(G, device=DEV)
        Rt = None if R is None else torch.as_tensor(np.ascontiguousarray(R, np.float32).reshape(B, 3, 3), device=DEV)
        Rp = None if Rt is None else h.ptr(Rt)
        nws = L.fr_decode_backward_workspace_bytes(B, self.N, self.ns, self.ne)
        if ws is None:
            ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
        else:
            assert ws.dtype == torch.uint8 and ws.numel() == nws, (ws.numel(), nws)     # (exactly the stated bytes)
        gp = torch.full_like(p, 7.0)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        b = self.net._basis
        if kind == "mu":
            rc = L.fr_decode_3dmm_backward_packed_mu(h.ptr(g), h.ptr(p), h.ptr(self.net.mu), h.ptr(b.image_t()), Rp, B, self.N,
                                                     self.ns, self.ne, IM, h.ptr(gp), h.ptr(ws), nws, st)
        elif kind == "packed":
            rc = L.fr_decode_3dmm_backward_packed(h.ptr(g), h.ptr(p), h.ptr(V), h.ptr(b.image_t()), Rp, B, self.N, self.ns,
                                                  self.ne, IM, h.ptr(gp), h.ptr(ws), nws, st)
        else:
            rc = L.fr_decode_3dmm_backward(h.ptr(g), h.ptr(p), h.ptr(V), h.ptr(self.net.pc_shape), h.ptr(self.net.pc_exp), Rp,
                                           B, self.N, self.ns, self.ne, IM, h.ptr(gp), h.ptr(ws), nws, st)
        assert rc == 0, (kind, rc)
        torch.cuda.synchronize()
        return gp.cpu().numpy().astype(np.float64)

    def autograd(self, P, G, R=None, from_mu=False):
        basis = self.net._basis
        basis.backward_from_mu = from_mu
        try:
            p = torch.as_tensor(P, device=DEV).requires_grad_(True)
            Rt = None if R is None else torch.as_tensor(R, device=DEV)
            self.net.vertices_transform(p, R=Rt).backward(torch.as_tensor(G, device=DEV))
            torch.cuda.synchronize()
            return p.grad.cpu().numpy().astype(np.float64)
        finally:
            basis.backward_from_mu = False


def _cb(rig, B):
    """the CB the launcher picks for a pass of min(B, 64) faces under the current FR_BWD_CB (0 = by batch)"""
    return _geom(rig, B)["cb"]


def _eq_rows(a, b, tag, skip_f=False):
    keep = np.ones(a.shape[1], bool)
    if skip_f:
        keep[6] = False
    ab = a[:, keep].astype(np.float32).view(np.uint32)      # the fp32 results' bit patterns (-0 != +0)
    bb = b[:, keep].astype(np.float32).view(np.uint32)
    if not np.array_equal(ab, bb):
        bad = np.argwhere(ab != bb)
        raise AssertionError("%s: %d differing results, first at %s" % (tag, len(bad), bad[0]))


def _invariants(rig, P, G, V, tag):
    """a face's bits do not depend on the batch it sits in: the full (<= 64-face) batch vs a permutation vs subsets, for every
    entry point; the same call twice is bit-equal; packed and mu differ in d f only.  The mu form's d f adds the workgroup's
    per-wave partial dot products in an order that follows CB (fr_decode_bwd.hip), so it is compared between batches of the
    same CB class only."""
    B = P.shape[0]
    assert B == 64
    perm = np.random.RandomState(B).permutation(B)
    subsets = [np.arange(5, 22), np.arange(0, 1), np.arange(60, 64)]
    for kind in rig.kinds():
        full = rig.call(kind, P, G, V)
        _eq_rows(full, rig.call(kind, P, G, V), "%s %s: the same call twice" % (tag, kind))
        pg = rig.call(kind, P[perm], G[perm], V[perm])
        _eq_rows(pg, full[perm], "%s %s: permuted batch" % (tag, kind))
        for idx in subsets:
            sub = rig.call(kind, P[idx], G[idx], V[idx])
            _eq_rows(sub, full[idx], "%s %s: faces %d..%d alone" % (tag, kind, idx[0], idx[-1]),
                     skip_f=kind == "mu" and _cb(rig, len(idx)) != _cb(rig, B))
        if kind == "packed" and "mu" in rig.kinds():
            _eq_rows(rig.call("mu", P, G, V), full, "%s: packed vs mu outside d f" % tag, skip_f=True)
    # with CB pinned, every output -- the mu form's d f included -- is the same across batch sizes, positions and orders
    if "mu" in rig.kinds():
        for cb in (2, 4):
            with _h().options(FR_BWD_CB=cb):
                assert _cb(rig, 1) == _cb(rig, B) == cb
                full = rig.call("mu", P, G, V)
                _eq_rows(rig.call("mu", P[perm], G[perm], V[perm]), full[perm], "%s mu CB=%d: permuted batch" % (tag, cb))
                for idx in subsets:
                    _eq_rows(rig.call("mu", P[idx], G[idx], V[idx]), full[idx],
                             "%s mu CB=%d: faces %d..%d alone" % (tag, cb, idx[0], idx[-1]))


def _b0_split(rig, P, G, V, ref, tag):
    """B > 64: the launcher runs 64-face chunks (b0) and picks CB again per chunk; every face's bits are those of the same face
    launched in a batch of its own chunk's size class, and the whole is within the bound"""
    B = P.shape[0]
    assert B > 64
    for kind in rig.kinds():
        got = rig.call(kind, P, G, V)
        _check(got, ref, _depths(kind, rig, B), kind, Vg=V.cpu().numpy(), tag="%s B=%d|%s" % (tag, B, kind))
        for lo in range(64, B, 64):
            idx = np.arange(lo, min(B, lo + 64))
            alone = rig.call(kind, P[idx], G[idx], V[idx])
            _eq_rows(alone, got[idx], "%s %s: faces %d.. of B=%d alone" % (tag, kind, lo, B))
        head = rig.call(kind, P[:64], G[:64], V[:64])
        _eq_rows(head, got[:64], "%s %s: first 64 of B=%d alone" % (tag, kind, B))


# ---- 1. the product shape --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_case(oracle, full_assets):
    rig = Rig(full_assets)
    rs = np.random.RandomState(20261016)
    P, G = _inputs(rs, 70, rig.N, rig.ns, rig.ne)
    V = rig.forward(P)
    return rig, P, G, V, Ref(oracle, full_assets, P, G)


@pytest.mark.parametrize("B", [1, 16, 32, 48, 64, 70])
def test_product_shape_every_entry_point_within_the_bound(full_case, B):
    """N = 53,215 at the default 256 chunks: 13 vertex groups per workgroup, the last workgroup 11, the last group 15 vertices
    (clamped tile origin).  B = 1 / 16 / 32 / 48 / 64 / 70 take NB = 1..4, both CBs of the by-batch rule and one b0 split."""
    rig, P, G, V, ref = full_case
    Vs = V[:B]
    Vn = Vs.cpu().numpy()
    outs = {}
    for kind in rig.kinds():
        outs[kind] = rig.call(kind, P[:B], G[:B], Vs)
        _check(outs[kind], ref.take(slice(0, B)), _depths(kind, rig, B), kind, Vg=Vn, tag="full-size B=%d|%s" % (B, kind))
    if B in (1, 70):
        _eq_rows(rig.autograd(P[:B], G[:B]), outs["packed"], "autograd = packed entry point")
        _eq_rows(rig.autograd(P[:B], G[:B], from_mu=True), outs["mu"], "autograd (backward_from_mu) = mu entry point")


def test_product_shape_invariants(full_case):
    rig, P, G, V, ref = full_case
    full70 = {k: rig.call(k, P, G, V) for k in rig.kinds()}
    for B in (1, 16, 32, 48, 64):
        for kind in rig.kinds():
            got = rig.call(kind, P[:B], G[:B], V[:B])
            _eq_rows(got, full70[kind][:B], "full-size %s: first %d faces vs the 70-face run" % (kind, B),
                     skip_f=kind == "mu" and _cb(rig, B) != _cb(rig, 70))
    _invariants(rig, P[:64], G[:64], V[:64], "full-size")
    _b0_split(rig, P, G, V, ref, "full-size")


# ---- 2. several groups per workgroup: FR_BWD_CHUNKS x FR_BWD_CB ------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid_case(oracle, synth):
    A = synth.make_assets(70, 61, 199, 29, patch=None, seed_basis=4270)
    rig = Rig(A)
    rs = np.random.RandomState(4270)
    P, G = _inputs(rs, 130, rig.N, rig.ns, rig.ne)
    V = rig.forward(P)
    return rig, P, G, V, Ref(oracle, A, P, G)


@pytest.mark.parametrize("chunks", [1, 3, 7, 256, 511, 512])
def test_chunks_and_cb_sweep(mid_case, chunks):
    rig, P, G, V, ref = mid_case
    h = _h()
    Vn = V.cpu().numpy()
    for B in (5, 33, 64):
        byc = {}
        for cb in (0, 2, 4):
            with h.options(FR_BWD_CHUNKS=chunks, FR_BWD_CB=cb):
                for kind in ("packed", "mu"):
                    got = rig.call(kind, P[:B], G[:B], V[:B])
                    _check(got, ref.take(slice(0, B)), _depths(kind, rig, B), kind, Vg=Vn[:B],
                           tag="mid chunks=%d B=%d|%s" % (chunks, B, kind), bar=chunks == 256)
                    byc[(kind, cb)] = got
        # for a fixed chunking CB changes no bit (the mu form's d f: see _invariants)
        for kind in ("packed", "mu"):
            for cb in (2, 4):
                _eq_rows(byc[(kind, cb)], byc[(kind, 0)], "mid chunks=%d B=%d %s: CB %d vs by-batch" % (chunks, B, kind, cb),
                         skip_f=kind == "mu" and cb != _cb(rig, B))
    if chunks == 256:
        for B in (5, 33, 64):
            got = rig.call("ref", P[:B], G[:B], V[:B])
            _check(got, ref.take(slice(0, B)), _depths("ref", rig, B), "ref", Vg=Vn[:B], tag="mid B=%d|ref" % B)


def test_mid_mesh_invariants_and_b0_chunks(mid_case):
    rig, P, G, V, ref = mid_case
    _invariants(rig, P[:64], G[:64], V[:64], "mid")
    _b0_split(rig, P, G, V, ref, "mid")
    _b0_split(rig, P[:70], G[:70], V[:70], ref.take(slice(0, 70)), "mid")


# ---- 4. R_override ---------------------------------------------------------------------------------------------------------------
def test_r_override(oracle, mid_case):
    """a host-supplied R that is NOT the rotation of the angles (the reference forms R on the host, tf.py_func), through
    vertices_transform(p, R=R) and through the C entry points, held to the oracle with that R; and R = the angles' own rotation,
    within the bound of the in-kernel-R gradient"""
    rig, P0, G0, _, _ = mid_case
    rs = np.random.RandomState(9)
    B = 37
    P, G = _inputs(rs, B, rig.N, rig.ns, rig.ne)
    R = _rotations(rs, B)
    ref = Ref(oracle, rig.A, P, G, R=R)
    V = rig.forward(P, R=R)
    Vn = V.cpu().numpy()
    for kind in rig.kinds():
        got = rig.call(kind, P, G, V, R=R)
        _check(got, ref, _depths(kind, rig, B), kind, Vg=Vn, tag="R_override|%s" % kind)
        if kind != "ref":
            _eq_rows(rig.autograd(P, G, R=R, from_mu=kind == "mu"), got, "autograd with R = %s entry point" % kind)
    Ra = oracle.rotation_matrix_batch(P[:, 0:3])
    ref0 = Ref(oracle, rig.A, P, G)
    Va = rig.forward(P, R=Ra)
    for kind in rig.kinds():
        got = rig.call(kind, P, G, Va, R=Ra)
        _check(got, ref0, _depths(kind, rig, B), kind, Vg=Va.cpu().numpy(), tag="R = own rotation|%s" % kind)


# ---- 5. shape edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gu,gv,ns,ne", [(11, 17, 0, 29), (11, 17, 199, 0), (11, 17, 240, 16), (11, 17, 241, 16),
                                         (4, 4, 199, 29), (17, 1, 199, 29), (31, 1, 199, 29), (3, 11, 199, 29)])
def test_shape_edges(oracle, synth, gu, gv, ns, ne):
    """no shape basis; no expression basis; exactly 16 coefficient blocks (the largest the packed path serves); 17 blocks (the
    reference-layout fallback, also through autograd); N = 16 / 17 / 31 / 33 (one whole group; one vertex past it; a clamped
    second group; three groups, the last with one vertex)"""
    A = synth.make_assets(gu, gv, ns, ne, patch=None, seed_basis=gu * gv + ns + ne)
    rig = Rig(A)
    N = gu * gv
    blocks = _cdiv(ns, 16) + _cdiv(ne, 16)
    L = _h().lib()
    assert (L.fr_decode_backward_basis_bytes(N, ns, ne) == 0) == (blocks > 16)
    assert rig.packed_ok == (blocks <= 16)
    rs = np.random.RandomState(N + ns)
    for B in (5, 37):
        P, G = _inputs(rs, B, N, ns, ne)
        ref = Ref(oracle, A, P, G)
        V = rig.forward(P)
        Vn = V.cpu().numpy()
        outs = {}
        for kind in rig.kinds():
            outs[kind] = rig.call(kind, P, G, V)
            _check(outs[kind], ref, _depths(kind, rig, B), kind, Vg=Vn, tag="edges|%s" % kind)
        ag = rig.autograd(P, G)
        _eq_rows(ag, outs["packed" if rig.packed_ok else "ref"], "autograd = %s" % ("packed" if rig.packed_ok else "ref"))
        if not rig.packed_ok:
            _eq_rows(rig.autograd(P, G, from_mu=True), outs["ref"], "autograd (backward_from_mu) falls back to ref")


# ---- 6. zero and non-finite faces ------------------------------------------------------------------------------------------------
def test_zero_nan_inf_faces_stay_in_their_rows(oracle, mid_case):
    rig, P0, G0, V0, _ = mid_case
    B = 40
    P, G = P0[:B].copy(), G0[:B].copy()
    zero, nanf, inff = 3, 17, 29
    G[zero] = 0.0
    G[nanf, 1, 1234] = np.nan
    # +Inf on the x row of the vertex farthest from t in x: (q - t)_x has the sign of (R v)_x there, in fp32 and in float64
    Vn = V0[:B].cpu().numpy()
    p_inf = int(np.argmax(np.abs(Vn[inff, 0] - P[inff, 3])))
    G[inff, 0, p_inf] = np.inf
    ref = Ref(oracle, rig.A, P, G)
    assert np.isnan(ref.want[nanf, 7:]).all() and np.isinf(ref.want[inff, 3])
    rest = np.array([b for b in range(B) if b not in (zero, nanf, inff)])
    assert _cb(rig, B) == _cb(rig, len(rest))
    for kind in rig.kinds():
        got = rig.call(kind, P, G, V0[:B])
        assert np.all(got[zero] == 0), kind                                 # an all-zero gradient: an exactly zero row (d f too)
        _check(got, ref, _depths(kind, rig, B), kind, Vg=Vn, tag="zero/NaN/Inf|%s" % kind)
        alone = rig.call(kind, P[rest], G[rest], V0[:B][rest])
        _eq_rows(got[rest], alone, "%s: the other faces, with vs without the zero / NaN / Inf faces" % kind)
        assert np.all(np.isfinite(got[rest]))
