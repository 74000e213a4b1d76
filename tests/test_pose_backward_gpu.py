"""GPU: the pose gradients (fr_decode_pose_backward, fr_decode_render_backward_pose and their autograd surface) held to the float64
reference of tests/ref_pose_backward.py by a PROVEN bound, plus the bit-level invariants their fixed summation order promises.

The bound (ref_pose_backward.PoseRef.bound; the construction of tests/test_decode_backward_bounds_gpu.py).  The kernel's pose
moment A[i][k] = sum_p dq_i (q_k - t_k) starts from the fp32 forward output, whose distance from the exact projection is measured
(E_q), not assumed; each term has 3 roundings; the longest chain of rounded fp32 additions is the fourth value of
fr_debug_pose_bwd_geom, the fp32 output adds one; the error is carried through |cof(R)| / |det(R)| to grad_R and through
|dR / d angle| to the angle columns, with a factor 1.01 for the second-order terms.  Nothing is fitted.
The discrimination cap -- for every face of every case the bound is below 1e-3 of the face's max |G_ij| -- is a condition on the
inputs and is checked on the CPU, with the reference alone (tests/test_pose_backward_cpu.py); the cases are
ref_pose_backward.case_list: N in {1, 7, 15, 16, 17, 4270, chunk + 1, chunk - 1}, B in {1, 17, 64, 65}, the in-kernel rotation,
random rotations, a mildly non-orthogonal and a singular override, a face with f = 0."""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import net_mod
import ref_pose_backward as RP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IM = 200.0
ND = 7 + RP.NS + RP.NE


def _h():
    return pkg("_lib")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


def _geom(N):
    out = (ctypes.c_int * 4)()
    _h().lib().fr_debug_pose_bwd_geom(1, N, out)
    return list(out)


def pose_c(G, V, P, R=None, ns=RP.NS, ne=RP.NE, im=IM, want_gp=True, want_R=True, fill=7.0, ws=None):
    """fr_decode_pose_backward on torch's current stream -> (grad_params pre-filled with `fill`, grad_R), not synchronised"""
    h, L = _h(), _h().lib()
    B, N = int(P.shape[0]), int(G.shape[2])
    nws = L.fr_decode_pose_backward_workspace_bytes(B, N)
    if ws is None:
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
    else:
        assert ws.dtype == torch.uint8 and ws.numel() == nws, (ws.numel(), nws)     # (exactly the stated bytes)
    gp = torch.full((B, 7 + ns + ne), fill, dtype=torch.float32, device=DEV) if want_gp else None
    gR = torch.full((B, 3, 3), fill, dtype=torch.float32, device=DEV) if want_R else None
    rc = L.fr_decode_pose_backward(h.ptr(G), h.ptr(V), h.ptr(P), h.ptr(R), B, N, ns, ne, im, h.ptr(gp), h.ptr(gR), h.ptr(ws), nws,
                                   _stream())
    assert rc == 0, rc
    return gp, gR


# ---- the C-level cases: inputs and float64 references, built once ------------------------------------------------------------------
_CASES = {}


def _case(oracle, name):
    if name not in _CASES:
        chunk, _, _, depth = _geom(4270)
        row = [c for c in RP.case_list(chunk) if c[0] == name][0]
        _, seed, B, N, mode, f0 = row
        c = RP.make_case(seed, B, N, mode, f0)
        ref = RP.PoseRef(oracle, c["G"], c["v"], c["P"], R=c["R"])
        bG, bang = ref.bound(c["Vg"], depth)
        dev = dict(G=_t(c["G"]), V=_t(c["Vg"]), P=_t(c["P"]), R=None if c["R"] is None else _t(c["R"]))
        _CASES[name] = (c, ref, bG, bang, dev)
    return _CASES[name]


CASE_NAMES = [c[0] for c in RP.case_list(2048)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_proven_bound_and_bit_invariants(oracle, name):
    c, ref, bG, bang, d = _case(oracle, name)
    B = c["P"].shape[0]
    gp, gR = pose_c(d["G"], d["V"], d["P"], d["R"])
    gp2, gR2 = pose_c(d["G"], d["V"], d["P"], d["R"])
    torch.cuda.synchronize()
    assert _same(gp, gp2) and _same(gR, gR2)                                   # two runs: the same bits
    assert bool((gp[:, 3:] == 7.0).all())                                      # columns 3.. of a pre-filled grad_params: untouched
    got_R, got_a = gR.cpu().numpy().astype(np.float64), gp[:, 0:3].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got_R)) and np.all(np.isfinite(got_a))
    errR, erra = np.abs(got_R - ref.grad_R), np.abs(got_a - ref.angles)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("%s: worst err / bound grad_R %.3f angles %.3f; worst bound / max|G| %.2e" %
              (name, np.nanmax(np.where(bG > 0, errR / bG, 0.0)), np.nanmax(np.where(bang > 0, erra / bang, 0.0)),
               np.nanmax(np.where(np.abs(ref.grad_R).max(axis=(1, 2)) > 0,
                                  bG.max(axis=(1, 2)) / np.abs(ref.grad_R).max(axis=(1, 2)), 0.0))))
    assert np.all(errR <= bG), (name, np.argwhere(errR > bG)[:4], errR.max())
    if c["R"] is None:
        assert np.all(erra <= bang), (name, np.argwhere(erra > bang)[:4])
    else:
        assert np.all(got_a == 0)                                              # R_override: the angles did not enter the forward
    if ref.singular.any():                                                     # det(R) == 0: DEFINED as zeros
        assert np.all(got_R[ref.singular] == 0) and np.abs(got_R[~ref.singular]).max() > 0
    # one output alone gives the same bits as both
    gp3, _ = pose_c(d["G"], d["V"], d["P"], d["R"], want_R=False)
    _, gR3 = pose_c(d["G"], d["V"], d["P"], d["R"], want_gp=False)
    torch.cuda.synchronize()
    assert _same(gp3, gp) and _same(gR3, gR)
    # a face computed alone equals the same face inside the batch
    for b in sorted({0, B // 2, B - 1}):
        Rb = None if d["R"] is None else d["R"][b:b + 1].contiguous()
        gp1, gR1 = pose_c(d["G"][b:b + 1].contiguous(), d["V"][b:b + 1].contiguous(), d["P"][b:b + 1].contiguous(), Rb)
        torch.cuda.synchronize()
        assert _same(gp1, gp[b:b + 1]) and _same(gR1, gR[b:b + 1]), (name, b)


# ---- the z-only route on a rendered small scene --------------------------------------------------------------------------------------
class Scene:
    """the 70 x 61 mesh (N = 4,270) rendered at 40 x 40: the planes, the kept hand-off, pixel gradients; the raw C calls of the routes"""

    def __init__(self, A, B=3, S=40, seed=3):
        h, L = _h(), _h().lib()
        self.A, self.B, self.S = A, B, S
        self.net = n = net_mod().FaceRecNet(mesh_data=A, batch_size=B, im_size=S)
        self.N, self.ns, self.ne, self.ntri = n.nvert, n.ndim_shape, n.ndim_exp, int(n.tri.shape[1])
        rs = np.random.RandomState(seed)
        P = np.zeros((B, n.ndim), np.float32)
        P[:, 0:3] = rs.uniform(-0.5, 0.5, (B, 3))
        P[:, 3:5] = rs.uniform(17, 23, (B, 2))
        P[:, 6] = rs.uniform(1.6e-4, 2.2e-4, B)
        P[:, 7:7 + self.ns] = rs.uniform(0, 1e4, (B, self.ns))
        P[:, 7 + self.ns:] = rs.uniform(-1.5, 1.5, (B, self.ne))
        self.Pn, self.P = P, _t(P)
        self.Rn = n.rotation_matrix_batch(P[:, 0:3] * 0.5)          # a caller-computed rotation: not that of the face's angles
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.im = torch.rand((B, S, S, 1), generator=g).to(DEV)
        self.gi = torch.rand((B, S, S, 1), generator=g).to(DEV)
        self.gn = torch.rand((B, S, S, 7), generator=g).to(DEV)
        self.image_t = n._basis.image_t()
        self.pitch = L.fr_decode_render_vertex_pitch(self.N)
        assert self.N == 4270 and self.pitch == 4288

    def forward(self, R=None):
        """-> (depth, tri_ind, hand-off as a [B,3,pitch] float tensor)"""
        h, L, n = _h(), _h().lib(), self.net
        B, S = self.B, self.S
        nws = L.fr_render_depth_workspace_bytes(B, self.N, self.ntri, S, S)
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
        nh = L.fr_decode_render_vertex_bytes(B, self.N)
        hand = torch.zeros((B, 3, self.pitch), dtype=torch.float32, device=DEV)
        assert nh == hand.numel() * 4
        o = dict(dtype=torch.float32, device=DEV)
        outs = (torch.empty((B, S, S, 7), **o), torch.empty((B, S, S, 1), **o), torch.empty((B, S, S, 1), **o),
                torch.empty((B, S, S, 1), **o))
        rc = L.fr_decode_rendering_layer_forward(h.ptr(self.P), h.ptr(n._basis.image), h.ptr(R), h.ptr(n.tri), h.ptr(n.vertex_code),
                                                 h.ptr(self.im), B, self.N, self.ns, self.ne, self.ntri, S, S, 1, float(S),
                                                 h.ptr(hand), nh, *[h.ptr(t) for t in outs], h.ptr(ws), nws, _stream(), 15)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert float((outs[3] >= 0).float().mean()) > 0.05
        return outs[2], outs[3], hand

    def bwd(self, depth, tri_ind, hand, R=None, pose=True, ws=None):
        h, L, n = _h(), _h().lib(), self.net
        B, S = self.B, self.S
        gp = torch.full((B, n.ndim), 7.0, dtype=torch.float32, device=DEV)
        common = (None, h.ptr(self.gi), h.ptr(self.gn), h.ptr(self.im), h.ptr(depth), h.ptr(n.tri), h.ptr(tri_ind), h.ptr(self.P),
                  h.ptr(n.mu), h.ptr(self.image_t), h.ptr(R), B, self.N, self.ns, self.ne, self.ntri, S, S, float(S), h.ptr(gp))
        if not pose:
            nws = L.fr_decode_render_backward_workspace_bytes(B, self.N, self.ns, self.ne, S, S)
            ws = torch.empty((nws,), dtype=torch.uint8, device=DEV) if ws is None else ws
            assert ws.numel() == nws
            assert L.fr_decode_render_backward(*common, h.ptr(ws), nws, _stream()) == 0
            torch.cuda.synchronize()
            return gp, None
        nws = L.fr_decode_render_backward_pose_workspace_bytes(B, self.N, self.ns, self.ne, S, S)
        ws = torch.empty((nws,), dtype=torch.uint8, device=DEV) if ws is None else ws
        assert ws.numel() == nws
        gR = torch.full((B, 3, 3), 7.0, dtype=torch.float32, device=DEV)
        assert L.fr_decode_render_backward_pose(*common, h.ptr(ws), nws, _stream(), h.ptr(hand), hand.numel() * 4, h.ptr(gR)) == 0
        torch.cuda.synchronize()
        return gp, gR

    def vertex_grad(self, depth, tri_ind):
        """the dense [B,3,N] vertex gradient (0, 0, z) of the composed chain: the torch pixel gradient -> fr_render_depth_backward_ws"""
        h, L, n = _h(), _h().lib(), self.net
        B, S = self.B, self.S
        dg = (self.gn[..., 0:1] * self.im * ((depth >= 1e-6) & (depth <= 1.0)).to(depth.dtype) +
              self.gi * (depth >= 1e-6).to(depth.dtype)).contiguous()
        dg = torch.zeros_like(depth) + dg
        vg = torch.full((B, 3, self.N), 7.0, dtype=torch.float32, device=DEV)
        nrw = L.fr_render_depth_backward_workspace_bytes(B, S, S)
        rws = torch.empty((nrw,), dtype=torch.uint8, device=DEV)
        assert L.fr_render_depth_backward_ws(h.ptr(dg), h.ptr(n.tri), h.ptr(tri_ind), h.ptr(vg), B, self.N, self.ntri, S, S,
                                             h.ptr(rws), nrw, _stream()) == 0
        torch.cuda.synchronize()
        assert bool((vg[:, 0:2] == 0).all()) and float(vg[:, 2].abs().max()) > 0
        return vg


@pytest.fixture(scope="module")
def scene(synth):
    # the 70 x 61 mesh (N = 4,270: three chunks, the last one ragged; pitch 4,288) with a 20 + 5 basis
    return Scene(synth.make_assets(70, 61, RP.NS, RP.NE, patch=None, seed_basis=4270))


@pytest.mark.parametrize("override", [False, True])
def test_z_only_route_equals_the_dense_route_and_the_render_backward(oracle, scene, override):
    sc = scene
    R = _t(sc.Rn) if override else None
    depth, tri_ind, hand = sc.forward(R)
    gp0, _ = sc.bwd(depth, tri_ind, hand, R, pose=False)
    gp, gR = sc.bwd(depth, tri_ind, hand, R, pose=True)
    gpb, gRb = sc.bwd(depth, tri_ind, hand, R, pose=True)
    assert _same(gp, gpb) and _same(gR, gRb)
    assert _same(gp[:, 3:], gp0[:, 3:]) and bool((gp0[:, 0:3] == 0).all())      # columns 3..: fr_decode_render_backward's bits
    # the dense route fed (0, 0, z) and the dense forward output (a copy of the hand-off's live columns)
    vg = sc.vertex_grad(depth, tri_ind)
    V = hand[:, :, :sc.N].contiguous()
    gpd, gRd = pose_c(vg, V, sc.P, R, ns=sc.ns, ne=sc.ne, im=float(sc.S))
    torch.cuda.synchronize()
    assert _same(gRd, gR) and _same(gpd[:, 0:3], gp[:, 0:3])
    if override:
        assert bool((gp[:, 0:3] == 0).all())
    else:
        assert float(gp[:, 0:3].abs().min()) > 0
    # ... and both against float64, from the model's own un-projected vertices
    ref = RP.PoseRef(oracle, vg.cpu().numpy(), RP.unprojected_f64(sc.A, sc.Pn), sc.Pn, R=sc.Rn if override else None,
                     im_size=float(sc.S))
    bG, bang = ref.bound(V.cpu().numpy(), _geom(sc.N)[3])
    errR = np.abs(gR.cpu().numpy().astype(np.float64) - ref.grad_R)
    erra = np.abs(gp[:, 0:3].cpu().numpy().astype(np.float64) - ref.angles)
    gmax = np.abs(ref.grad_R).max(axis=(1, 2), keepdims=True)
    print("z-only (override=%s): worst err / bound %.3f, worst err / max|G| %.2e, bound / max|G| %.2e" %
          (override, (errR / np.where(bG > 0, bG, 1)).max(), (errR / gmax).max(), (bG / gmax).max()))
    assert np.all(errR <= bG) and np.all(erra <= bang)
    assert np.all(gmax > 0) and np.all(errR <= 1e-3 * gmax)                     # (a sign or a transposition could not hide here)
    assert np.all(gR.cpu().numpy()[:, 0:2] == 0)                                # rows 0 and 1 of G: no x / y gradient exists


# ---- autograd --------------------------------------------------------------------------------------------------------------------------
def test_vertices_transform_pose_grad(scene):
    sc, net = scene, scene.net
    g = torch.Generator(device="cpu").manual_seed(11)
    w = torch.randn((sc.B, 3, sc.N), generator=g).to(DEV)

    def run(pose_grad, R=None):
        p = sc.P.clone().requires_grad_(True)
        V = net.vertices_transform(p, R=R, pose_grad=pose_grad) if pose_grad is not None else net.vertices_transform(p, R=R)
        (V * w).sum().backward()
        return p.grad, V.detach()
    g0, V0 = run(None)
    assert bool((g0[:, 0:3] == 0).all())                                        # the default: the angles get 0, exactly as before
    gF, _ = run(False)
    assert _same(gF, g0)
    g1, V1 = run(True)
    gpc, _ = pose_c(w, V0, sc.P, None, ns=sc.ns, ne=sc.ne, im=float(sc.S))
    torch.cuda.synchronize()
    assert _same(V1, V0) and _same(g1[:, 3:], g0[:, 3:]) and _same(g1[:, 0:3], gpc[:, 0:3])
    assert float(g1[:, 0:3].abs().min()) > 0
    # the memory-saving form is forced off for such a call, and only for it
    net._basis.backward_from_mu = True
    try:
        g2, _ = run(True)
        assert _same(g2[:, 0:3], g1[:, 0:3])
    finally:
        net._basis.backward_from_mu = False
    # a caller-computed R: a leaf that requires grad receives dL/dR, the angle columns stay 0
    R = _t(sc.Rn).requires_grad_(True)
    gR_, VR = run(True, R)
    _, gRc = pose_c(w, VR, sc.P, R.detach(), ns=sc.ns, ne=sc.ne, im=float(sc.S))
    torch.cuda.synchronize()
    assert R.grad is not None and _same(R.grad, gRc) and bool((gR_[:, 0:3] == 0).all())
    R2 = _t(sc.Rn).requires_grad_(True)
    gd, _ = run(None, R2)
    assert R2.grad is None and _same(gd[:, 3:], gR_[:, 3:])                     # the default: R gets no gradient, as before


def test_decode_rendering_layer_pose_grad_fused_and_two_step(scene):
    sc, net = scene, scene.net
    gw = sc.gn

    def run(route, pose_grad, R=None):
        p = sc.P.clone().requires_grad_(True)
        kw = {} if pose_grad is None else dict(pose_grad=pose_grad)
        if route == "fused":
            ni, di = net.decode_rendering_layer(p, im_gray=sc.im, R=R, **kw)
            assert type(ni.grad_fn).__name__.startswith("_DecodeRenderingLayer")
        elif route == "fallback":     # the fused node refuses: decode_rendering_layer IS the two-step route and passes the flag on
            o = net_mod()._ops()
            real = o.decode_rendering_layer

            def refuse(*a, **k):
                raise NotImplementedError("test")
            o.decode_rendering_layer = refuse
            try:
                ni, di = net.decode_rendering_layer(p, im_gray=sc.im, R=R, **kw)
            finally:
                o.decode_rendering_layer = real
            assert not type(ni.grad_fn).__name__.startswith("_DecodeRenderingLayer")
        else:
            ni, di = net.coarse_net_input(net.vertices_transform(p, R=R, **kw), im_gray=sc.im)
        ((ni * gw).sum() + (di * sc.gi).sum()).backward()
        return p.grad
    depth, tri_ind, hand = sc.forward(None)
    gpc, gRc = sc.bwd(depth, tri_ind, hand, None, pose=True)
    g0 = run("fused", None)
    assert bool((g0[:, 0:3] == 0).all())                                        # default: as today
    g1 = run("fused", True)
    assert _same(g1, gpc) and _same(g1[:, 3:], g0[:, 3:]) and float(g1[:, 0:3].abs().min()) > 0
    g2 = run("two", True)
    g3 = run("fallback", True)
    assert _same(g2[:, 0:3], g1[:, 0:3]) and _same(g3, g2)
    assert bool((run("fallback", None)[:, 0:3] == 0).all())
    # R as a leaf: R.grad is the C call's grad_R on every route; by default it is None
    depthR, tri_indR, handR = sc.forward(_t(sc.Rn))
    gpR, gRR = sc.bwd(depthR, tri_indR, handR, _t(sc.Rn), pose=True)
    for route in ("fused", "two"):
        R = _t(sc.Rn).requires_grad_(True)
        gp_ = run(route, True, R)
        assert R.grad is not None and _same(R.grad, gRR) and bool((gp_[:, 0:3] == 0).all()), route
    R = _t(sc.Rn).requires_grad_(True)
    gp_ = run("fused", None, R)
    assert R.grad is None and _same(gp_, sc.bwd(depthR, tri_indR, handR, _t(sc.Rn), pose=False)[0])


@pytest.mark.parametrize("fused_step", [False, True])
def test_coarse_net_pose_grad_reaches_earlier_iterations(small_assets, fused_step):
    netm, cn = pkg("nets.network"), pkg("nets.coarse_net")
    S, B = 40, 2
    face = netm.FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S)
    face.init_pred_params[..., 6] = 2e-4
    torch.manual_seed(1)
    im = torch.rand((B, S, S, 1), device=DEV)
    grads = []
    for pose_grad in (False, True):
        torch.manual_seed(0)
        model = cn.CoarseNet(face, nIter=2, fused_step=fused_step, pose_grad=pose_grad).cuda()
        params = model(im)
        model.depth(im, params).mean().backward()
        fc = model.iters[-1].fc
        assert bool(torch.isfinite(fc.weight.grad).all())
        grads.append(fc.weight.grad.clone())
    # the depth map's gradient now reaches the rows of the last layer that predict the three angles; the other rows are the same
    # quantity (to rounding, not bit for bit: the two models' convolutions may run under different MIOpen algorithms)
    assert bool((grads[0][0:3] == 0).all()) and float(grads[1][0:3].abs().max()) > 0
    assert torch.allclose(grads[0][3:], grads[1][3:], rtol=1e-3, atol=1e-3 * float(grads[0][3:].abs().max()))


# ---- threads -----------------------------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams(oracle):
    jobs = [_case(oracle, "above")[4], _case(oracle, "below")[4]]

    def run(d, stream):
        with torch.cuda.stream(stream):
            outs = [pose_c(d["G"], d["V"], d["P"], d["R"]) for _ in range(3)]
            stream.synchronize()
        return outs
    want = [run(d, torch.cuda.current_stream()) for d in jobs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in jobs]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    barrier = threading.Barrier(2)

    def go(i):
        barrier.wait(timeout=60)
        return run(jobs[i], streams[i])
    ex = ThreadPoolExecutor(max_workers=2)
    try:
        futs = [ex.submit(go, i) for i in range(2)]
        got = [f.result(timeout=120) for f in futs]
    finally:
        ex.shutdown(wait=False, cancel_futures=True)
    torch.cuda.synchronize()
    for i in range(2):
        for (a, b), (c, d) in zip(got[i], want[i]):
            assert _same(a, c) and _same(b, d)
