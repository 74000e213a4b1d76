"""GPU: fr_depth_normals_forward / _backward (depth_normals_forward_kernel, depth_normals_backward_kernel) held to their float64
model (tests/ref_depth_normals.py, pinned on the CPU by tests/test_depth_normals_cpu.py), the operator ops.depth_normals, and the
opt-in sfs_fine flag of the objective.

forward:   |normal - n_m| <= 2^-24 |n_m| + 2^-40          (one fp32 rounding + the float64 error on components of magnitude <= 1; the
           device's float64 divide and square root are not assumed to round as the host's: a bound, not a bit compare)
backward:  |grad_depth - G_m| <= 2^-24 |G_m| + 2^-40 A(p)  (A = the sum of the absolute values of the six terms of the gather)
Invalid pixels are exactly +0 in both.  Outputs are pre-filled with NaN.  Every figure is printed before it is asserted."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import ref_depth_normals as RD
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E40, E24 = 2.0 ** -40, 2.0 ** -24


def _h():
    return pkg("_lib")


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.int32)


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def fwd(depth, mask):
    """fr_depth_normals_forward on torch's current stream (not synchronised) -> normal [B,H,W,3] pre-filled with NaN"""
    h, L = _h(), _h().lib()
    B, H, W = tuple(depth.shape[:3])
    out = torch.full((B, H, W, 3), float("nan"), device=DEV)
    rc = L.fr_depth_normals_forward(h.ptr(depth), h.ptr(mask), B, H, W, h.ptr(out), _sp())
    assert rc == 0, rc
    return out


def bwd(g, depth, mask):
    """fr_depth_normals_backward -> grad_depth [B,H,W,1] pre-filled with NaN"""
    h, L = _h(), _h().lib()
    B, H, W = tuple(depth.shape[:3])
    out = torch.full((B, H, W, 1), float("nan"), device=DEV)
    rc = L.fr_depth_normals_backward(h.ptr(g), h.ptr(depth), h.ptr(mask), B, H, W, h.ptr(out), _sp())
    assert rc == 0, rc
    return out


class Run:
    """one case: inputs, the model (computed once, never changed), and one forward + backward of the product"""

    def __init__(self, case):
        self.case = case
        self.d = RD.inputs(case)
        self.m = RD.forward(self.d["depth"], self.d["mask"])
        self.G, self.A = RD.backward(self.d["grad_normal"], self.d["depth"], self.d["mask"], m=self.m)
        self.z, self.mask, self.g = _t(self.d["depth"]), _t(self.d["mask"]), _t(self.d["grad_normal"])
        self.n = fwd(self.z, self.mask)
        self.gd = bwd(self.g, self.z, self.mask)
        torch.cuda.synchronize()


_RUNS = {}


def _run(case):
    if case not in _RUNS:
        _RUNS[case] = Run(case)
    return _RUNS[case]


@pytest.fixture(params=RD.cases(), ids=RD.case_id)
def run(request):
    return _run(request.param)


def _dense():
    return _run(RD.Case(1, 33, 67, ("valid",)))


# ---- 1. forward against the model -------------------------------------------------------------------------------------------------
def test_forward_vs_model(run):
    want, v = run.m.normal, run.m.valid
    got32 = run.n.cpu().numpy()
    got = got32.astype(np.float64)
    bound = E24 * np.abs(want) + E40
    err = np.abs(got - want)
    print("normal: worst err / bound %.3g, valid pixels %d of %d" % ((err / bound).max(), v.sum(), v.size))
    assert np.isfinite(got).all()
    assert np.all(err <= bound)
    assert not got32[~v].view(np.uint32).any()                                # invalid pixels: exactly +0, all three components
    assert (got32[v][:, 2] > 0).all()
    if all(k in RD.FLAT for k in run.case.masks):                             # no valid neighbour anywhere: n = (0, 0, 1)
        assert np.array_equal(got32[v], np.tile(np.float32([0, 0, 1]), (int(v.sum()), 1)))


# ---- 2. backward against the model ------------------------------------------------------------------------------------------------
def test_backward_vs_model(run):
    G, A, v = run.G, run.A, run.m.valid
    got32 = run.gd.cpu().numpy()
    got = got32.astype(np.float64)
    bound = E24 * np.abs(G) + E40 * A
    err = np.abs(got - G)
    print("grad_depth: worst err / bound %.3g, max |G| %.3g" % ((err / np.where(bound > 0, bound, 1)).max(), np.abs(G).max()))
    assert np.isfinite(got).all()
    assert np.all(err <= bound)
    assert not got32[..., 0][~v].view(np.uint32).any()                        # invalid pixels: exactly +0
    if all(k in RD.FLAT for k in run.case.masks) or run.case.H * run.case.W == 1:
        assert not G.any() and not got32.any()                                # no valid pixel has a valid neighbour: the gradient is 0
    else:
        assert np.abs(G).max() > 1e-3                                         # (the test cannot pass on zeros)


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------
def test_same_call_twice_same_bits(run):
    assert _same(fwd(run.z, run.mask), run.n) and _same(bwd(run.g, run.z, run.mask), run.gd)


def test_null_mask_equals_a_mask_of_zeros():
    r = _run(RD.Case(1, 33, 67, ("null",)))
    assert r.mask is None
    zeros = torch.zeros((1, 33, 67, 1), device=DEV)
    assert _same(fwd(r.z, zeros), r.n) and _same(bwd(r.g, r.z, zeros), r.gd)
    assert float(r.gd.abs().max()) > 1e-3


def test_bits_do_not_depend_on_position_or_geometry():
    """a 20 x 37 patch (more than a tile each way) whose border ring is invalid: its interior's normals and gradients have the same
    bits on its own and inside a 3 x 60 x 70 image at two offsets, on two faces -- other tiles, other lanes, other halo lanes"""
    tw, th = RD.tile()
    Hp, Wp = th + 4, tw + 5
    rs = np.random.RandomState(7)
    pc = RD.Case(1, Hp, Wp, ("nan",))
    d = RD.inputs(pc, seed=3)
    mask = d["mask"].copy()
    mask[:, 0, :], mask[:, -1, :], mask[:, :, 0], mask[:, :, -1] = -1, -1, -1, -1
    z, m, g = _t(d["depth"]), _t(mask), _t(d["grad_normal"])
    n0, gd0 = fwd(z, m), bwd(g, z, m)
    assert float(gd0.abs().max()) > 1e-3 and float(n0[..., :2].abs().max()) > 1e-3
    B, H, W = 3, 60, 70
    for b, r0, c0 in ((0, 0, 0), (2, 13, 29), (1, H - Hp, W - Wp)):
        Z = torch.as_tensor(rs.uniform(1, 100, (B, H, W, 1)).astype(np.float32), device=DEV)
        M = torch.as_tensor(rs.randint(-1, 50, (B, H, W, 1)).astype(np.float32), device=DEV)
        Gn = torch.as_tensor(rs.standard_normal((B, H, W, 3)).astype(np.float32), device=DEV)
        Z[b, r0:r0 + Hp, c0:c0 + Wp] = z[0]
        M[b, r0:r0 + Hp, c0:c0 + Wp] = m[0]
        Gn[b, r0:r0 + Hp, c0:c0 + Wp] = g[0]
        N, GD = fwd(Z, M), bwd(Gn, Z, M)
        assert _same(N[b, r0:r0 + Hp, c0:c0 + Wp], n0[0]), (b, r0, c0)
        assert _same(GD[b, r0:r0 + Hp, c0:c0 + Wp], gd0[0]), (b, r0, c0)


# ---- 4. a non-finite depth stays in the stencils that read it -----------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_depth_is_contained(bad):
    r = _dense()
    tw, th = RD.tile()
    y, x = th, tw                                                             # the first pixel of the tile diagonal to tile (0, 0)
    z = r.z.clone()
    z[0, y, x, 0] = bad
    n, gd = fwd(z, r.mask), bwd(r.g, z, r.mask)
    torch.cuda.synchronize()
    H, W = r.case.H, r.case.W
    rr, cc = np.mgrid[0:H, 0:W]
    dist = np.abs(rr - y) + np.abs(cc - x)
    keep_f = torch.as_tensor(dist != 1, device=DEV)                           # the forward reads z(p) at p's four neighbours
    keep_b = torch.as_tensor(dist > 2, device=DEV)                            # the backward: the 13-point neighbourhood
    assert _same(n[0][keep_f], r.n[0][keep_f]) and _same(gd[0][keep_b], r.gd[0][keep_b])
    hit = torch.as_tensor(dist == 1, device=DEV)
    changed = int((_bits(n[0][hit]) != _bits(r.n[0][hit])).sum())
    print("forward: %d of %d stencil components changed" % (changed, int(hit.sum()) * 3))
    assert changed > 0 and not _same(gd, r.gd)


# ---- 5. two host threads, two streams ---------------------------------------------------------------------------------------------
def test_two_threads_two_streams():
    r = _run(RD.Case(3, 33, 67, ("disc", "runs2", "corner")))
    res, err = {}, []

    def work(i):
        try:
            s = torch.cuda.Stream(device=DEV)
            z, m, g = r.z.clone(), r.mask.clone(), r.g.clone()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                for _ in range(4):
                    n, gd = fwd(z, m), bwd(g, z, m)
            s.synchronize()
            res[i] = (n, gd)
        except Exception as e:  # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not err, err
    for i in range(2):
        assert _same(res[i][0], r.n) and _same(res[i][1], r.gd)


# ---- 6. operator surface ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [RD.Case(3, 33, 67, ("disc", "runs2", "corner")), RD.Case(1, 33, 67, ("null",))], ids=RD.case_id)
def test_operator_and_its_autograd(case):
    o = pkg("rendering_layer.ops")
    r = _run(case)
    B, H, W = case.B, case.H, case.W
    for shape in ((B, H, W, 1), (B, H, W)):
        z = r.z.clone().reshape(shape).requires_grad_(True)
        mask = None if r.mask is None else r.mask.reshape(shape)
        n = o.depth_normals(z, mask) if mask is not None else o.depth_normals(z)
        assert tuple(n.shape) == (B, H, W, 3) and _same(n, r.n)
        n.backward(r.g)
        assert tuple(z.grad.shape) == shape and _same(z.grad.reshape(B, H, W, 1), r.gd)
    z = r.z.clone().requires_grad_(True)
    with pytest.raises(ValueError):
        o.depth_normals(z, torch.zeros((B, H, W, 1), device=DEV, requires_grad=True))
    with pytest.raises(ValueError):
        o.depth_normals(z, torch.zeros((B, H, W + 1, 1), device=DEV))
    with pytest.raises(ValueError):
        o.depth_normals(r.z.reshape(B, H * W))
    with pytest.raises(RuntimeError):
        o.depth_normals(r.z.cpu())
    with pytest.raises(TypeError):
        o.depth_normals(r.z.double())
    assert not o.depth_normals(r.z, r.mask).requires_grad                     # nothing to differentiate: no node


# ---- 7. end to end: the objective's flag ------------------------------------------------------------------------------------------
def test_get_loss_sfs_fine(small_assets):
    netm, L = pkg("nets.network"), pkg("nets.losses")
    A = small_assets
    B, S = 4, 40
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S)
    rs = np.random.RandomState(3)                                             # the parameter recipe of test_sfs_gpu.py
    nd = net.ndim
    P = np.zeros((B, nd), np.float32)
    P[:, 0:3] = rs.uniform(-1.0, 1.0, (B, 3))
    P[:, 3:5] = rs.uniform(17, 23, (B, 2))
    P[:, 6] = rs.uniform(1.6e-4, 2.2e-4, B)
    P[:, 7:] = np.concatenate([rs.uniform(0, 1e4, (B, A["ndim_shape"])), rs.uniform(-1.5, 1.5, (B, A["ndim_exp"]))], 1)
    lab = P + rs.standard_normal(P.shape).astype(np.float32) * np.array([0.1] * 3 + [2, 2, 0, 1e-5] + [300.0] * (nd - 7),
                                                                         np.float32)
    pred = torch.as_tensor(P, device=DEV)
    label = torch.as_tensor(lab, device=DEV)
    im = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        V = net.vertices_transform(pred)
        coarse = net.coarse_net_input(V, im_gray=im)[1]
    fine = (coarse + 0.05 * torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(2)).to(DEV)).detach()
    fine.requires_grad_(True)                                                 # a leaf, as FineNet's output is to this objective

    def loss(**kw):
        return L.get_loss(net, pred, label, im, V, coarse, fine, **kw)

    def grad(scalar):
        if not scalar.requires_grad:
            return None
        return torch.autograd.grad(scalar, fine, retain_graph=True, allow_unused=True)[0]
    # flag off: today's bits, and the SfS scalar has no path to the fine depth map
    off, off2, off_flag = loss(), loss(), loss(sfs_fine=False)
    for k in off:
        assert _same(off[k], off2[k]) and _same(off[k], off_flag[k]), k
    g_off = grad(off["spherical_harmonics_loss"])
    assert g_off is None or not bool(g_off.any())
    assert bool(grad(off["fidelity_loss"]).any())                             # (the other terms do reach it)
    # the returned tri_ind is the render's, and the default return is unchanged
    a2, n2 = net.compute_abedo_image(V, net.tri, net.mu_tex)
    a3, n3, ti = net.compute_abedo_image(V, net.tri, net.mu_tex, with_tri_ind=True)
    assert _same(a2, a3) and _same(n2, n3) and tuple(ti.shape) == (B, S, S, 1) and bool((ti >= 0).any()) and bool((ti < 0).any())
    # flag on: both routes give the leaf a finite, non-zero gradient from the SfS term alone
    got = {}
    for fused in (False, True):
        on = loss(sfs_fine=True, sfs_fused=fused, sfs_rcond=1e-6)
        for k in off:
            if k not in ("spherical_harmonics_loss", "total_loss"):
                assert _same(off[k], on[k]), k
        fine.grad = None
        on["spherical_harmonics_loss"].backward()
        g = fine.grad.clone()
        covered = ti >= 0
        print("fused=%s: SfS loss %.6g, max |d SfS / d fine depth| %.3g, non-zero on %d of %d covered pixels"
              % (fused, float(on["spherical_harmonics_loss"].detach()), float(g.abs().max()), int((g != 0).sum()), int(covered.sum())))
        assert np.isfinite(float(on["spherical_harmonics_loss"].detach()))
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert not bool(g[~covered].any())                                    # nothing outside the face
        got[fused] = (float(on["spherical_harmonics_loss"].detach()), g)
    fine.grad = None
    # the other flags beside it: the gradient of the shaded normals is local and does not depend on which other outputs the fused
    # backward forms, so the fine depth map's gradient keeps the bits of the fused route (no process group: the sharded node equals
    # the one-call node)
    for kw in ({"gather_sfs": True, "sfs_fused_gather": True}, {"sfs_normal_grad": True, "sfs_tex_grad": True}):
        on = loss(sfs_fine=True, sfs_fused=True, sfs_rcond=1e-6, **kw)
        assert _same(on["spherical_harmonics_loss"], loss(sfs_fine=True, sfs_fused=True, sfs_rcond=1e-6)["spherical_harmonics_loss"]), kw
        assert _same(grad(on["spherical_harmonics_loss"]), got[True][1]), kw
    # the two routes: the intensity on the well-conditioned pixels to the tolerance test_sfs_gpu.py::test_get_loss_flags uses for
    # fused vs torch (rtol 2e-2, atol 2e-3)
    with torch.no_grad():
        alb, nmap = net.compute_abedo_image(V, net.tri, net.mu_tex)
        I_t = L.get_spherical_harmonics_model(net, V, im, rcond=1e-6, fine_depth=fine).cpu().numpy()
        I_f = L.get_spherical_harmonics_model(net, V, im, rcond=1e-6, fused=True, fine_depth=fine).cpu().numpy()
    Y = np.transpose(nmap.cpu().numpy(), [1, 2, 3, 0]).astype(np.float64)
    sv = np.linalg.svd(Y @ np.transpose(Y, [0, 1, 3, 2]), compute_uv=False)
    good = sv[..., 2] > 1e-3 * sv[..., 0]
    print("well-conditioned pixels: %d" % good.sum())
    assert good.sum() >= 20, int(good.sum())
    np.testing.assert_allclose(I_f[:, good], I_t[:, good], rtol=2e-2, atol=2e-3)
    # ... and the gradient, where the pixel and its four neighbours are well-conditioned (a gradient gathers their lighting): the
    # same relative tolerance, the absolute one scaled to the largest entry (the intensity is of order 1, the gradient is not)
    near = good.copy()
    near[1:] &= good[:-1]
    near[:-1] &= good[1:]
    near[:, 1:] &= good[:, :-1]
    near[:, :-1] &= good[:, 1:]
    g_t, g_f = got[False][1].cpu().numpy()[:, near], got[True][1].cpu().numpy()[:, near]
    print("gradient on %d pixels: max |fused - torch| %.3g, max |torch| %.3g" % (near.sum(), np.abs(g_f - g_t).max(), np.abs(g_t).max()))
    assert near.sum() >= 10 and np.abs(g_t).max() > 0
    np.testing.assert_allclose(g_f, g_t, rtol=2e-2, atol=2e-3 * np.abs(g_t).max())
    with pytest.raises(ValueError):
        L.get_loss(net, pred, label, im, V, coarse, None, sfs_fine=True)
