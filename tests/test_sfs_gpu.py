"""GPU: fr_sfs_intensity_forward / _backward (sfs_forward_kernel, sfs_backward_kernel) held to their float64 model
(tests/ref_sfs.py, pinned on the CPU by tests/test_sfs_cpu.py), to the project's numpy oracle of the reference formula, and the
opt-in sfs_* flags of the objective.

forward:   rank exact;  |P - P_m| <= 2^-40 ||P_m||,  |l - l_m| <= 2^-40 ||l_m||  per pixel;
           |intensity - I_m| <= 2^-24 |I_m| + 2^-40 a' ||l|| ||n'||       (one fp32 rounding + the float64 error under cancellation)
backward:  |grad_normal - G_m| <= 2^-24 |G_m| + 2^-40 |u_b| ||P||_F ||q||,   |grad_normal_new - G'_m| <= 2^-24 |G'_m| + 2^-40 |g_b a'_b| ||l||
Every figure is printed before it is asserted."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import ref_sfs as RS
from conftest import pkg
from oracle import losses_np as LN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E40, E24 = 2.0 ** -40, 2.0 ** -24
KEYS = ("abedo", "normal", "im_gray", "abedo_new", "normal_new")


def _h():
    return pkg("_lib")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def fwd(t, rcond=RS.RCOND, shape=None, state=None):
    """fr_sfs_intensity_forward on torch's current stream (device tensors; not synchronised) -> (intensity [B,H,W,1] pre-filled with
    NaN, state [10,H,W] float64 pre-filled with NaN unless `state` is given)"""
    h, L = _h(), _h().lib()
    B, H, W = shape or tuple(t["normal"].shape[:3])
    nst = L.fr_sfs_state_bytes(H, W)
    if state is None:
        state = torch.full((10, H, W), float("nan"), dtype=torch.float64, device=DEV)
    assert state.numel() * 8 == nst
    out = torch.full((B, H, W, 1), float("nan"), device=DEV)
    rc = L.fr_sfs_intensity_forward(h.ptr(t["abedo"]), h.ptr(t["normal"]), h.ptr(t["im_gray"]), h.ptr(t["abedo_new"]),
                                    h.ptr(t["normal_new"]), B, H, W, rcond, h.ptr(out), h.ptr(state), nst, _sp())
    assert rc == 0, rc
    return out, state


def bwd(g, t, state, which=(True, True), shape=None):
    """fr_sfs_intensity_backward -> (grad_normal, grad_normal_new), NaN pre-filled; an output not asked for is passed as NULL"""
    h, L = _h(), _h().lib()
    B, H, W = shape or tuple(t["normal"].shape[:3])
    outs = [torch.full((B, H, W, 3), float("nan"), device=DEV) if w else None for w in which]
    rc = L.fr_sfs_intensity_backward(h.ptr(g), h.ptr(t["abedo"]), h.ptr(t["im_gray"]), h.ptr(t["abedo_new"]), h.ptr(t["normal_new"]),
                                     h.ptr(state), L.fr_sfs_state_bytes(H, W), B, H, W, h.ptr(outs[0]), h.ptr(outs[1]), _sp())
    assert rc == 0, rc
    return outs


class Case:
    """one shape: inputs, the model (computed once, never changed), and one forward + backward of the product"""

    def __init__(self, shape):
        self.shape = shape
        self.d = RS.inputs(*shape)
        self.m = RS.model(*RS.args(self.d))
        self.g = RS.grad_out(*shape)
        self.t = {k: _t(v) for k, v in self.d.items()}
        self.gt = _t(self.g)
        self.out, self.state = fwd(self.t)
        self.gn, self.gn2 = bwd(self.gt, self.t, self.state)
        torch.cuda.synchronize()


_CASES = {}


@pytest.fixture(params=RS.CASES, ids=lambda c: "B%d_%dx%d" % c)
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param)
    return _CASES[request.param]


def _big():
    if RS.CASES[1] not in _CASES:
        _CASES[RS.CASES[1]] = Case(RS.CASES[1])
    return _CASES[RS.CASES[1]]


# ---- 1. forward against the model ---------------------------------------------------------------------------------------------
def test_forward_vs_model(case):
    m, d = case.m, case.d
    st = case.state.cpu().numpy()
    got = case.out.cpu().numpy().astype(np.float64)
    assert np.array_equal(st[9], m.rank.astype(np.float64))                   # kept eigenvalues: exact
    P6 = RS.p6(m.P)
    nP = np.sqrt((m.P ** 2).sum((-1, -2)))
    nl = np.sqrt((m.l ** 2).sum(-1))
    eP = np.abs(st[0:6] - P6).max(0)
    el = np.abs(st[6:9] - np.moveaxis(m.l, -1, 0)).max(0)
    print("P: worst err/||P|| %.3g   l: worst err/||l|| %.3g   (bound %.3g)" %
          ((eP / np.where(nP > 0, nP, 1)).max(), (el / np.where(nl > 0, nl, 1)).max(), E40))
    assert np.all(eP <= E40 * nP) and np.all(el <= E40 * nl)
    want = m.intensity
    a2 = d["abedo_new"].astype(np.float64)
    nn2 = np.sqrt((d["normal_new"].astype(np.float64) ** 2).sum(-1, keepdims=True))
    bound = E24 * np.abs(want) + E40 * a2 * nl[None, ..., None] * nn2
    err = np.abs(got - want)
    print("intensity: worst err / bound %.3g, max |I| %.3g" % ((err / np.where(bound > 0, bound, 1)).max(), np.abs(want).max()))
    assert np.all(err <= bound)
    assert bool((case.out[:, 0, 0] == 0).all()) and not st[:9, 0, 0].any()    # nobody covers pixel (0,0): exactly 0 for every face
    assert np.isfinite(got).all()


# ---- 2. forward against the project's oracle of the reference formula -----------------------------------------------------------
@pytest.mark.parametrize("shape,least", [((6, 5, 4), 16), ((64, 9, 70), 626), ((65, 3, 67), 197)], ids=lambda v: str(v))
def test_forward_vs_oracle(shape, least):
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    c = _CASES[shape]
    out, _ = fwd(c.t, rcond=1e-15)
    got = out.cpu().numpy()
    want = LN.spherical_harmonics_intensity(*RS.args(c.d))
    good = c.m.lam[..., 0] > 1e-3 * c.m.lam[..., 2]
    print("well-conditioned pixels: %d of %d" % (good.sum(), good.size))
    assert good.sum() >= least
    np.testing.assert_allclose(got[:, good], want[:, good], rtol=2e-3, atol=2e-4)


# ---- 3. backward against the model ----------------------------------------------------------------------------------------------
def test_backward_vs_model(case):
    m, d = case.m, case.d
    Gn, Gn2, q, ga = RS.grads(case.g, *RS.args(d), m=m)
    gn, gn2 = case.gn.cpu().numpy().astype(np.float64), case.gn2.cpu().numpy().astype(np.float64)
    nP = np.sqrt((m.P ** 2).sum((-1, -2)))
    nq = np.sqrt((q ** 2).sum(-1))
    nl = np.sqrt((m.l ** 2).sum(-1))
    b1 = E24 * np.abs(Gn) + E40 * (np.abs(m.u) * (nP * nq)[None])[..., None]
    b2 = E24 * np.abs(Gn2) + E40 * (np.abs(ga) * nl[None])[..., None]
    e1, e2 = np.abs(gn - Gn), np.abs(gn2 - Gn2)
    print("grad_normal: worst err / bound %.3g (max |G| %.3g)   grad_normal_new: %.3g (max %.3g)" %
          ((e1 / np.where(b1 > 0, b1, 1)).max(), np.abs(Gn).max(), (e2 / np.where(b2 > 0, b2, 1)).max(), np.abs(Gn2).max()))
    assert np.all(e1 <= b1) and np.all(e2 <= b2)
    assert np.abs(Gn).max() > 1e-3 and np.abs(Gn2).max() > 1e-3
    only_n, none = bwd(case.gt, case.t, case.state, which=(True, False))
    none2, only_n2 = bwd(case.gt, case.t, case.state, which=(False, True))
    assert none is None and none2 is None
    assert _same(only_n, case.gn) and _same(only_n2, case.gn2)                # each output alone: the joint call's bits


# ---- 4. association ---------------------------------------------------------------------------------------------------------------
def test_same_call_twice_same_bits(case):
    out, state = fwd(case.t)
    gn, gn2 = bwd(case.gt, case.t, case.state)
    assert _same(out, case.out) and _same(state, case.state) and _same(gn, case.gn) and _same(gn2, case.gn2)


@pytest.mark.parametrize("H,W", [(70, 9), (1, 630)])
def test_bits_do_not_depend_on_the_image_shape(H, W):
    c = _big()
    B = c.shape[0]
    out, state = fwd(c.t, shape=(B, H, W))                                    # the same memory read as [64,H,W,c]
    gn, gn2 = bwd(c.gt, c.t, state, shape=(B, H, W))
    assert _same(out.reshape(-1), c.out.reshape(-1)) and _same(state.reshape(10, -1), c.state.reshape(10, -1))
    assert _same(gn.reshape(-1), c.gn.reshape(-1)) and _same(gn2.reshape(-1), c.gn2.reshape(-1))


def test_aliased_normal_new(case):
    t_alias = dict(case.t, normal_new=case.t["normal"])
    t_copy = dict(case.t, normal_new=case.t["normal"].clone())
    assert t_alias["normal_new"].data_ptr() == t_alias["normal"].data_ptr() != t_copy["normal_new"].data_ptr()
    oa, sa = fwd(t_alias)
    oc, sc = fwd(t_copy)
    ga = bwd(case.gt, t_alias, sa)
    gc = bwd(case.gt, t_copy, sc)
    assert _same(oa, oc) and _same(sa, sc) and _same(ga[0], gc[0]) and _same(ga[1], gc[1])
    assert _same(sa, case.state)                                              # the state does not read normal_new at all


# ---- 5. a NaN stays in its pixel ------------------------------------------------------------------------------------------------
def test_nan_in_one_normal_stays_in_its_pixel():
    c = _big()
    B, H, W = c.shape
    y, x, b = 1, 30, 37                                                       # pixel 100: inside the second workgroup; a face of slice 2
    n = c.t["normal"].clone()
    n[b, y, x, 1] = float("nan")
    out, state = fwd(dict(c.t, normal=n))
    torch.cuda.synchronize()                                                  # (the call returned: no loop waits for convergence)
    assert bool(torch.isnan(out[:, y, x]).all()) and bool(torch.isnan(state[:9, y, x]).all())
    keep = torch.ones((H, W), dtype=torch.bool, device=DEV)
    keep[y, x] = False
    assert _same(out[:, keep], c.out[:, keep]) and _same(state[:, keep], c.state[:, keep])


# ---- 6. two host threads, two streams -------------------------------------------------------------------------------------------
def test_two_threads_two_streams():
    c = _big()
    res, err = {}, []

    def work(i):
        try:
            s = torch.cuda.Stream(device=DEV)
            t = {k: v.clone() for k, v in c.t.items()}
            g = c.gt.clone()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                for _ in range(4):
                    out, state = fwd(t)
                    gn, gn2 = bwd(g, t, state)
            s.synchronize()
            res[i] = (out, state, gn, gn2)
        except Exception as e:  # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not err, err
    for i in range(2):
        for got, want in zip(res[i], (c.out, c.state, c.gn, c.gn2)):
            assert _same(got, want)


# ---- operator surface -------------------------------------------------------------------------------------------------------------
def test_operator_and_its_autograd(case):
    o = pkg("rendering_layer.ops")
    t = case.t
    n = t["normal"].clone().requires_grad_(True)
    n2 = t["normal_new"].clone().requires_grad_(True)
    out = o.sfs_intensity(t["abedo"], n, t["im_gray"], t["abedo_new"], n2, rcond=RS.RCOND)
    assert _same(out, case.out)
    out.backward(case.gt)
    assert _same(n.grad, case.gn) and _same(n2.grad, case.gn2)
    one = t["normal"].clone().requires_grad_(True)                            # one tensor passed twice: autograd adds the two maps
    out1 = o.sfs_intensity(t["abedo"], one, t["im_gray"], t["abedo_new"], one, rcond=RS.RCOND)
    out1.backward(case.gt)
    st = fwd(dict(t, normal_new=t["normal"]))[1]
    a, b = bwd(case.gt, dict(t, normal_new=t["normal"]), st)
    assert _same(one.grad, a + b)
    with pytest.raises(ValueError):
        o.sfs_intensity(t["abedo"].clone().requires_grad_(True), n, t["im_gray"], t["abedo_new"], n2)
    with pytest.raises(ValueError):
        o.sfs_intensity(t["abedo"], n, t["im_gray"].clone().requires_grad_(True), t["abedo_new"], n2)
    with pytest.raises(RuntimeError):
        o.sfs_intensity(t["abedo"].cpu(), n, t["im_gray"], t["abedo_new"], n2)
    with pytest.raises(TypeError):
        o.sfs_intensity(t["abedo"].double(), n, t["im_gray"], t["abedo_new"], n2)


# ---- 7. end to end: the objective's flags -----------------------------------------------------------------------------------------
def test_get_loss_flags(small_assets):
    netm, L = pkg("nets.network"), pkg("nets.losses")
    A = small_assets
    B, S = 4, 40
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S)
    rs = np.random.RandomState(3)                                             # the parameter recipe of test_losses_gpu.py
    nd = net.ndim
    P = np.zeros((B, nd), np.float32)
    P[:, 0:3] = rs.uniform(-1.0, 1.0, (B, 3))
    P[:, 3:5] = rs.uniform(17, 23, (B, 2))
    P[:, 6] = rs.uniform(1.6e-4, 2.2e-4, B)
    P[:, 7:] = np.concatenate([rs.uniform(0, 1e4, (B, A["ndim_shape"])), rs.uniform(-1.5, 1.5, (B, A["ndim_exp"]))], 1)
    lab = P + rs.standard_normal(P.shape).astype(np.float32) * np.array([0.1] * 3 + [2, 2, 0, 1e-5] + [300.0] * (nd - 7),
                                                                         np.float32)
    pred = torch.as_tensor(P, device=DEV).requires_grad_(True)
    label = torch.as_tensor(lab, device=DEV)
    im = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(1)).to(DEV)
    V = net.vertices_transform(pred)
    coarse = net.coarse_net_input(V, im_gray=im)[1]
    fine = (coarse + 0.05 * torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(2)).to(DEV)).detach()

    def loss(**kw):
        return L.get_loss(net, pred, label, im, V, coarse, fine, **kw)

    def grad(scalar):
        if not scalar.requires_grad:                                          # no path to anything: nothing to differentiate
            return None
        return torch.autograd.grad(scalar, pred, retain_graph=True, allow_unused=True)[0]
    off, off2, fused = loss(), loss(), loss(sfs_fused=True)
    assert set(off) == set(fused)
    for k in off:                                                             # flags off: the same bits, call after call
        assert _same(off[k], off2[k]), k
    g_sh = grad(off["spherical_harmonics_loss"])                              # ... and the SfS scalar has no path to pred
    assert g_sh is None or not bool(g_sh.any())
    for k in off:
        if k not in ("spherical_harmonics_loss", "total_loss"):
            assert _same(off[k], fused[k]), k
    assert np.isfinite(float(fused["spherical_harmonics_loss"]))
    g_f = grad(fused["spherical_harmonics_loss"])                             # fused alone moves nothing either
    assert g_f is None or not bool(g_f.any())
    # the fused and the torch intensity on the pixels test_get_loss_vs_numpy selects
    with torch.no_grad():
        alb, nmap = net.compute_abedo_image(V, net.tri, net.mu_tex)
        tex_new = net.mu_tex + (net.pc_tex @ net.param_tex).reshape(3, -1)
        alb2, nmap2 = net.compute_abedo_image(V, net.tri, tex_new)
        I_t = L.spherical_harmonics_intensity(alb, nmap, im, alb2, nmap2).cpu().numpy()
        I_f = L.spherical_harmonics_intensity(alb, nmap, im, alb2, nmap2, fused=True).cpu().numpy()
    Y = np.transpose(nmap.cpu().numpy(), [1, 2, 3, 0]).astype(np.float64)
    sv = np.linalg.svd(Y @ np.transpose(Y, [0, 1, 3, 2]), compute_uv=False)
    good = sv[..., 2] > 1e-3 * sv[..., 0]
    print("well-conditioned pixels: %d" % good.sum())
    assert good.sum() >= 20, int(good.sum())
    np.testing.assert_allclose(I_f[:, good], I_t[:, good], rtol=2e-2, atol=2e-3)
    # the term moves the geometry once its renders carry the normal map's gradient
    g_off = grad(off["total_loss"])
    for fused_flag in (True, False):
        on = loss(sfs_normal_grad=True, sfs_fused=fused_flag, sfs_rcond=1e-6)
        g_on = grad(on["total_loss"])
        g_s = grad(on["spherical_harmonics_loss"])
        assert bool(torch.isfinite(g_on).all()) and bool(torch.isfinite(g_s).all())
        assert float(g_s[:, 7:].abs().max()) > 0
        assert not torch.equal(g_on[:, 7:], g_off[:, 7:])
        print("fused=%s: max |d SfS / d coeff| %.3g" % (fused_flag, float(g_s[:, 7:].abs().max())))
    # with pose gradients on as well, the SfS term reaches the three angles
    Vp = net.vertices_transform(pred, pose_grad=True)
    on = L.get_loss(net, pred, label, im, Vp, coarse, fine, sfs_normal_grad=True, sfs_fused=True, sfs_rcond=1e-6)
    g_p = torch.autograd.grad(on["spherical_harmonics_loss"], pred)[0]
    assert bool(torch.isfinite(g_p).all()) and float(g_p[:, 0:3].abs().max()) > 0
