"""GPU: the split shape-from-shading entry points (fr_sfs_moments / fr_sfs_solve_shade / fr_sfs_backward_q / fr_sfs_backward_apply),
the operator sfs_intensity_sharded and the fused_gather flags of the objective, held to
  * the one-call kernels, bit for bit, at one part, and
  * the float64 model of tests/ref_sfs.py on the CONCATENATED batch -- which does not know about the sharding -- at several parts,
    with the bounds of tests/test_sfs_gpu.py unchanged:
      rank exact;  |P - P_m| <= 2^-40 ||P_m||,  |l - l_m| <= 2^-40 ||l_m||  per pixel;
      |intensity - I_m| <= 2^-24 |I_m| + 2^-40 a' ||l|| ||n'||
      |grad_normal - G_m| <= 2^-24 |G_m| + 2^-40 |u_b| ||P||_F ||q||,   |grad_normal_new - G'_m| <= 2^-24 |G'_m| + 2^-40 |g_b a'_b| ||l||
      |grad_abedo_new - g (l_m . n')| <= 2^-24 |g (l_m . n')| + 2^-40 |g| ||l|| ||n'||
Every figure is printed before it is asserted."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_sfs as RS
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E40, E24 = 2.0 ** -40, 2.0 ** -24
NAN = float("nan")
# faces per part, ascending: S = 1, 2 and 4, uneven last slices, a one-face part, an empty part
SHARDINGS = {(6, 5, 4): ((3, 3), (1, 5), (0, 2, 4)),
             (64, 9, 70): ((8,) * 8, (40, 24), (17, 17, 17, 13)),
             (65, 3, 67): ((64, 1), (1, 64), (33, 32)),
             (1, 4, 4): ((0, 1),)}
ALL = [(shape, sh) for shape in RS.CASES for sh in SHARDINGS[shape]]
_ids = lambda v: "B%d_%dx%d-" % v[0] + "_".join(map(str, v[1]))  # noqa: E731


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


def _np(t):
    return t.cpu().numpy().astype(np.float64)


# ---- the C ABI, outputs pre-filled with NaN -------------------------------------------------------------------------------------------
def one_fwd(t, shape):
    h, L = _h(), _h().lib()
    B, H, W = shape
    state = torch.full((10, H, W), NAN, dtype=torch.float64, device=DEV)
    out = torch.full((B, H, W, 1), NAN, device=DEV)
    rc = L.fr_sfs_intensity_forward(h.ptr(t["abedo"]), h.ptr(t["normal"]), h.ptr(t["im_gray"]), h.ptr(t["abedo_new"]),
                                    h.ptr(t["normal_new"]), B, H, W, RS.RCOND, h.ptr(out), h.ptr(state), state.numel() * 8, _sp())
    assert rc == 0, rc
    return out, state


def _grad_outs(shape, which):
    B, H, W = shape
    return [torch.full((B, H, W, c), NAN, device=DEV) if w else None for w, c in zip(which, (3, 3, 1))]


def one_bwd(g, t, state, shape, which=(True, True, True)):
    h, L = _h(), _h().lib()
    B, H, W = shape
    o = _grad_outs(shape, which)
    rc = L.fr_sfs_intensity_backward_tex(h.ptr(g), h.ptr(t["abedo"]), h.ptr(t["im_gray"]), h.ptr(t["abedo_new"]),
                                         h.ptr(t["normal_new"]), h.ptr(state), state.numel() * 8, B, H, W, h.ptr(o[0]), h.ptr(o[1]),
                                         h.ptr(o[2]), _sp())
    assert rc == 0, rc
    return o


def moments(t, shape, m=None):
    h, L = _h(), _h().lib()
    B, H, W = shape
    if m is None:
        m = torch.full((9, H, W), NAN, dtype=torch.float64, device=DEV)
    assert m.numel() * 8 == L.fr_sfs_moments_bytes(H, W)
    rc = L.fr_sfs_moments(h.ptr(t["abedo"]), h.ptr(t["normal"]), h.ptr(t["im_gray"]), B, H, W, h.ptr(m), L.fr_sfs_moments_bytes(H, W),
                          _sp())
    assert rc == 0, rc
    return m


def solve_shade(parts, t, shape, state=None):
    h, L = _h(), _h().lib()
    B, H, W = shape
    assert parts.is_contiguous() and parts.dtype == torch.float64 and parts.numel() == parts.shape[0] * 9 * H * W
    if state is None:
        state = torch.full((10, H, W), NAN, dtype=torch.float64, device=DEV)
    assert state.numel() == 10 * H * W
    out = torch.full((B, H, W, 1), NAN, device=DEV)
    rc = L.fr_sfs_solve_shade(h.ptr(parts), int(parts.shape[0]), h.ptr(t["abedo_new"]), h.ptr(t["normal_new"]), B, H, W, RS.RCOND,
                              h.ptr(out), h.ptr(state), state.numel() * 8, _sp())
    assert rc == 0, rc
    return out, state


def backward_q(g, t, shape, q=None):
    h, L = _h(), _h().lib()
    B, H, W = shape
    if q is None:
        q = torch.full((3, H, W), NAN, dtype=torch.float64, device=DEV)
    assert q.numel() * 8 == L.fr_sfs_q_bytes(H, W)
    rc = L.fr_sfs_backward_q(h.ptr(g), h.ptr(t["abedo_new"]), h.ptr(t["normal_new"]), B, H, W, h.ptr(q), L.fr_sfs_q_bytes(H, W), _sp())
    assert rc == 0, rc
    return q


def backward_apply(g, t, state, qparts, shape, which=(True, True, True)):
    h, L = _h(), _h().lib()
    B, H, W = shape
    o = _grad_outs(shape, which)
    if qparts is not None:
        assert qparts.is_contiguous() and qparts.dtype == torch.float64 and qparts.numel() == qparts.shape[0] * 3 * H * W
    rc = L.fr_sfs_backward_apply(h.ptr(g), h.ptr(t["abedo"]), h.ptr(t["im_gray"]), h.ptr(t["abedo_new"]), h.ptr(t["normal_new"]),
                                 h.ptr(state), state.numel() * 8, h.ptr(qparts), int(qparts.shape[0]) if qparts is not None else 1,
                                 B, H, W, h.ptr(o[0]), h.ptr(o[1]), h.ptr(o[2]), _sp())
    assert rc == 0, rc
    return o


# ---- shared, computed once and never changed ----------------------------------------------------------------------------------------
class Case:
    """one shape: inputs, the whole-batch model and the one-call kernels' outputs"""

    def __init__(self, shape):
        self.shape = shape
        self.d = RS.inputs(*shape)
        self.m = RS.model(*RS.args(self.d))
        self.g = RS.grad_out(*shape)
        self.t = {k: _t(v) for k, v in self.d.items()}
        self.gt = _t(self.g)
        self.out, self.state = one_fwd(self.t, shape)
        self.gn, self.gn2, self.ga2 = one_bwd(self.gt, self.t, self.state, shape)
        torch.cuda.synchronize()


class Sharded:
    """one sharding of a case through the C ABI: a moment part per shard, every shard solved with the same stacked buffer, a q part
    per shard, every shard's gradients from the same stacked q"""

    def __init__(self, c, sizes, t=None, hw=None):
        assert sum(sizes) == c.shape[0]
        t = c.t if t is None else t
        H, W = hw or c.shape[1:]
        self.sizes, self.hw = sizes, (H, W)
        edges = np.concatenate([[0], np.cumsum(sizes)])
        self.shapes = [(n, H, W) for n in sizes]
        self.ts = [{k: v[lo:hi] for k, v in t.items()} for lo, hi in zip(edges[:-1], edges[1:])]
        self.gs = [c.gt[lo:hi] for lo, hi in zip(edges[:-1], edges[1:])]
        self.mparts = [moments(tp, sp) for tp, sp in zip(self.ts, self.shapes)]
        self.mstack = torch.stack(self.mparts).contiguous()
        fw = [solve_shade(self.mstack, tp, sp) for tp, sp in zip(self.ts, self.shapes)]
        self.outs, self.states = [f[0] for f in fw], [f[1] for f in fw]
        self.qparts = [backward_q(g, tp, sp) for g, tp, sp in zip(self.gs, self.ts, self.shapes)]
        self.qstack = torch.stack(self.qparts).contiguous()
        self.grads = [backward_apply(g, tp, st, self.qstack, sp) for g, tp, st, sp in zip(self.gs, self.ts, self.states, self.shapes)]
        torch.cuda.synchronize()
        self.live = [i for i, n in enumerate(sizes) if n]                   # (an empty shard's finishing calls write nothing)
        self.out = torch.cat(self.outs)
        self.gn, self.gn2, self.ga2 = (torch.cat([g[k] for g in self.grads]) for k in range(3))
        self.state = self.states[self.live[0]]


_CASES, _SHARDED = {}, {}


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


def _sharded(shape, sizes):
    if (shape, sizes) not in _SHARDED:
        _SHARDED[(shape, sizes)] = Sharded(_case(shape), sizes)
    return _SHARDED[(shape, sizes)]


@pytest.fixture(params=RS.CASES, ids=lambda c: "B%d_%dx%d" % c)
def case(request):
    return _case(request.param)


@pytest.fixture(params=ALL, ids=_ids)
def sharded(request):
    return _case(request.param[0]), _sharded(*request.param)


# ---- 1. one part: the one-call kernels' bits ------------------------------------------------------------------------------------------
def test_one_part_is_the_one_call_route(case):
    c = case
    m = moments(c.t, c.shape)
    out, state = solve_shade(m[None], c.t, c.shape)
    assert _same(out, c.out) and _same(state, c.state)
    q = backward_q(c.gt, c.t, c.shape)
    gn, gn2, ga2 = backward_apply(c.gt, c.t, c.state, q[None], c.shape)
    assert _same(gn, c.gn) and _same(gn2, c.gn2) and _same(ga2, c.ga2)
    for k in range(3):                                                        # each output alone: the joint call's bits
        which = tuple(j == k for j in range(3))
        alone = backward_apply(c.gt, c.t, c.state, q[None] if k == 0 else None, c.shape, which=which)
        assert [a is None for a in alone] == [not w for w in which]
        assert _same(alone[k], (c.gn, c.gn2, c.ga2)[k]), k
    assert _same(backward_apply(c.gt, c.t, c.state, q[None], c.shape, which=(False, True, True))[1], c.gn2)   # q_parts given, not read


# ---- 2. several parts: forward ------------------------------------------------------------------------------------------------------
def _check_forward(c, out, state):
    m, d = c.m, c.d
    st, got = state.cpu().numpy(), _np(out)
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
    assert np.isfinite(got).all()


def test_sharded_forward(sharded):
    c, s = sharded
    for i in s.live:
        assert _same(s.states[i], s.state), i                                 # every part holds the same lighting, bit for bit
    _check_forward(c, s.out, s.state)
    assert bool((s.out[:, 0, 0] == 0).all()) and not s.state.cpu().numpy()[:9, 0, 0].any()   # nobody covers pixel (0,0): exactly 0


# ---- 3. several parts: backward -------------------------------------------------------------------------------------------------------
def _check_backward(c, gn, gn2, ga2):
    m, d = c.m, c.d
    Gn, Gn2, q, ga = RS.grads(c.g, *RS.args(d), m=m)
    gn, gn2, ga2 = _np(gn), _np(gn2), _np(ga2)
    nP = np.sqrt((m.P ** 2).sum((-1, -2)))
    nq = np.sqrt((q ** 2).sum(-1))
    nl = np.sqrt((m.l ** 2).sum(-1))
    b1 = E24 * np.abs(Gn) + E40 * (np.abs(m.u) * (nP * nq)[None])[..., None]
    b2 = E24 * np.abs(Gn2) + E40 * (np.abs(ga) * nl[None])[..., None]
    e1, e2 = np.abs(gn - Gn), np.abs(gn2 - Gn2)
    print("grad_normal: worst err / bound %.3g (max |G| %.3g)   grad_normal_new: %.3g (max %.3g)" %
          ((e1 / np.where(b1 > 0, b1, 1)).max(), np.abs(Gn).max(), (e2 / np.where(b2 > 0, b2, 1)).max(), np.abs(Gn2).max()))
    assert np.all(e1 <= b1) and np.all(e2 <= b2)
    g64 = c.g.astype(np.float64)
    n2 = d["normal_new"].astype(np.float64)
    Ga = g64 * np.einsum("hwi,bhwi->bhw", m.l, n2)[..., None]                  # g (l_m . n')
    b3 = E24 * np.abs(Ga) + E40 * np.abs(g64) * nl[None, ..., None] * np.sqrt((n2 ** 2).sum(-1, keepdims=True))
    e3 = np.abs(ga2 - Ga)
    print("grad_abedo_new: worst err / bound %.3g (max %.3g)" % ((e3 / np.where(b3 > 0, b3, 1)).max(), np.abs(Ga).max()))
    assert np.all(e3 <= b3)
    assert np.abs(Gn).max() > 1e-3 and np.abs(Gn2).max() > 1e-3 and np.abs(Ga).max() > 1e-3


def test_sharded_backward(sharded):
    c, s = sharded
    _check_backward(c, s.gn, s.gn2, s.ga2)


# ---- 4. an empty part -----------------------------------------------------------------------------------------------------------------
def test_empty_part_changes_nothing():
    c = _case((6, 5, 4))
    a = _sharded(c.shape, (0, 2, 4))
    two = Sharded(c, (2, 4))                                                  # the same two parts without the empty one in front
    assert _same(a.out, two.out) and _same(a.state, two.state)
    assert _same(a.gn, two.gn) and _same(a.gn2, two.gn2) and _same(a.ga2, two.ga2)
    for i, j in ((1, 0), (2, 1)):
        assert _same(a.mparts[i], two.mparts[j]) and _same(a.qparts[i], two.qparts[j])
        assert _same(a.states[i], two.states[j])
    zero9, zero3 = torch.zeros((9, 5, 4), dtype=torch.float64, device=DEV), torch.zeros((3, 5, 4), dtype=torch.float64, device=DEV)
    assert _same(a.mparts[0], zero9) and _same(a.qparts[0], zero3)            # exact +0.0 over the NaN pre-fill
    assert bool(torch.isnan(a.states[0]).all())                               # B == 0: the finishing call wrote nothing
    one = _sharded((1, 4, 4), (0, 1))
    c1 = _case((1, 4, 4))
    assert _same(one.out, c1.out) and _same(one.state, c1.state) and _same(one.gn, c1.gn) and _same(one.gn2, c1.gn2)


# ---- 5. repeatability -------------------------------------------------------------------------------------------------------------------
def test_same_buffers_twice_same_bits(sharded):
    c, s = sharded
    for i in s.live:
        out, state = solve_shade(s.mstack, s.ts[i], s.shapes[i])
        gr = backward_apply(s.gs[i], s.ts[i], s.states[i], s.qstack, s.shapes[i])
        assert _same(out, s.outs[i]) and _same(state, s.states[i])
        assert all(_same(x, y) for x, y in zip(gr, s.grads[i]))
    for i in range(len(s.sizes)):
        assert _same(moments(s.ts[i], s.shapes[i]), s.mparts[i]) and _same(backward_q(s.gs[i], s.ts[i], s.shapes[i]), s.qparts[i])


@pytest.mark.parametrize("H,W", [(70, 9), (1, 630)])
def test_bits_do_not_depend_on_the_image_shape(H, W):
    c = _case((64, 9, 70))
    ref = _sharded(c.shape, (40, 24))
    s = Sharded(c, (40, 24), hw=(H, W))                                       # the same memory read as [n,H,W,c]
    assert _same(s.mstack.reshape(2, 9, -1), ref.mstack.reshape(2, 9, -1)) and _same(s.qstack.reshape(2, 3, -1), ref.qstack.reshape(2, 3, -1))
    assert _same(s.out.reshape(-1), ref.out.reshape(-1)) and _same(s.state.reshape(10, -1), ref.state.reshape(10, -1))
    for a, b in ((s.gn, ref.gn), (s.gn2, ref.gn2), (s.ga2, ref.ga2)):
        assert _same(a.reshape(-1), b.reshape(-1))


# ---- 6. a NaN stays in its pixel --------------------------------------------------------------------------------------------------------
def test_nan_in_one_normal_stays_in_its_pixel():
    c = _case((64, 9, 70))
    ref = _sharded(c.shape, (40, 24))
    B, H, W = c.shape
    y, x, b = 1, 30, 37                                                       # pixel 100: the second workgroup; a face of part 0
    n = c.t["normal"].clone()
    n[b, y, x, 1] = NAN
    s = Sharded(c, (40, 24), t=dict(c.t, normal=n))
    keep = torch.ones((H, W), dtype=torch.bool, device=DEV)
    keep[y, x] = False
    for i in range(2):
        assert bool(torch.isnan(s.outs[i][:, y, x]).all()) and bool(torch.isnan(s.states[i][:9, y, x]).all()), i
        assert _same(s.outs[i][:, keep], ref.outs[i][:, keep]) and _same(s.states[i][:, keep], ref.states[i][:, keep]), i


# ---- 7. the operator --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sizes,me", [((6, 5, 4), (3, 3), 0), ((6, 5, 4), (0, 2, 4), 0), ((64, 9, 70), (17, 17, 17, 13), 2),
                                            ((65, 3, 67), (64, 1), 1)], ids=lambda v: str(v).replace(" ", ""))
def test_operator_and_its_autograd(shape, sizes, me):
    o = pkg("rendering_layer.ops")
    c, s = _case(shape), _sharded(shape, sizes)
    t, g = s.ts[me], s.gs[me]
    calls = []

    def exchange(local):                                                      # the local planes among the other ranks' parts
        k = int(local.shape[0])
        calls.append(k)
        assert tuple(local.shape) == (k,) + tuple(c.shape[1:]) and local.dtype == torch.float64 and k in (9, 3)
        stack = (s.mstack if k == 9 else s.qstack).clone()
        assert _same(local, stack[me])                                        # what this rank contributes IS its C-ABI part
        stack[me] = local
        return stack

    n = t["normal"].clone().requires_grad_(True)
    n2 = t["normal_new"].clone().requires_grad_(True)
    a2 = t["abedo_new"].clone().requires_grad_(True)
    out = o.sfs_intensity_sharded(t["abedo"], n, t["im_gray"], a2, n2, rcond=RS.RCOND, abedo_grad=True, exchange=exchange)
    assert calls == [9] and tuple(out.shape) == (sizes[me],) + tuple(c.shape[1:]) + (1,)
    out.backward(g)
    assert calls == [9, 3]
    if sizes[me]:
        assert _same(out, s.outs[me])
        assert _same(n.grad, s.grads[me][0]) and _same(n2.grad, s.grads[me][1]) and _same(a2.grad, s.grads[me][2])
    # normal needs no gradient: no collective in the backward
    del calls[:]
    n2b = t["normal_new"].clone().requires_grad_(True)
    outb = o.sfs_intensity_sharded(t["abedo"], t["normal"], t["im_gray"], t["abedo_new"], n2b, rcond=RS.RCOND, exchange=exchange)
    outb.backward(g)
    assert calls == [9]
    if sizes[me]:
        assert _same(outb, s.outs[me]) and _same(n2b.grad, s.grads[me][1])


def test_operator_one_tensor_twice_refusals_and_no_group():
    o = pkg("rendering_layer.ops")
    c = _case((6, 5, 4))
    alias = dict(c.t, normal_new=c.t["normal"])
    s = Sharded(c, (3, 3), t=alias)                                           # the C-ABI composition with normal_new = normal
    t, g, me = s.ts[1], s.gs[1], 1

    def exchange(local):
        stack = (s.mstack if local.shape[0] == 9 else s.qstack).clone()
        stack[me] = local
        return stack
    one = t["normal"].clone().requires_grad_(True)                            # one tensor passed twice: autograd adds the two maps
    out = o.sfs_intensity_sharded(t["abedo"], one, t["im_gray"], t["abedo_new"], one, rcond=RS.RCOND, exchange=exchange)
    out.backward(g)
    assert _same(out, s.outs[me]) and _same(one.grad, s.grads[me][0] + s.grads[me][1])
    # the refusals of sfs_intensity
    t, n, n2 = c.t, c.t["normal"], c.t["normal_new"]
    with pytest.raises(ValueError):
        o.sfs_intensity_sharded(t["abedo"].clone().requires_grad_(True), n, t["im_gray"], t["abedo_new"], n2)
    with pytest.raises(ValueError):
        o.sfs_intensity_sharded(t["abedo"], n, t["im_gray"].clone().requires_grad_(True), t["abedo_new"], n2)
    with pytest.raises(ValueError):                                           # abedo_new only with abedo_grad=True
        o.sfs_intensity_sharded(t["abedo"], n, t["im_gray"], t["abedo_new"].clone().requires_grad_(True), n2)
    with pytest.raises(RuntimeError):
        o.sfs_intensity_sharded(t["abedo"].cpu(), n, t["im_gray"], t["abedo_new"], n2)
    with pytest.raises(TypeError):
        o.sfs_intensity_sharded(t["abedo"].double(), n, t["im_gray"], t["abedo_new"], n2)
    with pytest.raises(ValueError):                                           # an exchange that returns the wrong thing
        o.sfs_intensity_sharded(t["abedo"], n, t["im_gray"], t["abedo_new"], n2, exchange=lambda local: local)
    # no group, no exchange: sfs_intensity, bit for bit
    assert not torch.distributed.is_initialized()
    for shape in RS.CASES:
        cc = _case(shape)
        res = []
        for f in (o.sfs_intensity_sharded, o.sfs_intensity):
            nn = cc.t["normal"].clone().requires_grad_(True)
            nn2 = cc.t["normal_new"].clone().requires_grad_(True)
            aa2 = cc.t["abedo_new"].clone().requires_grad_(True)
            I = f(cc.t["abedo"], nn, cc.t["im_gray"], aa2, nn2, rcond=RS.RCOND, abedo_grad=True)
            I.backward(cc.gt)
            res.append((I, nn.grad, nn2.grad, aa2.grad))
        assert all(_same(x, y) for x, y in zip(*res)), shape
        assert _same(res[0][0], cc.out) and _same(res[0][1], cc.gn) and _same(res[0][2], cc.gn2) and _same(res[0][3], cc.ga2)


# ---- 8. two processes, one GPU, gloo over loopback --------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_processes_one_gpu(tmp_path):
    c = _case((6, 5, 4))
    s = _sharded(c.shape, (3, 3))
    port = _free_port()
    child = os.path.join(ROOT, "tests", "sfs_sharded_child.py")
    base = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [child]
    outs = [str(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    procs = []
    try:
        for r in range(2):                                                    # fresh children; each ends itself after 150 s at the most
            procs.append(subprocess.Popen(["timeout", "-k", "10", "150"] + base + [str(r), "2", str(port), outs[r]], cwd=ROOT,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        logs = [p.communicate(timeout=200)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d exited with %s:\n%s" % (r, p.returncode, logs[r][-3000:])
    got = [np.load(f) for f in outs]
    for r in range(2):
        # the composition of test 3 for sharding (3, 3), bit for bit
        for key, want in (("sharded_intensity", s.outs[r]), ("sharded_gn", s.grads[r][0]), ("sharded_gn2", s.grads[r][1])):
            assert _same(torch.as_tensor(got[r][key]), want.cpu()), (r, key)
        # flag off: the torch route, untouched
        for key in ("intensity", "gn", "gn2"):
            assert _same(torch.as_tensor(got[r]["default_" + key]), torch.as_tensor(got[r]["torch_" + key])), (r, key)
    # ... and inside the bounds against the whole-batch model
    cat = [torch.as_tensor(np.concatenate([got[0][k], got[1][k]])).to(DEV) for k in ("sharded_intensity", "sharded_gn", "sharded_gn2")]
    _check_forward(c, cat[0], s.state)
    _check_backward(c, cat[1], cat[2], s.ga2)


# ---- 9. the objective ---------------------------------------------------------------------------------------------------------------------
def test_get_loss_flag(small_assets):
    netm, L = pkg("nets.network"), pkg("nets.losses")
    A = small_assets
    B, S = 4, 40
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S)
    rs = np.random.RandomState(3)                                             # the recipe of test_sfs_gpu.py::test_get_loss_flags
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
    assert not torch.distributed.is_initialized()
    kw = dict(gather_sfs=True, sfs_fused=True, sfs_normal_grad=True, sfs_rcond=1e-6)
    off = L.get_loss(net, pred, label, im, V, coarse, fine, **kw)
    on = L.get_loss(net, pred, label, im, V, coarse, fine, sfs_fused_gather=True, **kw)
    assert set(on) == set(off) and len(on) == 6
    for k in off:
        print("%s: %r / %r" % (k, float(off[k].detach()), float(on[k].detach())))
        assert _same(off[k], on[k]), k
    g_off = torch.autograd.grad(off["total_loss"], pred, retain_graph=True)[0]   # (the two losses share the graph of V and coarse)
    g_on = torch.autograd.grad(on["total_loss"], pred, retain_graph=True)[0]
    print("max |d total / d pred| %.3g" % float(g_on.abs().max()))
    assert _same(g_off, g_on) and bool(torch.isfinite(g_on).all()) and float(g_on[:, 7:].abs().max()) > 0
    with pytest.raises(ValueError):
        L.get_loss(net, pred, label, im, V, coarse, fine, sfs_fused_gather=True, sfs_fused=True)
