"""GPU: the landmark term (fr_landmark_basis_build / _forward / _backward; include/fr_hotpath.h, "landmarks") against its numpy model
tests/ref_landmark.py -- the image, the points and the sse bit for bit; the gradient bit for bit outside the angle columns, which may
see a last-place difference of the device's double sincos -- then the Python surface against the dense route, SynthBatches, get_loss
and the example as a program.

Bounds.  u = 2^-24.
  * forward against the dense decode: (n_shape + n_exp + 8) u A per coordinate, A the sum of the absolute values of that coordinate's
    terms (the model's `absterms`): the a-priori bound of any fp32 chain of that length.
  * angle columns against the model: u |g| + 2^-40 S, S the sum of the absolute terms (the model's `angle_S`).
  * gradient against the dense route: the sum of (a) the dense route's own stated bounds -- tests/test_decode_backward_bounds_gpu.py
    for columns 3.., tests/ref_pose_backward.py::PoseRef.bound for the angles, each around the float64 gradient of the vertex
    gradient that actually reached the dense node --, (b) this route's u |g| + 2^-40 S around the model, and (c) what separates the
    two float64 gradients: the dense loss differentiates the dense forward's fp32 points, which stand within the forward bound E of
    the model's, so the point gradients differ by at most 2 |s| E + u |g| (s = the loss's factor w / (B max(sum w, 1))), carried to
    every output through the absolute values of the backward's own coefficients."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
from gpu_util import assert_bits_equal
import ref_landmark as RL
import ref_pose_backward as RP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
IM = 200.0


def _h():
    return pkg("_lib")


def _t(a, dtype=np.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype), device=DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def c_build(mu, pcs, pce, idx, N, ns, ne, img=None):
    h, L = _h(), _h().lib()
    K = len(idx)
    nb = L.fr_landmark_basis_bytes(K, ns, ne)
    assert nb == 4 * 3 * K * (2 * (ns + ne) + 1)
    if img is None:
        img = torch.full((nb // 4,), 7.0, dtype=torch.float32, device=DEV)
    assert img.dtype == torch.float32 and img.numel() * 4 == nb
    rc = L.fr_landmark_basis_build(h.ptr(mu), h.ptr(pcs), h.ptr(pce), h.ptr(_t(idx, np.int32)), N, ns, ne, K, h.ptr(img), nb, _stream())
    assert rc == 0, rc
    return img


def c_forward(c, P, R=None, target=None, weight=None):
    h, L = _h(), _h().lib()
    B, K = int(P.shape[0]), c["K"]
    points = torch.full((B, 3, K), 7.0, dtype=torch.float32, device=DEV)
    sse = torch.full((B,), 7.0, dtype=torch.float64, device=DEV)
    wb = 1 if weight is not None and weight.dim() == 2 else 0
    rc = L.fr_landmark_forward(h.ptr(P), h.ptr(c["img"]), c["img"].numel() * 4, h.ptr(R), h.ptr(target), h.ptr(weight), wb, B, K,
                               c["ns"], c["ne"], IM, h.ptr(points), h.ptr(sse), _stream())
    assert rc == 0, rc
    return points, sse


def c_backward(c, P, gp=None, gs=None, R=None, target=None, weight=None, pose_grad=1, fill=7.0):
    h, L = _h(), _h().lib()
    B, K = int(P.shape[0]), c["K"]
    out = torch.full((B, 7 + c["ns"] + c["ne"]), fill, dtype=torch.float32, device=DEV)
    gR = torch.full((B, 3, 3), fill, dtype=torch.float32, device=DEV)
    wb = 1 if weight is not None and weight.dim() == 2 else 0
    rc = L.fr_landmark_backward(h.ptr(gp), h.ptr(gs), h.ptr(P), h.ptr(c["img"]), c["img"].numel() * 4, h.ptr(R), h.ptr(target),
                                h.ptr(weight), wb, B, K, c["ns"], c["ne"], IM, h.ptr(out), h.ptr(gR), pose_grad, _stream())
    assert rc == 0, rc
    return out, gR


# ---- the cases: inputs and the model's image, built once ---------------------------------------------------------------------------------------
CASES = [("small", 1, 1), ("small", 3, 3), ("small", 65, 68), ("full", 3, 68), ("full", 65, 300), ("one", 3, 300), ("one", 1, 3)]
_ASSETS, _CASES = {}, {}


def _assets(kind):
    if kind not in _ASSETS:
        synth = pkg("utils.synth")
        ns, ne = {"small": (9, 5), "full": (199, 29), "one": (1, 1)}[kind]
        _ASSETS[kind] = synth.make_small_assets(n_shape=ns, n_exp=ne)
    return _ASSETS[kind]


def _ids(N, K, rs):
    """K ids that include 0, N - 1 and a duplicate where K allows"""
    idx = rs.randint(0, N, K)
    fixed = [0, N - 1, 17, 17][:K]
    idx[:len(fixed)] = fixed
    return idx.astype(np.int64)


def _case(kind, B, K):
    key = (kind, B, K)
    if key not in _CASES:
        A = _assets(kind)
        rs = np.random.RandomState(100 + 7 * B + K)
        ns, ne = A["ndim_shape"], A["ndim_exp"]
        N = np.asarray(A["mu"]).size // 3
        idx = _ids(N, K, rs)
        mu, pcs, pce = _t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"])
        img_np = RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], idx)
        mean, Um = RL.split_image(img_np, K, ns + ne)
        P = pkg("utils.synth").sample_params_batch(B, im_size=200, n_shape=ns, n_exp=ne, seed=50 + B).astype(np.float32)
        P[:, 5] = rs.uniform(-1, 1, B)
        if B > 1:
            P[B // 2, 6] = 0.0                                   # a face with f = 0
        R = RP.rotations(rs, B)
        fw = RL.Forward(P, mean, Um)
        target = (fw.points[:, 0:2].transpose(0, 2, 1) + rs.uniform(-3, 3, (B, K, 2))).astype(np.float32)
        wBK = rs.uniform(0.25, 2.0, (B, K)).astype(np.float32)
        wK = rs.uniform(0.25, 2.0, K).astype(np.float32)
        wBK[B - 1, K - 1] = 0.0
        wK[0] = 0.0
        nan_t = target.copy()
        nan_t[B - 1, K - 1] = np.nan                             # missing landmarks: weight 0 under a NaN target
        nan_k = target.copy()
        nan_k[:, 0] = np.nan
        gpts = (rs.standard_normal((B, 3, K)) * np.exp(rs.uniform(-3, 3, (B, 3, K)))).astype(np.float32)
        gsse = rs.uniform(0.5, 2.0, B) * np.where(rs.rand(B) < 0.3, -1.0, 1.0)
        _CASES[key] = dict(A=A, N=N, K=K, B=B, ns=ns, ne=ne, idx=idx, mu=mu, pcs=pcs, pce=pce, img_np=img_np, mean=mean, Um=Um, P=P, R=R,
                           target=target, wBK=wBK, wK=wK, nan_t=nan_t, nan_k=nan_k, gpts=gpts, gsse=gsse,
                           img=c_build(mu, pcs, pce, idx, N, ns, ne))
    return _CASES[key]


IDS = ["%s-B%d-K%d" % c for c in CASES]


@pytest.mark.parametrize("kind,B,K", CASES, ids=IDS)
def test_basis_image(kind, B, K):
    c = _case(kind, B, K)
    torch.cuda.synchronize()
    assert_bits_equal(c["img"].cpu().numpy(), c["img_np"], "image")


def test_out_of_range_id_at_the_c_level():
    c = _case("small", 3, 3)
    idx = np.array([5, c["N"], -1, 0, c["N"] - 1], np.int64)
    img = c_build(c["mu"], c["pcs"], c["pce"], idx, c["N"], c["ns"], c["ne"])
    torch.cuda.synchronize()
    want = RL.basis_image(c["A"]["mu"], c["A"]["pc_shape"], c["A"]["pc_exp"], idx)
    assert_bits_equal(img.cpu().numpy(), want, "image with ids outside [0, N)")
    mean, Um = RL.split_image(want, 5, c["ns"] + c["ne"])
    assert not mean[1:3].any() and not Um[1:3].any() and Um[0].any() and Um[4].any()
    # ... and such a landmark projects to t3d: v = +0
    cc = dict(c, K=5, img=img)
    P = _t(c["P"])
    points, _ = c_forward(cc, P)
    torch.cuda.synchronize()
    assert_bits_equal(points.cpu().numpy(), RL.Forward(c["P"], mean, Um).points, "points")
    # the Python layer refuses such ids before any launch
    ops = pkg("rendering_layer.ops")
    for bad in ([0, c["N"]], [-1]):
        with pytest.raises(ValueError):
            ops.landmark_basis(c["mu"], c["pcs"], c["pce"], bad)


def _forward_variants(c):
    """(name, R, target, weight) of every forward the case runs"""
    return [("rotation, no target", None, None, None), ("override, no target", c["R"], None, None),
            ("rotation, NULL weight", None, c["target"], None), ("override, [K] weight, NaN", c["R"], c["nan_k"], c["wK"]),
            ("rotation, [B,K] weight, NaN", None, c["nan_t"], c["wBK"])]


@pytest.mark.parametrize("kind,B,K", CASES, ids=IDS)
def test_forward_bit_for_bit(kind, B, K):
    c = _case(kind, B, K)
    P = _t(c["P"])
    for name, R, target, weight in _forward_variants(c):
        points, sse = c_forward(c, P, _t(R), _t(target), _t(weight))
        torch.cuda.synchronize()
        fw = RL.Forward(c["P"], c["mean"], c["Um"], R=R, target=target, weight=weight)
        assert_bits_equal(points.cpu().numpy(), fw.points, name)
        if target is None:
            assert bool((sse == 7.0).all()), name                       # ignored without a target
        else:
            got = sse.cpu().numpy()
            assert np.isfinite(got).all() and np.array_equal(_bits64(got), _bits64(fw.sse)), (name, got, fw.sse)
    if B > 1:   # f = 0: the face's landmarks are t3d, exactly
        b = B // 2
        fw = RL.Forward(c["P"], c["mean"], c["Um"])
        assert (fw.points[b, 0] == c["P"][b, 3]).all() and (fw.points[b, 2] == c["P"][b, 5]).all()


def _check_backward(c, name, got, gotR, bw, fw, pose_grad, fill=7.0):
    got, gotR = got.cpu().numpy(), gotR.cpu().numpy()
    assert_bits_equal(got[:, 3:], bw.grad_params[:, 3:], name + ": t3d, f, coefficients")
    if pose_grad and fw.override:
        assert_bits_equal(gotR, bw.grad_R, name + ": grad_R")
    else:
        assert (gotR == fill).all(), name                                     # untouched
    if pose_grad and not fw.override:
        want = bw.params64[:, 0:3]
        bound = U * np.abs(want) + 2.0 ** -40 * bw.angle_S
        err = np.abs(got[:, 0:3].astype(np.float64) - want)
        assert (err <= bound).all(), (name, err.max(), np.argwhere(err > bound)[:3])
        return float((err / np.where(bound > 0, bound, 1.0)).max()), float((got[:, 0:3] == bw.grad_params[:, 0:3]).mean())
    assert_bits_equal(got[:, 0:3], np.zeros((got.shape[0], 3), np.float32), name + ": angle columns +0")
    return 0.0, 1.0


@pytest.mark.parametrize("kind,B,K", CASES, ids=IDS)
def test_backward_against_the_model(kind, B, K):
    c = _case(kind, B, K)
    P = _t(c["P"])
    worst, same = 0.0, 1.0
    runs = [("points alone", c["gpts"], None, None, None, None), ("sse alone", None, c["gsse"], None, c["nan_t"], c["wBK"]),
            ("both", c["gpts"], c["gsse"], None, c["nan_k"], c["wK"]), ("both, override", c["gpts"], c["gsse"], c["R"], c["target"], None),
            ("points alone, override", c["gpts"], None, c["R"], None, None)]
    for name, gp, gs, R, target, weight in runs:
        fw = RL.Forward(c["P"], c["mean"], c["Um"], R=R, target=target, weight=weight)
        for pose_grad in (1, 0):
            bw = RL.Backward(fw, c["Um"], grad_points=gp, grad_sse=gs, pose_grad=bool(pose_grad))
            args = (c, P, _t(gp), _t(gs, np.float64), _t(R), _t(target), _t(weight), pose_grad)
            got, gotR = c_backward(*args)
            again, againR = c_backward(*args)
            torch.cuda.synchronize()
            assert np.isfinite(got.cpu().numpy()).all(), name
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(gotR.view(torch.int32), againR.view(torch.int32))
            r, s = _check_backward(c, "%s, pose_grad %d" % (name, pose_grad), got, gotR, bw, fw, pose_grad)
            worst, same = max(worst, r), min(same, s)
    print("%s B %d K %d: angle columns worst err / bound %.3g, share equal to the model's bits %.3f" % (kind, B, K, worst, same))


def _exact_case():
    """hand-made assets on which every value of the forward is exact in fp32: integer basis and mean, coefficients that are
    multiples of 1/4, a signed permutation as R, f a power of two, t3d multiples of 1/8 -- so the points ARE the float64 x, y"""
    rs = np.random.RandomState(3)
    N, ns, ne, K, B = 40, 3, 2, 7, 3
    mu = rs.randint(-50, 50, 3 * N).astype(np.float32)
    pcs = rs.randint(-8, 8, (3 * N, ns)).astype(np.float32)
    pce = rs.randint(-8, 8, (3 * N, ne)).astype(np.float32)
    idx = np.array([0, N - 1, 5, 5, 9, 20, 31], np.int64)
    P = np.zeros((B, 7 + ns + ne), np.float32)
    P[:, 3:6] = rs.randint(0, 800, (B, 3)) / 8.0
    P[:, 6] = [0.5, 0.25, 2.0]
    P[:, 7:] = rs.randint(-20, 20, (B, ns + ne)) / 4.0
    R = np.zeros((B, 3, 3), np.float32)
    for b, perm in enumerate(([0, 1, 2], [2, 0, 1], [1, 0, 2])):
        for i, j in enumerate(perm):
            R[b, i, j] = 1.0 if (i + b) % 2 else -1.0
    return dict(N=N, ns=ns, ne=ne, K=K, B=B, mu=mu, pcs=pcs, pce=pce, idx=idx, P=P, R=R)


def test_exact_zero():
    """target taken from the same forward's points: sse is +0 and every gradient exactly 0.  The sse compares x and y BEFORE their
    rounding to fp32, so the statement holds where that rounding is exact; the case is built so (see _exact_case), and the test
    asserts that it is."""
    e = _exact_case()
    c = dict(K=e["K"], ns=e["ns"], ne=e["ne"], img=c_build(_t(e["mu"]), _t(e["pcs"]), _t(e["pce"]), e["idx"], e["N"], e["ns"], e["ne"]))
    mean, Um = RL.split_image(RL.basis_image(e["mu"], e["pcs"], e["pce"], e["idx"]), e["K"], e["ns"] + e["ne"])
    P, R = _t(e["P"]), _t(e["R"])
    points, _ = c_forward(c, P, R)
    torch.cuda.synchronize()
    fw = RL.Forward(e["P"], mean, Um, R=e["R"])
    assert np.array_equal(fw.points.astype(np.float64).transpose(0, 2, 1), fw.xyz)          # the rounding is exact here
    assert_bits_equal(points.cpu().numpy(), fw.points, "points")
    target = points[:, 0:2].transpose(1, 2).contiguous()
    _, sse = c_forward(c, P, R, target)
    gs = torch.ones((e["B"],), dtype=torch.float64, device=DEV)
    for pose_grad, Rv in ((1, R), (0, R)):
        got, gotR = c_backward(c, P, None, gs, Rv, target, None, pose_grad)
        torch.cuda.synchronize()
        assert np.array_equal(_bits64(sse.cpu().numpy()), _bits64(np.zeros(e["B"])))        # +0, not -0
        assert not got.cpu().numpy().any()
        assert not gotR.cpu().numpy().any() if pose_grad else bool((gotR == 7.0).all())
    # all weights zero: the same, whatever the target
    w0 = torch.zeros((e["K"],), dtype=torch.float32, device=DEV)
    far = torch.full_like(target, float("nan"))
    _, sse0 = c_forward(c, P, None, far, w0)
    got0, _ = c_backward(c, P, None, gs, None, far, w0, 1)
    torch.cuda.synchronize()
    assert np.array_equal(_bits64(sse0.cpu().numpy()), _bits64(np.zeros(e["B"]))) and not got0.cpu().numpy().any()


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def face():
    A = _assets("small")
    return pkg("nets.network").FaceRecNet(mesh_data=A, batch_size=3, im_size=200, device=DEV)


def _abs_coefficients(fw, Um, dg):
    """what a change of the point gradients of at most dg [B,K,3] (on x, y, z) can move each output by: the backward over absolute
    values -> [B, 7 + Kt] (angle columns through |dR / d angle|)"""
    B, K, Kt = fw.v.shape[0], fw.v.shape[1], Um.shape[2]
    out = np.zeros((B, 7 + Kt))
    Ra, fa = np.abs(fw.R), np.abs(fw.f)
    out[:, 3:6] = dg.sum(axis=1)
    out[:, 6] = (dg * np.abs(fw.Rv)).sum(axis=(1, 2))
    rt = np.einsum("bic,bki->bkc", Ra, dg)
    out[:, 7:] = fa[:, None] * np.einsum("bkc,kcj->bj", rt, np.abs(Um))
    Ga = fa[:, None, None] * np.einsum("bki,bkj->bij", dg, np.abs(fw.v))
    _, dRabs = RL.rotation_derivatives(fw.P[:, 0:3])
    for a in range(3):
        out[:, a] = (Ga * dRabs[a]).sum(axis=(1, 2))
    return out


def test_python_surface_against_the_dense_route(face, oracle):
    import test_decode_backward_bounds_gpu as DB
    ops, losses = pkg("rendering_layer.ops"), pkg("nets.losses")
    c = _case("small", 3, 68)
    A, idx, B, K = c["A"], c["idx"], 3, 68
    Kt = c["ns"] + c["ne"]
    P32 = c["P"].copy()
    P32[1, 6] = 7e-4                                                   # (the case's face with f = 0 has no direction to compare)
    fw = RL.Forward(P32, c["mean"], c["Um"], target=c["target"], weight=c["wBK"])
    # forward
    p = _t(P32).requires_grad_(True)
    pts = face.landmarks(p, idx)
    V = face.vertices_transform(_t(P32))
    torch.cuda.synchronize()
    assert_bits_equal(pts.detach().cpu().numpy(), fw.points, "face.landmarks against the model")
    E = (Kt + 8) * U * fw.absterms                                     # [B,3,K]
    ratio = np.abs(pts.detach().cpu().numpy().astype(np.float64) - V[:, :, torch.as_tensor(idx, device=DEV)].cpu().numpy()) / E
    print("landmarks against the dense decode at idx: max |difference| / bound = %.3g" % ratio.max())
    assert (ratio <= 1.0).all()
    assert face.landmark_basis(idx) is face.landmark_basis(list(idx)) and len(face._landmark_bases) >= 1
    with pytest.raises(ValueError):
        face.landmark_basis([0, face.nvert])
    # the autograd node from grad_points: the C call's bits
    w = _t(c["gpts"])
    (pts * w).sum().backward()
    want, _ = c_backward(c, _t(P32), w, None, None, None, None, 0)
    torch.cuda.synchronize()
    assert torch.equal(p.grad.view(torch.int32), want.view(torch.int32)) and bool((p.grad[:, 0:3] == 0).all())
    with pytest.raises(ValueError):
        ops.landmark_sse(_t(P32), face.landmark_basis(idx), _t(c["target"]).requires_grad_(True))
    with pytest.raises(ValueError):
        ops.landmark_sse(_t(P32), face.landmark_basis(idx), _t(c["target"]), weight=_t(c["wK"]).requires_grad_(True))
    # R as a leaf: its gradient flows with pose_grad, the angle columns stay 0
    Rl = _t(c["R"]).requires_grad_(True)
    p3 = _t(P32).requires_grad_(True)
    ops.landmark_sse(p3, face.landmark_basis(idx), _t(c["target"]), R=Rl, im_size=200, pose_grad=True).sum().backward()
    bwR = RL.Backward(RL.Forward(P32, c["mean"], c["Um"], R=c["R"], target=c["target"]), c["Um"], grad_sse=np.ones(B), pose_grad=True)
    torch.cuda.synchronize()
    assert_bits_equal(Rl.grad.cpu().numpy(), bwR.grad_R, "R.grad")
    assert_bits_equal(p3.grad.cpu().numpy(), bwR.grad_params, "params.grad under an override")

    # landmark_loss against the same loss through the dense route
    target, weight = _t(c["target"]), _t(c["wBK"])
    p1 = _t(P32).requires_grad_(True)
    L1 = losses.landmark_loss(face, p1, idx, target, weight)
    L1.backward()
    p2 = _t(P32).requires_grad_(True)
    V2 = face.vertices_transform(p2, pose_grad=True)
    V2.retain_grad()
    xy = V2[:, 0:2, torch.as_tensor(idx, device=DEV)].transpose(1, 2).double()
    wsum = weight.double().sum(dim=1).clamp_min(1.0)
    L2 = ((weight.double() * ((xy - target.double()) ** 2).sum(dim=2)).sum(dim=1) / wsum).mean()
    L2.backward()
    torch.cuda.synchronize()
    s = c["wBK"].astype(np.float64) / (B * np.maximum(c["wBK"].astype(np.float64).sum(axis=1), 1.0))[:, None]      # [B,K]
    L1v, L2v = float(L1.detach()), float(L2.detach())
    assert abs(L1v - RL.landmark_loss(fw.sse, c["wBK"], B, K)) <= 1e-14 * abs(L1v)
    assert abs(L1v - L2v) <= 4 * float((s[:, :, None] * (np.abs(fw.xyz[:, :, 0:2] - fw.target) + E.transpose(0, 2, 1)[:, :, 0:2])
                                                    * E.transpose(0, 2, 1)[:, :, 0:2]).sum())
    g1, g2 = p1.grad.cpu().numpy().astype(np.float64), p2.grad.cpu().numpy().astype(np.float64)
    # (b) this route around the model
    bw = RL.Backward(fw, c["Um"], grad_sse=np.full(B, 1.0 / B) / wsum.cpu().numpy(), pose_grad=True)   # (autograd's own factor)
    b_lm = U * np.abs(bw.params64)
    b_lm[:, 0:3] += 2.0 ** -40 * bw.angle_S
    assert (np.abs(g1 - bw.params64) <= b_lm * 1.01 + 1e-300).all()
    # (a) the dense route around the float64 gradient of the vertex gradient that reached it
    G = V2.grad.cpu().numpy()
    Vg = V2.detach().cpu().numpy()

    class Rig:
        N, ns, ne = c["N"], c["ns"], c["ne"]
    ref = DB.Ref(oracle, A, P32, G)
    D = DB._depths("packed", Rig, B)
    b_dense = np.zeros_like(g2)
    b_dense[:, 3:6] = DB._gamma(D["t3d"]) * ref.S[:, 3:6]
    E1 = ref.e1(Vg)
    b_dense[:, 6] = E1 * 1.01 + DB._gamma(D["f"]) * (ref.S[:, 6] + E1)
    b_dense[:, 7:] = DB._gamma(D["coef"] + 5) * ref.Sw
    geom = (ctypes.c_int * 4)()
    _h().lib().fr_debug_pose_bwd_geom(1, c["N"], geom)
    pref = RP.PoseRef(oracle, G, RP.unprojected_f64(A, P32), P32, im_size=IM)
    b_dense[:, 0:3] = pref.bound(Vg, geom[3])[1]
    want_dense = ref.want.copy()
    want_dense[:, 0:3] = pref.angles
    assert (np.abs(g2 - want_dense) <= b_dense).all()
    # (c) what separates the two float64 gradients
    gk = np.zeros((B, K, 3))
    gk[:, :, 0:2] = 2 * s[:, :, None] * np.abs(fw.xyz[:, :, 0:2] - fw.target)
    dg = np.zeros((B, K, 3))
    dg[:, :, 0:2] = 2 * s[:, :, None] * E.transpose(0, 2, 1)[:, :, 0:2] + U * gk[:, :, 0:2]
    # (duplicate ids: index_select's backward adds their fp32 gradients in one more rounded sum each)
    dg += U * gk
    b_sep = 1.01 * _abs_coefficients(fw, c["Um"], dg)
    bound = b_lm * 1.01 + b_dense + b_sep
    err = np.abs(g1 - g2)
    ratio = err / np.where(bound > 0, bound, 1.0)
    scale = np.abs(bw.params64).max(axis=0)
    print("landmark_loss against the dense route: max |difference| / bound = %.3g; bound / max|g| per column at most %.3g" % (
        ratio.max(), (bound.max(axis=0) / np.where(scale > 0, scale, 1.0)).max()))
    assert (err <= bound).all(), (np.argwhere(err > bound)[:4], ratio.max())
    print("bound / max|g| per column, angles, t3d, f: %s" % np.array2string((bound.max(axis=0) / np.where(scale > 0, scale, 1.0))[:7], precision=2))
    assert np.abs(g1[:, 0:3]).min() > 0 and (bound.max(axis=0) <= 5e-2 * scale)[[3, 4]].all()   # (the check discriminates)
    # pose_grad=False: the angle columns are +0, the others the same bits
    p4 = _t(P32).requires_grad_(True)
    losses.landmark_loss(face, p4, idx, target, weight, pose_grad=False).backward()
    assert bool((p4.grad[:, 0:3] == 0).all()) and torch.equal(p4.grad[:, 3:].contiguous().view(torch.int32),
                                                              p1.grad[:, 3:].contiguous().view(torch.int32))


def test_synth_batches_landmarks(face):
    pipe, synth = pkg("pipeline"), pkg("utils.synth")
    idx = synth.landmark_ids(_assets("small"), 68)
    plain = pipe.SynthBatches(face, 3, 11, slots=1)
    with_lm = pipe.SynthBatches(face, 3, 11, slots=1, landmarks=idx)
    for _ in range(2):
        a, b = plain.next(), with_lm.next()
        torch.cuda.synchronize()
        assert sorted(b) == sorted(list(a) + ["landmarks", "landmark_visible"])
        for k in a:     # without the argument: today's stream, tensor for tensor
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        assert tuple(b["landmarks"].shape) == (3, 68, 2) and tuple(b["landmark_visible"].shape) == (3, 68)
        want = face.landmarks(b["params"], idx)[:, 0:2].transpose(1, 2).contiguous()
        assert torch.equal(b["landmarks"].view(torch.int32), want.view(torch.int32))
        vis = pkg("rendering_layer.ops").mesh_visible(face.tri, b["tri_ind"], face.nvert)
        assert torch.equal(b["landmark_visible"], vis[:, torch.as_tensor(idx, device=DEV)].float())
        assert set(np.unique(b["landmark_visible"].cpu().numpy()).tolist()) <= {0.0, 1.0} and float(b["landmark_visible"].sum()) > 0
        assert not b["landmarks"].requires_grad
    assert "landmarks" not in a


def test_get_loss_term(face):
    losses, pipe, synth = pkg("nets.losses"), pkg("pipeline"), pkg("utils.synth")
    idx = synth.landmark_ids(_assets("small"), 68)
    b = pipe.SynthBatches(face, 3, 13, slots=1, landmarks=idx).next()
    torch.cuda.synchronize()
    label = b["params"]
    g = torch.Generator(device="cpu").manual_seed(5)
    pred = (label + torch.randn(label.shape, generator=g).to(DEV) * label.abs() * 0.01).requires_grad_(True)
    ver = face.vertices_transform(pred)
    args = (face, pred, label, b["im_gray"], ver, b["depth"], b["depth"] * 1.01)
    base = losses.get_loss(*args)
    none = losses.get_loss(*args, landmark_target=None, landmark_idx=None)
    assert list(base) == list(none) and "landmark_loss" not in base
    for k in base:
        assert torch.equal(base[k].detach().reshape(-1).view(torch.int32 if base[k].dtype == torch.float32 else torch.int64),
                           none[k].detach().reshape(-1).view(torch.int32 if none[k].dtype == torch.float32 else torch.int64)), k
    with pytest.raises(ValueError):
        losses.get_loss(*args, landmark_target=b["landmarks"])
    lam = 0.25
    full = losses.get_loss(*args, landmark_target=b["landmarks"], landmark_idx=idx, landmark_weight=b["landmark_visible"],
                           lambda_landmark=lam)
    assert list(full) == list(base) + ["landmark_loss"]
    term = losses.landmark_loss(face, pred, idx, b["landmarks"], b["landmark_visible"])
    assert float(full["landmark_loss"]) == float(term) and float(term) > 0
    want = base["total_loss"] + (lam * term).to(base["total_loss"].dtype)
    assert float(full["total_loss"]) == float(want)
    for k in base:
        if k != "total_loss":
            assert float(full[k]) == float(base[k]), k
    full["total_loss"].backward()
    assert pred.grad is not None and float(pred.grad[:, 0:3].abs().max()) > 0       # the term reaches the angles


# ---- the example as a program ------------------------------------------------------------------------------------------------------------------
def _run(cmd, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[-2000:]
    return json.loads(lines[0])


def _finite(d):
    vals = [d["first"], d["last"]] + list(d["errors_before"].values()) + list(d["errors_after"].values())
    return d["finite"] is True and bool(np.isfinite(vals).all())


def test_photo_fit_landmarks_only_program():
    d = _run([sys.executable, "examples/photo_fit.py", "--small", "--fit-pose", "--landmarks-only", "--landmarks", "68"])
    print(json.dumps(d))
    assert d["landmarks"] == 68 and d["landmarks_only"] is True and _finite(d)
    assert d["last"] < d["first"]
    assert d["errors_after"]["t3d_rms"] < d["errors_before"]["t3d_rms"]


def test_photo_fit_landmarks_program():
    d = _run([sys.executable, "examples/photo_fit.py", "--small", "--fit-pose", "--landmarks", "68"])
    print(json.dumps(d))
    assert d["landmarks"] == 68 and d["landmarks_only"] is False and _finite(d)
    assert d["last"] < d["first"]
