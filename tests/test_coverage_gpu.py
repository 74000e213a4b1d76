"""GPU: fr_coverage_forward / fr_coverage_backward (csrc/fr_coverage.hip) held to their float64 model (tests/ref_coverage.py, pinned
on the CPU by tests/test_coverage_cpu.py), and the opt-in Python surface (ops.soft_coverage, FaceRecNet.soft_mask,
losses.silhouette_loss, examples/photo_fit.py --fit-pose).

forward:   bit for bit.
backward:  |got - S| <= 2^-24 |S| + n_v 2^(shift - 39) M     S the exact sum of the model's fp32 terms, n_v their number, M the
                                                             face's largest |term| -- evaluated in integers
                                                             (ref_normal_backward.check_bound); an element without terms is +0.
The scenes are those of tests/test_depth_interp_gpu.py (the small assets, 480 vertices, placed by its make_scene) and the hand-made
ones of tests/coverage_cases.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coverage_cases as CC
import ref_coverage as RC
import ref_normal_backward as RN
from conftest import ROOT, pkg
from gpu_util import ops, net_mod, assert_bits_equal
from raw_calls import cbwd, cfwd
from test_depth_interp_gpu import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _h():
    return pkg("_lib")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


def geom(B, nver, H, W):
    out = (ctypes.c_int * 6)()
    _h().lib().fr_debug_coverage_bwd_geom(B, nver, H, W, out)
    return dict(zip(("splits", "range", "shift", "chunks", "lds", "xcd"), out))


_SCENES = {}
SHAPES = ((3, 8, 9), (3, 33, 40), (1, 64, 64), (8, 64, 64))                   # (B, H, W): less than one 1,024-pixel chunk; one full
                                                                              # and a ragged one; B = 8 the XCD owner map


def scene(small_assets, B, H, W):
    """make_scene's dict plus the model's plane `cov` (computed once, shared; no test writes to it)"""
    key = (B, H, W)
    if key not in _SCENES:
        sc = make_scene(small_assets, B, H, W, 100 * B + H)
        sc["cov"] = RC.forward(sc["V"], sc["tri"], sc["tind"], H, W)
        _SCENES[key] = sc
    return _SCENES[key]


def _neighbours_share_state(ok):
    """ok [B,H,W] bool -> [B,H,W] bool: every existing 4-neighbour has the pixel's state"""
    pad = np.pad(ok, ((0, 0), (1, 1), (1, 1)), mode="edge")
    return (pad[:, 1:-1, :-2] == ok) & (pad[:, 1:-1, 2:] == ok) & (pad[:, :-2, 1:-1] == ok) & (pad[:, 2:, 1:-1] == ok)


# ---- forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_forward_is_the_model_bit_for_bit(small_assets, B, H, W):
    sc = scene(small_assets, B, H, W)
    assert sc["nver"] == 480
    got = cfwd(_t(sc["V"]), _t(sc["tri"]), _t(sc["tind"]), H, W).cpu().numpy()
    assert_bits_equal(got, sc["cov"], "soft coverage")
    c = got.reshape(B, H, W)
    ok = (sc["tind"] >= 0).reshape(B, H, W)                                   # (the product's forward names no bad id: covered is OK)
    assert ok.any() and not ok.all()
    assert ((c > 0) & (c < 1)).sum() >= 4 * B
    same = _neighbours_share_state(ok)
    assert (same & ok).any() and np.all(c[same & ok].view(np.uint32) == np.float32(1).view(np.uint32))
    assert (same & ~ok).any() and np.all(c[same & ~ok].view(np.uint32) == 0)


# ---- backward --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_backward_within_the_bound_of_the_exact_sums(small_assets, B, H, W):
    sc = scene(small_assets, B, H, W)
    gm = geom(B, 480, H, W)
    assert gm["lds"] <= 160 * 1024 and gm["shift"] == 0 and gm["xcd"] == (1 if B == 8 else 0)
    assert gm["chunks"] == (H * W + 1023) // 1024
    g, cov, V, tri, ti = _t(sc["g"]), _t(sc["cov"]), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"])
    R = RC.model(sc["g"], sc["cov"], sc["V"], sc["tri"], sc["tind"], H, W)
    assert not any(F.bad for F in R.faces) and all(len(p) for p in R.records)
    got = cbwd(g, cov, V, tri, ti, H, W)
    worst = RN.check_bound(got.cpu().numpy(), R)                              # ... and exactly +0 where no record names the vertex
    print("B=%d %dx%d: %d owners of %d vertices, worst error / bound = %.3f" % (B, H, W, gm["splits"], gm["range"], worst))
    assert worst <= 1.0
    assert float(got[:, 0].abs().max()) > 0 and float(got[:, 1].abs().max()) > 0
    assert not bool(_bits(got[:, 2]).any())                                   # the z row: exactly +0
    assert _same(cbwd(g, cov, V, tri, ti, H, W), got)                         # two calls: the same bits
    old = torch.randn(got.shape, generator=torch.Generator().manual_seed(B + H)).to(DEV)
    assert _same(cbwd(g, cov, V, tri, ti, H, W, out=old.clone(), accumulate=1), old + got)   # one fp32 add per element
    pitch = 480 + 22
    Vp = torch.full((B, 3, pitch), float("nan"), device=DEV)
    Vp[:, :, :480] = V
    assert _same(cfwd(Vp, tri, ti, H, W, pitch=(pitch, 480)), cov)
    assert _same(cbwd(g, cov, Vp, tri, ti, H, W, pitch=(pitch, 480)), got)


def test_a_face_alone_has_the_bits_it_has_in_a_batch_of_eight(small_assets):
    sc = scene(small_assets, 8, 64, 64)
    H = W = 64
    g, cov, V, tri, ti = _t(sc["g"]), _t(sc["cov"]), _t(sc["V"]), _t(sc["tri"]), _t(sc["tind"])
    first = cbwd(g, cov, V, tri, ti, H, W)
    assert geom(1, 480, H, W)["range"] != geom(8, 480, H, W)["range"]
    for b0 in (0, 5, 7):
        s = slice(b0, b0 + 1)
        part = cbwd(g[s].contiguous(), cov[s].contiguous(), V[s].contiguous(), tri, ti[s].contiguous(), H, W)
        assert _same(part, first[s]), b0
        assert _same(cfwd(V[s].contiguous(), tri, ti[s].contiguous(), H, W), cov[s])


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
def _against_the_model(V, tri, tind, H, W, g=None, seed=3):
    """forward bits, then the backward's bound with the forward's own plane -> (cov [B,H,W] numpy, vertex_grad numpy, model)"""
    B = V.shape[0]
    want = RC.forward(V, tri, tind, H, W)
    cov = cfwd(_t(V), _t(tri), _t(tind.reshape(B, H, W, 1)), H, W)
    assert_bits_equal(cov.cpu().numpy(), want, "soft coverage")
    if g is None:
        g = np.random.RandomState(seed).standard_normal((B, H * W)).astype(np.float32)
        g[g == 0] = 1.0
    R = RC.model(g, want, V, tri, tind, H, W)
    got = cbwd(_t(g), cov, _t(V), _t(tri), _t(tind), H, W).cpu().numpy()
    assert RN.check_bound(got, R) <= 1.0
    assert not got[:, 2].view(np.uint32).any()
    return want.reshape(B, H, W), got, R


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (8, 1)])
def test_images_one_pixel_wide_or_high(small_assets, H, W):
    """no neighbour above and below (or left and right, or at all): a hand-made tri_ind, half of it background"""
    sc = scene(small_assets, 3, 8, 9)
    rs = np.random.RandomState(H * 10 + W)
    ntri = sc["tri"].shape[1]
    tind = rs.randint(0, ntri, (3, H * W)).astype(np.float32)
    tind[rs.uniform(size=tind.shape) < 0.5] = -1
    tind[0, 0], tind[1, 0] = 5, -1
    cov, _, _ = _against_the_model(sc["V"], sc["tri"], tind, H, W)
    if H * W == 1:
        assert cov.reshape(-1).tolist() == [1, 0, cov.reshape(-1)[2]]         # no pair exists: hard


def test_a_face_pushed_across_the_image_border(small_assets):
    sc = scene(small_assets, 3, 33, 40)
    H, W = 33, 40
    V = sc["V"].copy()
    V[0, 0] += 0.45 * W                                                       # out through the right edge
    V[1, 1] -= 0.45 * H                                                       # out through the top
    V[2, 0] -= 0.4 * W
    V[2, 1] += 0.4 * H                                                        # a corner
    outs = ops().render_depth(_t(V), _t(sc["tri"]), _t(small_assets["vertex"]), torch.zeros((3, H, W, 3), device=DEV))
    tind = outs[3].cpu().numpy().reshape(3, H * W)
    ok = (tind >= 0).reshape(3, H, W)
    assert ok[0, :, -1].any() and ok[1, 0, :].any() and ok[2, -1, :].any() and ok[2, :, 0].any() and not ok.all(axis=(1, 2)).any()
    cov, got, R = _against_the_model(V, sc["tri"], tind, H, W)
    inner = _neighbours_share_state(ok) & ok                                  # (a neighbour outside the image does not exist)
    assert inner[0, :, -1].any() and inner[1, 0, :].any() and np.all(cov[inner] == 1)
    assert np.abs(got[:, 0:2]).max() > 0


def test_a_hand_made_tri_ind_with_every_kind_of_not_ok_pixel(small_assets):
    """[2,8,9,1]: -1, NaN, ntri, a value beyond int32 and a triangle with an id >= nver are all not OK -- background to their OK
    neighbours, and soft themselves"""
    sc = scene(small_assets, 3, 8, 9)
    V = sc["V"][:2].copy()
    nver, H, W = sc["nver"], 8, 9
    tri = sc["tri"].copy()
    ntri = tri.shape[1]
    bad_t = 7
    tri[1, bad_t] = nver
    rs = np.random.RandomState(8)
    tind = rs.randint(0, ntri, (2, H * W)).astype(np.float32)
    tind[tind == bad_t] = bad_t + 1
    special = (-1, np.nan, ntri, bad_t, 3e9, ntri + 5)
    tind[0, 20:26] = special
    tind[1, 40:46] = special[::-1]
    okt, _ = RC.ok_triangles(tri, tind[0], nver)
    assert np.all(okt[20:26] == -1) and np.all(okt[:20] >= 0)
    cov, got, R = _against_the_model(V, tri, tind, H, W)
    assert np.all(cov.reshape(2, -1)[0, :9] == 1)                             # the first row: OK among OK
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("case", ["lone_triangle", "border_3.25", "border_3.75", "border_2.75", "zero_area", "four_slivers",
                                  "tiny_triangle"])
def test_hand_made_scenes(case):
    """tests/coverage_cases.py, whose numbers tests/test_coverage_cpu.py works out by hand on the model"""
    V, tri, tind, H, W = getattr(CC, case)() if not case.startswith("border") else CC.vertical_border(float(case[7:]))
    ones = np.ones((1, H * W), np.float32)
    cov, got, R = _against_the_model(V, tri, tind, H, W, g=ones)
    cov = cov[0]
    if case == "lone_triangle":
        assert (cov[2, 2], cov[1, 2], cov[2, 3], cov[3, 2], cov[2, 1]) == (0.75, 0.125, 0.375, 0.375, 0) and cov.sum() == 1.625
        one = np.zeros((1, 25), np.float32)
        one[0, 12] = 1
        _, got, _ = _against_the_model(V, tri, tind, H, W, g=one)             # cov(c) = 0.5 + (2 - x0)
        assert abs(float(got[0, 0].astype(np.float64).sum()) + 1) < 1e-6 and got[0, 0, 1] == 0 and got[0, 1, 1] == 0
    elif case in ("border_3.25", "border_3.75"):
        xb = float(case[7:])
        assert np.all(cov[:, :3] == 1) and np.all(cov.sum(1) == np.float32(xb + 0.5))
        assert np.all(cov[:, 3] == (0.75 if xb < 3.5 else 1)) and np.all(cov[:, 4] == (0 if xb < 3.5 else 0.25))
        assert abs(float(got[0, 0, 0]) + float(got[0, 0, 1]) - H) < 1e-5 and got[0, 0, 2] == 0   # d sum(cov) / d xb = one per row
    elif case == "border_2.75":                                               # s = -0.25: clamped to 0, no gradient
        assert np.all(cov[:, 3] == 0.5) and not cov[:, 4:].any() and not got.view(np.uint32).any()
    elif case == "zero_area":                                                 # inert
        assert cov.reshape(-1).tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0] and not got.view(np.uint32).any()
    elif case == "four_slivers":                                              # the middle clamps at 1 and passes nothing back
        assert cov[2, 2] == 1 and np.abs(got).max() > 0
        one = np.zeros((1, 25), np.float32)
        one[0, 12] = 1
        _, got, _ = _against_the_model(V, tri, tind, H, W, g=one)
        assert not got.view(np.uint32).any()
    else:                                                                     # the pixel clamps at 0
        assert not cov.view(np.uint32).any() and not got.view(np.uint32).any()


# ---- Python surface ----------------------------------------------------------------------------------------------------------------------
def test_soft_coverage_under_autograd_is_the_raw_call(small_assets):
    sc = scene(small_assets, 3, 33, 40)
    H, W = 33, 40
    o = ops()
    tri, ti = _t(sc["tri"]), _t(sc["tind"].reshape(3, H, W, 1))
    w = _t(sc["g"].reshape(3, H, W, 1))
    V = _t(sc["V"]).requires_grad_(True)
    cov = o.soft_coverage(V, tri, ti)
    assert _same(cov, _t(sc["cov"])) and cov.requires_grad
    (cov * w).sum().backward()
    assert _same(V.grad, cbwd(w, cov.detach(), V.detach(), tri, ti, H, W))
    with pytest.raises(ValueError):
        o.soft_coverage(V, tri, ti.clone().requires_grad_(True))
    # a second backward on the same stream reuses the pooled workspace: the same bits
    V2 = _t(sc["V"]).requires_grad_(True)
    (o.soft_coverage(V2, tri, ti) * w).sum().backward()
    assert _same(V2.grad, V.grad)


def test_silhouette_loss_reaches_the_pose(small_assets):
    """silhouette_loss(...).backward() through vertices_transform(pose_grad=True): finite everywhere, non-zero at the x and y
    translations, at f and at the angles.  (t3d's third column moves z alone, and the coverage's z row is +0 by definition: that
    column is exactly 0.)"""
    A = small_assets
    B, S = 2, 64
    net = net_mod().FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=torch.device(DEV))
    losses = pkg("nets.losses")
    rs = np.random.RandomState(0)
    P = np.zeros((B, 7 + A["ndim_shape"] + A["ndim_exp"]), np.float32)
    P[:, 0:3] = rs.uniform(-0.4, 0.4, (B, 3))
    P[:, 3:5] = rs.uniform(29, 35, (B, 2))
    P[:, 6] = rs.uniform(2.8e-4, 3.4e-4, B)
    P[:, 7:7 + A["ndim_shape"]] = rs.uniform(0, 1e4, (B, A["ndim_shape"]))
    truth = _t(P)
    with torch.no_grad():
        mask = (net.soft_mask(net.vertices_transform(truth)) >= 0.5).float()
    assert 0.05 < float(mask.mean()) < 0.95
    moved = truth.clone()
    moved[:, 3] += 2.5
    moved[:, 4] -= 1.5
    moved[:, 6] *= 0.93
    p = moved.clone().requires_grad_(True)
    L = losses.silhouette_loss(net, net.vertices_transform(p, pose_grad=True), mask)
    L.backward()
    assert float(L.detach()) > 0 and bool(torch.isfinite(p.grad).all())
    assert bool((p.grad[:, 3:5] != 0).all()) and bool((p.grad[:, 6] != 0).all()) and bool((p.grad[:, 0:3] != 0).all())
    assert not bool(p.grad[:, 5].any())
    # a step against the gradient of the translation lowers the loss
    with torch.no_grad():
        q = moved.clone()
        q[:, 3:5] -= 0.5 * torch.sign(p.grad[:, 3:5])
        assert float(losses.silhouette_loss(net, net.vertices_transform(q), mask)) < float(L.detach())
        assert float(losses.silhouette_loss(net, net.vertices_transform(truth), mask)) < 0.25 * float(L.detach())
    # get_loss: absent by default, one more entry and lambda times it on top when asked for
    sig = __import__("inspect").signature(losses.get_loss).parameters
    assert sig["silhouette_mask"].default is None and sig["lambda_silhouette"].default == 1.0


def _program(cmd, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _record(p):
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[-2000:]
    return json.loads(lines[0])


def test_photo_fit_fits_the_pose():
    d = _record(_program(["examples/photo_fit.py", "--small", "--fit-pose"]))
    print("photo_fit --small --fit-pose:", json.dumps(d))
    assert d["fit_pose"] is True and d["finite"] is True and np.isfinite(d["first"]) and np.isfinite(d["last"])
    assert d["last"] < d["first"]
    assert d["errors_after"]["t3d_rms"] < d["errors_before"]["t3d_rms"]
    for k in ("t3d_rms", "f_rel_rms", "angle_rms"):
        assert np.isfinite(d["errors_before"][k]) and np.isfinite(d["errors_after"][k])


def test_get_loss_silhouette_term_is_opt_in(small_assets):
    """silhouette_mask=None: the dict and the total's bits are the default call's; given: one more entry and lambda times it on top"""
    B, S = 2, 64
    face = net_mod().FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S, device=torch.device(DEV))
    losses = pkg("nets.losses")
    label = torch.as_tensor(pkg("utils.synth").sample_params_batch(B, im_size=S, n_shape=face.ndim_shape, n_exp=face.ndim_exp,
                                                                   beta=0.7, seed=5), device=DEV)
    label[:, 6] = 3e-4
    gen = torch.Generator().manual_seed(2)
    im = torch.rand((B, S, S, 1), generator=gen).to(DEV)
    coarse, fine = torch.rand((B, S, S, 1), generator=gen).to(DEV), torch.rand((B, S, S, 1), generator=gen).to(DEV)
    with torch.no_grad():
        mask = (face.soft_mask(face.vertices_transform(label)) >= 0.5).float()
    pred = label.clone()
    pred[:, 3] += 2.0
    pred.requires_grad_(True)

    def run(**kw):
        return losses.get_loss(face, pred, label, im, face.vertices_transform(pred, pose_grad=True), coarse, fine, **kw)
    base, none, on = run(), run(silhouette_mask=None), run(silhouette_mask=mask, lambda_silhouette=0.5)
    assert "silhouette_loss" not in base and sorted(none) == sorted(base) and _same(none["total_loss"], base["total_loss"])
    assert sorted(on) == sorted(list(base) + ["silhouette_loss"]) and float(on["silhouette_loss"].detach()) > 0
    want = base["total_loss"] + (0.5 * on["silhouette_loss"]).to(base["total_loss"].dtype)
    assert _same(on["total_loss"], want)
    on["total_loss"].backward()
    assert bool(torch.isfinite(pred.grad).all()) and bool((pred.grad[:, 3] != 0).all())


def test_silhouette_loss_flag_needs_synthetic_data():
    p = _program(["examples/coarse_loop.py", "--small", "--train", "--steps", "1", "--warmup", "0", "--silhouette-loss"], timeout=120)
    assert p.returncode == 2 and "--silhouette-loss needs --synth-data" in p.stderr and not p.stdout.strip()
