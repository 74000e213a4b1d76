"""CPU: the photometric loss (csrc/fr_photo.hip) and the albedo blend's adjoint (csrc/fr_synth.hip).  The numpy model of the GPU tests
(tests/ref_photo_loss.py) is held to central differences of a float64 forward and to torch autograd of the stock composition; the
model's own image gives exact zeros; the blend's adjoint is held to the float64 einsum; the entry points exist, answer their sizes
and geometry, and return every code of the header before any HIP call; the Python surface keeps its defaults and raises where the
header says."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from conftest import pkg
import ref_photo_loss as RP
import ref_synth_batch as RS

NEW = ("fr_photo_loss_state_bytes", "fr_photo_loss_forward", "fr_photo_loss_backward", "fr_debug_photo_loss_geom",
       "fr_synth_texture_backward_workspace_bytes", "fr_synth_texture_backward")
F = np.float32
GAIN, OFFSET = 1.75, -0.125


def _L():
    return pkg("_lib").lib()


def test_symbols_exported():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert "fr_photo.hip" in pkg("_lib").SOURCES


# ---- the model's gradient -----------------------------------------------------------------------------------------------------------------
def _case64():
    tex, nrm, ti, light, target, weight = RP.smooth_case()
    st = RP.shade_terms(tex, nrm, ti, light, GAIN, OFFSET)
    cov = st["covered"]
    # the case keeps away from the kinks
    assert (np.abs(st["s"][cov]) > 0.05).all() and (st["s"][cov] > 0).all() and (tex > 0.1).all() and (st["mag"] > 1e-3).all()
    assert cov.any() and (~cov).any() and st["flipped"][cov].any() and (~st["flipped"][cov]).any()
    return tex, nrm, ti, light, target, weight, cov


def _bound(g):
    return 64 * 2.0 ** -24 * np.abs(g).max()


def test_model_gradient_against_central_differences():
    tex, nrm, ti, light, target, weight, cov = _case64()
    B = tex.shape[0]
    g_up = np.array([1.0, -0.75])[:B]
    gt, gn, gl, _ = RP.backward(tex, nrm, ti, light, target, g_up, weight, GAIN, OFFSET, rounded=False)
    x64 = [tex.astype(np.float64), nrm.astype(np.float64), light.astype(np.float64)]
    t64, w64 = target.astype(np.float64)[..., 0], weight.astype(np.float64)[..., 0]

    def loss(xs):
        return float((g_up * RP.forward64(xs[0], xs[1], cov, xs[2], t64, w64, GAIN, OFFSET)).sum())
    h = 1e-6
    for k, (name, want) in enumerate((("tex_img", gt), ("normal", gn), ("light", gl))):
        num = np.zeros(x64[k].shape)
        for idx in np.ndindex(*x64[k].shape):
            xs = [x.copy() for x in x64]
            xs[k][idx] += h
            up = loss(xs)
            xs[k][idx] -= 2 * h
            num[idx] = (up - loss(xs)) / (2 * h)
        err = np.abs(num - want).max()
        print("%s: max |model - central difference| = %.3g, bound %.3g, max |g| = %.3g" % (name, err, _bound(want), np.abs(want).max()))
        assert np.abs(want).max() > 1e-3 and err <= _bound(want), name
    assert not gt[~cov].any() and not gn[~cov].any()


def test_model_gradient_against_torch_autograd():
    """the stock composition (the formula of test_shade_against_the_stock_torch_composition, then a masked squared error) in float64
    under torch CPU autograd: an independent statement of the same derivative"""
    tex, nrm, ti, light, target, weight, cov = _case64()
    B = tex.shape[0]
    g_up = np.array([1.0, -0.75])[:B]
    t = lambda a: torch.tensor(a.astype(np.float64), requires_grad=True)   # noqa: E731
    tex_t, nrm_t, l_t = t(tex), t(nrm), t(light)
    a = torch.clamp_min(tex_t, 1e-6).mean(dim=-1, keepdim=True)
    n = torch.where(nrm_t[..., 2:3] < 0, -1.0 * nrm_t, nrm_t)
    mag = (n * n).sum(-1)
    mag = torch.where(mag > 1e-6, mag, torch.ones_like(mag))
    nm = n / (torch.sqrt(mag) + 1e-6)[..., None]
    s = l_t[:, None, None, 0:1] + (l_t[:, None, None, 1:4] * nm).sum(-1, keepdim=True)
    im = a * torch.relu(s) * GAIN + OFFSET
    r = im - torch.tensor(target.astype(np.float64))
    sse = (torch.tensor(cov[..., None].astype(np.float64) * weight.astype(np.float64)) * r * r).sum(dim=(1, 2, 3))
    (torch.tensor(g_up) * sse).sum().backward()
    gt, gn, gl, _ = RP.backward(tex, nrm, ti, light, target, g_up, weight, GAIN, OFFSET, rounded=False)
    sums = RP.forward(tex, nrm, ti, light, target, weight, GAIN, OFFSET)
    assert np.abs(sums[:, 0] - sse.detach().numpy()).max() <= 64 * 2.0 ** -24 * np.abs(sums[:, 0]).max()
    assert np.array_equal(sums[:, 1], cov.reshape(B, -1).sum(1).astype(np.float64))
    for name, want, got in (("tex_img", gt, tex_t.grad.numpy()), ("normal", gn, nrm_t.grad.numpy()), ("light", gl, l_t.grad.numpy())):
        err = np.abs(got - want).max()
        print("%s: max |model - autograd| = %.3g, bound %.3g" % (name, err, _bound(want)))
        assert err <= _bound(want), name


@pytest.mark.parametrize("weighted", [False, True])
def test_the_models_own_image_gives_exact_zeros(weighted):
    B, H, W = 3, 33, 17
    tex, nrm, ti, light, _, weight = RP.hand_planes(B, H, W, seed=5)
    assert RP.reaches_every_branch(tex, nrm, ti, light)
    target, _ = RS.shade(tex, nrm, ti, light, None, GAIN, OFFSET)
    w = weight if weighted else None
    sums = RP.forward(tex, nrm, ti, light, target, w, GAIN, OFFSET)
    assert not sums[:, 0].any() and not sums[:, 2:].any()
    assert np.array_equal(sums[:, 1], (ti[..., 0] >= 0).reshape(B, -1).sum(1).astype(np.float64))
    gt, gn, gl, _ = RP.backward(tex, nrm, ti, light, target, np.array([1.0, -2.0, 0.5]), w, GAIN, OFFSET)
    assert not gt.any() and not gn.any() and not gl.any()
    # ... and an independent target does not
    other = RP.hand_planes(B, H, W, seed=5)[4]
    gt, gn, gl, _ = RP.backward(tex, nrm, ti, light, other, np.array([1.0, -2.0, 0.5]), w, GAIN, OFFSET)
    assert gt.any() and gn.any() and gl.all()


def test_a_faces_sums_do_not_depend_on_the_batch():
    tex, nrm, ti, light, target, weight = RP.hand_planes(3, 33, 17, seed=8, nan=True)
    whole = RP.forward(tex, nrm, ti, light, target, weight, GAIN, OFFSET)
    for b in range(3):
        one = RP.forward(tex[b:b + 1], nrm[b:b + 1], ti[b:b + 1], light[b:b + 1], target[b:b + 1], weight[b:b + 1], GAIN, OFFSET)
        assert np.array_equal(one.view(np.uint64), whole[b:b + 1].view(np.uint64)) or (b == 2 and np.isnan(one[0, 0]))
    assert np.isnan(whole[2, 0]) and np.isfinite(whole[:2]).all() and np.isfinite(whole[2, 1])


# ---- the blend's adjoint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, K, B", [(480, 3, 1), (480, 10, 3), (515, 17, 9), (85, 33, 2), (5500, 3, 2)])
def test_blend_adjoint_model_against_float64_einsum(N, K, B):
    rs = np.random.RandomState(N + K + B)
    pc = rs.standard_normal((3 * N, K)).astype(F)
    g = (rs.standard_normal((B, 3, N)) * np.exp2(rs.randint(-8, 8, (B, 3, N)))).astype(F)
    got64 = RP.texture_backward(pc, g, rounded=False)
    want = np.einsum("rk,br->bk", pc.astype(np.float64), g.reshape(B, -1).astype(np.float64))
    mag = np.einsum("rk,br->bk", np.abs(pc).astype(np.float64), np.abs(g.reshape(B, -1)).astype(np.float64))
    bound = 3 * N * 2.0 ** -53 * mag
    print("blend adjoint: max |model - einsum| / bound = %.3g" % (np.abs(got64 - want) / bound).max())
    assert (np.abs(got64 - want) <= bound).all()
    got = RP.texture_backward(pc, g)
    assert got.dtype == F and np.array_equal(got, got64.astype(F))
    assert (np.abs(got.astype(np.float64) - want) <= bound + 2.0 ** -24 * np.abs(want)).all()


def test_blend_adjoint_sizes():
    L = _L()
    for B, N, K in [(1, 480, 3), (3, 480, 10), (64, 35709, 80), (9, 515, 17), (1, 1, 1)]:
        assert L.fr_synth_texture_backward_workspace_bytes(B, N, K) == -(-3 * N // RP.TX_ROWS) * B * K * 8, (B, N, K)
    for bad in [(0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (65536, 5, 5), (1, (1 << 31) // 3, 1)]:
        assert L.fr_synth_texture_backward_workspace_bytes(*bad) == 0, bad


# ---- sizes, geometry and return codes -------------------------------------------------------------------------------------------------------
def test_sizes_and_geometry():
    L = _L()
    for B, H, W in [(1, 5, 6), (3, 33, 17), (2, 64, 64), (64, 200, 200), (65535, 1, 1), (1, 1, 1), (1, 16, 16)]:
        g = RP.geom(B, H, W)
        assert g == [256, -(-H * W // 256), 256, 6], (B, H, W)
        assert L.fr_photo_loss_state_bytes(B, H, W) == B * g[1] * 6 * 8
    assert RP.geom(1, 5, 6)[1] == 1 and RP.geom(3, 33, 17)[1] == 3 and 33 * 17 == 2 * 256 + 49 and RP.geom(2, 64, 64)[1] == 16
    for bad in [(0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (65536, 1, 1), (1, 1 << 16, 1 << 15),
                (1, (1 << 31) - 1, (1 << 31) - 1)]:
        assert RP.geom(*bad) == [0] * 4 and L.fr_photo_loss_state_bytes(*bad) == 0, bad
    # the model's association reads this geometry: a face's sums are a function of (H, W) alone
    assert RP.geom(1, 33, 17) == RP.geom(7, 33, 17)


GOOD, ODD = 0x1000, 0x1008          # made-up addresses: 16-byte aligned, and not


def test_return_codes_without_a_gpu():
    """Every call here trips a check, so none reaches HIP.  SKIPS where a GPU is visible, as tests/test_fine_losses_cpu.py does: it
    checks host code, and a case that slipped through validation would launch on the made-up addresses."""
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    L = _L()
    P = ctypes.c_void_p
    nst = L.fr_photo_loss_state_bytes(3, 17, 33)

    def fwd(B=3, H=17, W=33, state=GOOD, state_bytes=nst, **nul):
        p = {k: P(0 if k in nul else GOOD) for k in ("tex_img", "normal", "tri_ind", "light", "target", "weight", "sums")}
        return L.fr_photo_loss_forward(p["tex_img"], p["normal"], p["tri_ind"], p["light"], p["target"], p["weight"], B, H, W, 1.0, 0.0,
                                       p["sums"], P(state), state_bytes, P(0))

    def bwd(B=3, H=17, W=33, **nul):
        p = {k: P(0 if k in nul else GOOD) for k in ("grad_sse", "sums", "tex_img", "normal", "tri_ind", "light", "target", "weight",
                                                     "gt", "gn", "gl")}
        return L.fr_photo_loss_backward(p["grad_sse"], p["sums"], p["tex_img"], p["normal"], p["tri_ind"], p["light"], p["target"],
                                        p["weight"], B, H, W, 1.0, 0.0, p["gt"], p["gn"], p["gl"], P(0))
    for fn in (fwd, bwd):
        for neg in (dict(B=-1), dict(H=-1), dict(W=-5)):
            assert fn(**neg) == -1 and fn(tex_img=0, **neg) == -1
        for empty in (dict(B=0), dict(H=0), dict(W=0)):
            assert fn(**empty) == 0 and fn(tex_img=0, normal=0, tri_ind=0, light=0, target=0, sums=0, **empty) == 0
        for req in ("tex_img", "normal", "tri_ind", "light", "target"):
            assert fn(**{req: 0}) == -1, (fn.__name__, req)
            assert fn(B=65536, **{req: 0}) == -1                          # the pointers come before the grid
        for big in (dict(B=65536), dict(H=1 << 16, W=1 << 15)):
            assert fn(**big) == -4, (fn.__name__, big)
    assert fwd(sums=0) == -1
    for kw in (dict(state=0), dict(state=ODD), dict(state_bytes=nst - 1), dict(state_bytes=0)):
        assert fwd(**kw) == -2, kw
        assert fwd(tex_img=0, **kw) == -1                                  # a NULL pointer comes before the state
    assert fwd(B=65536, state=0) == -2 and fwd(B=65536, state_bytes=0) == -4   # (beyond one grid the state's size is 0)
    assert fwd(W=0, state=0, state_bytes=0) == 0
    assert bwd(grad_sse=0) == -1
    assert bwd(sums=0) == -1 and bwd(sums=0, gl=0, B=65536) == -4           # sums serve grad_light alone
    assert bwd(gt=0, gn=0, gl=0) == 0                                       # nothing wanted: nothing launched
    assert bwd(gt=0, gn=0, gl=0, B=65536) == -4 and bwd(weight=0, B=65536) == -4

    # the blend's adjoint: the codes of fr_synth_texture, then the workspace
    nws = L.fr_synth_texture_backward_workspace_bytes(3, 480, 10)

    def txb(B=3, N=480, K=10, pc=GOOD, g=GOOD, out=GOOD, ws=GOOD, nbytes=nws):
        return L.fr_synth_texture_backward(P(pc), P(g), B, N, K, P(out), P(ws), nbytes, P(0))
    assert txb(B=0) == -1 and txb(N=0) == -1 and txb(K=-1) == -1 and txb(B=0, pc=0) == -1
    assert txb(B=65536) == -4 and txb(B=65536, pc=0) == -4 and txb(N=(1 << 31) // 3) == -4
    assert txb(K=0) == 0 and txb(K=0, pc=0, g=0, out=0, ws=0, nbytes=0) == 0
    assert txb(pc=0) == -1 and txb(g=0) == -1 and txb(out=0) == -1 and txb(pc=0, ws=0) == -1
    assert txb(ws=0) == -2 and txb(ws=ODD) == -2 and txb(nbytes=nws - 1) == -2 and txb(nbytes=0) == -2


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
def test_python_surface_defaults_and_errors():
    losses, ops = pkg("nets.losses"), pkg("rendering_layer.ops")
    p = inspect.signature(losses.get_loss).parameters
    want = dict(photo_light=None, photo_alpha=None, photo_weight=None, photo_gain=1.0, photo_offset=0.0, lambda_photo=1.0)
    assert {k: p[k].default for k in want} == want
    # together, in this order, behind every argument a caller could sensibly pass by position (geometry_gram keeps the last place
    # tests/test_geometry_gram_cpu.py gives it, as fine_fused and sfs_alpha_lse left it there)
    assert list(p)[-len(want) - 1:-1] == list(want) and list(p)[-1] == "geometry_gram"
    assert list(inspect.signature(ops.photo_loss).parameters) == ["tex_img", "normal", "tri_ind", "light", "target", "weight", "gain",
                                                                  "offset"]
    assert list(inspect.signature(losses.photometric_loss).parameters) == ["face_net", "vertices_proj", "im_gray", "light", "alpha",
                                                                           "weight", "gain", "offset"]
    assert issubclass(ops._PhotoLoss, torch.autograd.Function) and issubclass(ops._SynthTexture, torch.autograd.Function)
    x = torch.zeros(2, 4)
    for kw in (dict(photo_light=x), dict(photo_alpha=x)):
        with pytest.raises(ValueError, match="photo_light and photo_alpha"):
            losses.get_loss(None, None, None, None, None, None, None, **kw)
    alpha = torch.zeros(2, 3, requires_grad=True)
    with pytest.raises(ValueError, match="out="):
        ops.synth_texture(torch.zeros(3, 5), torch.zeros(15, 3), alpha, out=torch.zeros(2, 3, 5))


def test_get_loss_defaults_return_todays_keys(monkeypatch):
    """get_loss on stand-ins for the parts that need a GPU (the basis product, the SfS renders): with the new arguments at their
    defaults the dict holds today's six keys; the photometric term is the only thing the new arguments add"""
    import types
    losses = pkg("nets.losses")
    B, d = 2, 12
    fn = types.SimpleNamespace(ndim=d, ndim_pose=7, geometry_product=lambda x: x * 2.0)
    monkeypatch.setattr(losses, "get_spherical_harmonics_model", lambda fn, v, im, **kw: im * 0.5)
    monkeypatch.setattr(losses, "photometric_loss", lambda fn, v, im, light, alpha, **kw: (light.double().sum() + alpha.double().sum()))
    rs = np.random.RandomState(0)
    t = lambda *s: torch.as_tensor(rs.standard_normal(s).astype(F))   # noqa: E731
    args = (fn, t(B, d), t(B, d), t(B, 4, 4, 1), None, t(B, 4, 4, 1), t(B, 4, 4, 1))
    base = losses.get_loss(*args)
    assert set(base) == {"pose_loss", "geometry_loss", "spherical_harmonics_loss", "fidelity_loss", "smoothness_loss", "total_loss"}
    light, alpha = t(B, 4), t(B, 3)
    with_photo = losses.get_loss(*args, photo_light=light, photo_alpha=alpha, lambda_photo=0.25)
    assert set(with_photo) == set(base) | {"photometric_loss"}
    for k in base:
        if k != "total_loss":
            assert torch.equal(base[k], with_photo[k]), k
    want = base["total_loss"] + (0.25 * with_photo["photometric_loss"]).to(base["total_loss"].dtype)
    assert torch.equal(with_photo["total_loss"], want) and with_photo["total_loss"].dtype == base["total_loss"].dtype
