"""CPU: the fine-depth losses (csrc/fr_fine_losses.hip).  The float64 model of the GPU tests (tests/ref_fine_losses.py) is held to the
torch expressions it replaces, in float64, with autograd for the gradients; the entry points exist, answer their sizes and their
geometry, and validate in the header's order before any HIP call -- every single bad argument and every pair, the earlier item
winning; the Python surface keeps its defaults."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import pkg
import ref_fine_losses as RF

NEW = ("fr_fine_losses_state_bytes", "fr_fine_losses_forward", "fr_fine_losses_backward", "fr_debug_fine_losses_geom")
U = 2.0 ** -53


def _L():
    return pkg("_lib").lib()


def test_symbols_exported():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert "fr_fine_losses.hip" in pkg("_lib").SOURCES


def test_sizes_and_geometry():
    L = _L()
    tw, th = RF.tile()
    assert tw > 0 and th > 0 and tw * th % 64 == 0
    for B, H, W in RF.shapes() + [(64, 200, 200), (65535, 1, 1)]:
        g = RF.geom(B, H, W)
        assert g[:3] == [tw, th, tw * th] and g[3] == -(-W // tw) and g[4] == -(-H // th), (B, H, W)
        assert g[5] >= 64 and g[5] % 64 == 0 and g[5] // 64 <= 64 and (g[5] // 64) & (g[5] // 64 - 1) == 0
        assert 0 < g[6] <= 64 * 1024
        assert L.fr_fine_losses_state_bytes(B, H, W) == (2 + 2 * g[3] * g[4] * B) * 8
    for bad in [(0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (65536, 1, 1), (1, 65535 * th + 1, 1),
                (1, 1 << 16, 1 << 15), (1, (1 << 31) - 1, (1 << 31) - 1)]:
        assert RF.geom(*bad) == [0] * 7 and L.fr_fine_losses_state_bytes(*bad) == 0, bad
    # the test shapes sit where they say: one tile exactly, one past it, ragged multi-tile
    hw = sorted(set((H, W) for _, H, W in RF.shapes()))
    assert (th, tw) in hw and (th + 1, tw + 1) in hw and (2 * th + 1, 2 * tw + 3) in hw and (3, 3) in hw and (1, 1) in hw
    assert RF.geom(1, th, tw)[3:5] == [1, 1] and RF.geom(1, th + 1, tw + 1)[3:5] == [2, 2]
    assert RF.geom(1, 2 * th + 1, 2 * tw + 3)[3:5] == [3, 3]


# ---- the checks: every single bad argument, and every pair ----------------------------------------------------------------------------
# A defect = (the header's item it trips, the arguments it replaces).  The code a call answers is that of the LOWEST item among its
# defects: 1 negative size -> -1, 2 empty shape -> 0, 3 NULL required pointer -> -1, 4 state -> -2, 5 beyond one grid -> -4.
CODE = {1: -1, 2: 0, 3: -1, 4: -2, 5: -4}
GOOD, ODD = 0x1000, 0x1008          # made-up addresses: 16-byte aligned, and not
BASE = dict(B=3, H=17, W=33)
POINTERS = ("pred", "coarse", "fidelity", "smoothness", "state", "gf", "gs", "grad_pred", "grad_coarse")


def _entry_points():
    L = _L()
    nul = ctypes.c_void_p(0)
    nst = L.fr_fine_losses_state_bytes(3, 17, 33)
    assert nst > 0

    def fwd(a):
        return L.fr_fine_losses_forward(a["pred"], a["coarse"], a["B"], a["H"], a["W"], a["fidelity"], a["smoothness"], a["state"],
                                        a["state_bytes"], nul)

    def bwd(a):
        return L.fr_fine_losses_backward(a["gf"], a["gs"], a["pred"], a["coarse"], a["B"], a["H"], a["W"], a["grad_pred"],
                                         a["grad_coarse"], nul)
    shape_bad = [(1, dict(B=-1)), (1, dict(H=-1)), (1, dict(W=-5)), (2, dict(B=0)), (2, dict(H=0)), (2, dict(W=0)),
                 (5, dict(B=65536)), (5, dict(H=1 << 16, W=1 << 15)), (5, dict(H=65535 * RF.tile()[1] + 1))]
    return {
        "forward": (fwd, dict(pred=GOOD, coarse=GOOD, fidelity=GOOD, smoothness=GOOD, state=GOOD, state_bytes=nst),
                    shape_bad + [(3, dict(pred=0)), (3, dict(coarse=0)), (3, dict(fidelity=0)), (3, dict(smoothness=0)),
                                 (4, dict(state=0)), (4, dict(state=ODD)), (4, dict(state_bytes=nst - 1)),
                                 (4, dict(state_bytes=0))]),
        "backward": (bwd, dict(gf=GOOD, gs=GOOD, pred=GOOD, coarse=GOOD, grad_pred=GOOD, grad_coarse=GOOD),
                     shape_bad + [(3, dict(pred=0)), (3, dict(coarse=0)), (3, dict(grad_pred=0))]),
    }


def _call(fn, base, *defects):
    a = dict(BASE, **base)
    for _, d in defects:
        a.update(d)
    for k in POINTERS:
        if k in a:
            a[k] = ctypes.c_void_p(a[k])
    return fn(a)


def test_checks_hold_singly_and_in_pairs():
    """Every call here carries at least one defect, so each returns from the checks: none reaches HIP.  The test SKIPS where a GPU is
    visible, as tests/test_capi_codes_cpu.py and tests/test_geometry_gram_cpu.py do: it checks host code, and if a regression let a
    case through the checks, the call would launch on the made-up addresses.
    (A shape beyond one grid has a state size of 0, so the forward's state_bytes of the base shape never fails it: the state check
    then asks for a present, aligned pointer alone.)"""
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    singles = pairs = 0
    for name, (fn, base, defects) in _entry_points().items():
        for d in defects:
            assert _call(fn, base, d) == CODE[d[0]], (name, d)
            singles += 1
        for d1, d2 in itertools.combinations(defects, 2):
            if set(d1[1]) & set(d2[1]):
                continue                                       # two values for one argument: not a pair
            if {d1[0], d2[0]} == {4, 5} and "state_bytes" in (set(d1[1]) | set(d2[1])):
                continue                                       # a shape beyond one grid needs no bytes: a small state is no defect there
            want = CODE[min(d1[0], d2[0])]
            assert _call(fn, base, d1, d2) == want, (name, d1, d2, want)
            pairs += 1
    print("held %d single defects and %d pairs over two entry points" % (singles, pairs))
    assert singles >= 29 and pairs >= 150
    # the optional pointers are no defects: a call without them gets as far as the next check
    fn, base, _ = _entry_points()["backward"]
    assert _call(fn, base, (0, dict(gf=0, gs=0, grad_coarse=0)), (5, dict(B=65536))) == -4
    assert _call(fn, base, (0, dict(gf=0)), (3, dict(grad_pred=0))) == -1
    # an empty shape writes nothing and needs nothing
    assert _call(fn, base, (2, dict(B=0, gf=0, gs=0, pred=0, coarse=0, grad_pred=0, grad_coarse=0))) == 0
    fn, base, _ = _entry_points()["forward"]
    assert _call(fn, base, (2, dict(W=0, pred=0, coarse=0, fidelity=0, smoothness=0, state=0, state_bytes=0))) == 0
    # beyond one grid with a small state: the size is 0 there, so the answer is the grid's
    assert _call(fn, base, (5, dict(B=65536)), (0, dict(state_bytes=0))) == -4


# ---- the model against torch ----------------------------------------------------------------------------------------------------------
def test_torch_sign_is_the_headers_s():
    x = torch.tensor([3.0, -2.0, 0.0, -0.0, float("nan"), float("inf"), -float("inf")], dtype=torch.float64)
    got = torch.sign(x).numpy()
    want = RF.sign(x.numpy())
    print("torch.sign", got, "model", want)
    assert np.isnan(got[4]) or got[4] == 0.0
    keep = np.array([0, 1, 2, 3, 5, 6])
    assert np.array_equal(got[keep], want[keep]) and want[4] == 0.0
    # what matters is the gradient of abs, which is where the objective meets sign: 0 at +-0
    y = torch.tensor([0.0, -0.0, 2.0, -2.0], dtype=torch.float64, requires_grad=True)
    y.abs().sum().backward()
    assert y.grad.tolist() == [0.0, 0.0, 1.0, -1.0]


def _torch_route(z, c, g_f, g_s):
    """the objective's two expressions in float64 and their autograd gradients -> (fidelity, smoothness, L, grad_pred, grad_coarse)"""
    zt = torch.tensor(z.astype(np.float64)[..., None], requires_grad=True)
    ct = torch.tensor(c.astype(np.float64)[..., None], requires_grad=True)
    k = torch.tensor(RF.K, dtype=torch.float64)[None, None]
    Lp = F.conv2d(zt[..., 0][:, None], k, padding=1)[:, 0]
    fid = F.mse_loss(zt, ct)
    sm = Lp.abs().sum()
    (float(np.float32(g_f)) * fid + float(np.float32(g_s)) * sm).backward()
    return float(fid.detach()), float(sm.detach()), Lp.detach().numpy(), zt.grad[..., 0].numpy(), ct.grad[..., 0].numpy()


@pytest.mark.parametrize("wide", [False, True], ids=["near", "wide"])
@pytest.mark.parametrize("shape", RF.shapes(), ids=RF.case_id)
def test_model_vs_torch_float64(shape, wide):
    """The model is a float64 evaluation in one stated order, torch's another: each L within 9 roundings of its terms' magnitudes
    (exactly equal where the inputs make every partial sum exact: the planted regions), each sum within n u sum |term| of fsum, which
    bounds torch's sum the same way, and the gradients within a few roundings of their two terms."""
    B, H, W = shape
    z, c, planted = RF.inputs(B, H, W, wide=wide)
    n = B * H * W
    Lm = RF.laplacian(z)
    fwd = RF.forward(z, c)
    fid_t, sm_t, Lt, gp_t, gc_t = _torch_route(z, c, 1.0, 1.0)
    # L
    mag = RF.laplacian(np.abs(z)) + 12.0 * np.abs(z.astype(np.float64))      # sum |k_t z| (the centre tap enters with -6: add 2 x 6)
    errL = np.abs(Lm - Lt)
    print("%s: largest |L model - L torch| / (9 u sum|k z|) = %.3g" % (RF.case_id(shape), float((errL / (9 * U * mag + 1e-300)).max())))
    assert (errL <= 9 * U * mag).all()
    assert (Lm[planted] == 0).all() and (Lt[planted] == 0).all()
    share = float((Lm == 0).sum()) / n
    print("share of pixels with L == 0 on the model: %.3f" % share)
    if B == 3:
        assert share >= 0.1
    # the sums, each against fsum and torch's against the same bound
    tf, ts = RF.terms(z, c)
    for name, S, exact, tot, torch_val, scale in (("S_f", fwd["S_f"], fwd["fsum_f"], float(tf.sum()), fid_t * n, 1.0),
                                                  ("S_s", fwd["S_s"], fwd["fsum_s"], float(ts.sum()), sm_t, 1.0)):
        bound = n * U * tot + 1e-300
        print("%s: |model - fsum| / bound = %.3g, |torch - fsum| / bound = %.3g" % (name, abs(S - exact) / bound,
                                                                                  abs(torch_val - exact) / (bound + 20 * U * tot)))
        assert abs(S - exact) <= bound
        # torch's own sum obeys the same bound, plus the roundings of its terms (L within 9 u of its magnitude; mse's division)
        slack = 20 * U * (tot + float(mag.sum()) if name == "S_s" else tot)
        assert abs(torch_val - exact) <= bound + slack
    assert fwd["fidelity"] == np.float32(fwd["S_f"] / n) and fwd["smoothness"] == np.float32(fwd["S_s"])
    # gradients at (1, 1), and at the other pairs
    for g_f, g_s in RF.GRADS:
        _, _, _, gp_t, gc_t = _torch_route(z, c, g_f, g_s)
        gp, gc = RF.backward(z, c, g_f, g_s, rounded=False)
        cf = 2.0 / n
        a = abs(float(np.float32(g_f))) * cf * np.abs(z.astype(np.float64) - c.astype(np.float64))
        b = abs(float(np.float32(g_s))) * 12.0          # |T| <= sum |k| = 12
        tol = 8 * U * (a + b)
        # a pixel whose L the two evaluations round to different signs would differ by a multiple of 0.5 g_s: none may
        assert (np.abs(gp - gp_t) <= tol).all(), (g_f, g_s, float(np.abs(gp - gp_t).max()))
        assert (np.abs(gc - gc_t) <= tol).all()
        r32 = RF.backward(z, c, g_f, g_s)
        assert np.array_equal(r32[0], gp.astype(np.float32)) and np.array_equal(r32[1], gc.astype(np.float32))


def test_model_nan_and_zero_pixels():
    """a NaN depth: torch's abs backward multiplies by sign(NaN); the header's s(NaN) = 0 keeps T finite.  Where torch gives NaN
    there the model gives a finite number, by design; everywhere else the two agree, and the model's NaN footprint is one pixel."""
    B, H, W = 3, 17, 33
    z, c, _ = RF.inputs(B, H, W)
    z = z.copy()
    z[1] = RF.inputs(B, H, W, seed=5)[0][0]                          # face 1: random instead of all zero
    clean = RF.backward(z, c, 1.0, 1.0)
    bad = z.copy()
    bad[1, 8, 20] = np.nan
    fwd = RF.forward(bad, c)
    assert np.isnan(fwd["fidelity"]) and np.isnan(fwd["smoothness"])
    gp, gc = RF.backward(bad, c, 1.0, 1.0)
    assert np.array_equal(gp[[0, 2]].view(np.uint32), clean[0][[0, 2]].view(np.uint32))
    nonfinite = np.argwhere(~np.isfinite(gp))
    assert nonfinite.tolist() == [[1, 8, 20]] and np.argwhere(~np.isfinite(gc)).tolist() == [[1, 8, 20]]
    changed = np.argwhere(gp[1].view(np.uint32) != clean[0][1].view(np.uint32))
    assert len(changed) > 1 and (np.abs(changed - np.array([8, 20])).max(axis=1) <= 2).all()   # the 5 x 5 ring, no further
    # torch on the same input: equal outside the 5 x 5 ring
    _, _, Lt, gp_t, _ = _torch_route(bad, c, 1.0, 1.0)
    far = np.ones((B, H, W), bool)
    far[1, 6:11, 18:23] = False
    g64 = RF.backward(bad, c, 1.0, 1.0, rounded=False)[0]
    assert (np.abs(g64[far] - gp_t[far]) <= 8 * U * (np.abs(g64[far]) + 12.0)).all()
    # -0 and +0: an all-zero face has L == +0 everywhere and a zero smoothness gradient
    zz = np.zeros((1, 5, 7), np.float32)
    zz[0, 2, 3] = -0.0
    Lz = RF.laplacian(zz)
    assert not Lz.view(np.uint64).any()                              # +0, not -0: the chain starts from +0.0
    assert not RF.T_plane(zz).view(np.uint64).any()


def test_python_surface_defaults():
    losses, ops = pkg("nets.losses"), pkg("rendering_layer.ops")
    p = inspect.signature(losses.get_loss).parameters
    assert p["fine_fused"].default is False
    assert list(inspect.signature(ops.fine_depth_losses).parameters) == ["pred", "coarse"]
    assert issubclass(ops._FineDepthLosses, torch.autograd.Function)
