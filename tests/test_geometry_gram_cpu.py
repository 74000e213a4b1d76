"""CPU: the Gram-form geometry loss's entry points (csrc/fr_geometry.hip) exist, answer their sizes and their build geometry, and
validate in the header's order before any HIP call -- every single bad argument and every pair, the earlier item of the list winning;
the float64 model of the GPU tests (tests/ref_geometry_gram.py) is held to the objective's numpy restatement (oracle/losses_np.py)
and to central differences; the Python surface keeps its defaults."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import losses_np as LN
import ref_geometry_gram as RG

NEW = ("fr_geometry_gram_bytes", "fr_geometry_gram_workspace_bytes", "fr_geometry_gram_build", "fr_geometry_loss_state_bytes",
       "fr_geometry_loss_forward", "fr_geometry_loss_backward", "fr_debug_geometry_gram_geom")


def _L():
    return pkg("_lib").lib()


def _geom(N, ns, ne):
    out = (ctypes.c_int * 6)()
    _L().fr_debug_geometry_gram_geom(N, ns, ne, out)
    return list(out)


def test_symbols_exported():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert "fr_geometry.hip" in pkg("_lib").SOURCES
    assert L.fr_version().startswith(b"fr_hotpath 0.4 ")


def test_sizes():
    L = _L()
    assert L.fr_geometry_gram_bytes(199, 29) == 240 * 240 * 8
    assert L.fr_geometry_gram_bytes(0, 0) == 0 and L.fr_geometry_gram_bytes(257, 0) == 0 and L.fr_geometry_gram_bytes(228, 29) == 0
    assert L.fr_geometry_gram_bytes(256, 0) == 256 * 256 * 8 and L.fr_geometry_gram_bytes(0, 1) == 16 * 16 * 8
    assert L.fr_geometry_gram_bytes(-1, 30) == 0 and L.fr_geometry_gram_bytes(30, -1) == 0
    assert L.fr_geometry_gram_bytes((1 << 31) - 1, (1 << 31) - 1) == 0
    for ns, ne in RG.PAIRS:
        kp = (ns + ne + 15) // 16 * 16
        assert L.fr_geometry_gram_bytes(ns, ne) == kp * kp * 8
        for B in (0, 1, 64, 65):
            assert L.fr_geometry_loss_state_bytes(B, ns, ne) == (B * kp + B + 1) * 8
        for N in (1, 341, 342, 53215):
            g = _geom(N, ns, ne)
            assert L.fr_geometry_gram_workspace_bytes(N, ns, ne) == g[1] * g[3] * 256 * 8
    assert L.fr_geometry_loss_state_bytes(-1, 199, 29) == 0 and L.fr_geometry_loss_state_bytes(4, 0, 0) == 0
    assert L.fr_geometry_loss_state_bytes(4, 200, 57) == 0
    assert L.fr_geometry_gram_workspace_bytes(0, 199, 29) == 0 and L.fr_geometry_gram_workspace_bytes(-3, 199, 29) == 0
    assert L.fr_geometry_gram_workspace_bytes(10, 0, 0) == 0 and L.fr_geometry_gram_workspace_bytes(10, 257, 0) == 0


def test_geometry():
    c = _geom(1, 1, 0)[0]
    assert c > 0 and c % 4 == 0                     # whole float64 MFMA steps of four rows
    for N in (1, 5, 341, 342, 683, 53215, 200000, (1 << 31) // 3):
        for ns, ne in RG.PAIRS:
            g = _geom(N, ns, ne)
            tiles = (ns + ne + 15) // 16
            assert g[0] == c, (N, ns, ne)           # the chunk is no function of the shape
            assert g[1] == -(-3 * N // c) and g[4] == g[1]
            assert g[2] == 16 * tiles and g[3] == tiles * (tiles + 1) // 2
            assert 0 < g[5] <= 64 * 1024
    assert _geom(53215, 199, 29)[1:4] == [-(-3 * 53215 // c), 240, 120]
    assert _geom(0, 199, 29) == [0] * 6 and _geom(-1, 199, 29) == [0] * 6 and _geom(5, 0, 0) == [0] * 6
    assert _geom(5, 257, 0) == [0] * 6 and _geom(5, -1, 30) == [0] * 6
    sizes = RG.chunk_edge_sizes(c)
    assert [-(-3 * N // c) for N in sizes] == [1, 1, 1, 2, 3] and 3 * sizes[2] <= c < 3 * sizes[3] and 2 * c < 3 * sizes[4]


# ---- the checks: every single bad argument, and every pair ----------------------------------------------------------------------------
# A defect = (the header's item it trips, the arguments it replaces).  The code a call answers is that of the LOWEST item among
# its defects: 1 -> -1, 2 -> -4, 3 (B == 0) -> 0, 4 -> -1, 5 -> -2.
CODE = {1: -1, 2: -4, 3: 0, 4: -1, 5: -2}
GOOD, ODD = 0x1000, 0x1008          # made-up addresses: 16-byte aligned, and not
BASE = dict(B=3, N=10, ns=7, ne=3)


def _entry_points():
    L = _L()
    nul = ctypes.c_void_p(0)
    sizes = dict(gram_bytes=L.fr_geometry_gram_bytes(7, 3), ws_bytes=L.fr_geometry_gram_workspace_bytes(10, 7, 3),
                 state_bytes=L.fr_geometry_loss_state_bytes(3, 7, 3))
    assert all(v > 0 for v in sizes.values())

    def build(a):
        return L.fr_geometry_gram_build(a["pc_shape"], a["pc_exp"], a["N"], a["ns"], a["ne"], a["gram"], a["gram_bytes"],
                                        a["workspace"], a["ws_bytes"], nul)

    def fwd(a):
        return L.fr_geometry_loss_forward(a["diff"], a["gram"], a["B"], a["N"], a["ns"], a["ne"], a["loss"], a["state"],
                                          a["state_bytes"], nul)

    def bwd(a):
        return L.fr_geometry_loss_backward(a["grad_loss"], a["state"], a["state_bytes"], a["B"], a["N"], a["ns"], a["ne"],
                                           a["grad_diff"], nul)
    sizes_bad = [(1, dict(N=-1)), (1, dict(N=0)), (1, dict(ns=-1)), (1, dict(ne=-1)), (2, dict(ns=0, ne=0)), (2, dict(ns=254)),
                 (2, dict(ne=250))]
    batch_bad = [(1, dict(B=-1)), (3, dict(B=0))]
    eps = {
        "build": (build, dict(pc_shape=GOOD, pc_exp=GOOD, gram=GOOD, workspace=GOOD, **sizes),
                  sizes_bad + [(4, dict(pc_shape=0)), (4, dict(pc_exp=0)), (5, dict(gram=0)), (5, dict(gram=ODD)),
                               (5, dict(gram_bytes=sizes["gram_bytes"] - 1)), (5, dict(workspace=0)), (5, dict(workspace=ODD)),
                               (5, dict(ws_bytes=sizes["ws_bytes"] - 1))]),
        "forward": (fwd, dict(diff=GOOD, gram=GOOD, loss=GOOD, state=GOOD, **sizes),
                    sizes_bad + batch_bad + [(4, dict(diff=0)), (4, dict(loss=0)), (5, dict(gram=0)), (5, dict(gram=ODD)),
                                             (5, dict(state=0)), (5, dict(state=ODD)),
                                             (5, dict(state_bytes=sizes["state_bytes"] - 1))]),
        "backward": (bwd, dict(grad_loss=GOOD, grad_diff=GOOD, state=GOOD, **sizes),
                     sizes_bad + batch_bad + [(4, dict(grad_loss=0)), (4, dict(grad_diff=0)), (5, dict(state=0)),
                                              (5, dict(state=ODD)), (5, dict(state_bytes=sizes["state_bytes"] - 1))]),
    }
    return eps


def _call(fn, base, *defects):
    a = dict(BASE, **base)
    for _, d in defects:
        a.update(d)
    for k in ("pc_shape", "pc_exp", "gram", "workspace", "diff", "loss", "state", "grad_loss", "grad_diff"):
        if k in a:
            a[k] = ctypes.c_void_p(a[k])
    return fn(a)


def test_checks_hold_singly_and_in_pairs():
    """Every call here carries at least one defect, so each returns from the checks: none reaches HIP.  The test SKIPS where a GPU is
    visible, as tests/test_capi_codes_cpu.py does: it checks host code, and if a regression let a case through the checks, the call
    would launch on the made-up addresses."""
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
            want = CODE[min(d1[0], d2[0])]
            assert _call(fn, base, d1, d2) == want, (name, d1, d2, want)
            pairs += 1
    print("held %d single defects and %d pairs over three entry points" % (singles, pairs))
    assert singles >= 40 and pairs >= 250
    # a basis matrix without columns is not read: its NULL pointer is no defect, and such a call gets as far as the buffers
    fn, base, _ = _entry_points()["build"]
    assert _call(fn, base, (0, dict(ns=0, pc_shape=0)), (5, dict(gram=0))) == -2
    assert _call(fn, base, (0, dict(ne=0, pc_exp=0)), (5, dict(workspace=ODD))) == -2
    # B == 0 writes nothing and needs nothing
    fn, base, _ = _entry_points()["forward"]
    assert _call(fn, base, (3, dict(B=0, diff=0, gram=0, loss=0, state=0, state_bytes=0))) == 0
    fn, base, _ = _entry_points()["backward"]
    assert _call(fn, base, (3, dict(B=0, grad_loss=0, grad_diff=0, state=0, state_bytes=0))) == 0


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ns,ne,B", [(5, 7, 3, 3), (342, 17, 16, 4), (700, 199, 29, 2)])
def test_model_vs_the_objectives_restatement(N, ns, ne, B):
    """the chains on numpy's float64 Gram matrix against oracle/losses_np.geometry_loss -- the reference's own form, two float64
    products and their mean squared difference -- to 1e-12 relative; the gradient against central differences of the direct form"""
    pc_shape, pc_exp = RG.basis(N, ns, ne)
    G, _ = RG.gram(pc_shape, pc_exp)
    rs = np.random.RandomState(5)
    label = np.concatenate([np.zeros((B, 7)), rs.uniform(0, 1e4, (B, ns)), rs.uniform(-1.5, 1.5, (B, ne))], 1).astype(np.float32)
    d = RG.diffs(B, ns, ne)
    pred = label.astype(np.float64)
    pred[:, 7:] += d                                   # float64: pred - label is d exactly
    want = LN.geometry_loss(pred, label, pc_shape, pc_exp)
    y, q, S, loss = RG.forward(d, G, N)
    got = S / (3.0 * N * B)
    print("loss %.17g, restatement %.17g, relative difference %.3g" % (got, want, abs(got - want) / want))
    assert abs(got - want) <= 1e-12 * want
    assert loss == np.float32(got) and abs(RG.direct_loss(d, pc_shape, pc_exp) - want) <= 1e-12 * want
    # gradient: the direct form is a quadratic in d, so a central difference is exact up to rounding; step 1e-3 of the entry's scale
    grad = RG.backward(1.0, y, N).astype(np.float64)
    U = RG.U64(pc_shape, pc_exp)
    d64 = d.astype(np.float64)
    worst = 0.0
    for b, k in [(0, 0), (B - 1, ns + ne - 1), (B // 2, (ns + ne) // 2), (0, ns - 1), (B - 1, ns)]:
        h = 1e-3 * (1e4 if k < ns else 3.0)
        vals = []
        for sgn in (1.0, -1.0):
            e = d64.copy()
            e[b, k] += sgn * h
            g = U @ e.T
            vals.append(np.mean(g * g))
        fd = (vals[0] - vals[1]) / (2 * h)
        scale = np.abs(grad[b]).max()
        worst = max(worst, abs(fd - grad[b, k]) / scale)
    print("largest |central difference - model gradient| / max |gradient row|: %.3g (bound 1e-6)" % worst)
    assert worst <= 1e-6                               # fp32 rounding of the gradient gives 6e-8; the difference quotient ~1e-10


def test_python_surface_defaults():
    net, losses = pkg("nets.network"), pkg("nets.losses")
    p = inspect.signature(losses.get_loss).parameters
    assert p["geometry_gram"].default is False and list(p)[-1] == "geometry_gram"
    p = inspect.signature(net.FaceRecNet.geometry_loss).parameters
    assert list(p) == ["self", "geometry_diff", "gram"] and p["gram"].default is False
    assert callable(net.FaceRecNet.gram) and issubclass(net._GeometryGramLoss, torch.autograd.Function)
