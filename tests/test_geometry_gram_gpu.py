"""GPU: the Gram-form geometry loss (csrc/fr_geometry.hip; FaceRecNet.gram / geometry_loss(gram=True); get_loss(geometry_gram=True)).

  1  the Gram build against numpy's float64 U^T U under the header's bound, at every shape on the chunk's edges and once at the full
     mesh: symmetric as bits, pads +0, bit-reproducible, independent of what the buffers held;
  2  the loss and its gradient bit for bit against the model (tests/ref_geometry_gram.py) fed the GPU's own G;
  3  both against the float64 truth mean((U d)^2), and the product route beside them;
  4  a NaN in one face's diff;
  5  the operator and the objective's flag, on and off;
  6  two host threads on two streams.
The shapes come from the build's own chunk constant (fr_debug_geometry_gram_geom), not from a re-derivation."""
import ctypes
import functools
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import assert_bits_equal
import ref_geometry_gram as RG

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _h():
    return pkg("_lib")


def _chunk():
    out = (ctypes.c_int * 6)()
    _h().lib().fr_debug_geometry_gram_geom(1, 1, 0, out)
    return out[0]


CASES = RG.cases(_chunk())
LOSS_N = RG.chunk_edge_sizes(_chunk())[3]          # the loss kernels see N in their denominators alone: one N, every K


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a):
    """a device tensor of `a` that owns at least 16 bytes (an empty basis matrix is passed as a valid pointer that is never read)"""
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if t.numel() else torch.zeros((4,), dtype=t.dtype, device=DEV)


def build_gram(pc_shape, pc_exp, fill=None, G=None, ws=None):
    """fr_geometry_gram_build through the raw C ABI -> G [Kp,Kp] float64 (numpy).  fill: a byte both buffers are filled with first.
    G, ws: uint8 device tensors of exactly the stated sizes to build into, as the caller placed and filled them."""
    h = _h()
    L = h.lib()
    N, ns, ne = pc_shape.shape[0] // 3, pc_shape.shape[1], pc_exp.shape[1]
    nb, nws = L.fr_geometry_gram_bytes(ns, ne), L.fr_geometry_gram_workspace_bytes(N, ns, ne)
    kp = (ns + ne + 15) // 16 * 16
    assert nb == kp * kp * 8 and nws > 0
    mk = (lambda n: torch.full((n,), fill, dtype=torch.uint8, device=DEV)) if fill is not None else \
        (lambda n: torch.empty((n,), dtype=torch.uint8, device=DEV))
    G, ws = mk(nb) if G is None else G, mk(nws) if ws is None else ws
    assert G.numel() == nb and ws.numel() == nws
    ps, pe = _dev(pc_shape), _dev(pc_exp)
    rc = L.fr_geometry_gram_build(h.ptr(ps), h.ptr(pe), N, ns, ne, h.ptr(G), nb, h.ptr(ws), nws, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return G.view(torch.float64).reshape(kp, kp).cpu().numpy()


@functools.lru_cache(maxsize=None)
def rig(N, ns, ne):
    """(pc_shape, pc_exp, the GPU's G) of a shape: built once, shared by every test, never written"""
    pc_shape, pc_exp = RG.basis(N, ns, ne)
    G = build_gram(pc_shape, pc_exp)
    G.setflags(write=False)
    return pc_shape, pc_exp, G


def loss_fwd_bwd(G, diff, N, ns, ne, grad_losses=(1.0,), stream=None, state=None):
    """fr_geometry_loss_forward + one fr_geometry_loss_backward per grad_loss through the raw C ABI -> (loss fp32, [grad_diff])"""
    h = _h()
    L = h.lib()
    B = diff.shape[0]
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(DEV)).cuda_stream)
    Gt, dt = torch.tensor(G, device=DEV), torch.as_tensor(diff, device=DEV)      # (G may be read-only: a copy)
    nst = L.fr_geometry_loss_state_bytes(B, ns, ne)
    if state is None:
        state = torch.full((nst,), 0xFF, dtype=torch.uint8, device=DEV)
    assert state.dtype == torch.uint8 and state.numel() == nst
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    assert L.fr_geometry_loss_forward(h.ptr(dt), h.ptr(Gt), B, N, ns, ne, h.ptr(loss), h.ptr(state), nst, st) == 0
    grads = []
    for gl in grad_losses:
        g = torch.tensor(gl, dtype=torch.float32, device=DEV)
        gd = torch.full((B, ns + ne), float("nan"), dtype=torch.float32, device=DEV)
        assert L.fr_geometry_loss_backward(h.ptr(g), h.ptr(state), nst, B, N, ns, ne, h.ptr(gd), st) == 0
        grads.append(gd)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), [g.cpu().numpy() for g in grads]


# ---- 1: the Gram matrix ---------------------------------------------------------------------------------------------------------------
def _check_gram(G, pc_shape, pc_exp, tag):
    K = pc_shape.shape[1] + pc_exp.shape[1]
    want, bound = RG.gram(pc_shape, pc_exp)
    err = np.abs(G[:K, :K] - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: largest |G - U64.T @ U64| / bound = %.3g" % (tag, ratio))
    assert np.isfinite(G).all(), tag
    assert (err <= bound).all(), (tag, ratio)
    assert np.array_equal(G.view(np.uint64), G.T.copy().view(np.uint64)), tag            # symmetric as bits
    pad = np.ones(G.shape, bool)
    pad[:K, :K] = False
    assert not G.view(np.uint64)[pad].any(), tag                                         # pads: +0, not -0
    assert np.abs(np.diag(G)[:K]).min() > 0, tag


@pytest.mark.parametrize("case", CASES, ids=RG.case_id)
def test_gram_vs_float64(case):
    pc_shape, pc_exp, G = rig(*case)
    _check_gram(G, pc_shape, pc_exp, RG.case_id(case))
    again = build_gram(pc_shape, pc_exp)
    assert np.array_equal(again.view(np.uint64), G.view(np.uint64))                      # two builds
    filled = build_gram(pc_shape, pc_exp, fill=0xFF)
    assert np.array_equal(filled.view(np.uint64), G.view(np.uint64))                     # buffers that held 0xFF bytes


@pytest.fixture(scope="module")
def full_net(full_assets):
    return pkg("nets.network").FaceRecNet(mesh_data=full_assets, batch_size=1, im_size=200)


def test_gram_full_mesh(full_assets, full_net):
    A = full_assets
    pc_shape, pc_exp = np.asarray(A["pc_shape"], np.float32), np.asarray(A["pc_exp"], np.float32)
    assert pc_shape.shape == (3 * 53215, 199) and pc_exp.shape == (3 * 53215, 29)
    G = full_net.gram()
    assert G.dtype == torch.float64 and tuple(G.shape) == (240, 240) and full_net.gram() is G
    Gn = G.cpu().numpy()
    _check_gram(Gn, pc_shape, pc_exp, "full mesh")
    assert np.array_equal(build_gram(pc_shape, pc_exp, fill=0xFF).view(np.uint64), Gn.view(np.uint64))


def test_gram_pads_with_a_non_finite_basis():
    """pads are +0 whatever the basis holds; a NaN entry reaches its own row and column of G alone"""
    N, ns, ne = 5, 7, 3
    pc_shape, pc_exp = (a.copy() for a in RG.basis(N, ns, ne))
    pc_shape[4, 2] = np.nan
    pc_exp[9, 1] = np.inf
    G = build_gram(pc_shape, pc_exp)
    K = ns + ne
    pad = np.ones(G.shape, bool)
    pad[:K, :K] = False
    assert not G.view(np.uint64)[pad].any()
    clean = np.ones((K, K), bool)
    clean[[2, ns + 1], :] = False
    clean[:, [2, ns + 1]] = False
    ref = rig(N, ns, ne)[2]
    assert np.array_equal(G[:K, :K][clean].view(np.uint64), ref[:K, :K][clean].view(np.uint64))
    assert not np.isfinite(G[2, :K]).any() and not np.isfinite(G[ns + 1, :K]).any()


# ---- 2, 3: the loss and its gradient ----------------------------------------------------------------------------------------------
def _check_loss(pc_shape, pc_exp, G, B, tag):
    """bit for bit against the model on the GPU's G; then against the truth"""
    N, ns, ne = pc_shape.shape[0] // 3, pc_shape.shape[1], pc_exp.shape[1]
    K = ns + ne
    d = RG.diffs(B, ns, ne)
    loss, grads = loss_fwd_bwd(G, d, N, ns, ne, RG.GRAD_LOSSES)
    y, q, S, want_loss = RG.forward(d, G, N)
    assert_bits_equal(loss, want_loss, tag + " loss")
    for gl, g in zip(RG.GRAD_LOSSES, grads):
        assert_bits_equal(g, RG.backward(gl, y, N), "%s grad_diff at grad_loss %g" % (tag, gl))
    # the truth: mean((U d)^2) and (2 / (3N B)) U^T U d in float64
    truth = RG.direct_loss(d, pc_shape, pc_exp)
    rel = abs(float(loss) - truth) / truth
    U = RG.U64(pc_shape, pc_exp)
    d64 = d.astype(np.float64)
    Gx = U.T @ U
    c = 2.0 / (3.0 * N * B)
    want = c * (d64 @ Gx)
    bound = 2.0 ** -24 * np.abs(want) + (K + 3 * N) * 2.0 ** -52 * (np.abs(d64) @ np.abs(Gx)) * c
    err = np.abs(grads[0].astype(np.float64) - want)
    print("%s: loss %.9g, |loss - truth| / truth = %.3g (bound 2^-23 = 1.19e-07); largest gradient error / bound = %.3g"
          % (tag, float(loss), rel, float((err / np.maximum(bound, 1e-300)).max())))
    assert truth > 0 and rel <= 2.0 ** -23
    assert (err <= bound).all()
    assert np.abs(grads[0]).max() > 0


@pytest.mark.parametrize("B", RG.BATCHES)
@pytest.mark.parametrize("ns,ne", RG.PAIRS)
def test_loss_and_gradient_bits_and_truth(ns, ne, B):
    pc_shape, pc_exp, G = rig(LOSS_N, ns, ne)
    _check_loss(pc_shape, pc_exp, G, B, "N%d-%d+%d B=%d" % (LOSS_N, ns, ne, B))


@pytest.mark.parametrize("N", [n for n in RG.chunk_edge_sizes(_chunk()) if n != LOSS_N])
def test_loss_at_the_other_sizes(N):
    pc_shape, pc_exp, G = rig(N, 17, 16)
    _check_loss(pc_shape, pc_exp, G, 3, "N%d-17+16 B=3" % N)


def test_loss_full_mesh_and_the_product_route(full_assets, full_net):
    """64 faces of the full mesh: the model's bits, the truth, and the product route on the same input inside its own tolerance
    (tests/test_losses_gpu.py: 1e-5 relative on the loss), so the two routes agree to that"""
    A = full_assets
    pc_shape, pc_exp = np.asarray(A["pc_shape"], np.float32), np.asarray(A["pc_exp"], np.float32)
    G = full_net.gram().cpu().numpy()
    _check_loss(pc_shape, pc_exp, G, 64, "full mesh B=64")
    d = RG.diffs(5, 199, 29)
    truth = RG.direct_loss(d, pc_shape, pc_exp)
    x = torch.as_tensor(d, device=DEV)
    prod = float(full_net.geometry_loss(x))
    gram = float(full_net.geometry_loss(x, gram=True))
    print("5 faces: truth %.9g, product route %.9g (%.3g relative), Gram route %.9g (%.3g relative)"
          % (truth, prod, abs(prod - truth) / truth, gram, abs(gram - truth) / truth))
    assert abs(prod - truth) <= 1e-5 * truth and abs(gram - truth) <= 2.0 ** -23 * truth


# ---- 4: non-finite ----------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_face():
    N, ns, ne, B = LOSS_N, 17, 16, 5
    pc_shape, pc_exp, G = rig(N, ns, ne)
    d = RG.diffs(B, ns, ne)
    clean_loss, (clean,) = loss_fwd_bwd(G, d, N, ns, ne)
    bad = d.copy()
    bad[2, 11] = np.nan
    loss, (g,) = loss_fwd_bwd(G, bad, N, ns, ne)
    assert np.isnan(loss) and np.isnan(g[2]).all() and np.isfinite(clean_loss)
    y, _, _, want_loss = RG.forward(bad, G, N)
    assert np.isnan(want_loss)
    others = [0, 1, 3, 4]
    assert_bits_equal(g[others], RG.backward(1.0, y, N)[others], "rows of the other faces")
    assert_bits_equal(g[others], clean[others], "rows of the other faces against the clean call")


# ---- 5: the operator and the objective ------------------------------------------------------------------------------------------------
def _same(a, b):
    return bool((a.detach().view(torch.int32) == b.detach().view(torch.int32)).all())


def test_operator_and_get_loss(small_assets):
    netm, Ls = pkg("nets.network"), pkg("nets.losses")
    A = small_assets
    B, S = 4, 40
    ns, ne = A["ndim_shape"], A["ndim_exp"]
    N = np.asarray(A["mu"]).size // 3
    rs = np.random.RandomState(3)
    P = np.zeros((B, 7 + ns + ne), np.float32)
    P[:, 0:3] = rs.uniform(-1.0, 1.0, (B, 3))
    P[:, 3:5] = rs.uniform(17, 23, (B, 2))
    P[:, 6] = rs.uniform(1.6e-4, 2.2e-4, B)
    P[:, 7:] = np.concatenate([rs.uniform(0, 1e4, (B, ns)), rs.uniform(-1.5, 1.5, (B, ne))], 1)
    lab = P + rs.standard_normal(P.shape).astype(np.float32) * np.array([0.1] * 3 + [2, 2, 0, 1e-5] + [300.0] * (ns + ne), np.float32)
    label = torch.as_tensor(lab, device=DEV)
    im = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(1)).to(DEV)

    def run(net, **kw):
        pred = torch.as_tensor(P, device=DEV).requires_grad_(True)
        with torch.no_grad():
            V = net.vertices_transform(pred)
            coarse = net.coarse_net_input(V, im_gray=im)[1]
        out = Ls.get_loss(net, pred, label, im, V, coarse, coarse.clone(), **kw)
        out["geometry_loss"].backward()
        torch.cuda.synchronize()
        return out, pred.grad

    on_net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S)
    on, g_on = run(on_net, geometry_gram=True)
    assert on_net._basis_nomu is None and on_net._gram is not None            # the second image was never built
    assert on["geometry_loss"].dim() == 0 and on["geometry_loss"].dtype == torch.float32
    # ... as the model says, on the operator's own G and the fp32 difference torch formed
    G = on_net.gram().cpu().numpy()
    d = (torch.as_tensor(P, device=DEV)[:, 7:] - label[:, 7:]).cpu().numpy()
    y, _, _, want = RG.forward(d, G, N)
    assert_bits_equal(on["geometry_loss"].detach().cpu().numpy(), want, "get_loss(geometry_gram=True)")
    gw = RG.backward(1.0, y, N)
    assert_bits_equal(g_on[:, 7:].cpu().numpy(), gw, "pred.grad")
    assert not g_on[:, :7].any()
    pc_shape, pc_exp = np.asarray(A["pc_shape"], np.float32), np.asarray(A["pc_exp"], np.float32)
    truth = RG.direct_loss(d, pc_shape, pc_exp)
    assert abs(float(on["geometry_loss"]) - truth) <= 2.0 ** -23 * truth
    # the label side: d / d label = -d / d pred, through torch's subtraction
    pred = torch.as_tensor(P, device=DEV)
    lab_t = label.clone().requires_grad_(True)
    on_net.geometry_loss(pred[:, 7:] - lab_t[:, 7:], gram=True).backward()
    assert_bits_equal(lab_t.grad[:, 7:].cpu().numpy(), -gw, "label.grad")
    # a scaled loss: grad_loss arrives as a device scalar
    x = torch.as_tensor(d, device=DEV).requires_grad_(True)
    (on_net.geometry_loss(x, gram=True) * -0.37).backward()
    assert_bits_equal(x.grad.cpu().numpy(), RG.backward(-0.37, y, N), "grad at grad_loss -0.37")
    # two forwards in flight before their backwards: each node owns its state
    x1 = torch.as_tensor(d, device=DEV).requires_grad_(True)
    x2 = torch.as_tensor(d[::-1].copy(), device=DEV).requires_grad_(True)
    l1, l2 = on_net.geometry_loss(x1, gram=True), on_net.geometry_loss(x2, gram=True)
    l1.backward()
    l2.backward()
    assert_bits_equal(x1.grad.cpu().numpy(), gw, "first of two in flight")
    assert_bits_equal(x2.grad.cpu().numpy(), RG.backward(1.0, RG.forward(d[::-1], G, N)[0], N), "second of two in flight")
    assert sum(len(v) for v in on_net._gram_state.values()) <= 4

    # the flag off: today's expression, bit for bit, and the second image is built as today
    off_net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S)
    off, g_off = run(off_net)
    off2, g_off2 = run(off_net, geometry_gram=False)
    assert off_net._basis_nomu is not None and off_net._gram is None
    x = torch.as_tensor(d, device=DEV)
    want_off = (off_net.geometry_product(x) ** 2).mean()
    assert _same(off_net.geometry_loss(x), want_off) and _same(off_net.geometry_loss(x, gram=False), want_off)
    assert _same(off["geometry_loss"], want_off) and _same(off2["geometry_loss"], want_off) and _same(g_off, g_off2)
    assert abs(float(want_off) - truth) <= 1e-5 * truth                        # the two routes agree to the product route's tolerance
    for k in ("pose_loss", "fidelity_loss", "smoothness_loss"):
        assert _same(on[k], off[k]), k
    # an empty batch takes the product route, whatever that makes of it
    calls, product = [], on_net.geometry_product
    on_net.geometry_product = lambda x: calls.append(int(x.shape[0])) or product(x)
    try:
        on_net.geometry_loss(torch.zeros((0, ns + ne), device=DEV), gram=True)
    except (RuntimeError, ValueError):
        pass
    assert calls == [0]


# ---- 6: threads -----------------------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams():
    """two host threads, a stream and a state each, one shared G: the single-thread bits (the pattern of tests/test_threads_gpu.py)"""
    N, ns, ne = LOSS_N, 199, 29
    _, _, G = rig(N, ns, ne)
    jobs = [(RG.diffs(64, ns, ne, seed=1), 1.0), (RG.diffs(3, ns, ne, seed=2), -0.37)]
    refs = [loss_fwd_bwd(G, d, N, ns, ne, (gl,)) for d, gl in jobs]
    for (d, gl), (loss, (g,)) in zip(jobs, refs):
        y, _, _, want = RG.forward(d, G, N)
        assert_bits_equal(loss, want, "single-thread loss")
        assert_bits_equal(g, RG.backward(gl, y, N), "single-thread gradient")
    streams = [torch.cuda.Stream(device=DEV) for _ in jobs]
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(jobs))

    def worker(i):
        bad = []
        barrier.wait(timeout=60)
        d, gl = jobs[i]
        with torch.cuda.stream(streams[i]):
            for it in range(20):
                loss, (g,) = loss_fwd_bwd(G, d, N, ns, ne, (gl,), stream=streams[i])
                if loss.view(np.uint32) != refs[i][0].view(np.uint32) or not np.array_equal(g.view(np.uint32), refs[i][1][0].view(np.uint32)):
                    bad.append("thread %d iteration %d" % (i, it))
        return bad

    ex = ThreadPoolExecutor(max_workers=len(jobs))
    try:
        futs = [ex.submit(worker, i) for i in range(len(jobs))]
        bad = sum((f.result(timeout=180) for f in futs), [])
    finally:
        ex.shutdown(wait=False, cancel_futures=True)
    assert not bad, bad[:10]
