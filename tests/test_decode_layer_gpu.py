"""GPU: the differentiable decode -> rendering-layer step (include/fr_hotpath.h).

Forward: fr_decode_rendering_layer_forward against fr_decode_3dmm -> fr_rendering_layer_forward, bit for bit, and against the
CPU oracle chain.  Backward: fr_decode_render_backward against the composed chain on the same inputs -- the torch expression of
_RenderingLayerFused.backward -> fr_render_depth_backward_ws -> fr_decode_3dmm_backward_packed_mu -- bit for bit (the identity is
derived: the same fixed-point sums give the same z values, dv is the identical expression with +0 / -0 for the absent rows, and
the pose partials only add signed zeros to +0), and against a float64 evaluation.  Then the autograd node, CoarseNet's
`fused_step`, and two host threads.  Every figure a tolerance is applied to is printed before it is asserted."""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import net_mod, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _seeded():
    torch.manual_seed(1234)      # (device-side torch.rand inputs: the same ones every run)


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


class Rig:
    """One mesh + basis on the GPU and the raw C-ABI calls of both routes."""

    def __init__(self, A, H, W, im_size=None):
        self.A, self.H, self.W = A, H, W
        self.im_size = float(H if im_size is None else im_size)
        self.net = net_mod().FaceRecNet(mesh_data=A, batch_size=1, im_size=int(self.im_size))
        n = self.net
        self.N, self.ns, self.ne, self.ntri = n.nvert, n.ndim_shape, n.ndim_exp, int(n.tri.shape[1])
        self.nd = 7 + self.ns + self.ne
        self.image_t = n._basis.image_t()
        assert self.image_t is not None

    # ---- forward ----
    def _planes(self, B):
        o = dict(dtype=torch.float32, device=DEV)
        return (torch.full((B, self.H, self.W, 7), 7.0, **o), torch.full((B, self.H, self.W, 1), 7.0, **o),
                torch.full((B, self.H, self.W, 1), 7.0, **o), torch.full((B, self.H, self.W, 1), 7.0, **o))

    def fwd_fused(self, P, im, phases=(15,), R=None, tex=None, expect=0, ws=None, hand=None):
        """ws, hand: uint8 device tensors of exactly the stated sizes to use in place of the call's own"""
        h, L, n = _h(), _h().lib(), self.net
        B = int(P.shape[0])
        tex = n.vertex_code if tex is None else tex
        tb = 1 if tex.dim() == 2 else int(tex.shape[0])
        nws = L.fr_render_depth_workspace_bytes(B, self.N, self.ntri, self.H, self.W)
        nh = L.fr_decode_render_vertex_bytes(B, self.N)
        assert (ws is None or ws.numel() == nws) and (hand is None or hand.numel() == nh)       # (exactly the stated bytes)
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV) if ws is None else ws
        hand = torch.empty((nh,), dtype=torch.uint8, device=DEV) if hand is None else hand
        outs = self._planes(B)
        for ph in phases:
            rc = L.fr_decode_rendering_layer_forward(h.ptr(P), h.ptr(n._basis.image), h.ptr(R), h.ptr(n.tri), h.ptr(tex), h.ptr(im),
                                                     B, self.N, self.ns, self.ne, self.ntri, self.H, self.W, tb, self.im_size,
                                                     h.ptr(hand), nh, *[h.ptr(o) for o in outs], h.ptr(ws), nws, _stream(), ph)
            assert rc == expect, (rc, ph)
        torch.cuda.synchronize()
        return outs

    def fwd_chain(self, P, im, R=None, tex=None):
        h, L, n = _h(), _h().lib(), self.net
        B = int(P.shape[0])
        tex = n.vertex_code if tex is None else tex
        tb = 1 if tex.dim() == 2 else int(tex.shape[0])
        V = torch.empty((B, 3, self.N), dtype=torch.float32, device=DEV)
        assert L.fr_decode_3dmm(h.ptr(P), h.ptr(n._basis.image), h.ptr(R), B, self.N, self.ns, self.ne, self.im_size, h.ptr(V),
                                _stream()) == 0
        nws = L.fr_render_depth_workspace_bytes(B, self.N, self.ntri, self.H, self.W)
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
        outs = self._planes(B)
        assert L.fr_rendering_layer_forward(h.ptr(V), h.ptr(n.tri), h.ptr(tex), h.ptr(im), B, self.N, self.ntri, self.H, self.W, tb,
                                            *[h.ptr(o) for o in outs], h.ptr(ws), nws, _stream()) == 0
        torch.cuda.synchronize()
        return outs

    # ---- backward ----
    def bwd_fused(self, P, gd, gi, gn, im, depth, tri_ind, R=None, ws=None):
        h, L, n = _h(), _h().lib(), self.net
        B = int(P.shape[0])
        nws = L.fr_decode_render_backward_workspace_bytes(B, self.N, self.ns, self.ne, self.H, self.W)
        assert nws > 0
        ws = torch.empty((nws,), dtype=torch.uint8, device=DEV) if ws is None else ws
        assert ws.numel() == nws
        gp = torch.full((B, self.nd), 7.0, dtype=torch.float32, device=DEV)
        rc = L.fr_decode_render_backward(h.ptr(gd), h.ptr(gi), h.ptr(gn), h.ptr(im), h.ptr(depth), h.ptr(n.tri), h.ptr(tri_ind),
                                         h.ptr(P), h.ptr(n.mu), h.ptr(self.image_t), h.ptr(R), B, self.N, self.ns, self.ne,
                                         self.ntri, self.H, self.W, self.im_size, h.ptr(gp), h.ptr(ws), nws, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return gp

    @staticmethod
    def pixel_grad(gd, gi, gn, im, depth):
        """the torch expression of rendering_layer/ops.py::_RenderingLayerFused.backward"""
        dg = torch.zeros_like(depth)
        if gn is not None:
            dg = dg + gn[..., 0:1] * im * ((depth >= 1e-6) & (depth <= 1.0)).to(depth.dtype)
        if gi is not None:
            dg = dg + gi * (depth >= 1e-6).to(depth.dtype)
        if gd is not None:
            dg = dg + gd
        return dg.contiguous()

    def bwd_chain(self, P, gd, gi, gn, im, depth, tri_ind, R=None):
        """-> (grad_params, pixel gradient, vertex gradient [B,3,N]) of the composed chain"""
        h, L, n = _h(), _h().lib(), self.net
        B = int(P.shape[0])
        dg = self.pixel_grad(gd, gi, gn, im, depth)
        vg = torch.full((B, 3, self.N), 7.0, dtype=torch.float32, device=DEV)
        nrw = L.fr_render_depth_backward_workspace_bytes(B, self.H, self.W)
        rws = torch.empty((nrw,), dtype=torch.uint8, device=DEV)
        assert L.fr_render_depth_backward_ws(h.ptr(dg), h.ptr(n.tri), h.ptr(tri_ind), h.ptr(vg), B, self.N, self.ntri, self.H,
                                             self.W, h.ptr(rws), nrw, _stream()) == 0
        ndw = L.fr_decode_backward_workspace_bytes(B, self.N, self.ns, self.ne)
        dws = torch.empty((ndw,), dtype=torch.uint8, device=DEV)
        gp = torch.full((B, self.nd), 7.0, dtype=torch.float32, device=DEV)
        assert L.fr_decode_3dmm_backward_packed_mu(h.ptr(vg), h.ptr(P), h.ptr(n.mu), h.ptr(self.image_t), h.ptr(R), B, self.N,
                                                   self.ns, self.ne, self.im_size, h.ptr(gp), h.ptr(dws), ndw, _stream()) == 0
        torch.cuda.synchronize()
        return gp, dg, vg


@pytest.fixture(scope="module")
def full(full_assets):
    return Rig(full_assets, 200, 200)


@pytest.fixture(scope="module")
def mid(synth):
    # N = 187: N % 16 = 11 (a clamped last vertex group), N % 32 != 0; 217 coefficients; H != W
    A = synth.make_assets(11, 17, 200, 17, patch=None, seed_basis=187)
    return Rig(A, 37, 53, im_size=45)


def _params(synth, rig, B, seed):
    P = synth.sample_params_batch(B, im_size=int(rig.im_size), n_shape=rig.ns, n_exp=rig.ne, beta=0.7, seed=seed)
    if rig.N < 1000:   # the tiny mesh is a few pixels wide at f ~ 1e-3 * im / 200: scale it up so that it covers pixels
        P[:, 6] = np.float32(2.5e-4) * (1.0 + 0.1 * np.arange(B) % 3)
        P[:, 3] = rig.W / 2.0
        P[:, 4] = rig.im_size - rig.H / 2.0
    return _t(P)


def _scene(synth, rig, B, seed):
    """params, im_gray, the forward's planes and random gradients for all three inputs"""
    P = _params(synth, rig, B, seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    im = torch.rand((B, rig.H, rig.W, 1), generator=g).to(DEV)
    net_in, depth_img, depth, tri_ind = rig.fwd_fused(P, im)
    gd = torch.randn((B, rig.H, rig.W, 1), generator=g).to(DEV)
    gi = torch.randn((B, rig.H, rig.W, 1), generator=g).to(DEV)
    gn = torch.randn((B, rig.H, rig.W, 7), generator=g).to(DEV)
    return P, im, depth, tri_ind, gd, gi, gn


# ---- 1. forward, bit for bit ------------------------------------------------------------------------------------------------
def _oracle_forward(oracle, rig, P, im, faces, got, tex=None, R=None):
    A = rig.A
    Pn, imn = P.cpu().numpy(), im.cpu().numpy()
    net_in, depth_img, depth, tri_ind = (g.cpu().numpy() for g in got)
    texn = A["vertex"][None] if tex is None else tex.cpu().numpy()
    for b in faces:
        Rb = None if R is None else R[b:b + 1].cpu().numpy()
        V = oracle.decode_3dmm(Pn[b:b + 1], A["mu"], A["pc_shape"], A["pc_exp"], rig.im_size, R=Rb)
        tb = texn if texn.shape[0] == 1 else texn[b:b + 1]
        d, tx, _, ti = oracle.render_depth(V, A["tri"], tb, rig.H, rig.W)
        np.testing.assert_array_equal(depth[b:b + 1], d)
        np.testing.assert_array_equal(tri_ind[b:b + 1], ti)
        np.testing.assert_array_equal(net_in[b:b + 1, ..., 1:4], np.clip(tx, np.float32(1e-6), np.float32(1.0)))
        np.testing.assert_array_equal(net_in[b:b + 1, ..., 0:1], np.clip(d, np.float32(1e-6), np.float32(1.0)) * imn[b:b + 1])
        np.testing.assert_array_equal(depth_img[b:b + 1], np.maximum(d, np.float32(1e-6)))


@pytest.mark.parametrize("B", [3, 64])
def test_forward_full_size(oracle, synth, full, B):
    """The full-size mesh: the one call against the two calls, every plane bit for bit; depth, tri_ind and the clamp channels
    against the CPU oracle chain (every face at B = 3; the first, a middle and the last face at B = 64 -- the faces of a batch
    are independent in every kernel of the chain, and the oracle renders one face in about a second)."""
    P = _params(synth, full, B, seed=21 + B)
    im = torch.rand((B, 200, 200, 1), device=DEV)
    got = full.fwd_fused(P, im)
    want = full.fwd_chain(P, im)
    for g, w, name in zip(got, want, ("net_input", "depth_img", "depth", "tri_ind")):
        assert _same(g, w), name
    cov = float((got[3] >= 0).float().mean())
    print("covered pixels: %.1f %%" % (100 * cov))
    assert cov >= 0.20                                         # non-vacuity (the CPU oracle gives 22.6 - 41.9 % over four faces)
    _oracle_forward(oracle, full, P, im, range(B) if B <= 3 else (0, B // 2, B - 1), got)


def test_forward_small_odd_shapes_texture_phases_and_hint(oracle, synth, mid):
    B = 5
    P = _params(synth, mid, B, seed=3)
    im = torch.rand((B, mid.H, mid.W, 1), device=DEV)
    R = _t(oracle.rotation_matrix_batch(P[:, :3].cpu().numpy() * 0.5))
    got = mid.fwd_fused(P, im)
    assert float((got[3] >= 0).float().mean()) > 0.05
    for g, w in zip(got, mid.fwd_chain(P, im)):
        assert _same(g, w)
    _oracle_forward(oracle, mid, P, im, range(B), got)
    # a caller-computed rotation
    gotR = mid.fwd_fused(P, im, R=R)
    for g, w in zip(gotR, mid.fwd_chain(P, im, R=R)):
        assert _same(g, w)
    _oracle_forward(oracle, mid, P, im, range(B), gotR, R=R)
    assert not _same(gotR[2], got[2])
    # per-face texture
    tex = torch.rand((B, 3, mid.N), device=DEV)
    gotT = mid.fwd_fused(P, im, tex=tex)
    for g, w in zip(gotT, mid.fwd_chain(P, im, tex=tex)):
        assert _same(g, w)
    _oracle_forward(oracle, mid, P, im, range(B), gotT, tex=tex)
    # pack once (4), then decode + emit + resolve (11), against everything at once (15); the phases one by one
    for phases in ((4, 11), (4, 8, 1, 2), (12, 3)):
        for g, w in zip(mid.fwd_fused(P, im, phases=phases), got):
            assert _same(g, w), phases
    # a strip-height hint changes no bit (passed with every phase of the workspace)
    rows = _h().lib().fr_render_depth_strip_rows(B, mid.ntri, mid.H, mid.W)
    assert rows > 0
    for hint in (rows + 3, max(4, rows - 1)):
        for g, w in zip(mid.fwd_fused(P, im, phases=(4 | (hint << 8), 11 | (hint << 8))), got):
            assert _same(g, w), hint


def test_forward_hint_and_phases_full_size(synth, full):
    B = 3
    P = _params(synth, full, B, seed=8)
    im = torch.rand((B, 200, 200, 1), device=DEV)
    got = full.fwd_fused(P, im)
    for phases in ((4, 11), (4 | (8 << 8), 11 | (8 << 8))):
        for g, w in zip(full.fwd_fused(P, im, phases=phases), got):
            assert _same(g, w), phases


def test_forward_unsupported_under_the_scan_rasteriser(synth, mid):
    B = 2
    P = _params(synth, mid, B, seed=4)
    im = torch.rand((B, mid.H, mid.W, 1), device=DEV)
    with _h().options(FR_RENDER_IMPL=1):
        outs = mid.fwd_fused(P, im, expect=-4)
        assert all(float(o.min()) == 7.0 and float(o.max()) == 7.0 for o in outs)      # nothing was launched
        # ... and the Python surface composes the two-step route instead
        ni, di = mid.net.decode_rendering_layer(P, im_gray=im)
        ni2, di2 = mid.net.coarse_net_input(mid.net.vertices_transform(P), im_gray=im)
        assert _same(ni, ni2) and _same(di, di2)
    ni3, di3 = mid.net.decode_rendering_layer(P, im_gray=im)
    assert _same(ni3[..., 0:4], ni[..., 0:4]) and _same(di3, di)


# ---- 2. backward, bit for bit -----------------------------------------------------------------------------------------------
def _bwd_both(rig, P, gd, gi, gn, im, depth, tri_ind, R=None):
    got = rig.bwd_fused(P, gd, gi, gn, im, depth, tri_ind, R=R)
    again = rig.bwd_fused(P, gd, gi, gn, im, depth, tri_ind, R=R)
    want, dg, vg = rig.bwd_chain(P, gd, gi, gn, im, depth, tri_ind, R=R)
    assert _same(got, again)                                   # run to run
    assert bool(torch.isfinite(got).all())
    assert _same(got, want), int((_bits(got) != _bits(want)).sum())
    return got, dg, vg


@pytest.mark.parametrize("B", [1, 16, 32, 48, 64, 70])
def test_backward_product_shape(synth, full, B):
    P, im, depth, tri_ind, gd, gi, gn = _scene(synth, full, B, seed=100 + B)
    assert float((tri_ind >= 0).float().mean()) >= 0.20
    got, dg, vg = _bwd_both(full, P, gd, gi, gn, im, depth, tri_ind)
    assert float(got.abs().max()) > 0 and float(got[:, 5].abs().min()) > 0 and float(got[:, 7:].abs().max()) > 0
    assert float(vg[:, :2].abs().max()) == 0.0                 # what the composed chain carries as zeros


SUBSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


@pytest.mark.parametrize("rig_name,B", [("full", 3), ("mid", 5)])
def test_backward_every_subset_of_the_gradient_planes(synth, request, rig_name, B):
    rig = request.getfixturevalue(rig_name)
    P, im, depth, tri_ind, gd, gi, gn = _scene(synth, rig, B, seed=7)
    seen = []
    for a, b, c in SUBSETS:
        got, _, _ = _bwd_both(rig, P, gd if a else None, gi if b else None, gn if c else None, im, depth, tri_ind)
        assert float(got.abs().max()) > 0
        seen.append(got)
    assert not _same(seen[0], seen[1]) and not _same(seen[0], seen[2]) and not _same(seen[3], seen[6])


def test_backward_R_override_mid_mesh_and_zero_focal(oracle, synth, full, mid):
    for rig, B in ((mid, 70), (mid, 5), (full, 3)):
        P, im, depth, tri_ind, gd, gi, gn = _scene(synth, rig, B, seed=31 + B)
        R = _t(oracle.rotation_matrix_batch(P[:, :3].cpu().numpy() * 0.5))
        a, _, _ = _bwd_both(rig, P, gd, gi, gn, im, depth, tri_ind)
        b, _, _ = _bwd_both(rig, P, gd, gi, gn, im, depth, tri_ind, R=R)
        assert not _same(a, b)
        # a face with f == 0 (the planes are those of the rendered scene: the backward takes its parameters as given)
        P0 = P.clone()
        P0[min(1, B - 1), 6] = 0.0
        z, _, _ = _bwd_both(rig, P0, gd, gi, gn, im, depth, tri_ind)
        k = min(1, B - 1)
        assert float(z[k, 6]) == 0.0 and float(z[k, 7:].abs().max()) == 0.0
        keep = [i for i in range(B) if i != k]
        assert _same(z[keep], a[keep])


@pytest.mark.parametrize("chunks", [1, 7, 256, 512])
@pytest.mark.parametrize("cb", [2, 4])
def test_backward_under_the_launch_knobs(synth, full, mid, chunks, cb):
    with _h().options(FR_BWD_CHUNKS=chunks, FR_BWD_CB=cb):
        for rig, B in ((mid, 70), (mid, 3)) + (((full, 17),) if chunks >= 256 else ((full, 2),)):
            P, im, depth, tri_ind, gd, gi, gn = _scene(synth, rig, B, seed=chunks + cb + B)
            _bwd_both(rig, P, gd, gi, gn, im, depth, tri_ind)


# ---- 3. thresholds -----------------------------------------------------------------------------------------------------------
def test_backward_thresholds(synth, full):
    """A rendered depth alone leaves m1 untested (about 0.2 % of covered pixels lie in [1e-6, 1]): the test supplies the depth
    plane -- exactly 1e-6f and 1.0f, their 1-ulp neighbours, and values well inside / outside -- on the rendered tri_ind."""
    B = 3
    P, im, _, tri_ind, gd, gi, gn = _scene(synth, full, B, seed=55)
    lo, one = np.float32(1e-6), np.float32(1.0)
    vals = np.array([lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(1)), one, np.nextafter(one, np.float32(0)),
                     np.nextafter(one, np.float32(2)), 0.5, 1e-3, 0.25, 2.0, 37.5, 1e-7, 0.0, -3.0, -99999999999999.0], np.float32)
    rs = np.random.RandomState(1)
    depth_n = vals[rs.randint(0, len(vals), (B, 200, 200, 1))]
    depth = _t(depth_n)
    cov = (tri_ind >= 0).cpu().numpy()
    m1 = (depth_n >= lo) & (depth_n <= one)
    m2 = depth_n >= lo
    for m in (m1, m2):
        frac = float(m[cov].mean())
        print("mask true on %.1f %% of covered pixels" % (100 * frac))
        assert 0.10 <= frac <= 0.90
    for v in vals[:6]:
        assert int(((depth_n == v) & cov).sum()) > 100
    # torch's comparison against the Python scalar IS the fp32 compare the header states
    assert np.array_equal(((depth >= 1e-6) & (depth <= 1.0)).cpu().numpy(), m1) and np.array_equal((depth >= 1e-6).cpu().numpy(), m2)
    for a, b, c in ((0, 0, 1), (0, 1, 0), (1, 1, 1)):
        _bwd_both(full, P, gd if a else None, gi if b else None, gn if c else None, im, depth, tri_ind)
    # the pixel-gradient formula itself, through d t_z = sum of the z plane: with g = 1 on every pixel each covered pixel inside
    # the mask hands out 3 * (1/3): the count of such pixels, to the rounding of the thirds
    ones1 = torch.ones((B, 200, 200, 1), device=DEV)
    ones7 = torch.ones((B, 200, 200, 7), device=DEV)
    for gi_, gn_, m in ((ones1, None, m2), (None, ones7, m1)):
        got = full.bwd_fused(P, None, gi_, gn_, ones1, depth, tri_ind)
        want = (m & cov).sum(axis=(1, 2, 3)).astype(np.float64)
        np.testing.assert_allclose(got[:, 5].cpu().numpy().astype(np.float64), want, rtol=1e-5)


# ---- 5. specials -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("special", [float("inf"), float("-inf"), float("nan")])
def test_backward_specials_stay_in_their_face(synth, full, special):
    B = 3
    P, im, depth, tri_ind, gd, gi, gn = _scene(synth, full, B, seed=77)
    clean = full.bwd_fused(P, gd, gi, gn, im, depth, tri_ind)
    ys, xs = np.nonzero(tri_ind[1, :, :, 0].cpu().numpy() >= 0)
    gd2 = gd.clone()
    gd2[1, int(ys[len(ys) // 2]), int(xs[len(xs) // 2]), 0] = special
    got = full.bwd_fused(P, gd2, gi, gn, im, depth, tri_ind)
    want, _, _ = full.bwd_chain(P, gd2, gi, gn, im, depth, tri_ind)
    assert _same(got[[0, 2]], clean[[0, 2]])                    # no bit of any other face's row
    assert not bool(torch.isfinite(got[1]).all())
    # its own row: the Inf / NaN path uses float atomics (order dependent): equal up to that, NaN == NaN
    g1, w1 = got[1].cpu().numpy(), want[1].cpu().numpy()
    assert np.array_equal(np.isnan(g1), np.isnan(w1))
    fin = np.isfinite(w1)
    assert np.array_equal(g1[~fin & ~np.isnan(w1)], w1[~fin & ~np.isnan(w1)])
    np.testing.assert_allclose(g1[fin], w1[fin], rtol=1e-4, atol=0)


# ---- 6. float64 sanity -------------------------------------------------------------------------------------------------------
def _f64_check(oracle, rig, P, dg, tri_ind, got, tol, R=None):
    A = rig.A
    B = int(P.shape[0])
    tri = A["tri"].astype(np.int64)
    ti = tri_ind.cpu().numpy().reshape(B, -1).astype(np.int64)
    g = dg.cpu().numpy().reshape(B, -1).astype(np.float64)
    G = np.zeros((B, 3, rig.N), np.float64)                      # the float64 z plane: g / 3 to the three vertices of every covered pixel
    for b in range(B):
        c = ti[b] >= 0
        for k in range(3):
            np.add.at(G[b, 2], tri[k, ti[b][c]], g[b][c] / 3.0)
    want = oracle.decode_3dmm_backward_f64(G, P.cpu().numpy(), A["mu"], A["pc_shape"], A["pc_exp"],
                                           R=None if R is None else R.cpu().numpy())
    gotn = got.cpu().numpy().astype(np.float64)
    assert np.all(gotn[:, 0:3] == 0) and np.all(want[:, 0:3] == 0)
    ns = rig.ns
    for sl in (slice(3, 6), slice(6, 7), slice(7, 7 + ns), slice(7 + ns, None)):
        scale = np.abs(want[:, sl]).max() + 1e-30
        err = np.abs(gotn[:, sl] - want[:, sl]).max() / scale
        print("float64 check: outputs %s relative error %.3g (bound %.1g)" % (sl, err, tol))
        assert err < tol, (sl, err)


def test_backward_vs_float64(oracle, synth, full, mid):
    for rig, B, tol in ((mid, 5, 2e-5), (mid, 70, 2e-5), (full, 3, 5e-5)):
        P, im, depth, tri_ind, gd, gi, gn = _scene(synth, rig, B, seed=13 + B)
        got = rig.bwd_fused(P, gd, gi, gn, im, depth, tri_ind)
        dn, imn = depth.cpu().numpy(), im.cpu().numpy()
        lo, one = np.float32(1e-6), np.float32(1.0)
        dg = (gn[..., 0:1].cpu().numpy() * imn) * ((dn >= lo) & (dn <= one)) + gi.cpu().numpy() * (dn >= lo) + gd.cpu().numpy()
        _f64_check(oracle, rig, P, torch.as_tensor(dg), tri_ind, got, tol)


# ---- 7. autograd -------------------------------------------------------------------------------------------------------------
def _autograd_pair(net, P, im, gw, gd):
    p1 = P.clone().requires_grad_(True)
    ni, di = net.decode_rendering_layer(p1, im_gray=im)
    node = ni.grad_fn
    ((ni * gw).sum() + (di * gd).sum()).backward()
    p2 = P.clone().requires_grad_(True)
    ni2, di2, _, _ = ops().rendering_layer_fused(net.vertices_transform(p2), net.tri, net.vertex_code, im)
    ((ni2 * gw).sum() + (di2 * gd).sum()).backward()
    assert _same(ni, ni2) and _same(di, di2)
    return p1.grad, p2.grad, node


def test_autograd_node_matches_the_two_nodes_bit_for_bit(full_assets, synth):
    B = 2
    net = net_mod().FaceRecNet(mesh_data=full_assets, batch_size=B, im_size=200)
    P = _t(synth.sample_params_batch(B, beta=0.7, seed=5))
    im = torch.rand((B, 200, 200, 1), device=DEV)
    gw = torch.rand((B, 200, 200, 7), device=DEV)
    gd = torch.rand((B, 200, 200, 1), device=DEV)
    net._basis.backward_from_mu = True
    g1, g2, node = _autograd_pair(net, P, im, gw, gd)
    assert type(node).__name__.startswith("_DecodeRenderingLayer")
    assert float(g1.abs().max()) > 0 and bool(torch.isfinite(g1).all())
    assert _same(g1, g2)
    # nothing of the size of the vertex tensor is kept for the backward
    p3 = P.clone().requires_grad_(True)
    ni, _ = net.decode_rendering_layer(p3, im_gray=im)
    saved = [t for t in ni.grad_fn.saved_tensors if t is not None]
    assert len(saved) == 5
    assert max(int(t.numel()) for t in saved) < B * 3 * net.nvert
    # a caller-computed rotation goes through the node as well
    R = _t(net.rotation_matrix_batch(P[:, :3].cpu().numpy() * 0.5))
    p4 = P.clone().requires_grad_(True)
    ni4, di4 = net.decode_rendering_layer(p4, im_gray=im, R=R)
    ((ni4 * gw).sum() + (di4 * gd).sum()).backward()
    p5 = P.clone().requires_grad_(True)
    ni5, di5, _, _ = ops().rendering_layer_fused(net.vertices_transform(p5, R=R), net.tri, net.vertex_code, im)
    ((ni5 * gw).sum() + (di5 * gd).sum()).backward()
    assert _same(ni4, ni5) and _same(p4.grad, p5.grad) and not _same(p4.grad, g1)
    # the default composed form (d f from the forward's output) differs in d f alone
    net._basis.backward_from_mu = False
    g3, g4, _ = _autograd_pair(net, P, im, gw, gd)
    keep = [i for i in range(g3.shape[1]) if i != 6]
    assert _same(g3, g1) and _same(g3[:, keep], g4[:, keep])


def test_autograd_node_against_the_default_composed_form(full_assets, synth):
    """params.grad through the node against vertices_transform -> rendering_layer_fused in its DEFAULT form (d f from the
    forward's output, fr_decode_3dmm_backward_packed), at rtol = 0, atol = 2e-5 -- the tolerance of
    test_fused_gradient_matches_unfused.  The two routes differ in d f alone (bit for bit elsewhere: the test above), whose two
    forms agree to rounding, not by construction: on these inputs |d f| is about 5e8, so the absolute bound holds only where the
    two roundings coincide.  Inputs are drawn from one seeded CPU generator; the figures are printed before the assertion."""
    B = 2
    net = net_mod().FaceRecNet(mesh_data=full_assets, batch_size=B, im_size=200)
    P = _t(synth.sample_params_batch(B, beta=0.7, seed=5))
    g = torch.Generator(device="cpu").manual_seed(5)
    im = torch.rand((B, 200, 200, 1), generator=g).to(DEV)
    gw = torch.rand((B, 200, 200, 7), generator=g).to(DEV)
    gd = torch.rand((B, 200, 200, 1), generator=g).to(DEV)
    g1, g2, _ = _autograd_pair(net, P, im, gw, gd)
    d = (g1 - g2).abs()
    print("max |difference| %.3g at column %d; |d f| up to %.3g; relative %.3g" %
          (float(d.max()), int(d.max(dim=0).values.argmax()), float(g2[:, 6].abs().max()),
           float(d.max() / g2[:, 6].abs().max())))
    assert torch.allclose(g1, g2, rtol=0, atol=2e-5)


def test_coarse_net_fused_step(small_assets):
    netm, cn = pkg("nets.network"), pkg("nets.coarse_net")
    S, B = 40, 3
    face = netm.FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S)
    face.init_pred_params[..., 6] = 2e-4
    im = torch.rand((B, S, S, 1), device=DEV)
    # the first iteration's input, both routes
    p0 = face.init_pred_params[:B].reshape(B, face.ndim)
    a, da = face.decode_rendering_layer(p0, im_gray=im)
    b, db = face.coarse_net_input(face.vertices_transform(p0), im_gray=im)
    assert _same(a, b) and _same(da, db) and float((a[..., 1:4] > 1e-6).float().mean()) > 0.02
    torch.manual_seed(0)
    fused = cn.CoarseNet(face, nIter=2, fused_step=True).cuda()
    seen = []
    real = face.decode_rendering_layer
    face.decode_rendering_layer = lambda *a_, **k: (seen.append(1) or real(*a_, **k))
    try:
        params = fused(im)
        depth = fused.depth(im, params)
    finally:
        del face.decode_rendering_layer
    assert len(seen) == 3                                        # every iteration and the depth
    params = fused(im)
    depth = fused.depth(im, params)
    assert tuple(depth.shape) == (B, S, S, 1)
    (1e-3 * depth.mean() + 1e-6 * params.sum()).backward()
    for p in fused.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert max(float(p.grad.abs().max()) for p in fused.iters[-1].parameters()) > 0
    # the whole model: vertices_proj still comes out for the SfS loss, by a plain vertices_transform
    model = cn.FaceReconModel(face, nIter=1, fine=False, fused_step=True).cuda().eval()
    with torch.no_grad():
        out = model(im)
        assert tuple(out["vertices_proj"].shape) == (B, 3, face.nvert)
        assert _same(out["coarse_depth_map"], face.coarse_net_input(out["vertices_proj"], im_gray=im)[1])
        assert model(im, with_vertices=False)["vertices_proj"] is None


# ---- 8. threads --------------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams(full_assets, synth):
    B = 4
    net = net_mod().FaceRecNet(mesh_data=full_assets, batch_size=B, im_size=200)
    net._basis.image_t()                                          # (built once, before the threads)
    jobs = []
    for i in range(2):
        P = _t(synth.sample_params_batch(B, beta=0.7, seed=40 + i))
        g = torch.Generator(device="cpu").manual_seed(i)
        jobs.append((P, torch.rand((B, 200, 200, 1), generator=g).to(DEV), torch.rand((B, 200, 200, 7), generator=g).to(DEV),
                     torch.rand((B, 200, 200, 1), generator=g).to(DEV)))

    def run(job, stream=None):
        P, im, gw, gd = job
        outs = []
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
        with ctx:
            for _ in range(3):
                p = P.clone().requires_grad_(True)
                ni, di = net.decode_rendering_layer(p, im_gray=im)
                ((ni * gw).sum() + (di * gd).sum()).backward()
                outs.append((ni.detach(), di.detach(), p.grad))
            torch.cuda.current_stream().synchronize()
        return outs

    want = [run(j) for j in jobs]
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
        got = [f.result(timeout=180) for f in futs]
    finally:
        ex.shutdown(wait=False, cancel_futures=True)
    torch.cuda.synchronize()
    for i in range(2):
        for rnd_g, rnd_w in zip(got[i], want[i]):
            for g, w in zip(rnd_g, rnd_w):
                assert _same(g, w), i
        assert float(want[i][0][2].abs().max()) > 0
