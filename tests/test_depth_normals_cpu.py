"""CPU: the depth-map-normal entry points (fr_depth_normals_forward / _backward) exist, validate before any HIP call and report their
launch geometry; the float64 model of the GPU tests (tests/ref_depth_normals.py) is held to central finite differences of its own
forward and to the renderer's convention -- the normalised normal map compute_abedo_image makes of a render of a tessellated plane."""
import ctypes

import numpy as np
import pytest

from conftest import pkg
import ref_depth_normals as RD

NEW = ("fr_depth_normals_forward", "fr_depth_normals_backward", "fr_debug_depth_normals_geom")


def _L():
    return pkg("_lib").lib()


def _geom(B, H, W):
    out = (ctypes.c_int * 6)()
    _L().fr_debug_depth_normals_geom(B, H, W, out)
    return list(out)


def test_symbols_exported():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert "fr_depth_normals.hip" in pkg("_lib").SOURCES


def test_validates_before_any_hip_call():
    L = _L()
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(4)
    B, H, W = 3, 8, 9

    def fwd(z=one, m=one, B=B, H=H, W=W, out=one):
        return L.fr_depth_normals_forward(z, m, B, H, W, out, nul)

    def bwd(g=one, z=one, m=one, B=B, H=H, W=W, out=one):
        return L.fr_depth_normals_backward(g, z, m, B, H, W, out, nul)
    for call in (fwd, bwd):
        for k in ("B", "H", "W"):
            assert call(**{k: -1}) == -1, k                                  # 1. a negative size
        assert call(B=0) == 0 and call(H=0) == 0 and call(W=0) == 0          # 2. no work
        assert call(B=0, H=-1) == -1 and call(H=0, W=-1) == -1               # ... after the sign check
        assert call(B=0, z=nul, m=nul, out=nul) == 0                         # ... and before the pointer check
        assert call(z=nul) == -1 and call(out=nul) == -1                     # 3. a NULL depth or output
        assert call(H=1 << 16, W=1 << 15) == -4                              # 4. 2^31 pixels
        assert call(H=1 << 16, W=1 << 15, z=nul) == -1                       # ... after the pointer check
        assert call(H=1, W=(1 << 31) - 64) == -4 and call(H=(1 << 31) - 64, W=1) == -4
    assert bwd(g=nul) == -1
    assert bwd(B=0, g=nul, z=nul, m=nul, out=nul) == 0
    # a NULL mask is legal (every pixel valid): such a call gets as far as the size check
    assert fwd(m=nul, H=1 << 16, W=1 << 15) == -4 and bwd(m=nul, H=1 << 16, W=1 << 15) == -4


def test_geometry():
    assert _geom(0, 5, 4) == [0] * 6 and _geom(2, 0, 4) == [0] * 6 and _geom(2, 5, 0) == [0] * 6
    assert _geom(-1, 5, 4) == [0] * 6 and _geom(1, 1 << 16, 1 << 15) == [0] * 6
    tw, th = RD.tile()
    for B, H, W in [(c.B, c.H, c.W) for c in RD.cases()] + [(32, 200, 200), (64, 200, 200)]:
        g = _geom(B, H, W)
        assert g[0] == tw and g[1] == th and g[2] == tw * th and g[2] % 64 == 0 and g[2] <= 1024
        assert g[3] == -(-W // tw) and g[4] == -(-H // th)
        assert 0 < g[5] <= 64 * 1024
        assert g[:3] == _geom(1, 1, 1)[:3]                                   # the tile is no function of the shape
    assert _geom(1, th, tw)[3:5] == [1, 1] and _geom(1, th + 1, tw + 1)[3:5] == [2, 2]
    assert _geom(1, 33, 67)[3] * _geom(1, 33, 67)[4] > 2                     # the "several tiles" case is several tiles
    kinds = {k for c in RD.cases() for k in c.masks}
    assert kinds == set(RD.MASKS)


# ---- the model's self-checks -------------------------------------------------------------------------------------------------
FD_CASES = [c for c in RD.cases() if c.H * c.W <= 400 or c.B == 3][::2] + [RD.Case(1, 33, 67, ("disc",))]


def _fwd64(z, v):
    """the model's forward on float64 depths [B,H,W] (ref_depth_normals.forward widens fp32 first and then does exactly this)"""
    L, R, U, D = RD._nbrs(v)
    dx = np.where(v, RD._diff(z, L, R, 0, 1), 0.0)
    dy = np.where(v, RD._diff(z, U, D, 1, 0), 0.0)
    s = np.sqrt((dx * dx + dy * dy) + 1.0)
    return np.where(v[..., None], np.stack([-dx / s, -dy / s, 1.0 / s], -1), 0.0)


@pytest.mark.parametrize("case", FD_CASES, ids=RD.case_id)
def test_model_gradient_vs_finite_differences(case):
    """d/dz of L(z) = sum(g . n(z)) by central differences of the model's forward at step 1e-5, float64 throughout.  Truncation
    ~ h^2, rounding ~ 1e-16 / h, both near 1e-10 for slopes of order 1: the bound is 1e-7 of the largest entry.
    Moving z(r, c) moves the normals of (r, c) and its four neighbours only, so L is summed over the 3 x 3 block around the pixel,
    and the forward is run on the 5 x 5 window around it: every pixel of the block has its whole stencil inside the window, or
    outside the image on both."""
    d = RD.inputs(case)
    z0 = d["depth"].astype(np.float64)[..., 0]
    g = d["grad_normal"].astype(np.float64)
    G, A = RD.backward(d["grad_normal"], d["depth"], d["mask"])
    v = RD.valid_of(d["mask"], z0.shape)
    assert np.array_equal(_fwd64(z0, v), RD.forward(d["depth"], d["mask"]).normal)
    h = 1e-5
    fd = np.zeros_like(z0)
    for b, r, c in np.argwhere(v):
        wr, wc = max(r - 2, 0), max(c - 2, 0)                                 # the window's origin
        win = (slice(b, b + 1), slice(wr, min(r + 3, case.H)), slice(wc, min(c + 3, case.W)))
        blk = (slice(0, 1), slice(max(r - 1, 0) - wr, min(r + 2, case.H) - wr), slice(max(c - 1, 0) - wc, min(c + 2, case.W) - wc))
        vals = []
        for sgn in (1.0, -1.0):
            z = z0[win].copy()
            z[0, r - wr, c - wc] += sgn * h
            vals.append(float((g[win][blk] * _fwd64(z, v[win])[blk]).sum()))
        fd[b, r, c] = (vals[0] - vals[1]) / (2 * h)
    big = np.abs(G).max()
    err = np.abs(G[..., 0] - fd).max()
    print("%s: max |G| %.3g, max |G - FD| %.3g (bound %.3g)" % (RD.case_id(case), big, err, 1e-7 * big))
    assert not G[..., 0][~v].any() and not A[..., 0][~v].any()                # invalid pixels: exactly 0
    if all(k in RD.FLAT for k in case.masks) or case.H * case.W == 1:
        assert big == 0 and not fd.any()                                      # no valid pixel has a valid neighbour
    else:
        assert big > 1e-3
        assert err <= 1e-7 * big


def _plane_scene(a, b):
    """a 16 x 16-vertex unit grid at offset (-1.75, -1.75), two triangles per cell, both windings, on z = a x + b y + 40"""
    n = 16
    gx, gy = np.meshgrid(np.arange(n) - 1.75, np.arange(n) - 1.75)           # vertex id = row * 16 + column
    x, y = gx.ravel(), gy.ravel()
    ver = np.stack([x, y, a * x + b * y + 40.0]).astype(np.float32)[None]     # [1,3,256]
    tri = []
    for r in range(n - 1):
        for c in range(n - 1):
            v00, v01, v10, v11 = r * n + c, r * n + c + 1, (r + 1) * n + c, (r + 1) * n + c + 1
            if (r + c) % 2 == 0:
                tri += [(v00, v01, v11), (v00, v11, v10)]                     # one winding
            else:
                tri += [(v00, v11, v01), (v00, v10, v11)]                     # the other
    return ver, np.array(tri, np.float32).T.copy()


@pytest.mark.parametrize("a,b", [(0.5, -0.25), (-1.5, 0.75), (0.0, 2.0)])
def test_model_vs_the_renderers_convention(oracle, a, b):
    """The depth normals of a rendered plane against compute_abedo_image's normalised normal map of the same render (its
    post-processing restated in numpy fp32).  Bound 5e-6: the +1e-6 in the render's normalisation gives up to 1e-6, the fp32
    rounding of two triangle depths near 40 (half an ulp = 1.9e-6 each) up to 3.8e-6.  Every pixel must be covered."""
    H, W = 12, 14
    ver, tri = _plane_scene(a, b)
    depth, _, nrm, tind = oracle.render_depth(ver, tri, np.zeros((1, 3, ver.shape[2]), np.float32), H, W)
    covered = int((tind >= 0).sum())
    print("covered pixels: %d of %d" % (covered, H * W))
    assert covered == H * W
    n = nrm.astype(np.float32)
    n = np.where(n[..., 2:3] < 0, np.float32(-1.0) * n, n)                    # network.py: flip to z >= 0, normalise
    mag = (n * n).sum(-1)
    mag = np.where(mag > 1e-6, mag, np.float32(1.0))
    nmap = n / (np.sqrt(mag) + np.float32(1e-6))[..., None]
    m = RD.forward(depth, tind)
    want = np.array([-a, -b, 1.0]) / np.sqrt(a * a + b * b + 1.0)
    e_render = np.abs(m.normal - nmap.astype(np.float64)).max()
    e_plane = np.abs(m.normal - want).max()
    print("slopes (%g, %g): max |depth normals - render's normal map| %.3g, - the plane's normal %.3g (bound 5e-6)"
          % (a, b, e_render, e_plane))
    assert e_render <= 5e-6
    assert (m.normal[..., 2] > 0).all()
