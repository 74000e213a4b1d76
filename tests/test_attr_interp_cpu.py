"""CPU: the smooth planes' surface and models (include/fr_hotpath.h, "smooth planes"; tests/ref_attr_interp.py).

- the four entry points are exported, bound from a signature row each, declare no sized buffer, and return the documented codes
  before any HIP call;
- the models' derivatives -- the interpolation's with respect to the attribute and the vertices, the vertex normals' with respect to
  the vertices -- agree with central differences of their own float64 forwards on directional derivatives, tri_ind held fixed;
- the forward model reproduces the render's flat texture lookup where a triangle has no area.

THE BOUND OF THE DIRECTIONAL DERIVATIVES.  f(t) is the float64 forward along V + t dV (and A + t dA), weighted by a fixed G.
The central difference D = (f(e) - f(-e)) / 2e differs from f'(0) by the truncation e^2 / 6 |f'''(xi)| and by the rounding of
the two evaluations, at most r F / e with F the sum of the magnitudes of f's summands and r the relative error of one summand.
f''' is taken from the five-point stencil (f(2e) - 2 f(e) + 2 f(-e) - f(-2e)) / 2e^3 of the same forward and doubled (it is
itself an estimate, over an interval in which no weight changes sign: the steps are asserted to keep every pixel's sign
pattern); r is 64 roundings of 2^-53 times the cancellation of the one difference the chain forms from like-sized products (den
for the interpolation, the summed facet normals against |N| for the normals).  Nothing in the bound comes from the derivative
under test."""
import ctypes
import os
import re

import numpy as np

import ref_attr_interp as RA
import ref_normal_backward as RN
from conftest import ROOT, pkg

NEW = ("fr_attr_interp_forward", "fr_attr_interp_backward", "fr_mesh_vertex_normals_backward", "fr_debug_attr_interp_bwd_geom")


def _header():
    with open(os.path.join(ROOT, "include", "fr_hotpath.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_exports_and_signature_rows():
    host = pkg("_lib")
    L = host.lib()
    for name in NEW:
        assert name in host.SIGNATURES and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, _header()), name
    assert "fr_attr_interp.hip" in host.SOURCES and any(p.endswith("fr_point_weight.h") for p in host.HEADERS)


def test_no_sized_buffer_is_declared():
    """records, partial and h are typed tensors whose shapes the header states: no size function, no byte count"""
    host = pkg("_lib")
    sized = re.findall(r"size_t\s+(fr_\w+_bytes)\s*\(", _header())
    assert sized and not [s for s in sized if "attr_interp" in s or "vertex_normals" in s or "smooth" in s]
    for name in NEW:
        assert "z" not in host.SIGNATURES[name], name
        proto = re.search(r"\b%s\s*\(([^()]*)\)" % name, _header()).group(1)
        assert "size_t" not in proto and "hip_stream" not in proto, name
        assert name.startswith("fr_debug_") or re.search(r"void\*\s+stream$", proto.strip()), name


def test_geometry_hook_is_the_depth_interps():
    L = pkg("_lib").lib()
    for args in ((3, 480, 33, 40), (3, 480, 8, 9), (1, 480, 64, 64), (8, 480, 64, 64), (64, 53215, 200, 200), (0, 5, 4, 4), (2, 0, 4, 4),
                 (1, 5, 65536, 65536)):
        a, d = (ctypes.c_int * 6)(), (ctypes.c_int * 6)()
        L.fr_debug_attr_interp_bwd_geom(*args, a)
        L.fr_debug_depth_interp_bwd_geom(*args, d)
        assert list(a) == list(d), args
    a = (ctypes.c_int * 6)()
    L.fr_debug_attr_interp_bwd_geom(8, 480, 33, 40, a)
    assert a[3] == 2 and a[5] == 1 and a[2] == 0


def test_return_codes_before_any_hip_call():
    L = pkg("_lib").lib()
    nul, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(256), ctypes.c_void_p(260)

    def fwd(vertex=one, vp=64, attr=one, ap=64, tri=one, ti=one, B=2, nver=64, ntri=5, H=8, W=8, out=one):
        return L.fr_attr_interp_forward(vertex, vp, attr, ap, tri, ti, B, nver, ntri, H, W, out, nul)

    def bwd(grad=one, vertex=one, vp=64, attr=one, ap=64, tri=one, ti=one, ag=one, aacc=0, vg=one, vacc=0, B=2, nver=64, ntri=5, H=8,
            W=8, rec=one, part=one):
        return L.fr_attr_interp_backward(grad, vertex, vp, attr, ap, tri, ti, ag, aacc, vg, vacc, B, nver, ntri, H, W, rec, part, nul)

    def nbw(g=one, gp=64, vertex=one, vp=64, tri=one, a0=one, a1=one, B=2, nver=64, ntri=5, h=one, vg=one, op=64, acc=0):
        return L.fr_mesh_vertex_normals_backward(g, gp, vertex, vp, tri, a0, a1, B, nver, ntri, h, vg, op, acc, nul)

    for f in (fwd, bwd):
        assert f(B=-1) == -1 and f(nver=-1) == -1 and f(ntri=-1) == -1 and f(H=-1) == -1 and f(W=-1) == -1
        assert f(vp=63) == -1 and f(ap=63) == -1
        assert f(B=0) == 0 and f(H=0) == 0 and f(W=0) == 0
        assert f(B=0, ti=nul) == 0 and f(B=0, vp=63) == -1                     # the sizes and pitches come first
        assert f(ti=nul) == -1 and f(tri=nul) == -1 and f(vertex=nul) == -1 and f(attr=nul) == -1
        assert f(ntri=1 << 24) == -4 and f(H=70000, W=70000) == -4
    assert fwd(out=nul) == -1 and fwd(ntri=0, out=nul) == -1
    assert bwd(aacc=2) == -1 and bwd(vacc=-1) == -1 and bwd(aacc=2, B=0) == -1
    assert bwd(nver=0, vp=0, ap=0, ag=nul, vg=nul) == 0                        # empty gradients: nothing to write
    assert bwd(ag=nul, vg=nul) == -1 and bwd(grad=nul) == -1
    assert bwd(rec=nul) == -2 and bwd(part=nul) == -2 and bwd(rec=ctypes.c_void_p(264)) == -2 and bwd(part=odd) == -2
    assert bwd(rec=nul, grad=nul) == -1 and bwd(rec=nul, ntri=1 << 24) == -4   # a bad argument wins over the workspace
    assert bwd(ag=nul, rec=nul) == -2 and bwd(vg=nul, part=nul) == -2
    assert nbw(B=-1) == -1 and nbw(nver=-1) == -1 and nbw(ntri=-1) == -1 and nbw(gp=63) == -1 and nbw(vp=63) == -1 and nbw(op=63) == -1
    assert nbw(acc=2) == -1 and nbw(B=0) == 0 and nbw(nver=0, gp=0, vp=0, op=0) == 0 and nbw(B=0, acc=3) == -1
    assert nbw(g=nul) == -1 and nbw(vertex=nul) == -1 and nbw(vg=nul) == -1 and nbw(tri=nul) == -1 and nbw(a0=nul) == -1 and nbw(a1=nul) == -1
    assert nbw(ntri=1 << 24) == -4 and nbw(h=nul) == -2 and nbw(h=odd) == -2 and nbw(h=nul, g=nul) == -1


# ---- the derivatives ----------------------------------------------------------------------------------------------------------------
def _five_point(f, e):
    """-> (the central difference at step e, the bound's truncation part): f evaluated at +-e and +-2e"""
    fp, fm, fpp, fmm = f(e), f(-e), f(2 * e), f(-2 * e)
    d3 = (fpp - 2 * fp + 2 * fm - fmm) / (2 * e ** 3)
    return (fp - fm) / (2 * e), 2 * (e * e / 6) * abs(d3)


def _interp_scene(seed, nver=14, ntri=12, H=6, W=7):
    """random well-shaped triangles around the image, a random triangle (or none) per pixel -- extrapolation is legal"""
    rs = np.random.RandomState(seed)
    V = np.stack([rs.uniform(-2, W + 2, nver), rs.uniform(-2, H + 2, nver), rs.uniform(1, 9, nver)]).astype(np.float32)
    tri = []
    while len(tri) < ntri:
        p = rs.choice(nver, 3, replace=False)
        a, b = V[:2, p[1]] - V[:2, p[0]], V[:2, p[2]] - V[:2, p[0]]
        if abs(a[0] * b[1] - a[1] * b[0]) > 0.2 * np.linalg.norm(a) * np.linalg.norm(b) and min(np.linalg.norm(a), np.linalg.norm(b)) > 1:
            tri.append(p)
    tri = np.array(tri).T.astype(np.float32)
    tind = rs.randint(-1, ntri, H * W).astype(np.float32)
    A = rs.uniform(-1, 1, (3, nver)).astype(np.float32)
    A[A == 0] = 0.5
    G = rs.standard_normal((H * W, 3)).astype(np.float32)
    return dict(V=V, A=A, tri=tri, tind=tind, G=G, H=H, W=W, nver=nver)


def test_interpolation_derivatives_agree_with_central_differences():
    worst = 0.0
    for seed in (1, 2, 3):
        sc = _interp_scene(seed)
        H, W, nver = sc["H"], sc["W"], sc["nver"]
        px, ids = RN.contributing(sc["tri"], sc["tind"], nver)
        assert 20 < len(px) < H * W
        ga, gv = RA.sums64(sc["G"][None], sc["V"][None], sc["A"][None], sc["tri"], sc["tind"][None], H, W)
        assert not ga[0][:, np.setdiff1d(np.arange(nver), ids)].any() and not gv[0, 2].any()      # untouched vertices, the z row
        V0, A0, G = sc["V"].astype(np.float64), sc["A"].astype(np.float64), sc["G"][px].astype(np.float64)
        rs = np.random.RandomState(100 + seed)
        for what in ("attr", "vertex", "both"):
            dV = rs.standard_normal(V0.shape) * (what != "attr")
            dA = rs.standard_normal(A0.shape) * (what != "vertex")
            e = 2.0 ** -13

            def f(t):
                return float((RA.forward64(V0 + t * dV, A0 + t * dA, ids, px, W)[0] * G).sum())
            _, w0, den0 = RA.forward64(V0, A0, ids, px, W)
            for t in (-2 * e, 2 * e):                                                             # the sign pattern holds over the stencil
                _, w, den = RA.forward64(V0 + t * dV, A0 + t * dA, ids, px, W)
                assert np.array_equal(np.sign(w), np.sign(w0)) and np.array_equal(np.sign(den), np.sign(den0))
            P = [V0[:, ids[k]] for k in range(3)]
            d00 = ((P[2][:2] - P[0][:2]) ** 2).sum(0)
            d11 = ((P[1][:2] - P[0][:2]) ** 2).sum(0)
            cancel = float((2 * d00 * d11 / np.abs(den0)).max())                                   # den = dot00 dot11 - dot01^2
            F = float(sum((np.abs(w0[k])[:, None] * np.abs(A0[:, ids[k]].T) * np.abs(G)).sum() for k in range(3)))
            want = float((ga[0] * dA).sum() + (gv[0] * dV).sum())
            got, trunc = _five_point(f, e)
            bound = trunc + 64 * 2.0 ** -53 * cancel * F / e
            rng = float(np.abs(ga[0] * dA).sum() + np.abs(gv[0] * dV).sum())
            print("seed %d %-6s: derivative %+.6e (summands up to %.3e), central difference off by %.3e, bound %.3e"
                  % (seed, what, want, rng, abs(got - want), bound))
            assert abs(want) > 1e-3 * rng and bound < 1e-4 * rng                                   # the check can tell a wrong derivative
            assert abs(got - want) <= bound
            worst = max(worst, abs(got - want) / bound)
    print("worst error / bound = %.3f" % worst)


def _grid(nu=5, nv=6, seed=4):
    """an nu x nv vertex grid bent out of its plane, jittered; one vertex without a triangle, one triangle naming a vertex twice"""
    rs = np.random.RandomState(seed)
    iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    V = np.stack([iv.ravel() * 2.0, iu.ravel() * 2.0, 0.3 * (iu.ravel() - 2.0) ** 2 + 0.2 * iv.ravel()])
    V = np.concatenate([V + rs.uniform(-0.3, 0.3, V.shape), [[50.0], [50.0], [1.0]]], axis=1).astype(np.float32)   # the last: alone
    t = []
    for a in range(nu - 1):
        for b in range(nv - 1):
            p = a * nv + b
            t += [(p, p + 1, p + nv), (p + 1, p + nv + 1, p + nv)]
    t.append((0, 0, 7))                                                                           # contributes a zero normal
    return V, np.array(t).T.astype(np.float32)


def test_vertex_normal_derivative_agrees_with_central_differences():
    mesh_io = pkg("utils.mesh_io")
    V, tri = _grid()
    nver = V.shape[1]
    a0, a1 = mesh_io.vertex_adjacency(tri, nver)
    rs = np.random.RandomState(9)
    g = rs.standard_normal((1, 3, nver)).astype(np.float32)
    out, R, Hh = RA.normals_backward(g, V[None], tri, a0, a1)
    assert not R[0, :, nver - 1].any() and not Hh[0, :, nver - 1].any() and R[0, :, :nver - 1].all()
    assert np.array_equal(out, R.astype(np.float32))
    V0, G = V.astype(np.float64), g[0].astype(np.float64)
    n0 = RA.normals64(V0, tri, a0, a1)
    assert np.allclose((n0[:, :nver - 1] ** 2).sum(0), 1.0, atol=1e-12) and not n0[:, nver - 1].any()
    # the cancellation of a vertex's sum: the facet normals' magnitudes against the length of their sum
    ids = RN.f2i_x86(tri)
    mags = np.zeros(nver)
    P = [V0[:, ids[k]] for k in range(3)]
    facet = np.linalg.norm(np.cross((P[1] - P[0]).T, (P[2] - P[0]).T), axis=1)
    for k in range(3):
        np.add.at(mags, ids[k], facet)
    _, N, S = RA._normal_sums(V0, ids, a0, a1)
    cancel = max(mags[v] / S[v] for v in range(nver - 1))
    worst = 0.0
    for trial in range(3):
        dV = rs.standard_normal(V0.shape)
        e = 2.0 ** -13

        def f(t):
            return float((RA.normals64(V0 + t * dV, tri, a0, a1) * G).sum())
        want = float((R[0] * dV).sum())
        rng = float(np.abs(R[0] * dV).sum())
        got, trunc = _five_point(f, e)
        bound = trunc + 64 * 2.0 ** -53 * cancel * float(np.abs(G).sum()) / e
        print("trial %d: derivative %+.6e (summands up to %.3e), central difference off by %.3e, bound %.3e"
              % (trial, want, rng, abs(got - want), bound))
        assert abs(want) > 1e-3 * rng and bound < 1e-4 * rng
        assert abs(got - want) <= bound
        worst = max(worst, abs(got - want) / bound)
    print("worst error / bound = %.3f" % worst)


def test_forward_model_is_the_renders_lookup_without_area():
    """every triangle collapsed to a point in the screen plane (x = y = 0): den == 0 at every pixel, and the model's plane is the CPU
    oracle's tex_img wherever a triangle wins, bit for bit; (+0, +0, +0) elsewhere"""
    import workspace_cases as WC
    sc = WC.scene("even")
    B, H, W = sc["B"], sc["H"], sc["W"]
    V = sc["V"].copy()
    V[:, 0:2] = 0
    got = RA.forward(V, sc["tex"], sc["tri"], sc["tind"], H, W)
    cov = sc["tind"].reshape(B, H, W) >= 0
    assert cov.any() and not cov.all()
    assert np.array_equal(got[cov].view(np.uint32), np.ascontiguousarray(sc["tex_img"], np.float32)[cov].view(np.uint32))
    assert not got[~cov].view(np.uint32).any()
    # ... and the backward's terms there: a third of the gradient to each vertex, in fp32; nothing through x and y
    g = sc["g3"].reshape(B, H * W, 3)
    _, _, Ta32, _, Tv32 = RA.terms(g[0], V[0], sc["tex"][0], np.asarray(sc["tri"]), sc["tind"].reshape(B, -1)[0], sc["nver"], W)
    px, _ = RN.contributing(np.asarray(sc["tri"]), sc["tind"].reshape(B, -1)[0], sc["nver"])
    third = (g[0][px] * np.float32(1.0)) / np.float32(3.0)
    assert all(np.array_equal(Ta32[:, k].view(np.uint32), third.view(np.uint32)) for k in range(3)) and not Tv32.view(np.uint32).any()
