"""CPU: colour shading (csrc/fr_shade.h, fr_photo.hip, fr_synth.hip; include/fr_hotpath.h, "colour shading").  The numpy model of the
GPU tests (tests/ref_photo_rgb.py) is held to central differences of a float64 forward; the planes of the GPU tests reach every branch;
the new entry points return every code of the header before any HIP call; the compiler's resource report shows no scratch for the new
kernels; the binding rows match the header; the Python surface keeps its defaults and raises where it says."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import pkg
import ref_photo_rgb as RC

NEW = ("fr_synth_light_rgb", "fr_synth_shade_rgb", "fr_photo_loss_rgb_state_bytes", "fr_photo_loss_rgb_forward",
       "fr_photo_loss_rgb_backward", "fr_debug_photo_loss_rgb_geom")
F = np.float32
GAIN, OFFSET = 1.75, -0.125
SHAPES, SEEDS = RC.SHAPES, RC.SEEDS          # the GPU test's


def _L():
    return pkg("_lib").lib()


def test_symbols_exported_and_bound_as_the_header_says():
    h = pkg("_lib")
    L = _L()
    with open(os.path.join(os.path.dirname(h._CSRC), "..", "include", "fr_hotpath.h")) as f:
        src = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    letter = {"int": "i", "float": "f", "size_t": "z", "unsigned long long": "u", "int*": "I", "void": "v"}
    for name in NEW:
        assert hasattr(L, name) and name in h.EXPORTS, name
        ret, args = re.search(r"([a-z_ ]+?)\s+%s\s*\(([^()]*)\)\s*;" % name, src).groups()
        row = letter[ret.strip()] + ":"
        for a in args.split(","):
            ty = re.sub(r"\s+", " ", re.match(r"^(.*?)(\w+)$", a.strip(), flags=re.S).group(1)).strip().replace(" *", "*")
            row += letter.get(ty, "p" if ty.endswith("*") else None)
        assert h.SIGNATURES[name] == row, (name, row)


# ---- the model's gradient -----------------------------------------------------------------------------------------------------------------
def _case64():
    tex, nrm, ti, light, target, weight = RC.smooth_case()
    st = RC.shade_terms(tex, nrm, ti, light, GAIN, OFFSET)
    cov = st["covered"]
    # the case keeps away from the kinks
    assert (st["s"][cov] > 0.25).all() and (tex > 0.1).all() and (st["mag"] > 1e-3).all()
    assert cov.any() and (~cov).any() and st["flipped"][cov].any() and (~st["flipped"][cov]).any()
    return tex, nrm, ti, light, target, weight, cov, st


def test_model_gradient_against_central_differences():
    """DIRECTIONAL derivatives of f = sum_b g_b sse_b (forward64) along random directions v, by central differences, against <model
    gradient, v>.  The model's backward runs unrounded and on a float64 shading chain (F=np.float64: the same formulas and the same
    code as the GPU tests' model, without the fp32 roundings of the shader, which are no part of a derivative).
    THE BOUND.  f is a sum of N = 3 x (covered pixels) terms g w r^2, each a chain of fewer than 64 float64 operations on magnitudes
    that T = sum |g| w (|im| + |target|)^2 bounds (|im| formed with every coefficient's absolute value), so one evaluation of f is
    within e_f = (N + 128) 2^-53 T of its exact value, and a central difference with step h within e_f / h of the exact quotient.
    The model's own gradient is held to the same budget once more: its elements are chains of fewer than 128 operations on the
    derivatives of those terms with respect to quantities this case keeps above 0.1 (tex >= 0.2, s >= 0.25, |n| >= 0.3), i.e. on
    magnitudes below 10 T, and 128 x 10 < (N + 128) / h for every step used.
    In tex and in light f is a quadratic polynomial along any line that stays clear of the clamps (it does: both ends are checked),
    so the central difference has NO truncation error: the bound is 2 e_f / h with the large step h = 2^-5.  In the normal f is not a
    polynomial: the quotient is Richardson-extrapolated, D*(h) = (4 D(h/2) - D(h)) / 3, whose rounding error is at most
    (4 e_f / (h/2) + e_f / h) / 3 = 3 e_f / h and whose truncation error is O(h^4), estimated a posteriori as |D*(h) - D*(h/2)|
    (fifteen times the leading term's estimate of the finer value's error); the value tested is D*(h/2) with h = 2^-8 and the bound
    2 x 3 e_f / (h/2) + |D*(h) - D*(h/2)|.
    CONDITION ON THE INPUTS: every bound is below 1e-6 of the derivative it is held against."""
    tex, nrm, ti, light, target, weight, cov, st = _case64()
    B = tex.shape[0]
    g_up = np.array([1.0, -0.75])[:B]
    gt, gn, gl, _ = RC.backward(tex, nrm, ti, light, target, g_up, weight, GAIN, OFFSET, rounded=False, F=np.float64)
    x64 = [tex.astype(np.float64), nrm.astype(np.float64), light.astype(np.float64)]
    t64, w64 = target.astype(np.float64), weight.astype(np.float64)[..., 0]

    def loss(xs):
        return float((g_up * RC.forward64(xs[0], xs[1], cov, xs[2], t64, w64, GAIN, OFFSET)).sum())

    def central(k, v, h):
        up, dn = [x.copy() for x in x64], [x.copy() for x in x64]
        up[k] = up[k] + h * v
        dn[k] = dn[k] - h * v
        return (loss(up) - loss(dn)) / (2 * h)
    # T: the terms' magnitudes
    im_abs = st["a"].astype(np.float64) * np.einsum("bck,bhwk->bhwc", np.abs(x64[2]), np.abs(st["H"].astype(np.float64))) * GAIN + abs(OFFSET)
    T = float((np.abs(g_up)[:, None, None] * np.where(cov, w64 * ((im_abs + np.abs(t64)) ** 2).sum(-1), 0.0)).sum())
    e_f = (3 * int(cov.sum()) + 128) * 2.0 ** -53 * T
    rs = np.random.RandomState(11)
    for k, (name, want) in enumerate((("tex_img", gt), ("normal", gn), ("light", gl))):
        for trial in range(6):
            v = rs.uniform(0.25, 1.0, want.shape) * np.where(rs.uniform(size=want.shape) < 0.5, -1.0, 1.0)
            exact = float((want * v).sum())
            if name == "normal":
                h = 2.0 ** -8
                d1, d2, d4 = central(k, v, h), central(k, v, h / 2), central(k, v, h / 4)
                coarse, num = (4 * d2 - d1) / 3, (4 * d4 - d2) / 3
                bound = 2 * 3 * e_f / (h / 2) + abs(coarse - num)
            else:
                h = 2.0 ** -5
                if name == "tex_img":
                    assert (x64[0] - h > 0.1).all()                                   # clear of the albedo clamp at both ends
                else:
                    for sign in (-1.0, 1.0):                                          # every channel stays lit at both ends
                        assert (RC.shade_terms(tex, nrm, ti, (x64[2] + sign * h * v), GAIN, OFFSET)["s"][cov] > 0.05).all()
                num = central(k, v, h)
                bound = 2 * e_f / h
            err = abs(num - exact)
            print("%s, direction %d: derivative %.6g, |model - difference| = %.3g, bound %.3g" % (name, trial, exact, err, bound))
            assert bound < 1e-6 * abs(exact), (name, trial, bound, exact)
            assert err <= bound, (name, trial, err, bound)
    assert not gt[~cov].any() and not gn[~cov].any()


def test_forward64_agrees_with_the_models_sums():
    tex, nrm, ti, light, target, weight, cov, _ = _case64()
    sums = RC.forward(tex, nrm, ti, light, target, weight, GAIN, OFFSET)
    f64 = RC.forward64(tex.astype(np.float64), nrm.astype(np.float64), cov, light.astype(np.float64), target.astype(np.float64),
                       weight.astype(np.float64)[..., 0], GAIN, OFFSET)
    # the fp32 shader's image carries a relative 2^-24 per operation, squared residuals twice that: 64 roundings are generous
    assert np.abs(sums[:, 0] - f64).max() <= 64 * 2.0 ** -24 * np.abs(f64).max()
    assert np.array_equal(sums[:, 1], cov.reshape(cov.shape[0], -1).sum(1).astype(np.float64))


# ---- the planes of the GPU tests ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-%dx%d" % s)
def test_hand_planes_reach_every_branch(shape):
    tex, nrm, ti, light, target, weight = RC.hand_planes_rgb(*shape, seed=SEEDS[shape])
    got = RC.branches(tex, nrm, ti, light, weight)
    assert tuple(got) == RC.BRANCHES and len(RC.BRANCHES) == 4 + 12 + 3
    assert all(got.values()), [k for k, v in got.items() if not v]
    assert RC.reaches_every_branch(tex, nrm, ti, light, weight)
    assert target.shape == shape + (3,) and light.shape == (shape[0], 3, 9)
    bad = RC.hand_planes_rgb(*shape, seed=SEEDS[shape], nan=True)
    assert np.isnan(bad[0]).sum() == 1 and (bad[2][..., 0] >= 0)[np.isnan(bad[0]).any(-1)].all()


@pytest.mark.parametrize("weighted", [False, True])
def test_the_models_own_image_gives_exact_zeros(weighted):
    B, H, W = 3, 33, 17
    tex, nrm, ti, light, _, weight = RC.hand_planes_rgb(B, H, W, seed=SEEDS[(B, H, W)])
    target, gray, mask = RC.shade(tex, nrm, ti, light, None, GAIN, OFFSET)
    w = weight if weighted else None
    sums = RC.forward(tex, nrm, ti, light, target, w, GAIN, OFFSET)
    assert sums.shape == (B, 29) and not sums[:, 0].any() and not sums[:, 2:].any()
    assert np.array_equal(sums[:, 1], mask.reshape(B, -1).sum(1).astype(np.float64))
    gt, gn, gl, _ = RC.backward(tex, nrm, ti, light, target, np.array([1.0, -2.0, 0.5]), w, GAIN, OFFSET)
    assert not gt.any() and not gn.any() and not gl.any()
    other = RC.hand_planes_rgb(B, H, W, seed=SEEDS[(B, H, W)])[4]
    gt, gn, gl, _ = RC.backward(tex, nrm, ti, light, other, np.array([1.0, -2.0, 0.5]), w, GAIN, OFFSET)
    assert gt.any() and gn.any() and gl.all()
    assert np.array_equal(gray[..., 0], (F(0.3) * target[..., 0] + F(0.59) * target[..., 1]) + F(0.11) * target[..., 2])


def test_sampler_model():
    a = RC.sample_light(7, 3, 4)
    assert a.shape == (4, 3, 9) and a.dtype == F
    rg = np.asarray(RC.LIGHT_RANGES_RGB, F)
    assert (a.reshape(4, 27) >= rg[:, 0]).all() and (a.reshape(4, 27) <= rg[:, 1]).all()
    # a face's values depend on (seed, global face index) alone
    assert np.array_equal(RC.sample_light(7, 5, 2), a[2:4]) and not np.array_equal(RC.sample_light(8, 3, 4), a)
    assert len(np.unique(a)) == a.size
    assert pkg("rendering_layer.ops").SYNTH_LIGHT_RANGES_RGB == RC.LIGHT_RANGES_RGB


# ---- sizes, geometry and return codes -------------------------------------------------------------------------------------------------------
def test_sizes_and_geometry():
    L = _L()
    for B, H, W in SHAPES + [(64, 200, 200), (65535, 1, 1), (1, 1, 1)]:
        g = RC.geom_rgb(B, H, W)
        assert g == [256, -(-H * W // 256), 256, 29], (B, H, W)
        assert g[:3] == RC.geom(B, H, W)[:3]                                        # the gray loss's tiling
        assert L.fr_photo_loss_rgb_state_bytes(B, H, W) == B * g[1] * 29 * 8
    assert RC.geom_rgb(1, 5, 6)[1] == 1 and RC.geom_rgb(1, 257, 256)[1] == RC.geom_rgb(1, 257, 256)[2] + 1
    for bad in [(0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (65536, 1, 1), (1, 1 << 16, 1 << 15)]:
        assert RC.geom_rgb(*bad) == [0] * 4 and L.fr_photo_loss_rgb_state_bytes(*bad) == 0, bad


GOOD, ODD = 0x1000, 0x1008          # made-up addresses: 16-byte aligned, and not


def test_return_codes_without_a_gpu():
    """Every call here trips a check, so none reaches HIP: single bad arguments, and pairs of them to fix the checks' order.  SKIPS
    where a GPU is visible, as tests/test_photo_loss_cpu.py does: it checks host code, and a case that slipped through validation
    would launch on the made-up addresses."""
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    L = _L()
    P = ctypes.c_void_p
    nst = L.fr_photo_loss_rgb_state_bytes(3, 17, 33)

    def fwd(B=3, H=17, W=33, state=GOOD, state_bytes=nst, **nul):
        p = {k: P(0 if k in nul else GOOD) for k in ("tex_img", "normal", "tri_ind", "light", "target", "weight", "sums")}
        return L.fr_photo_loss_rgb_forward(p["tex_img"], p["normal"], p["tri_ind"], p["light"], p["target"], p["weight"], B, H, W, 1.0,
                                           0.0, p["sums"], P(state), state_bytes, P(0))

    def bwd(B=3, H=17, W=33, **nul):
        p = {k: P(0 if k in nul else GOOD) for k in ("grad_sse", "sums", "tex_img", "normal", "tri_ind", "light", "target", "weight",
                                                     "gt", "gn", "gl")}
        return L.fr_photo_loss_rgb_backward(p["grad_sse"], p["sums"], p["tex_img"], p["normal"], p["tri_ind"], p["light"], p["target"],
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
    assert fwd(state_bytes=L.fr_photo_loss_state_bytes(3, 17, 33)) == -2   # the gray loss's state is too small
    assert fwd(B=65536, state=0) == -2 and fwd(B=65536, state_bytes=0) == -4   # (beyond one grid the state's size is 0)
    assert fwd(W=0, state=0, state_bytes=0) == 0
    assert bwd(grad_sse=0) == -1
    assert bwd(sums=0) == -1 and bwd(sums=0, gl=0, B=65536) == -4           # sums serve grad_light alone
    assert bwd(gt=0, gn=0, gl=0) == 0                                       # nothing wanted: nothing launched
    assert bwd(gt=0, gn=0, gl=0, B=65536) == -4 and bwd(weight=0, B=65536) == -4

    # the sampler: the order of fr_synth_params
    ok = (ctypes.c_float * 54)(*[v for pair in RC.LIGHT_RANGES_RGB for v in pair])

    def ranges(**at):
        r = (ctypes.c_float * 54)(*ok)
        for k, v in at.items():
            r[int(k[1:])] = v
        return r

    def lgt(B=3, rg=ok, light=GOOD):
        return L.fr_synth_light_rgb(1, 0, B, rg, P(light), P(0))
    assert lgt(B=0) == -1 and lgt(B=-2) == -1 and lgt(B=0, light=0) == -1
    assert lgt(B=65536) == -4 and lgt(B=65536, light=0) == -4 and lgt(B=65536, rg=None) == -4      # the limit comes before the pointers
    assert lgt(light=0) == -1 and lgt(rg=None) == -1
    for bad in (ranges(i0=float("nan")), ranges(i53=float("inf")), ranges(i10=1.0, i11=0.5), ranges(i52=float("-inf"))):
        assert lgt(rg=bad) == -1
        assert lgt(B=65536, rg=bad) == -4                                    # ... and before the ranges

    # the shader: the order of fr_synth_shade, im_rgb in im_gray's place, im_gray nullable
    def shd(B=3, H=17, W=33, bg=0, bgb=0, **nul):
        p = {k: P(0 if k in nul else GOOD) for k in ("t", "n", "ti", "l", "rgb", "gray", "mask")}
        return L.fr_synth_shade_rgb(p["t"], p["n"], p["ti"], p["l"], P(bg), bgb, B, H, W, 1.0, 0.0, p["rgb"], p["gray"], p["mask"], P(0))
    for empty in (dict(B=0), dict(H=0), dict(W=0), dict(B=-1)):
        assert shd(**empty) == -1 and shd(t=0, **empty) == -1
    for kw in (dict(bgb=1), dict(bgb=3), dict(bg=GOOD, bgb=0), dict(bg=GOOD, bgb=2)):
        assert shd(**kw) == -1, kw
        assert shd(B=65536 if "bg" not in kw else 3, **kw) == -1
    for req in ("t", "n", "ti", "l", "rgb", "mask"):
        assert shd(**{req: 0}) == -1, req
        assert shd(B=65536, **{req: 0}) == -1                                # the pointers come before the grid
        assert shd(bgb=1, **{req: 0}) == -1
    for big in (dict(B=65536), dict(H=1 << 16, W=1 << 15), dict(B=65536, gray=0), dict(B=65536, bg=GOOD, bgb=65536),
                dict(H=1 << 16, W=1 << 15, bg=GOOD, bgb=1)):
        assert shd(**big) == -4, big


def test_colour_kernels_keep_everything_in_registers():
    """29 float64 lane trees per tile: the forward holds 58 registers of sums per lane beside the shading.  The compiler's resource
    report must show no scratch and no spill for the colour kernels, the finish step's two instantiations and the shader."""
    h = pkg("_lib")
    want = {"fr_photo.hip": ("photo_loss_rgb_forward_kernel", "photo_loss_rgb_backward_kernel", "photo_loss_finish_kernelILi29E",
                             "photo_loss_finish_kernelILi6E", "photo_loss_forward_kernel", "photo_loss_backward_kernel"),
            "fr_synth.hip": ("synth_shade_rgb_kernel", "synth_light_rgb_kernel")}
    for src, names in want.items():
        cmd = [h._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(h._CSRC, src)]
        out = subprocess.run(cmd, cwd=h._CSRC, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
        for name in names:
            mine = [b for b in blocks if name in b.split("\n", 1)[0]]
            assert len(mine) == 1, (name, [b.split("\n", 1)[0] for b in blocks])
            assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", mine[0]), mine[0][:600]
            assert re.search(r"VGPRs Spill: 0\b", mine[0]) and re.search(r"SGPRs Spill: 0\b", mine[0]), mine[0][:600]
            print(name, re.search(r"VGPRs: (\d+)", mine[0]).group(1), "VGPRs")


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
def test_python_surface_defaults_and_errors():
    losses, ops = pkg("nets.losses"), pkg("rendering_layer.ops")
    assert len(ops.SYNTH_LIGHT_RANGES_RGB) == 27
    for c in range(3):
        assert ops.SYNTH_LIGHT_RANGES_RGB[9 * c:9 * c + 4] == tuple(ops.SYNTH_LIGHT_RANGES)
        assert ops.SYNTH_LIGHT_RANGES_RGB[9 * c + 4:9 * c + 9] == ((-0.15, 0.15),) * 5
    assert list(inspect.signature(ops.photo_loss_rgb).parameters) == list(inspect.signature(ops.photo_loss).parameters)
    assert list(inspect.signature(ops.synth_shade_rgb).parameters) == list(inspect.signature(ops.synth_shade).parameters)
    assert issubclass(ops._PhotoLossRGB, torch.autograd.Function)
    # the parameter list is the gray route's: the colour picture travels in the picture's place
    assert list(inspect.signature(losses.photometric_loss).parameters) == ["face_net", "vertices_proj", "im_gray", "light", "alpha", "weight",
                                                                           "gain", "offset"]
    assert inspect.signature(losses.get_loss).parameters["photo_target_rgb"].default is None
    with pytest.raises(RuntimeError):
        ops.synth_light_rgb(1, 0, 2, device="cpu")                          # a data source on the GPU only: no CPU fallback
    x = torch.zeros(2, 4)
    with pytest.raises(ValueError, match="photo_target_rgb"):
        losses.get_loss(None, None, None, None, None, None, None, photo_target_rgb=torch.zeros(2, 4, 4, 3))
    # the route is chosen by light's shape; the picture has to go with it (checked before anything touches the GPU)
    net = type("N", (), dict(mu_tex=x, pc_tex=x))()
    for light, picture in ((torch.zeros(2, 3, 9), torch.zeros(2, 4, 4)), (torch.zeros(2, 3, 9), torch.zeros(2, 4, 4, 1)),
                           (torch.zeros(2, 3, 4), torch.zeros(2, 4, 4, 3)), (torch.zeros(2, 4), torch.zeros(2, 4, 4, 3))):
        with pytest.raises(ValueError, match="im_rgb"):
            losses.photometric_loss(net, None, picture, light, None)
    sig = inspect.signature(_pipeline().SynthBatches.__init__).parameters
    assert sig["colour"].default is False and list(sig)[-1] == "colour"


def _pipeline():
    return pkg("pipeline")


def test_callers_know_the_flags():
    import importlib.util
    from conftest import ROOT
    for prog, flag, dest in (("coarse_loop.py", "--synth-colour", "synth_colour"), ("photo_fit.py", "--colour", "colour")):
        spec = importlib.util.spec_from_file_location("prog_for_rgb_test_" + dest, os.path.join(ROOT, "examples", prog))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        ap = mod.build_parser()
        assert getattr(ap.parse_args([]), dest) is False and getattr(ap.parse_args([flag]), dest) is True
