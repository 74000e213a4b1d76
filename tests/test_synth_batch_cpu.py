"""CPU: the synthetic-batch feature (csrc/fr_synth.hip, pipeline.SynthBatches).  The numpy model of the GPU tests
(tests/ref_synth_batch.py) is held to Philox4x32-10's published known answers and to the reference sampler's intervals; the face
numbering tiles over ranks; the entry points exist and validate in the header's order before any HIP call; the caller knows its
flag."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, pkg
import ref_synth_batch as RS

F = np.float32
NEW = ("fr_synth_params", "fr_synth_texture", "fr_synth_shade")
LIGHT = ((0.3, 0.7), (-0.4, 0.4), (-0.4, 0.4), (0.2, 0.9))


def _L():
    return pkg("_lib").lib()


# ---- Philox ---------------------------------------------------------------------------------------------------------------------------
# the known answers of the Random123 distribution's kat_vectors for philox4x32 with 10 rounds
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr, key, want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w) for w in RS.philox4x32_10(ctr, key))
    assert got == want, [hex(w) for w in got]


def test_philox_vectorised_equals_scalar():
    rs = np.random.RandomState(5)
    ctr = rs.randint(0, 2 ** 32, (4, 7), dtype=np.uint64)
    key = (0x12345678, 0x9abcdef0)
    got = RS.philox4x32_10(tuple(ctr), key)
    for i in range(7):
        one = RS.philox4x32_10(tuple(int(c) for c in ctr[:, i]), key)
        assert [int(g[i]) for g in got] == [int(w) for w in one]


# ---- the model's ranges ---------------------------------------------------------------------------------------------------------------
def test_uniforms_are_in_the_unit_interval_and_counted_by_global_face():
    u = RS.uniforms(seed=77, first_face=0, B=64, ndraw=249)
    assert u.dtype == F and u.shape == (64, 249)
    assert (u >= 0).all() and (u < 1).all()
    assert 0.45 < u.mean() < 0.55 and u.min() < 0.001 and u.max() > 0.999
    # 24-bit draws: every value is a multiple of 2^-24
    assert np.array_equal(u * F(2.0 ** 24), np.floor(u * F(2.0 ** 24)))
    # rows 5..7 of a batch of 8 are the batch of 3 that starts at face 5; another draw count is a prefix
    assert np.array_equal(u[5:8], RS.uniforms(77, 5, 3, 249))
    assert np.array_equal(u[:, :23], RS.uniforms(77, 0, 64, 23))
    assert not np.array_equal(u, RS.uniforms(78, 0, 64, 249))
    # the counter's word boundary: faces 2^32 - 2 .. 2^32 + 1 are four different faces, the last two with g_hi = 1
    w = RS.uniforms(77, 2 ** 32 - 2, 4, 16)
    assert len({r.tobytes() for r in w}) == 4
    assert np.array_equal(w[2:], RS.uniforms(77, 2 ** 32, 2, 16)) and not np.array_equal(w[2:], RS.uniforms(77, 0, 2, 16))


@pytest.mark.parametrize("beta", [0.7, 1.0])
def test_sampled_parameters_lie_in_the_reference_samplers_intervals(beta):
    ns, ne, K, im = 199, 29, 10, 200
    P, light, alpha, u = RS.sample(31, 0, 256, ns, ne, K, im, beta, LIGHT, [(-1.0, 1.0)] * K)
    assert P.shape == (256, 7 + ns + ne) and P.dtype == F
    # the intervals of get_random_params.m, their ends pushed through the same float32 operations (monotone: pose_intervals)
    iv = RS.pose_intervals(im, beta)
    for c in range(7):
        assert (P[:, c] >= iv[c, 0]).all() and (P[:, c] <= iv[c, 1]).all(), (c, P[:, c].min(), P[:, c].max(), iv[c])
    # ... which are the reference's own to float32 rounding: (1 - beta) [-75, 45] deg, beta im / 2 + (1 - beta) [0, 60], ...
    omb = 1.0 - float(F(beta))
    want = np.array([[-75 * omb * np.pi / 180, 45 * omb * np.pi / 180], [-90 * omb * np.pi / 180, 90 * omb * np.pi / 180],
                     [-30 * omb * np.pi / 180, 30 * omb * np.pi / 180], [beta * im / 2, beta * im / 2 + omb * 60],
                     [beta * im / 2, beta * im / 2 + omb * 60], [0, 0], [beta * 1e-3, beta * 1e-3 + omb * 1e-3]])
    assert np.allclose(iv, want, rtol=8 * 2.0 ** -24, atol=0)      # (at most six roundings, each 2^-24 relative)
    assert (P[:, 5] == 0).all() and not np.signbit(P[:, 5]).any()                       # tz = 0 exactly
    shp, exp = P[:, 7:7 + ns], P[:, 7 + ns:]
    assert (shp >= 0).all() and (shp <= F(1e4)).all() and (exp >= F(-1.5)).all() and (exp <= F(1.5)).all()
    lr = np.asarray(LIGHT, F)
    assert (light >= lr[:, 0]).all() and (light <= lr[:, 1]).all() and (alpha >= -1).all() and (alpha <= 1).all()
    if beta == 1.0:
        base = np.array([0, 0, 0, im / 2, im / 2, 0, F(1e-3)], F)
        assert np.array_equal(P[:, :7], np.repeat(base[None], 256, 0))                  # the pose IS the base
    else:
        assert P[:, :5].std(0).min() > 0 and shp.std() > 1e3 and exp.std() > 0.5


def test_model_texture_and_shade_on_hand_values():
    mu = np.array([[1, 2], [3, 4], [5, 6]], F)
    pc = np.arange(12, dtype=F).reshape(6, 2)
    al = np.array([[1, 0], [0.5, -1]], F)
    t = RS.texture(mu, pc, al)
    assert np.array_equal(t[0].reshape(-1), mu.reshape(-1) + pc[:, 0])
    assert np.array_equal(t[1].reshape(-1), mu.reshape(-1) + pc[:, 0] * F(0.5) - pc[:, 1])
    assert np.array_equal(RS.texture(mu, np.zeros((6, 0), F), np.zeros((3, 0), F)), np.repeat(mu[None], 3, 0))
    tex = np.full((1, 1, 3, 3), 0.6, F)
    nrm = np.array([[[[0, 0, 2], [0, 0, -2], [0, 0, 0]]]], F)
    ti = np.array([[[[0], [5], [-1]]]], F)
    im, mask = RS.shade(tex, nrm, ti, np.array([[0.25, 0, 0, 0.5]], F), background=np.full((1, 1, 3, 1), 9, F), gain=2, offset=1)
    nz = F(2) / (np.sqrt(F(4)) + F(1e-6))
    want = (((F(0.6) + F(0.6)) + F(0.6)) / F(3)) * (F(0.25) + F(0.5) * nz) * F(2) + F(1)
    assert im[0, 0, 0, 0] == want and im[0, 0, 1, 0] == want and im[0, 0, 2, 0] == 9      # the flipped normal shades alike
    assert mask.reshape(-1).tolist() == [1, 1, 0]


# ---- the face numbering -----------------------------------------------------------------------------------------------------------------
def _pipeline():   # (pipeline.py imports torch only; nothing here touches a device)
    return pkg("pipeline")


@pytest.mark.parametrize("world", [1, 2, 8])
def test_face_ranges_tile_the_same_sequence(world):
    rng = _pipeline().synth_face_range
    batch, faces = 3, 48
    steps = faces // (world * batch)
    seen = []
    for step in range(steps):
        for rank in range(world):
            a, b = rng(step, rank, world, batch)
            assert b - a == batch
            seen.extend(range(a, b))
    assert seen == list(range(faces))                      # no gap, no overlap, in order: the single-process sequence
    assert rng(5, 0, 1, 4) == (20, 24)
    for bad in [(-1, 0, 1, 4), (0, 1, 1, 4), (0, -1, 2, 4), (0, 0, 0, 4), (0, 0, 1, 0)]:
        with pytest.raises(ValueError):
            rng(*bad)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_names_in_header_signatures_and_sources():
    host = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "fr_hotpath.h")).read()
    for name in NEW:
        assert name in host.SIGNATURES and name in host.EXPORTS and hasattr(_L(), name), name
        assert ("int %s(" % name) in hdr, name
    assert "fr_synth.hip" in host.SOURCES and os.path.exists(os.path.join(ROOT, "3dfacerecon_amd", "csrc", "fr_synth.hip"))
    assert "FR_SYNTH_MAX_TEX = 64" in hdr


GOOD = 0x1000   # a made-up device address: every check below answers before any HIP call


def _ranges(pairs):
    return (ctypes.c_float * (2 * len(pairs)))(*[v for p in pairs for v in p])


def test_sampler_checks_in_the_headers_order():
    L = _L()
    lr, ar = _ranges(LIGHT), _ranges([(-1, 1)] * 10)

    def call(**kw):
        a = dict(B=3, ns=9, ne=5, K=10, im=32.0, beta=0.7, focal=1e-3, lr=lr, ar=ar, params=GOOD, light=GOOD, alpha=GOOD)
        a.update(kw)
        return L.fr_synth_params(1, 0, a["B"], a["ns"], a["ne"], a["K"], a["im"], a["beta"], a["focal"], a["lr"], a["ar"],
                                 a["params"], a["light"], a["alpha"], None)
    nan, inf = float("nan"), float("inf")
    invalid = [dict(B=0), dict(B=-1), dict(ns=-1), dict(ne=-1), dict(K=-1), dict(beta=-0.1), dict(beta=1.5), dict(beta=nan),
               dict(im=inf), dict(focal=nan)]
    unsupported = [dict(K=65), dict(B=65536), dict(ns=2 ** 31 - 70)]
    null = [dict(params=None), dict(light=None), dict(lr=None), dict(alpha=None), dict(ar=None)]
    ranges = [dict(lr=_ranges(((0.7, 0.3),) + LIGHT[1:])), dict(lr=_ranges((((nan, 1.0)),) + LIGHT[1:])),
              dict(ar=_ranges([(-1, 1)] * 9 + [(0, inf)])), dict(ar=_ranges([(2, 1)] + [(-1, 1)] * 9))]
    for d in invalid + null + ranges:
        assert call(**d) == -1, d
    for d in unsupported:
        assert call(**d) == -4, d
    # the earlier item wins: a bad size before an unserved one, an unserved one before a NULL, a NULL before a bad range
    assert call(B=0, K=65) == -1 and call(K=65, params=None) == -4 and call(B=65536, lr=None) == -4
    assert call(params=None, lr=_ranges(((0.7, 0.3),) + LIGHT[1:])) == -1 and call(beta=nan, K=65) == -1


def test_texture_and_shade_checks():
    L = _L()

    def tex(**kw):
        a = dict(mu=GOOD, pc=GOOD, al=GOOD, B=3, N=40, K=10, out=GOOD)
        a.update(kw)
        return L.fr_synth_texture(a["mu"], a["pc"], a["al"], a["B"], a["N"], a["K"], a["out"], None)
    for d in [dict(B=0), dict(N=0), dict(K=-1), dict(B=-2), dict(mu=None), dict(out=None), dict(pc=None), dict(al=None)]:
        assert tex(**d) == -1, d
    assert tex(B=65536) == -4 and tex(B=65536, mu=None) == -4 and tex(B=0, mu=None) == -1

    def shade(**kw):
        a = dict(t=GOOD, n=GOOD, ti=GOOD, l=GOOD, bg=None, bgb=0, B=3, H=5, W=6, im=GOOD, mask=GOOD)
        a.update(kw)
        return L.fr_synth_shade(a["t"], a["n"], a["ti"], a["l"], a["bg"], a["bgb"], a["B"], a["H"], a["W"], 1.0, 0.0, a["im"],
                                a["mask"], None)
    for d in [dict(B=0), dict(H=0), dict(W=-1), dict(bgb=1), dict(bg=GOOD, bgb=0), dict(bg=GOOD, bgb=2), dict(t=None), dict(n=None),
              dict(ti=None), dict(l=None), dict(im=None), dict(mask=None)]:
        assert shade(**d) == -1, d
    assert shade(H=1 << 16, W=1 << 15) == -4 and shade(B=65536) == -4 and shade(B=65536, t=None) == -1


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
def test_operators_and_pipeline_surface():
    import inspect
    ops, pipe = pkg("rendering_layer.ops"), _pipeline()
    for name in ("synth_params", "synth_texture", "synth_shade"):
        assert callable(getattr(ops, name)), name
    sig = inspect.signature(pipe.SynthBatches.__init__).parameters
    for name, dflt in (("slots", 2), ("first_face", 0), ("stride", None), ("background", None), ("gain", 1.0), ("offset", 0.0)):
        assert sig[name].default == dflt, name
    assert list(sig)[1:4] == ["net", "batch", "seed"] and "light_ranges" in sig and "alpha_ranges" in sig
    assert callable(pipe.SynthBatches.next)
    with pytest.raises(RuntimeError):
        ops.synth_params(1, 0, 2, 9, 5, 3, 32, device="cpu")              # a data source on the GPU only: no CPU fallback


def test_caller_knows_the_flag():
    spec = importlib.util.spec_from_file_location("coarse_loop_for_synth_test", os.path.join(ROOT, "examples", "coarse_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    a = ap.parse_args(["--synth-data", "--synth-seed", "9"])
    assert a.synth_data is True and a.synth_seed == 9
    b = ap.parse_args([])
    assert b.synth_data is False and isinstance(b.synth_seed, int)
