"""GPU: the Q30 decode forward (fr_decode_3dmm_q30_lv / fr_decode_render_forward_q30, csrc/fr_decode_q.hip) held to its written
definition (oracle/fr_oracle.c "Q30 decode") at every schedule the launcher can pick, at every level count and at the edges of its
domain -- the treatment tests/test_decode_forward_edges_gpu.py gives the f32 decode, whose rig this file extends.

Everything is compared with oracle.decode_3dmm_q30(..., R=R, levels=lv) by BIT PATTERN (gpu_util.assert_bits_equal).  The C entry
points are called through ctypes; the rotation is supplied by the host unless a test is about the in-kernel one; every output is
pre-filled with a finite sentinel, so an element the kernel does not write is a mismatch too.  Shapes are chosen by asking the
launcher's own decision function (fr_debug_decode_q_geom, with the CU count the launcher plans for) which (N, B) reach a geometry.
FR_DECODE_CUS (a test knob: the launchers plan for min(n, device) compute units) is what lets a mesh of a thousand vertices walk
several ragged rounds of tiles per wave -- the ring wrapping from one tile's last fragments into the next tile's first, the payload
slot rewritten for the second tile, the re-request at the end of a walk.  The oracle result of a (shape, N, B, levels) is computed
once and shared by every schedule."""
import ctypes
import time

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import assert_bits_equal
from test_decode_forward_edges_gpu import (ANGLES, BAD_ANGLES, BAND, CLEAN_FACES, IM, N_SPECIAL_FACES, PATTERN, SENTINEL, Rig,
                                           _guarded, rand_params, special_params)

pytestmark = pytest.mark.gpu

QFIELDS = ("b0", "cols", "kernel", "nbw", "waves", "h2", "ring", "launches", "lds", "grid")
GENERIC, RING = 0, 1
LEVELS = (7, 5, 4)
SCHEDULES = [{}, {"FR_Q30_SCHED": 1}, {"FR_DECODE_IMPL": 1}]
# four shapes of 15 live 16-coefficient groups (the ring kernel): the model's, one live coefficient in the last group, the last
# group full, no shape basis; then 14 groups and 16 groups (generic: with 4 groups in the last k-step the payload cannot ride in
# a short fragment), and a small shape
FAMILIES = [(199, 29), (225, 0), (211, 29), (0, 230), (200, 24), (212, 29), (33, 16)]
RING_FAMILIES = FAMILIES[:4]
CAPS = (1, 2, 3, 8)


def _sid(k):
    return "-".join("%s%d" % (n[3:], v) for n, v in k.items()) or "default"


def _h():
    return pkg("_lib")


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def qgeom(B, N, ns, ne, lv, cap=0):
    """[{field: value} per pass] of the Q30 launcher under the current knobs, planning for what FR_DECODE_CUS = cap makes it plan for"""
    out = (ctypes.c_int * (1 + 10 * ((B + 63) // 64 + 1)))()
    rc = _h().lib().fr_debug_decode_q_geom(B, N, ns, ne, lv, min(cap, _cus()) if cap else _cus(), out)
    assert rc == 0, rc
    return [dict(zip(QFIELDS, out[1 + 10 * i:11 + 10 * i])) for i in range(out[0])]


def rounds(p, N):
    """(rounds of tiles a slot of pass p walks, tiles in the last round, tiles a full round holds)"""
    tiles = (N + 15) // 16
    per = (p["waves"] // p["h2"]) * p["grid"]
    return -(-tiles // per), tiles - (-(-tiles // per) - 1) * per, per


def _gline(g):
    return " | ".join("%s nbw%d w%d h%d r%d x%d grid%d" % (("generic", "ring")[p["kernel"]], p["nbw"], p["waves"], p["h2"], p["ring"],
                                                            p["launches"], p["grid"]) for p in g)


# ---- rig: the f32 file's bases and parameter zoo, packed into the Q30 image and decoded through the Q30 entry points -------------
class QRig(Rig):
    def __init__(self, ns, ne, N, signed_zero=False, arrays=None):
        if arrays is None:
            Rig.__init__(self, ns, ne, N, signed_zero)
        else:
            self.ns, self.ne, self.N = ns, ne, N
            self.mu, self.pc_shape, self.pc_exp = (np.ascontiguousarray(a, np.float32) for a in arrays)
            assert self.mu.shape == (3 * N,) and self.pc_shape.shape == (3 * N, ns) and self.pc_exp.shape == (3 * N, ne)
        self._qimage = None

    def pack_into(self, ptr, nbytes):
        h = _h()
        dev = torch.device("cuda:0")
        t = [torch.as_tensor(a, device=dev) for a in (self.mu, self.pc_shape, self.pc_exp)]
        rc = h.lib().fr_decode_q30_pack(h.ptr(t[0]), h.ptr(t[1]), h.ptr(t[2]), self.N, self.ns, self.ne, ptr, nbytes, h.stream_ptr(dev))
        h.check(rc, "fr_decode_q30_pack")
        torch.cuda.synchronize()

    @property
    def qimage(self):
        if self._qimage is None:
            nbytes = _h().lib().fr_decode_q30_image_bytes(self.N, self.ns, self.ne)
            assert nbytes > 0
            self._qimage = torch.empty((nbytes,), dtype=torch.uint8, device="cuda:0")
            assert self._qimage.data_ptr() % 256 == 0
            self.pack_into(_h().ptr(self._qimage), nbytes)
        return self._qimage

    def decode(self, P, R=None, lv=7, im=IM, ws=None, qimage=None):
        h = _h()
        L = h.lib()
        dev = torch.device("cuda:0")
        B = P.shape[0]
        p = torch.as_tensor(np.ascontiguousarray(P, np.float32), device=dev)
        r = None if R is None else torch.as_tensor(np.ascontiguousarray(R, np.float32).reshape(B, 9), device=dev)
        nws = L.fr_decode_q30_workspace_bytes(self.ns, self.ne)
        ws = torch.empty((nws,), dtype=torch.uint8, device=dev) if ws is None else ws
        qimage = self.qimage if qimage is None else qimage
        assert ws.numel() == nws
        out = torch.full((B, 3, self.N), SENTINEL, dtype=torch.float32, device=dev)
        rc = L.fr_decode_3dmm_q30_lv(h.ptr(p), h.ptr(qimage), h.ptr(r), B, self.N, self.ns, self.ne, float(im), lv, h.ptr(out),
                                     h.ptr(ws), nws, h.stream_ptr(dev))
        h.check(rc, "fr_decode_3dmm_q30_lv")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def oracle(self, O, P, R=None, lv=7, im=IM):
        return O.decode_3dmm_q30(P, self.mu, self.pc_shape, self.pc_exp, im, R=R, levels=lv)


_QRIGS, _WANT, SPEC_SECONDS = {}, {}, [0.0]


def qrig(ns, ne, N, signed_zero=False):
    k = (ns, ne, N, signed_zero)
    if k not in _QRIGS:
        _QRIGS[k] = QRig(ns, ne, N, signed_zero)
    return _QRIGS[k]


def spec(O, g, P, R, lv):
    t0 = time.time()
    want = g.oracle(O, P, R, lv)
    SPEC_SECONDS[0] += time.time() - t0
    want.setflags(write=False)
    return want


def case(O, ns, ne, N, B, lv):
    """(rig, P, R, spec result) of a random batch, computed once per (shape, N, B, levels) and shared by every schedule"""
    k = (ns, ne, N, B, lv)
    if k not in _WANT:
        g = qrig(ns, ne, N)
        P = rand_params(np.random.RandomState(7 * N + B), B, ns, ne)
        R = O.rotation_matrix_batch(P[:, :3])
        _WANT[k] = (g, P, R, spec(O, g, P, R, lv))
    return _WANT[k]


# ---- 1. schedule x geometry matrix ------------------------------------------------------------------------------------------------
# every batch boundary of the launcher (1, 2, 3, 4 live column blocks, their edges, a second and a third pass) at small meshes of
# every raggedness: N mod 16 = 13, 4, 3, 0, 1, 15, 15, 1, 0, 13 (one tile of 13 vertices), 1; 9, 7, 7, 6, 5, 4, 2, 2, 3, 1, 3 tiles
# -- at most one tile per wave, and with 1 .. 7 tiles fewer tiles than the 8 (or 6) slots of one workgroup: the waves past the
# last tile leave after the prologue's requests
SMALL = ((141, 1), (100, 16), (99, 17), (96, 32), (65, 33), (63, 48), (31, 49), (17, 64), (48, 65), (13, 128), (33, 129))
B_MULTI = (64, 5, 20, 40)        # a full pass, and one batch each of 1, 2 and 3 live column blocks
_MULTI_N = {}


def _all_passes(N, ns, ne, lv, cap):
    """the passes of the four B_MULTI batches under each schedule of the matrix"""
    ps = []
    for knobs in SCHEDULES:
        with _h().options(**knobs):
            for B in B_MULTI:
                ps += qgeom(B, N, ns, ne, lv, cap)
    return ps


def multi_round_n(ns, ne, lv):
    """(N3, N8): the smallest N from 700 at which, under every schedule of the matrix and for every batch of B_MULTI, every wave slot
    walks at least three rounds of tiles with a ragged last one when the launcher plans for 1, 2 and 3 compute units; and the smallest
    at which a plan for 8 launches exactly 8 workgroups (tile_walk's `(grid & 7) == 0` permutation) that walk at least three rounds
    too, the last one ragged: every slot then has a middle tile, one that the ring wraps into and out of.  One N per (family,
    levels) for all schedules, so that they share the spec result."""
    k = (ns, ne, lv)
    if k not in _MULTI_N:
        def ok3(N):
            return all(rounds(p, N)[0] >= 3 and rounds(p, N)[1] < rounds(p, N)[2] for cap in CAPS[:3] for p in _all_passes(N, ns, ne, lv, cap))

        def ok8(N):
            return all(p["grid"] == 8 and rounds(p, N)[0] >= 3 and rounds(p, N)[1] < rounds(p, N)[2] for p in _all_passes(N, ns, ne, lv, 8))
        n3 = next(N for N in range(700, 4225) if N % 16 and ok3(N))
        n8 = next(N for N in range(700, 4225) if N % 16 and ok8(N))
        _MULTI_N[k] = (n3, n8)
    return _MULTI_N[k]


@pytest.mark.parametrize("ns,ne", FAMILIES, ids=["%d+%d" % f for f in FAMILIES])
@pytest.mark.parametrize("knobs", SCHEDULES, ids=_sid)
@pytest.mark.parametrize("lv", LEVELS, ids=["levels%d" % l for l in LEVELS])
def test_schedule_geometry_matrix(oracle, lv, knobs, ns, ne):
    h = _h()
    assert _cus() >= 8, "the capped cells are written for a part of at least 8 compute units"
    n3, n8 = multi_round_n(ns, ne, lv)
    pts = [(N, B, 0) for N, B in SMALL] + [(n3, B, cap) for cap in CAPS[:3] for B in B_MULTI] + [(n8, B, 8) for B in B_MULTI]
    ring_family = (ns, ne) in RING_FAMILIES
    sched1 = knobs.get("FR_Q30_SCHED") == 1
    with h.options(**knobs):
        geoms = [qgeom(B, N, ns, ne, lv, cap) for N, B, cap in pts]
        # the cell reaches what it was written for
        want_kernel = RING if ring_family and not knobs.get("FR_DECODE_IMPL") else GENERIC
        assert all(p["kernel"] == want_kernel for g in geoms for p in g), (want_kernel, geoms)
        for part in (geoms[:len(SMALL)], geoms[len(SMALL):]):       # at one tile per wave AND over several rounds
            reached = {(p["nbw"], p["waves"], p["h2"], p["launches"]) for g in part for p in g}
            if want_kernel == GENERIC:
                assert reached == {(1, 8, 1, 1), (2, 8, 1, 1), (2, 8, 1, 2)}, reached
            elif sched1:      # 3-4 live blocks: the halves schedule, on 12 waves with all seven levels
                assert reached == {(1, 8, 1, 1), (2, 8, 1, 1), (2, 12 if lv == 7 else 16, 2, 1)}, reached
            else:
                assert reached == {(1, 8, 1, 1), (2, 8, 1, 1), (4, 8, 1, 1)}, reached
        if want_kernel == RING and sched1:
            for (N, B, cap), g in zip(pts, geoms):
                assert all((p["h2"] == 2) == (p["cols"] > 32) for p in g), (N, B, g)
            # 33 .. 48 columns: the second wave of a pair owns one live and one dead column block
            assert any(p["h2"] == 2 and 32 < p["cols"] <= 48 for g in geoms[:len(SMALL)] for p in g)
            assert any(p["h2"] == 2 and 32 < p["cols"] <= 48 for g in geoms[len(SMALL):] for p in g)
        for (N, B, cap), g in zip(pts, geoms):
            for p in g:
                tiles, slots = (N + 15) // 16, p["waves"] // p["h2"]
                if cap:
                    assert -(-tiles // slots) > p["grid"] and p["grid"] == min(cap, _cus()), (N, B, cap, p)
                    assert rounds(p, N)[0] >= 3 and rounds(p, N)[1] < rounds(p, N)[2], (N, B, cap, p)
                else:
                    assert rounds(p, N)[0] == 1, (N, B, p)
        assert any(p["grid"] == 8 for (N, B, cap), g in zip(pts, geoms) if cap == 8 for p in g)
        assert {N % 16 for N, _, _ in pts} >= {0, 1, 3, 4, 13, 15} and any(N < 16 for N, _, _ in pts)
        assert {((N + 15) // 16) & 1 for N, _ in SMALL} == {0, 1} and any((N + 15) // 16 < 6 for N, _ in SMALL)
        assert {B for _, B in SMALL} == {1, 16, 17, 32, 33, 48, 49, 64, 65, 128, 129}
        # the block of this cell in profiles/decode_q30_schedule_matrix.txt: per variant its grids, the rounds walked under a cap
        agg = {}
        for (N, B, cap), g in zip(pts, geoms):
            for p in g:
                a = agg.setdefault(_gline([p]).rsplit(" grid", 1)[0], (set(), set(), set()))
                a[0].add(p["grid"])
                if cap:
                    a[1].add(rounds(p, N)[0])
                if p["h2"] == 2 and 32 < p["cols"] <= 48:
                    a[2].add(1)
        print("\nlevels%d %s %d+%d\n" % (lv, _sid(knobs), ns, ne) + "\n".join(
            "    %s grids %s%s%s" % (k, sorted(a[0]), " rounds %s" % sorted(a[1]) if a[1] else "", " half-dead pair" if a[2] else "")
            for k, a in agg.items()))
        for N, B, cap in pts:
            g, P, R, want = case(oracle, ns, ne, N, B, lv)
            with h.options(FR_DECODE_CUS=cap):
                got = g.decode(P, R, lv)
            assert_bits_equal(got, want, "levels%d %s %d+%d N=%d B=%d cus=%d" % (lv, _sid(knobs), ns, ne, N, B, cap))


# ---- 2. special values ----------------------------------------------------------------------------------------------------------------
_SPECIAL = {}


def special_case(O, ns, ne, N, lv):
    k = (ns, ne, N, lv)
    if k not in _SPECIAL:
        g = qrig(ns, ne, N, signed_zero=True)
        P, R = special_params(O, ns, ne)
        _SPECIAL[k] = (g, P, R, spec(O, g, P, R, lv))
    return _SPECIAL[k]


@pytest.mark.parametrize("ns,ne,N", [(199, 29, 150), (33, 16, 99)], ids=["ring", "generic"])
@pytest.mark.parametrize("knobs", SCHEDULES, ids=_sid)
@pytest.mark.parametrize("lv", LEVELS, ids=["levels%d" % l for l in LEVELS])
def test_special_values(oracle, lv, knobs, ns, ne, N):
    """The 24 special faces of the f32 suite (special_params) over its signed-zero basis: Inf / NaN parameters poison their own face
    and no other; subnormal parameters; 3e38 and a blend beyond fp32; zero, -0.0 and alternating-zero coefficient rows over mu
    entries of -0.0; f in {0, -0.0, -1e-3, 1e-41, Inf}; a non-finite t component -- bit for bit the spec's, NaN for NaN, in every
    schedule, at 70 faces (64 + 6), 64, 33 and 24.

    What the Q30 definition yields where the f32 chain is sign-sensitive (printed below): the blend is ONE rounding of
    mu + I 2^e with I an integer, so a zero blend (all coefficients 0 or -0.0: faces 3, 10, 21) is the exact +0, and mu + 0 keeps
    mu's value but not the sign of a -0.0 mu (-0.0 + +0.0 = +0.0): those vertices come out +0.0, and f = -1 (face 21) turns them into
    -0.0 in the epilogue alone.  Coefficients of 1e-45 (face 12) are not lost one product at a time as in the f32 chain: the face's
    own exponent scales them to full 31-bit operands, and the sum is rounded to fp32 once -- to a zero of the sum's sign where it is
    below half the smallest subnormal."""
    g, P, R, want = special_case(oracle, ns, ne, N, lv)
    # the spec's own picture: the cases are alive
    assert np.isnan(want[1]).all() and np.isnan(want[2]).all(), "a non-finite parameter makes the face's vertices NaN"
    assert np.isfinite(want[list(CLEAN_FACES)]).all() and np.isfinite(want[N_SPECIAL_FACES:]).all()
    assert np.isfinite(want[5]).all() and not np.isfinite(want[9]).all() and not np.isfinite(want[17]).all()
    for b in (18, 19, 20):
        assert np.isfinite(want[b]).any() and not np.isfinite(want[b]).all()
    u = want.view(np.uint32)
    neg0 = {b: int((u[b][[0, 2]] == 0x80000000).sum()) for b in (3, 10, 12, 21)}
    pos0 = {b: int((u[b][[0, 2]] == 0).sum()) for b in (3, 10, 12, 21)}
    if knobs == {}:
        print("\nlevels%d %d+%d: x / z elements that are -0.0 per face %r, +0.0 %r (of %d each over a mu of -0.0, %d over +0.0)" % (
            lv, ns, ne, neg0, pos0, 2 * len(range(0, N, 3)), 2 * len(set(range(1, N, 7)) - set(range(0, N, 3)))))
    # zero blends: +0.0 over a mu of either sign (faces 3, 10), -0.0 only through f = -1 (face 21)
    zero_mu = sorted(set(range(0, N, 3)) | set(range(1, N, 7)))
    assert (u[3][[0, 2]][:, zero_mu] == 0).all() and (u[10][[0, 2]][:, zero_mu] == 0).all()
    assert (u[21][[0, 2]][:, zero_mu] == 0x80000000).all()
    with _h().options(**knobs):
        for B in (70, 64, 33, 24):
            got = g.decode(P[:B], R[:B], lv)
            assert np.array_equal(np.isnan(got), np.isnan(want[:B])), "levels%d %s B=%d: NaN mask" % (lv, _sid(knobs), B)
            assert_bits_equal(got, want[:B], "levels%d %s %d+%d B=%d" % (lv, _sid(knobs), ns, ne, B))


# ---- 3. special basis on the ring shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv", LEVELS, ids=["levels%d" % l for l in LEVELS])
def test_special_basis_through_the_ring(oracle, lv):
    """A NaN / Inf basis entry (the packed row's e10 == 1023, which reaches the ring kernel in lanes 48 .. 63 of a tile's first
    fragment) poisons its own vertex and nothing else -- in the first tile, in the last (ragged) tile and, with the launcher
    planning for one compute unit, in tiles a wave reaches in its second and third round; an all-zero column, all-zero rows, a
    column 1e30 times and one 1e-30 times the rest follow the spec.  40 faces: three live column blocks."""
    ns, ne, N, B = 199, 29, 300, 40
    base = qrig(ns, ne, N)
    S, E = base.pc_shape.copy().reshape(3, N, ns), base.pc_exp.copy().reshape(3, N, ne)
    (p,) = qgeom(B, N, ns, ne, lv, 1)    # what the launcher plans under FR_DECODE_CUS = 1, default schedule
    per = rounds(p, N)[2]
    assert p["kernel"] == RING and p["grid"] == 1 and rounds(p, N)[0] == 3 and rounds(p, N)[1] < per
    # the kernels' own walk deals the first `per` tiles one to each slot of the one workgroup (fr_debug_decode_walk), and a slot's
    # stride is `per`: tile t is reached in round t // per
    visits = (ctypes.c_int * (per * p["h2"]))()
    assert _h().lib().fr_debug_decode_walk(per, p["waves"], p["h2"], 1, visits) == 0 and list(visits) == [1] * (per * p["h2"])
    t2, t3 = per, 2 * per                # a tile of the second round and one of the third
    assert (t2 // per, t3 // per) == (1, 2) and 16 * t3 + 15 < N
    bad = {7: (0, "S", 0, np.nan), 9: (1, "E", 2, np.inf), N - 2: (2, "S", ns - 1, np.nan), 16 * t2 + 5: (0, "E", ne - 1, -np.inf),
           16 * t2 + 15: (2, "S", 100, np.nan), 16 * t3 + 0: (1, "S", 64, np.inf)}
    for v, (c, which, k, x) in bad.items():
        (S if which == "S" else E)[c, v, k] = x
    S[:, :, 4] = 0.0                     # an all-zero column
    for v in (20, 16 * t2 + 12):         # all-zero rows (one coordinate; all three)
        S[1, v, :] = 0.0
        E[1, v, :] = 0.0
    S[:, 16 * t3 + 3, :] = 0.0
    E[:, 16 * t3 + 3, :] = 0.0
    S[:, :, 9] *= np.float32(1e30)
    E[:, :, 1] *= np.float32(1e-30)
    g = QRig(ns, ne, N, arrays=(base.mu, S.reshape(3 * N, ns), E.reshape(3 * N, ne)))
    P = rand_params(np.random.RandomState(2), B, ns, ne)
    P[:, 7 + 9] *= np.float32(1e-30)
    R = oracle.rotation_matrix_batch(P[:, :3])
    want = spec(oracle, g, P, R, lv)
    mask = np.zeros((B, 3, N), bool)
    mask[:, :, sorted(bad)] = True
    assert np.array_equal(np.isnan(want), mask) and np.isfinite(want[~mask]).all(), "each non-finite entry poisons its own vertex only"
    for knobs in SCHEDULES[:2]:
        for cap in (0, 1):
            with _h().options(FR_DECODE_CUS=cap, **knobs):
                assert all(q["kernel"] == RING for q in qgeom(B, N, ns, ne, lv, cap))
                got = g.decode(P, R, lv)
            assert np.array_equal(np.isnan(got), mask), "levels%d %s cus=%d: NaN mask" % (lv, _sid(knobs), cap)
            assert_bits_equal(got, want, "levels%d %s cus=%d" % (lv, _sid(knobs), cap))
    with _h().options(FR_DECODE_IMPL=1):
        assert_bits_equal(g.decode(P, R, lv), want, "levels%d generic" % lv)


# ---- 4. accumulator bound -------------------------------------------------------------------------------------------------------------
def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


# fp32 magnitudes whose 31-bit quantisation against their own power of two, q = rint(m 2^30) with m the frexp mantissa, has the
# balanced base-256 digits (most significant first) ... -- test_accumulator_bound asserts them through the spec's own steps
TOP = _bits(0x3FFFFFFF)          # m = 1 - 2^-24:  q = 2^30 - 64 = 0x3FFFFFC0:  (64, 0, 0, -64): the largest leading digit
NEG = _bits(0x3F7DFDFE)          # m = 0.99215..:  q = 2^30 - 0x808080:         (64, -128, -128, -128): the most negative digit pattern
POW2 = np.float32(1.0)           # m = 1 / 2:      q = 2^29:                    (32, 0, 0, 0)
DIGITS = {"pow2": (32, 0, 0, 0), "top": (64, 0, 0, -64), "alternating": (64, 0, 0, -64), "negative-digits": (64, -128, -128, -128)}


def _digits(q):
    """balanced base-256 digits of the int64 array q, most significant first (fr_q30_digits of the spec)"""
    d = []
    for _ in range(3):
        l = ((q + 128) & 255) - 128
        d.append(l)
        q = (q - l) >> 8
    return [q] + d[::-1]


def q30_level_sums(A, x):
    """the spec's quantisation of a basis A [rows, K] and of parameter rows x [B, K], restated in numpy (oracle/fr_oracle.c "Q30 decode":
    ce, re, be, qA, qB): (digits of qA [4][rows, K], digits of qB [4][B, K], level sums L [7][rows, B] with L_s = sum_k sum_{i+j=s} a_i b_j)"""
    A, x = A.astype(np.float64), x.astype(np.float64)
    cmax = np.abs(A).max(axis=0)
    ce = np.where(cmax > 0, np.frexp(cmax)[1], 0)
    ea = np.where(A != 0, np.frexp(A)[1] - ce[None], -10 ** 6)
    re = np.where((A != 0).any(axis=1), ea.max(axis=1), 0)
    qA = np.rint(np.ldexp(A, 30 - re[:, None] - ce[None])).astype(np.int64)
    ex = np.where(x != 0, np.frexp(x)[1] + ce[None], -10 ** 6)
    be = np.where((x != 0).any(axis=1), ex.max(axis=1), 0)
    qB = np.rint(np.ldexp(x, ce[None] + 30 - be[:, None])).astype(np.int64)
    da, db = _digits(qA), _digits(qB)
    L = [sum(da[i] @ db[s - i].T for i in range(4) if 0 <= s - i < 4) for s in range(7)]
    return da, db, L


@pytest.mark.parametrize("variant", ["pow2", "top", "alternating", "negative-digits"])
def test_accumulator_bound(oracle, variant):
    """512 coefficients (the most the Q30 kernels take), every basis entry and every parameter at its row / column maximum, so that
    every term of a level sum has the largest digits the quantisation can produce: q_finish's claim "|L_0| <= 2^21 and |L_1| <= 2^23,
    so L_0 * 256 + L_1 is exact in int32" and the int32 level accumulators are held at the bound.
      pow2: +-2^e, all one sign per row (digits 32, 0, 0, 0: |L_0| = 512 * 32 * 32 = 2^19)
      top: the fp32 numbers just below a power of two (digits 64, 0, 0, -64): L_0 = 512 * 64 * 64 = 2^21, the stated bound itself
      alternating: `top` with alternating signs along k in the basis (every level sum cancels to 0) and along the faces in the parameters
      negative-digits: (64, -128, -128, -128) on both sides: L_0 = 2^21 and L_1 = -512 * 2 * 64 * 128 = -2^23, both stated bounds
      themselves, L_2 = 512 * (-2 * 64 + 128) * 128 = 0, L_3 = 512 * 2 * (128 * 128 - 64 * 128) = 2^23, L_4 = 3 * 2^23 below.
    The digits and the level sums are asserted here through a numpy restatement of the spec's quantisation (q30_level_sums), so a
    constant that misses its pattern fails instead of passing as a weaker case.  The integer I is about 2^69: the spec takes its level
    chain with its own float64 roundings, which the kernel must follow."""
    ns, ne, N, B = 512, 0, 40, 64
    rs = np.random.RandomState(5)
    c = {"pow2": POW2, "top": TOP, "alternating": TOP, "negative-digits": NEG}[variant]
    S = np.full((3 * N, ns), c, np.float32) * np.float32(2.0 ** -7)       # basis entries of 2^-7 scale ...
    x = np.full((B, ns), c, np.float32) * np.float32(2.0 ** 13)           # ... against parameters of 2^13 scale
    if variant == "alternating":
        S[:, 1::2] *= -1
        S[1::2] *= -1
        x[1::2] *= -1
    if variant == "pow2":
        S[N:2 * N] *= -1                                                   # one sign per row: the y rows negative
    # what the variant relies on: every operand has the digit pattern, and the level sums sit where the docstring puts them
    da, db, L = q30_level_sums(S, x)
    for i, d in enumerate(DIGITS[variant]):
        assert (np.abs(da[i]) == abs(d)).all() and (np.abs(db[i]) == abs(d)).all(), (variant, i, d, da[i][0, :4], db[i][0, :4])
        assert (da[i] * np.sign(S) == d).all() and (db[i] * np.sign(x) == d).all(), (variant, i)
    want_L = {"pow2": (2 ** 19, 0, 0), "top": (2 ** 21, 0, 0), "alternating": (0, 0, 0), "negative-digits": (2 ** 21, 2 ** 23, 0)}[variant]
    for s_, w in enumerate(want_L):
        assert np.abs(L[s_]).max() == w and np.abs(L[s_]).min() == w, (variant, s_, int(np.abs(L[s_]).max()), w)
    if variant == "negative-digits":
        assert (L[1] == -2 ** 23).all() and (L[3] == 2 ** 23).all() and (L[4] == 3 * 2 ** 23).all()
    assert max(int(np.abs(l).max()) for l in L) < 2 ** 31 and int(np.abs(L[0] * 256 + L[1]).max()) < 2 ** 31
    mu = rs.uniform(-1e5, 1e5, 3 * N).astype(np.float32)
    g = QRig(ns, ne, N, arrays=(mu, S, np.zeros((3 * N, 0), np.float32)))
    P = rand_params(rs, B, ns, ne)
    P[:, 7:] = x
    R = oracle.rotation_matrix_batch(P[:, :3])
    for lv in LEVELS:
        (p,) = qgeom(B, N, ns, ne, lv)
        assert p["kernel"] == GENERIC and p["launches"] == 2 and p["lds"] == 8 * 16384 + 3328
        want = spec(oracle, g, P, R, lv)
        assert np.isfinite(want).all()
        if variant != "alternating":   # the blend is alive: 512 * c^2 * 2^6 ~ 2^15 .. 2^17 beside a mu below 2^17
            I = np.tile(np.eye(3, dtype=np.float32)[None], (B, 1, 1))
            P1 = P.copy()
            P1[:, 3:6] = 0
            P1[:, 6] = 1.0
            v = g.oracle(oracle, P1, I, lv)[:, 0].astype(np.float64) - mu[None, :N]
            assert np.allclose(v, 512.0 * float(c) ** 2 * 64.0, rtol=1e-3), (variant, lv, v.min(), v.max())
        assert_bits_equal(g.decode(P, R, lv), want, "%s levels%d" % (variant, lv))


# ---- 5. in-kernel rotation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,ne,N", [(199, 29, 40), (9, 5, 40)], ids=["ring", "generic"])
def test_in_kernel_rotation_edges(oracle, ns, ne, N):
    """q_stage_kernel's float64 rotation (R_override = NULL) at the angles of the f32 suite's test: exact zeros of both signs,
    multiples of pi / 2, a subnormal, arguments that need a full range reduction, and non-finite angles.  The project's rule: the
    same NaN faces as the spec with glibc's sin / cos (all of the face for gamma and theta; phi leaves the x row), the rest within
    2 fp32 ulp of max(|want|, 1)."""
    g = qrig(ns, ne, N)
    nv = len(ANGLES)
    B = 4 * nv + 4 * len(BAD_ANGLES) + 2
    P = rand_params(np.random.RandomState(11), B, ns, ne)
    for i, v in enumerate(ANGLES):
        P[4 * i, 0:3] = v
        for j in range(3):
            P[4 * i + 1 + j, j] = v
    bad0 = 4 * nv
    for i, v in enumerate(BAD_ANGLES):
        P[bad0 + 4 * i, 0:3] = v
        for j in range(3):
            P[bad0 + 4 * i + 1 + j, j] = v
    good = [b for b in range(B) if not bad0 <= b < bad0 + 4 * len(BAD_ANGLES)]
    for lv in (7, 4):
        assert qgeom(B, N, ns, ne, lv)[0]["kernel"] == (RING if ns == 199 else GENERIC)
        want = spec(oracle, g, P, None, lv)
        got = g.decode(P, None, lv)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        for i in range(len(BAD_ANGLES)):
            f = bad0 + 4 * i
            assert np.isnan(got[[f, f + 2, f + 3]]).all()                  # all three, gamma alone, theta alone
            assert np.isnan(got[f + 1, 1:]).all() and not np.isnan(got[f + 1, 0]).any()   # phi alone: the x row does not see it
        assert not np.isnan(got[good]).any()
        w, q = want[good], got[good]
        ulp = np.spacing(np.maximum(np.abs(w), np.float32(1.0)))
        err = np.abs(q.astype(np.float64) - w.astype(np.float64)) / ulp
        print("\nQ30 in-kernel rotation %d+%d levels%d: worst error %.3f ulp of max(|want|, 1) at face %d, exact share %.4f" % (
            ns, ne, lv, err.max(), good[int(np.argmax(err.max(axis=(1, 2))))], float((q == w).mean())))
        assert err.max() <= 2.0


# ---- 6. where it writes ---------------------------------------------------------------------------------------------------------------
def _only_inside(buf, lo, n, what):
    """every element of the pattern-filled int32 buffer outside [lo, lo + n) still holds the pattern"""
    a = buf.cpu().numpy()
    assert (a[:lo] == PATTERN).all() and (a[lo + n:] == PATTERN).all(), what + ": written outside its allocation"
    return a[lo:lo + n]


@pytest.mark.parametrize("N", [63, 99, 1000])
@pytest.mark.parametrize("ns,ne", [(199, 29), (33, 16)], ids=["ring", "generic"])
def test_stores_stay_inside_their_allocations(oracle, ns, ne, N):
    """fr_decode_q30_pack, fr_decode_3dmm_q30_lv (dense rows) and fr_decode_render_forward_q30 with phases = 8 (pitched rows), every
    buffer they write carved from the middle of a pattern-filled allocation with 64 KiB on both sides: the Q30 image of exactly
    fr_decode_q30_image_bytes, the staging workspace of exactly fr_decode_q30_workspace_bytes at an address that is a multiple of 16
    but not of 32, the dense output at float alignment, the pitched hand-off -- whose pad floats [N, pitch) keep the pattern too.
    The elements are the spec's.  (Observation only: nothing here reads or writes outside an allocation by design.)"""
    h = _h()
    L = h.lib()
    dev = torch.device("cuda:0")
    g = qrig(ns, ne, N)
    pitch = L.fr_decode_render_vertex_pitch(N)
    assert pitch >= N and pitch % 32 == 0
    # the image: packed in place between its bands
    nimg = L.fr_decode_q30_image_bytes(N, ns, ne)
    assert nimg % 4 == 0
    ibuf, io = _guarded(nimg, 256)
    iptr = ctypes.c_void_p(ibuf.data_ptr() + 4 * io)
    g.pack_into(iptr, nimg)
    packed = _only_inside(ibuf, io, nimg // 4, "%d+%d N=%d: fr_decode_q30_pack" % (ns, ne, N))
    assert np.array_equal(packed.view(np.uint8), g.qimage.cpu().numpy()), "the image does not depend on where it is built"
    nws = L.fr_decode_q30_workspace_bytes(ns, ne)
    assert nws % 16 == 0
    reached = set()
    for lv in (7, 4):
        _, P129, R129, want129 = case(oracle, ns, ne, N, 129, lv)
        for knobs in SCHEDULES[:2]:
            with h.options(**knobs):
                for B in (1, 17, 65, 129):
                    reached |= {(p["kernel"], p["nbw"], p["waves"], p["h2"], p["launches"]) for p in qgeom(B, N, ns, ne, lv)}
                    what = "levels%d %s %d+%d N=%d B=%d" % (lv, _sid(knobs), ns, ne, N, B)
                    p = torch.as_tensor(P129[:B], device=dev)
                    r = torch.as_tensor(R129[:B].reshape(B, 9), device=dev)
                    # dense [B,3,N] at float alignment, the workspace at 16 mod 32
                    wbuf, wo = _guarded(nws + 16, 32)
                    wo += 4
                    wptr = ctypes.c_void_p(wbuf.data_ptr() + 4 * wo)
                    assert wptr.value % 32 == 16
                    buf, o = _guarded(B * 3 * N * 4, 4)
                    out_ptr = ctypes.c_void_p(buf.data_ptr() + 4 * o)
                    h.check(L.fr_decode_3dmm_q30_lv(h.ptr(p), iptr, h.ptr(r), B, N, ns, ne, IM, lv, out_ptr, wptr, nws, h.stream_ptr(dev)),
                            "fr_decode_3dmm_q30_lv")
                    torch.cuda.synchronize()
                    a = _only_inside(buf, o, B * 3 * N, what + ": dense output")
                    _only_inside(wbuf, wo, nws // 4, what + ": staging workspace")
                    assert_bits_equal(a.view(np.float32).reshape(B, 3, N), want129[:B], what + " dense")
                    # pitched hand-off: 128-byte aligned, fr_decode_render_vertex_bytes
                    nbytes = L.fr_decode_render_vertex_bytes(B, N)
                    assert nbytes == B * 3 * pitch * 4
                    wbuf, wo = _guarded(nws + 16, 32)
                    wo += 4
                    wptr = ctypes.c_void_p(wbuf.data_ptr() + 4 * wo)
                    buf, o = _guarded(nbytes, 128)
                    vptr = ctypes.c_void_p(buf.data_ptr() + 4 * o)
                    rc = L.fr_decode_render_forward_q30(h.ptr(p), iptr, h.ptr(r), None, None, B, N, ns, ne, 0, 0, 0, 1, IM, lv, vptr,
                                                        nbytes, None, None, None, None, None, 0, wptr, nws, h.stream_ptr(dev), 8)
                    h.check(rc, "fr_decode_render_forward_q30")
                    torch.cuda.synchronize()
                    rows = _only_inside(buf, o, B * 3 * pitch, what + ": pitched hand-off").reshape(B, 3, pitch)
                    _only_inside(wbuf, wo, nws // 4, what + ": staging workspace (pitched)")
                    assert (rows[:, :, N:] == PATTERN).all(), what + ": a pad float [N, pitch) was written"
                    assert_bits_equal(np.ascontiguousarray(rows[:, :, :N]).view(np.float32), want129[:B], what + " pitched")
    _only_inside(ibuf, io, nimg // 4, "%d+%d N=%d: the image's bands after the decodes" % (ns, ne, N))
    if (ns, ne) == (199, 29):
        assert reached == {(RING, 1, 8, 1, 1), (RING, 2, 8, 1, 1), (RING, 4, 8, 1, 1), (RING, 2, 12, 2, 1), (RING, 2, 16, 2, 1)}, reached
    else:
        assert reached == {(GENERIC, 1, 8, 1, 1), (GENERIC, 2, 8, 1, 1), (GENERIC, 2, 8, 1, 2)}, reached


# ---- 7. large N, once -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv", [7, 4], ids=["levels7", "levels4"])
def test_second_tile_per_wave_on_the_whole_part(oracle, lv):
    """The smallest mesh at which the default launcher, planning for the whole part, gives some waves a second tile (asked of
    fr_debug_decode_q_geom: one tile past waves x workgroups), 64 faces: the ring schedule, the halves schedule and the generic
    kernel give the same bits on all faces, and four faces -- the first, the last and the two on either side of a column-block
    seam -- are the spec's."""
    ns, ne, B = 199, 29, 64
    cus = _cus()
    # the first tile count at which the launcher's answer gives a slot a second tile, at that tile's first vertex
    N = next(16 * t + 1 for t in range(1, 1 << 16) if rounds(qgeom(B, 16 * t + 1, ns, ne, lv)[0], 16 * t + 1)[0] >= 2)
    (p,) = qgeom(B, N, ns, ne, lv)
    (q,) = qgeom(B, N - 1, ns, ne, lv)
    assert p["kernel"] == RING and p["nbw"] == 4 and p["grid"] == cus and rounds(p, N)[:2] == (2, 1) and rounds(q, N - 1)[0] == 1
    assert 30000 < N < 16 * 16 * cus, N
    rs = np.random.RandomState(97)
    mu = rs.uniform(-1.0e5, 1.0e5, 3 * N).astype(np.float32)
    A = np.empty((3 * N, ns + ne), np.float32)
    for c in range(3):
        A[c * N:(c + 1) * N] = rs.standard_normal((N, ns + ne)).astype(np.float32)
    S = np.ascontiguousarray(A[:, :ns]) * np.float32(1e-2)
    E = np.ascontiguousarray(A[:, ns:]) * np.float32(300.0)
    del A
    g = QRig(ns, ne, N, arrays=(mu, S, E))
    P = rand_params(rs, B, ns, ne)
    R = oracle.rotation_matrix_batch(P[:, :3])
    got = g.decode(P, R, lv)
    faces = [0, 15, 16, 63]
    want = spec(oracle, g, P[faces], R[faces], lv)
    assert_bits_equal(got[faces], want, "levels%d ring N=%d faces %r" % (lv, N, faces))
    for knobs in SCHEDULES[1:]:
        with _h().options(**knobs):
            (p2,) = qgeom(B, N, ns, ne, lv)
            assert (p2["kernel"], p2["h2"]) == ((RING, 2) if "FR_Q30_SCHED" in knobs else (GENERIC, 1)) and rounds(p2, N)[0] >= 2
            assert_bits_equal(g.decode(P, R, lv), got, "levels%d %s N=%d against the default schedule" % (lv, _sid(knobs), N))
    g._qimage = None
