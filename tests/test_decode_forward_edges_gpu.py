"""GPU: the default f32 decode forward (fr_decode_3dmm, csrc/fr_decode.hip) held to its written definition (oracle/fr_oracle.c:
k-ordered fmaf chains from +0) at every schedule the launcher can pick and at the edges of its domain.

Everything is compared with oracle.decode_3dmm by BIT PATTERN (gpu_util.assert_bits_equal: -0.0 is not +0.0; a NaN equals any
NaN).  The rotation is supplied by the host unless a test is about the in-kernel one.  Shapes are chosen by asking the launcher's
own decision function (fr_debug_decode_geom, with the CU count the launcher plans for: the device's, or FR_DECODE_CUS where a cell
caps it so that a small mesh walks several rounds of tiles) which (N, B) reach a geometry, never by re-deriving its rules.
Outputs are pre-filled with a finite sentinel, so an element the kernel does not write is a mismatch too."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import assert_bits_equal, net_mod

pytestmark = pytest.mark.gpu

IM = 200.0
SENTINEL = 12345.678
FIELDS = ("b0", "cols", "kernel", "nbw", "waves", "mb", "halves", "nt", "prio", "tr", "lds", "grid")
SCHEDULES = [{}, {"FR_DECODE_NT": 0}, {"FR_DECODE_NT": 1}, {"FR_DECODE_NBW": 1}, {"FR_DECODE_NBW": 4}, {"FR_DECODE_WAVES": 8},
             {"FR_DECODE_IMPL": 1}, {"FR_DECODE_WIDE": 0}, {"FR_DECODE_STORE": 1}]
FAMILIES = [(199, 29), (200, 17), (33, 16)]      # the ring shape, the same 13 + 2 groups with other paddings, a generic shape
NMAX = 4224


def _sid(k):
    return "-".join("%s%d" % (n[len("FR_DECODE_"):], v) for n, v in k.items()) or "default"


def _h():
    return pkg("_lib")


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def geom(B, N, ns, ne, cus=None):
    out = (ctypes.c_int * (1 + 12 * ((B + 63) // 64 + 1)))()
    rc = _h().lib().fr_debug_decode_geom(B, N, ns, ne, cus or _cus(), out)
    assert rc == 0, rc
    return [dict(zip(FIELDS, out[1 + 12 * i:13 + 12 * i])) for i in range(out[0])]


# ---- assets: one random basis per (ns, ne), cut to the N a case needs; packed once per (ns, ne, N, variant) ------------------------
_BASIS, _RIGS, _WANT = {}, {}, {}


def _basis(ns, ne):
    if (ns, ne) not in _BASIS:
        rs = np.random.RandomState(1000 * ns + ne)
        mu = (rs.uniform(-1.0e5, 1.0e5, (3, NMAX))).astype(np.float32)
        S = (rs.standard_normal((3, NMAX, ns)) * 1e-2).astype(np.float32)    # unit-norm-column scale of a mesh of ~10^4 vertices
        E = (rs.standard_normal((3, NMAX, ne)) * 300.0).astype(np.float32)   # the expression basis' scale (utils/synth.py)
        _BASIS[(ns, ne)] = (mu, S, E)
    return _BASIS[(ns, ne)]


class Rig:
    def __init__(self, ns, ne, N, signed_zero=False):
        mu, S, E = _basis(ns, ne)
        self.ns, self.ne, self.N = ns, ne, N
        mu, S, E = mu[:, :N].copy(), S[:, :N].copy(), E[:, :N].copy()
        if signed_zero:
            # every third vertex sits at -0.0 in all three coordinates, its expression rows are below 0.5 (times the smallest
            # subnormal they underflow) and the LAST column of both its bases is negative: a face whose every coefficient is the
            # smallest subnormal blends it to S = E = -0.0, v = -0.0 (test_special_values, face 12).  Every seventh sits at +0.0.
            mu[:, 1::7] = 0.0
            mu[:, 0::3] = -0.0
            E[:, 0::3] *= np.float32(1e-4)
            if ns:
                S[:, 0::3, ns - 1] = -np.abs(S[:, 0::3, ns - 1]) - np.float32(1e-3)
            if ne:
                E[:, 0::3, ne - 1] = -np.abs(E[:, 0::3, ne - 1]) - np.float32(1e-3)
        self.mu = mu.reshape(3 * N)
        self.pc_shape = S.reshape(3 * N, ns)
        self.pc_exp = E.reshape(3 * N, ne)
        self._packed = None

    @property
    def packed(self):
        if self._packed is None:
            dev = torch.device("cuda:0")
            self.t = [torch.as_tensor(a, device=dev) for a in (self.mu, self.pc_shape, self.pc_exp)]
            self._packed = net_mod().PackedBasis(self.t[0], self.t[1], self.t[2], self.N, self.ns, self.ne, dev)
        return self._packed

    def decode(self, P, R=None, im=IM):
        h = _h()
        dev = torch.device("cuda:0")
        B = P.shape[0]
        p = torch.as_tensor(np.ascontiguousarray(P, np.float32), device=dev)
        r = None if R is None else torch.as_tensor(np.ascontiguousarray(R, np.float32).reshape(B, 9), device=dev)
        out = torch.full((B, 3, self.N), SENTINEL, dtype=torch.float32, device=dev)
        rc = h.lib().fr_decode_3dmm(h.ptr(p), h.ptr(self.packed.image), h.ptr(r), B, self.N, self.ns, self.ne, float(im), h.ptr(out),
                                    h.stream_ptr(dev))
        h.check(rc, "fr_decode_3dmm")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def oracle(self, O, P, R=None, im=IM):
        return O.decode_3dmm(P, self.mu, self.pc_shape, self.pc_exp, im, R=R)


def rig(ns, ne, N, signed_zero=False):
    k = (ns, ne, N, signed_zero)
    if k not in _RIGS:
        _RIGS[k] = Rig(ns, ne, N, signed_zero)
    return _RIGS[k]


def rand_params(rs, B, ns, ne, im=IM):
    P = np.zeros((B, 7 + ns + ne), np.float32)
    P[:, 0:3] = rs.uniform(-1.5, 1.5, (B, 3))
    P[:, 3:5] = rs.uniform(0, im, (B, 2))
    P[:, 5] = rs.uniform(-1, 1, B)
    P[:, 6] = rs.uniform(0, 1e-3, B)
    P[:, 7:7 + ns] = rs.uniform(0, 1e4, (B, ns))
    P[:, 7 + ns:] = rs.uniform(-1.5, 1.5, (B, ne))
    return P


def case(O, ns, ne, N, B):
    """(rig, P, R, oracle result) of a random batch, computed once per shape and shared by every schedule"""
    k = (ns, ne, N, B)
    if k not in _WANT:
        g = rig(ns, ne, N)
        P = rand_params(np.random.RandomState(7 * N + B), B, ns, ne)
        R = O.rotation_matrix_batch(P[:, :3])
        want = g.oracle(O, P, R)
        want.setflags(write=False)
        _WANT[k] = (g, P, R, want)
    return _WANT[k]


# ---- schedule x geometry matrix -----------------------------------------------------------------------------------------------
GRIDS = (1, 2, 7, 8, 9, 16)
B_EDGES = (16, 17, 32, 33, 64, 65, 128, 129, 192, 193)
N_EDGES = (99, 63, 65, 100, 96, 13, 31, 17, 48, 33)      # N mod 16 = 3, 15, 1, 4, 0, 13 (< 16), 15, 1, 0, 1; 1 .. 7 tiles


def _n_for_grid(B, ns, ne, cus, want_grid, which, pick):
    """an N at which pass `which` of a B-face decode runs on `want_grid` workgroups under the current knobs -- the pick-th of the
    contiguous range the launcher answers that grid for (clipped to its end: pick = 15 reaches N mod 16 = 0)"""
    lo = None
    for N in range(1, NMAX + 1):
        g = geom(B, N, ns, ne, cus)[which]["grid"]
        if g == want_grid and lo is None:
            lo = N
        if g > want_grid:
            break
        hi = N
    assert lo is not None, (B, ns, ne, want_grid)
    return min(lo + pick, hi)


CAPS = (1, 2, 3, 8)      # FR_DECODE_CUS: the launcher plans for so many compute units (8: tile_walk's `(grid & 7) == 0` permutation)


def walk_rounds(p, N):
    """(rounds of tiles a wave slot of pass p walks, tiles in the last round, tiles a full round holds)"""
    tiles = (N + 15) // 16
    per = (p["waves"] // p["halves"]) * p["grid"]
    return -(-tiles // per), tiles - (-(-tiles // per) - 1) * per, per


def _n_for_rounds(B, ns, ne, cap_cus):
    """the smallest N from 700, no multiple of 16, at which the first pass of a B-face decode planned for cap_cus compute units runs
    on that many workgroups whose wave slots walk at least three rounds of tiles, the last one ragged, under the current knobs"""
    for N in range(700, NMAX + 1):
        p = geom(B, N, ns, ne, cap_cus)[0]
        r = walk_rounds(p, N)
        if N % 16 and p["grid"] == cap_cus and r[0] >= 3 and r[1] < r[2]:
            return N
    raise AssertionError((B, ns, ne, cap_cus))


def matrix_points(ns, ne, cus):
    """[(N, B, cap)] of one (schedule, family) cell, under the current knobs: every batch boundary of the launcher at small meshes of
    every raggedness, then every grid size of GRIDS at 64 faces (the pass every 64-column variant serves), and a few grids at 20
    faces (one item per tile) and at 129 (a 128-column pass and a pass of one face) -- all of them one round of tiles, cap = 0: the
    launcher plans for the device -- and then, at 64 faces, the multi-round cells: FR_DECODE_CUS = cap of CAPS at an N that makes
    every wave slot walk three rounds or more (the ring wrapping from one item's last fragments into the next item's first)"""
    pts = [(N, B, 0) for N, B in zip(N_EDGES, B_EDGES)]
    for i, g in enumerate(GRIDS):
        pts.append((_n_for_grid(64, ns, ne, cus, g, 0, (0, 2, 3, 14, 15, 7)[i]), 64, 0))
    pts.append((_n_for_grid(20, ns, ne, cus, 7, 0, 5), 20, 0))
    pts.append((_n_for_grid(20, ns, ne, cus, 16, 0, 15), 20, 0))
    pts.append((_n_for_grid(129, ns, ne, cus, 2, 0, 3), 129, 0))
    pts.append((_n_for_grid(129, ns, ne, cus, 9, 0, 0), 129, 0))
    for cap in CAPS:
        pts.append((_n_for_rounds(64, ns, ne, min(cap, cus)), 64, cap))
    return pts


@pytest.mark.parametrize("ns,ne", FAMILIES, ids=["%d+%d" % f for f in FAMILIES])
@pytest.mark.parametrize("knobs", SCHEDULES, ids=_sid)
def test_schedule_geometry_matrix(oracle, knobs, ns, ne):
    cus = _cus()
    assert cus >= 16, "the grid cases are written for a part of at least 16 compute units"
    with _h().options(**knobs):
        pts = matrix_points(ns, ne, cus)
        geoms = [geom(B, N, ns, ne, min(cap, cus) if cap else cus) for N, B, cap in pts]
        # the cell reaches what it was written for
        grids = {p["grid"] for g in geoms for p in g}
        assert grids >= set(GRIDS), (sorted(grids), pts)
        assert {N % 16 for N, _, _ in pts} >= {0, 1, 3, 4, 15} and any(N < 16 for N, _, _ in pts)
        assert {((N + 15) // 16) & 1 for N, _, _ in pts} == {0, 1}
        assert {B for _, B, _ in pts} >= set(B_EDGES)
        assert {cap for _, _, cap in pts} == {0} | set(CAPS)
        for (N, B, cap), g in zip(pts, geoms):
            r = walk_rounds(g[0], N)
            if cap:     # more tiles than one round of the capped grid holds: three rounds or more, the last one ragged
                slots = g[0]["waves"] // g[0]["halves"]
                assert -(-((N + 15) // 16) // slots) > g[0]["grid"] == min(cap, cus) and r[0] >= 3 and r[1] < r[2], (N, B, cap, g)
            else:
                assert r[0] == 1, (N, B, g)
        # the block of this cell in profiles/decode_forward_schedule_matrix.txt: per variant its grids, the rounds walked under a cap
        agg = {}
        for (N, B, cap), g in zip(pts, geoms):
            for i, p in enumerate(g):
                a = agg.setdefault("%s nbw%d w%d mb%d h%d nt%d prio%d tr%d" % (
                    ("generic", "ring")[p["kernel"]], p["nbw"], p["waves"], p["mb"], p["halves"], p["nt"], p["prio"], p["tr"]), (set(), set()))
                a[0].add(p["grid"])
                if cap and i == 0:
                    a[1].add(walk_rounds(p, N)[0])
        print("\n%s %d+%d\n" % (_sid(knobs), ns, ne) + "\n".join(
            "    %s grids %s%s" % (k, sorted(a[0]), " rounds %s" % sorted(a[1]) if a[1] else "") for k, a in agg.items()))
        for N, B, cap in pts:
            g, P, R, want = case(oracle, ns, ne, N, B)
            with _h().options(FR_DECODE_CUS=cap):
                got = g.decode(P, R)
            assert_bits_equal(got, want, "%s %d+%d N=%d B=%d cus=%d" % (_sid(knobs), ns, ne, N, B, cap))


# ---- basis shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,ne", [(0, 0), (256, 0), (0, 29), (64, 0), (16, 16), (17, 1), (1, 17), (300, 100)])
def test_basis_shapes_generic_kernel(oracle, ns, ne):
    """no basis at all (v = mu: the packed image then holds only mu), one empty basis, exactly full k-groups, one coefficient past a
    full group, one coefficient, more groups than the model's"""
    N = 99
    for B in (4, 20, 70):
        assert all(p["kernel"] == 0 for p in geom(B, N, ns, ne)), "the generic kernel serves this shape"
        g, P, R, want = case(oracle, ns, ne, N, B)
        assert_bits_equal(g.decode(P, R), want, "%d+%d B=%d" % (ns, ne, B))
        for knobs in ({"FR_DECODE_NBW": 1}, {"FR_DECODE_NBW": 4}):
            with _h().options(**knobs):
                assert_bits_equal(g.decode(P, R), want, "%d+%d B=%d %s" % (ns, ne, B, _sid(knobs)))


# ---- special values -------------------------------------------------------------------------------------------------------------
CLEAN_FACES = (0, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 21, 22, 23)
N_SPECIAL_FACES = 24


def special_params(O, ns, ne):
    """70 faces: 24 special ones, then random neighbours.  Faces 3, 10, 12 and 21 have the exact identity for R, |f| = 1 and
    t = -0.0, so that the sign of a zero blend reaches the x and z rows."""
    rs = np.random.RandomState(3)
    P = rand_params(rs, 70, ns, ne)
    c = 7
    P[1, c + 5 % ns] = np.inf                         # poison: this face NaN, no other
    P[2, c + ns + 1 % ne] = np.nan
    P[3, c:] = 0.0                                    # all-zero coefficients
    P[4, c:] = 0.0
    P[4, c + 3] = 1e-41                               # one subnormal parameter
    P[5, c + 17 % ns] = 3e38                          # near the top of the range (the products stay finite)
    P[6, c:] *= np.float32(1e-30)                     # a face scaled by 1e-30
    P[7, c:c + ns:2] = 0.0                            # alternating zeros
    P[8, c + ns - 1] = -1e7                           # the last live k of the shape chain (beside the padding)
    P[9, c + ns] = 3e38                               # a chain that overflows to Inf (expression basis entries ~ 300)
    P[10, c:] = -0.0                                  # all -0.0 coefficients
    P[11, c:c + ns] = rs.uniform(0, 1, ns) * 1e-37    # products (basis ~ 1e-2) and running sums subnormal
    P[11, c + ns:] = rs.uniform(0, 1, ne) * 1e-42
    P[12, c:] = 1e-45                                 # every product underflows to a zero of its own sign
    P[21, c:] = 0.0                                   # f = -1 over a +0.0 blend: -0.0 from the epilogue alone
    for b in (3, 10, 12, 21):
        P[b, 0:6] = (0.0, 0.0, 0.0, -0.0, -0.0, -0.0)
        P[b, 6] = -1.0 if b == 21 else 1.0
    P[13, 6] = 0.0                                    # pose scalars
    P[14, 6] = -0.0
    P[15, 6] = -1e-3
    P[16, 6] = 1e-41
    P[17, 6] = np.inf
    P[18, 3] = np.inf                                 # non-finite t components
    P[19, 4] = np.nan
    P[20, 5] = -np.inf
    R = O.rotation_matrix_batch(P[:, :3])
    R[[3, 10, 12, 21]] = np.eye(3, dtype=np.float32)
    return P, R


_SPECIAL = {}


def special_case(O, ns, ne, N):
    k = (ns, ne, N)
    if k not in _SPECIAL:
        g = rig(ns, ne, N, signed_zero=True)
        P, R = special_params(O, ns, ne)
        want = g.oracle(O, P, R)
        want.setflags(write=False)
        _SPECIAL[k] = (g, P, R, want)
    return _SPECIAL[k]


@pytest.mark.parametrize("ns,ne,N", [(199, 29, 150), (33, 16, 99), (32, 16, 99)], ids=["ring", "generic", "generic-no-padding"])
@pytest.mark.parametrize("knobs", SCHEDULES, ids=_sid)
def test_special_values(oracle, knobs, ns, ne, N):
    """Inf / NaN parameters poison their own face and no other; subnormal parameters, products and sums; 3e38 and an overflowing
    chain; zero, -0.0 and alternating-zero coefficient rows over mu entries of -0.0; f in {0, -0.0, -1e-3, 1e-41, Inf}; a non-finite
    t component -- bit for bit the oracle's, NaN for NaN, in every schedule, at 70 faces (a 128-column pass, or 64 + 6), 64, 33 and
    24 (the neighbours of a poisoned face share its column block, its work item or only its pass)."""
    g, P, R, want = special_case(oracle, ns, ne, N)
    # the oracle's own picture: the cases are alive
    assert not np.isfinite(want[1]).any() and np.isnan(want[2]).all() and np.isfinite(want[list(CLEAN_FACES)]).all()
    assert np.isfinite(want[N_SPECIAL_FACES:]).all() and not np.isfinite(want[9]).all()
    # face 12: the -0.0 blend of the prepared vertices reaches x and z as -0.0; the all-zero and all-(-0.0) rows blend to +0.0
    # over a mu of either sign (a chain from +0 turns -0 only by underflow); face 21: f = -1 turns that +0.0 into -0.0
    u = want.view(np.uint32)
    assert (u[12][[0, 2]][:, 0::3] == 0x80000000).all() and (u[21][[0, 2]][:, 1::7] == 0x80000000).all()
    assert (u[3][[0, 2]][:, 0::3] == 0).all() and (u[10][[0, 2]][:, 0::3] == 0).all()
    for b in (18, 19, 20):
        assert np.isfinite(want[b]).any() and not np.isfinite(want[b]).all()
    sub = np.abs(g.pc_shape.astype(np.float64) * 1e-37)
    assert 0 < sub.max() < 2.0 ** -126, "face 11's products are subnormal"
    with _h().options(**knobs):
        for B in (70, 64, 33, 24):
            got = g.decode(P[:B], R[:B])
            assert np.array_equal(np.isnan(got), np.isnan(want[:B])), "%s B=%d: NaN mask" % (_sid(knobs), B)
            assert_bits_equal(got, want[:B], "%s %d+%d B=%d" % (_sid(knobs), ns, ne, B))


# ---- in-kernel rotation ---------------------------------------------------------------------------------------------------------
ANGLES = (0.0, -0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 1e-41, 1e4, -1e4, 1e6, -1e6)
BAD_ANGLES = (np.nan, np.inf, -np.inf)


@pytest.mark.parametrize("ns,ne,N", [(199, 29, 40), (9, 5, 40)], ids=["ring", "generic"])
def test_in_kernel_rotation_edges(oracle, ns, ne, N):
    """The float64 rotation evaluated in the kernel at the angles a uniform draw from +-1.5 never produces: exact zeros of both
    signs, multiples of pi / 2 (cosines of 6e-17), a subnormal, arguments that need a full range reduction.  Rule of the existing
    test: within 2 fp32 ulp of max(|want|, 1) of the oracle with glibc's sin / cos.  A non-finite angle makes the oracle's
    elements NaN (all of the face for gamma and theta; phi leaves the x row, whose R entries do not contain it) and nothing else."""
    g = rig(ns, ne, N)
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
    want = g.oracle(oracle, P)
    got = g.decode(P)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for i in range(len(BAD_ANGLES)):
        f = bad0 + 4 * i
        assert np.isnan(got[[f, f + 2, f + 3]]).all()                  # all three, gamma alone, theta alone
        assert np.isnan(got[f + 1, 1:]).all() and not np.isnan(got[f + 1, 0]).any()   # phi alone: the x row does not see it
    good = [b for b in range(B) if not bad0 <= b < bad0 + 4 * len(BAD_ANGLES)]
    assert not np.isnan(got[good]).any()
    w, q = want[good], got[good]
    ulp = np.spacing(np.maximum(np.abs(w), np.float32(1.0)))
    err = np.abs(q.astype(np.float64) - w.astype(np.float64)) / ulp
    print("\nin-kernel rotation %d+%d: worst error %.3f ulp of max(|want|, 1) at face %d, exact share %.4f" % (
        ns, ne, err.max(), good[int(np.argmax(err.max(axis=(1, 2))))], float((q == w).mean())))
    assert err.max() <= 2.0


# ---- where the kernel writes ----------------------------------------------------------------------------------------------------
BAND = 64 * 1024
PATTERN = 0x5A5AA5A5      # (as a float: 1.5e16 -- finite, and nothing a decode produces)
WRITE_SCHEDULES = [{}, {"FR_DECODE_STORE": 1}, {"FR_DECODE_NBW": 4},
                   # FR_DECODE_STORE acts on 64-column passes of the ring shape only: these two bring the ragged batches to it
                   {"FR_DECODE_STORE": 1, "FR_DECODE_NT": 1}, {"FR_DECODE_STORE": 1, "FR_DECODE_WIDE": 0}]


def _guarded(nbytes, align):
    """(whole int32 buffer filled with PATTERN, element offset of an `align`-aligned region of nbytes between two 64 KiB bands)"""
    buf = torch.full(((2 * BAND + nbytes + 2 * align) // 4 + 1,), PATTERN, dtype=torch.int32, device="cuda:0")
    base = buf.data_ptr()
    off = (-(base + BAND)) % align + BAND
    assert (base + off) % align == 0 and off >= BAND and off + nbytes + BAND <= buf.numel() * 4
    return buf, off // 4


@pytest.mark.parametrize("N", [63, 99, 1000])
@pytest.mark.parametrize("ns,ne", [(199, 29), (33, 16)], ids=["ring", "generic"])
def test_stores_stay_inside_the_output(oracle, ns, ne, N):
    """fr_decode_3dmm (dense rows) and fr_decode_render_forward with phases = 8 (pitched rows) through ctypes, the output carved
    from the middle of one pattern-filled allocation: 64 KiB on both sides and, in the pitched hand-off, the pad floats [N, pitch)
    of every row keep the pattern; the elements are the oracle's."""
    h = _h()
    L = h.lib()
    dev = torch.device("cuda:0")
    g, P129, R129, want129 = case(oracle, ns, ne, N, 129)
    pitch = L.fr_decode_render_vertex_pitch(N)
    assert pitch >= N and pitch % 32 == 0
    reached = set()
    for knobs in WRITE_SCHEDULES:
        with h.options(**knobs):
            for B in (1, 17, 65, 129):
                reached |= {(p["kernel"], p["nbw"], p["tr"]) for p in geom(B, N, ns, ne)}
                what = "%s %d+%d N=%d B=%d" % (_sid(knobs), ns, ne, N, B)
                p = torch.as_tensor(P129[:B], device=dev)
                r = torch.as_tensor(R129[:B].reshape(B, 9), device=dev)
                # dense [B,3,N]: no alignment beyond a float's is required -- take the row phase the mesh gives (N odd: 4 mod 8)
                buf, o = _guarded(B * 3 * N * 4, 4)
                out_ptr = ctypes.c_void_p(buf.data_ptr() + 4 * o)
                h.check(L.fr_decode_3dmm(h.ptr(p), h.ptr(g.packed.image), h.ptr(r), B, N, ns, ne, IM, out_ptr, h.stream_ptr(dev)),
                        "fr_decode_3dmm")
                torch.cuda.synchronize()
                a = buf.cpu().numpy()
                assert (a[:o] == PATTERN).all() and (a[o + B * 3 * N:] == PATTERN).all(), what + ": dense, a guard band was written"
                assert_bits_equal(a[o:o + B * 3 * N].view(np.float32).reshape(B, 3, N), want129[:B], what + " dense")
                # pitched hand-off: 128-byte aligned, fr_decode_render_vertex_bytes
                nbytes = L.fr_decode_render_vertex_bytes(B, N)
                assert nbytes == B * 3 * pitch * 4
                buf, o = _guarded(nbytes, 128)
                vptr = ctypes.c_void_p(buf.data_ptr() + 4 * o)
                rc = L.fr_decode_render_forward(h.ptr(p), h.ptr(g.packed.image), h.ptr(r), None, None, B, N, ns, ne, 0, 0, 0, 1, IM, vptr,
                                                nbytes, None, None, None, None, None, 0, h.stream_ptr(dev), 8)
                h.check(rc, "fr_decode_render_forward")
                torch.cuda.synchronize()
                a = buf.cpu().numpy()
                assert (a[:o] == PATTERN).all() and (a[o + B * 3 * pitch:] == PATTERN).all(), what + ": pitched, a guard band was written"
                rows = a[o:o + B * 3 * pitch].reshape(B, 3, pitch)
                assert (rows[:, :, N:] == PATTERN).all(), what + ": a pad float [N, pitch) was written"
                assert_bits_equal(np.ascontiguousarray(rows[:, :, :N]).view(np.float32), want129[:B], what + " pitched")
    if (ns, ne) == (199, 29):
        assert (1, 2, 1) in reached and (1, 4, 0) in reached and (1, 1, 0) in reached   # transposed stores, wide pass, 16-column items
    else:
        assert (0, 4, 0) in reached and (0, 2, 0) in reached and (0, 1, 0) in reached   # decode_kernel<4, 12>, <2, 16>, <1, 16>


# ---- geometry_product ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gu,gv,ns,ne", [(9, 11, 199, 29), (7, 9, 20, 3)], ids=["ring", "generic"])
def test_geometry_product_is_the_decode_of_its_docstring(oracle, synth, gu, gv, ns, ne):
    """geometry_product == the decode with mu = 0, R = I, f = 1, t = 0, im_size = 1, bit for bit"""
    A = synth.make_assets(gu, gv, ns, ne, patch=None, seed_basis=gu + gv)
    net = net_mod().FaceRecNet(mesh_data=A, batch_size=70, im_size=200)
    for B in (5, 70):
        rs = np.random.RandomState(B)
        G = np.concatenate([rs.uniform(0, 1e4, (B, ns)), rs.uniform(-1.5, 1.5, (B, ne))], 1).astype(np.float32)
        P = np.zeros((B, 7 + ns + ne), np.float32)
        P[:, 6] = 1.0
        P[:, 7:] = G
        I = np.tile(np.eye(3, dtype=np.float32)[None], (B, 1, 1))
        want = oracle.decode_3dmm(P, np.zeros_like(A["mu"]), A["pc_shape"], A["pc_exp"], 1.0, R=I)
        got = net.geometry_product(torch.as_tensor(G, device="cuda:0"))
        torch.cuda.synchronize()
        assert_bits_equal(got.detach().cpu().numpy(), want, "geometry_product %d+%d B=%d" % (ns, ne, B))
