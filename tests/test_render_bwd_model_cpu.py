"""CPU: pins tests/ref_render_bwd_model.py -- the integer model the GPU tests hold fr_render_depth_backward(_ws) to bit
for bit -- before it is used as a judge: against the exact integer sum within a DERIVED bound, against the oracle's
sequential fp32 sum where every partial sum is exact, and on the hand cases of tests/test_backward_gpu.py.

The bound.  Per vertex with n_v terms, on a face with scale exponent e and shift s:
  * each q = rint(c * 2^(40 - s - e)) is off by at most half a grid unit: n_v * 2^(e - 41 + s) in all;
  * the int64 -> fp32 rounding of the sum is at most half an ulp;
  * a subnormal result is rounded a second time by the final conversion (the header says so): another half ulp.
So |model - exact| <= n_v * 2^(e - 41 + s) + ulp_fp32(exact).  Everything is compared in Python ints (units of 2^-170:
ref_render_bwd_model.bound_ratio)."""
import json
import os

import numpy as np
import pytest

import ref_render_bwd_model as R
from conftest import GOLDEN, kat_inputs

def _scene(rs, B, H, W, nver, ntri, cover=0.8):
    tri = rs.randint(0, nver, (3, ntri)).astype(np.float32)
    ti = np.where(rs.rand(B, H, W, 1) < cover, rs.randint(0, ntri, (B, H, W, 1)), -1).astype(np.float32)
    return tri, ti


def check_bound(g, tri, ti, nver, H, W):
    """asserts the derived bound (ref_render_bwd_model.bound_ratio) on every vertex; returns the worst error / bound"""
    M = R.model(g, tri, ti, nver, H, W)
    X, n = R.exact(g, tri, ti, nver, H, W)
    z = M.bits.view(np.float32)
    assert not M.bad.any() and not M.bits[:, :2].any()
    worst = max(R.bound_ratio(z[b, 2], X[b], n[b], M.e[b], M.shift) for b in range(z.shape[0]))
    return worst, M


PROFILES = {
    "unit": lambda rs, sh: rs.standard_normal(sh),
    "decades12": lambda rs, sh: rs.standard_normal(sh) * np.exp(rs.uniform(-14, 14, sh)),
    "subnormal": lambda rs, sh: rs.standard_normal(sh) * 1e-41,
    "lowest_normal_binade": lambda rs, sh: np.where(rs.rand(*sh) < 0.01, 1.9e-38, rs.standard_normal(sh) * 1e-40),
    "huge": lambda rs, sh: rs.standard_normal(sh) * 1e30,
    "one_2pow45": lambda rs, sh: np.where(rs.rand(*sh) < 1e-4, 2.0 ** 45, 1.0) * rs.standard_normal(sh),
}


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_model_is_within_the_derived_bound_of_the_exact_sum(profile):
    rs = np.random.RandomState(sorted(PROFILES).index(profile))
    B, H, W, nver, ntri = 2, 200, 200, 1500, 4000
    tri, ti = _scene(rs, B, H, W, nver, ntri)
    g = PROFILES[profile](rs, (B, H, W, 1)).astype(np.float32)
    worst, M = check_bound(g, tri, ti, nver, H, W)
    print("%s: worst error / bound %.3f, e %s" % (profile, worst, M.e.tolist()))
    if profile == "subnormal":
        assert worst == 0.0 and np.all(M.e == -127)             # every term is on the grid: the sum is exact
    if profile == "lowest_normal_binade":
        assert np.all(M.e == -126)


def test_bound_holds_above_2_pow_20_pixels():
    rs = np.random.RandomState(7)
    for H, W, shift in ((1024, 1024, 0), (1025, 1024, 1), (1025, 2048, 2)):
        tri, ti = _scene(rs, 1, H, W, 40, 90)
        g = (rs.standard_normal((1, H, W, 1)) * np.exp(rs.uniform(-14, 14, (1, H, W, 1)))).astype(np.float32)
        worst, M = check_bound(g, tri, ti, 40, H, W)
        assert M.shift == shift and 0 < worst <= 1


def test_overflowing_sum_gives_the_infinity_of_the_rounded_exact_sum():
    fmax = np.finfo(np.float32).max
    tri = np.array([[0, 1, 2], [0, 3, 4]], np.float32).T.copy()
    ti = np.array([0, 0, 0, 0, 1, 1, -1, -1], np.float32).reshape(1, 2, 4, 1)
    g = np.array([fmax, fmax, fmax, fmax, -fmax, 1e30, fmax, np.inf], np.float32).reshape(1, 2, 4, 1)
    worst, M = check_bound(g, tri, ti, 5, 2, 4)
    z = M.bits.view(np.float32)[0, 2]
    assert not M.bad[0] and M.e[0] == 127
    assert np.isposinf(z[1]) and np.isposinf(z[2])              # 4 * FLT_MAX / 3
    assert np.isfinite(z[0]) and np.isfinite(z[3])              # vertex 0: ... - FLT_MAX / 3 + 1e30 / 3 comes back
    g[0, 0, :, 0] *= -1
    assert np.isneginf(R.model(g, tri, ti, 5, 2, 4).bits.view(np.float32)[0, 2, 1])


def test_the_headers_error_claim_follows_from_the_bound():
    """include/fr_hotpath.h: 'up to n * 2^-39 * max|term|' (2^-38 at 2^21 pixels, ...).  max|term| = fp32(m / 3) >= 2^(e - 2)
    for a normal m, so n * 2^(-39 + s) * max|term| >= n * 2^(e - 41 + s): the header's figure dominates the model's grid error.
    For a subnormal m the claim has nothing to dominate: every q is exact (checked above: error 0)."""
    rs = np.random.RandomState(3)
    bits = np.concatenate([rs.randint(0x00800000, 0x7F800000, 4000), [0x00800000, 0x7F7FFFFF, 0x3F800000, 0x3FFFFFFF]])
    m = bits.astype(np.uint32).view(np.float32)
    term = (m * np.float32(1.0)) / np.float32(3.0)
    e = (bits >> 23) - 127
    for s in (0, 1, 2):
        assert np.all(np.ldexp(term.astype(np.float64), -39 + s) >= np.ldexp(1.0, e - 41 + s))


def test_model_equals_the_sequential_fp32_sum_where_every_partial_sum_is_exact(oracle):
    """gradients that are small-integer multiples of 3: every term and every partial sum is a small integer, so the
    oracle's row-major fp32 order (oracle.render_depth_grad) loses nothing and must equal the model bit for bit"""
    rs = np.random.RandomState(5)
    for B, H, W, nver, ntri in ((3, 40, 33, 200, 500), (1, 7, 1, 3, 1), (2, 200, 200, 900, 1500)):
        tri, ti = _scene(rs, B, H, W, nver, ntri)
        tri[rs.randint(0, 3), rs.randint(0, ntri)] = float(nver)      # a bad id: skipped by both
        g = (3.0 * rs.randint(-40, 41, (B, H, W, 1))).astype(np.float32)
        M = R.model(g, tri, ti, nver, H, W)
        want = oracle.render_depth_grad(g, tri, ti, nver)
        np.testing.assert_array_equal(M.bits, want.view(np.uint32))
        assert not M.bad.any()


def test_kat_k6_comes_out_of_the_model(oracle):
    KAT = json.load(open(os.path.join(GOLDEN, "kat_survey.json")))
    k, W, H = KAT["K6_grad"], KAT["W"], KAT["H"]
    ver, tri, tex = kat_inputs(k, W, H)
    tind = oracle.render_depth(ver, tri, tex, H, W)[3]
    g = np.where(tind >= 0, np.float32(k["depth_grad_on_covered"]), np.float32(0)).astype(np.float32)
    M = R.model(g, tri, tind, ver.shape[2], H, W)
    np.testing.assert_array_equal(M.bits.view(np.float32)[0, 2], np.array(k["vertex_grad_z"], np.float32))
    assert not M.bits[0, :2].any()


def test_hand_case_background_and_bad_ids():
    """tests/test_backward_gpu.py::test_background_and_bad_ids_are_skipped"""
    H, W = 8, 8
    tri = np.array([[0, 1, 2]], np.float32).T.copy()
    tind = -np.ones((1, H, W, 1), np.float32)
    tind[0, 2, 2, 0] = 0
    tind[0, 3, 3, 0] = 5
    tind[0, 4, 4, 0] = np.nan
    g = np.ones((1, H, W, 1), np.float32)
    M = R.model(g, tri, tind, 4, H, W)
    np.testing.assert_array_equal(M.bits.view(np.float32)[0, 2], np.array([1 / 3, 1 / 3, 1 / 3, 0], np.float32))
    assert M.m[0] == 0x3F800000 and M.e[0] == 0 and not M.bad[0]


def test_hand_case_inf_nan_gradients():
    """tests/test_backward_gpu.py::test_backward_inf_nan_gradients_and_small_batch_owners"""
    H, W = 6, 5
    tri = np.array([[0, 1, 2], [2, 3, 4], [1, 3, 5]], np.float32).T.copy()
    tind = np.array([[0, 0, 1, 1, -1], [2, 2, 2, 0, 1], [1, 1, -1, -1, 2], [0, 2, 1, 0, 0], [-1, -1, -1, -1, -1],
                     [2, 1, 0, 2, 1]], np.float32).reshape(1, H, W, 1)
    g = np.arange(H * W, dtype=np.float32).reshape(1, H, W, 1) - 7
    want = np.zeros(6, np.float64)
    for i in range(H * W):
        t = int(tind.reshape(-1)[i])
        if t >= 0:
            for k in range(3):
                want[int(tri[k, t])] += np.float32(g.reshape(-1)[i] / np.float32(3.0))
    M = R.model(g, tri, tind, 6, H, W)
    np.testing.assert_allclose(M.bits.view(np.float32)[0, 2], want, rtol=1e-6, atol=1e-6)
    g2 = g.copy()
    g2[0, 0, 0, 0] = np.inf       # triangle 0 -> vertices 0, 1, 2
    g2[0, 1, 0, 0] = np.nan       # triangle 2 -> vertices 1, 3, 5
    M2 = R.model(g2, tri, tind, 6, H, W)
    assert M2.bad[0]
    assert M2.cls[0].tolist() == [R.POS_INF, R.NAN, R.POS_INF, R.NAN, R.FINITE, R.NAN]
    assert abs(M2.sum64[0][4] - want[4]) < 1e-5 and M2.nterm[0][4] == 8
    g2[0, 0, 1, 0] = -np.inf      # +Inf and -Inf meet on vertices 0, 1, 2
    assert R.model(g2, tri, tind, 6, H, W).cls[0].tolist() == [R.NAN, R.NAN, R.NAN, R.NAN, R.FINITE, R.NAN]


def test_conversions_and_what_counts():
    nan, inf = np.nan, np.inf
    got = R.f2i_x86(np.array([-0.5, -0.0, 0.75, 2.7, -1.0, -1.5, 2147483520.0, 2147483648.0, -2147483648.0, 3e9, -3e9, nan,
                              inf, -inf], np.float32))
    I = R.INT_MIN
    assert got.tolist() == [0, 0, 0, 2, -1, -1, 2147483520, I, I, I, I, I, I, I]
    # ntri = 3: tri_ind -0.5 selects triangle 0, 2.7 triangle 2; 3.0 and NaN nothing.  Triangle 1 has a vertex id out of
    # range: its pixel adds nothing but its gradient -- the largest -- sets the scale, and its Inf makes the face bad.
    tri = np.array([[0, 1, 2], [1, 9, 2], [2.75, 3.9, 0.75]], np.float32).T.copy()
    ti = np.array([-0.5, 2.7, 1.0, 3.0, nan, -1.0], np.float32).reshape(1, 1, 6, 1)
    g = np.array([3.0, 6.0, 96.0, 1e9, inf, nan], np.float32).reshape(1, 1, 6, 1)
    M = R.model(g, tri, ti, 4, 1, 6)
    assert not M.bad[0] and M.m[0] == np.float32(96.0).view(np.uint32) and M.e[0] == 6
    np.testing.assert_array_equal(M.bits.view(np.float32)[0, 2], np.array([3, 1, 3, 2], np.float32))
    g[0, 0, 2, 0] = inf
    M = R.model(g, tri, ti, 4, 1, 6)
    assert M.bad[0] and M.m[0] == np.float32(6.0).view(np.uint32)
    assert M.cls[0].tolist() == [R.FINITE] * 4 and M.sum64[0].tolist() == [3, 1, 3, 2] and M.nterm[0].tolist() == [2, 1, 2, 1]
    # all-zero faces and empty faces: m = 0, everything +0
    M = R.model(np.array([0.0, -0.0, 0.0, -0.0, 0.0, 5.0], np.float32), tri, ti, 4, 1, 6)
    assert M.m[0] == 0 and M.e[0] == -127 and not M.bits.any()
    assert R.shift_of(1 << 20) == 0 and R.shift_of((1 << 20) + 1) == 1 and R.shift_of((1 << 21) + 1) == 2 and R.shift_of(1) == 0
