"""CPU: the float64 decode-backward oracle with an explicit rotation and the sums of |terms|
(oracle.decode_3dmm_backward_f64(..., R=, abs_sum=)), which tests/test_decode_backward_bounds_gpu.py holds the HIP kernels to."""
import numpy as np


def _case(synth, gu, gv, ns, ne, B, seed):
    A = synth.make_assets(gu, gv, ns, ne, patch=None, seed_basis=seed)
    rs = np.random.RandomState(seed)
    P = np.zeros((B, 7 + ns + ne), np.float32)
    P[:, 0:3] = rs.uniform(-1.0, 1.0, (B, 3))
    P[:, 3:5] = rs.uniform(60, 140, (B, 2))
    P[:, 5] = rs.uniform(-1, 1, B)
    P[:, 6] = rs.uniform(2e-4, 1e-3, B)
    P[:, 7:7 + ns] = rs.uniform(0, 1e4, (B, ns))
    P[:, 7 + ns:] = rs.uniform(-1.5, 1.5, (B, ne))
    G = (rs.standard_normal((B, 3, gu * gv)) * np.exp(rs.uniform(-6, 6, (B, 3, gu * gv)))).astype(np.float32)
    return A, P, G


def test_explicit_rotation_and_abs_sums_leave_the_gradient_bits_alone(oracle, synth):
    for gu, gv, ns, ne, B in ((5, 7, 9, 4, 3), (4, 4, 0, 29, 2), (3, 6, 17, 0, 2)):
        A, P, G = _case(synth, gu, gv, ns, ne, B, gu * gv + ns)
        args = (G, P, A["mu"], A["pc_shape"], A["pc_exp"])
        old = oracle.decode_3dmm_backward_f64(*args)
        new, S = oracle.decode_3dmm_backward_f64(*args, abs_sum=True)
        np.testing.assert_array_equal(new, old)
        R = oracle.rotation_matrix_batch(P[:, 0:3])
        withR, SR = oracle.decode_3dmm_backward_f64(*args, R=R, abs_sum=True)
        np.testing.assert_array_equal(withR, old)                          # the angles' own rotation: the same bits
        np.testing.assert_array_equal(SR, S)
        np.testing.assert_array_equal(oracle.decode_3dmm_backward_f64(*args, R=R), old)
        assert np.all(S[:, 0:3] == 0) and np.all(new[:, 0:3] == 0)
        assert np.all(S >= np.abs(new))
        # d t3d: the sum of |dq|, exactly representable term by term
        dq = G.astype(np.float64) * np.array([1.0, -1.0, 1.0])[None, :, None]
        np.testing.assert_allclose(S[:, 3:6], np.abs(dq).sum(2), rtol=1e-14)


def test_a_rotation_that_is_not_the_angles_changes_the_gradient(oracle, synth):
    A, P, G = _case(synth, 5, 7, 9, 4, 3, 11)
    args = (G, P, A["mu"], A["pc_shape"], A["pc_exp"])
    R = oracle.rotation_matrix_batch(P[:, 0:3])
    Rt = np.ascontiguousarray(R.transpose(0, 2, 1))
    a = oracle.decode_3dmm_backward_f64(*args, R=R)
    b = oracle.decode_3dmm_backward_f64(*args, R=Rt)
    np.testing.assert_array_equal(a[:, 3:6], b[:, 3:6])                  # d t3d does not see R
    assert np.all(a[:, 6] != b[:, 6]) and np.all(a[:, 7:] != b[:, 7:])


def test_hand_sized_case_exact_values(oracle):
    """N = 2, one shape component, no expression, a non-symmetric rotation: every value is a small dyadic rational, so the
    float64 evaluation is exact and the expected numbers are written out by hand.
      R = [[0,1,0],[-1,0,0],[0,0,1]], f = 0.5, t = (1, 2, 3), alpha = 2
      mu   : vertex 0 = (1, 2, 3), vertex 1 = (-1, 0, 2)      pc_shape : vertex 0 = (1, 0, -1), vertex 1 = (2, 1, 0)
      v = mu + 2 pc : vertex 0 = (3, 2, 1), vertex 1 = (3, 2, 2);  R v : vertex 0 = (2, -3, 1), vertex 1 = (2, -3, 2)
      g    : vertex 0 = (1, 2, -1), vertex 1 = (3, -1, 2)  ->  dq = (g_x, -g_y, g_z): vertex 0 = (1, -2, -1), vertex 1 = (3, 1, 2)
      d t3d = (4, -1, 1);  |.|: (4, 3, 3)
      d f = (2 + 6 - 1) + (6 - 3 + 4) = 14;  sum |(R v)_i dq_i| = (2 + 6 + 1) + (6 + 3 + 4) = 22
      dv = f R^T dq: vertex 0 = 0.5 (2, 1, -1), vertex 1 = 0.5 (-1, 3, 2)
      d alpha = pc . dv = 0.5 ((2 + 0 + 1) + (-2 + 3 + 0)) = 2;  |pc|.|dv| = 0.5 ((2 + 1) + (2 + 3)) = 4"""
    N = 2
    mu = np.array([1, -1, 2, 0, 3, 2], np.float32)          # blocked: x row, y row, z row
    pcs = np.array([[1], [2], [0], [1], [-1], [0]], np.float32)
    pce = np.zeros((6, 0), np.float32)
    P = np.array([[0.3, -0.2, 0.1, 1, 2, 3, 0.5, 2]], np.float32)
    G = np.array([[[1, 3], [2, -1], [-1, 2]]], np.float32)
    R = np.array([[[0, 1, 0], [-1, 0, 0], [0, 0, 1]]], np.float32)
    got, S = oracle.decode_3dmm_backward_f64(G, P, mu, pcs, pce, R=R, abs_sum=True)
    assert got.shape == (1, 8) and N == 2
    np.testing.assert_array_equal(got[0], [0, 0, 0, 4, -1, 1, 14, 2])
    np.testing.assert_array_equal(S[0], [0, 0, 0, 4, 3, 3, 22, 4])
