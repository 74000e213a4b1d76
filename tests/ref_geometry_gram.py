"""Float64 numpy model of the Gram-form geometry loss (include/fr_hotpath.h, "Gram-form geometry loss"): the four chains of the
loss and its gradient exactly as the header writes them -- numpy fuses nothing, so a loop of vectorised multiply-then-add IS the
chain, rounding for rounding -- the Gram matrix's float64 reference with its bound, and the shapes and inputs the tests share."""
import collections

import numpy as np

PAIRS = ((1, 0), (0, 1), (7, 3), (16, 0), (17, 16), (199, 29), (240, 16))    # (n_shape, n_exp)
BATCHES = (1, 3, 64, 65)
GRAD_LOSSES = (1.0, -0.37, 1e-3)
Case = collections.namedtuple("Case", "N ns ne")


def chunk_edge_sizes(c):
    """the vertex counts the tests use, from the build's rows per chunk c (fr_debug_geometry_gram_geom): 1, 5, the largest N with
    3N <= c, the smallest with 3N > c, the smallest with 3N > 2c"""
    return (1, 5, c // 3, c // 3 + 1, 2 * c // 3 + 1)


def cases(c):
    return [Case(N, ns, ne) for N in chunk_edge_sizes(c) for ns, ne in PAIRS]


def case_id(case):
    return "N%d-%d+%d" % tuple(case)


def basis(N, ns, ne, seed=0):
    """pc_shape [3N,ns], pc_exp [3N,ne] fp32, scaled like utils/synth.py: shape columns of norm ~1, expression columns of rms 300"""
    rs = np.random.RandomState(1000 + seed + 7 * N + 31 * ns + 131 * ne)
    pc_shape = (rs.standard_normal((3 * N, ns)) / np.sqrt(3.0 * N)).astype(np.float32)
    pc_exp = (rs.standard_normal((3 * N, ne)) * 300.0).astype(np.float32)
    return pc_shape, pc_exp


def diffs(B, ns, ne, seed=0):
    """coefficient differences as tests/test_losses_gpu.py draws them: +-1e4 shape, +-3 expression"""
    rs = np.random.RandomState(2000 + seed + B)
    return np.concatenate([rs.uniform(-1e4, 1e4, (B, ns)), rs.uniform(-3, 3, (B, ne))], 1).astype(np.float32)


def U64(pc_shape, pc_exp):
    return np.concatenate([np.asarray(pc_shape, np.float64), np.asarray(pc_exp, np.float64)], 1)


def gram(pc_shape, pc_exp):
    """-> (G [K,K] = U^T U in numpy's float64, bound [K,K] = 3N 2^-53 sum_r |U[r][i] U[r][j]|).  The bound: the 3N products of
    widened fp32 entries are exact, a sum of n exact terms in ANY association carries at most n - 1 roundings on the path to a
    term, each of relative size u = 2^-53, so |error| <= ((1 + u)^(n-1) - 1) sum|terms| <= n u sum|terms| for n u < 0.01.  numpy's
    own float64 product sits at a few thousandths of the bound from the exact value, so it serves as the reference as it is."""
    U = U64(pc_shape, pc_exp)
    A = np.abs(U)
    return U.T @ U, U.shape[0] * 2.0 ** -53 * (A.T @ A)


def forward(diff, G, N):
    """the header's chains: diff [B,K] fp32, G [>=K, >=K] float64 -> (y [B,K], q [B], S, loss fp32)"""
    d = np.asarray(diff, np.float32).astype(np.float64)
    B, K = d.shape
    G = np.asarray(G, np.float64)
    with np.errstate(all="ignore"):
        y = np.zeros((B, K))
        for j in range(K):
            y = y + G[j, :K][None, :] * d[:, j:j + 1]
        q = np.zeros(B)
        for k in range(K):
            q = q + d[:, k] * y[:, k]
        S = np.float64(0.0)
        for b in range(B):
            S = S + q[b]
        loss = np.float32(S / (np.float64(3 * N) * np.float64(B)))
    return y, q, S, loss


def backward(grad_loss, y, N):
    """grad_diff [B,K] fp32 from the forward's y"""
    B = y.shape[0]
    with np.errstate(all="ignore"):
        c = np.float64(np.float32(grad_loss)) * (np.float64(2.0) / (np.float64(3 * N) * np.float64(B)))
        return (c * y).astype(np.float32)


def direct_loss(diff, pc_shape, pc_exp):
    """mean((U d)^2) in float64, the form the product route evaluates"""
    g = U64(pc_shape, pc_exp) @ np.asarray(diff, np.float32).astype(np.float64).T
    return float(np.mean(g * g))
