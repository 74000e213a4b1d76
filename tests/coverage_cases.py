"""Hand-made scenes of the soft coverage, shared by tests/test_coverage_cpu.py (the model, by hand) and tests/test_coverage_gpu.py
(the kernels against the model).  Each returns (V [1,3,nver] fp32, tri [3,ntri] fp32, tind [1,H*W] fp32, H, W)."""
import numpy as np


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def right_triangle(x0, y0, L):
    """P1 = (x0, y0), P2 = (x0 + L, y0), P3 = (x0, y0 + L): e1 = L (y - y0), e2 = L (x0 + y0 + L - x - y), e3 = L (x - x0), area > 0"""
    return _f([[[x0, x0 + L, x0], [y0, y0, y0 + L], [5, 5, 5]]]), _f([[0], [1], [2]])


def lone_triangle():
    """c = (2, 2) alone in 5 x 5 with x0 = 1.75, y0 = 1.375, L = 1.75 (all dyadic: every step is exact): s = 0.25 to the left,
    0.625 up, 0.875 to the right and down"""
    V, tri = right_triangle(1.75, 1.375, 1.75)
    tind = np.full((1, 25), -1, np.float32)
    tind[0, 2 * 5 + 2] = 0
    return V, tri, tind, 5, 5


def vertical_border(xb):
    """Columns 0 .. 3 of a 4 x 7 image name one triangle whose edge (P1, P2) is the line x = xb: e(P1, P2, X) = -30 (Xx - xb), the
    area is positive, s = xb - 3 for every pair ((3, y), (4, y))"""
    H, W = 4, 7
    V = _f([[[xb, xb, -30], [-10, 20, 5], [1, 1, 1]]])
    tind = np.full((H, W), -1, np.float32)
    tind[:, :4] = 0
    return V, _f([[0], [1], [2]]), tind.reshape(1, -1), H, W


def zero_area():
    """the centre of 3 x 3 names a triangle with three collinear vertices: every pair is inert"""
    tind = np.full((1, 9), -1, np.float32)
    tind[0, 4] = 0
    return _f([[[1, 2, 3], [1, 2, 3], [1, 1, 1]]]), _f([[0], [1], [2]]), tind, 3, 3


def four_slivers():
    """5 x 5, the background pixel u = (2, 2); its four neighbours each name a thin triangle of their own that points at u and ends
    about 0.9 of the way: each adds about 0.4, u clamps at 1"""
    tips = {(1, 2): (1.9, 2.005), (3, 2): (2.1, 1.995), (2, 1): (2.005, 1.9), (2, 3): (1.995, 2.1)}
    vx, vy, tri = [], [], []
    tind = np.full((5, 5), -1, np.float32)
    for t, ((cx, cy), (tx, ty)) in enumerate(tips.items()):
        dx, dy = np.sign(tx - cx) * (abs(tx - cx) > 0.5), np.sign(ty - cy) * (abs(ty - cy) > 0.5)
        bx, by = cx - 0.3 * dx, cy - 0.3 * dy                                # the base, behind the centre, 0.4 wide
        vx += [bx - 0.2 * dy, bx + 0.2 * dy, tx]
        vy += [by - 0.2 * dx, by + 0.2 * dx, ty]
        tri.append([3 * t, 3 * t + 1, 3 * t + 2])
        tind[cy, cx] = t
    V = _f([[vx, vy, [1.0] * len(vx)]])
    return V, _f(np.array(tri).T), tind.reshape(1, -1), 5, 5


def tiny_triangle():
    """the centre of 5 x 5 names a triangle 0.1 around it: every pair ends at s of about 0.1, the pixel clamps at 0"""
    tind = np.full((1, 25), -1, np.float32)
    tind[0, 12] = 0
    return _f([[[1.9, 2.1, 2.0], [1.93, 1.93, 2.12], [1, 1, 1]]]), _f([[0], [1], [2]]), tind, 5, 5
