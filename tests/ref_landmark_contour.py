"""numpy float64 model of the contour-landmark selection (include/fr_hotpath.h, "contour landmarks"), built on the landmark model's
forward (tests/ref_landmark.py::Forward, whose xyz are the projections BEFORE the fp32 rounding): explicit loops over the lines and
their candidates m in ascending order with strict comparisons, every product and every sum rounded on its own.  The kernel is held to
this file bit for bit (tests/test_landmark_contour_gpu.py)."""
import numpy as np

import ref_landmark as RL

NEAREST, EXTREME = 0, 1


def _line_weights(line_weight, B, C):
    if line_weight is None:
        return np.ones((B, C), np.float32)
    w = np.asarray(line_weight, np.float32)
    return np.broadcast_to(w, (B, C)) if w.ndim == 1 else w


class Select:
    """The select call of B faces over a compact image of Kf fixed ids followed by C lines of M candidates (mean [K,3], U [K,3,Kt]
    float64 of ref_landmark.split_image, K = Kf + C M).  P [B, 7 + Kt] fp32; R None or [B,3,3]; line_target None or [B,C,2];
    line_weight None, [C] or [B,C]; fixed_target None or [B,Kf,2]; fixed_weight None, [Kf] or [B,Kf]; line_dir None or [C,2].
    Fields: sel [B,C] int32, line_points [B,C,2] fp32, target [B,K,2] fp32 or None (without line_target, or with fixed ids and no
    fixed_target), weight [B,K] fp32."""

    def __init__(self, P, mean, U, Kf, C, M, rule, line_target=None, line_weight=None, fixed_target=None, fixed_weight=None,
                 line_dir=None, R=None, im_size=200.0):
        P = np.asarray(P, np.float32)
        B, K = P.shape[0], Kf + C * M
        assert mean.shape[0] == K and rule in (NEAREST, EXTREME)
        assert (line_target is not None) if rule == NEAREST else (line_dir is not None)
        fw = RL.Forward(P, mean, U, R=R, im_size=im_size)
        xyz = fw.xyz
        lw = _line_weights(line_weight, B, C)
        lt = None if line_target is None else np.asarray(line_target, np.float32).reshape(B, C, 2)
        ld = None if line_dir is None else np.asarray(line_dir, np.float32).astype(np.float64).reshape(C, 2)
        sel = np.full((B, C), -1, np.int32)
        pts = np.zeros((B, C, 2), np.float32)
        weight = np.zeros((B, K), np.float32)
        if Kf:
            weight[:, :Kf] = 1.0 if fixed_weight is None else np.asarray(fixed_weight, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for b in range(B):
                for c in range(C):
                    if lw[b, c] == 0:          # not looked at: the target is never read
                        continue
                    best = np.inf if rule == NEAREST else -np.inf
                    for m in range(M):
                        k = Kf + c * M + m
                        x, y = xyz[b, k, 0], xyz[b, k, 1]
                        if rule == NEAREST:
                            dx, dy = x - np.float64(lt[b, c, 0]), y - np.float64(lt[b, c, 1])
                            s = dx * dx + dy * dy
                            wins = s < best
                        else:
                            s = ld[c, 0] * x + ld[c, 1] * y
                            wins = s > best
                        if wins:
                            best = s
                            sel[b, c] = m
                            pts[b, c, 0], pts[b, c, 1] = np.float32(x), np.float32(y)
                    if sel[b, c] >= 0:
                        weight[b, Kf + c * M + sel[b, c]] = lw[b, c]
        self.fw, self.sel, self.line_points, self.weight = fw, sel, pts, weight
        self.target = None
        if lt is not None and (Kf == 0 or fixed_target is not None):
            target = np.empty((B, K, 2), np.float32)
            if Kf:
                target[:, :Kf] = np.asarray(fixed_target, np.float32).reshape(B, Kf, 2)
            target[:, Kf:] = np.repeat(lt, M, axis=1)
            self.target = target


def sse(P, mean, U, sel, R=None, im_size=200.0):
    """the landmark model's forward under a Select's own target and weight -> sse [B] float64"""
    return RL.Forward(P, mean, U, R=R, target=sel.target, weight=sel.weight, im_size=im_size).sse
