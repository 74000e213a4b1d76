"""CPU: contour landmarks (include/fr_hotpath.h, "contour landmarks") without a GPU -- the binding row, every return code of the
header's checks (all before any HIP call), utils/synth.py::contour_lines, the ValueErrors the Python surface raises before it
touches a device, and the numpy model (tests/ref_landmark_contour.py): its nearest selection against the truth's own contour finds
that contour with F = 0 exactly, and the contour slides with the yaw on the small assets."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
import ref_landmark as RL
import ref_landmark_contour as RC

ROW = "i:ppzpppippipiiiiiiifppppp"
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4


def test_name_and_row():
    host = pkg("_lib")
    assert "fr_landmark_contour_select" in host.EXPORTS and host.SIGNATURES["fr_landmark_contour_select"] == ROW
    assert "fr_landmark_contour.hip" in host.SOURCES
    src = open(os.path.join(ROOT, "include", "fr_hotpath.h")).read()
    assert "---- contour landmarks ----" in src
    m = re.search(r"\bfr_landmark_contour_select\(([^;]*)\);", src)
    assert m and len(m.group(1).split(",")) == len(ROW.split(":")[1]) == 24
    assert re.search(r"fr_landmark_contour_select\([^;]*void\* stream\);", src)
    getattr(host.lib(), "fr_landmark_contour_select")


# ---- return codes: made-up non-NULL pointers; every case returns before any HIP call ---------------------------------------------------
def test_return_codes():
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    L = pkg("_lib").lib()
    p, q, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), None   # q: not 16-byte aligned
    Kf, C, M, ns, ne, B = 5, 3, 7, 9, 5, 3
    nb = L.fr_landmark_basis_bytes(Kf + C * M, ns, ne)

    def sel(params=p, lb=p, nbytes=None, R=nul, ft=p, fw=nul, fwb=0, lt=p, lw=nul, lwb=0, ld=p, rule=0, B=B, Kf=Kf, C=C, M=M, ns=ns,
            ne=ne, sel=p, lp=p, target=p, weight=p):
        if nbytes is None:
            nbytes = L.fr_landmark_basis_bytes(Kf + C * M, ns, ne) if Kf >= 0 and C >= 0 and M >= 0 else 0
        return L.fr_landmark_contour_select(params, lb, nbytes, R, ft, fw, fwb, lt, lw, lwb, ld, rule, B, Kf, C, M, ns, ne, 200.0, sel,
                                            lp, target, weight, nul)
    # (1) negative sizes, the rule and the flags
    for kw in (dict(B=-1), dict(Kf=-1), dict(C=-1), dict(M=-1), dict(ns=-1), dict(ne=-1), dict(rule=2), dict(rule=-1), dict(fwb=2),
               dict(fwb=-1), dict(lwb=2), dict(lwb=-1)):
        assert sel(**kw) == INVALID, kw
    # (2) nothing to do
    assert sel(B=0) == OK and sel(C=0) == OK and sel(B=0, params=nul, sel=nul, lp=nul) == OK and sel(C=0, M=0, lb=nul) == OK
    # (3) what must be there
    assert sel(params=nul) == INVALID and sel(sel=nul) == INVALID and sel(lp=nul) == INVALID
    assert sel(rule=0, lt=nul, target=nul) == INVALID and sel(rule=1, ld=nul) == INVALID
    assert sel(rule=1, lt=nul) == INVALID                                  # a target output needs the lines' targets
    assert sel(ft=nul) == INVALID                                          # ... and, with fixed ids, theirs
    # (4) the limits
    assert sel(M=0) == UNSUPPORTED and sel(Kf=1024) == UNSUPPORTED and sel(Kf=0, C=257, M=1) == UNSUPPORTED
    assert sel(Kf=0, C=4, M=257) == UNSUPPORTED and sel(ns=200, ne=57) == UNSUPPORTED
    assert sel(Kf=0, C=65536, M=65536) == UNSUPPORTED                      # (C M past 2^31)
    # (5) the image
    assert sel(lb=nul) == WORKSPACE and sel(lb=q) == WORKSPACE and sel(nbytes=nb - 1) == WORKSPACE
    # the order of the checks
    assert sel(B=-1, C=0) == INVALID and sel(rule=2, B=0) == INVALID and sel(C=0, params=nul) == OK
    assert sel(params=nul, M=0) == INVALID and sel(ft=nul, Kf=1024) == INVALID and sel(M=0, lb=nul) == UNSUPPORTED
    # the optional arguments may be absent: only the image is then left to object
    assert sel(rule=1, lt=nul, target=nul, ft=nul, weight=nul, lb=nul) == WORKSPACE
    assert sel(rule=0, ld=nul, Kf=0, ft=nul, lb=nul) == WORKSPACE
    assert sel(Kf=1023, C=1, M=1, lb=nul) == WORKSPACE and sel(Kf=0, C=4, M=256, lb=nul) == WORKSPACE
    assert sel(Kf=0, C=256, M=4, lb=nul) == WORKSPACE


# ---- contour_lines ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gu,gv,per_side,M,stride", [(20, 24, 4, 8, 1), (145, 367, 8, 24, 4), (5, 2, 3, 1, 1), (20, 24, 1, 3, 5)])
def test_contour_lines(synth, gu, gv, per_side, M, stride):
    lines, line_dir = synth.contour_lines(gu, gv, per_side, M, stride)
    again = synth.contour_lines(gu, gv, per_side, M, stride=stride)
    assert lines.dtype == np.int64 and lines.shape == (2 * per_side, M)
    assert line_dir.dtype == np.float32 and line_dir.shape == (2 * per_side, 2)
    assert np.array_equal(lines, again[0]) and np.array_equal(line_dir, again[1])
    assert lines.min() >= 0 and lines.max() < gu * gv
    iu, iv = lines // gv, lines % gv
    assert (iu == iu[:, :1]).all()                                            # a line stays on its row
    assert (iv[:per_side, 0] == 0).all() and (iv[per_side:, 0] == gv - 1).all()    # the rim at position 0
    assert (np.diff(iv[:per_side], axis=1) == stride).all() and (np.diff(iv[per_side:], axis=1) == -stride).all()
    assert np.array_equal(iu[:per_side, 0], iu[per_side:, 0])
    rows = iu[:per_side, 0]
    assert rows.min() >= 1 and rows.max() <= gu - 2 and (np.diff(rows) >= 1).all()
    assert len(np.unique(lines)) == lines.size                                # the two sides never meet
    assert (line_dir[:per_side] == [-1, 0]).all() and (line_dir[per_side:] == [1, 0]).all()


def test_contour_lines_refuses(synth):
    for bad in ((20, 24, 0, 8, 1), (20, 24, 4, 0, 1), (20, 24, 4, 8, 0), (20, 24, 4, 13, 1), (20, 24, 4, 8, 2), (5, 24, 4, 2, 1)):
        with pytest.raises(ValueError):
            synth.contour_lines(*bad)


# ---- the ValueErrors that come before any device is touched ---------------------------------------------------------------------------
def test_value_errors():
    ops = pkg("rendering_layer.ops")
    mu, pcs, pce = torch.zeros(30), torch.zeros(30, 2), torch.zeros(30, 1)      # N = 10
    for lines in ([[1, 2], [3]], [], [[]], [1, 2, 3], np.zeros((2, 2, 2), np.int64)):
        with pytest.raises(ValueError):
            ops.landmark_contour_basis(mu, pcs, pce, [0], lines)
    with pytest.raises(ValueError, match="outside"):
        ops.landmark_contour_basis(mu, pcs, pce, [0], [[1, 10]])
    with pytest.raises(ValueError, match="outside"):
        ops.landmark_contour_basis(mu, pcs, pce, [-1], [[1, 2]])
    with pytest.raises(ValueError, match="1024"):
        ops.landmark_contour_basis(mu, pcs, pce, list(range(10)) * 100, [[1] * 5] * 5)     # 1000 + 25
    with pytest.raises(ValueError):
        ops.landmark_contour_basis(mu, pcs, pce, [], [[1]] * 257)
    cb = ops.LandmarkBasis(torch.zeros(16, dtype=torch.uint8), 7, 2, 1, range(7), n_fixed=1, C=2, M=3)
    assert (cb.n_fixed, cb.C, cb.M) == (1, 2, 3)
    plain = ops.LandmarkBasis(torch.zeros(16, dtype=torch.uint8), 7, 2, 1, range(7))
    assert (plain.n_fixed, plain.C, plain.M) == (7, 0, 0)
    P = torch.zeros(2, 10)
    lt = torch.zeros(2, 2, 2)
    for call in (ops.landmark_contour_select, ops.landmark_contour_sse):
        with pytest.raises(ValueError, match="rule"):
            call(P, cb, lt, rule="farthest")
        with pytest.raises(ValueError, match="grad"):
            call(P, cb, lt.clone().requires_grad_(True))
        with pytest.raises(ValueError, match="grad"):
            call(P, cb, lt, line_weight=torch.ones(2, requires_grad=True))
        with pytest.raises(ValueError, match="lines"):
            call(P, plain, lt)
    with pytest.raises(ValueError, match="rule"):
        ops.landmark_fit(P, cb, torch.zeros(2, 1, 2), line_target=lt, rule="farthest")
    with pytest.raises(ValueError, match="grad"):
        ops.landmark_fit(P, cb, torch.zeros(2, 1, 2), line_target=lt.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="lines"):
        ops.landmark_fit(P, plain, torch.zeros(2, 7, 2), line_target=lt)


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def fit_setting(A, synth, yaw):
    """The setting of the issue's CPU experiment: the small assets, 20 fixed ids, 4 rows a side with the 8 outermost columns as
    candidates, the truth (0.1, yaw, -0.1, 100, 100, 1e-3) at coefficients 0 and the start (+0.05, -+0.15, +0.05 rad, +3 px, -3 px,
    f + 5 %) off it.  -> dict(fixed, lines, line_dir, mean, U, truth, start)"""
    ns, ne = A["ndim_shape"], A["ndim_exp"]
    fixed = synth.landmark_ids(A, 20)
    lines, line_dir = synth.contour_lines(20, 24, 4, 8)
    ids = np.concatenate([fixed, lines.reshape(-1)])
    mean, U = RL.split_image(RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], ids), len(ids), ns + ne)
    truth = np.zeros((1, 7 + ns + ne), np.float32)
    truth[0, :7] = [0.1, yaw, -0.1, 100.0, 100.0, 0.0, 1e-3]
    start = truth.copy()
    start[0, :7] += np.array([0.05, -0.15 * np.sign(yaw), 0.05, 3.0, -3.0, 0.0, 0.05e-3], np.float32)
    return dict(fixed=fixed, lines=lines, line_dir=line_dir, mean=mean, U=U, truth=truth, start=start, Kf=20, C=8, M=8)


@pytest.mark.parametrize("yaw", [0.5, -0.5, 0.0])
def test_nearest_at_the_truth_finds_the_truths_contour(small_assets, synth, yaw):
    s = fit_setting(small_assets, synth, yaw)
    Kf, C, M = s["Kf"], s["C"], s["M"]
    ext = RC.Select(s["truth"], s["mean"], s["U"], Kf, C, M, RC.EXTREME, line_dir=s["line_dir"])
    print("yaw %+.1f: the contour sits at positions %s" % (yaw, ext.sel[0].tolist()))
    assert (ext.sel >= 0).all()
    if yaw == 0.0:
        assert (ext.sel == 0).all()                               # frontal: the rim
    else:
        far = ext.sel[0, :4] if yaw > 0 else ext.sel[0, 4:]       # the side turned away from the camera slides inwards ...
        near = ext.sel[0, 4:] if yaw > 0 else ext.sel[0, :4]
        assert (far >= 2).all() and (far < M - 1).all() and (near == 0).all(), (far, near)     # ... and stays inside the line
    # the winners' points are the forward's own, rounded once
    k = Kf + np.arange(C) * M + ext.sel[0]
    assert np.array_equal(ext.line_points[0].view(np.uint32), ext.fw.points[0, 0:2, k].view(np.uint32))
    # nearest against those points: the same selection, and F = 0 exactly (the fixed targets are the forward's points too)
    fixed_target = np.ascontiguousarray(ext.fw.points[:, 0:2, :Kf].transpose(0, 2, 1))
    near_sel = RC.Select(s["truth"], s["mean"], s["U"], Kf, C, M, RC.NEAREST, line_target=ext.line_points, fixed_target=fixed_target)
    assert np.array_equal(near_sel.sel, ext.sel)
    assert near_sel.target.shape == (1, Kf + C * M, 2) and near_sel.weight.sum() == Kf + C
    # F under the call's own fp32 targets is the rounding of the points alone: |x - fl32(x)| <= u |x|, |x| < 200
    F = RC.sse(s["truth"], s["mean"], s["U"], near_sel)
    assert 0.0 <= F[0] <= (Kf + C) * 2 * (2.0 ** -24 * 200.0) ** 2
    # ... and against the unrounded points (the issue's float64 experiment) it is 0 exactly: the rule's own loop, on float64 targets
    xy = ext.fw.xyz[0, :, 0:2]
    F64 = 0.0
    for c in range(C):
        tx, ty = xy[Kf + c * M + ext.sel[0, c]]
        best, bm = np.inf, -1
        for m in range(M):
            x, y = xy[Kf + c * M + m]
            d = (x - tx) * (x - tx) + (y - ty) * (y - ty)
            if d < best:
                best, bm = d, m
        assert bm == ext.sel[0, c]
        F64 = F64 + best
    assert F64 == 0.0
    # at the start of the fit the selection differs from the truth's on the far side: the correspondence has to slide
    at_start = RC.Select(s["start"], s["mean"], s["U"], Kf, C, M, RC.NEAREST, line_target=ext.line_points, fixed_target=fixed_target)
    assert (at_start.sel >= 0).all()


def test_model_rules_and_specials(small_assets, synth):
    s = fit_setting(small_assets, synth, 0.5)
    Kf, C, M = s["Kf"], s["C"], s["M"]
    P = np.repeat(s["truth"], 3, axis=0)
    P[1, :] = np.nan                                               # a failing face
    lt = np.full((3, C, 2), 100.0, np.float32)
    lw = np.ones((3, C), np.float32)
    lw[0, 2] = 0.0
    lt[0, 2] = np.nan                                              # a missing line: weight 0 under a NaN target
    r = RC.Select(P, s["mean"], s["U"], Kf, C, M, RC.NEAREST, line_target=lt, line_weight=lw)
    assert r.target is None                                        # fixed ids without fixed_target
    assert (r.sel[1] == -1).all() and not r.line_points[1].any() and not r.weight[1, Kf:].any() and (r.weight[1, :Kf] == 1).all()
    assert r.sel[0, 2] == -1 and not r.weight[0, Kf + 2 * M:Kf + 3 * M].any()
    keep = np.arange(C) != 2                                       # face 2 has face 0's parameters: the other lines agree
    assert np.array_equal(r.sel[2, keep], r.sel[0, keep]) and r.sel[2, 2] >= 0
    assert (r.weight[2, Kf:].reshape(C, M).sum(axis=1) == 1).all()
    # a line of one repeated id: every candidate ties, the lowest m wins -- under either rule
    mean, U = s["mean"].copy(), s["U"].copy()
    mean[Kf:Kf + M], U[Kf:Kf + M] = mean[Kf + 3], U[Kf + 3]
    for rule in (RC.NEAREST, RC.EXTREME):
        d = RC.Select(s["truth"], mean, U, Kf, C, M, rule, line_target=lt[2:3], line_dir=s["line_dir"])
        assert d.sel[0, 0] == 0
