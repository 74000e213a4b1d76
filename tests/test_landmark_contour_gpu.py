"""GPU: contour landmarks (fr_landmark_contour_select; include/fr_hotpath.h, "contour landmarks") against the numpy model
tests/ref_landmark_contour.py -- sel, line_points, target and weight bit for bit --, a cross-check that needs no model (the masked
forward against the forward over the winners alone: the same sse bits), the fit of the issue's experiment with sliding and with
fixed correspondences, the Python surface, SynthBatches, the example as a program, and the defaults: without the new arguments
landmark_fit and landmark_loss give the bits of the loop and the formula they had before."""
import ctypes
import json
import sys

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import assert_bits_equal
import ref_landmark as RL
import ref_landmark_contour as RC
import ref_pose_backward as RP
import test_landmark_contour_cpu as TC      # (fit_setting: the issue's experiment)
import test_landmark_gpu as TG              # (its helpers: the C calls of the landmark term, the program runner)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IM = 200.0
_t = TG._t


def _h():
    return pkg("_lib")


def _ops():
    return pkg("rendering_layer.ops")


def c_select(c, P, rule, R=None, line_target=None, line_weight=None, fixed_target=None, fixed_weight=None, line_dir=None,
             want_target=True, want_weight=True):
    """the raw call on prefilled outputs -> (sel, line_points, target or None, weight or None) as numpy"""
    h, L = _h(), _h().lib()
    B, Kf, C, M = int(P.shape[0]), c["Kf"], c["C"], c["M"]
    K = Kf + C * M
    sel = torch.full((B, C), -7, dtype=torch.int32, device=DEV)
    pts = torch.full((B, C, 2), 7.0, dtype=torch.float32, device=DEV)
    target = torch.full((B, K, 2), 7.0, dtype=torch.float32, device=DEV) if want_target else None
    weight = torch.full((B, K), 7.0, dtype=torch.float32, device=DEV) if want_weight else None
    fwb = 1 if fixed_weight is not None and fixed_weight.dim() == 2 else 0
    lwb = 1 if line_weight is not None and line_weight.dim() == 2 else 0
    rc = L.fr_landmark_contour_select(h.ptr(P), h.ptr(c["img"]), c["img"].numel() * 4, h.ptr(R), h.ptr(fixed_target), h.ptr(fixed_weight),
                                      fwb, h.ptr(line_target), h.ptr(line_weight), lwb, h.ptr(line_dir), rule, B, Kf, C, M, c["ns"],
                                      c["ne"], IM, h.ptr(sel), h.ptr(pts), h.ptr(target), h.ptr(weight),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (sel.cpu().numpy(), pts.cpu().numpy(), None if target is None else target.cpu().numpy(),
            None if weight is None else weight.cpu().numpy())


# ---- the cases: inputs and the model's image, built once ---------------------------------------------------------------------------
# (Kf, C, M).  In (250, 2, 5) and (250, 3, 5) line 1 is k = 255 .. 259: it straddles the chunk boundary at k = 256 (the last line in
# the one, a middle line in the other); its ids are distinct and the case is built so that its winner lies in the second chunk.
SHAPES = [(0, 1, 1), (5, 3, 7), (250, 2, 5), (250, 3, 5), (0, 4, 256), (1023, 1, 1)]
CASES = [(kt, B) + s for kt in (0, 14) for B in (1, 3) for s in SHAPES]
IDS = ["Kt%d-B%d-Kf%d-C%d-M%d" % c for c in CASES]
_ASSETS, _CASES = {}, {}


def _assets(kt):
    if kt not in _ASSETS:
        ns, ne = {0: (0, 0), 14: (9, 5)}[kt]
        _ASSETS[kt] = pkg("utils.synth").make_small_assets(n_shape=ns, n_exp=ne)
    return _ASSETS[kt]


def _case(kt, B, Kf, C, M):
    key = (kt, B, Kf, C, M)
    if key not in _CASES:
        A = _assets(kt)
        rs = np.random.RandomState(1000 + 31 * B + Kf + 7 * C + M + kt)
        ns, ne = A["ndim_shape"], A["ndim_exp"]
        N = np.asarray(A["mu"]).size // 3
        K = Kf + C * M
        idx = rs.randint(0, N, K).astype(np.int64)
        straddle = [ci for ci in range(C) if Kf + ci * M < 256 < Kf + (ci + 1) * M]
        straddle = straddle[0] if straddle else None
        dup = 0 if M > 1 and straddle != 0 else None
        if dup is not None:
            idx[Kf:Kf + M] = idx[Kf]                                # line 0 repeats one id: every candidate ties, m = 0 wins
        P = pkg("utils.synth").sample_params_batch(B, im_size=200, n_shape=ns, n_exp=ne, seed=70 + B).astype(np.float32)
        R = RP.rotations(rs, B)
        line_dir = rs.standard_normal((C, 2)).astype(np.float32)
        first = None if straddle is None else Kf + straddle * M
        if straddle is not None:
            idx[first:first + M] = rs.choice(N, M, replace=False)   # distinct vertices: no ties on this line
        img_np = RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], idx)
        mean, Um = RL.split_image(img_np, K, ns + ne)
        fw = RL.Forward(P, mean, Um)
        if straddle is not None:
            # face 0's extreme candidate along the line's direction goes behind the boundary: if it lies in the first chunk, its id
            # changes places with the line's last one
            d = line_dir[straddle].astype(np.float64)
            m_ext = int(np.argmax(d[0] * fw.xyz[0, first:first + M, 0] + d[1] * fw.xyz[0, first:first + M, 1]))
            if first + m_ext < 256:
                idx[[first + m_ext, first + M - 1]] = idx[[first + M - 1, first + m_ext]]
                img_np = RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], idx)
                mean, Um = RL.split_image(img_np, K, ns + ne)
                fw = RL.Forward(P, mean, Um)
        # targets near the face: a random candidate's point plus noise, so that the nearest is not trivially one of the ends
        pick = Kf + np.arange(C) * M + rs.randint(0, M, (B, C))
        lt = (np.take_along_axis(fw.xyz[:, :, 0:2], pick[:, :, None], axis=1) + rs.uniform(-5, 5, (B, C, 2))).astype(np.float32)
        if straddle is not None:     # ... and face 0's target on that line is the point of a candidate of the second chunk
            lt[0, straddle] = fw.xyz[0, max(256, first + M - 2), 0:2].astype(np.float32)
        ft = (fw.xyz[:, :Kf, 0:2] + rs.uniform(-3, 3, (B, Kf, 2))).astype(np.float32)
        if Kf:
            ft[B - 1, 0, 1] = np.nan                                # (copied bit for bit, whatever it holds)
        lwC, lwBC = rs.uniform(0.25, 2.0, C).astype(np.float32), rs.uniform(0.25, 2.0, (B, C)).astype(np.float32)
        fwK, fwBK = rs.uniform(0.25, 2.0, Kf).astype(np.float32), rs.uniform(0.25, 2.0, (B, Kf)).astype(np.float32)
        lwC[0] = 0.0                                                # a missing line: weight 0 under a NaN target
        lwBC[B - 1, C - 1] = 0.0
        ltC, ltBC = lt.copy(), lt.copy()
        ltC[:, 0] = np.nan
        ltBC[B - 1, C - 1] = np.nan
        mu, pcs, pce = _t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"])
        _CASES[key] = dict(A=A, N=N, K=K, Kf=Kf, C=C, M=M, B=B, ns=ns, ne=ne, idx=idx, straddle=straddle, dup=dup, mean=mean, Um=Um, P=P, R=R, line_dir=line_dir, lt=lt,
                           ft=ft, weights=[("NULL", lt, None, None), ("per line", ltC, lwC, fwK), ("per face", ltBC, lwBC, fwBK)],
                           img=TG.c_build(mu, pcs, pce, idx, N, ns, ne))
    return _CASES[key]


def _assert_select(got, want, name, with_target=True):
    sel, pts, target, weight = got
    assert np.array_equal(sel, want.sel), (name, sel, want.sel)
    assert_bits_equal(pts, want.line_points, name + ": line_points")
    assert_bits_equal(weight, want.weight, name + ": weight")
    if with_target:
        assert_bits_equal(target, want.target, name + ": target")
        assert np.array_equal(np.isnan(target), np.isnan(want.target)), name


@pytest.mark.parametrize("kt,B,Kf,C,M", CASES, ids=IDS)
def test_select_bit_for_bit(kt, B, Kf, C, M):
    c = _case(kt, B, Kf, C, M)
    P = _t(c["P"])
    chosen = set()
    for rule in (RC.NEAREST, RC.EXTREME):
        for R in (None, c["R"]):
            for wname, lt, lw, fw_ in c["weights"]:
                name = "rule %d, %s, %s weights" % (rule, "override" if R is not None else "rotation", wname)
                got = c_select(c, P, rule, R=_t(R), line_target=_t(lt), line_weight=_t(lw), fixed_target=_t(c["ft"]) if Kf else None,
                               fixed_weight=_t(fw_) if Kf else None, line_dir=_t(c["line_dir"]))
                want = RC.Select(c["P"], c["mean"], c["Um"], Kf, C, M, rule, line_target=lt, line_weight=lw,
                                 fixed_target=c["ft"] if Kf else None, fixed_weight=fw_ if Kf else None, line_dir=c["line_dir"], R=R)
                _assert_select(got, want, name)
                if lw is not None:     # the missing line has no winner
                    gone = got[0][:, 0] if lw.ndim == 1 else got[0][B - 1:, C - 1]
                    assert (gone == -1).all(), name
                if c["dup"] is not None and (lw is None or (lw.ndim == 2 and (B > 1 or C > 1))):   # one repeated id: the lowest m
                    assert got[0][0, c["dup"]] == 0, name
                if c["straddle"] is not None and lw is None and R is None:
                    # the line across k = 256: face 0's winner lies in the second chunk -- the lane's carried (best, m, x, y) was
                    # overwritten there, and line_points holds that candidate's point (compared with the model above)
                    first = Kf + c["straddle"] * M
                    assert first < 256 <= first + int(got[0][0, c["straddle"]]), (name, got[0][0])
                chosen.update(got[0].reshape(-1).tolist())
    if M >= 5:
        assert len(chosen - {-1, 0}) >= 2, chosen              # the cases do not all end on the rim
    # the optional outputs may be absent, and the extreme rule needs no target at all
    got = c_select(c, P, RC.EXTREME, line_dir=_t(c["line_dir"]), want_target=False, want_weight=False)
    want = RC.Select(c["P"], c["mean"], c["Um"], Kf, C, M, RC.EXTREME, line_dir=c["line_dir"])
    assert got[2] is None and got[3] is None and np.array_equal(got[0], want.sel)
    assert_bits_equal(got[1], want.line_points, "extreme, no outputs")


def test_a_failing_face_stays_in_its_face():
    c = _case(14, 3, 5, 3, 7)
    P = c["P"].copy()
    P[1, :] = np.nan
    args = dict(line_target=_t(c["lt"]), fixed_target=_t(c["ft"]), line_dir=_t(c["line_dir"]))
    for rule in (RC.NEAREST, RC.EXTREME):
        sel, pts, target, weight = c_select(c, _t(P), rule, **args)
        assert (sel[1] == -1).all() and not pts[1].any() and not np.signbit(pts[1]).any()
        assert not weight[1, 5:].any() and (weight[1, :5] == 1).all()
        for b in (0, 2):     # the neighbours: the bits of the face alone, and of the batch without the NaN
            alone = c_select(c, _t(P[b:b + 1]), rule, **{k: v[b:b + 1] if k != "line_dir" else v for k, v in args.items()})
            healthy = c_select(c, _t(c["P"]), rule, **args)
            for g, a, hh in zip((sel, pts, target, weight), alone, healthy):
                assert np.array_equal(g[b:b + 1].view(np.uint32), a.view(np.uint32))
                assert np.array_equal(g[b].view(np.uint32), hh[b].view(np.uint32))
        want = RC.Select(P, c["mean"], c["Um"], 5, 3, 7, rule, line_target=c["lt"], fixed_target=c["ft"], line_dir=c["line_dir"])
        _assert_select((sel, pts, target, weight), want, "NaN face, rule %d" % rule)


@pytest.mark.parametrize("kt,Kf,C,M", [(14, 5, 3, 7), (14, 250, 2, 5), (0, 0, 4, 256), (14, 0, 1, 1)])
def test_masked_forward_equals_the_forward_over_the_winners(kt, Kf, C, M):
    """No model: the call's target and weight through fr_landmark_forward over all K, against fr_landmark_forward over a compact
    image of the fixed ids plus the winners alone, in line order -- the non-zero terms are the same and arrive in the same order, so
    the two sse agree in every bit."""
    c = _case(kt, 1, Kf, C, M)
    P = _t(c["P"])
    A = c["A"]
    ft = np.nan_to_num(c["ft"], nan=50.0)        # (the case's NaN fixed target stands under a weight that is not 0: not here)
    for wname, lt, lw, fw_ in c["weights"]:
        sel, pts, target, weight = c_select(c, P, RC.NEAREST, line_target=_t(lt), line_weight=_t(lw),
                                            fixed_target=_t(ft) if Kf else None, fixed_weight=_t(fw_) if Kf else None)
        full = dict(K=c["K"], img=c["img"], ns=c["ns"], ne=c["ne"])
        _, sse_masked = TG.c_forward(full, P, target=_t(target), weight=_t(weight))
        won = [ci for ci in range(C) if sel[0, ci] >= 0]
        keep = list(range(Kf)) + [Kf + ci * M + int(sel[0, ci]) for ci in won]
        if not keep:
            torch.cuda.synchronize()
            assert float(sse_masked[0]) == 0.0
            continue
        ids = c["idx"][keep]
        mu, pcs, pce = _t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"])
        small = dict(K=len(keep), img=TG.c_build(mu, pcs, pce, ids, c["N"], c["ns"], c["ne"]), ns=c["ns"], ne=c["ne"])
        points, sse_small = TG.c_forward(small, P, target=_t(target[:, keep]), weight=_t(weight[:, keep]))
        torch.cuda.synchronize()
        a, b = sse_masked.cpu().numpy(), sse_small.cpu().numpy()
        assert np.isfinite(a).all() and a[0] > 0 and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (wname, a, b)
        # ... and the winners' points are that forward's own
        assert_bits_equal(points.cpu().numpy()[0, 0:2, Kf:].T, pts[0, won], wname + ": line_points")


# ---- the fit: the issue's experiment ----------------------------------------------------------------------------------------------
def test_fit_slides_to_the_truth_where_the_fixed_correspondence_is_biased(small_assets, synth):
    """Two faces, yaw +0.5 and -0.5, pose only, coefficients 0 (as in the CPU experiment: no coefficients are fitted or set), ten
    iterations from the experiment's start; the targets are the forward's fp32 points at the truth, the contour's by the extreme
    rule.  Sliding: the final selection is the truth's, the cost never increases -- across re-selections too --, and the angle and
    translation errors are each under a tenth of the fixed-correspondence fit's (each line held to its rim vertex)."""
    ops = _ops()
    sp, sn = TC.fit_setting(small_assets, synth, 0.5), TC.fit_setting(small_assets, synth, -0.5)
    truth, start = _t(np.concatenate([sp["truth"], sn["truth"]])), _t(np.concatenate([sp["start"], sn["start"]]))
    A = small_assets
    mu, pcs, pce = _t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"])
    cb = ops.landmark_contour_basis(mu, pcs, pce, sp["fixed"], sp["lines"])
    assert (cb.n_fixed, cb.C, cb.M, cb.K) == (20, 8, 8, 84)
    ld = _t(sp["line_dir"])
    sel_truth, line_target, _, _ = ops.landmark_contour_select(truth, cb, rule="extreme", line_dir=ld)
    fixed_target = ops.landmarks(truth, cb)[:, 0:2, :20].transpose(1, 2).contiguous()
    fitted, info = ops.landmark_fit(start, cb, fixed_target, line_target=line_target, iters=10)
    rim = ops.landmark_contour_basis(mu, pcs, pce, sp["fixed"], sp["lines"][:, :1])
    fitted_rim, info_rim = ops.landmark_fit(start, rim, fixed_target, line_target=line_target, iters=10)
    torch.cuda.synchronize()
    sel_truth = sel_truth.cpu().numpy()
    assert np.array_equal(sel_truth, [[3, 5, 5, 3, 0, 0, 0, 0], [0, 0, 0, 0, 3, 5, 5, 3]])      # (the model's: test_landmark_contour_cpu.py)
    sel = info["sel"].cpu().numpy()
    cost, cost_rim = info["cost"].cpu().numpy(), info_rim["cost"].cpu().numpy()
    assert sel.shape == (11, 2, 8) and sel.dtype == np.int32 and cost.shape == (11, 2) and info["accepted"].shape == (10, 2)
    assert not info_rim["sel"].any()

    def errors(p):
        e = (p.double() - truth.double()).abs().cpu().numpy()
        return e[:, 0:3].max(axis=1), e[:, 3:5].max(axis=1), e[:, 6] / 1e-3
    (ang, tr, fr), (ang_r, tr_r, fr_r) = errors(fitted), errors(fitted_rim)
    for b in range(2):
        print("face %d sliding: angle %.3g rad, translation %.3g px, f %.3g rel, F %.3g -> %.3g; sel %s" % (
            b, ang[b], tr[b], fr[b], cost[0, b], cost[-1, b], sel[-1, b].tolist()))
        print("face %d fixed:   angle %.3g rad, translation %.3g px, f %.3g rel, F %.3g -> %.3g" % (
            b, ang_r[b], tr_r[b], fr_r[b], cost_rim[0, b], cost_rim[-1, b]))
    assert np.array_equal(sel[-1], sel_truth)
    assert np.isfinite(cost).all() and (np.diff(cost, axis=0) <= 0).all(), cost
    assert (np.diff(cost_rim, axis=0) <= 0).all()
    assert (ang < 0.1 * ang_r).all() and (tr < 0.1 * tr_r).all(), (ang, ang_r, tr, tr_r)
    assert (ang_r > 0.02).all() and (tr_r > 1.0).all()          # the bias of the fixed correspondence, as the experiment found it
    # FaceRecNet passes the arguments through and caches the basis
    net = pkg("nets.network").FaceRecNet(mesh_data=A, batch_size=2, im_size=200, device=DEV)
    nb = net.landmark_contour_basis(sp["fixed"], sp["lines"])
    assert nb is net.landmark_contour_basis(list(sp["fixed"]), sp["lines"].tolist()) and (nb.n_fixed, nb.C, nb.M) == (20, 8, 8)
    fitted_net, info_net = net.landmark_fit(start, nb, fixed_target, line_target=line_target, iters=10)
    assert torch.equal(fitted_net, fitted) and torch.equal(info_net["sel"], info["sel"]) and torch.equal(info_net["cost"], info["cost"])


# ---- the Python surface --------------------------------------------------------------------------------------------------------------
def test_surface_against_the_c_call_and_the_gradient():
    ops = _ops()
    c = _case(14, 3, 5, 3, 7)
    A = c["A"]
    mu, pcs, pce = _t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"])
    lines = c["idx"][5:].reshape(3, 7)
    cb = ops.landmark_contour_basis(mu, pcs, pce, c["idx"][:5], lines)
    assert cb.idx == tuple(c["idx"].tolist()) and (cb.n_fixed, cb.C, cb.M, cb.K) == (5, 3, 7, 26)
    torch.cuda.synchronize()
    assert torch.equal(cb.image.view(torch.float32), c["img"])
    P = _t(c["P"])
    _, lt, lw, fw_ = c["weights"][2]
    got = ops.landmark_contour_select(P, cb, _t(lt), line_weight=_t(lw), fixed_target=_t(c["ft"]), fixed_weight=_t(fw_), im_size=IM)
    raw = c_select(c, P, RC.NEAREST, line_target=_t(lt), line_weight=_t(lw), fixed_target=_t(c["ft"]), fixed_weight=_t(fw_))
    for g, r in zip(got, raw):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), r.view(np.uint32))
    assert not any(t.requires_grad for t in got)
    ext = ops.landmark_contour_select(P, cb, rule="extreme", line_dir=_t(c["line_dir"]), R=_t(c["R"]))
    assert ext[2] is None and ext[3].shape == (3, 26)
    # the sse is landmark_sse under the selection, and so is its gradient: the selection is a constant
    ft = _t(np.nan_to_num(c["ft"], nan=50.0))       # (the case's NaN fixed target stands under a weight that is not 0: not here)
    p1 = P.clone().requires_grad_(True)
    sse = ops.landmark_contour_sse(p1, cb, _t(lt), line_weight=_t(lw), fixed_target=ft, fixed_weight=_t(fw_), pose_grad=True)
    sse.sum().backward()
    p2 = P.clone().requires_grad_(True)
    want = ops.landmark_sse(p2, cb, torch.cat([ft, got[2][:, 5:]], dim=1), got[3], pose_grad=True)
    want.sum().backward()
    assert sse.dtype == torch.float64 and bool(torch.isfinite(sse).all()) and torch.equal(sse, want)
    assert torch.equal(p1.grad, p2.grad) and bool(p1.grad.abs().sum() > 0)
    # the ValueErrors that need a device
    for bad in (dict(line_target=_t(lt)[:, :2]), dict(line_target=_t(lt), line_weight=_t(lw)[:, :2]),
                dict(line_target=_t(lt), fixed_target=_t(c["ft"])[:, :4]), dict(line_target=_t(lt), fixed_weight=_t(fw_)[:2]),
                dict(line_target=None), dict(rule="extreme"), dict(rule="extreme", line_dir=_t(c["line_dir"])[:2]),
                dict(line_target=_t(lt), R=_t(c["R"])[:2])):
        with pytest.raises(ValueError):
            ops.landmark_contour_select(P, cb, **bad)
    with pytest.raises(ValueError):
        ops.landmark_contour_select(P[:, :20], cb, _t(lt))
    with pytest.raises(ValueError):
        ops.landmark_contour_sse(P, cb, _t(lt))                                  # fixed ids without fixed_target
    with pytest.raises(ValueError):
        ops.landmark_fit(P, cb, None, line_target=_t(lt))
    with pytest.raises(ValueError):
        ops.landmark_contour_basis(mu, pcs, pce, [0, c["N"]], lines)


def test_losses_and_synth_batches(small_assets, synth):
    ops, losses, pipe = _ops(), pkg("nets.losses"), pkg("pipeline")
    B, S = 3, 32
    net = pkg("nets.network").FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S, device=DEV)
    idx = synth.landmark_ids(small_assets, 20)
    lines, line_dir = synth.contour_lines(20, 24, 4, 8)
    kw = dict(slots=1, focal=1e-3 * S / 200.0, landmarks=idx)
    plain = {k: v.clone() for k, v in pipe.SynthBatches(net, B, 77, **kw).next().items()}
    stream = pipe.SynthBatches(net, B, 77, contour_lines=(lines, line_dir), **kw)
    b = {k: v.clone() for k, v in stream.next().items()}
    torch.cuda.synchronize()
    assert set(b) == set(plain) | {"contour_landmarks", "contour_sel"}
    for k, v in plain.items():                                               # every existing key keeps its bits
        assert torch.equal(v, b[k]), k
    assert b["contour_landmarks"].shape == (B, 8, 2) and b["contour_sel"].shape == (B, 8) and b["contour_sel"].dtype == torch.int32
    cb = net.landmark_contour_basis(None, lines)
    sel, pts, _, _ = ops.landmark_contour_select(b["params"], cb, rule="extreme", line_dir=_t(line_dir), im_size=S)
    assert torch.equal(sel, b["contour_sel"]) and torch.equal(pts, b["contour_landmarks"]) and bool((sel >= 0).all())
    # the loss at the truth: the nearest candidate is the contour itself, so only the rounding of the targets is left
    p = b["params"].clone().requires_grad_(True)
    L0 = losses.landmark_loss(net, p, idx, b["landmarks"], lines=lines, line_target=b["contour_landmarks"])
    assert L0.dtype == torch.float64 and 0 <= float(L0) < 1e-8
    # ... and off the truth it is landmark_sse under the selection over the sum of the weights, with its gradient
    q = b["params"].clone()
    q[:, 3] += 0.75
    q.requires_grad_(True)
    lw = torch.tensor([1, 1, 0.5, 1, 1, 2, 1, 1], dtype=torch.float32, device=DEV)
    L1 = losses.landmark_loss(net, q, idx, b["landmarks"], weight=b["landmark_visible"], lines=lines, line_target=b["contour_landmarks"],
                              line_weight=lw)
    L1.backward()
    cb20 = net.landmark_contour_basis(idx, lines)
    _, _, t_k, w_k = ops.landmark_contour_select(q.detach(), cb20, b["contour_landmarks"], line_weight=lw, fixed_target=b["landmarks"],
                                                 fixed_weight=b["landmark_visible"], im_size=S)
    q2 = q.detach().clone().requires_grad_(True)
    want = (ops.landmark_sse(q2, cb20, t_k, w_k, im_size=S, pose_grad=True)
            / (b["landmark_visible"].double().sum(dim=1) + lw.double().sum()).clamp_min(1.0)).mean()
    want.backward()
    assert torch.equal(L1, want) and torch.equal(q.grad, q2.grad) and float(L1) > 0
    with pytest.raises(ValueError):
        losses.landmark_loss(net, p, idx, b["landmarks"], lines=lines)
    with pytest.raises(ValueError):
        losses.landmark_loss(net, p, idx, b["landmarks"], line_target=b["contour_landmarks"])
    # get_loss: the term under its own names, with fixed landmarks beside the lines and without
    pred = q.detach().clone().requires_grad_(True)
    ver = net.vertices_transform(pred)
    args = (net, pred, b["params"], b["im_gray"], ver, b["depth"], b["depth"] * 1.01)
    base = losses.get_loss(*args)
    assert "landmark_loss" not in base
    for kw in (dict(landmark_lines=lines), dict(landmark_line_target=b["contour_landmarks"]),
               dict(landmark_line_weight=lw), dict(landmark_lines=lines, landmark_line_target=b["contour_landmarks"],
                                                   landmark_target=b["landmarks"])):
        with pytest.raises(ValueError):
            losses.get_loss(*args, **kw)
    lam = 0.25
    full = losses.get_loss(*args, landmark_target=b["landmarks"], landmark_idx=idx, landmark_weight=b["landmark_visible"],
                           landmark_lines=lines, landmark_line_target=b["contour_landmarks"], landmark_line_weight=lw, lambda_landmark=lam)
    assert list(full) == list(base) + ["landmark_loss"]
    assert torch.equal(full["landmark_loss"].detach(), L1.detach())
    assert float(full["total_loss"]) == float(base["total_loss"] + (lam * L1.detach()).to(base["total_loss"].dtype))
    for k in base:
        if k != "total_loss":
            assert float(full[k]) == float(base[k]), k
    alone = losses.get_loss(*args, landmark_lines=lines, landmark_line_target=b["contour_landmarks"])
    term = losses.landmark_loss(net, pred, None, None, lines=lines, line_target=b["contour_landmarks"])
    assert torch.equal(alone["landmark_loss"].detach(), term.detach()) and float(term) > 0
    full["total_loss"].backward()
    assert pred.grad is not None and float(pred.grad[:, 0:3].abs().max()) > 0       # the term reaches the angles


def test_photo_fit_contour_program():
    base = [sys.executable, "examples/photo_fit.py", "--small", "--fit-pose", "--landmarks", "20", "--contour", "4", "--landmarks-only",
            "--landmark-init", "10", "--steps", "0"]
    d = TG._run(base)
    print(json.dumps(d))
    ct, init = d["contour"], d["landmark_init"]
    assert ct["per_side"] == 4 and ct["depth"] == 8 and ct["fixed"] is False and d["yaw"] is None
    assert np.array(ct["sel_truth"]).shape == (3, 8) and ct["sel_fitted"] == ct["sel_truth"]
    assert d["finite"] is True and init["iters"] == 10 and init["cost_last"] < 1e-6 * init["cost_first"]
    assert d["errors_after"]["t3d_rms"] < 1e-3 and d["errors_after"]["angle_rms"] < 1e-4
    # the truth turned by half a radian: the contour leaves the rim on the far side, and the fit follows it there
    y = TG._run(base + ["--yaw", "0.5"])
    print(json.dumps(y))
    st = np.array(y["contour"]["sel_truth"])
    assert y["yaw"] == 0.5 and (st[:, :4] >= 2).all() and (st[:, 4:] == 0).all() and y["contour"]["sel_fitted"] == y["contour"]["sel_truth"]
    assert y["errors_after"]["t3d_rms"] < 1e-3 and y["errors_after"]["angle_rms"] < 1e-4


# ---- the defaults ------------------------------------------------------------------------------------------------------------------
def test_defaults_keep_their_bits(small_assets, synth):
    """landmark_fit and landmark_loss without the new arguments: the loop and the formula they had before this feature, restated
    here from the operators that did not change (landmark_solve_step, landmark_sse) -- the same bits, before and after the contour
    calls have run in the process."""
    ops, losses = _ops(), pkg("nets.losses")
    c = TG._case("small", 3, 68)
    P, target, weight = _t(c["P"]), _t(c["target"]), _t(c["wBK"])
    net = pkg("nets.network").FaceRecNet(mesh_data=c["A"], batch_size=3, im_size=200, device=DEV)
    lb = net.landmark_basis(c["idx"])
    assert (lb.n_fixed, lb.C, lb.M) == (68, 0, 0)
    P0 = P.clone()
    P0[:, 3:5] += 2.0
    ridge, center = (_t(a) for a in synth.coefficient_prior(c["ns"], c["ne"]))

    def fit_before(fit_coef):
        cur = P0.clone()
        damp = torch.full((3,), 1e-3, dtype=torch.float64, device=DEV)
        three = torch.full((3,), 3.0, dtype=torch.float64, device=DEV)

        def F_of(p):
            F = ops.landmark_sse(p, lb, target, weight)
            if fit_coef:
                d = p[:, 7:].double() - center.double()
                F = F + (ridge.double() * d * d).sum(dim=1)
            return F
        F = F_of(cur)
        costs = [F]
        for _ in range(4):
            delta, _, ok = ops.landmark_solve_step(cur, lb, target, weight, ridge=ridge, center=center, damp=damp, fit_coef=fit_coef)
            cand = (cur.double() + delta).float()
            F_new = F_of(cand)
            acc = (ok != 0) & (F_new < F)
            cur = torch.where(acc[:, None], cand, cur)
            F = torch.where(acc, F_new, F)
            damp = torch.where(acc, (damp / three).clamp_min(1e-9), (damp * 4.0).clamp_max(1e9))
            costs.append(F)
        return cur, torch.stack(costs), damp

    def now():
        out = []
        for fit_coef in (False, True):
            fitted, info = ops.landmark_fit(P0, lb, target, weight, ridge=ridge, center=center, iters=4, fit_coef=fit_coef)
            assert set(info) == {"cost", "damp", "accepted"}
            out += [fitted, info["cost"], info["damp"]]
        p = P.clone().requires_grad_(True)
        L = losses.landmark_loss(net, p, c["idx"], target, weight=weight)
        L.backward()
        return out + [L.detach(), p.grad]
    first = now()
    want = list(fit_before(False)) + list(fit_before(True))
    p = P.clone().requires_grad_(True)
    Lw = (ops.landmark_sse(p, lb, target, weight=weight, pose_grad=True) / weight.double().sum(dim=1).clamp_min(1.0)).mean()
    Lw.backward()
    want += [Lw.detach(), p.grad]
    cb = net.landmark_contour_basis(c["idx"][:60], c["idx"][60:].reshape(2, 4))
    ops.landmark_fit(P0, cb, target[:, :60], line_target=target[:, 60:62].contiguous(), iters=2)
    again = now()
    torch.cuda.synchronize()
    for i, (a, w, g) in enumerate(zip(first, want, again)):
        assert a.dtype == w.dtype and torch.equal(a, w) and torch.equal(a, g), i
    assert bool((first[1][-1] <= first[1][0]).all()) and bool((first[1][-1] < first[1][0]).any())      # (one face has f = 0 and stays)
