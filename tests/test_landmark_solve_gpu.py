"""GPU: the landmark solver (fr_landmark_solve_step; include/fr_hotpath.h, "landmark solver") against its numpy model
tests/ref_landmark_solve.py, then the Python surface (landmark_solve_step, landmark_fit, FaceRecNet.landmark_fit) and the example as a
program.

What is held bit for bit: ok, cost[:, 0] (F) and the failure rule in every call; and delta and cost[:, 1] wherever neither an angle nor
the coefficients are fitted -- there the kernel and the model run the same float64 chains, the same Cholesky and the same
substitutions, operation for operation.

Where bit equality is not attainable, and the bound that takes its place.  u = 2^-53.  Two things separate the kernel from the model:
  (a) the angle columns of J start from the device's double sincos, which may differ from numpy's in the last places: each within 2
      resp. 1 units in the last place of the exact value, so 6 u apart in relative terms; an entry of dR_a is a sum of products of at
      most three such factors formed in two 3-term dots (3 * 6 u + 6 u of roundings), and the entry of J adds the dot with v and the
      product with f (4 u more): |J_dev - J_model| <= 28 u Jabs, entry by entry, Jabs the same expression over absolute values
      (the model's `Jabs`; equal to |J| outside the angle columns, where the difference is 0).  With m_i = |W^1/2 J_i|_2 and
      rho_i = |W^1/2 Jabs_i|_2 / m_i:  |W^1/2 (J_dev - J_model)_i|_2 <= eta_i m_i,  eta_i = 28 u rho_i for an angle column, else 0.
  (b) the coefficient-coefficient block of J^T W J is summed on the float64 matrix cores, four rows per instruction with the
      hardware's own rounding inside, where the model adds term by term.  Any order of summing n = 2 K products, fused or not,
      stays within gamma = (2 K + 3) u of the exact sum relative to the sum of the absolute values of the terms, which Cauchy-Schwarz
      holds below m_i m_j; two such sums stand within 2 gamma m_i m_j of each other.
  Together, for every entry of M = J^T W J:  |M_dev - M_model|_ij <= (2 gamma + eta_i + eta_j) m_i m_j (first order).  A = M + diag(ridge)
  + damp diag(M) has A_ii >= m_i^2, so in the Jacobi scaling S = diag(sqrt(A_ii)), A^ = S^-1 A S^-1, y^ = S delta:
      |A^_dev - A^_model|_2 <= |.|_F <= E_A = 2 gamma P + 2 sqrt(P) |eta|_2.
  The residuals r carry no derivative of the rotation and are the same bits on both sides, so g differs through J alone:
      |S^-1 (g_dev - g_model)|_2 <= E_g = sqrt(sse) |eta + 2 gamma [eta > 0]|_2.
  The perturbation theorem of a linear system and the classical bound of a Cholesky solve, 8 P kappa_2 u |y^|_2 on each side, give
      |S (delta_dev - delta_model)|_2 <= T_d = 1.01 ( |A^-1|_2 (E_A |y^|_2 + E_g) / (1 - |A^-1|_2 E_A)  +  16 P kappa_2 u |y^|_2 ).
  The prediction c1 = F + sum_i delta_i (2 g_i + (H delta)_i) moves with delta through its gradient 2 g + 2 H delta, with H and g
  directly, and by the rounding of its own P (P + 4) operations on each side:
      |c1_dev - c1_model| <= T_c = 1.01 ( |S^-1 (2 g + 2 H delta)|_2 T_d + E_A |y^|_2^2 + 2 E_g |y^|_2
                                          + 2 (P + 4) u sum_i |delta_i| (2 |g_i| + (|H| |delta|)_i) + 2 u (|F| + |c1 - F|) ).
  Every quantity on the right is the model's; nothing is fitted to the device's output.  The test asserts |A^-1|_2 E_A <= 0.5 (the
  bound is informative) and prints the measured error over the bound and how many faces came out bit for bit."""
import ctypes
import json
import sys

import numpy as np
import pytest
import torch

from conftest import pkg
import ref_landmark as RL
import ref_landmark_solve as RS
import test_landmark_gpu as TG                # (_run: the example as a program)
import test_landmark_solve_cpu as TC          # (_fit_case: the example's batch and perturbed start)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U53 = 2.0 ** -53
IM = 200.0
SENT = 7.0


def _h():
    return pkg("_lib")


def _t(a, dtype=np.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype), device=DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits_equal(a, b):
    """float64 arrays equal by bit pattern, a NaN equal to a NaN whatever its sign (the default NaN differs by platform)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def c_step(c, P, target, weight=None, ridge=None, center=None, damp=None, mask=RS.ALL_POSE, coef=0, im=IM, ws=None):
    """the raw call: tensors in, (delta, cost, ok) prefilled with a sentinel"""
    h, L = _h(), _h().lib()
    B, K, ns, ne = int(P.shape[0]), c["K"], c["ns"], c["ne"]
    delta = torch.full((B, 7 + ns + ne), SENT, dtype=torch.float64, device=DEV)
    cost = torch.full((B, 2), SENT, dtype=torch.float64, device=DEV)
    ok = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    nws = L.fr_landmark_solve_workspace_bytes(B, ns, ne)
    if ws is None:
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
    else:
        assert ws.dtype == torch.uint8 and ws.numel() == nws, (ws.numel(), nws)     # (exactly the stated bytes)
    wb = 1 if weight is not None and weight.dim() == 2 else 0
    rc = L.fr_landmark_solve_step(h.ptr(P), h.ptr(c["img"]), c["img"].numel() * 4, h.ptr(target), h.ptr(weight), wb, h.ptr(ridge),
                                  h.ptr(center), h.ptr(damp), mask, coef, B, K, ns, ne, im, h.ptr(delta), h.ptr(cost), h.ptr(ok),
                                  h.ptr(ws) if coef else None, nws if coef else 0, _stream())
    assert rc == 0, rc
    return delta, cost, ok


# ---- the cases: inputs and the model's image, built once -----------------------------------------------------------------------------------
CASES = [("small", 1, 1), ("small", 3, 3), ("small", 65, 68), ("full", 3, 68), ("full", 2, 300), ("one", 3, 3)]
IDS = ["%s-B%d-K%d" % c for c in CASES]
_CASES = {}


def _case(kind, B, K):
    key = (kind, B, K)
    if key not in _CASES:
        synth = pkg("utils.synth")
        A = TG._assets(kind)
        rs = np.random.RandomState(300 + 7 * B + K)
        ns, ne = A["ndim_shape"], A["ndim_exp"]
        N = np.asarray(A["mu"]).size // 3
        idx = np.sort(rs.permutation(N)[:K]).astype(np.int64)        # distinct: the systems are to be well conditioned
        mu, pcs, pce = _t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"])
        img_np = RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], idx)
        mean, Um = RL.split_image(img_np, K, ns + ne)
        P = synth.sample_params_batch(B, im_size=200, n_shape=ns, n_exp=ne, seed=70 + B).astype(np.float32)
        P[:, 5] = rs.uniform(-1, 1, B)
        fw = RL.Forward(P, mean, Um)
        target = (fw.points[:, 0:2].transpose(0, 2, 1) + rs.uniform(-3, 3, (B, K, 2))).astype(np.float32)
        wBK = rs.uniform(0.25, 2.0, (B, K)).astype(np.float32)
        wK = rs.uniform(0.25, 2.0, K).astype(np.float32)
        nan_t = target.copy()
        zero_face = f0_face = bad_face = None
        if B >= 3:
            f0_face, zero_face, bad_face = B // 2, 0, B - 1
            P[f0_face, 6] = 0.0                                   # a face with f = 0
            wBK[zero_face] = 0.0                                  # a face whose weights are all 0 ...
            nan_t[zero_face] = np.nan                             # ... and whose targets are never read
        if K >= 8:   # (at K = 3 every landmark is needed: six rows for six pose columns)
            wBK[B - 1, K - 1] = 0.0                               # missing landmarks: weight 0 under a NaN target
            wK[0] = 0.0
            nan_t[B - 1, K - 1] = np.nan
        P_bad = P.copy()
        if bad_face is not None:
            P_bad[bad_face, 4] = np.inf                           # one non-finite parameter in one face
        ridge, center = synth.coefficient_prior(ns, ne, 0.5)
        damp = rs.choice([0.0, 1e-3, 0.1, 3.0], B)
        _CASES[key] = dict(kind=kind, A=A, N=N, K=K, B=B, ns=ns, ne=ne, idx=idx, mean=mean, Um=Um, P=P, P_bad=P_bad, target=target,
                           nan_t=nan_t, wBK=wBK, wK=wK, ridge=ridge, center=center, damp=damp, f0_face=f0_face, zero_face=zero_face,
                           bad_face=bad_face, img=TG.c_build(mu, pcs, pce, idx, N, ns, ne))
    return _CASES[key]


def _modes(c):
    if c["K"] == 1:
        return [("tx ty", RS.pose_mask(["tx", "ty"]), 0)]
    return [("pose", RS.ALL_POSE, 0), ("tx ty f", RS.pose_mask(["tx", "ty", "f"]), 0), ("coefficients", 0, 1), ("both", RS.ALL_POSE, 1)]


def _weights(c):
    """(name, weight, target): the [K] weight has a zero under a NaN target only where the [B,K] one has too, so each gets its own"""
    tK = c["target"].copy()
    if c["wK"][0] == 0:
        tK[:, 0] = np.nan
    return [("NULL", None, c["target"]), ("[K]", c["wK"], tK), ("[B,K]", c["wBK"], c["nan_t"])]


def _tolerances(st, b, K):
    """T_d, T_c of the docstring for face b of the model's step"""
    A, H, g, x, P = st.A[b], st.H[b], st.g[b], st.x[b], st.Pn
    s = np.sqrt(np.diag(A))
    Ah = A / s[:, None] / s[None, :]
    sv = np.linalg.svd(Ah, compute_uv=False)
    inv, kappa = 1.0 / sv[-1], sv[0] / sv[-1]
    w = st.wrow[b][:, None]
    m = np.sqrt((w * st.J[b] ** 2).sum(axis=0))
    mabs = np.sqrt((w * st.Jabs[b] ** 2).sum(axis=0))
    angle = np.array([i < st.n_pose and st.slots[i] < 3 for i in range(P)])
    eta = np.where(angle, 28 * U53 * mabs / np.where(m > 0, m, 1.0), 0.0)
    gamma = (2 * K + 3) * U53
    E_A = 2 * gamma * P + 2 * np.sqrt(P) * np.linalg.norm(eta)
    E_g = np.sqrt(max(st.fw.sse[b], 0.0)) * np.linalg.norm(eta + 2 * gamma * (eta > 0))
    y = s * x
    ny = np.linalg.norm(y)
    assert inv * E_A <= 0.5, (b, inv, E_A)
    T_d = 1.01 * (inv * (E_A * ny + E_g) / (1 - inv * E_A) + 16 * P * kappa * U53 * ny)
    grad = (2 * g + 2 * H @ x) / s
    terms = (np.abs(x) * (2 * np.abs(g) + np.abs(H) @ np.abs(x))).sum()
    T_c = 1.01 * (np.linalg.norm(grad) * T_d + E_A * ny * ny + 2 * E_g * ny + 2 * (P + 4) * U53 * terms
                  + 2 * U53 * (abs(st.F[b]) + abs(st.pred[b] - st.F[b])))
    return s, T_d, T_c


def _check(c, name, st, delta, cost, ok, exact):
    """device outputs (numpy) against the model's step `st`; -> (worst error / bound, faces bit for bit, faces compared)"""
    B = delta.shape[0]
    assert not (delta == SENT).any() and not (cost == SENT).any() and not (ok == 7).any(), name      # every element written
    assert np.array_equal(ok, st.ok), (name, ok.tolist(), st.ok.tolist())
    assert _bits_equal(cost[:, 0], st.cost[:, 0]).all(), (name, cost[:, 0], st.cost[:, 0])
    worst, same, n = 0.0, 0, 0
    for b in range(B):
        if not st.ok[b]:
            assert not delta[b].any() and not np.signbit(delta[b]).any(), (name, b)
            assert _bits_equal(cost[b, 1], cost[b, 0]).all(), (name, b)
            continue
        n += 1
        unfit = np.setdiff1d(np.arange(delta.shape[1]), st.cols)
        assert not delta[b, unfit].any() and not np.signbit(delta[b, unfit]).any(), (name, b)
        bit = bool(_bits_equal(delta[b], st.delta[b]).all() and _bits_equal(cost[b, 1], st.cost[b, 1]).all())
        same += bit
        if exact:
            assert bit, (name, b, delta[b, st.cols], st.delta[b, st.cols], cost[b], st.cost[b])
            continue
        s, T_d, T_c = _tolerances(st, b, c["K"])
        e_d = np.linalg.norm(s * (delta[b, st.cols] - st.x[b]))
        e_c = abs(cost[b, 1] - st.cost[b, 1])
        worst = max(worst, e_d / T_d if T_d > 0 else 0.0, e_c / T_c if T_c > 0 else 0.0)
        assert e_d <= T_d, (name, b, e_d, T_d)
        assert e_c <= T_c, (name, b, e_c, T_c)
    return worst, same, n


@pytest.mark.parametrize("kind,B,K", CASES, ids=IDS)
def test_step_against_the_model(kind, B, K):
    c = _case(kind, B, K)
    rg, ce = _t(c["ridge"]), _t(c["center"])
    for mname, mask, coef in _modes(c):
        exact = not coef and not (mask & 7)
        for wname, weight, target in _weights(c):
            for dname, damp in (("NULL", None), ("per face", c["damp"])):
                for pname, P in (("", c["P"]),) + ((("non-finite", c["P_bad"]),) if mname == "both" and wname == "[B,K]" else ()):
                    name = "%s, weight %s, damp %s %s" % (mname, wname, dname, pname)
                    kw = dict(ridge=c["ridge"], center=c["center"]) if coef else {}
                    st = RS.Step(P, c["mean"], c["Um"], target, weight=weight, damp=damp, pose_mask=mask, fit_coef=coef, **kw)
                    got = c_step(c, _t(P), _t(target), _t(weight), rg if coef else None, ce if coef else None,
                                 _t(damp, np.float64), mask, coef)
                    torch.cuda.synchronize()
                    delta, cost, ok = (t.cpu().numpy() for t in got)
                    worst, same, n = _check(c, name, st, delta, cost, ok, exact)
                    print("%s: ok %d of %d faces, bit for bit %d of %d, worst error / bound %.3g" % (name, int(st.ok.sum()), B, same, n, worst))
                    if B >= 3:   # the failure cases report exactly the stated values (checked above); which faces they are:
                        if mask & 7:
                            assert not st.ok[c["f0_face"]], name                   # f = 0 with an angle fitted
                        if wname == "[B,K]" and mask:
                            assert not st.ok[c["zero_face"]], name                 # all weights 0 with a pose column fitted
                        if pname:
                            assert not st.ok[c["bad_face"]], name                  # a non-finite parameter that is read
                        assert st.ok.sum() >= B - 3, (name, st.ok)


@pytest.mark.parametrize("kind,B,K", [cs for cs in CASES if cs[1] >= 3], ids=[i for i, cs in zip(IDS, CASES) if cs[1] >= 3])
def test_failures_leave_their_neighbours_alone(kind, B, K):
    """the faces beside a failing face, bit for bit what the same face gives alone with B = 1 -- which also shows that a face's
    outputs do not depend on the batch or its place in it -- and twice the same bits"""
    c = _case(kind, B, K)
    P, target, weight, damp = c["P_bad"], c["nan_t"], c["wBK"], c["damp"]
    rg, ce = _t(c["ridge"]), _t(c["center"])
    for mask, coef in ((RS.ALL_POSE, 0), (RS.ALL_POSE, 1)):
        args = lambda sl: (_t(P[sl]), _t(target[sl]), _t(weight[sl]), rg if coef else None, ce if coef else None,   # noqa: E731
                           _t(damp[sl], np.float64), mask, coef)
        a = [t.cpu().numpy() for t in c_step(c, *args(slice(None)))]
        a2 = [t.cpu().numpy() for t in c_step(c, *args(slice(None)))]
        for x, y in zip(a, a2):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))         # reproducible
        failed = [b for b in range(B) if not a[2][b]]
        assert set(failed) >= {c["f0_face"], c["zero_face"], c["bad_face"]}
        near = sorted({b + d for b in failed for d in (-1, 1) if 0 <= b + d < B and a[2][b + d]})
        assert near or B == 3
        for b in near + failed:
            one = [t.cpu().numpy() for t in c_step(c, *args(slice(b, b + 1)))]
            assert _bits_equal(one[0][0], a[0][b]).all() and _bits_equal(one[1][0], a[1][b]).all() and one[2][0] == a[2][b], b


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------------
def _lbasis(c):
    ops = pkg("rendering_layer.ops")
    A = c["A"]
    return ops.landmark_basis(_t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"]), c["idx"])


def test_landmark_solve_step_is_the_raw_call():
    ops = pkg("rendering_layer.ops")
    c = _case("full", 3, 68)
    lb = _lbasis(c)
    P, target, wBK, damp = _t(c["P"]), _t(c["nan_t"]), _t(c["wBK"]), _t(c["damp"], np.float64)
    rg, ce = _t(c["ridge"]), _t(c["center"])
    for fit_pose, mask, coef, kw in ((True, RS.ALL_POSE, 0, {}), (("tx", "f"), RS.pose_mask(["tx", "f"]), 0, {}),
                                     (False, 0, 1, dict(ridge=rg, center=ce)), (True, RS.ALL_POSE, 1, dict(ridge=rg, center=ce))):
        got = ops.landmark_solve_step(P.clone().requires_grad_(True), lb, target, weight=wBK, damp=damp, fit_pose=fit_pose,
                                      fit_coef=bool(coef), **kw)
        raw = c_step(c, P, target, wBK, kw.get("ridge"), kw.get("center"), damp, mask, coef)
        assert got[0].dtype == torch.float64 and got[2].dtype == torch.int32 and not got[0].requires_grad
        for x, y in zip(got, raw):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), (fit_pose, coef)
    # defaults: the six pose columns, no coefficients, no damping, im_size 200
    d0 = ops.landmark_solve_step(P, lb, target, weight=wBK)
    r0 = c_step(c, P, target, wBK)
    assert torch.equal(d0[0], r0[0]) and torch.equal(d0[2], r0[2])


def test_value_errors():
    ops = pkg("rendering_layer.ops")
    c = _case("small", 3, 3)
    lb = _lbasis(c)
    P, target = _t(c["P"]), _t(c["target"])
    Kt = c["ns"] + c["ne"]
    for fn in (ops.landmark_solve_step, ops.landmark_fit):
        for bad in (dict(fit_pose=("tz",)), dict(fit_pose=("yaw",)), dict(fit_pose=False), dict(fit_pose=(), fit_coef=False),
                    dict(weight=torch.ones(4, device=DEV)), dict(ridge=torch.ones(Kt + 1, device=DEV), fit_coef=True),
                    dict(center=torch.ones(Kt - 1, device=DEV), fit_coef=True)):
            with pytest.raises(ValueError):
                fn(P, lb, target, **bad)
        with pytest.raises(ValueError):
            fn(P[:, :-1], lb, target)
        with pytest.raises(ValueError):
            fn(P, lb, target[:, :2])
        with pytest.raises(ValueError):
            fn(P, lb, None)
        with pytest.raises(ValueError):
            fn(P, lb, target.clone().requires_grad_(True))
    for bad in (torch.ones(3, device=DEV), torch.ones(2, dtype=torch.float64, device=DEV), [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError):
            ops.landmark_solve_step(P, lb, target, damp=bad)
    with pytest.raises(ValueError):
        ops.landmark_fit(P, lb, target, iters=-1)
    with pytest.raises(ValueError):
        ops.landmark_fit(P, lb, target, damp0=-1.0)


def test_landmark_fit_pose(small_assets, synth):
    """the CPU test's pose-only condition on the device, decision for decision the model's loop, and FaceRecNet's method"""
    ops = pkg("rendering_layer.ops")
    c = TC._fit_case(small_assets, synth, 4)
    S = c["S"]
    idx = synth.landmark_ids(small_assets, 68)
    target32 = c["target64"].astype(np.float32)
    P0 = np.concatenate([c["pose0"].numpy(), c["P32"][:, 7:]], axis=1).astype(np.float32)
    lb = ops.landmark_basis(_t(np.asarray(small_assets["mu"]).reshape(-1)), _t(small_assets["pc_shape"]), _t(small_assets["pc_exp"]), idx)
    fitted, info = ops.landmark_fit(_t(P0), lb, _t(target32), iters=6, im_size=S)
    torch.cuda.synchronize()
    cost, acc = info["cost"].cpu().numpy(), info["accepted"].cpu().numpy()
    assert cost.shape == (7, 3) and acc.shape == (6, 3) and acc.dtype == bool and tuple(info["damp"].shape) == (3,)
    fit_np = fitted.cpu().numpy()
    t3d = float(np.sqrt(np.mean((fit_np[:, 3:6].astype(np.float64) - c["P32"][:, 3:6]) ** 2)))
    print("landmark_fit, pose only: F", " -> ".join("%.3g" % v for v in cost.sum(axis=1)), "; accepted", acc.sum(axis=1).tolist(),
          "; t3d_rms %.3g px" % t3d)
    assert np.isfinite(cost).all() and (np.diff(cost, axis=0) <= 0).all()
    assert (cost[-1] <= 1e-8 * cost[0]).all(), cost[-1] / cost[0]
    assert t3d <= 1e-3
    assert fitted.dtype == torch.float32 and np.array_equal(fit_np[:, 5], P0[:, 5]) and np.array_equal(fit_np[:, 7:], P0[:, 7:])
    want, winfo = RS.fit(P0, c["mean"], c["U"], target32, iters=6, im_size=float(S))
    assert np.array_equal(acc, winfo["accepted"])
    assert np.array_equal(info["damp"].cpu().numpy(), winfo["damp"])
    # FaceRecNet.landmark_fit: the same tensor, by ids and by the image
    face = pkg("nets.network").FaceRecNet(mesh_data=small_assets, batch_size=3, im_size=S, device=DEV)
    for which in (idx, face.landmark_basis(idx)):
        f2, i2 = face.landmark_fit(_t(P0)[:, None, None, :], which, _t(target32), iters=6)
        assert torch.equal(f2.view(torch.int32), fitted.view(torch.int32)) and torch.equal(i2["cost"], info["cost"])
    # iters = 0: the parameters as they came, one cost row
    f0, i0 = ops.landmark_fit(_t(P0), lb, _t(target32), iters=0, im_size=S)
    assert torch.equal(f0, _t(P0)) and tuple(i0["cost"].shape) == (1, 3) and tuple(i0["accepted"].shape) == (0, 3)


def test_landmark_fit_coefficients(small_assets, synth):
    """pose and coefficients under the sampler's prior, the CPU test's case: the device's loop takes the model's decisions"""
    ops = pkg("rendering_layer.ops")
    c = TC._fit_case(small_assets, synth, 1)
    S = c["S"]
    idx = synth.landmark_ids(small_assets, 68)
    rs = np.random.RandomState(3)
    target = (c["target64"] + 0.5 * rs.standard_normal(c["target64"].shape)).astype(np.float32)
    ridge, center = synth.coefficient_prior(c["ns"], c["ne"], 0.5)
    P0 = np.concatenate([c["pose0"].numpy(), np.broadcast_to(center, (c["B"], center.size))], axis=1).astype(np.float32)
    lb = ops.landmark_basis(_t(np.asarray(small_assets["mu"]).reshape(-1)), _t(small_assets["pc_shape"]), _t(small_assets["pc_exp"]), idx)
    fitted, info = ops.landmark_fit(_t(P0), lb, _t(target), ridge=_t(ridge), center=_t(center), iters=3, fit_coef=True, im_size=S)
    torch.cuda.synchronize()
    cost, acc = info["cost"].cpu().numpy(), info["accepted"].cpu().numpy()
    want, winfo = RS.fit(P0, c["mean"], c["U"], target, ridge=ridge, center=center, iters=3, fit_coef=True, im_size=float(S))
    print("landmark_fit, pose and coefficients: F", " -> ".join("%.6g" % v for v in cost.sum(axis=1)), "; model",
          " -> ".join("%.6g" % v for v in winfo["cost"].sum(axis=1)))
    assert np.isfinite(cost).all() and (np.diff(cost, axis=0) <= 0).all() and (cost[-1] < 0.5 * cost[0]).all()
    assert np.array_equal(acc, winfo["accepted"]) and acc[0].all()


# ---- the example as a program ----------------------------------------------------------------------------------------------------------------------
def test_photo_fit_landmark_init_program():
    base = [sys.executable, "examples/photo_fit.py", "--small", "--fit-pose", "--landmarks", "68", "--landmarks-only", "--pose-noise", "4"]
    d = TG._run(base + ["--landmark-init", "6", "--steps", "0"])
    print(json.dumps(d))
    init = d["landmark_init"]
    assert d["steps"] == 0 and init["iters"] == 6 and d["finite"] is True
    vals = [d["last"], init["cost_first"], init["cost_last"]] + list(d["errors_before"].values()) + list(d["errors_after"].values())
    assert np.isfinite(vals).all() and np.isfinite([v for k, v in init.items()]).all()
    assert d["errors_after"]["t3d_rms"] < d["errors_before"]["t3d_rms"]
    assert d["errors_after"]["t3d_rms"] == init["t3d_rms"] and init["cost_last"] < init["cost_first"]
    adam = TG._run(base + ["--steps", "100"])
    print(json.dumps(adam))
    assert adam["landmark_init"] is None and adam["errors_before"] == d["errors_before"]
    assert d["errors_after"]["t3d_rms"] < adam["errors_after"]["t3d_rms"]
