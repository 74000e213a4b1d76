"""CPU: the landmark term (include/fr_hotpath.h, "landmarks") without a GPU -- the binding rows, every return code of the header's
checks (all before any HIP call), the numpy model (tests/ref_landmark.py) against central differences of its own float64 forward and
against the oracle's dense decode, the id helpers, and the convergence pre-check of the --landmarks-only fit that
tests/test_landmark_gpu.py runs as a program."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
import ref_landmark as RL
import ref_synth_batch as RS

ROWS = {"fr_landmark_basis_bytes": "z:iii",
        "fr_landmark_basis_build": "i:ppppiiiipzp",
        "fr_landmark_forward": "i:ppzpppiiiiifppp",
        "fr_landmark_backward": "i:ppppzpppiiiiifppip"}
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -4


def test_names_and_rows():
    host = pkg("_lib")
    for name, row in ROWS.items():
        assert name in host.EXPORTS and host.SIGNATURES[name] == row, name
    assert "fr_landmark.hip" in host.SOURCES
    src = open(os.path.join(ROOT, "include", "fr_hotpath.h")).read()
    assert "---- landmarks ----" in src
    L = host.lib()
    assert L.fr_landmark_basis_bytes(68, 199, 29) == 4 * 3 * 68 * (2 * 228 + 1)
    assert L.fr_landmark_basis_bytes(1, 0, 0) == 12 and L.fr_landmark_basis_bytes(1024, 256, 0) == 4 * 3072 * 513
    for bad in ((0, 9, 5), (1025, 9, 5), (5, 200, 57), (5, -1, 5), (-1, 9, 5)):
        assert L.fr_landmark_basis_bytes(*bad) == 0, bad


# ---- return codes: made-up non-NULL pointers; every case returns before any HIP call -------------------------------------------------------
def test_return_codes():
    if torch.cuda.is_available():
        pytest.skip("host-code check: never run where a case that slipped through validation could launch")
    L = pkg("_lib").lib()
    p, q, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), None   # q: not 16-byte aligned
    K, ns, ne, B = 5, 9, 5, 3
    nb = L.fr_landmark_basis_bytes(K, ns, ne)
    assert nb == 4 * 15 * 29

    def build(mu=p, pcs=p, pce=p, idx=p, N=100, ns=ns, ne=ne, K=K, lb=p, nbytes=nb):
        return L.fr_landmark_basis_build(mu, pcs, pce, idx, N, ns, ne, K, lb, nbytes, nul)
    assert build(N=-1) == INVALID and build(ns=-1) == INVALID and build(ne=-1) == INVALID and build(K=-1) == INVALID
    assert build(K=0) == OK and build(K=0, idx=nul, lb=nul) == OK
    assert build(idx=nul) == INVALID and build(mu=nul) == INVALID and build(pcs=nul) == INVALID and build(pce=nul) == INVALID
    assert build(pcs=nul, ns=0, lb=nul) == WORKSPACE and build(mu=nul, pcs=nul, pce=nul, N=0, lb=nul) == WORKSPACE   # (not read)
    assert build(K=1025) == UNSUPPORTED and build(ns=200, ne=57) == UNSUPPORTED
    assert build(lb=nul) == WORKSPACE and build(lb=q) == WORKSPACE and build(nbytes=nb - 1) == WORKSPACE
    assert build(K=-1, idx=nul) == INVALID and build(idx=nul, K=1025) == INVALID and build(K=1025, lb=nul) == UNSUPPORTED

    def fwd(params=p, lb=p, nbytes=nb, R=nul, target=p, weight=nul, wb=0, B=B, K=K, ns=ns, ne=ne, points=p, sse=p):
        return L.fr_landmark_forward(params, lb, nbytes, R, target, weight, wb, B, K, ns, ne, 200.0, points, sse, nul)
    assert fwd(B=-1) == INVALID and fwd(K=-1) == INVALID and fwd(ns=-1) == INVALID and fwd(ne=-1) == INVALID
    assert fwd(wb=2) == INVALID and fwd(wb=-1) == INVALID
    assert fwd(B=0) == OK and fwd(K=0) == OK and fwd(B=0, params=nul, points=nul) == OK
    assert fwd(params=nul) == INVALID and fwd(points=nul) == INVALID and fwd(sse=nul) == INVALID
    assert fwd(K=1025) == UNSUPPORTED and fwd(ns=256, ne=1) == UNSUPPORTED
    assert fwd(lb=nul) == WORKSPACE and fwd(lb=q) == WORKSPACE and fwd(nbytes=nb - 1) == WORKSPACE
    assert fwd(B=-1, params=nul) == INVALID and fwd(params=nul, K=1025) == INVALID and fwd(K=1025, lb=nul) == UNSUPPORTED

    def bwd(gp=p, gs=p, params=p, lb=p, nbytes=nb, R=nul, target=p, weight=nul, wb=0, B=B, K=K, ns=ns, ne=ne, gpar=p, gR=nul, pg=0):
        return L.fr_landmark_backward(gp, gs, params, lb, nbytes, R, target, weight, wb, B, K, ns, ne, 200.0, gpar, gR, pg, nul)
    assert bwd(B=-1) == INVALID and bwd(K=-1) == INVALID and bwd(ns=-1) == INVALID and bwd(ne=-1) == INVALID
    assert bwd(wb=2) == INVALID and bwd(pg=2) == INVALID and bwd(pg=-1) == INVALID
    assert bwd(B=0) == OK and bwd(K=0) == OK and bwd(B=0, gp=nul, gs=nul, gpar=nul) == OK
    assert bwd(params=nul) == INVALID and bwd(gpar=nul) == INVALID and bwd(gp=nul, gs=nul) == INVALID
    assert bwd(target=nul) == INVALID                    # grad_sse needs the target
    assert bwd(R=p, pg=1, gR=nul) == INVALID             # grad_R is required under an override with pose_grad
    assert bwd(K=1025) == UNSUPPORTED and bwd(ns=1, ne=256) == UNSUPPORTED
    assert bwd(lb=nul) == WORKSPACE and bwd(lb=q) == WORKSPACE and bwd(nbytes=nb - 1) == WORKSPACE
    assert bwd(pg=2, params=nul) == INVALID and bwd(gpar=nul, K=1025) == INVALID and bwd(K=1025, nbytes=0) == UNSUPPORTED


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
B_, K_ = 3, 5


def _case(small_assets, seed=5):
    rs = np.random.RandomState(seed)
    A = small_assets
    N = np.asarray(A["mu"]).size // 3
    idx = np.array([0, N - 1, 17, 17, N // 2])
    ns, ne = A["ndim_shape"], A["ndim_exp"]
    img = RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], idx)
    mean, U = RL.split_image(img, K_, ns + ne)
    P = pkg("utils.synth").sample_params_batch(B_, im_size=200, n_shape=ns, n_exp=ne, seed=11).astype(np.float32)
    fw = RL.Forward(P, mean, U)
    target = (fw.points[:, 0:2].transpose(0, 2, 1) + rs.uniform(-2, 2, (B_, K_, 2))).astype(np.float32)
    weight = rs.uniform(0.5, 2.0, (B_, K_)).astype(np.float32)
    weight[1, 2] = 0.0
    gpts = rs.standard_normal((B_, 3, K_)).astype(np.float32)
    gsse = rs.uniform(0.5, 1.5, B_) * np.array([1.0, -1.0, 1.0])
    return dict(A=A, idx=idx, mean=mean, U=U, P=P, target=target, weight=weight, gpts=gpts, gsse=gsse, ns=ns, ne=ne, rs=rs)


def test_basis_image_is_the_gather(small_assets):
    c = _case(small_assets)
    A, idx = c["A"], c["idx"]
    N = np.asarray(A["mu"]).size // 3
    mu = np.asarray(A["mu"], np.float32).reshape(-1)
    for k, i in enumerate(idx):
        for cc in range(3):
            assert c["mean"][k, cc] == mu[cc * N + i]
            assert np.array_equal(c["U"][k, cc, :c["ns"]], np.asarray(A["pc_shape"], np.float32)[cc * N + i])
            assert np.array_equal(c["U"][k, cc, c["ns"]:], np.asarray(A["pc_exp"], np.float32)[cc * N + i])
    img = RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], [3, N, -1])
    mean, U = RL.split_image(img, 3, c["ns"] + c["ne"])
    assert not mean[1:].any() and not U[1:].any() and U[0].any() and not np.signbit(img).all()


def test_model_gradient_against_central_differences(small_assets):
    """L = sum g . xyz + sum_b gs_b sse_b as a float64 function of float64 parameters (RL.forward_f64) against the model's gradient
    (exact=True: the rotation not rounded to fp32), on the directional derivative of every parameter group.

    The step and the bound.  phi(s) = L(P + s d); the central difference (phi(h) - phi(-h)) / 2h misses phi'(0) by at most
    h^2 / 6 max|phi'''| + E / h, with E the rounding error of one evaluation of L.
      * E <= n 2^-53 Mabs with Mabs the sum of the absolute values of L's terms (RL.Forward.absterms and the squared distances over
        absolute values) and n = Kt + 16 the longest chain of rounded operations behind a term.
      * phi''' = 0 for a direction inside t3d, f, the shape or the expression coefficients or R: xyz is linear in each of these
        groups, so L is a quadratic along the line.  Along the angles (|d|_1 = 1): every entry of every mixed derivative of
        R_pitch R_yaw R_roll is a sum of at most 4 products of sines and cosines, so the k-th derivative of a coordinate along d is at
        most X = 4 |f| sum_c |v_c|, and |phi'''| <= sum |g| X + sum_b |gs_b| sum_k w_k 2 (6 X^2 + 2 |x - tx| X) =: M3.
      * h = 2^-17 balances the two for M3 of the order of Mabs: (2^-34 / 6) M3 against (Kt + 16) 2^-36 Mabs.
    Nothing is fitted; the measured agreement is printed.  A direction's derivative must stand at least 100 bounds tall, or the
    comparison would show nothing."""
    c = _case(small_assets)
    mean, U, P = c["mean"], c["U"], c["P"]
    Kt = c["ns"] + c["ne"]
    rs = c["rs"]
    t64 = c["target"].astype(np.float64)
    w64 = c["weight"].astype(np.float64)
    g64 = c["gpts"].astype(np.float64).transpose(0, 2, 1)
    h = 2.0 ** -17
    for override in (False, True):
        R32 = RL.rotation32(rs.uniform(-1, 1, (B_, 3)).astype(np.float32)) if override else None
        fw = RL.Forward(P, mean, U, R=R32, target=c["target"], weight=c["weight"], exact=True)
        bw = RL.Backward(fw, U, grad_points=c["gpts"], grad_sse=c["gsse"], pose_grad=True)
        assert fw.sse is not None and (fw.sse > 0).all()

        def loss(P64, R64):
            xyz = RL.forward_f64(P64, mean, U, R64)
            d2 = (xyz[:, :, 0] - t64[:, :, 0]) ** 2 + (xyz[:, :, 1] - t64[:, :, 1]) ** 2
            return float((g64 * xyz).sum() + (c["gsse"] * (w64 * d2).sum(axis=1)).sum())
        dist = np.abs(fw.xyz[:, :, 0:2]) + np.abs(t64)
        Mabs = (np.abs(c["gpts"]) * fw.absterms).sum() + (np.abs(c["gsse"]) * (w64 * (dist ** 2).sum(axis=2)).sum(axis=1)).sum()
        X = 4 * np.abs(fw.f)[:, None] * np.abs(fw.v).sum(axis=2)                   # [B,K]
        dev = np.abs(fw.xyz[:, :, 0:2] - t64)
        M3 = (np.abs(g64).sum(axis=2) * X).sum() + (np.abs(c["gsse"]) * (w64 * (2 * (6 * X * X)[:, :, None]
                                                                                 + 2 * dev * X[:, :, None]).sum(axis=2)).sum(axis=1)).sum()
        P64 = P.astype(np.float64)
        R64 = None if R32 is None else R32.astype(np.float64)
        groups = [("t3d", slice(3, 6), 1.0), ("f", slice(6, 7), float(np.abs(P64[:, 6]).max())), ("shape", slice(7, 7 + c["ns"]), 1e3),
                  ("expression", slice(7 + c["ns"], 7 + Kt), 0.3)]
        groups.append(("R", None, 1.0) if override else ("angles", slice(0, 3), 1.0))
        for name, cols, scale in groups:
            dP, dR = np.zeros_like(P64), None
            if cols is None:
                dR = rs.uniform(-1, 1, (B_, 3, 3))
                want = float((bw.G64 * dR).sum())
            else:
                d = rs.uniform(-1, 1, dP[:, cols].shape)
                if name == "angles":
                    d = d / np.abs(d).sum(axis=1, keepdims=True)
                dP[:, cols] = d * scale
                want = float((bw.params64 * dP).sum())
            up = loss(P64 + h * dP, None if R64 is None else R64 + (0 if dR is None else h * dR))
            dn = loss(P64 - h * dP, None if R64 is None else R64 - (0 if dR is None else h * dR))
            num = (up - dn) / (2 * h)
            bound = 1.01 * ((h * h / 6) * (M3 if name == "angles" else 0.0) + (Kt + 16) * 2.0 ** -53 * Mabs / h)
            print("%s%s: model %.9g, central difference %.9g, |difference| %.3g, bound %.3g" % (
                name, " (override)" if override else "", want, num, abs(num - want), bound))
            assert abs(want) >= 100 * bound, (name, want, bound)
            assert abs(num - want) <= bound, (name, num, want, bound)
        if override:
            assert not bw.params64[:, 0:3].any() and bw.grad_R is not None
        else:
            assert bw.params64[:, 0:3].all() and bw.grad_R is None
    # pose_grad off: the angle columns are +0 and no grad_R exists
    off = RL.Backward(RL.Forward(P, mean, U, target=c["target"]), U, grad_sse=c["gsse"])
    assert not off.grad_params[:, 0:3].any() and not np.signbit(off.grad_params[:, 0:3]).any() and off.grad_R is None


def test_model_forward_against_the_dense_decode(small_assets, oracle):
    """the model's points against the oracle's fp32 dense decode at idx: within (n_shape + n_exp + 8) 2^-24 A per coordinate, A the
    sum of the absolute values of that coordinate's terms -- the a-priori bound of any fp32 chain of that length"""
    c = _case(small_assets)
    A = c["A"]
    for R in (None, RL.rotation32(np.array([[0.3, -0.2, 0.1]] * B_, np.float32))):
        fw = RL.Forward(c["P"], c["mean"], c["U"], R=R)
        dense = oracle.decode_3dmm(c["P"], A["mu"], A["pc_shape"], A["pc_exp"], 200.0, R=R)[:, :, c["idx"]]
        bound = (c["ns"] + c["ne"] + 8) * RL.U24 * fw.absterms
        ratio = np.abs(fw.points.astype(np.float64) - dense) / bound
        print("model against the dense decode: max |difference| / bound = %.3g" % ratio.max())
        assert (ratio <= 1.0).all()
    # the model's rotation is the oracle's, bit for bit (the same float64 chain rounded once)
    assert np.array_equal(RL.rotation32(c["P"][:, 0:3]).view(np.uint32), oracle.rotation_matrix_batch(c["P"][:, 0:3]).view(np.uint32))


def test_sse_skips_weight_zero_and_matches_the_plain_formula(small_assets):
    c = _case(small_assets)
    target = c["target"].copy()
    target[1, 2] = np.nan                      # weight[1, 2] == 0: a missing landmark
    fw = RL.Forward(c["P"], c["mean"], c["U"], target=target, weight=c["weight"])
    ref = RL.Forward(c["P"], c["mean"], c["U"], target=c["target"], weight=c["weight"])
    assert np.isfinite(fw.sse).all() and np.array_equal(fw.sse, ref.sse)
    d2 = ((ref.xyz[:, :, 0:2] - c["target"].astype(np.float64)) ** 2).sum(axis=2)
    assert np.allclose(ref.sse, (c["weight"] * d2).sum(axis=1), rtol=1e-13)
    bw = RL.Backward(fw, c["U"], grad_sse=c["gsse"], pose_grad=True)
    assert np.isfinite(bw.grad_params).all()
    assert np.array_equal(RL.Forward(c["P"], c["mean"], c["U"], target=c["target"], weight=c["weight"][0]).sse[0], ref.sse[0])


# ---- the id helpers ----------------------------------------------------------------------------------------------------------------------------
def test_landmark_ids_are_deterministic_and_distinct(small_assets, synth):
    N = np.asarray(small_assets["mu"]).size // 3
    a, b = synth.landmark_ids(small_assets), synth.landmark_ids(small_assets)
    assert a.shape == (68,) and np.array_equal(a, b) and len(set(a.tolist())) == 68
    assert a.min() >= 0 and a.max() < N and (np.diff(a) > 0).all()
    assert not np.array_equal(a, synth.landmark_ids(small_assets, seed=1))
    assert len(set(synth.landmark_ids(small_assets, K=N).tolist())) == N and synth.landmark_ids(small_assets, K=1).shape == (1,)
    with pytest.raises(ValueError):
        synth.landmark_ids(small_assets, K=N + 1)
    with pytest.raises(ValueError):
        synth.landmark_ids(small_assets, K=0)


def test_read_keypoints_round_trip(small_assets, tmp_path):
    import scipy.io as sio
    parser = pkg("utils.parser_3dmm")
    d = str(tmp_path / "model")
    parser.write_3dmm_model(d, small_assets)
    assert parser.read_keypoints(d) is None
    before = parser.read_3dmm_model(d)
    shapefile = os.path.join(d, "Model_Shape.mat")
    data = {k: v for k, v in sio.loadmat(shapefile).items() if not k.startswith("__")}
    kp = np.array([[5, 1, 480, 17, 17]], np.float64)          # MATLAB: a 1 x K row of 1-based ids
    data["keypoints"] = kp
    sio.savemat(shapefile, data, do_compression=True)
    got = parser.read_keypoints(d)
    assert got.dtype == np.int64 and got.tolist() == [4, 0, 479, 16, 16]
    assert parser.read_keypoints(d, base=0).tolist() == [5, 1, 480, 17, 17]
    after = parser.read_3dmm_model(d)
    assert sorted(after) == sorted(before) and "keypoints" not in after
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k


# ---- the convergence pre-check of the --landmarks-only fit -------------------------------------------------------------------------------------
def _photo_fit():
    spec = importlib.util.spec_from_file_location("photo_fit_example", os.path.join(ROOT, "examples", "photo_fit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _torch_points(P, mean, U, im_size):
    """the model's forward in float64 under torch autograd (the rotation of the angles exact) -> x, y [B,K,2]"""
    s, co = torch.sin(P[:, 0:3]), torch.cos(P[:, 0:3])
    o, z = torch.ones_like(s[:, 0]), torch.zeros_like(s[:, 0])

    def m(*e):
        return torch.stack(e, dim=1).reshape(-1, 3, 3)
    Rp = m(o, z, z, z, co[:, 0], s[:, 0], z, -s[:, 0], co[:, 0])
    Ry = m(co[:, 1], z, -s[:, 1], z, o, z, s[:, 1], z, co[:, 1])
    Rr = m(co[:, 2], s[:, 2], z, -s[:, 2], co[:, 2], z, z, z, o)
    R = Rp @ Ry @ Rr
    v = mean[None] + torch.einsum("bj,kcj->bkc", P[:, 7:], U)
    q = P[:, 6, None, None] * torch.einsum("bic,bkc->bki", R, v) + P[:, None, 3:6]
    return torch.stack([q[:, :, 0], (im_size - q[:, :, 1]) - 1.0], dim=2)


def test_landmarks_only_fit_converges_in_the_model(small_assets, synth):
    """`photo_fit.py --small --fit-pose --landmarks-only --landmarks 68` with the float64 model under torch-CPU autograd in the
    kernels' place: the same batch (tests/ref_synth_batch.py is the sampler, bit for bit), the same perturbation (the example's own
    generator and draw order), the same optimiser and steps (the example's own loop).  It must meet the program test's condition:
    finite, last < first, t3d_rms after below before."""
    ex = _photo_fit()
    args = ex.build_parser().parse_args(["--small", "--fit-pose", "--landmarks-only", "--landmarks", "68"])
    B, S = 3, 32
    A = small_assets
    ns, ne = A["ndim_shape"], A["ndim_exp"]
    idx = synth.landmark_ids(A, args.landmarks)
    P32 = RS.sample(args.seed, 0, B, ns, ne, 10, S, 0.7, [(0.0, 1.0)] * 4, [(-1.0, 1.0)] * 10, focal=1e-3 * S / 200.0)[0]
    mean, U = RL.split_image(RL.basis_image(A["mu"], A["pc_shape"], A["pc_exp"], idx), len(idx), ns + ne)
    fw = RL.Forward(P32, mean, U, im_size=float(S))
    target = torch.as_tensor(fw.points[:, 0:2].transpose(0, 2, 1).astype(np.float64))      # the batch's "landmarks"
    params = torch.as_tensor(P32)
    dev = torch.device("cpu")
    noise = ex.make_noise(args.seed, dev)
    noise(torch.zeros(B, 4), args.light_noise)       # the example perturbs light and alpha first: the same draws, in the same order
    noise(torch.zeros(B, 10), args.alpha_noise)
    pose_gt = params[:, :7]
    pose0, pose_scale = ex.pose_start(pose_gt, noise, args.pose_noise)
    pose = torch.zeros_like(pose_gt, requires_grad=True)
    opt = torch.optim.Adam([{"params": [pose], "lr": args.lr}])
    mean_t, U_t = torch.as_tensor(mean), torch.as_tensor(U)

    def pose_now():
        return pose0 + pose * pose_scale

    def loss_of():
        P = torch.cat([pose_now(), params[:, 7:]], dim=1).double()
        xy = _torch_points(P, mean_t, U_t, float(S))
        return args.landmark_lambda * (((xy - target) ** 2).sum(dim=(1, 2)) / len(idx)).mean()
    before = ex.rms(pose_now()[:, 3:6], pose_gt[:, 3:6])
    first, last = ex.descend(opt, loss_of, args.steps)
    after = ex.rms(pose_now()[:, 3:6], pose_gt[:, 3:6])
    print("landmarks-only fit in the model: loss %.4g -> %.4g, t3d_rms %.4g -> %.4g px" % (first, last, before, after))
    assert np.isfinite([first, last, after]).all() and torch.isfinite(pose).all()
    assert last < first and after < before
