"""GPU: the per-face albedo fit (fr_albedo_basis_build, fr_sfs_lighting, fr_albedo_lse_forward) against tests/ref_albedo_lse.py.
The basis and the lighting state bit for bit; the moments within the summation-order bound gamma_n sum |x_i x_j| of the fsum value
(the x themselves are bit-identical by construction), symmetric, reproducible and independent of the batch; the solve by its
backward error on the kernel's own moments; the failure rules; the operator surface bit for bit against the raw calls."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from conftest import pkg
import ref_albedo_lse as RA
from raw_calls import raw_fit as _raw_fit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = RA.STD_K


def _ops():
    return pkg("rendering_layer.ops")


def _L():
    return pkg("_lib").lib()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        u, v = a.view(np.uint32), np.asarray(b, np.float32).view(np.uint32)
    else:
        u, v = _bits64(a), _bits64(b)
    return a.shape == b.shape and bool(((u == v) | (np.isnan(a) & np.isnan(b))).all())


def _tile():
    out = (ctypes.c_int * 5)()
    _L().fr_debug_albedo_lse_geom(1, 1, 1, K, out)
    return out[0]


def _np(inp):
    return {k: v.cpu().numpy() for k, v in inp.items() if isinstance(v, torch.Tensor)}


def _ref(inp, ridge):
    n = _np(inp)
    return RA.fit_ref(n["basis"], n["tri_ind"], n["lighting"], n["normal"], n["abedo"], n["im_gray"], ridge)


def _faces(inp, sel):
    return dict(inp, **{k: inp[k][sel].contiguous() for k in ("tri_ind", "normal", "abedo", "im_gray")})


@pytest.fixture(scope="module")
def net(small_assets):
    A = dict(small_assets, pc_tex=RA.std_pc_tex(small_assets))
    return pkg("nets.network").FaceRecNet(mesh_data=A, batch_size=RA.STD_B, im_size=RA.STD_S, device=DEV)


def _rendered(net, B, shift=None, seed=6):
    """the standard inputs for B faces through the project's own render"""
    A = {"mu": net.mu.cpu().numpy()}
    V = _dev(RA.std_vertices(A, B=B, shift=shift))
    with torch.no_grad():
        a, n, tind = net.compute_abedo_image(V, net.tri, net.mu_tex, with_tri_ind=True)
    basis = net.albedo_basis()
    l = RA.std_lighting(RA.STD_S, RA.STD_S)
    star = RA.std_alpha_star(B, seed)
    I = RA.std_image(basis.cpu().numpy(), tind.cpu().numpy(), l, n.cpu().numpy(), a.cpu().numpy(), star)
    return dict(basis=basis, tri_ind=tind.contiguous(), lighting=_dev(l, torch.float64), normal=n.contiguous(),
                abedo=a.contiguous(), im_gray=_dev(I), star=star, V=V)


@pytest.fixture(scope="module")
def std(net):
    return _rendered(net, RA.STD_B)


def _synthetic(B, H, W, seed, ntri=37):
    """small shapes with no render behind them: random winners (a third background), unit normals, albedo in (0.2, 0.8)"""
    rs = np.random.RandomState(seed)
    tind = np.where(rs.rand(B, H, W, 1) < 0.3, -1.0, rs.randint(0, ntri, (B, H, W, 1))).astype(np.float32)
    n = rs.standard_normal((B, H, W, 3))
    n[..., 2] = np.abs(n[..., 2]) + 0.5
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    basis = rs.standard_normal((ntri, K)) * 0.05
    return dict(basis=_dev(basis, torch.float64), tri_ind=_dev(tind), lighting=_dev(RA.std_lighting(H, W, seed), torch.float64),
                normal=_dev(n), abedo=_dev(rs.uniform(0.2, 0.8, (B, H, W, 1))), im_gray=_dev(rs.uniform(0.0, 1.0, (B, H, W, 1))))


@pytest.fixture(scope="module")
def cases(std):
    T = _tile()
    return {"standard": std, "13x11": _synthetic(1, 13, 11, 1), "tiles+1": _synthetic(2, 1, 2 * T + 1, 2),
            "ragged": _synthetic(3, 7, T // 7 * 5 + 3, 3)}


# ---- basis -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kb", [1, 10, 15])
def test_basis_build_is_bit_exact(small_assets, Kb):
    rs = np.random.RandomState(Kb)
    N = np.asarray(small_assets["mu"]).size // 3
    pc = (0.05 * rs.standard_normal((3 * N, Kb))).astype(np.float32)
    tri = np.asarray(small_assets["tri"], np.float32).copy()
    tri[0, 2], tri[1, 5], tri[2, 9], tri[1, 11] = N, -1.0, np.nan, 3e9      # out-of-range ids -> rows of +0.0
    got = _ops().albedo_basis(_dev(tri), _dev(pc))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = RA.basis_ref(tri, pc)
    assert got.dtype == np.float64 and got.shape == (tri.shape[1], Kb)
    assert _same_bits(got, want)
    for t in (2, 5, 9, 11):
        assert not _bits64(got[t]).any()                                    # +0.0, not -0.0
    assert np.abs(got).max() > 0


# ---- lighting ----------------------------------------------------------------------------------------------------------------------
def test_lighting_state_equals_the_fused_forwards():
    L = _L()
    rs = np.random.RandomState(4)
    B, H, W = 5, 13, 11
    n = rs.standard_normal((B, H, W, 3))
    n = _dev(n / np.linalg.norm(n, axis=-1, keepdims=True))
    a, I = _dev(rs.uniform(0.1, 0.9, (B, H, W, 1))), _dev(rs.uniform(0, 1, (B, H, W, 1)))
    I[0, 3, 4, 0] = float("nan")                                            # a poisoned pixel travels the same way
    a2, out = _dev(rs.uniform(0.1, 0.9, (B, H, W, 1))), torch.empty((B, H, W, 1), device=DEV)
    nst, nmo = L.fr_sfs_state_bytes(H, W), L.fr_sfs_moments_bytes(H, W)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def state():
        return torch.full((10, H, W), 7.0, dtype=torch.float64, device=DEV)
    s_fwd = state()
    assert L.fr_sfs_intensity_forward(_p(a), _p(n), _p(I), _p(a2), _p(n), B, H, W, 1e-15, _p(out), _p(s_fwd), nst, stream) == 0
    got = _ops().sfs_lighting(a, n, I)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, H, W) and not got.requires_grad
    assert _same_bits(got.cpu().numpy(), s_fwd[6:9].cpu().numpy())
    for cuts in ((0, 5), (0, 2, 5), (0, 1, 3, 5)):
        parts = torch.empty((len(cuts) - 1, 9, H, W), dtype=torch.float64, device=DEV)
        for k in range(len(cuts) - 1):
            b0, b1 = cuts[k], cuts[k + 1]
            part = torch.empty((9, H, W), dtype=torch.float64, device=DEV)     # (a buffer of its own: 16-byte aligned)
            assert L.fr_sfs_moments(_p(a[b0:b1]), _p(n[b0:b1]), _p(I[b0:b1]), b1 - b0, H, W, _p(part), nmo, stream) == 0
            parts[k] = part
        s_split, s_light = state(), state()
        assert L.fr_sfs_solve_shade(_p(parts), len(cuts) - 1, _p(a2), _p(n), B, H, W, 1e-15, _p(out), _p(s_split), nst, stream) == 0
        assert L.fr_sfs_lighting(_p(parts), len(cuts) - 1, H, W, 1e-15, _p(s_light), nst, stream) == 0
        torch.cuda.synchronize()
        assert _same_bits(s_light.cpu().numpy(), s_split.cpu().numpy()), cuts
        if len(cuts) == 2:
            assert _same_bits(s_light.cpu().numpy(), s_fwd.cpu().numpy())


# ---- moments, solve ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["standard", "13x11", "tiles+1", "ragged"])
@pytest.mark.parametrize("ridge", [0.0, 1e-6])
def test_moments_and_solve(cases, name, ridge):
    inp = cases[name]
    B, H, W = inp["tri_ind"].shape[:3]
    alpha, stats, M = _raw_fit(inp, ridge)
    ralpha, rstats, RM, RS = _ref(inp, ridge)
    # moments: only the order of summation differs from the fsum value
    bound = RA.gamma(H * W) * RS
    err = np.abs(M - RM)
    print("%s ridge %g: max |M - fsum| / (gamma_n sum|x_i x_j|) = %.3g" % (name, ridge, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert _same_bits(M, np.transpose(M, (0, 2, 1)))
    assert not _bits64(M[:, K + 1:, :]).any() and not _bits64(M[:, :, K + 1:]).any()
    assert np.array_equal(stats[:, 0], rstats[:, 0]) and np.array_equal(stats[:, 1], M[:, K, K])
    # run to run, and a face alone against the same face in the batch
    alpha2, stats2, M2 = _raw_fit(inp, ridge)
    assert _same_bits(M, M2) and _same_bits(alpha, alpha2) and _same_bits(stats, stats2)
    for b in range(B):
        a1, s1, M1 = _raw_fit(_faces(inp, slice(b, b + 1)), ridge)
        assert _same_bits(M1[0], M[b]) and _same_bits(a1[0], alpha[b]) and _same_bits(s1[0], stats[b]), b
    # solve: backward error on the kernel's own moments
    for b in range(B):
        assert stats[b, 3] == 1.0 and rstats[b, 3] == 1.0, b
        G, r = M[b, :K, :K], M[b, :K, K]
        Gp = G + RA.ridge_lambda(M[b], K, ridge) * np.eye(K)
        ah = alpha[b].astype(np.float64)
        res = np.abs(Gp @ ah - r).max()
        lim = 2.0 ** -23 * ((np.abs(Gp) @ np.abs(ah)).max() + np.abs(r).max())
        print("  face %d: backward error %.3g of %.3g, E0 %.6g, E1 %.6g" % (b, res, lim, stats[b, 1], stats[b, 2]))
        assert res <= lim
        want = RA.e1_ref(M[b], K, alpha[b])
        assert abs(stats[b, 2] - want) <= 1e-12 * abs(want)
        assert stats[b, 2] <= stats[b, 1]
    if name == "standard":
        for b in range(B):
            rec = np.linalg.norm(alpha[b] - inp["star"][b]) / np.linalg.norm(inp["star"][b])
            assert rec <= 1e-5, (b, rec)


# ---- the failure rules -------------------------------------------------------------------------------------------------------------
def test_face_off_the_image(net):
    inp = _rendered(net, 5, shift={3: (100.0, 0.0)})
    assert float((inp["tri_ind"][3] >= 0).sum()) == 0 and float((inp["tri_ind"][4] >= 0).sum()) > 300
    alpha, stats, M = _raw_fit(inp, 1e-6)
    assert stats[:, 3].tolist() == [1.0, 1.0, 1.0, 0.0, 1.0]
    assert stats[3].tolist() == [0.0, 0.0, 0.0, 0.0] and not alpha[3].view(np.uint32).any() and not _bits64(M[3]).any()
    keep = [0, 1, 2, 4]
    a4, s4, M4 = _raw_fit(_faces(inp, keep), 1e-6)
    assert _same_bits(a4, alpha[keep]) and _same_bits(s4, stats[keep]) and _same_bits(M4, M[keep])


def test_three_pixel_face_fails_without_a_ridge_and_fits_with_one(std):
    tind = std["tri_ind"].clone()
    flat = tind.view(RA.STD_B, -1)
    cov = torch.nonzero(flat[1] >= 0)[:, 0]
    flat[1, cov[3:]] = -1.0
    inp = dict(std, tri_ind=tind)
    a0, s0, M0 = _raw_fit(inp, 0.0)
    assert s0[:, 0].tolist()[1] == 3.0 and s0[:, 3].tolist() == [1.0, 0.0, 1.0]
    assert not a0[1].view(np.uint32).any() and s0[1, 2] == s0[1, 1]
    a1, s1, M1 = _raw_fit(inp, 1e-6)
    assert s1[:, 3].tolist() == [1.0, 1.0, 1.0] and a1[1].any() and s1[1, 2] <= s1[1, 1]
    assert _same_bits(M0, M1)
    full = _raw_fit(std, 0.0)
    for b in (0, 2):                                                        # the failed face leaves the others' bits alone
        assert _same_bits(a0[b], full[0][b]) and _same_bits(s0[b], full[1][b]) and _same_bits(M0[b], full[2][b])


def test_poisoned_face(std):
    I = std["im_gray"].clone()
    cov = torch.nonzero(std["tri_ind"].view(RA.STD_B, -1)[1] >= 0)[:, 0]
    I.view(RA.STD_B, -1)[1, cov[17]] = float("nan")
    alpha, stats, M = _raw_fit(dict(std, im_gray=I), 1e-6)
    clean = _raw_fit(std, 1e-6)
    assert stats[:, 3].tolist() == [1.0, 0.0, 1.0] and not alpha[1].view(np.uint32).any()
    assert np.isnan(M[1, K, K]) and stats[1, 0] == clean[1][1, 0]
    for b in (0, 2):
        assert _same_bits(alpha[b], clean[0][b]) and _same_bits(stats[b], clean[1][b]) and _same_bits(M[b], clean[2][b])
    # a NaN at a pixel the face does not cover is not read
    I = std["im_gray"].clone()
    out = torch.nonzero(std["tri_ind"].view(RA.STD_B, -1)[1] < 0)[:, 0]
    I.view(RA.STD_B, -1)[1, out[5]] = float("nan")
    again = _raw_fit(dict(std, im_gray=I), 1e-6)
    assert all(_same_bits(x, y) for x, y in zip(again, clean))


# ---- operator ----------------------------------------------------------------------------------------------------------------------
def test_operator_equals_the_raw_calls(std):
    alpha, stats = _ops().albedo_lse(std["basis"], std["tri_ind"], std["lighting"], std["normal"], std["abedo"], std["im_gray"])
    torch.cuda.synchronize()
    assert alpha.dtype == torch.float32 and stats.dtype == torch.float64 and not alpha.requires_grad and not stats.requires_grad
    ra, rs, _ = _raw_fit(std, 1e-6)
    assert _same_bits(alpha.cpu().numpy(), ra) and _same_bits(stats.cpu().numpy(), rs)
    a0, s0 = _ops().albedo_lse(std["basis"], std["tri_ind"], std["lighting"], std["normal"], std["abedo"], std["im_gray"], ridge=0.0)
    assert _same_bits(a0.cpu().numpy(), _raw_fit(std, 0.0)[0])


def _residuals(intensity, I):
    return ((intensity.double() - I.double()) ** 2).sum(dim=(1, 2, 3)).cpu().numpy()


def test_model_with_the_fit_equals_the_chain_by_hand_and_lowers_every_face(net, std):
    losses, ops = pkg("nets.losses"), _ops()
    V, I = std["V"], std["im_gray"]
    with torch.no_grad():
        got = losses.get_spherical_harmonics_model(net, V, I, fused=True, alpha_lse=True)
        a, n, tind = net.compute_abedo_image(V, net.tri, net.mu_tex, with_tri_ind=True)
        l = ops.sfs_lighting(a, n, I)
        alpha, stats = ops.albedo_lse(net.albedo_basis(), tind, l, n, a, I)
        tex = net.mu_tex[None] + (alpha @ net.pc_tex.t()).reshape(RA.STD_B, 3, -1)
        a2, n2 = net.compute_abedo_image(V, net.tri, tex)
        want = ops.sfs_intensity(a, n, I, a2, n2)
        off = losses.get_spherical_harmonics_model(net, V, I, fused=True)
    torch.cuda.synchronize()
    assert _same_bits(got.cpu().numpy(), want.cpu().numpy())
    assert stats[:, 3].tolist() == [1.0] * RA.STD_B
    r_on, r_off = _residuals(got, I), _residuals(off, I)
    print("sum (intensity_recover - I)^2 per face: shared param_tex", r_off, "fitted", r_on)
    assert (r_on < r_off).all()
    # with the fine depth's normals as the shaded ones
    fine = (torch.rand((RA.STD_B, RA.STD_S, RA.STD_S, 1), generator=torch.Generator().manual_seed(3)) * 4.0).to(DEV)
    with torch.no_grad():
        got = losses.get_spherical_harmonics_model(net, V, I, fused=True, alpha_lse=True, fine_depth=fine, rcond=1e-6)
        l = ops.sfs_lighting(a, n, I, rcond=1e-6)
        nf = ops.depth_normals(fine, mask=tind)
        alpha, _ = ops.albedo_lse(net.albedo_basis(), tind, l, nf, a, I)
        tex = net.mu_tex[None] + (alpha @ net.pc_tex.t()).reshape(RA.STD_B, 3, -1)
        a2, _ = net.compute_abedo_image(V, net.tri, tex)
        want = ops.sfs_intensity(a, n, I, a2, nf, rcond=1e-6)
    assert _same_bits(got.cpu().numpy(), want.cpu().numpy())


def test_get_loss_passes_the_flags_and_is_unchanged_without_them(net, std):
    losses = pkg("nets.losses")
    B, S = RA.STD_B, RA.STD_S
    g = torch.Generator().manual_seed(9)
    pred = torch.zeros((B, net.ndim), device=DEV)
    lab = (0.1 * torch.randn((B, net.ndim), generator=g)).to(DEV)
    coarse, fine = torch.rand((B, S, S, 1), generator=g).to(DEV), torch.rand((B, S, S, 1), generator=g).to(DEV)
    args = (net, pred, lab, std["im_gray"], std["V"], coarse, fine)
    with torch.no_grad():
        plain = losses.get_loss(*args, sfs_fused=True)
        off = losses.get_loss(*args, sfs_fused=True, sfs_alpha_lse=False, sfs_alpha_ridge=1e-6)
        on = losses.get_loss(*args, sfs_fused=True, sfs_alpha_lse=True)
        want = torch.nn.functional.mse_loss(losses.get_spherical_harmonics_model(net, std["V"], std["im_gray"], fused=True,
                                                                                 alpha_lse=True), std["im_gray"])
    for k in plain:
        assert _same_bits(plain[k].cpu().numpy(), off[k].cpu().numpy()), k
    assert _same_bits(on["spherical_harmonics_loss"].cpu().numpy(), want.cpu().numpy())
    assert float(on["spherical_harmonics_loss"]) < float(plain["spherical_harmonics_loss"])
    with pytest.raises(ValueError):
        losses.get_loss(*args, sfs_alpha_lse=True)


# ---- threads -----------------------------------------------------------------------------------------------------------------------
def test_two_threads_two_streams(std):
    ops = _ops()
    inputs = [std, dict(std, im_gray=(std["im_gray"] * 0.5 + 0.1).contiguous())]
    single = []
    for inp in inputs:
        a, s = ops.albedo_lse(inp["basis"], inp["tri_ind"], inp["lighting"], inp["normal"], inp["abedo"], inp["im_gray"])
        single.append((a.cpu().numpy(), s.cpu().numpy()))
    torch.cuda.synchronize()
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            stream = torch.cuda.Stream(device=DEV)
            inp = inputs[i]
            with torch.cuda.stream(stream):
                gate.wait(timeout=30)
                outs = [ops.albedo_lse(inp["basis"], inp["tri_ind"], inp["lighting"], inp["normal"], inp["abedo"], inp["im_gray"])
                        for _ in range(20)]
                stream.synchronize()
            results[i] = [(a.cpu().numpy(), s.cpu().numpy()) for a, s in outs]
        except Exception as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        for a, s in results[i]:
            assert _same_bits(a, single[i][0]) and _same_bits(s, single[i][1]), i
