"""CPU: the pose-gradient entry points (fr_decode_pose_backward, fr_decode_render_backward_pose) exist, validate before any HIP
call and size their workspace as the header says; the float64 reference of the GPU tests (tests/ref_pose_backward.py) is itself
held to central differences of a float64 decode; the inputs of the GPU cases satisfy the discrimination cap; the new kernels
keep everything in registers."""
import ctypes
import os
import re

import numpy as np

from conftest import pkg
import ref_pose_backward as RP

NEW = ("fr_decode_pose_backward_workspace_bytes", "fr_decode_pose_backward", "fr_decode_render_backward_pose_workspace_bytes",
       "fr_decode_render_backward_pose", "fr_debug_pose_bwd_geom")


def _L():
    return pkg("_lib").lib()


def _geom(B, N):
    out = (ctypes.c_int * 4)()
    _L().fr_debug_pose_bwd_geom(B, N, out)
    return list(out)


def test_symbols_exported():
    L = _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS


def test_pose_backward_validates_before_any_hip_call():
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(1), ctypes.c_void_p(4096)
    f = ctypes.c_float(200.0)
    call = L.fr_decode_pose_backward
    need = L.fr_decode_pose_backward_workspace_bytes(2, 100)

    def args(g=one, v=one, par=one, R=nul, B=2, N=100, ns=5, ne=3, gp=one, gR=one, ws=al, nb=need):
        return (g, v, par, R, B, N, ns, ne, f, gp, gR, ws, nb, nul)
    assert call(*args(B=-1)) == -1 and call(*args(N=-1)) == -1 and call(*args(ns=-1)) == -1
    assert call(*args(B=0)) == 0 and call(*args(B=0, gp=nul, gR=nul, ws=nul, nb=0)) == 0     # empty batch
    assert call(*args(gp=nul, gR=nul)) == -1                                                  # both outputs NULL
    assert call(*args(g=nul)) == -1 and call(*args(v=nul)) == -1 and call(*args(par=nul)) == -1
    assert call(*args(nb=need - 1)) == -2 and call(*args(ws=nul)) == -2                       # workspace too small / missing
    assert call(*args(ws=ctypes.c_void_p(4096 + 8))) == -2                                    # not 16-byte aligned
    assert call(*args(gp=nul, nb=need - 1)) == -2 and call(*args(gR=nul, nb=need - 1)) == -2  # one output is enough to get that far


def test_fused_step_validates_like_the_render_backward():
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(128), ctypes.c_void_p(4096)
    f = ctypes.c_float(200.0)
    B, N, ns, ne, ntri, H, W = 2, 64, 5, 3, 7, 8, 8
    wsb = L.fr_decode_render_backward_pose_workspace_bytes
    base = L.fr_decode_render_backward_workspace_bytes(B, N, ns, ne, H, W)
    need = wsb(B, N, ns, ne, H, W)
    assert need % 256 == 0 and need >= base + L.fr_decode_pose_backward_workspace_bytes(B, N)
    hb = L.fr_decode_render_vertex_bytes(B, N)
    call = L.fr_decode_render_backward_pose

    def args(gd=one, gi=one, gn=one, img=one, dep=one, tri=one, ti=one, par=one, mu=one, pt=one, B=B, N=N, ns=ns, ne=ne,
             gp=one, ws=al, nb=need, hand=al, hbytes=hb, gR=one):
        return (gd, gi, gn, img, dep, tri, ti, par, mu, pt, nul, B, N, ns, ne, ntri, H, W, f, gp, ws, nb, nul, hand, hbytes, gR)
    assert call(*args(B=0)) == 0 and call(*args(B=-1)) == -1
    for k in ("tri", "ti", "par", "mu", "pt", "gp"):
        assert call(*args(**{k: nul})) == -1, k
    assert call(*args(gd=nul, gi=nul, gn=nul)) == -1
    assert call(*args(img=nul)) == -1 and call(*args(dep=nul)) == -1
    assert call(*args(nb=need - 1)) == -2 and call(*args(nb=base)) == -2 and call(*args(ws=nul)) == -2
    assert call(*args(ws=ctypes.c_void_p(4096 + 128))) == -2
    assert call(*args(hand=nul)) == -2 and call(*args(hbytes=hb - 1)) == -2 and call(*args(hand=ctypes.c_void_p(4096 + 64))) == -2
    # FR_ERR_UNSUPPORTED exactly where fr_decode_render_backward answers it
    assert wsb(B, N, 250, 29, H, W) == 0 and call(*args(ns=250, ne=29, nb=1 << 30)) == -4
    assert wsb(B, 15, ns, ne, H, W) == 0 and call(*args(N=15, nb=1 << 30)) == -4
    assert wsb(0, N, ns, ne, H, W) == 0


def test_workspace_sizes_and_geometry():
    L = _L()
    wsb = L.fr_decode_pose_backward_workspace_bytes
    assert wsb(0, 100) == 0 and wsb(-1, 100) == 0 and wsb(4, 0) == 0 and wsb(4, -3) == 0
    assert _geom(4, 0) == [0, 0, 0, 0]
    prev = 0
    for B in (1, 2, 17, 64, 65, 128):
        got = wsb(B, 53215)
        assert got > prev and got % 16 == 0
        prev = got
    prev = 0
    for N in (1, 7, 16, 2047, 2048, 2049, 4270, 53215, 200000):
        chunk, chunks, threads, depth = _geom(64, N)
        assert _geom(1, N) == [chunk, chunks, threads, depth]          # the chunking depends on N alone
        assert chunk % 4 == 0 and threads % 64 == 0 and chunks == -(-N // chunk) and depth >= 1
        got = wsb(64, N)
        assert got >= prev and got >= 64 * chunks * 9 * 4 and got % 16 == 0
        prev = got
    assert _geom(64, 53215)[:3] == [2048, 26, 256]


# ---- the reference against central differences of a float64 decode -----------------------------------------------------------------
def _loss(G, v, R, t, f, im):
    return (G.astype(np.float64) * RP.decode_f64(v, R, t, f, im)).sum(axis=(1, 2))


def _moderate(rs, B, N):
    P = np.zeros((B, 7), np.float32)
    P[:, 0:3] = rs.uniform(-1.0, 1.0, (B, 3))
    P[:, 3:5] = rs.uniform(60, 140, (B, 2))
    P[:, 5] = rs.uniform(-1, 1, B)
    P[:, 6] = rs.uniform(2e-4, 1e-3, B)
    G = rs.standard_normal((B, 3, N)).astype(np.float32)
    v = rs.uniform(-1e5, 1e5, (B, 3, N))
    return P, G, v


def test_reference_angles_against_central_differences(oracle):
    rs = np.random.RandomState(5)
    B, N, im, h = 6, 37, 200.0, 1e-6
    P, G, v = _moderate(rs, B, N)
    ref = RP.PoseRef(oracle, G, v, P, R=None, im_size=im)
    a = P[:, 0:3].astype(np.float64)
    t, f = P[:, 3:6].astype(np.float64), P[:, 6].astype(np.float64)
    # the float64 rotation of this file IS the oracle's, to fp32 rounding
    assert np.abs(RP.rotation_f64(a)[0] - oracle.rotation_matrix_batch(P[:, 0:3])).max() <= 2.0 ** -24
    fd = np.zeros((B, 3))
    for k in range(3):
        ap, am = a.copy(), a.copy()
        ap[:, k] += h
        am[:, k] -= h
        fd[:, k] = (_loss(G, v, RP.rotation_f64(ap)[0], t, f, im) - _loss(G, v, RP.rotation_f64(am)[0], t, f, im)) / (2 * h)
    scale = np.abs(fd).max(axis=1, keepdims=True)
    assert np.all(scale > 0)
    assert np.abs(ref.angles - fd).max() <= 1e-6 * scale.min(), np.abs((ref.angles - fd) / scale).max()
    assert np.all(np.abs(ref.angles - fd) <= 1e-6 * scale)


def test_reference_grad_R_against_central_differences_non_orthogonal(oracle):
    rs = np.random.RandomState(6)
    B, N, im, h = 5, 41, 200.0, 1e-6
    P, G, v = _moderate(rs, B, N)
    R = (RP.rotations(rs, B).astype(np.float64) @ (np.eye(3) + 0.1 * rs.uniform(-1, 1, (B, 3, 3)))).astype(np.float32)
    assert np.abs(np.einsum("bij,bkj->bik", R, R) - np.eye(3)).max() > 0.05      # really not a rotation
    ref = RP.PoseRef(oracle, G, v, P, R=R, im_size=im)
    assert np.all(ref.angles == 0)
    t, f = P[:, 3:6].astype(np.float64), P[:, 6].astype(np.float64)
    Rm = R.astype(np.float64)
    fd = np.zeros((B, 3, 3))
    for i in range(3):
        for j in range(3):
            Rp_, Rm_ = Rm.copy(), Rm.copy()
            Rp_[:, i, j] += h
            Rm_[:, i, j] -= h
            fd[:, i, j] = (_loss(G, v, Rp_, t, f, im) - _loss(G, v, Rm_, t, f, im)) / (2 * h)
    scale = np.abs(fd).max(axis=(1, 2), keepdims=True)
    assert np.all(np.abs(ref.grad_R - fd) <= 1e-6 * scale), np.abs((ref.grad_R - fd) / scale).max()
    # ... and the kernels' route to it: the pose moment of the EXACT forward output through cof(R) / det(R); A R is not it
    dq = G.astype(np.float64).copy()
    dq[:, 1] = -dq[:, 1]
    q = ref.V.copy()
    q[:, 1] = (im - 1.0) - q[:, 1]
    A = np.einsum("bip,bkp->bik", dq, q - t[:, :, None])
    cof, det = RP.cofactor(Rm)
    assert np.all(np.abs(A @ cof / det[:, None, None] - ref.grad_R) <= 1e-9 * scale)
    assert np.abs(A @ Rm - ref.grad_R).max() > 0.05 * scale.min()


def test_reference_singular_rotation_and_zero_focal_give_zeros(oracle):
    rs = np.random.RandomState(7)
    P, G, v = _moderate(rs, 3, 19)
    R = RP.rotations(rs, 3)
    R[1, 2] = R[1, 0]                       # face 1: det == 0
    P[2, 6] = 0.0                           # face 2: f == 0
    ref = RP.PoseRef(oracle, G, v, P, R=R)
    assert list(ref.singular) == [False, True, False]
    assert np.all(ref.grad_R[1] == 0) and np.all(ref.grad_R[2] == 0) and np.abs(ref.grad_R[0]).max() > 0
    ref = RP.PoseRef(oracle, G, v, P, R=None)
    assert np.all(ref.grad_R[2] == 0) and np.all(ref.angles[2] == 0) and np.abs(ref.angles[:2]).min() > 0
    bG, bang = ref.bound(ref.V.astype(np.float32), 16)
    assert np.all(np.isfinite(bG)) and np.all(np.isfinite(bang))


def test_gpu_case_inputs_satisfy_the_discrimination_cap(oracle):
    """A condition on the INPUTS of tests/test_pose_backward_gpu.py, checked with the reference alone: for every face of every
    case the proven bound is below 1e-3 of the face's max |G_ij| (and of its largest angle gradient), so that a sign or a
    transposition error cannot hide under it.  Faces whose gradient is zero by definition (det == 0, f == 0) have no scale: the
    GPU test holds the first to exact zeros and the second to the bound."""
    chunk, _, _, depth = _geom(1, 4270)
    seen_N, seen_B = set(), set()
    for name, seed, B, N, mode, f0 in RP.case_list(chunk):
        c = RP.make_case(seed, B, N, mode, f0)
        ref = RP.PoseRef(oracle, c["G"], c["v"], c["P"], R=c["R"])
        bG, bang = ref.bound(c["Vg"], depth)
        zero = ref.singular | (ref.f == 0)
        gmax = np.abs(ref.grad_R).max(axis=(1, 2))
        assert np.all(gmax[~zero] > 0), name
        assert np.all(bG.max(axis=(1, 2))[~zero] < 1e-3 * gmax[~zero]), (name, (bG.max(axis=(1, 2)) / np.where(zero, 1, gmax)).max())
        if mode is None:
            amax = np.abs(ref.angles).max(axis=1)
            assert np.all(bang.max(axis=1)[~zero] < 1e-3 * amax[~zero]), (name, (bang.max(axis=1) / np.where(zero, 1, amax)).max())
        seen_N.add(N)
        seen_B.add(B)
    assert {1, 7, 15, 16, 17, 4270, chunk + 1, chunk - 1} <= seen_N and {1, 17, 64, 65} <= seen_B


def test_pose_kernels_keep_everything_in_registers():
    import subprocess
    h = pkg("_lib")
    src = os.path.join(h._CSRC, "fr_decode_bwd.hip")
    cmd = [h._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src]
    out = subprocess.run(cmd, cwd=h._CSRC, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: Function Name: ", out.stderr)[1:] if b.startswith("_ZN2fr22bwd_pose_")]
    assert len(blocks) == 3            # the moment kernel's two layouts and the finish kernel
    for b in blocks:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b[:400]
        assert re.search(r"VGPRs Spill: 0\b", b), b[:400]
