"""CPU: the split shape-from-shading entry points (include/fr_hotpath.h, "shape-from-shading term across ranks") -- exports,
validation before any HIP call, sizes, launch geometry -- the exchange helper utils/dist.py::all_gather_stack on a two-rank gloo
group, and the ValueErrors of the fused_gather flags.  No GPU is touched."""
import ctypes
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

import ref_sfs as RS
from conftest import ROOT, pkg

NEW = ("fr_sfs_moments_bytes", "fr_sfs_moments", "fr_sfs_solve_shade", "fr_sfs_q_bytes", "fr_sfs_backward_q", "fr_sfs_backward_apply",
       "fr_debug_sfs_split_geom")
INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4


def _L():
    return pkg("_lib").lib()


def test_symbols_exported_and_version_unchanged():
    host, L = pkg("_lib"), _L()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in host.EXPORTS, name
    assert L.fr_version().startswith(b"fr_hotpath 0.4 ")


def test_sizes():
    L = _L()
    for H, W in ((5, 4), (200, 200), (1, 1), (3, 67)):
        assert L.fr_sfs_moments_bytes(H, W) == 9 * H * W * 8
        assert L.fr_sfs_q_bytes(H, W) == 3 * H * W * 8
    for H, W in ((0, 4), (4, 0), (0, 0), (-1, 4), (4, -1)):
        assert L.fr_sfs_moments_bytes(H, W) == 0 and L.fr_sfs_q_bytes(H, W) == 0
    assert L.fr_sfs_moments_bytes(46341, 46341) == 9 * 46341 * 46341 * 8     # no 32-bit overflow


def _geom(B, H, W):
    out = (ctypes.c_int * 6)()
    _L().fr_debug_sfs_split_geom(B, H, W, out)
    return list(out)


def test_geometry():
    for B, H, W in RS.CASES + ((32, 200, 200), (64, 200, 200), (0, 5, 4), (3, 5, 4), (17, 9, 70), (13, 9, 70)):
        S = min(4, max(1, B // 4))
        assert _geom(B, H, W) == [64, S, (H * W + 63) // 64, 9 * S * 64 * 8, 3 * 64 * 8, 3 * S * 64 * 8], (B, H, W)
        if B > 0:                                                            # the one-call route's slices and workgroups
            one = (ctypes.c_int * 4)()
            _L().fr_debug_sfs_geom(B, H, W, one)
            assert _geom(B, H, W)[:3] == list(one)[:3]
    assert _geom(0, 5, 4)[:3] == [64, 1, 1]                                  # an empty shard still launches the part kernels
    assert _geom(6, 0, 4) == [0] * 6 and _geom(6, 5, 0) == [0] * 6 and _geom(-1, 5, 4) == [0] * 6
    assert _geom(1, 46341, 46341) == [0] * 6                                 # past the pixel limit: refused, so no geometry


def test_validates_before_any_hip_call():
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(4), ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4096 + 8)
    B, H, W = 6, 5, 4
    nm, nq, nst = L.fr_sfs_moments_bytes(H, W), L.fr_sfs_q_bytes(H, W), L.fr_sfs_state_bytes(H, W)

    def mom(a=one, n=one, im=one, B=B, H=H, W=W, out=al, nb=nm):
        return L.fr_sfs_moments(a, n, im, B, H, W, out, nb, nul)

    def sol(parts=one, nparts=2, a2=one, n2=one, B=B, H=H, W=W, rc=1e-6, out=one, st=al, nb=nst):
        return L.fr_sfs_solve_shade(parts, nparts, a2, n2, B, H, W, rc, out, st, nb, nul)

    def bq(g=one, a2=one, n2=one, B=B, H=H, W=W, out=al, nb=nq):
        return L.fr_sfs_backward_q(g, a2, n2, B, H, W, out, nb, nul)

    def app(g=one, a=one, im=one, a2=one, n2=one, st=al, nb=nst, parts=one, nparts=2, B=B, H=H, W=W, gn=one, gn2=one, ga2=one):
        return L.fr_sfs_backward_apply(g, a, im, a2, n2, st, nb, parts, nparts, B, H, W, gn, gn2, ga2, nul)

    # negative sizes
    for call in (mom, sol, bq, app):
        assert call(B=-1) == INVALID and call(H=-1) == INVALID and call(W=-1) == INVALID
        assert call(B=0, H=-1) == INVALID and call(H=0, W=-1) == INVALID     # the scalar checks come before "no work"
    # rcond
    for rc in (-1e-9, float("nan"), float("inf")):
        assert sol(rc=rc) == INVALID and sol(rc=rc, B=0) == INVALID and sol(rc=rc, H=0) == INVALID
    assert sol(rc=0.0, B=0) == 0
    # nparts
    for call in (sol, app):
        assert call(nparts=0) == INVALID and call(nparts=-3) == INVALID and call(nparts=4097) == INVALID
        assert call(nparts=0, B=0) == INVALID and call(nparts=4097, H=0) == INVALID          # ... and so do these
        assert call(nparts=1, B=0) == 0 and call(nparts=4096, B=0) == 0
        assert call(nparts=4096, st=nul) == WORKSPACE                        # 4096 parts pass the scalar checks
    assert app(nparts=0, gn=nul, parts=nul) == INVALID                       # checked even where q_parts is not read
    # no work: an empty image everywhere; B == 0 in the two finishing calls (pointers are not looked at)
    for call in (mom, sol, bq, app):
        assert call(H=0) == 0 and call(W=0) == 0
    assert mom(H=0, a=nul, n=nul, im=nul, out=nul, nb=0) == 0 and bq(W=0, g=nul, a2=nul, n2=nul, out=nul, nb=0) == 0
    assert sol(B=0, parts=nul, a2=nul, n2=nul, out=nul, st=nul, nb=0) == 0
    assert app(B=0, g=nul, a=nul, im=nul, a2=nul, n2=nul, st=nul, nb=0, parts=nul, gn=nul, gn2=nul, ga2=nul) == 0
    # B == 0 with an image: the part kernels still have planes to write, so their buffer is checked (the face pointers are not)
    assert mom(B=0, a=nul, n=nul, im=nul, out=nul) == WORKSPACE and mom(B=0, a=nul, n=nul, im=nul, nb=nm - 1) == WORKSPACE
    assert bq(B=0, g=nul, a2=nul, n2=nul, out=odd) == WORKSPACE
    # NULL pointers
    for k in ("a", "n", "im"):
        assert mom(**{k: nul}) == INVALID
    for k in ("parts", "a2", "n2", "out"):
        assert sol(**{k: nul}) == INVALID
    for k in ("g", "a2", "n2"):
        assert bq(**{k: nul}) == INVALID
    for k in ("g", "a", "im", "a2", "n2"):
        assert app(**{k: nul}) == INVALID
    assert app(gn=nul, gn2=nul, ga2=nul) == INVALID                          # all three outputs NULL
    assert app(parts=nul) == INVALID                                         # grad_normal wants q_parts
    assert app(parts=nul, gn2=nul, ga2=nul) == INVALID
    # q_parts may be NULL exactly when grad_normal is NULL: these pass every check before the launch, so they are shown to pass
    # the pointer checks by failing the NEXT one (the state)
    assert app(parts=nul, gn=nul, st=nul) == WORKSPACE and app(parts=nul, gn=nul, gn2=nul, st=nul) == WORKSPACE
    assert app(parts=nul, st=nul) == INVALID                                 # ... which the refused form never reaches
    # NULL comes before the buffers
    assert mom(a=nul, out=nul) == INVALID and sol(parts=nul, st=nul) == INVALID and bq(g=nul, out=nul) == INVALID
    # buffers: missing, too small, not 16-byte aligned
    assert mom(out=nul) == WORKSPACE and mom(nb=nm - 1) == WORKSPACE and mom(out=odd) == WORKSPACE
    assert bq(out=nul) == WORKSPACE and bq(nb=nq - 1) == WORKSPACE and bq(out=odd) == WORKSPACE
    for call in (sol, app):
        assert call(st=nul) == WORKSPACE and call(nb=nst - 1) == WORKSPACE and call(st=odd) == WORKSPACE
    # the pixel limit (2^31 - 65 pixels pass it; the buffer sizes are the caller's word here)
    big = 1 << 62
    assert mom(H=46341, W=46341, nb=big) == UNSUPPORTED and bq(H=46341, W=46341, nb=big) == UNSUPPORTED
    assert sol(H=46341, W=46341, nb=big) == UNSUPPORTED and app(H=46341, W=46341, nb=big) == UNSUPPORTED
    assert mom(H=46341, W=46341, nb=nm) == WORKSPACE                         # ... and the buffer check comes before it


def test_flags_raise_value_error():
    L = pkg("nets.losses")
    z = torch.zeros((1, 2, 2, 1))
    n = torch.zeros((1, 2, 2, 3))
    for kw in ({}, {"gather": True}, {"fused": True}):
        with pytest.raises(ValueError, match="fused_gather"):
            L.spherical_harmonics_intensity(z, n, z, z, n, fused_gather=True, **kw)
        with pytest.raises(ValueError, match="fused_gather"):                # refused before the face_net is looked at
            L.get_spherical_harmonics_model(None, None, z, fused_gather=True, **kw)


def test_get_loss_passes_the_flag_down(monkeypatch):
    L = pkg("nets.losses")
    seen = {}

    def fake(fn, vp, im, **kw):
        seen.update(kw)
        raise ValueError("fused_gather probe")
    monkeypatch.setattr(L, "get_spherical_harmonics_model", fake)

    class Net:
        ndim, ndim_pose = 9, 7

        @staticmethod
        def geometry_product(x):
            return x
    p = torch.zeros((2, 9))
    with pytest.raises(ValueError, match="probe"):
        L.get_loss(Net, p, p, None, None, None, None, gather_sfs=True, sfs_fused=True, sfs_fused_gather=True)
    assert seen.get("fused_gather") is True and seen.get("gather") is True and seen.get("fused") is True
    seen.clear()
    with pytest.raises(ValueError, match="probe"):
        L.get_loss(Net, p, p, None, None, None, None)
    assert "fused_gather" not in seen                                        # flag off: the call is the parent's, word for word


# ---- the exchange helper ------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import importlib
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    d = importlib.import_module("3dfacerecon_amd.utils.dist")
    d.init_from_env("gloo")
    t = (torch.arange(9 * 2 * 3, dtype=torch.float64).reshape(9, 2, 3) + 1000.0 * rank).requires_grad_(rank == 0)
    out = d.all_gather_stack(t)
    f = d.all_gather_stack(torch.full((3,), float(rank), dtype=torch.float32))
    strided = d.all_gather_stack((torch.arange(12, dtype=torch.float64) + 100.0 * rank).reshape(3, 4).t())   # not contiguous
    q.put((rank, tuple(out.shape), str(out.dtype), out.requires_grad, out.is_contiguous(), out.tolist(), f.tolist(),
           strided.tolist()))
    d.finalize()


def test_all_gather_stack_two_rank_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    base = torch.arange(54, dtype=torch.float64).reshape(9, 2, 3)
    want = torch.stack([base, base + 1000.0]).tolist()
    st = torch.arange(12, dtype=torch.float64).reshape(3, 4).t()
    for rank, shape, dtype, rg, contig, vals, f, strided in res:
        assert shape == (2, 9, 2, 3) and dtype == "torch.float64" and not rg and contig
        assert vals == want                                                  # rank order, the same on both ranks
        assert f == [[0.0] * 3, [1.0] * 3]
        assert strided == torch.stack([st, st + 100.0]).tolist()


def test_all_gather_stack_without_a_group():
    d = pkg("utils.dist")
    t = torch.arange(6, dtype=torch.float64).reshape(3, 2).requires_grad_(True)
    out = d.all_gather_stack(t)
    assert tuple(out.shape) == (1, 3, 2) and torch.equal(out[0], t.detach()) and not out.requires_grad
    assert out.data_ptr() == t.data_ptr()                                    # t[None]: a view, nothing is copied
