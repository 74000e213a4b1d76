"""The raw C entry points of the tri_ind consumers, called through ctypes on torch's current stream with buffers of the call's own:
the helpers the per-kernel GPU tests and the consumer fuzz (tests/test_fuzz_consumers_gpu.py) share.  Outputs are pre-filled with
NaN (or a sentinel), so an element a kernel did not write shows."""
import ctypes

import numpy as np
import torch

from conftest import pkg

DEV = "cuda:0"
SENT = 0x7FC12345   # a NaN no kernel produces
GAIN, OFFSET = 1.75, -0.125


def _h():
    return pkg("_lib")


def _t(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device=DEV)


def _stream(stream=None):
    return ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)


def _ws(ws, nws):
    """the call's own workspace of nws bytes, or `ws`: a uint8 device tensor of exactly nws bytes the caller placed and filled"""
    if ws is None:
        return torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() == nws, (ws.numel(), nws)
    return ws


def _sentinel(shape):
    return torch.full(shape, SENT, dtype=torch.int32, device=DEV).view(torch.float32)


# ---- fr_render_depth_backward_ws -------------------------------------------------------------------------------------------------------
def rbwd(g, tri, ti, nver, H, W, ws=None):
    """fr_render_depth_backward_ws on torch's current stream (device tensors; not synchronised) -> vertex_grad [B,3,nver], pre-filled
    with NaN"""
    h, L = _h(), _h().lib()
    B, ntri = int(ti.shape[0]), int(tri.shape[1])
    nws = L.fr_render_depth_backward_workspace_bytes(B, H, W)
    ws = _ws(ws, nws)
    out = torch.full((B, 3, nver), float("nan"), device=DEV)
    rc = L.fr_render_depth_backward_ws(h.ptr(g), h.ptr(tri), h.ptr(ti), h.ptr(out), B, nver, ntri, H, W, h.ptr(ws), nws, _stream())
    assert rc == 0, rc
    return out


# ---- fr_render_normal_backward ---------------------------------------------------------------------------------------------------------
def nbwd(g, V, tri, ti, H, W, mode, out=None, accumulate=0, stride=3, offset=0, pitch=None, ws=None):
    """fr_render_normal_backward on torch's current stream (device tensors; not synchronised) -> vertex_grad, pre-filled with
    NaN unless `out` is given"""
    h, L = _h(), _h().lib()
    B = int(V.shape[0])
    nver = int(V.shape[2]) if pitch is None else pitch[1]                     # pitch = (floats per vertex row, nver)
    ntri = int(tri.shape[1])
    nws = L.fr_render_normal_backward_workspace_bytes(B, nver, H, W)
    ws = _ws(ws, nws)
    if out is None:
        out = torch.full((B, 3, nver), float("nan"), device=DEV)
    rc = L.fr_render_normal_backward(ctypes.c_void_p(g.data_ptr() + 4 * offset), stride, h.ptr(V),
                                     nver if pitch is None else pitch[0], h.ptr(tri), h.ptr(ti), h.ptr(out), B, nver, ntri, H, W,
                                     mode, accumulate, h.ptr(ws), nws, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return out


# ---- fr_depth_interp_forward / fr_depth_interp_backward --------------------------------------------------------------------------------
def dfwd(V, tri, ti, H, W, pitch=None, stream=None):
    """fr_depth_interp_forward (device tensors; not synchronised) -> depth [B,H,W,1], pre-filled with NaN.
    pitch = (floats per vertex row, nver)"""
    h, L = _h(), _h().lib()
    B = int(V.shape[0])
    nver = int(V.shape[2]) if pitch is None else pitch[1]
    out = torch.full((B, H, W, 1), float("nan"), device=DEV)
    rc = L.fr_depth_interp_forward(h.ptr(V), nver if pitch is None else pitch[0], h.ptr(tri), h.ptr(ti), B, nver, int(tri.shape[1]),
                                   H, W, h.ptr(out), _stream(stream))
    assert rc == 0, rc
    return out


def dbwd(g, V, tri, ti, H, W, out=None, accumulate=0, pitch=None, stream=None, ws=None):
    """fr_depth_interp_backward with a workspace of its own -> vertex_grad, pre-filled with NaN unless `out` is given"""
    h, L = _h(), _h().lib()
    B = int(V.shape[0])
    nver = int(V.shape[2]) if pitch is None else pitch[1]
    nws = L.fr_depth_interp_backward_workspace_bytes(B, nver, H, W)
    ws = _ws(ws, nws)
    if out is None:
        out = torch.full((B, 3, nver), float("nan"), device=DEV)
    rc = L.fr_depth_interp_backward(h.ptr(g), h.ptr(V), nver if pitch is None else pitch[0], h.ptr(tri), h.ptr(ti), h.ptr(out), B,
                                    nver, int(tri.shape[1]), H, W, accumulate, h.ptr(ws), nws, _stream(stream))
    assert rc == 0, rc
    return out


# ---- fr_render_texture_backward --------------------------------------------------------------------------------------------------------
def tbwd(g, tri, ti, nver, H, W, tb, out=None, accumulate=0, stride=3, offset=0, ws=None):
    """fr_render_texture_backward on torch's current stream (device tensors; not synchronised) -> texture_grad [tb,3,nver],
    pre-filled with NaN unless `out` is given"""
    h, L = _h(), _h().lib()
    B = int(ti.shape[0])
    ntri = int(tri.shape[1])
    nws = L.fr_render_texture_backward_workspace_bytes(B, nver, H, W, tb)
    ws = _ws(ws, nws)
    if out is None:
        out = torch.full((tb, 3, nver), float("nan"), device=DEV)
    rc = L.fr_render_texture_backward(ctypes.c_void_p(g.data_ptr() + 4 * offset), stride, h.ptr(tri), h.ptr(ti), h.ptr(out), B, nver,
                                      ntri, H, W, tb, accumulate, h.ptr(ws), nws,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return out


# ---- fr_mesh_visible / fr_mesh_lift / fr_mesh_vertex_normals ---------------------------------------------------------------------------
def raw_visible(tri, tind, nver):
    h, L = _h(), _h().lib()
    B, H, W = tind.shape
    out = torch.full((B, nver), 7, dtype=torch.uint8, device=DEV)
    rc = L.fr_mesh_visible(h.ptr(tri) if tri.numel() else None, h.ptr(tind), B, nver, int(tri.shape[1]), H, W, h.ptr(out), _stream())
    assert rc == 0, rc
    return out


def raw_lift(vertex, nver, tind, vis, fine, coarse, ntri, out_pitch):
    """vertex [B,3,pitch] -> (vertex_out [B,3,out_pitch] pre-filled with the sentinel, state pre-filled with 7)"""
    h, L = _h(), _h().lib()
    B, H, W = tind.shape
    out = _sentinel((B, 3, out_pitch))
    state = torch.full((B, nver), 7, dtype=torch.uint8, device=DEV)
    rc = L.fr_mesh_lift(h.ptr(vertex), int(vertex.shape[2]), h.ptr(tind), h.ptr(vis), h.ptr(fine), h.ptr(coarse), B, nver, ntri, H,
                        W, h.ptr(out), out_pitch, h.ptr(state), _stream())
    assert rc == 0, rc
    return out, state


def raw_normals(vertex, nver, tri, adj, out_pitch):
    h, L = _h(), _h().lib()
    B = int(vertex.shape[0])
    out = _sentinel((B, 3, out_pitch))
    a0, a1 = _t(adj[0], np.int32), _t(adj[1], np.int32)
    rc = L.fr_mesh_vertex_normals(h.ptr(vertex), int(vertex.shape[2]), h.ptr(tri) if tri.numel() else None, h.ptr(a0),
                                  h.ptr(a1) if a1.numel() else None, B, nver, int(tri.shape[1]), h.ptr(out), out_pitch, _stream())
    assert rc == 0, rc
    return out


# ---- fr_photo_loss_forward / fr_photo_loss_backward ------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _tn(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=torch.device(DEV))


class PhotoCall:
    """the two entry points called directly, with buffers of the call's own (state, sums, gradients) on a given stream; every output
    is pre-filled with NaN"""
    ENTRY, NSUMS, LIGHT = "fr_photo_loss", 6, (4,)                          # the gray loss; PhotoRgbCall below is the colour one

    def __init__(self, planes, weighted, gain=GAIN, offset=OFFSET):
        tex, nrm, ti, light, target, weight = planes
        self.B, self.H, self.W = ti.shape[:3]
        self.t = [_tn(tex), _tn(nrm), _tn(ti), _tn(light), _tn(target), _tn(weight) if weighted else None]
        self.gain, self.offset = gain, offset
        self.L = pkg("_lib").lib()

    def forward(self, stream=None, state=None):
        dev = torch.device(DEV)
        st = torch.cuda.current_stream(dev) if stream is None else stream
        nst = getattr(self.L, self.ENTRY + "_state_bytes")(self.B, self.H, self.W)
        with torch.cuda.stream(st):
            if state is None:
                state = torch.full((nst,), 0xA5, dtype=torch.uint8, device=dev)   # (needs nothing cleared)
            assert state.dtype == torch.uint8 and state.numel() == nst
            sums = torch.full((self.B, self.NSUMS), float("nan"), dtype=torch.float64, device=dev)
            rc = getattr(self.L, self.ENTRY + "_forward")(*[_p(x) for x in self.t], self.B, self.H, self.W, self.gain, self.offset,
                                                          _p(sums), _p(state), nst, ctypes.c_void_p(st.cuda_stream))
        assert rc == 0
        self.keep = state
        return sums

    def backward(self, sums, g, want=(True, True, True), stream=None):
        dev = torch.device(DEV)
        st = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(st):
            nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)   # noqa: E731
            out = [nan(self.B, self.H, self.W, 3), nan(self.B, self.H, self.W, 3), nan(self.B, *self.LIGHT)]
            g_t = torch.as_tensor(np.asarray(g, np.float64), device=dev)
            rc = getattr(self.L, self.ENTRY + "_backward")(_p(g_t), _p(sums), *[_p(x) for x in self.t], self.B, self.H, self.W,
                                                           self.gain, self.offset, *[_p(o) if w else None for o, w in zip(out, want)],
                                                           ctypes.c_void_p(st.cuda_stream))
        assert rc == 0
        self.keep_g = g_t
        return out


class PhotoRgbCall(PhotoCall):
    """fr_photo_loss_rgb_forward / _backward the same way: 29 sums per face, light and grad_light [B,3,9], target [B,H,W,3]"""
    ENTRY, NSUMS, LIGHT = "fr_photo_loss_rgb", 29, (3, 9)


def assert_f64_bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d of %d float64 differ, first at %s: got %r want %r" % (
        what, bad.sum(), got.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


# ---- fr_coverage_forward / fr_coverage_backward ----------------------------------------------------------------------------------------
def cfwd(V, tri, ti, H, W, pitch=None):
    """fr_coverage_forward (device tensors; not synchronised) -> cov [B,H,W,1], pre-filled with NaN.
    pitch = (floats per vertex row, nver)"""
    h, L = _h(), _h().lib()
    B = int(V.shape[0])
    nver = int(V.shape[2]) if pitch is None else pitch[1]
    out = torch.full((B, H, W, 1), float("nan"), device=DEV)
    rc = L.fr_coverage_forward(h.ptr(V), nver if pitch is None else pitch[0], h.ptr(tri), h.ptr(ti), B, nver, int(tri.shape[1]), H, W,
                               h.ptr(out), _stream())
    assert rc == 0, rc
    return out


def cbwd(g, cov, V, tri, ti, H, W, out=None, accumulate=0, pitch=None, ws=None):
    """fr_coverage_backward with a workspace of its own -> vertex_grad, pre-filled with NaN unless `out` is given"""
    h, L = _h(), _h().lib()
    B = int(V.shape[0])
    nver = int(V.shape[2]) if pitch is None else pitch[1]
    nws = L.fr_coverage_backward_workspace_bytes(B, nver, H, W)
    ws = _ws(ws, nws)
    if out is None:
        out = torch.full((B, 3, nver), float("nan"), device=DEV)
    rc = L.fr_coverage_backward(h.ptr(g), h.ptr(cov), h.ptr(V), nver if pitch is None else pitch[0], h.ptr(tri), h.ptr(ti), h.ptr(out),
                                B, nver, int(tri.shape[1]), H, W, accumulate, h.ptr(ws), nws, _stream())
    assert rc == 0, rc
    return out


# ---- fr_albedo_basis_build / fr_albedo_lse_forward -------------------------------------------------------------------------------------
def raw_basis(tri, pc_tex, nver, ws=None):
    """fr_albedo_basis_build on a buffer of its own (tri [3,ntri], pc_tex [3 nver,K] device tensors) -> basis [ntri,K] float64,
    pre-filled with NaN; ws: the bytes to build into instead (the result is a view of them)"""
    L = _h().lib()
    ntri, K = int(tri.shape[1]), int(pc_tex.shape[1])
    if ws is None:
        out = torch.full((max(ntri, 1), K), float("nan"), dtype=torch.float64, device=DEV)[:ntri]
    else:
        out = _ws(ws, L.fr_albedo_basis_bytes(ntri, K)).view(torch.float64).view(ntri, K)
    rc = L.fr_albedo_basis_build(_p(tri), _p(pc_tex), nver, ntri, K, _p(out), L.fr_albedo_basis_bytes(ntri, K), _stream())
    assert rc == 0, rc
    return out


def raw_fit(inp, ridge, ws=None):
    """fr_albedo_lse_forward on buffers of its own, every output pre-filled with 7.0 (inp: device tensors basis [ntri,K] float64,
    tri_ind, lighting [3,H,W] float64, normal, abedo, im_gray) -> (alpha, stats, moments) as numpy, synchronised"""
    L = _h().lib()
    B, H, W = inp["tri_ind"].shape[:3]
    T, Kb = inp["basis"].shape
    alpha = torch.full((B, Kb), 7.0, dtype=torch.float32, device=DEV)
    moments = torch.full((B, 16, 16), 7.0, dtype=torch.float64, device=DEV)
    stats = torch.full((B, 4), 7.0, dtype=torch.float64, device=DEV)
    nws = L.fr_albedo_lse_workspace_bytes(B, H, W, Kb)
    ws = _ws(ws, nws)
    rc = L.fr_albedo_lse_forward(_p(inp["basis"]), _p(inp["tri_ind"]), _p(inp["lighting"]), _p(inp["normal"]), _p(inp["abedo"]),
                                 _p(inp["im_gray"]), B, T, H, W, Kb, float(ridge), _p(alpha), _p(moments), _p(stats), _p(ws), nws,
                                 _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return alpha.cpu().numpy(), stats.cpu().numpy(), moments.cpu().numpy()
