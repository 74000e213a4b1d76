"""One table of every caller-owned buffer whose size comes from a `fr_*_bytes` function of include/fr_hotpath.h -- workspaces,
forward-to-backward states, packed bases and images -- and the three promises the header makes about each: the call needs none of
the buffer cleared, writes nothing outside the stated bytes, and the stated alignment is enough.

A case is one (entry point, buffer) pair: the size function and its arguments per shape, the alignment the header states, and `run`,
which makes the raw C call(s) on a buffer it is GIVEN (a uint8 device tensor of exactly the stated bytes) and returns every output.
Where the buffer carries something between calls -- a backward reading the forward's state, render phases reading the table a pack
phase left, a consumer of a packed basis or image -- `run` makes the writer's call first and the reader's after it, with nothing
between the two.  The raw calls are the helpers of tests/raw_calls.py and of the per-kernel GPU test modules (imported where they are
used: this module itself imports without a GPU); an entry point that has no such helper is called here through ctypes.

Every case has the shapes "even" and "ragged" -- at "ragged" every divisor of the launch leaves a remainder, which
tests/test_workspace_cases_cpu.py holds against the entry's own fr_debug_*_geom hook -- and "large", which only lays leftovers.
tests/test_workspace_contract_gpu.py runs the table.  A NEW entry point that takes a sized buffer registers it here; the CPU test
fails for a `size_t fr_*_bytes(` of the header that is neither in the table nor in EXCLUDED with a reason."""
import ctypes
import functools

import numpy as np
import torch

from conftest import pkg

DEV = "cuda:0"
GUARD = 4096
GUARD_BYTE = 0xC3
FILLS = (("Z", 0x00), ("F", 0xFF), ("H", 0x7F))
# the guards hold another byte under every fill, so that a READ past either end of the buffer changes an output as well
GUARD_BYTES = {"Z": 0xC3, "F": 0x5A, "H": 0xA5, "L": 0x96}
NTRI = 90
# B, H, W, nver of the pixel-grid cases.  17 x 31 = 527 pixels: ragged against 64, 256 and 1,024.  `nver_owner`: the owner-scatter
# backwards give every vertex an owner of its own below ~97 vertices, so their ragged mesh is the smallest one whose owner ranges
# (2 .. 3 vertices, 129 for the texture backward) do not divide it.
DIM = {"even": dict(B=1, H=32, W=32, nver=64, nver_owner=64, K=9, S=32),
       "ragged": dict(B=3, H=17, W=31, nver=61, nver_owner=257, K=15, S=23),
       "large": dict(B=4, H=40, W=45, nver=130, nver_owner=517, K=15, S=40)}
SHAPES = ("even", "ragged")
EXCLUDED = {}            # size function -> why it has no case (an empty reason fails the CPU test)
# Entry points that take a sized buffer (a size_t byte count in _lib.SIGNATURES) and have no case of their own -> why.  A case names
# the entry points it calls in its name; the CPU test fails for an entry point that is neither named by a case nor listed here.
UNCASED = {
    "fr_decode_3dmm_q30": "the header defines it as fr_decode_3dmm_q30_lv at levels = 7, which is what both Q30 cases call",
    "fr_sfs_intensity_backward": "the header defines it as fr_sfs_intensity_backward_tex with a NULL grad_abedo_new: the case calls the _tex form",
    "fr_decode_render_forward": "one call that launches fr_decode_3dmm and fr_render_depth_forward_phases on the hand-off (the header: "
                                "bit-identical to the two calls); its three buffers are held through decode_rendering_layer_forward, which "
                                "shares its decode, hand-off and emit launches and differs in the resolver alone, and its callers "
                                "(pipeline.DecodeRenderPlan) own their buffers: nothing pooled reaches it",
    "fr_decode_render_forward_q30": "the same call with the Q30 decode in front: hand-off and render workspace as above, q_workspace is the "
                                    "staging buffer of the decode_3dmm_q30_lv case, handed to the same launcher",
    "fr_landmark_contour_select": "reads a landmark_basis_build image through the loader landmark_forward and landmark_backward use, and "
                                  "writes no sized buffer; its inputs are the line layouts of tests/test_landmark_contour_gpu.py",
}


def lib():
    return pkg("_lib").lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _t(a, dtype=np.float32):
    return torch.as_tensor(np.array(a, dtype), device=DEV)                    # (a copy: the shared inputs are read-only arrays)


def _full(shape, value=float("nan"), dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def hook(name, n, *args):
    """a fr_debug_*_geom hook (host code: no GPU) -> list of n ints"""
    out = (ctypes.c_int * n)()
    getattr(lib(), name)(*args, out)
    return list(out)


# ---- the two comparison helpers (tests/test_workspace_cases_cpu.py shows each able to fail) ----------------------------------------------
def bits(x):
    """a tensor or array -> its bit patterns, as a flat unsigned numpy array of the element's width"""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    a = np.ascontiguousarray(a).reshape(-1)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def bit_difference(got, want):
    """None when the two output dicts are equal BIT FOR BIT (a NaN equals only the same NaN; -0 is not +0), else a description"""
    if sorted(got) != sorted(want):
        return "outputs %s against %s" % (sorted(got), sorted(want))
    for k in sorted(want):
        g, w = bits(got[k]), bits(want[k])
        if g.dtype != w.dtype or g.shape != w.shape:
            return "%s: %s%s against %s%s" % (k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.flatnonzero(g != w)
        if bad.size:
            return "%s: %d of %d elements differ in their bits, first at %d: 0x%x against 0x%x" % (k, bad.size, g.size, bad[0], g[bad[0]],
                                                                                                  w[bad[0]])
    return None


def place(nbytes, align, device=DEV, guard_byte=GUARD_BYTE):
    """-> (whole, off): one uint8 tensor [slack | GUARD | nbytes | GUARD | slack] filled with guard_byte; whole[off:off + nbytes] starts
    at an address that is a multiple of `align` and of NO larger power of two"""
    whole = torch.full((nbytes + 2 * GUARD + 4 * align,), guard_byte, dtype=torch.uint8, device=device)
    off = GUARD + (align - (whole.data_ptr() + GUARD) % (2 * align)) % (2 * align)
    assert (whole.data_ptr() + off) % (2 * align) == align and off >= GUARD and off + nbytes + GUARD <= whole.numel()
    return whole, off


def guard_damage(whole, off, nbytes, guard_byte=GUARD_BYTE):
    """None when the GUARD bytes before and behind whole[off:off + nbytes] still hold guard_byte, else a description"""
    for name, g in (("before", whole[off - GUARD:off]), ("behind", whole[off + nbytes:off + nbytes + GUARD])):
        bad = torch.nonzero(g != guard_byte)
        if bad.numel():
            return "%d guard bytes %s the buffer were written, first at %+d" % (
                bad.shape[0], name, int(bad[0]) - (GUARD if name == "before" else -nbytes))
    return None


# ---- shared inputs: computed once per shape on the CPU, never written -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(shape, owner=False):
    """A rendered scene of about NTRI random triangles over `nver` points inside the image: numpy V [B,3,nver], tri [3,NTRI], tex
    [B,3,nver], the CPU oracle's planes (depth, tex_img, normal, tind) and pixel gradients g1 [B,H,W,1], g3 [B,H,W,3]."""
    from oracle import oracle as O
    d = DIM[shape]
    B, H, W, nver = d["B"], d["H"], d["W"], d["nver_owner" if owner else "nver"]
    rs = np.random.RandomState(1000 * B + nver + 7 * H)
    V = np.empty((B, 3, nver), np.float32)
    V[:, 0], V[:, 1], V[:, 2] = rs.uniform(0, W - 1, (B, nver)), rs.uniform(0, H - 1, (B, nver)), rs.uniform(1, 9, (B, nver))
    tri = np.stack([rs.choice(nver, 3, replace=False) for _ in range(NTRI)], axis=1).astype(np.float32)
    tri[:, 0] = (0, nver // 2, nver - 1)
    tex = rs.uniform(0.1, 0.9, (B, 3, nver)).astype(np.float32)
    depth, tex_img, normal, tind = O.render_depth(V, tri, tex, H, W)
    g1, g3 = rs.standard_normal((B, H, W, 1)).astype(np.float32), rs.standard_normal((B, H, W, 3)).astype(np.float32)
    g1[g1 == 0], g3[g3 == 0] = 1.0, 1.0
    im = rs.uniform(0.1, 1.0, (B, H, W, 1)).astype(np.float32)
    out = dict(B=B, H=H, W=W, nver=nver, V=V, tri=tri, tex=tex, depth=depth, tex_img=tex_img, normal=normal, tind=tind, g1=g1, g3=g3, im=im)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def scene_cover(shape, owner=False):
    return float((scene(shape, owner)["tind"] >= 0).mean())


@functools.lru_cache(maxsize=None)
def _scene_dev(shape, owner=False):
    return {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in scene(shape, owner).items()}


@functools.lru_cache(maxsize=None)
def assets(shape):
    """the decode entries' model: small_assets at "even" (480 vertices: whole tiles of 16), a 19 x 23 grid at "ragged" (437 = 27 tiles
    + 5 vertices, pitch 448) and a 25 x 30 one for the leftovers"""
    synth = pkg("utils.synth")
    return synth.make_small_assets() if shape == "even" else synth.make_small_assets(*((19, 23) if shape == "ragged" else (25, 30)))


def asset_dims(shape):
    A = assets(shape)
    return np.asarray(A["mu"]).size // 3, int(A["ndim_shape"]), int(A["ndim_exp"])


@functools.lru_cache(maxsize=None)
def decode_inputs(shape):
    """numpy P [B, 7 + ns + ne], the oracle's rotation R [B,3,3], vertices V [B,3,N] (the CPU oracle's decode) and a gradient G"""
    from oracle import oracle as O
    A, B = assets(shape), DIM[shape]["B"]
    N, ns, ne = asset_dims(shape)
    P = pkg("utils.synth").sample_params_batch(B, im_size=200, n_shape=ns, n_exp=ne, beta=0.7, seed=40 + B).astype(np.float32)
    R = O.rotation_matrix_batch(P[:, :3])
    V = O.decode_3dmm(P, A["mu"], A["pc_shape"], A["pc_exp"], 200.0, R=R)
    G = np.random.RandomState(N + B).standard_normal((B, 3, N)).astype(np.float32)
    return P, R.astype(np.float32), V, G


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
class Case:
    """name; size_fn: the fr_*_bytes function; args(shape) -> its arguments; align; run(shape, buf) -> {name: output}; ragged(shape) ->
    [(what, bool)] held at "ragged" on the CPU; other: (case name, shape) of the call that shares this buffer's pool kind and lays the
    leftovers (None: this case at "large"); cover(shape) -> share of covered pixels, or None where the entry has no pixels;
    ok: the outputs that must be 1 on every unit; anchor(shape, outs): holds the zero-filled run to an existing reference check"""

    def __init__(self, name, size_fn, args, align, run, ragged, other=None, cover=None, ok=(), anchor=None):
        self.name, self.size_fn, self.args, self.align, self.run, self.ragged = name, size_fn, args, align, run, ragged
        self.other, self.cover, self.ok, self.anchor = other, cover, ok, anchor

    def nbytes(self, shape):
        return int(getattr(lib(), self.size_fn)(*self.args(shape)))


CASES = {}


def case(name, size_fn, args, align, ragged, **kw):
    def register(run):
        assert name not in CASES
        CASES[name] = Case(name, size_fn, args, align, run, ragged, **kw)
        return run
    return register


def _dims(shape, *keys):
    return tuple(DIM[shape][k] for k in keys)


def _px(shape):
    B, H, W = _dims(shape, "B", "H", "W")
    return H * W


# ---- render forward: fr_render_depth_workspace_bytes ---------------------------------------------------------------------------------------
def _render_args(shape):
    B, H, W, nver = _dims(shape, "B", "H", "W", "nver")
    return B, nver, NTRI, H, W


def _render_ragged(shape):
    B, nver, ntri, H, W = _render_args(shape)
    rows, strips, segments, binned = hook("fr_debug_render_geom", 4, B, ntri, H, W, 0)
    return [("the binned rasteriser serves the shape", binned == 1), ("H %% %d rows per strip" % rows, rows > 0 and H % rows != 0),
            ("pixels % 64", (H * W) % 64 != 0), ("triangles % 64", ntri % 64 != 0)]


def _render_planes(B, H, W):
    return [_full((B, H, W, c)) for c in (1, 3, 3, 1)]


def _render_anchor(shape, outs):
    from gpu_util import assert_render_equal
    sc = scene(shape)
    assert_render_equal(tuple(outs[k].cpu().numpy() for k in ("depth", "tex_img", "normal", "tri_ind")),
                        (sc["depth"], sc["tex_img"], sc["normal"], sc["tind"]), "render " + shape)


def _render_call(shape, buf, phases_list):
    d = _scene_dev(shape)
    B, nver, ntri, H, W = _render_args(shape)
    o = _render_planes(B, H, W)
    for ph in phases_list:
        rc = lib().fr_render_depth_forward_phases(_p(d["V"]), _p(d["tri"]), _p(d["tex"]), B, nver, ntri, H, W, 3, B, *[_p(x) for x in o],
                                                  _p(buf), buf.numel(), _st(), ph)
        assert rc == 0, (rc, ph)
    return dict(zip(("depth", "tex_img", "normal", "tri_ind"), o))


@case("render_depth_forward", "fr_render_depth_workspace_bytes", _render_args, 16, _render_ragged, cover=scene_cover, anchor=_render_anchor)
def _(shape, buf):
    d = _scene_dev(shape)
    B, nver, ntri, H, W = _render_args(shape)
    o = _render_planes(B, H, W)
    rc = lib().fr_render_depth_forward(_p(d["V"]), _p(d["tri"]), _p(d["tex"]), B, nver, ntri, H, W, 3, B, *[_p(x) for x in o], _p(buf),
                                       buf.numel(), _st())
    assert rc == 0, rc
    return dict(zip(("depth", "tex_img", "normal", "tri_ind"), o))


@case("render_depth_forward_phases[pack, then emit + resolve]", "fr_render_depth_workspace_bytes", _render_args, 16, _render_ragged,
      cover=scene_cover, anchor=_render_anchor)
def _(shape, buf):
    return _render_call(shape, buf, (4, 3))


@case("rendering_layer_forward", "fr_render_depth_workspace_bytes", _render_args, 16, _render_ragged, cover=scene_cover)
def _(shape, buf):
    d = _scene_dev(shape)
    B, nver, ntri, H, W = _render_args(shape)
    o = [_full((B, H, W, 7))] + [_full((B, H, W, 1)) for _ in range(3)]
    rc = lib().fr_rendering_layer_forward(_p(d["V"]), _p(d["tri"]), _p(d["tex"]), _p(d["im"]), B, nver, ntri, H, W, B, *[_p(x) for x in o],
                                          _p(buf), buf.numel(), _st())
    assert rc == 0, rc
    return dict(zip(("net_input", "depth_img", "depth", "tri_ind"), o))


@case("rendering_layer_forward_phases[pack, then emit + resolve]", "fr_render_depth_workspace_bytes", _render_args, 16, _render_ragged,
      cover=scene_cover)
def _(shape, buf):
    d = _scene_dev(shape)
    B, nver, ntri, H, W = _render_args(shape)
    o = [_full((B, H, W, 7))] + [_full((B, H, W, 1)) for _ in range(3)]
    for ph in (4, 3):
        rc = lib().fr_rendering_layer_forward_phases(_p(d["V"]), _p(d["tri"]), _p(d["tex"]), _p(d["im"]), B, nver, ntri, H, W, B,
                                                     *[_p(x) for x in o], _p(buf), buf.numel(), _st(), ph)
        assert rc == 0, (rc, ph)
    return dict(zip(("net_input", "depth_img", "depth", "tri_ind"), o))


# ---- the owner-scatter backwards (csrc/fr_owner_scatter.h): 1,024-pixel record chunks, owner ranges of vertices ------------------------------
def _owner_ragged(hook_name, tb=None):
    def ragged(shape):
        B, H, W, nver = _dims(shape, "B", "H", "W", "nver_owner")
        g = hook(hook_name, 7, *((B, nver, H, W) if tb is None else (B, nver, H, W, tb(B))))
        out = [("pixels % 1024", (H * W) % 1024 != 0), ("nver %% owner range %d" % g[1], g[1] > 0 and nver % g[1] != 0)]
        if tb is not None and tb(B) == 1:
            out.append(("face slices %d" % g[6], g[6] > 1))
        return out
    return ragged


def _owner_cover(shape):
    return scene_cover(shape, True)


def _bwd_ws_args(shape):
    return _dims(shape, "B", "H", "W")


def _owner_args(shape):
    return _dims(shape, "B", "nver_owner", "H", "W")


def _rbwd_anchor(shape, outs):
    import ref_render_bwd_model as R
    sc = scene(shape, True)
    M = R.model(sc["g1"], sc["tri"], sc["tind"], sc["nver"], sc["H"], sc["W"])
    assert not M.bad.any()
    np.testing.assert_array_equal(outs["vertex_grad"].cpu().numpy().view(np.uint32), M.bits)


@case("render_depth_backward_ws", "fr_render_depth_backward_workspace_bytes", _bwd_ws_args, 16, _owner_ragged("fr_debug_render_bwd_geom"),
      cover=_owner_cover, anchor=_rbwd_anchor)
def _(shape, buf):
    from raw_calls import rbwd
    d = _scene_dev(shape, True)
    return {"vertex_grad": rbwd(d["g1"], d["tri"], d["tind"], d["nver"], d["H"], d["W"], ws=buf)}


def _bound_anchor(model_of):
    def anchor(shape, outs):
        import ref_normal_backward as RN
        worst = RN.check_bound(outs["vertex_grad"].cpu().numpy(), model_of(shape, scene(shape, True)))
        print("%s: worst error / bound %.3f" % (shape, worst))
        assert worst <= 1.0
    return anchor


def _nbwd_model(shape, sc):
    import ref_normal_backward as RN
    return RN.model(sc["g3"], sc["V"], sc["tri"], sc["tind"], sc["H"], sc["W"], 0)


@case("render_normal_backward", "fr_render_normal_backward_workspace_bytes", _owner_args, 16,
      _owner_ragged("fr_debug_render_normal_bwd_geom"), cover=_owner_cover, anchor=_bound_anchor(_nbwd_model))
def _(shape, buf):
    from raw_calls import nbwd
    d = _scene_dev(shape, True)
    return {"vertex_grad": nbwd(d["g3"], d["V"], d["tri"], d["tind"], d["H"], d["W"], 0, ws=buf)}


def _dbwd_model(shape, sc):
    import ref_depth_interp as RD
    return RD.model(sc["g1"], sc["V"], sc["tri"], sc["tind"], sc["H"], sc["W"])


@case("depth_interp_backward", "fr_depth_interp_backward_workspace_bytes", _owner_args, 16, _owner_ragged("fr_debug_depth_interp_bwd_geom"),
      cover=_owner_cover, anchor=_bound_anchor(_dbwd_model))
def _(shape, buf):
    from raw_calls import dbwd
    d = _scene_dev(shape, True)
    return {"vertex_grad": dbwd(d["g1"], d["V"], d["tri"], d["tind"], d["H"], d["W"], ws=buf)}


@functools.lru_cache(maxsize=None)
def _coverage_plane(shape):
    import ref_coverage as RC
    sc = scene(shape, True)
    return RC.forward(sc["V"], sc["tri"], sc["tind"], sc["H"], sc["W"])


def _cbwd_model(shape, sc):
    import ref_coverage as RC
    return RC.model(sc["g1"], _coverage_plane(shape), sc["V"], sc["tri"], sc["tind"], sc["H"], sc["W"])


@case("coverage_backward", "fr_coverage_backward_workspace_bytes", _owner_args, 16, _owner_ragged("fr_debug_coverage_bwd_geom"),
      cover=_owner_cover, anchor=_bound_anchor(_cbwd_model))
def _(shape, buf):
    from raw_calls import cbwd, cfwd
    d = _scene_dev(shape, True)
    cov = cfwd(d["V"], d["tri"], d["tind"], d["H"], d["W"])
    return {"vertex_grad": cbwd(d["g1"], cov, d["V"], d["tri"], d["tind"], d["H"], d["W"], ws=buf)}


def _tbwd_case(name, tb):
    def args(shape):
        B, nver, H, W = _owner_args(shape)
        return B, nver, H, W, tb(B)

    def anchor(shape, outs):
        import ref_texture_backward as RT
        from gpu_util import assert_bits_equal
        sc = scene(shape, True)
        M = RT.model(sc["g3"], sc["tri"], sc["tind"], sc["nver"], sc["H"], sc["W"], tb(sc["B"]))
        assert not M.bad.any()
        assert_bits_equal(outs["texture_grad"].cpu().numpy(), M.value(), name)

    @case(name, "fr_render_texture_backward_workspace_bytes", args, 16, _owner_ragged("fr_debug_render_texture_bwd_geom", tb),
          cover=_owner_cover, anchor=anchor)
    def _(shape, buf):
        from raw_calls import tbwd
        d = _scene_dev(shape, True)
        return {"texture_grad": tbwd(d["g3"], d["tri"], d["tind"], d["nver"], d["H"], d["W"], tb(d["B"]), ws=buf)}


_tbwd_case("render_texture_backward[a texture per face]", lambda B: B)
_tbwd_case("render_texture_backward[one shared texture]", lambda B: 1)


# ---- decode: the packed bases and images, the Q30 staging buffer, the backward's slabs ------------------------------------------------------
def _basis_args(shape):
    return asset_dims(shape)


def _decode_ragged(shape):
    N, ns, ne = asset_dims(shape)
    pitch = lib().fr_decode_render_vertex_pitch(N)
    rows = hook("fr_debug_decode_bwd_geom", 7, DIM[shape]["B"], N, ns, ne)[4]
    return [("N % 16", N % 16 != 0), ("N != hand-off pitch %d" % pitch, pitch != N), ("(ns + ne) % 16", (ns + ne) % 16 != 0),
            ("3 N %% %d rows per GEMM workgroup" % rows, rows > 0 and (3 * N) % rows != 0)]


def _basis_tensors(shape):
    A = assets(shape)
    return _t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"])


def _decode_anchor(shape, outs):
    np.testing.assert_array_equal(outs["vertex_proj"].cpu().numpy(), decode_inputs(shape)[2])


@case("decode_pack_basis -> decode_3dmm", "fr_decode_packed_basis_bytes", _basis_args, 16, _decode_ragged, anchor=_decode_anchor)
def _(shape, buf):
    N, ns, ne = asset_dims(shape)
    mu, pcs, pce = _basis_tensors(shape)
    P, R, _, _ = decode_inputs(shape)
    B = P.shape[0]
    assert lib().fr_decode_pack_basis(_p(mu), _p(pcs), _p(pce), N, ns, ne, _p(buf), buf.numel(), _st()) == 0
    out, Pt, Rt = _full((B, 3, N)), _t(P), _t(R)
    assert lib().fr_decode_3dmm(_p(Pt), _p(buf), _p(Rt), B, N, ns, ne, 200.0, _p(out), _st()) == 0
    return {"vertex_proj": out}


@functools.lru_cache(maxsize=None)
def _qrig(shape):
    from test_decode_q30_edges_gpu import QRig
    A = assets(shape)
    N, ns, ne = asset_dims(shape)
    return QRig(ns, ne, N, arrays=(np.asarray(A["mu"]).reshape(-1), A["pc_shape"], A["pc_exp"]))


def _q30_ragged(shape):
    N, ns, ne = asset_dims(shape)
    B = DIM[shape]["B"]
    g = (ctypes.c_int * (1 + 10 * ((B + 63) // 64)))()
    assert lib().fr_debug_decode_q_geom(B, N, ns, ne, 7, 256, g) == 0
    return [("one pass", g[0] == 1), ("live columns %d %% 16 per column block" % g[2], g[2] == B and g[2] % 16 != 0), ("N % 16", N % 16 != 0),
            ("(ns + ne) % 16", (ns + ne) % 16 != 0)]


def _q30_anchor(shape, outs):
    from gpu_util import assert_bits_equal
    from oracle import oracle as O
    P, R, _, _ = decode_inputs(shape)
    assert_bits_equal(outs["vertex_proj"], _qrig(shape).oracle(O, P, R, 7, 200.0), "Q30 decode " + shape)


@case("decode_q30_pack -> decode_3dmm_q30_lv", "fr_decode_q30_image_bytes", _basis_args, 256, _q30_ragged, anchor=_q30_anchor)
def _(shape, buf):
    g = _qrig(shape)
    P, R, _, _ = decode_inputs(shape)
    g.pack_into(_p(buf), buf.numel())
    return {"vertex_proj": g.decode(P, R, qimage=buf, im=200.0)}


@case("decode_3dmm_q30_lv", "fr_decode_q30_workspace_bytes", lambda shape: asset_dims(shape)[1:], 16, _q30_ragged, anchor=_q30_anchor)
def _(shape, buf):
    P, R, _, _ = decode_inputs(shape)
    return {"vertex_proj": _qrig(shape).decode(P, R, ws=buf, im=200.0)}


@functools.lru_cache(maxsize=None)
def _brig(shape):
    from test_decode_backward_bounds_gpu import Rig
    return Rig(assets(shape))


def _decode_bwd_args(shape):
    return (DIM[shape]["B"],) + asset_dims(shape)


_BWD_ENTRY = {"ref": "decode_3dmm_backward", "packed": "decode_3dmm_backward_packed", "mu": "decode_3dmm_backward_packed_mu"}


@functools.lru_cache(maxsize=None)
def _decode_bwd_ref(shape):
    """tests/test_decode_backward_bounds_gpu.py's float64 reference of the shape's inputs, with the magnitudes behind its bound"""
    from oracle import oracle as O
    from test_decode_backward_bounds_gpu import Ref
    P, R, _, G = decode_inputs(shape)
    return Ref(O, assets(shape), P, G, R=R)


def _decode_bwd_anchor(kind):
    """that module's proven bound, under the summation depths of the launch the launcher's own geometry hook reports"""
    def anchor(shape, outs):
        from test_decode_backward_bounds_gpu import _check, _depths
        P, _, V, _ = decode_inputs(shape)
        r = _check(outs["grad_params"], _decode_bwd_ref(shape), _depths(kind, _brig(shape), P.shape[0]), kind, Vg=V,
                   tag="workspace %s|%s" % (shape, kind))
        print("%s %s: worst error / bound %.3g" % (kind, shape, float(r.max())))
    return anchor


def _decode_bwd_case(kind, other):
    @case(_BWD_ENTRY[kind], "fr_decode_backward_workspace_bytes", _decode_bwd_args, 16, _decode_ragged, other=(_BWD_ENTRY[other], "large"),
          anchor=_decode_bwd_anchor(kind))
    def _(shape, buf):
        from test_decode_backward_bounds_gpu import IM
        assert IM == 200.0
        P, R, V, G = decode_inputs(shape)
        return {"grad_params": _brig(shape).call(kind, P, G, _t(V), R, ws=buf)}


_decode_bwd_case("ref", "packed")        # (the three entry points share PackedBasis.backward_workspace's pool, keyed by the byte count)
_decode_bwd_case("packed", "ref")
_decode_bwd_case("mu", "ref")


@case("decode_backward_pack_basis -> decode_3dmm_backward_packed", "fr_decode_backward_basis_bytes", _basis_args, 16, _decode_ragged,
      anchor=_decode_bwd_anchor("packed"))
def _(shape, buf):
    N, ns, ne = asset_dims(shape)
    _, pcs, pce = _basis_tensors(shape)
    P, R, V, G = decode_inputs(shape)
    assert lib().fr_decode_backward_pack_basis(_p(pcs), _p(pce), N, ns, ne, _p(buf), buf.numel(), _st()) == 0
    rig = _brig(shape)
    basis = rig.net._basis
    basis.image_t()
    keep, basis._image_t = basis._image_t, buf           # (the rig's call reads the image the basis holds: hand it this one)
    try:
        return {"grad_params": rig.call("packed", P, G, _t(V), R)}
    finally:
        basis._image_t = keep


def _pose_args(shape):
    return DIM[shape]["B"], {"even": 2048, "ragged": 4270, "large": 6000}[shape]


def _pose_ragged(shape):
    B, N = _pose_args(shape)
    g = hook("fr_debug_pose_bwd_geom", 4, B, N)
    return [("N %% chunk %d" % g[0], N % g[0] != 0), ("chunks per face", g[1] > 1), ("N % 16", N % 16 != 0)]


@functools.lru_cache(maxsize=None)
def _pose_case(shape):
    import ref_pose_backward as RP
    B, N = _pose_args(shape)
    return RP.make_case(77 + B, B, N, None, False)


@case("decode_pose_backward", "fr_decode_pose_backward_workspace_bytes", _pose_args, 16, _pose_ragged)
def _(shape, buf):
    from test_pose_backward_gpu import pose_c
    c = _pose_case(shape)
    gp, gR = pose_c(_t(c["G"]), _t(c["Vg"]), _t(c["P"]), None, fill=0.0, ws=buf)
    return {"grad_params": gp, "grad_R": gR}


# ---- decode -> rendering layer: the hand-off, the render workspace behind the fused decode, the two fused backwards -----------------------
@functools.lru_cache(maxsize=None)
def _lrig(shape):
    from test_decode_layer_gpu import Rig
    H, W = _dims(shape, "H", "W")
    return Rig(assets(shape), H, W, im_size=max(H, W))


def layer_params(shape):
    """parameters under which the small mesh fills a good part of the H x W image (tests/test_decode_layer_gpu.py::_params' recipe)"""
    B, H, W = _dims(shape, "B", "H", "W")
    N, ns, ne = asset_dims(shape)
    P = pkg("utils.synth").sample_params_batch(B, im_size=max(H, W), n_shape=ns, n_exp=ne, beta=0.7, seed=60 + B).astype(np.float32)
    P[:, 0:3] *= 0.3
    P[:, 6] = np.float32(2.0e-4) * (1.0 + 0.1 * (np.arange(B) % 3)) * max(H, W) / 45.0
    P[:, 3] = W / 2.0
    P[:, 4] = max(H, W) - H / 2.0
    return P


@functools.lru_cache(maxsize=None)
def layer_cover(shape):
    from oracle import oracle as O
    A = assets(shape)
    H, W = _dims(shape, "H", "W")
    V = O.decode_3dmm(layer_params(shape), A["mu"], A["pc_shape"], A["pc_exp"], float(max(H, W)))
    return float((O.render_depth(V, A["tri"], A["vertex"][None], H, W)[3] >= 0).mean())


def _layer_ragged(shape):
    return _decode_ragged(shape) + [("pixels % 64", _px(shape) % 64 != 0)]


def _layer_forward(shape, **bufs):
    rig = _lrig(shape)
    im = _t(scene(shape)["im"])
    return rig, dict(zip(("net_input", "depth_img", "depth", "tri_ind"), rig.fwd_fused(_t(layer_params(shape)), im, **bufs)))


def _layer_anchor(shape, outs):
    from oracle import oracle as O
    from test_decode_layer_gpu import _oracle_forward
    _oracle_forward(O, _lrig(shape), _t(layer_params(shape)), _t(scene(shape)["im"]), range(DIM[shape]["B"]),
                    tuple(outs[k] for k in ("net_input", "depth_img", "depth", "tri_ind")))


@case("decode_rendering_layer_forward[hand-off]", "fr_decode_render_vertex_bytes", lambda s: (DIM[s]["B"], asset_dims(s)[0]), 128,
      _layer_ragged, cover=layer_cover, anchor=_layer_anchor)
def _(shape, buf):
    rig, outs = _layer_forward(shape, hand=buf)
    B, N = DIM[shape]["B"], rig.N
    outs["hand-off"] = buf.view(torch.float32).view(B, 3, -1)[:, :, :N].clone()      # (the pad floats are never written or read)
    return outs


@case("decode_rendering_layer_forward[render workspace]", "fr_render_depth_workspace_bytes",
      lambda s: (DIM[s]["B"], asset_dims(s)[0], int(np.asarray(assets(s)["tri"]).shape[1]), DIM[s]["H"], DIM[s]["W"]), 16, _layer_ragged,
      cover=layer_cover, anchor=_layer_anchor)
def _(shape, buf):
    return _layer_forward(shape, ws=buf)[1]


@functools.lru_cache(maxsize=None)
def _pscene(shape):
    """tests/test_pose_backward_gpu.py's scene (the 70 x 61 mesh, N = 4,270 = 266 tiles + 14 vertices) rendered at S x S, with its
    forward's planes and hand-off (buffers of the forward's own)"""
    import ref_pose_backward as RP
    from test_pose_backward_gpu import Scene
    B, S = _dims(shape, "B", "S")
    sc = Scene(pkg("utils.synth").make_assets(70, 61, RP.NS, RP.NE, patch=None, seed_basis=4270), B=B, S=S)
    P = sc.Pn.copy()                                             # (the scene's pose is for 40 x 40: keep the face on the S x S image)
    P[:, 3:5] *= S / 40.0
    P[:, 6] *= S / 40.0
    sc.Pn, sc.P = P, _t(P)
    return sc, sc.forward()


def _pscene_cover(shape):
    return float((_pscene(shape)[1][1] >= 0).float().mean())


def _fused_bwd_args(shape):
    import ref_pose_backward as RP
    B, S = _dims(shape, "B", "S")
    return B, 4270, RP.NS, RP.NE, S, S


def _fused_bwd_ragged(shape):
    S = DIM[shape]["S"]
    return [("pixels % 1024", (S * S) % 1024 != 0), ("pixels % 64", (S * S) % 64 != 0), ("N % 16", 4270 % 16 != 0),
            ("N % pose chunk", 4270 % hook("fr_debug_pose_bwd_geom", 4, 1, 4270)[0] != 0)]


def _fused_bwd_case(name, size_fn, pose, other):
    @case(name, size_fn, _fused_bwd_args, 256, _fused_bwd_ragged, other=(other, "large"), cover=_pscene_cover)
    def _(shape, buf):
        sc, (depth, tri_ind, hand) = _pscene(shape)
        gp, gR = sc.bwd(depth, tri_ind, hand, pose=pose, ws=buf)
        return {"grad_params": gp, "grad_R": gR} if pose else {"grad_params": gp}


_fused_bwd_case("decode_render_backward", "fr_decode_render_backward_workspace_bytes", False, "decode_render_backward_pose")   # ("bwd")
_fused_bwd_case("decode_render_backward_pose", "fr_decode_render_backward_pose_workspace_bytes", True, "decode_render_backward")


# ---- shape from shading: the state, and the moment and q parts of the split route ------------------------------------------------------------
# (B, H, W) and the seed of tests/ref_sfs.py::inputs.  The model's bounds need its eigenvalue-gap condition (no pixel whose 3 x 3 moment
# matrix is nearly singular); no seed meets it at 17 x 31 with fewer than seven faces, and the batch is cut into more than one slice from
# eight faces on: the ragged batch is 9 (two slices, of 5 and 4 faces), not 3.
SFS = {"even": ((1, 32, 32), 1), "ragged": ((9, 17, 31), 1), "large": ((10, 40, 45), 1)}


@functools.lru_cache(maxsize=None)
def sfs_inputs(shape):
    """-> (tests/ref_sfs.py's inputs: abedo, normal, im_gray, abedo_new, normal_new; the gradient of the intensity)"""
    import ref_sfs as RS
    dims, seed = SFS[shape]
    return RS.inputs(*dims, seed=seed), RS.grad_out(*dims, seed=seed)


def sfs_cover(shape):
    return float(sfs_inputs(shape)[0]["normal"].any(-1).mean())


@functools.lru_cache(maxsize=None)
def _sfs_dev(shape):
    d, g = sfs_inputs(shape)
    return {k: _t(v) for k, v in d.items()}, _t(g)


@functools.lru_cache(maxsize=None)
def _sfs_model(shape):
    """what tests/test_sfs_sharded_gpu.py's checks read of a case: shape, d, g and the float64 model m"""
    import types

    import ref_sfs as RS
    d, g = sfs_inputs(shape)
    return types.SimpleNamespace(shape=SFS[shape][0], d=d, g=g, m=RS.model(*RS.args(d)))


def _sfs_anchor(shape, outs):
    from test_sfs_sharded_gpu import _check_backward, _check_forward
    c = _sfs_model(shape)
    if "intensity" in outs:
        _check_forward(c, outs["intensity"], outs["state"])
    if "grad_abedo_new" in outs:
        _check_backward(c, outs["grad_normal"], outs["grad_normal_new"], outs["grad_abedo_new"])


def _sfs_ragged_by(hook_name, n):
    def ragged(shape):
        B, H, W = SFS[shape][0]
        g = hook(hook_name, n, B, H, W)
        return [("pixels %% %d per workgroup" % g[0], g[0] > 0 and (H * W) % g[0] != 0), ("faces %% %d slices" % g[1], g[1] > 1 and B % g[1] != 0)]
    return ragged


_sfs_ragged, _sfs_split_ragged = _sfs_ragged_by("fr_debug_sfs_geom", 4), _sfs_ragged_by("fr_debug_sfs_split_geom", 6)


def _hw(shape):
    return SFS[shape][0][1:]


@case("sfs_intensity_forward -> sfs_intensity_backward_tex", "fr_sfs_state_bytes", _hw, 16, _sfs_ragged, cover=sfs_cover, anchor=_sfs_anchor)
def _(shape, buf):
    from test_sfs_gpu import fwd
    from test_sfs_sharded_gpu import one_bwd
    t, g = _sfs_dev(shape)
    B, H, W = SFS[shape][0]
    state = buf.view(torch.float64).view(10, H, W)
    out, _ = fwd(t, state=state)
    o = one_bwd(g, t, state, (B, H, W))
    return dict(zip(("intensity", "state", "grad_normal", "grad_normal_new", "grad_abedo_new"), [out, state.clone()] + list(o)))


@case("sfs_moments -> sfs_solve_shade, sfs_lighting", "fr_sfs_moments_bytes", _hw, 16, _sfs_split_ragged, cover=sfs_cover, anchor=_sfs_anchor)
def _(shape, buf):
    from test_sfs_sharded_gpu import moments, solve_shade
    t, _g = _sfs_dev(shape)
    B, H, W = SFS[shape][0]
    m = moments(t, (B, H, W), m=buf.view(torch.float64).view(9, H, W))
    out, state = solve_shade(m[None], t, (B, H, W))
    light = _full((10, H, W), dtype=torch.float64)
    assert lib().fr_sfs_lighting(_p(m), 1, H, W, 1e-6, _p(light), light.numel() * 8, _st()) == 0
    return {"intensity": out, "state": state, "lighting state": light}


@case("sfs_backward_q -> sfs_backward_apply", "fr_sfs_q_bytes", _hw, 16, _sfs_split_ragged, cover=sfs_cover, anchor=_sfs_anchor)
def _(shape, buf):
    from test_sfs_sharded_gpu import backward_apply, backward_q, one_fwd
    t, g = _sfs_dev(shape)
    B, H, W = SFS[shape][0]
    _, state = one_fwd(t, (B, H, W))
    q = backward_q(g, t, (B, H, W), q=buf.view(torch.float64).view(3, H, W))
    o = backward_apply(g, t, state, q[None], (B, H, W))
    return dict(zip(("grad_normal", "grad_normal_new", "grad_abedo_new"), o))


@case("sfs_solve_shade -> sfs_backward_apply", "fr_sfs_state_bytes", _hw, 16, _sfs_split_ragged, cover=sfs_cover, anchor=_sfs_anchor)
def _(shape, buf):
    from test_sfs_sharded_gpu import backward_apply, backward_q, moments, solve_shade
    t, g = _sfs_dev(shape)
    B, H, W = SFS[shape][0]
    state = buf.view(torch.float64).view(10, H, W)
    out, _ = solve_shade(moments(t, (B, H, W))[None], t, (B, H, W), state=state)
    o = backward_apply(g, t, state, backward_q(g, t, (B, H, W))[None], (B, H, W))
    return dict(zip(("intensity", "state", "grad_normal", "grad_normal_new", "grad_abedo_new"), [out, state.clone()] + list(o)))


# ---- Gram-form geometry loss ------------------------------------------------------------------------------------------------------------------
def _gram_dims(shape):
    return {"even": (1024, 16, 0), "ragged": (437, 9, 5), "large": (2500, 40, 9)}[shape]          # (N, ns, ne)


def _gram_ragged(shape):
    N, ns, ne = _gram_dims(shape)
    g = hook("fr_debug_geometry_gram_geom", 6, N, ns, ne)
    return [("rows %% chunk %d" % g[0], (3 * N) % g[0] != 0), ("chunks", g[1] > 1), ("K % 16", (ns + ne) % 16 != 0)]


@functools.lru_cache(maxsize=None)
def _gram_in(shape):
    import ref_geometry_gram as RG
    N, ns, ne = _gram_dims(shape)
    return RG.basis(N, ns, ne) + (RG.diffs(DIM[shape]["B"], ns, ne),)


def _gram_run(shape, **bufs):
    from test_geometry_gram_gpu import build_gram, loss_fwd_bwd
    N, ns, ne = _gram_dims(shape)
    pcs, pce, diff = _gram_in(shape)
    G = build_gram(pcs, pce, **bufs)
    loss, (gd,) = loss_fwd_bwd(G, diff, N, ns, ne)
    return {"gram": G, "loss": loss, "grad_diff": gd}


def _gram_anchor(shape, outs):
    from test_geometry_gram_gpu import _check_gram
    pcs, pce, _ = _gram_in(shape)
    _check_gram(outs["gram"], pcs, pce, "gram " + shape)


@case("geometry_gram_build[gram] -> geometry_loss_forward", "fr_geometry_gram_bytes", lambda s: _gram_dims(s)[1:], 16, _gram_ragged,
      anchor=_gram_anchor)
def _(shape, buf):
    return _gram_run(shape, G=buf)


@case("geometry_gram_build[workspace]", "fr_geometry_gram_workspace_bytes", _gram_dims, 16, _gram_ragged, anchor=_gram_anchor)
def _(shape, buf):
    return _gram_run(shape, ws=buf)


@functools.lru_cache(maxsize=None)
def _gram_of(shape):
    from test_geometry_gram_gpu import build_gram
    pcs, pce, _ = _gram_in(shape)
    return build_gram(pcs, pce)


def _gram_loss_anchor(shape, outs):
    """the loss and its gradient bit for bit against the model fed the GPU's own G (tests/test_geometry_gram_gpu.py, part 2)"""
    import ref_geometry_gram as RG
    from gpu_util import assert_bits_equal
    N = _gram_dims(shape)[0]
    y, _, _, loss = RG.forward(_gram_in(shape)[2], _gram_of(shape), N)
    assert_bits_equal(outs["loss"], loss, "loss")
    assert_bits_equal(outs["grad_diff"], RG.backward(1.0, y, N), "grad_diff")


@case("geometry_loss_forward -> geometry_loss_backward", "fr_geometry_loss_state_bytes", lambda s: (DIM[s]["B"],) + _gram_dims(s)[1:], 16,
      _gram_ragged, anchor=_gram_loss_anchor)
def _(shape, buf):
    from test_geometry_gram_gpu import loss_fwd_bwd
    N, ns, ne = _gram_dims(shape)
    loss, (gd,) = loss_fwd_bwd(_gram_of(shape), _gram_in(shape)[2], N, ns, ne, state=buf)
    return {"loss": loss, "grad_diff": gd}


# ---- fine-depth losses ------------------------------------------------------------------------------------------------------------------------
def _bhw(shape):
    return _dims(shape, "B", "H", "W")


def _fine_ragged(shape):
    B, H, W = _bhw(shape)
    g = hook("fr_debug_fine_losses_geom", 7, B, H, W)
    return [("W %% tile width %d" % g[0], W % g[0] != 0), ("H %% tile height %d" % g[1], H % g[1] != 0)]


@functools.lru_cache(maxsize=None)
def _fine_in(shape):
    import ref_fine_losses as RF
    z, c, _ = RF.inputs(*_bhw(shape))
    return z, c


def _fine_anchor(shape, outs):
    import ref_fine_losses as RF
    from gpu_util import assert_bits_equal
    from test_fine_losses_gpu import assert_bits64_equal
    want = RF.forward(*_fine_in(shape))
    P = want["part_f"].size
    assert_bits64_equal(outs["state"][2:2 + P], want["part_f"], "fidelity partials")
    assert_bits64_equal(outs["state"][2 + P:], want["part_s"], "smoothness partials")
    assert_bits64_equal(outs["state"][:2], [want["S_f"], want["S_s"]], "S_f, S_s")
    assert_bits_equal(outs["fidelity"], want["fidelity"], "fidelity")
    assert_bits_equal(outs["smoothness"], want["smoothness"], "smoothness")


@case("fine_losses_forward", "fr_fine_losses_state_bytes", _bhw, 16, _fine_ragged, anchor=_fine_anchor)
def _(shape, buf):
    from test_fine_losses_gpu import raw_forward
    fid, sm, state = raw_forward(*_fine_in(shape), state=buf)
    return {"fidelity": fid, "smoothness": sm, "state": state}


# ---- the tile kernels: 256 pixels per tile, 4 tiles per workgroup (albedo fit, colour solve), the photometric losses ---------------------
def _tile_ragged(hook_name, n, extra=()):
    def ragged(shape):
        B, H, W = _bhw(shape)
        g = hook(hook_name, n, B, H, W, *extra)
        out = [("pixels %% %d per tile" % g[0], g[0] > 0 and (H * W) % g[0] != 0)]
        if n > 4:
            out.append(("tiles %d %% 4 per workgroup" % g[1], g[1] % 4 != 0))
        return out
    return ragged


@functools.lru_cache(maxsize=None)
def albedo_inputs(shape, K):
    """tests/test_albedo_lse_gpu.py::_synthetic's recipe at K coefficients, numpy: random winners (a third background)"""
    import ref_albedo_lse as RA
    B, H, W = _bhw(shape)
    rs = np.random.RandomState(100 * K + H)
    ntri, nver = 37, 30
    tind = np.where(rs.rand(B, H, W, 1) < 0.3, -1.0, rs.randint(0, ntri, (B, H, W, 1))).astype(np.float32)
    n = rs.standard_normal((B, H, W, 3))
    n[..., 2] = np.abs(n[..., 2]) + 0.5
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    tri = np.stack([rs.choice(nver, 3, replace=False) for _ in range(ntri)], axis=1).astype(np.float32)
    pc_tex = (0.05 * rs.standard_normal((3 * nver, K))).astype(np.float32)
    return dict(tri=tri, pc_tex=pc_tex, nver=nver, basis=RA.basis_ref(tri, pc_tex), tri_ind=tind, lighting=RA.std_lighting(H, W, K), normal=n,
                abedo=rs.uniform(0.2, 0.8, (B, H, W, 1)).astype(np.float32), im_gray=rs.uniform(0.0, 1.0, (B, H, W, 1)).astype(np.float32))


def _albedo_dev(shape, K):
    a = albedo_inputs(shape, K)
    return dict(basis=_t(a["basis"], np.float64), tri_ind=_t(a["tri_ind"]), lighting=_t(a["lighting"], np.float64), normal=_t(a["normal"]),
                abedo=_t(a["abedo"]), im_gray=_t(a["im_gray"]))


def _fit_outs(x, stats, M, what="alpha"):
    return {what: x, "stats": stats, "moments": M, "ok": stats[..., 3].copy()}


def _albedo_lse_case(K):
    @case("albedo_lse_forward[K=%d]" % K, "fr_albedo_lse_workspace_bytes", lambda s: _bhw(s) + (K,), 16,
          _tile_ragged("fr_debug_albedo_lse_geom", 5, (K,)), cover=lambda s: float((albedo_inputs(s, K)["tri_ind"] >= 0).mean()), ok=("ok",))
    def _(shape, buf):
        from raw_calls import raw_fit
        return _fit_outs(*raw_fit(_albedo_dev(shape, K), 1e-6, ws=buf))


for _K in (1, 9, 15):
    _albedo_lse_case(_K)


def _albedo_basis_anchor(shape, outs):
    from raw_calls import assert_f64_bits_equal
    assert_f64_bits_equal(outs["basis"].cpu().numpy(), albedo_inputs(shape, DIM[shape]["K"])["basis"], "albedo basis")


@case("albedo_basis_build -> albedo_lse_forward", "fr_albedo_basis_bytes", lambda s: (37, DIM[s]["K"]), 16,
      lambda s: [("elements % 256 threads of the builder", (37 * DIM[s]["K"]) % 256 != 0)],
      cover=lambda s: float((albedo_inputs(s, DIM[s]["K"])["tri_ind"] >= 0).mean()), ok=("ok",), anchor=_albedo_basis_anchor)
def _(shape, buf):
    from raw_calls import raw_basis, raw_fit
    K = DIM[shape]["K"]
    a = albedo_inputs(shape, K)
    basis = raw_basis(_t(a["tri"]), _t(a["pc_tex"]), a["nver"], ws=buf)
    return dict(_fit_outs(*raw_fit(dict(_albedo_dev(shape, K), basis=basis), 1e-6)), basis=basis.clone())


@functools.lru_cache(maxsize=None)
def solve_inputs(shape, K):
    """tests/test_photo_solve_rgb_gpu.py::_synthetic's recipe at K coefficients"""
    import ref_photo_solve_rgb as RS
    B, H, W = _bhw(shape)
    rs = np.random.RandomState(200 * K + H)
    ntri, nver = 37, 30
    tind = np.where(rs.rand(B, H, W, 1) < 0.3, -1.0, rs.randint(0, ntri, (B, H, W, 1))).astype(np.float32)
    n = rs.standard_normal((B, H, W, 3))
    n[..., 2] = np.abs(n[..., 2]) + 0.7
    n = (n * rs.uniform(0.5, 2.0, (B, H, W, 1))).astype(np.float32)
    tri = np.stack([rs.choice(nver, 3, replace=False) for _ in range(ntri)], axis=1).astype(np.float32)
    pc_tex = (0.05 * rs.standard_normal((3 * nver, K))).astype(np.float32)
    mu_tex = rs.uniform(0.3, 0.8, (3, nver)).astype(np.float32)
    basis = RS.basis_ref(tri, mu_tex, pc_tex)
    star, light = (0.5 * rs.standard_normal((B, K))).astype(np.float32), RS.std_light(B, K)
    target, tex, _ = RS.std_target(basis, tind, n, light, star)
    target = (target + 0.05 * rs.standard_normal(target.shape) * (tind >= 0)).astype(np.float32)
    return dict(tri=tri, mu_tex=mu_tex, pc_tex=pc_tex, nver=nver, basis=basis, tri_ind=tind, normal=n, target=target, tex=tex, light=light)


def _solve_cover(K):
    return lambda s: float((solve_inputs(s, K)["tri_ind"] >= 0).mean())


def _solve_ragged():
    return _tile_ragged("fr_debug_photo_solve_rgb_geom", 6)


def _solve_anchor(units, Kfit, ridge):
    """tests/test_photo_solve_rgb_gpu.py::_check_solve on every fitted unit: the backward error on the kernel's own moments"""
    def anchor(shape, outs):
        from test_photo_solve_rgb_gpu import _check_solve
        x, st, M = (np.asarray(outs[k]) for k in (units, "stats", "moments"))
        x, st, M = x.reshape((-1,) + x.shape[-1:]), st.reshape(-1, 4), M.reshape(-1, 16, 16)
        for u in range(x.shape[0]):
            _check_solve(M[u], Kfit, ridge, x[u], st[u], "%s unit %d" % (shape, u))
    return anchor


def _solve_cases(K):
    @case("photo_light_lse_rgb_forward[K=%d]" % K, "fr_photo_solve_rgb_workspace_bytes", _bhw, 16, _solve_ragged(), cover=_solve_cover(K),
          other=("albedo_lse_rgb_forward[K=%d]" % K, "large"), ok=("ok",), anchor=_solve_anchor("light", 9, 0.0))   # (kind "photo_solve_rgb")
    def _(shape, buf):
        from test_photo_solve_rgb_gpu import raw_light
        inp = solve_inputs(shape, K)
        return _fit_outs(*raw_light(inp, inp["tex"], ws=buf), what="light")

    @case("albedo_lse_rgb_forward[K=%d]" % K, "fr_photo_solve_rgb_workspace_bytes", _bhw, 16, _solve_ragged(), cover=_solve_cover(K),
          other=("photo_light_lse_rgb_forward[K=%d]" % K, "large"), ok=("ok",), anchor=_solve_anchor("alpha", K, 1e-6))
    def _(shape, buf):
        from test_photo_solve_rgb_gpu import raw_albedo
        inp = solve_inputs(shape, K)
        return _fit_outs(*raw_albedo(inp, inp["light"], ridge=1e-6, ws=buf))


for _K in (1, 9, 15):
    _solve_cases(_K)


def _basis_rgb_anchor(shape, outs):
    from raw_calls import assert_f64_bits_equal
    assert_f64_bits_equal(outs["basis"].cpu().numpy(), solve_inputs(shape, DIM[shape]["K"])["basis"], "colour albedo basis")
    _solve_anchor("alpha", DIM[shape]["K"], 1e-6)(shape, outs)


@case("albedo_basis_rgb_build -> albedo_lse_rgb_forward, albedo_image_rgb", "fr_albedo_basis_rgb_bytes", lambda s: (37, DIM[s]["K"]), 16,
      lambda s: [("elements % 256 threads of the builder", (37 * 3 * (DIM[s]["K"] + 1)) % 256 != 0)],
      cover=lambda s: _solve_cover(DIM[s]["K"])(s), ok=("ok",), anchor=_basis_rgb_anchor)
def _(shape, buf):
    from test_photo_solve_rgb_gpu import raw_albedo
    K = DIM[shape]["K"]
    inp = solve_inputs(shape, K)
    B, H, W = _bhw(shape)
    tri, mu, pc = _t(inp["tri"]), _t(inp["mu_tex"]), _t(inp["pc_tex"])
    assert lib().fr_albedo_basis_rgb_build(_p(tri), _p(mu), _p(pc), inp["nver"], 37, K, _p(buf), buf.numel(), _st()) == 0
    basis = buf.view(torch.float64).view(37, 3, K + 1)
    alpha, stats, M = raw_albedo(inp, inp["light"], ridge=1e-6, basis=basis)
    img, ti, al = _full((B, H, W, 3)), _t(inp["tri_ind"]), _t(alpha)
    assert lib().fr_albedo_image_rgb(_p(basis), _p(ti), _p(al), B, 37, H, W, K, _p(img), _st()) == 0
    return dict(_fit_outs(alpha, stats, M), basis=basis.clone(), image=img)


def _photo_case(name, size_fn, hook_name, call_name, planes_of, other):
    @functools.lru_cache(maxsize=None)
    def planes(shape):
        B, H, W = _bhw(shape)
        return planes_of(B, H, W, seed=5 + H)

    def anchor(shape, outs):
        import ref_photo_loss as RP
        import ref_photo_rgb as RC
        from raw_calls import GAIN, OFFSET, assert_f64_bits_equal
        p = planes(shape)
        want = (RP if call_name == "PhotoCall" else RC).forward(*p[:5], p[5], GAIN, OFFSET)
        assert_f64_bits_equal(outs["sums"].cpu().numpy(), want, name)

    @case(name, size_fn, _bhw, 16, _tile_ragged(hook_name, 4), other=(other, "large"), cover=lambda s: float((planes(s)[2] >= 0).mean()),
          anchor=anchor)
    def _(shape, buf):
        import raw_calls
        return {"sums": getattr(raw_calls, call_name)(planes(shape), True).forward(state=buf)}


def _hand_planes(*a, **k):
    import ref_photo_loss as RP
    return RP.hand_planes(*a, **k)


def _hand_planes_rgb(*a, **k):
    import ref_photo_rgb as RC
    return RC.hand_planes_rgb(*a, **k)


# (the two losses keep their states under two pool kinds, "photo_loss" and "photo_loss_rgb": neither ever finds the other's leftovers in
# the pool.  Each is still given the other's -- another layout at the same base, a stricter leftover than its own at a larger shape.)
_photo_case("photo_loss_forward", "fr_photo_loss_state_bytes", "fr_debug_photo_loss_geom", "PhotoCall", _hand_planes, "photo_loss_rgb_forward")
_photo_case("photo_loss_rgb_forward", "fr_photo_loss_rgb_state_bytes", "fr_debug_photo_loss_rgb_geom", "PhotoRgbCall", _hand_planes_rgb,
            "photo_loss_forward")


# ---- the albedo blend's adjoint -----------------------------------------------------------------------------------------------------------
def _synth_args(shape):
    return DIM[shape]["B"], asset_dims(shape)[0], DIM[shape]["K"]


def _synth_ragged(shape):
    import ref_photo_loss as RP
    B, N, K = _synth_args(shape)
    return [("3 N %% %d rows per tile" % RP.TX_ROWS, (3 * N) % RP.TX_ROWS != 0), ("K % 16", K % 16 != 0)]


@functools.lru_cache(maxsize=None)
def _synth_in(shape):
    B, N, K = _synth_args(shape)
    rs = np.random.RandomState(N + K)
    return (0.05 * rs.standard_normal((3 * N, K))).astype(np.float32), rs.standard_normal((B, 3, N)).astype(np.float32)


def _synth_anchor(shape, outs):
    import ref_photo_loss as RP
    from gpu_util import assert_bits_equal
    assert_bits_equal(outs["grad_alpha"].cpu().numpy(), RP.texture_backward(*_synth_in(shape)), "synth_texture_backward " + shape)


@case("synth_texture_backward", "fr_synth_texture_backward_workspace_bytes", _synth_args, 16, _synth_ragged, anchor=_synth_anchor)
def _(shape, buf):
    B, N, K = _synth_args(shape)
    pc, g = (_t(a) for a in _synth_in(shape))
    out = _full((B, K))
    assert lib().fr_synth_texture_backward(_p(pc), _p(g), B, N, K, _p(out), _p(buf), buf.numel(), _st()) == 0
    return {"grad_alpha": out}


# ---- landmarks ------------------------------------------------------------------------------------------------------------------------------
_LM = {"even": ("small", 1, 1), "ragged": ("small", 3, 3), "large": ("small", 65, 68)}       # tests/test_landmark_solve_gpu.py's cases


@functools.lru_cache(maxsize=None)
def _lm_case(shape):
    from test_landmark_solve_gpu import _case
    c = dict(_case(*_LM[shape]))
    P = c["P"].copy()
    P[:, 6] = np.where(P[:, 6] == 0, np.float32(5e-4), P[:, 6])                                  # (every face is to solve: no f = 0 face)
    c["P"] = P
    return c


def _lm_dims(shape):
    """(B, K, n_shape, n_exp) of the case: the model is tests/test_landmark_gpu.py's asset kind"""
    from test_landmark_gpu import _assets
    kind, B, K = _LM[shape]
    A = _assets(kind)
    return B, K, int(A["ndim_shape"]), int(A["ndim_exp"])


def _lm_ragged(shape):
    """(the landmark kernels have no geometry hook: one workgroup per face; the solver's matrix-core tiles are 16 coefficients and 4
    rows, the header's "landmark solver")"""
    B, K, ns, ne = _lm_dims(shape)
    return [("B > 1", B > 1), ("(ns + ne) % 16", (ns + ne) % 16 != 0), ("3 K rows % 4", (3 * K) % 4 != 0)]


def _lm_solve_anchor(shape, outs):
    import ref_landmark_solve as RS
    from test_landmark_solve_gpu import _check
    c = _lm_case(shape)
    st = RS.Step(c["P"], c["mean"], c["Um"], c["target"], weight=None, damp=c["damp"], pose_mask=0, fit_coef=1, ridge=c["ridge"],
                 center=c["center"])
    worst, same, n = _check(c, "coefficients " + shape, st, *(outs[k].cpu().numpy() for k in ("delta", "cost", "ok")), False)
    print("%s: bit for bit %d of %d faces, worst error / bound %.3g" % (shape, same, n, worst))


def _lm_basis_anchor(shape, outs):
    import ref_landmark as RL
    from gpu_util import assert_bits_equal
    c = _lm_case(shape)
    assert_bits_equal(outs["image"].cpu().numpy(), RL.basis_image(c["A"]["mu"], c["A"]["pc_shape"], c["A"]["pc_exp"], c["idx"]).reshape(-1),
                      "landmark basis image")


@case("landmark_basis_build -> landmark_forward, landmark_backward", "fr_landmark_basis_bytes", lambda s: _lm_dims(s)[1:], 16, _lm_ragged,
      anchor=_lm_basis_anchor)
def _(shape, buf):
    from test_landmark_gpu import c_backward, c_build, c_forward
    c = _lm_case(shape)
    A = c["A"]
    img = c_build(_t(np.asarray(A["mu"]).reshape(-1)), _t(A["pc_shape"]), _t(A["pc_exp"]), c["idx"], c["N"], c["ns"], c["ne"],
                  img=buf.view(torch.float32))
    points, sse = c_forward(dict(c, img=img), _t(c["P"]), target=_t(c["target"]))
    gs = _t(np.linspace(0.5, 1.5, c["P"].shape[0]), np.float64)
    gp, _ = c_backward(dict(c, img=img), _t(c["P"]), None, gs, None, _t(c["target"]), None, 1)
    return {"image": img.clone(), "points": points, "sse": sse, "grad_params": gp}


@case("landmark_solve_step", "fr_landmark_solve_workspace_bytes", lambda s: _lm_dims(s)[:1] + _lm_dims(s)[2:], 16, _lm_ragged, ok=("ok",),
      anchor=_lm_solve_anchor)
def _(shape, buf):
    from test_landmark_solve_gpu import c_step
    c = _lm_case(shape)
    delta, cost, ok = c_step(c, _t(c["P"]), _t(c["target"]), ridge=_t(c["ridge"]), center=_t(c["center"]), damp=_t(c["damp"], np.float64),
                             mask=0, coef=1, ws=buf)
    return {"delta": delta, "cost": cost, "ok": ok}
