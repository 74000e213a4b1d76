"""CPU: the C-ABI library loads and exports every symbol include/fr_hotpath.h declares; argument validation
returns the documented codes before any HIP call; host-side logic (sharding, sampler, synthetic assets)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "fr_hotpath.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fr_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported():
    host = pkg("_lib")
    L = host.lib()
    syms = _declared_symbols()
    assert len(syms) >= 8
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(host.EXPORTS) == syms
    assert b"gfx950" in L.fr_version()
    assert L.fr_strerror(0) == b"ok" and L.fr_strerror(-1) == b"invalid argument"


def test_validation_codes_without_gpu():
    L = pkg("_lib").lib()
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    # C != 3  (render_depth_op.cc:418)
    assert L.fr_render_depth_forward(one, one, one, 1, 3, 1, 4, 4, 4, 1, one, one, one, one, nul, 0, nul) == -1
    # tex_batch neither 1 nor B
    assert L.fr_render_depth_forward(one, one, one, 4, 3, 1, 4, 4, 3, 2, one, one, one, one, nul, 0, nul) == -1
    # negative sizes
    assert L.fr_render_depth_forward(one, one, one, -1, 3, 1, 4, 4, 3, 1, one, one, one, one, nul, 0, nul) == -1
    # null outputs
    assert L.fr_render_depth_forward(one, one, one, 1, 3, 1, 4, 4, 3, 1, nul, one, one, one, nul, 0, nul) == -1
    # empty batch / empty image: ok, nothing launched
    assert L.fr_render_depth_forward(nul, nul, nul, 0, 3, 1, 4, 4, 3, 0, nul, nul, nul, nul, nul, 0, nul) == 0
    assert L.fr_render_depth_forward(one, one, one, 2, 3, 1, 0, 4, 3, 2, nul, nul, nul, nul, nul, 0, nul) == 0
    # too many triangles for float-stored ids
    assert L.fr_render_depth_forward(one, one, one, 1, 3, 1 << 24, 4, 4, 3, 1, one, one, one, one, nul, 0, nul) == -4
    assert L.fr_render_depth_backward(one, one, one, nul, 1, 3, 1, 4, 4, nul) == -1
    assert L.fr_render_depth_backward(nul, nul, nul, nul, 0, 3, 1, 4, 4, nul) == 0
    assert L.fr_decode_pack_basis(one, one, one, 10, 2, 2, one, 8, nul) == -2          # packed buffer too small
    assert L.fr_decode_pack_basis(one, one, one, -1, 2, 2, one, 1 << 20, nul) == -1
    assert L.fr_decode_3dmm(nul, one, nul, 2, 10, 2, 2, 200.0, one, nul) == -1
    assert L.fr_decode_3dmm(nul, nul, nul, 0, 10, 2, 2, 200.0, nul, nul) == 0
    # binned rasteriser workspace: 16-byte hit records (one slot per triangle) + 64 u16 bucket offsets per segment
    # + per-record normals (float4, same slots) + texture-mean table (float4 per triangle, same bound)
    seg = 504  # triangles (= record slots) per segment
    nseg = (105840 + seg - 1) // seg
    assert L.fr_render_depth_workspace_bytes(64, 53215, 105840, 200, 200) == \
        64 * nseg * (seg * 16 + 64 * 2) + 2 * 64 * nseg * seg * 16 + (2 * nseg * seg + 1) * 16  # + triangle table by id + its header + the table in lane order
    assert L.fr_render_depth_workspace_bytes(0, 5, 5, 8, 8) == 0
    # workspace too small
    assert L.fr_render_depth_forward(one, one, one, 1, 3, 1, 4, 4, 3, 1, one, one, one, one, nul, 0, nul) == -2


def test_round3_entry_points_validate_before_any_hip_call():
    """fr_decode_render_forward, the Q30 entry points and the packed decode backward return the documented codes for bad
    arguments without touching the GPU (no device in this container)."""
    L = pkg("_lib").lib()
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(128)
    f = ctypes.c_float(200.0)
    # sizes
    assert L.fr_decode_render_vertex_pitch(53215) == 53216 and L.fr_decode_render_vertex_pitch(64) == 64
    assert L.fr_decode_render_vertex_pitch(0) == 0 and L.fr_decode_render_vertex_bytes(64, 53215) == 64 * 3 * 53216 * 4
    args = lambda phases, hand=one, hbytes=3 * 32 * 4, B=1: (one, one, nul, one, one, B, 20, 2, 2, 5, 8, 8, 1, f, hand, hbytes,  # noqa: E731
                                                             one, one, one, one, nul, 0, nul, phases)
    assert L.fr_decode_render_forward(*args(0)) == -1 and L.fr_decode_render_forward(*args(16)) == -1      # phase bits
    assert L.fr_render_depth_strip_rows(64, 105840, 200, 200) == 10 and L.fr_render_depth_strip_rows(0, 5, 8, 8) == 0
    assert L.fr_render_depth_strip_rows(32, 105840, 200, 200) == 7 and L.fr_render_depth_strip_rows(16, 105840, 448, 448) == 14
    # round 6: bits 8-15 carry the strip-height hint (FR_PHASES_STRIP_ROWS); a hint without a phase, or any bit beyond, is refused
    assert L.fr_decode_render_forward(*args(8 << 8)) == -1 and L.fr_decode_render_forward(*args(11 | 0x10000)) == -1
    assert L.fr_decode_render_forward(*args(11 | (8 << 8), B=0)) == 0 and L.fr_decode_render_forward(*args(11 | (8 << 8), hand=nul)) == -2
    assert L.fr_decode_render_forward(*args(11, B=0)) == 0                                                  # empty batch
    assert L.fr_decode_render_forward(*args(11, hand=nul)) == -2                                            # no hand-off buffer
    assert L.fr_decode_render_forward(*args(11, hbytes=16)) == -2                                           # too small
    assert L.fr_decode_render_forward(*args(11, hand=ctypes.c_void_p(16))) == -2                            # not 128-byte aligned
    a = list(args(11)); a[12] = 3                                                                           # tex_batch neither 1 nor B
    assert L.fr_decode_render_forward(*a) == -1
    # Q30: unsupported shape, missing workspace
    assert L.fr_decode_q30_pack(one, one, one, 10, 600, 10, ctypes.c_void_p(256), 1 << 20, nul) == -4
    assert L.fr_decode_3dmm_q30(one, ctypes.c_void_p(256), nul, 1, 10, 5, 3, f, one, nul, 0, nul) == -2
    assert L.fr_decode_3dmm_q30(one, ctypes.c_void_p(256), nul, 1, 10, 600, 3, f, one, one, 1 << 20, nul) == -4
    assert L.fr_decode_3dmm_q30(one, ctypes.c_void_p(256), nul, 0, 10, 5, 3, f, one, nul, 0, nul) == 0
    # round 5: the level count is an argument (7 / 5 / 4), validated before anything else
    q = ctypes.c_void_p(256)
    assert L.fr_decode_3dmm_q30_lv(one, q, nul, 1, 10, 5, 3, f, 6, one, one, 1 << 20, nul) == -1
    assert L.fr_decode_3dmm_q30_lv(one, q, nul, 1, 10, 5, 3, f, 4, one, nul, 0, nul) == -2
    assert L.fr_decode_3dmm_q30_lv(one, q, nul, 0, 10, 5, 3, f, 5, one, nul, 0, nul) == 0
    qargs = lambda phases, lv=4, hand=one, qws=one, qb=1 << 20, B=1: (one, q, nul, one, one, B, 20, 2, 2, 5, 8, 8, 1, f, lv, hand,  # noqa: E731
                                                                       3 * 32 * 4, one, one, one, one, nul, 0, qws, qb, nul, phases)
    assert L.fr_decode_render_forward_q30(*qargs(0)) == -1 and L.fr_decode_render_forward_q30(*qargs(11, lv=3)) == -1
    assert L.fr_decode_render_forward_q30(*qargs(8 << 8)) == -1 and L.fr_decode_render_forward_q30(*qargs(11 | (8 << 8), B=0)) == 0
    assert L.fr_decode_render_forward_q30(*qargs(11, B=0)) == 0
    assert L.fr_decode_render_forward_q30(*qargs(11, hand=nul)) == -2
    assert L.fr_decode_render_forward_q30(*qargs(11, qws=nul, qb=0)) == -2        # no staging workspace
    # packed backward: image size = row blocks x coefficient blocks x 1 KiB; too small a buffer; null image
    rb, sb = (3 * 53215 + 15) // 16, 13 + 2
    assert L.fr_decode_backward_basis_bytes(53215, 199, 29) == rb * sb * 1024
    assert L.fr_decode_backward_basis_bytes(15, 9, 5) == 0 and L.fr_decode_backward_basis_bytes(16, 9, 5) > 0   # whole tiles only
    assert L.fr_decode_backward_pack_basis(one, one, 53215, 199, 29, one, 1024, nul) == -2
    assert L.fr_decode_3dmm_backward_packed(one, one, one, nul, nul, 2, 10, 5, 3, f, one, one, 1 << 30, nul) == -1
    assert L.fr_decode_3dmm_backward_packed(one, one, one, one, nul, 2, 10, 5, 3, f, one, one, 16, nul) == -2
    # ... and its mu form: unsupported where the fused kernel is (N < 16 here), null mu, small workspace
    assert L.fr_decode_3dmm_backward_packed_mu(one, one, one, one, nul, 2, 10, 5, 3, f, one, one, 1 << 30, nul) == -4
    assert L.fr_decode_3dmm_backward_packed_mu(one, one, nul, one, nul, 2, 64, 5, 3, f, one, one, 1 << 30, nul) == -1
    assert L.fr_decode_3dmm_backward_packed_mu(one, one, one, one, nul, 2, 64, 5, 3, f, one, one, 16, nul) == -2
    assert L.fr_decode_3dmm_backward_packed_mu(one, one, one, one, nul, 0, 64, 5, 3, f, one, one, 16, nul) == 0


def test_options_read_the_environment_once_and_never_on_the_launch_path(monkeypatch):
    """The launcher knobs take their initial value from the environment ONCE per process; afterwards only fr_set_option
    changes them -- a later change of os.environ (putenv) must not change behaviour, and no kernel source calls getenv
    outside that one-time initialisation."""
    host = pkg("_lib")
    L = host.lib()
    before = {k: host.get_option(k) for k in ("FR_EMIT_FILTER", "FR_RENDER_ROWS", "FR_DECODE_NT", "FR_RENDER_IMPL")}
    monkeypatch.setenv("FR_EMIT_FILTER", "0")
    monkeypatch.setenv("FR_RENDER_ROWS", "7")
    monkeypatch.setenv("FR_DECODE_NT", "0")
    monkeypatch.setenv("FR_RENDER_IMPL", "scan")
    assert {k: host.get_option(k) for k in before} == before
    out = (ctypes.c_int * 4)()
    L.fr_debug_render_geom(64, 105840, 200, 200, 0, out)     # the geometry the launcher would pick: FR_RENDER_ROWS unchanged
    assert out[0] == 10 or before["FR_RENDER_ROWS"] != 0
    with host.options(FR_RENDER_ROWS=7):
        assert host.get_option("FR_RENDER_ROWS") == 7
    assert host.get_option("FR_RENDER_ROWS") == before["FR_RENDER_ROWS"]
    assert L.fr_set_option(b"FR_NO_SUCH_KNOB", 1) == -1
    v = ctypes.c_int(0)
    assert L.fr_get_option(b"FR_NO_SUCH_KNOB", ctypes.byref(v)) == -1 and L.fr_get_option(b"FR_EMIT_FILTER", None) == -1
    # getenv appears in exactly one place of the native sources: the one-time option initialisation
    hits = []
    csrc = os.path.join(ROOT, "3dfacerecon_amd", "csrc")
    for fn in sorted(os.listdir(csrc)):
        for i, line in enumerate(open(os.path.join(csrc, fn)), 1):
            if re.search(r"\bgetenv\s*\(", line):
                hits.append((fn, i))
    assert [h[0] for h in hits] == ["fr_capi.hip"], hits


def test_decode_cus_option_round_trips():
    """FR_DECODE_CUS (test knob: the CU count the decode forward launchers plan for) is in the option table, 0 by default"""
    host = pkg("_lib")
    L = host.lib()
    v = ctypes.c_int(-5)
    assert L.fr_get_option(b"FR_DECODE_CUS", ctypes.byref(v)) == 0 and v.value == int(os.environ.get("FR_DECODE_CUS") or 0)
    before = v.value
    for n in (1, 3, 8, 300, 0):
        assert L.fr_set_option(b"FR_DECODE_CUS", n) == 0
        assert L.fr_get_option(b"FR_DECODE_CUS", ctypes.byref(v)) == 0 and v.value == n
    with host.options(FR_DECODE_CUS=2):
        assert host.get_option("FR_DECODE_CUS") == 2
    assert host.get_option("FR_DECODE_CUS") == 0
    assert L.fr_set_option(b"FR_DECODE_CUS", before) == 0


def test_binary_only_deployment_loads_without_sources(tmp_path, monkeypatch):
    """A copied .so without csrc/, include/ or the .srchash sidecar: the identity is read from the hash embedded in the
    binary, nothing tries to open a source file, and with sources present a sidecar-less library is not declared stale."""
    host = pkg("_lib")
    host.lib()
    real = host.LIB_PATH
    assert host._built_hash() == host.src_hash()
    import shutil
    copy = str(tmp_path / "libfr_hotpath.so")
    shutil.copy(real, copy)
    monkeypatch.setattr(host, "LIB_PATH", copy)
    assert host._built_hash() == host.src_hash() and not host.is_stale()      # no sidecar next to the copy
    monkeypatch.setattr(host, "HEADERS", [str(tmp_path / "gone.h")])
    assert host.src_hash() is None and not host.is_stale()
    monkeypatch.setattr(host, "LIB_PATH", str(tmp_path / "absent.so"))
    assert host.is_stale()
    with pytest.raises(RuntimeError):
        host.compile()


def test_render_geometry_window_never_spans_three_strips():
    """An 8x4 hit window is filed under its strip's bucket or the boundary bucket between two strips; strips shorter
    than the window (FR_RENDER_ROWS = 1..3, or a very wide image whose strip must shrink to fit LDS) would let it span
    three: such shapes must leave the binned path."""
    L = pkg("_lib").lib()
    out = (ctypes.c_int * 4)()

    def geom(B, T, H, W, ov=0):
        L.fr_debug_render_geom(B, T, H, W, ov, out)
        return tuple(out)
    rows, strips, nseg, ok = geom(64, 105840, 200, 200)
    assert (rows, strips, nseg, ok) == (10, 20, 210, 1)
    for ov in (1, 2, 3):
        rows, strips, _, ok = geom(64, 105840, 200, 200, ov)
        assert rows == ov and strips > 1 and ok == 0
    assert geom(64, 105840, 200, 200, 7)[3] == 1 and geom(64, 105840, 200, 200, 25)[3] == 1
    assert geom(64, 105840, 200, 200, 4)[3] == 0   # 50 strips: more than the bucket-offset table holds -> scan path
    # a single strip may be shorter than the window (nothing to straddle)
    assert geom(1, 10, 3, 16)[1:] == (1, 1, 1)
    # very wide image: only 3 rows of keys fit LDS -> strips of 3 rows -> not binned
    rows, strips, _, ok = geom(1, 1000, 96, 6000)
    assert rows < 4 and strips > 1 and ok == 0
    # every binned geometry keeps the invariant
    for (B, H, W) in ((1, 200, 200), (64, 200, 200), (16, 448, 448), (7, 33, 1000), (300, 64, 64), (2, 5, 4096)):
        rows, strips, _, ok = geom(B, 5000, H, W)
        assert not ok or rows >= 4 or strips == 1


def test_packed_basis_size():
    L = pkg("_lib").lib()
    # the default image.  f32: tiles of 16 vertices; 16-wide k groups for shape and exp separately; + packed mu.
    n = L.fr_decode_packed_basis_bytes(53215, 199, 29)
    tiles, G = (53215 + 15) // 16, 13 + 2
    assert n == tiles * G * 3 * 64 * 16 + tiles * 3 * 16 * 4
    # the opt-in Q30 image is a buffer of its own: 64 ints of column exponents per k-step of 64, then per tile
    # 3 coordinates x ceil(228 / 16) = 15 live 16-k groups x 4 digits x 256 bytes + a 256-byte payload (mu, row exponents);
    # + 1 KiB slack; its staging workspace is S * 16 KiB of parameter digits + Mt [64][12] floats + be [64] ints
    assert L.fr_decode_q30_image_bytes(53215, 199, 29) == 4 * 64 * 4 + tiles * (3 * 15 * 4 * 256 + 256) + 1024
    assert L.fr_decode_q30_workspace_bytes(199, 29) == 4 * 16384 + 64 * 12 * 4 + 64 * 4
    # more than 512 coefficients: the Q30 kernels do not take the shape
    t2 = (100 + 15) // 16
    assert L.fr_decode_packed_basis_bytes(100, 600, 10) == t2 * (38 + 1) * 3 * 64 * 16 + t2 * 3 * 16 * 4
    assert L.fr_decode_q30_image_bytes(100, 600, 10) == 0 and L.fr_decode_q30_workspace_bytes(600, 10) == 0


def test_ops_module_surface_mirrors_reference():
    ops = pkg("rendering_layer.ops")
    assert ops.OP_NAMES == ['render_depth']
    assert callable(ops.compile) and callable(ops.render_depth) and callable(ops.render_depth_grad)
    with pytest.raises(ValueError):
        ops.compile("no_such_op")


def test_product_fails_loudly_on_cpu_tensors(small_assets):
    import torch
    ops = pkg("rendering_layer.ops")
    ver = torch.zeros((1, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_depth(ver, torch.zeros((3, 2)), torch.zeros((1, 3, 4)), torch.zeros((1, 8, 8, 3)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg("nets.network").FaceRecNet(mesh_data=small_assets, batch_size=1, im_size=40, device="cpu")


def test_product_never_imports_oracle():
    import subprocess
    import sys
    code = ("import sys, importlib; sys.path.insert(0, %r);"
            "importlib.import_module('3dfacerecon_amd.rendering_layer.ops');"
            "importlib.import_module('3dfacerecon_amd.nets.network');"
            "importlib.import_module('3dfacerecon_amd.pipeline');"
            "bad=[m for m in sys.modules if m.split('.')[0]=='oracle']; assert not bad, bad") % ROOT
    subprocess.check_call([sys.executable, "-c", code])
    for dirpath, _, files in os.walk(os.path.join(ROOT, "3dfacerecon_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "fr_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


def test_synthetic_assets_shape(full_assets):
    A = full_assets
    assert A["vertex"].shape == (3, 53215) and A["tri"].shape == (3, 105840)
    assert A["mu"].shape == (159645, 1) and A["pc_shape"].shape == (159645, 199) and A["pc_exp"].shape == (159645, 29)
    tri = A["tri"]
    assert tri.dtype == np.float32 and tri.min() == 0 and tri.max() == 53214 and np.all(tri == np.floor(tri))
    base = set(map(tuple, tri[:, :105408].T.astype(np.int64).tolist()))
    extra = list(map(tuple, tri[:, 105408:].T.astype(np.int64).tolist()))
    assert len(extra) == 432 and all(e in base for e in extra)   # duplicated patch -> exact depth ties
    nrm = np.linalg.norm(A["pc_shape"].astype(np.float64), axis=0)
    np.testing.assert_allclose(nrm, 1.0, rtol=1e-4)


def test_param_layout_and_ranges(synth):
    P = synth.sample_params_batch(8, beta=0.7, seed=3456)
    assert P.shape == (8, 235) and P.dtype == np.float32
    assert np.all(P[:, 5] == 0)                                   # tz
    assert np.all((P[:, 6] >= 0.7e-3 - 1e-9) & (P[:, 6] <= 1e-3))  # f = 0.7*1e-3 + 0.3*U[0,1e-3]
    assert np.all((P[:, 3:5] >= 70) & (P[:, 3:5] <= 88))
    assert np.all((P[:, 7:206] >= 0) & (P[:, 7:206] <= 1e4)) and np.all(np.abs(P[:, 206:]) <= 1.5)
    # config 1: beta = 1.0 gives the fixed pose exactly (sample_test.py:32-33, 93)
    pose, _, _ = synth.get_random_params(200, 199, 29, 1.0, rand=np.random.RandomState(0).rand)
    np.testing.assert_array_equal(pose[:, 0], np.array([0, 0, 0, 100, 100, 0, 0.001], np.float32).astype(np.float64))


def test_shard_range_partitions():
    d = pkg("utils.dist")
    for total in (0, 1, 7, 64, 65, 256):
        for world in (1, 2, 3, 4, 8):
            spans = [d.shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        d.shard_range(4, 2, 2)


@pytest.mark.parametrize("source,prefix,min_kernels", [("fr_decode.hip", "_ZN2fr18decode_ring_kernel", 2),
                                                        ("fr_decode_q.hip", "_ZN2fr20decode_q_ring_kernel", 3)])
def test_ring_decode_kernel_keeps_its_stream_in_registers(source, prefix, min_kernels):
    """The ring kernels (f32 chain and Q30) issue their A-fragment requests through inline asm and count them by hand
    (s_waitcnt vmcnt(R-1) / vmcnt(R-4)): that accounting is only valid if the compiler neither spills an in-flight ring
    slot nor adds scratch traffic, which shares the vmcnt counter.  The compiler's own resource report must show no
    scratch for every instantiation."""
    import subprocess
    h = pkg("_lib")
    src = os.path.join(h._CSRC, source)
    cmd = [h._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src]
    out = subprocess.run(cmd, cwd=h._CSRC, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    ring = [b for b in blocks if b.startswith(prefix)]
    assert len(ring) >= min_kernels
    for b in ring:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b[:400]
        assert re.search(r"VGPRs Spill: 0\b", b), b[:400]
    # the requests take their base address from an SGPR pair handed to inline asm: the compiler's hazard recogniser does
    # not look inside asm, so an SGPR written by a VALU instruction (v_readfirstlane / v_readlane) must not feed a request
    # within the 5 wait states gfx9 demands -- the addresses have to be pure SALU arithmetic
    asm_out = subprocess.run(cmd[:-4] + ["-S", "-o", "-", src], cwd=h._CSRC, capture_output=True, text=True)
    assert asm_out.returncode == 0, asm_out.stderr[-2000:]
    lines = asm_out.stdout.split("\n")
    starts = [i for i, l in enumerate(lines) if l.startswith(prefix)]
    ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
    assert len(starts) >= min_kernels
    for si in starts:
        body = lines[si:min(e for e in ends if e > si)]
        loads = [i for i, l in enumerate(body) if "global_load_dwordx4" in l and ", s[" in l]
        valu_sgpr = [i for i, l in enumerate(body) if "v_readfirstlane" in l or "v_readlane" in l]
        assert len(loads) >= 48
        for li in loads:
            assert all(not (0 < li - r <= 8) for r in valu_sgpr), (lines[si][:80], li)


def test_fused_decode_backward_keeps_its_streams_in_registers():
    """bwd_fused_kernel counts its inline-asm loads by hand too (tile: vmcnt(3 CB); a coordinate's fragments: vmcnt(5 CB + 12) /
    vmcnt(5 CB)): no instantiation may spill or touch scratch (a run-time ring index once put the whole fragment ring there)."""
    import subprocess
    h = pkg("_lib")
    src = os.path.join(h._CSRC, "fr_decode_bwd.hip")
    cmd = [h._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src]
    out = subprocess.run(cmd, cwd=h._CSRC, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: Function Name: ", out.stderr)[1:] if b.startswith("_ZN2fr16bwd_fused_kernel")]
    assert len(blocks) == 8            # NB = 1..4 live column blocks x CB = 2 / 4 coefficient blocks per wave
    for b in blocks:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b[:400]
        assert re.search(r"VGPRs Spill: 0\b", b), b[:400]


def test_decode_backward_geometry_hook():
    """fr_debug_decode_bwd_geom: the launch geometry tests/test_decode_backward_bounds_gpu.py derives its bounds from.
    Full size (N = 53,215, 15 coefficient blocks): 3,326 vertex groups, 13 per fused workgroup (the last one 11) in 256
    workgroups; CB 4 up to 32 faces and 2 beyond (eight waves); the reference layout takes 312 rows per GEMM workgroup in 512
    of them and 832 prepass workgroups.  The 70 x 61 mesh: two groups per workgroup, 134 workgroups.  The knobs move it."""
    host = pkg("_lib")
    L = host.lib()

    def geom(B, N, ns=199, ne=29):
        out = (ctypes.c_int * 7)()
        L.fr_debug_decode_bwd_geom(B, N, ns, ne, out)
        return list(out)

    with host.options(FR_BWD_CHUNKS=256, FR_BWD_CB=0):
        assert geom(64, 53215) == [13, 256, 2, 8, 312, 512, 832]
        assert geom(70, 53215) == geom(64, 53215)
        assert geom(32, 53215) == [13, 256, 4, 4, 312, 512, 832]
        assert geom(33, 53215)[2:4] == [2, 8] and geom(1, 53215)[2:4] == [4, 4]
        assert geom(64, 4270) == [2, 134, 2, 8, 28, 458, 67]
        assert geom(5, 4270, 240, 16)[2:4] == [4, 4] and geom(64, 4270, 240, 16)[2:4] == [2, 8]
        assert geom(64, 0) == [0] * 7
    with host.options(FR_BWD_CHUNKS=512, FR_BWD_CB=4):
        assert geom(64, 53215)[:4] == [7, 476, 4, 4]
    with host.options(FR_BWD_CHUNKS=1, FR_BWD_CB=2):
        assert geom(1, 4270)[:4] == [267, 1, 2, 8]


def test_render_backward_geometry_hook():
    """fr_debug_render_bwd_geom: {owners per face, vertices per owner, shift, record chunks, dynamic LDS bytes, XCD map} from
    the function the launcher itself reads.  The rows are the launch shapes tests/test_render_backward_exact_gpu.py is
    written for: owners clamped to the vertex count; 256 owners of 208 at one face; the XCD block map with several owners at
    a batch of 8; the product batch, whose 106,576 B need the full-LDS opt-in; the other block map at 65 / 70; the largest
    owner range (131,216 B of LDS) and the short second owner one vertex above it; the shift above 2^20 pixels."""
    L = pkg("_lib").lib()

    def geom(B, nver, H=200, W=200):
        out = (ctypes.c_int * 6)()
        L.fr_debug_render_bwd_geom(B, nver, H, W, out)
        return list(out)

    assert geom(1, 3) == [3, 1, 0, 40, 152, 0]
    assert geom(1, 10)[:2] == [10, 1] and geom(1, 1)[:2] == [1, 1]
    assert geom(1, 53215) == [256, 208, 0, 40, 1808, 0]
    assert geom(3, 53215)[:2] == [86, 619] and geom(7, 53215)[:2] == [37, 1439]
    assert geom(8, 53215) == [32, 1663, 0, 40, 13448, 1]
    assert geom(16, 53215)[:2] == [16, 3326] and geom(16, 53215)[5] == 1
    assert geom(64, 53215) == [4, 13304, 0, 40, 106576, 1]
    assert geom(64, 53215)[4] > 64 * 1024                      # above the default dynamic-LDS limit: fr_allow_full_lds
    assert geom(65, 53215) == [4, 13304, 0, 40, 106576, 0] and geom(70, 53215) == geom(65, 53215)
    assert geom(256, 16384, 32, 32) == [1, 16384, 0, 1, 131216, 1]
    assert geom(256, 16385, 32, 32) == [2, 8193, 0, 1, 65688, 1]
    assert geom(16, 70000)[:2] == [16, 4375]
    assert [geom(2, 50, 1, n)[3] for n in (1, 1023, 1024, 1025, 8193)] == [1, 1, 1, 2, 9]
    assert geom(2, 50, 1024, 1024)[2:4] == [0, 1024] and geom(2, 50, 1025, 1024)[2:4] == [1, 1025]
    assert geom(2, 50, 1025, 2048)[2] == 2 and geom(1, 400, 1100, 1000)[2] == 1
    assert geom(0, 5) == [0] * 6 and geom(4, 0) == [0] * 6 and geom(4, 5, 0, 9) == [0] * 6
    assert geom(1, 5, 65536, 65536) == [0] * 6                 # more than 2^31 - 1 pixels: refused by the launcher
