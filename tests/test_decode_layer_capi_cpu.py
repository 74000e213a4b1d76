"""The differentiable decode -> rendering-layer step at the C ABI, without a GPU: the three entry points exist, refuse bad
arguments with the documented codes before any HIP call, size their workspace as the header says, and the z-only fused
decode backward keeps its hand-counted load stream in registers."""
import ctypes
import os
import re

from conftest import pkg

N_FULL, NS, NE = 53215, 199, 29


def _L():
    return pkg("_lib").lib()


def test_symbols_load_and_version():
    L = _L()
    for name in ("fr_decode_rendering_layer_forward", "fr_decode_render_backward_workspace_bytes", "fr_decode_render_backward"):
        assert hasattr(L, name), name
        assert name in pkg("_lib").EXPORTS
    assert b"fr_hotpath 0.4 " in L.fr_version()


def test_forward_validates_before_any_hip_call():
    L = _L()
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(128)
    f = ctypes.c_float(200.0)

    def args(phases, hand=one, hbytes=3 * 32 * 4, B=1, img=one, net=one, ntri=5, N=20, tb=1, ws=nul, wsb=0):
        return (one, one, nul, one, one, img, B, N, 2, 2, ntri, 8, 8, tb, f, hand, hbytes, net, one, one, one, ws, wsb, nul,
                phases)
    fwd = L.fr_decode_rendering_layer_forward
    assert fwd(*args(0)) == -1 and fwd(*args(16)) == -1                       # phase bits
    assert fwd(*args(8 << 8)) == -1 and fwd(*args(11 | 0x10000)) == -1        # a hint without a phase; a bit beyond
    assert fwd(*args(11, B=0)) == 0 and fwd(*args(11 | (8 << 8), B=0)) == 0   # empty batch
    assert fwd(*args(11, tb=3)) == -1                                         # tex_batch neither 1 nor B
    assert fwd(*args(11, hand=nul)) == -2                                     # no hand-off buffer
    assert fwd(*args(11, hbytes=16)) == -2                                    # too small
    assert fwd(*args(11, hand=ctypes.c_void_p(16))) == -2                     # not 128-byte aligned
    assert fwd(*args(11, img=nul)) == -1                                      # im_gray is required by the fused resolve
    assert fwd(*args(11, net=nul)) == -1
    assert fwd(*args(15, ntri=0)) == -4                                       # nothing to fuse: as fr_rendering_layer_forward
    assert fwd(*args(15, ntri=1 << 24)) == -4
    assert fwd(*args(15)) == -2                                               # render workspace missing
    # what only the fallback rasteriser covers: FR_ERR_UNSUPPORTED, like fr_rendering_layer_forward
    assert L.fr_rendering_layer_forward(one, one, one, one, 1, 20, 5, 2, 70000, 1, one, one, one, one, one, 1 << 30, nul) == -4
    wide = list(args(15, ws=one, wsb=1 << 30))
    wide[11], wide[12] = 2, 70000
    assert fwd(*wide) == -4


def test_backward_validates_before_any_hip_call():
    L = _L()
    nul, one, al = ctypes.c_void_p(0), ctypes.c_void_p(128), ctypes.c_void_p(4096)
    f = ctypes.c_float(200.0)
    wsb = L.fr_decode_render_backward_workspace_bytes
    bwd = L.fr_decode_render_backward
    B, N, ns, ne, ntri, H, W = 2, 64, 5, 3, 7, 8, 8
    need = wsb(B, N, ns, ne, H, W)
    assert need > 0 and need % 256 == 0

    def args(gd=one, gi=one, gn=one, img=one, dep=one, tri=one, ti=one, par=one, mu=one, pt=one, B=B, N=N, ns=ns, ne=ne,
             gp=one, ws=al, nb=need):
        return (gd, gi, gn, img, dep, tri, ti, par, mu, pt, nul, B, N, ns, ne, ntri, H, W, f, gp, ws, nb, nul)
    assert bwd(*args(B=0)) == 0
    assert bwd(*args(B=-1)) == -1
    for k in ("tri", "ti", "par", "mu", "pt", "gp"):                           # NULL required pointers
        assert bwd(*args(**{k: nul})) == -1, k
    assert bwd(*args(gd=nul, gi=nul, gn=nul)) == -1                            # no gradient at all
    assert bwd(*args(img=nul)) == -1 and bwd(*args(dep=nul)) == -1             # needed by the masked planes ...
    assert bwd(*args(gi=nul, gn=nul, img=nul, dep=nul, nb=need - 1)) == -2     # ... not by g_depth alone (fails later, on the size)
    assert bwd(*args(mu=ctypes.c_void_p(132))) == -1                           # mu / image alignment, as the packed backward
    assert bwd(*args(nb=need - 1)) == -2                                       # one byte short
    assert bwd(*args(ws=nul)) == -2
    assert bwd(*args(ws=ctypes.c_void_p(4096 + 128))) == -2                    # 256-byte alignment
    assert bwd(*args(ws=ctypes.c_void_p(4096 + 16))) == -2
    # what the fused decode backward does not serve: more than 256 coefficients, fewer than 16 vertices
    assert wsb(B, N, 250, 29, H, W) == 0 and bwd(*args(ns=250, ne=29, nb=1 << 30)) == -4
    assert wsb(B, 15, ns, ne, H, W) == 0 and bwd(*args(N=15, nb=1 << 30)) == -4
    assert wsb(0, N, ns, ne, H, W) == 0


def test_backward_workspace_size():
    L = _L()
    wsb = L.fr_decode_render_backward_workspace_bytes
    prev = 0
    for B in (1, 2, 16, 63, 64, 65, 70, 128):
        for (N, ns, ne, H, W) in ((N_FULL, NS, NE, 200, 200), (1000 + 7, 9, 5, 37, 53)):
            pitch = L.fr_decode_render_vertex_pitch(N)
            parts = (L.fr_render_depth_backward_workspace_bytes(B, H, W) + B * pitch * 4 +
                     L.fr_decode_backward_workspace_bytes(B, N, ns, ne))
            got = wsb(B, N, ns, ne, H, W)
            assert got >= parts and got % 256 == 0
            assert got <= parts + 3 * 256                                       # nothing but the alignment on top
        full = wsb(B, N_FULL, NS, NE, 200, 200)
        assert full > prev                                                      # monotone in B
        prev = full


def test_z_only_fused_backward_keeps_its_streams_in_registers():
    """bwd_fused_z_kernel counts its inline-asm loads by hand (tile: vmcnt(3 CB); a coordinate's fragments: vmcnt(5 CB + 8) in a
    staging wave -- two four-load tiles -- and vmcnt(5 CB) elsewhere): no instantiation may spill or touch scratch, which shares
    the counter.  It is a kernel of its own: bwd_fused_kernel keeps its eight instantiations."""
    import subprocess
    h = pkg("_lib")
    src = os.path.join(h._CSRC, "fr_decode_bwd.hip")
    cmd = [h._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src]
    out = subprocess.run(cmd, cwd=h._CSRC, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    z = [b for b in blocks if b.startswith("_ZN2fr18bwd_fused_z_kernel")]
    assert len(z) == 8                 # NB = 1..4 live column blocks x CB = 2 / 4 coefficient blocks per wave
    for b in z:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b[:400]
        assert re.search(r"VGPRs Spill: 0\b", b), b[:400]
    assert len([b for b in blocks if b.startswith("_ZN2fr16bwd_fused_kernel")]) == 8
    # the counted waits in the generated code: a staging wave's fragment wait is 5 CB + 8 (28 / 18), never the dense tile's 32 / 22
    asm_out = subprocess.run(cmd[:-4] + ["-S", "-o", "-", src], cwd=h._CSRC, capture_output=True, text=True)
    assert asm_out.returncode == 0, asm_out.stderr[-2000:]
    lines = asm_out.stdout.split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"_ZN2fr18bwd_fused_z_kernel\w+:", l)]
    ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
    assert len(starts) == 8
    for si in starts:
        body = "\n".join(lines[si:min(e for e in ends if e > si)])
        cb4 = re.match(r"_ZN2fr18bwd_fused_z_kernelILi\dELi(\d)E", lines[si]).group(1) == "4"
        waits = set(re.findall(r"s_waitcnt vmcnt\((\d+)\)", body))
        assert ({"28", "20", "12"} if cb4 else {"18", "10", "6"}) <= waits, (lines[si][:60], sorted(waits))
        assert not ({"32", "22"} & waits), (lines[si][:60], sorted(waits))
