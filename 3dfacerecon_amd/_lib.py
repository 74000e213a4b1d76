"""Loader / builder of the C-ABI shared library (include/fr_hotpath.h) and thin ctypes call helpers.

There is deliberately NO fallback: if libfr_hotpath.so cannot be built or loaded, or a tensor is not on a GPU,
the hot path raises.  PyTorch is used only for device memory and streams.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys
import threading
import types

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG_DIR, "csrc")
LIB_PATH = os.path.join(_PKG_DIR, "libfr_hotpath.so")
SOURCES = ["fr_capi.hip", "fr_render.hip", "fr_decode.hip", "fr_decode_q.hip", "fr_decode_bwd.hip", "fr_render_bwd.hip", "fr_render_nbwd.hip",
           "fr_render_tbwd.hip", "fr_sfs.hip", "fr_depth_normals.hip", "fr_geometry.hip", "fr_fine_losses.hip", "fr_depth_interp.hip",
           "fr_albedo_lse.hip", "fr_synth.hip", "fr_photo.hip", "fr_mesh.hip", "fr_coverage.hip", "fr_landmark.hip",
           "fr_landmark_solve.hip", "fr_landmark_contour.hip", "fr_photo_solve.hip", "fr_attr_interp.hip"]
HEADERS = [os.path.join(_CSRC, "fr_common.h"), os.path.join(_CSRC, "fr_decode_shared.h"), os.path.join(_CSRC, "fr_sfs_pinv.h"),
           os.path.join(_CSRC, "fr_owner_scatter.h"), os.path.join(_CSRC, "fr_shade.h"), os.path.join(_CSRC, "fr_landmark_shared.h"),
           os.path.join(_CSRC, "fr_point_weight.h"),
           os.path.join(_PKG_DIR, "..", "include", "fr_hotpath.h")]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
               "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"]  # single-lane LDS atomics stay single instructions

FR_OK = 0
_ERR_NAMES = {-1: "invalid argument", -2: "workspace / packed buffer too small", -3: "HIP launch or runtime error",
              -4: "size not supported by the gfx950 kernels"}

_lock = threading.Lock()
_lib = None


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def sources_present():
    """False for a binary-only deployment (the .so shipped without csrc/ or include/)."""
    return all(os.path.exists(d) for d in [os.path.join(_CSRC, s) for s in SOURCES] + HEADERS)


def src_hash():
    """sha256 over the kernel sources, the headers and the compile flags (16 hex digits): the identity of a build.
    None when the sources are not in the tree (binary-only deployment: nothing to compare the library with)."""
    if not sources_present():
        return None
    h = hashlib.sha256(" ".join(HIPCC_FLAGS).encode())
    for d in [os.path.join(_CSRC, s) for s in SOURCES] + HEADERS:
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _built_hash():
    """The source hash the existing .so was built from: its sidecar file, or -- when the sidecar did not travel with the
    binary -- the hash embedded in the binary itself (the `src=` field of fr_version(), found by scanning the file: the
    library is not loaded to ask it)."""
    try:
        with open(LIB_PATH + ".srchash") as f:
            return f.read().strip()
    except OSError:
        pass
    try:
        with open(LIB_PATH, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    tag = b"(gfx950) src="
    i = blob.find(tag)
    if i < 0:
        return None
    return blob[i + len(tag):i + len(tag) + 16].decode("ascii", "replace")


def is_stale():
    """True when libfr_hotpath.so is missing or was built from other sources than the ones in the tree (content hash,
    not mtimes: the .so travels to the GPU box in a snapshot whose timestamps mean nothing).  Without sources in the
    tree an existing library is taken as it is."""
    if not os.path.exists(LIB_PATH):
        return True
    want = src_hash()
    return want is not None and _built_hash() != want


def compile(force=False, verbose=False):
    """Cross-compiles the HIP kernels + C ABI for gfx950 with hipcc (works without a GPU)."""
    if not force and not is_stale():
        return LIB_PATH
    hipcc = _hipcc()
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        raise RuntimeError("fr_hotpath: %s is %s and hipcc is not available to rebuild it -- there is no CPU fallback"
                           % (LIB_PATH, "stale" if os.path.exists(LIB_PATH) else "missing"))
    want = src_hash()
    if want is None:
        raise RuntimeError("fr_hotpath: %s is missing and the kernel sources are not in the tree" % LIB_PATH)
    tmp = LIB_PATH + ".tmp%d" % os.getpid()
    cmd = [hipcc] + HIPCC_FLAGS + ['-DFR_SRC_HASH="%s"' % want, "-o", tmp] + [os.path.join(_CSRC, s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=_CSRC)
    with open(LIB_PATH + ".srchash.tmp%d" % os.getpid(), "w") as f:
        f.write(want + "\n")
    os.replace(tmp, LIB_PATH)
    os.replace(LIB_PATH + ".srchash.tmp%d" % os.getpid(), LIB_PATH + ".srchash")
    return LIB_PATH


# The C ABI of include/fr_hotpath.h, one row per entry point: "return:arguments", one letter per type as Python sees it.
# The library is bound from this table alone (a binary-only deployment has no header to read);
# tests/test_capi_signatures_cpu.py holds every row to the header's prototype, position by position.
_CTYPE = {"p": ctypes.c_void_p, "i": ctypes.c_int, "z": ctypes.c_size_t, "u": ctypes.c_ulonglong, "f": ctypes.c_float,
          "d": ctypes.c_double, "s": ctypes.c_char_p, "I": ctypes.POINTER(ctypes.c_int), "D": ctypes.POINTER(ctypes.c_double),
          "v": None}
SIGNATURES = {
    "fr_version":                                     "s:",
    "fr_strerror":                                    "s:i",
    "fr_set_option":                                  "i:si",
    "fr_get_option":                                  "i:sI",
    "fr_render_depth_workspace_bytes":                "z:iiiii",
    "fr_render_depth_forward":                        "i:pppiiiiiiipppppzp",
    "fr_render_depth_forward_phases":                 "i:pppiiiiiiipppppzpi",
    "fr_rendering_layer_forward":                     "i:ppppiiiiiipppppzp",
    "fr_rendering_layer_forward_phases":              "i:ppppiiiiiipppppzpi",
    "fr_render_depth_backward":                       "i:ppppiiiiip",
    "fr_render_depth_backward_workspace_bytes":       "z:iii",
    "fr_render_depth_backward_ws":                    "i:ppppiiiiipzp",
    "fr_decode_packed_basis_bytes":                   "z:iii",
    "fr_decode_pack_basis":                           "i:pppiiipzp",
    "fr_decode_3dmm":                                 "i:pppiiiifpp",
    "fr_render_depth_strip_rows":                     "i:iiii",
    "fr_decode_render_vertex_pitch":                  "i:i",
    "fr_decode_render_vertex_bytes":                  "z:ii",
    "fr_decode_render_forward":                       "i:pppppiiiiiiiifpzpppppzpi",
    "fr_decode_q30_image_bytes":                      "z:iii",
    "fr_decode_q30_pack":                             "i:pppiiipzp",
    "fr_decode_q30_workspace_bytes":                  "z:ii",
    "fr_decode_3dmm_q30":                             "i:pppiiiifppzp",
    "fr_decode_3dmm_q30_lv":                          "i:pppiiiifippzp",
    "fr_decode_render_forward_q30":                   "i:pppppiiiiiiiifipzpppppzpzpi",
    "fr_decode_backward_workspace_bytes":             "z:iiii",
    "fr_decode_3dmm_backward":                        "i:ppppppiiiifppzp",
    "fr_decode_backward_basis_bytes":                 "z:iii",
    "fr_decode_backward_pack_basis":                  "i:ppiiipzp",
    "fr_decode_3dmm_backward_packed":                 "i:pppppiiiifppzp",
    "fr_decode_3dmm_backward_packed_mu":              "i:pppppiiiifppzp",
    "fr_decode_rendering_layer_forward":              "i:ppppppiiiiiiiifpzpppppzpi",
    "fr_decode_render_backward_workspace_bytes":      "z:iiiiii",
    "fr_decode_render_backward":                      "i:pppppppppppiiiiiiifppzp",
    "fr_decode_pose_backward_workspace_bytes":        "z:ii",
    "fr_decode_pose_backward":                        "i:ppppiiiifpppzp",
    "fr_decode_render_backward_pose_workspace_bytes": "z:iiiiii",
    "fr_decode_render_backward_pose":                 "i:pppppppppppiiiiiiifppzppzp",
    "fr_render_normal_backward_workspace_bytes":      "z:iiii",
    "fr_render_normal_backward":                      "i:pipipppiiiiiiipzp",
    "fr_debug_render_normal_bwd_geom":                "v:iiiiI",
    "fr_render_texture_backward_workspace_bytes":     "z:iiiii",
    "fr_render_texture_backward":                     "i:pipppiiiiiiipzp",
    "fr_debug_render_texture_bwd_geom":               "v:iiiiiI",
    "fr_sfs_state_bytes":                             "z:ii",
    "fr_sfs_intensity_forward":                       "i:pppppiiidppzp",
    "fr_sfs_intensity_backward":                      "i:ppppppziiippp",
    "fr_sfs_intensity_backward_tex":                  "i:ppppppziiipppp",
    "fr_debug_sfs_geom":                              "v:iiiI",
    "fr_debug_sfs_pinv":                              "i:DdDI",
    "fr_sfs_moments_bytes":                           "z:ii",
    "fr_sfs_moments":                                 "i:pppiiipzp",
    "fr_sfs_solve_shade":                             "i:pippiiidppzp",
    "fr_sfs_q_bytes":                                 "z:ii",
    "fr_sfs_backward_q":                              "i:pppiiipzp",
    "fr_sfs_backward_apply":                          "i:ppppppzpiiiipppp",
    "fr_debug_sfs_split_geom":                        "v:iiiI",
    "fr_depth_normals_forward":                       "i:ppiiipp",
    "fr_depth_normals_backward":                      "i:pppiiipp",
    "fr_debug_depth_normals_geom":                    "v:iiiI",
    "fr_geometry_gram_bytes":                         "z:ii",
    "fr_geometry_gram_workspace_bytes":               "z:iii",
    "fr_geometry_gram_build":                         "i:ppiiipzpzp",
    "fr_geometry_loss_state_bytes":                   "z:iii",
    "fr_geometry_loss_forward":                       "i:ppiiiippzp",
    "fr_geometry_loss_backward":                      "i:ppziiiipp",
    "fr_debug_geometry_gram_geom":                    "v:iiiI",
    "fr_fine_losses_state_bytes":                     "z:iii",
    "fr_fine_losses_forward":                         "i:ppiiipppzp",
    "fr_fine_losses_backward":                        "i:ppppiiippp",
    "fr_debug_fine_losses_geom":                      "v:iiiI",
    "fr_depth_interp_forward":                        "i:pippiiiiipp",
    "fr_depth_interp_backward_workspace_bytes":       "z:iiii",
    "fr_depth_interp_backward":                       "i:ppipppiiiiiipzp",
    "fr_debug_depth_interp_bwd_geom":                 "v:iiiiI",
    "fr_albedo_basis_bytes":                          "z:ii",
    "fr_albedo_basis_build":                          "i:ppiiipzp",
    "fr_sfs_lighting":                                "i:piiidpzp",
    "fr_albedo_lse_workspace_bytes":                  "z:iiii",
    "fr_albedo_lse_forward":                          "i:ppppppiiiiidppppzp",
    "fr_debug_albedo_lse_geom":                       "v:iiiiI",
    "fr_synth_params":                                "i:uuiiiifffpppppp",
    "fr_synth_texture":                               "i:pppiiipp",
    "fr_synth_shade":                                 "i:pppppiiiiffppp",
    "fr_synth_texture_backward_workspace_bytes":      "z:iii",
    "fr_synth_texture_backward":                      "i:ppiiippzp",
    "fr_photo_loss_state_bytes":                      "z:iii",
    "fr_photo_loss_forward":                          "i:ppppppiiiffppzp",
    "fr_photo_loss_backward":                         "i:ppppppppiiiffpppp",
    "fr_debug_photo_loss_geom":                       "v:iiiI",
    "fr_synth_light_rgb":                             "i:uuippp",
    "fr_synth_shade_rgb":                             "i:pppppiiiiffpppp",
    "fr_photo_loss_rgb_state_bytes":                  "z:iii",
    "fr_photo_loss_rgb_forward":                      "i:ppppppiiiffppzp",
    "fr_photo_loss_rgb_backward":                     "i:ppppppppiiiffpppp",
    "fr_debug_photo_loss_rgb_geom":                   "v:iiiI",
    "fr_albedo_basis_rgb_bytes":                      "z:ii",
    "fr_albedo_basis_rgb_build":                      "i:pppiiipzp",
    "fr_albedo_image_rgb":                            "i:pppiiiiipp",
    "fr_photo_solve_rgb_workspace_bytes":             "z:iii",
    "fr_photo_light_lse_rgb_forward":                 "i:ppppppiiiffdppppzp",
    "fr_albedo_lse_rgb_forward":                      "i:ppppppiiiiiffdppppzp",
    "fr_debug_photo_solve_rgb_geom":                  "v:iiiI",
    "fr_mesh_visible":                                "i:ppiiiiipp",
    "fr_mesh_lift":                                   "i:pippppiiiiipipp",
    "fr_mesh_vertex_normals":                         "i:pipppiiipip",
    "fr_attr_interp_forward":                         "i:pipippiiiiipp",
    "fr_attr_interp_backward":                        "i:ppipipppipiiiiiippp",
    "fr_mesh_vertex_normals_backward":                "i:pipipppiiippiip",
    "fr_debug_attr_interp_bwd_geom":                  "v:iiiiI",
    "fr_coverage_forward":                            "i:pippiiiiipp",
    "fr_coverage_backward_workspace_bytes":           "z:iiii",
    "fr_coverage_backward":                           "i:pppipppiiiiiipzp",
    "fr_debug_coverage_bwd_geom":                     "v:iiiiI",
    "fr_landmark_basis_bytes":                        "z:iii",
    "fr_landmark_basis_build":                        "i:ppppiiiipzp",
    "fr_landmark_forward":                            "i:ppzpppiiiiifppp",
    "fr_landmark_backward":                           "i:ppppzpppiiiiifppip",
    "fr_landmark_solve_workspace_bytes":              "z:iii",
    "fr_landmark_solve_step":                         "i:ppzppipppiiiiiifppppzp",
    "fr_landmark_contour_select":                     "i:ppzpppippipiiiiiiifppppp",
    "fr_debug_render_geom":                           "v:iiiiiI",
    "fr_debug_decode_bwd_geom":                       "v:iiiiI",
    "fr_debug_decode_geom":                           "i:iiiiiI",
    "fr_debug_decode_q_geom":                         "i:iiiiiiI",
    "fr_debug_decode_walk":                           "i:iiiiI",
    "fr_debug_pose_bwd_geom":                         "v:iiI",
    "fr_debug_render_bwd_geom":                       "v:iiiiI",
    "fr_debug_div3_sweep":                            "i:uupp",
    "fr_debug_clock_probe":                           "i:piip",
}
EXPORTS = list(SIGNATURES)


def bind(cdll, names=None):
    """Sets restype / argtypes on a loaded library, ours or another build of it: every entry point of SIGNATURES, or `names`
    alone (a library built from one source file exports only that file's)."""
    for name in (SIGNATURES if names is None else names):
        ret, args = SIGNATURES[name].split(":")
        fn = getattr(cdll, name)
        fn.restype = _CTYPE[ret]
        fn.argtypes = [_CTYPE[c] for c in args]
    return cdll


def lib():
    """Returns the bound ctypes library.  The .so is (re)built first when it is missing or stale -- built from other
    sources than the tree holds -- (the reference's build-on-import fallback, rendering_layer/ops.py:63-72); a stale
    binary that cannot be rebuilt is refused, never loaded.  Raises if it can be neither built nor loaded."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                import torch  # noqa: F401  (loads the ROCm runtime this library binds to, by SONAME)
                if is_stale():
                    compile()
                try:
                    L = bind(ctypes.CDLL(LIB_PATH))
                except OSError as e:
                    raise RuntimeError("fr_hotpath: cannot load %s (%s); run compile() -- there is no CPU fallback"
                                       % (LIB_PATH, e))
                want = src_hash()
                if want is not None and want.encode() not in L.fr_version():
                    raise RuntimeError("fr_hotpath: %s reports %r but the sources hash to %s: stale binary refused"
                                       % (LIB_PATH, L.fr_version(), want))
                _lib = L
    return _lib


# ---- host-side choices --------------------------------------------------------------------------------------------
DECODE_ARITH_Q30, DECODE_ARITH_F32 = 0, 1
# This file is loaded under two module names (the package's `3dfacerecon_amd._lib`, and by path from the reference-style
# flat modules rendering_layer/ops.py, nets/network.py, pipeline.py): process-wide choices live in ONE shared namespace.
_STATE = sys.modules.setdefault("_fr_hotpath_state", types.SimpleNamespace(decode_arith=None, q30_levels=7, option_epoch=0,
                                                                           pools={}))
_ARITH_ENV = {"q30": 7, "q30l7": 7, "q30l5": 5, "q30l4": 4}


def _torch_stream_key(dev):
    import torch
    return (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream,
            torch.cuda.is_current_stream_capturing())


class StreamBuffers:
    """Device buffers that live from call to call, one per (kind, device, stream): a bounded pool.  What is kept in one is dead
    once the call that wrote it has been enqueued -- the render forward writes every part of its workspace (hit records, bucket
    offsets, tables: ~330 MB at 64 faces) that it later reads and its backward needs none of it; a loss's partial sums are
    consumed by its own finish launch -- and launches on one stream are ordered, so consecutive calls on a stream share a buffer
    where the reference cudaMallocs / cudaFrees six per call (render_depth_op.cu.cc:272-277, 335-340).  The rules:

      R1  A pooled buffer is handed out only inside a hold -- `with pool.hold(kind, dev, nbytes) as ent:` -- and the entry's lock
          is held until the with-block is left, i.e. until the C call that launches on `ent.buf` has returned.  Threads that share
          a stream (every thread that sets none shares torch's default stream) share its entries, and one call's kernels must not
          land between another call's launches on the same buffer.  The launches are asynchronous: the lock is held for
          microseconds.  `ent.note` is the holder's own slot, read and written under the same lock (the render path keeps there
          which triangle list the table in its workspace was packed from).
      R2  A request larger than the entry replaces the entry: a new buffer, a new lock, an empty note.  A thread still inside a
          hold on the old entry keeps the old buffer alive until it lets go.
      R3  While the current stream is being captured into a hipGraph the hold yields a fresh entry that is never inserted, and
          the pool is left exactly as it was: a captured launch must not point at a buffer the pool may later replace, so the
          capture gets one of its own from the graph's memory pool.
      R4  Lock order: an entry's lock, then the pool's dict lock.  The dict lock is a leaf -- taken for the lookup alone and
          released before the entry's lock is waited for.  Holds nest in one place, render workspace -> "hand"
          (rendering_layer/ops.py, _DecodeRenderingLayer.forward), and always in that order.
      R5  Process-wide: the named pools (stream_buffers()) live in the namespace both loads of this file share, so every module
          name this package is loaded under finds the same buffers.
      Bounded: at most `bound` entries, the least recently used dropped first (a caller that cycles streams does not accumulate a
      buffer per stream handle it ever used); clear() drops them all.  No buffer is smaller than `floor` bytes.

    `alloc(nbytes, dev)` and `stream_key(dev)` -> (device index, stream handle, whether the stream is being captured) default to
    torch's; a test without a GPU passes its own.  An entry carries the handle it was taken on as `stream`: a host-bound holder
    launches on it without asking torch a second time."""

    class Entry:
        __slots__ = ("buf", "nbytes", "stream", "lock", "note", "pooled")

        def __init__(self, buf, nbytes, stream, pooled):
            self.buf, self.nbytes, self.stream, self.pooled = buf, nbytes, stream, pooled
            self.lock = threading.Lock()
            self.note = None

    class _Hold:
        __slots__ = ("ent", "asked")

        def __init__(self, ent, asked):
            self.ent, self.asked = ent, asked

        def __enter__(self):
            self.ent.lock.acquire()
            return self.ent if self.asked is None else (self.asked, self.ent.buf)

        def __exit__(self, *exc):
            self.ent.lock.release()
            return False

    def __init__(self, bound, floor, alloc=None, stream_key=None):
        self.bound, self.floor = bound, floor
        self._alloc = alloc if alloc is not None else byte_buffer
        self._stream_key = stream_key if stream_key is not None else _torch_stream_key
        self._entries = {}   # (insertion order = least recently used first)
        self._lock = threading.Lock()

    def __len__(self):
        return len(self._entries)

    def clear(self):
        with self._lock:
            self._entries.clear()

    def snapshot(self):
        """{(kind, device index, stream handle): entry}, least recently used first"""
        with self._lock:
            return dict(self._entries)

    def hold(self, kind, dev, nbytes, sized=False):
        """The context manager of R1: entering it takes the entry's lock and gives the entry (`buf`: at least nbytes bytes) --
        sized=True: the pair (nbytes, buf) instead, for a caller that hands exactly these two to its C call."""
        asked = nbytes if sized else None
        index, stream, capturing = self._stream_key(dev)
        if capturing:
            n = max(nbytes, self.floor)
            return self._Hold(self.Entry(self._alloc(n, dev), n, stream, False), asked)
        key = (kind, index, stream)
        with self._lock:
            ent = self._entries.pop(key, None)
            if ent is None or ent.nbytes < nbytes:
                n = max(nbytes, self.floor)
                ent = self.Entry(self._alloc(n, dev), n, stream, True)
            self._entries[key] = ent   # (re-inserted last: most recently used)
            while len(self._entries) > self.bound:
                del self._entries[next(iter(self._entries))]
        return self._Hold(ent, asked)


def stream_buffers(name, bound, floor):
    """The process-wide pool of that name (R5), created at the first request."""
    pool = _STATE.pools.get(name)
    if pool is None:
        pool = _STATE.pools.setdefault(name, StreamBuffers(bound, floor))
    return pool


def decode_arith():
    """Which written definition of the basis blend the Python callers (FaceRecNet.vertices_transform, DecodeRenderPlan)
    use: DECODE_ARITH_F32 (default: fr_decode_3dmm, the k-ordered fmaf chain) or DECODE_ARITH_Q30 (fr_decode_3dmm_q30_lv,
    the fixed-point blend on the int8 matrix cores with q30_levels() digit-product levels; its image and workspace are built
    on first use).  Process-wide; the initial value comes from the environment variable FR_DECODE_ARITH = "f32" | "q30"
    (all seven levels) | "q30l5" | "q30l4", read once."""
    if _STATE.decode_arith is None:
        lv = _ARITH_ENV.get(os.environ.get("FR_DECODE_ARITH", ""))
        _STATE.decode_arith = DECODE_ARITH_Q30 if lv else DECODE_ARITH_F32
        if lv:
            _STATE.q30_levels = lv
    return _STATE.decode_arith


def q30_levels():
    """Digit-product levels of the Q30 blend (include/fr_hotpath.h): 7 = the exact product, 5, or 4."""
    decode_arith()
    return _STATE.q30_levels


def set_decode_arith(mode, levels=None):
    if mode not in (DECODE_ARITH_Q30, DECODE_ARITH_F32):
        raise ValueError("decode arithmetic must be DECODE_ARITH_F32 or DECODE_ARITH_Q30")
    if levels is not None and int(levels) not in (4, 5, 7):
        raise ValueError("Q30 levels must be 7, 5 or 4")
    decode_arith()
    _STATE.decode_arith = mode
    if levels is not None:
        _STATE.q30_levels = int(levels)


def set_option(name, value):
    """fr_set_option: a launcher knob by its FR_* name (the environment is only read once, at the first launch).  Every
    change bumps option_epoch(): host-side caches of what a launch left in a workspace (rendering_layer/ops.py: the packed
    triangle table) are keyed on it, since some knobs decide whether and how that state is written."""
    check(lib().fr_set_option(name.encode(), int(value)), "fr_set_option(%s)" % name)
    _STATE.option_epoch += 1


def option_epoch():
    return _STATE.option_epoch


def get_option(name):
    v = ctypes.c_int(0)
    check(lib().fr_get_option(name.encode(), ctypes.byref(v)), "fr_get_option(%s)" % name)
    return v.value


class options:
    """Context manager for A/B runs and tests: `with options(FR_EMIT_FILTER=0): ...` sets the knobs and restores them."""

    def __init__(self, **kv):
        self.kv = kv
        self.old = {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def check(rc, what):
    if rc != FR_OK:
        msg = _ERR_NAMES.get(rc, "unknown error %d" % rc)
        if rc == -1:
            raise ValueError("%s: %s" % (what, msg))
        raise RuntimeError("%s: %s" % (what, msg))


def require_gpu_f32(t, name):
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: the fr_hotpath kernels run on an MI355X only (no CPU fallback)"
                           % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    return t.contiguous()


def byte_buffer(nbytes, dev, floor=16):
    """A fresh device buffer of nbytes bytes, never smaller than `floor` (a size query may answer 0; a pointer must exist)."""
    import torch
    return torch.empty((max(nbytes, floor),), dtype=torch.uint8, device=dev)


def stream_ptr(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None
