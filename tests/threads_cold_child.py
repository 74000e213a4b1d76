"""Child process of tests/test_threads_gpu.py::test_cold_start_every_entry_point_at_once (not a test module).

`python threads_cold_child.py DIR` loads the library and starts one thread per job of JOBS on a barrier.  Apart from loading the
library (fr_version) and packing the Q30 image, nothing calls into it before the barrier -- every buffer size comes from
DIR/sizes.json, written by the parent -- so the jobs' launches are the process's first: the option table and the per-device
launch-attribute caches are cold when eight threads reach them at once.  Each thread has its own stream and its own output and
workspace buffers.  The results go to DIR/out_<job>_<name>.npy; the parent holds them to its own single-threaded references.

The parent imports this file too: run_job() is the one definition of every job, for the references and for the threads."""
import ctypes
import importlib
import json
import os
import sys
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

JOBS = ("decode", "decode_q30", "render", "render_phases", "layer", "render_bwd", "decode_bwd", "decode_render")
Q30_LEVELS = 7


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def upload(inputs, dev):
    import torch
    return {k: torch.as_tensor(np.ascontiguousarray(v), device=dev) for k, v in inputs.items()}


def prepare(job, T, S, dev):
    """Every buffer of `job` (outputs filled with 7.0, so an unwritten element shows), allocated with torch only."""
    import torch
    f32 = dict(dtype=torch.float32, device=dev)
    B, N, H, W = S["B"], S["N"], S["H"], S["W"]
    b = {}

    def ws(n):
        return torch.empty((max(n, 16),), dtype=torch.uint8, device=dev)

    if job in ("decode", "decode_render"):
        b["image"] = ws(S["packed_basis_bytes"])
    if job == "decode":
        b["out"] = torch.full((B, 3, N), 7.0, **f32)
    elif job == "decode_q30":
        b["out"] = torch.full((B, 3, N), 7.0, **f32)
        b["ws"] = ws(S["q30_ws_bytes"])
    elif job in ("render", "render_phases", "decode_render"):
        for k, c in (("depth", 1), ("tex_img", 3), ("normal", 3), ("tri_ind", 1)):
            b[k] = torch.full((B, H, W, c), 7.0, **f32)
        b["ws"] = ws(S["render_ws_bytes"])
        if job == "decode_render":
            b["vertex"] = torch.full((B, 3, S["pitch"]), 7.0, **f32)
    elif job == "layer":
        for k, c in (("net_in", 7), ("depth_img", 1), ("depth", 1), ("tri_ind", 1)):
            b[k] = torch.full((B, H, W, c), 7.0, **f32)
        b["ws"] = ws(S["render_ws_bytes"])
    elif job == "render_bwd":
        b["vg_ws"] = torch.full((B, 3, N), 7.0, **f32)
        b["vg"] = torch.full((B, 3, N), 7.0, **f32)
        b["ws"] = ws(S["render_bwd_ws_bytes"])
    elif job == "decode_bwd":
        b["gp"] = torch.full(tuple(T["P"].shape), 7.0, **f32)
        b["ws"] = ws(S["decode_bwd_ws_bytes"])
    return b


def pack_q30(L, T, S, qimage, st):
    rc = L.fr_decode_q30_pack(_p(T["mu"]), _p(T["pc_shape"]), _p(T["pc_exp"]), S["N"], S["ns"], S["ne"], _p(qimage),
                              S["q30_image_bytes"], st)
    assert rc == 0, ("fr_decode_q30_pack", rc)


def run_job(L, job, T, S, b, st, qimage=None):
    """Launches `job` on stream `st` (a c_void_p) -> {name: output tensor}.  Raises on a non-zero return code."""
    B, N, ns, ne, T_, H, W = S["B"], S["N"], S["ns"], S["ne"], S["ntri"], S["H"], S["W"]
    im = ctypes.c_float(S["im"])
    rcs = []
    if job in ("decode", "decode_render"):   # its own copy of the packed basis, on its own stream: the job's first call
        rcs.append(L.fr_decode_pack_basis(_p(T["mu"]), _p(T["pc_shape"]), _p(T["pc_exp"]), N, ns, ne, _p(b["image"]),
                                          S["packed_basis_bytes"], st))
    if job == "decode":
        rcs.append(L.fr_decode_3dmm(_p(T["P"]), _p(b["image"]), _p(T["R"]), B, N, ns, ne, im, _p(b["out"]), st))
        names = ("out",)
    elif job == "decode_q30":
        rcs.append(L.fr_decode_3dmm_q30_lv(_p(T["P"]), _p(qimage), _p(T["R"]), B, N, ns, ne, im, Q30_LEVELS, _p(b["out"]),
                                           _p(b["ws"]), S["q30_ws_bytes"], st))
        names = ("out",)
    elif job in ("render", "render_phases"):
        args = (_p(T["V"]), _p(T["tri"]), _p(T["tex"]), B, N, T_, H, W, 3, 1, _p(b["depth"]), _p(b["tex_img"]), _p(b["normal"]),
                _p(b["tri_ind"]), _p(b["ws"]), S["render_ws_bytes"], st)
        rcs.append(L.fr_render_depth_forward(*args) if job == "render" else L.fr_render_depth_forward_phases(*args, 7))
        names = ("depth", "tex_img", "normal", "tri_ind")
    elif job == "layer":
        rcs.append(L.fr_rendering_layer_forward(_p(T["V"]), _p(T["tri"]), _p(T["tex"]), _p(T["im_gray"]), B, N, T_, H, W, 1,
                                                _p(b["net_in"]), _p(b["depth_img"]), _p(b["depth"]), _p(b["tri_ind"]),
                                                _p(b["ws"]), S["render_ws_bytes"], st))
        names = ("net_in", "depth_img", "depth", "tri_ind")
    elif job == "render_bwd":
        rcs.append(L.fr_render_depth_backward_ws(_p(T["G_px"]), _p(T["tri"]), _p(T["tri_ind"]), _p(b["vg_ws"]), B, N, T_, H, W,
                                                 _p(b["ws"]), S["render_bwd_ws_bytes"], st))
        rcs.append(L.fr_render_depth_backward(_p(T["G_px"]), _p(T["tri"]), _p(T["tri_ind"]), _p(b["vg"]), B, N, T_, H, W, st))
        names = ("vg_ws", "vg")
    elif job == "decode_bwd":
        rcs.append(L.fr_decode_3dmm_backward(_p(T["G_v"]), _p(T["P"]), _p(T["V"]), _p(T["pc_shape"]), _p(T["pc_exp"]),
                                             _p(T["R"]), B, N, ns, ne, im, _p(b["gp"]), _p(b["ws"]), S["decode_bwd_ws_bytes"],
                                             st))
        names = ("gp",)
    elif job == "decode_render":
        rcs.append(L.fr_decode_render_forward(_p(T["P"]), _p(b["image"]), _p(T["R"]), _p(T["tri"]), _p(T["tex"]), B, N, ns, ne,
                                              T_, H, W, 1, im, _p(b["vertex"]), S["vertex_bytes"], _p(b["depth"]),
                                              _p(b["tex_img"]), _p(b["normal"]), _p(b["tri_ind"]), _p(b["ws"]),
                                              S["render_ws_bytes"], st, 15))
        names = ("vertex", "depth", "tex_img", "normal", "tri_ind")
    else:
        raise ValueError(job)
    if any(rcs):
        raise RuntimeError("%s: return codes %s" % (job, rcs))
    return {n: b[n] for n in names}


def main(d):
    import torch
    sys.path.insert(0, ROOT)
    h = importlib.import_module("3dfacerecon_amd._lib")
    L = h.lib()                                   # (fr_version only: the build identity check)
    S = json.load(open(os.path.join(d, "sizes.json")))
    z = np.load(os.path.join(d, "inputs.npz"))
    dev = torch.device("cuda:0")
    T = upload({k: z[k] for k in z.files}, dev)
    streams = {j: torch.cuda.Stream(device=dev) for j in JOBS}
    bufs = {j: prepare(j, T, S, dev) for j in JOBS}
    qimage = torch.empty((max(S["q30_image_bytes"], 256),), dtype=torch.uint8, device=dev)
    pack_q30(L, T, S, qimage, ctypes.c_void_p(streams["decode_q30"].cuda_stream))
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(JOBS))

    def work(j):
        st = streams[j]
        barrier.wait(timeout=60)
        out = run_job(L, j, T, S, bufs[j], ctypes.c_void_p(st.cuda_stream), qimage)
        st.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    with ThreadPoolExecutor(max_workers=len(JOBS)) as ex:
        futs = {j: ex.submit(work, j) for j in JOBS}
        res = {j: f.result(timeout=120) for j, f in futs.items()}
    for j, outs in res.items():
        for k, v in outs.items():
            np.save(os.path.join(d, "out_%s_%s.npy" % (j, k)), v)
    print("cold start: %d jobs done" % len(res))


if __name__ == "__main__":
    main(sys.argv[1])
