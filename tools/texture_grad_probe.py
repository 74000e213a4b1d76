#!/usr/bin/env python3
"""What the texture gradients cost, in ONE process through the raw C ABI (modelled on tools/normal_grad_probe.py): alternating
rounds, device events, medians, the full-size mesh at 200 x 200.

  'depth'          = fr_render_depth_backward_ws alone                              (the z-only backward every caller runs)
  'tex_per_face'   = fr_render_texture_backward, tex_batch == B, dense [B,H,W,3] gradient, accumulate 0
  'tex_shared'     = fr_render_texture_backward, tex_batch == 1 (what compute_abedo_image passes): face slices, integer slabs
                     in the workspace, the finish kernel
  'sfs_bwd'        = fr_sfs_intensity_backward, grad_normal_new only                (the SfS backward without the albedo output)
  'sfs_bwd_tex'    = fr_sfs_intensity_backward_tex, grad_normal_new and grad_abedo_new

Beside the new call: the bytes it must move -- tex_grad and tri_ind read (16 B per pixel), the id gathers (12 B per covered
pixel), three rows written (12 B per vertex and texture) -- the time those take at the measured copy rate of 6.29 TB/s, and the
bytes its own scheme moves on top (24-byte records written for the covered pixels, the id plane re-read by every owner, the
slabs of the shared texture written and read once).  The clock the part holds is read behind the timed rounds
(fr_debug_clock_probe).  The results are also compared with a float64 scatter of the call's terms (recorded, not asserted).

--trace: a few calls of each route and nothing else, for a `rocprofv3 --kernel-trace --stats -- python tools/texture_grad_probe.py
--trace` run of its own (per-kernel times).  --out FILE: where the JSON goes besides stdout (default
profiles/render_texture_backward.json)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s: the measured device-to-device copy figure of the part

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_texture_backward.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("texture_grad_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
H = W = 200
GEOM = ("owners_per_face_or_slice", "vertices_per_owner", "shift", "chunks", "lds_bytes", "xcd_map", "face_slices")


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / calls * 1e3, 2)


def summary(xs):
    return {"us": xs, "median": round(statistics.median(xs), 2), "spread_max_minus_min": round(max(xs) - min(xs), 2)}


def clock_ghz():
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ticks = torch.zeros((cus, 2), dtype=torch.int64, device=dev)
    assert L.fr_debug_clock_probe(h.ptr(ticks), cus, int(2e-3 * 2.1e9 / (6 * 32 * 4)), st) == 0
    torch.cuda.synchronize()
    t = ticks.cpu().double()
    return round(float((0.1 * t[:, 0] / t[:, 1].clamp(min=1)).median()), 3)


def float64_check(got, g, tri, tind, faces, nver):
    """the result against a float64 scatter of g / 3 formed with torch on the device, summed over `faces`: the largest
    |difference| over the largest |value| (a transposition or a sign could not hide; the tests hold the bits to the model)"""
    want = torch.zeros((3, nver), dtype=torch.float64, device=dev)
    for b in faces:
        t = tind[b].reshape(-1).long()
        px = (t >= 0).nonzero().squeeze(1)
        ids = tri[:, t[px]].long()
        term = (g[b].reshape(-1, 3)[px].double() / 3.0).T.contiguous()
        for k in range(3):
            want.index_add_(1, ids[k], term)
    return float((got.double() - want).abs().max() / want.abs().max())


out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    N, ntri = net.nvert, int(net.tri.shape[1])
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    V = net.vertices_transform(P).detach().contiguous()
    tri_ind = ops.render_depth(V, net.tri, net.vertex_code, torch.zeros((B, H, W, 3), **o))[3].contiguous()
    covered = int((tri_ind >= 0).sum())
    gd, g3 = torch.randn((B, H, W, 1), **o), torch.randn((B, H, W, 3), **o)
    ndw = L.fr_render_depth_backward_workspace_bytes(B, H, W)
    dws = torch.empty((ndw,), dtype=torch.uint8, device=dev)
    vg = torch.empty((B, 3, N), **o)
    tws, tg, geo = {}, {}, {}
    for tb in (B, 1):
        n = L.fr_render_texture_backward_workspace_bytes(B, N, H, W, tb)
        tws[tb] = (torch.empty((n,), dtype=torch.uint8, device=dev), n)
        tg[tb] = torch.empty((tb, 3, N), **o)
        geo[tb] = (ctypes.c_int * 7)()
        L.fr_debug_render_texture_bwd_geom(B, N, H, W, tb, geo[tb])
    # the SfS backward on maps of the same shape
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)   # noqa: E731
    nm, nm2 = unit(torch.randn((B, H, W, 3), **o)), unit(torch.randn((B, H, W, 3), **o))
    al, al2, im, gi = (torch.rand((B, H, W, 1), **o) for _ in range(4))
    nst = L.fr_sfs_state_bytes(H, W)
    state = torch.empty((nst // 8,), dtype=torch.float64, device=dev)
    inten, gnn, gan = torch.empty((B, H, W, 1), **o), torch.empty((B, H, W, 3), **o), torch.empty((B, H, W, 1), **o)
    assert L.fr_sfs_intensity_forward(h.ptr(al), h.ptr(nm), h.ptr(im), h.ptr(al2), h.ptr(nm2), B, H, W, 1e-6, h.ptr(inten),
                                      h.ptr(state), nst, st) == 0

    def depth():
        return L.fr_render_depth_backward_ws(h.ptr(gd), h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W, h.ptr(dws), ndw, st)

    def tex(tb):
        return L.fr_render_texture_backward(h.ptr(g3), 3, h.ptr(net.tri), h.ptr(tri_ind), h.ptr(tg[tb]), B, N, ntri, H, W, tb, 0,
                                            h.ptr(tws[tb][0]), tws[tb][1], st)

    def sfs_bwd():
        return L.fr_sfs_intensity_backward(h.ptr(gi), h.ptr(al), h.ptr(im), h.ptr(al2), h.ptr(nm2), h.ptr(state), nst, B, H, W, None,
                                           h.ptr(gnn), st)

    def sfs_bwd_tex():
        return L.fr_sfs_intensity_backward_tex(h.ptr(gi), h.ptr(al), h.ptr(im), h.ptr(al2), h.ptr(nm2), h.ptr(state), nst, B, H, W,
                                               None, h.ptr(gnn), h.ptr(gan), st)
    routes = {"depth": depth, "tex_per_face": lambda: tex(B), "tex_shared": lambda: tex(1), "sfs_bwd": sfs_bwd,
              "sfs_bwd_tex": sfs_bwd_tex}
    for fn in routes.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    if args.trace:
        for fn in routes.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        continue
    agree = {"tex_per_face_face0": float64_check(tg[B][0], g3, net.tri, tri_ind, (0,), N),
             "tex_shared": float64_check(tg[1][0], g3, net.tri, tri_ind, range(B), N)}
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rec["clock_GHz_held"] = clock_ghz()
    rec["bytes"], rec["geometry"] = {}, {}
    for name, tb in (("tex_per_face", B), ("tex_shared", 1)):
        g = geo[tb]
        must = B * H * W * 16 + covered * 12 + tb * 3 * N * 4
        slabs = g[6] * 3 * N * 8
        scheme = covered * 24 + g[0] * B * H * W * 16 + covered * 8 + 2 * slabs
        t = rec[name]["median"]
        rec[name + "_vs_bytes"] = {"time_at_copy_rate_us": round(must / COPY_RATE * 1e6, 2),
                                   "fraction_of_copy_rate": round(must / COPY_RATE * 1e6 / t, 3)}
        rec["bytes"][name] = {"must_move": must, "tex_grad_and_tri_ind_read": B * H * W * 16, "id_gathers": covered * 12,
                              "rows_written": tb * 3 * N * 4, "scheme_on_top": scheme, "records_written": covered * 24,
                              "id_plane_read_by_every_owner": g[0] * B * H * W * 16, "second_plane_read": covered * 8,
                              "slabs_written_and_read": 2 * slabs}
        rec["geometry"][name] = dict(zip(GEOM, g))
    sfs_must = B * H * W * 4 * (1 + 1 + 3 + 3) + 3 * H * W * 8          # g, abedo_new, normal_new read, grad_normal_new written, l
    rec["bytes"]["sfs_bwd"] = {"must_move": sfs_must, "time_at_copy_rate_us": round(sfs_must / COPY_RATE * 1e6, 2)}
    rec["bytes"]["sfs_bwd_tex"] = {"must_move": sfs_must + B * H * W * 4,
                                   "time_at_copy_rate_us": round((sfs_must + B * H * W * 4) / COPY_RATE * 1e6, 2)}
    rec["covered_pixels"] = covered
    rec["vs_float64_scatter_max_rel"] = agree
    rec["albedo_output_adds_us"] = round(rec["sfs_bwd_tex"]["median"] - rec["sfs_bwd"]["median"], 2)
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

if not args.trace:
    doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, raw C ABI, full-size "
                   "mesh (N = 53,215, 105,840 triangles) at 200 x 200; tex_per_face / tex_shared = fr_render_texture_backward with "
                   "tex_batch == B / == 1 (dense gradient, accumulate 0); depth = fr_render_depth_backward_ws on the same tri_ind; "
                   "sfs_bwd / sfs_bwd_tex = the SfS backward writing grad_normal_new without / with grad_abedo_new; must_move = the "
                   "bytes any scheme moves, fraction_of_copy_rate = (must_move / 6.29 TB/s) / time; scheme_on_top = what the records "
                   "pass, the owners and the slabs move besides (mostly L2 traffic: every owner re-reads the id plane of its faces).  "
                   "Only the integer-slab reduction of the shared texture was built; the 64-bit global atomic form was not."
                   % (args.calls, args.rounds),
           "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
           "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
