#!/usr/bin/env python3
"""What the fine mesh costs, in ONE process through the raw C ABI (modelled on tools/depth_interp_probe.py): alternating rounds, device
events, medians of the rounds, the full-size mesh at 200 x 200, 32 and 64 faces.

  'visible'        = fr_mesh_visible          (a memset of the plane and one pass over the pixels)
  'lift'           = fr_mesh_lift             (one lane per (face, vertex): copies x and y, samples fine - coarse for z)
  'normals'        = fr_mesh_vertex_normals   (one lane per (face, vertex): the CSR gather)
  'torch_visible'  = the same plane from stock torch ops: mask, gather of the ids, index_put_
  'torch_lift'     = the same lift from stock torch ops: four masked corner gathers, weights, sums (float64)
  'torch_normals'  = the same normals from stock torch ops: facet cross products, three index_add_, normalise (float64 sums)
  'copy'           = a device-to-device copy of 512 MiB: the copy rate of THIS run, which prices the bytes below

Beside each kernel: the bytes it must move -- visible: tri_ind read (4 B per pixel), the id gathers of the covered pixels (12 B), the
plane written (1 B per vertex); lift: three rows read and written, visible read, state written (26 B per vertex) and the corners of
the lifted vertices (up to 4 x 12 B); normals: three rows read once and three written (24 B per vertex) and the tables once -- the
time those take at the run's copy rate, and what the gathers move on top (out of L2: 52 B per (face, vertex, triangle) for the
normals).  The kernels' results are compared with the stock-torch ones (recorded, not asserted: the tests hold the bits).

--trace: a few calls of each route and nothing else, for a `rocprofv3 --kernel-trace --stats -- python tools/fine_mesh_probe.py --trace`
run of its own.  --out FILE: where the JSON goes besides stdout (default profiles/fine_mesh.json)."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_mesh.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("fine_mesh_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
H = W = 200
COPY_BYTES = 512 << 20


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


out = {}
src = torch.empty((COPY_BYTES // 4,), dtype=torch.float32, device=dev).normal_()
dst = torch.empty_like(src)
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    N, ntri = net.nvert, int(net.tri.shape[1])
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    V = net.vertices_transform(P).detach().contiguous()
    r = ops.render_depth(V, net.tri, net.vertex_code, torch.zeros((B, H, W, 3), **o))
    tri_ind, coarse = r[3].contiguous(), r[0].clamp_min(1e-6).contiguous()
    fine = (coarse + 0.01 * torch.randn_like(coarse)).contiguous()
    covered = int((tri_ind >= 0).sum())
    adj = net.adjacency()
    entries = int(adj.adj_start[-1])
    visible = torch.empty((B, N), dtype=torch.uint8, device=dev)
    state = torch.empty((B, N), dtype=torch.uint8, device=dev)
    Vf, Nf = torch.empty((B, 3, N), **o), torch.empty((B, 3, N), **o)
    tri_l = net.tri.long()
    face_of = torch.arange(B, device=dev)[:, None]

    def k_visible():
        return L.fr_mesh_visible(h.ptr(net.tri), h.ptr(tri_ind), B, N, ntri, H, W, h.ptr(visible), st)

    def k_lift():
        return L.fr_mesh_lift(h.ptr(V), N, h.ptr(tri_ind), h.ptr(visible), h.ptr(fine), h.ptr(coarse), B, N, ntri, H, W, h.ptr(Vf), N,
                              h.ptr(state), st)

    def k_normals():
        return L.fr_mesh_vertex_normals(h.ptr(Vf), N, h.ptr(net.tri), h.ptr(adj.adj_start), h.ptr(adj.adj_tri), B, N, ntri, h.ptr(Nf), N,
                                        st)

    def t_visible():
        t = tri_ind.reshape(B, -1).long()
        ok = t >= 0
        ids = tri_l[:, t.clamp_min(0)]                                        # [3,B,HW]
        vis = torch.zeros((B, N + 1), dtype=torch.uint8, device=dev)
        for k in range(3):
            vis.index_put_((face_of.expand_as(t), torch.where(ok, ids[k], N)), torch.ones((), dtype=torch.uint8, device=dev))
        t_visible.out = vis[:, :N]
        return 0

    def t_lift():
        x, y, z = V[:, 0].double(), V[:, 1].double(), V[:, 2].double()
        c0, r0 = x.floor(), y.floor()
        fx, fy = x - c0, y - r0
        diff = (fine.double() - coarse.double()).reshape(B, -1)
        on = (tri_ind >= 0).reshape(B, -1)
        num, den = torch.zeros_like(x), torch.zeros_like(x)
        for dr, dc, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
            rr, cc = r0 + dr, c0 + dc
            inside = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
            idx = torch.where(inside, rr * W + cc, torch.zeros_like(rr)).long()
            use = inside & (w != 0) & on.gather(1, idx)
            num = num + torch.where(use, w * diff.gather(1, idx), torch.zeros_like(w))
            den = den + torch.where(use, w, torch.zeros_like(w))
        seen = visible.bool()
        lifted = seen & (den > 0)
        t_lift.out = torch.where(lifted, z + num / den.clamp_min(1e-300), z).float()
        t_lift.state = torch.where(seen, torch.where(lifted, 1, 2), 0).to(torch.uint8)
        return 0

    def t_normals():
        Q = Vf.double()
        P1, P2, P3 = (Q[:, :, tri_l[k]] for k in range(3))
        n = torch.cross(P2 - P1, P3 - P1, dim=1)
        acc = torch.zeros((B, 3, N), dtype=torch.float64, device=dev)
        for k in range(3):
            acc.index_add_(2, tri_l[k], n)
        s = acc.norm(dim=1, keepdim=True)
        t_normals.out = torch.where(s > 0, acc / s.clamp_min(1e-300), torch.zeros_like(acc)).float()
        return 0

    def copy():
        dst.copy_(src)
        return 0
    routes = {"visible": k_visible, "lift": k_lift, "normals": k_normals, "torch_visible": t_visible, "torch_lift": t_lift,
              "torch_normals": t_normals, "copy": copy}
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
    lifted = int((state == 1).sum())
    agree = {"visible_equal": bool(torch.equal(visible, t_visible.out)), "state_equal": bool(torch.equal(state, t_lift.state)),
             "lift_max_abs_diff": float((Vf[:, 2] - t_lift.out).abs().max()),
             "normals_max_abs_diff": float((Nf - t_normals.out).abs().max())}
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, fn in routes.items():
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    rate = 2 * COPY_BYTES / (rec["copy"]["median"] * 1e-6)
    rec["copy_rate_bytes_per_s"] = round(rate, -9)
    must = {"visible": B * H * W * 4 + covered * 12 + B * N,
            "lift": B * N * 26 + lifted * 4 * 12,
            "normals": B * N * 24 + ntri * 12 + 3 * ntri * 4 + (N + 1) * 4}
    for k, m in must.items():
        t = rec[k]["median"]
        rec[k + "_vs_bytes"] = {"must_move": m, "time_at_copy_rate_us": round(m / rate * 1e6, 2),
                                "fraction_of_copy_rate": round(m / rate * 1e6 / t, 3),
                                "stock_torch_over_kernel": round(rec["torch_" + k]["median"] / t, 1)}
    rec["bytes"] = {"normals_gathers_out_of_l2": B * entries * 52, "visible_marks": covered * 3}
    rec["covered_pixels"], rec["visible_vertices"], rec["lifted_vertices"] = covered, int(visible.sum()), lifted
    rec["adjacency_entries"] = entries
    rec["vs_stock_torch"] = agree
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

if not args.trace:
    doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds (medians of the rounds; spread = max - "
                   "min of the rounds), one process, raw C ABI, full-size mesh (N = 53,215, 105,840 triangles) at 200 x 200; visible / "
                   "lift / normals = fr_mesh_visible / fr_mesh_lift / fr_mesh_vertex_normals; torch_* = the same operator composed "
                   "from stock torch ops on the same inputs; copy = a 512 MiB device-to-device copy, copy_rate = 2 x 512 MiB / its "
                   "median; must_move = the bytes any scheme moves, fraction_of_copy_rate = (must_move / copy_rate) / time; "
                   "normals_gathers_out_of_l2 = the id, triangle and vertex gathers of the CSR walk" % (args.calls, args.rounds),
           "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
