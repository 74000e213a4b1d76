#!/usr/bin/env python3
"""What the geometry loss costs on its two routes, in ONE process (modelled on tools/depth_normals_probe.py): alternating rounds,
device events, medians, 32 and 64 faces of the full synthetic mesh (N = 53,215, K = 228).

  'product_fwd_bwd'   = the default route: FaceRecNet.geometry_product -> (g * g).mean() -> backward (the MFMA decode over the second
                        packed image, a [B,3,N] tensor, fr_decode_3dmm_backward_packed over the K-major image)
  'gram_fwd_bwd'      = FaceRecNet.geometry_loss(gram=True) -> backward (the autograd node; loss and gradient allocated per call);
                        both routes' backward is handed dL / d loss = 1 as a device scalar, as the objective hands it down
  'gram_kernels'      = fr_geometry_loss_forward + fr_geometry_loss_backward through the raw C ABI: the three launches alone
  'gram_build'        = fr_geometry_gram_build through the raw C ABI (load time; once per model)
  'peak_bytes'        = torch.cuda.max_memory_allocated over one get_loss + backward of the whole objective on each route, above
                        what was allocated before the call, on a net of its own per route

Beside them the byte arithmetic: at 64 faces the product route must move the 153 MB packed image, the 40.9 MB product four times
(written by the decode, read for the mean; 2 g / n written, read by the packed backward) and the 153 MB K-major image: 470 MB, 75 us
at the measured copy rate of 6.29 TB/s.  The build must read the 146 MB basis once: 23 us.  The gate: 'gram_fwd_bwd' at 64 faces
below that 75 us.

--out FILE: where the JSON goes besides stdout (default profiles/geometry_gram.json)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s: the measured device-to-device copy figure of the part

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--build-calls", type=int, default=5)
ap.add_argument("--faces", type=int, nargs="+", default=[32, 64])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_gram.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("geometry_gram_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
losses = importlib.import_module("3dfacerecon_amd.nets.losses")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
S = 200


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


def peak_of_get_loss(B, **kw):
    """bytes get_loss + backward add to what is allocated, on a fresh net (its lazy images are built inside the call, as in a first
    training step) and again on the second call (the steady state)"""
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=dev)
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=S, beta=0.7), device=dev)
    lab = torch.as_tensor(synth.sample_params_batch(B, im_size=S, beta=0.7, seed=9), device=dev)
    im = torch.rand((B, S, S, 1), generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        V = net.vertices_transform(P)
        coarse = net.coarse_net_input(V, im_gray=im)[1]
    fine = coarse.clone()
    out = []
    for _ in range(2):
        pred = P.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        losses.get_loss(net, pred, lab, im, V, coarse, fine, **kw)["total_loss"].backward()
        torch.cuda.synchronize()
        out.append(int(torch.cuda.max_memory_allocated(dev) - before))
    held = int((net._basis_nomu.image.numel() if net._basis_nomu is not None else 0)
               + (net._gram.numel() * 8 if net._gram is not None else 0))
    return {"first_call": out[0], "steady": out[1], "held_by_the_route_afterwards": held}


N, ns, ne = A["mu"].size // 3, A["pc_shape"].shape[1], A["pc_exp"].shape[1]
K = ns + ne
net = netm.FaceRecNet(mesh_data=A, batch_size=1, im_size=S, device=dev)
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
G = net.gram()
nb, nws = L.fr_geometry_gram_bytes(ns, ne), L.fr_geometry_gram_workspace_bytes(N, ns, ne)
G2 = torch.empty_like(G)
ws = torch.empty((nws,), dtype=torch.uint8, device=dev)


def build():
    assert L.fr_geometry_gram_build(h.ptr(net.pc_shape), h.ptr(net.pc_exp), N, ns, ne, h.ptr(G2), nb, h.ptr(ws), nws, st) == 0


build()
torch.cuda.synchronize()
assert bool((G2.view(torch.int64) == G.view(torch.int64)).all())

out = {}
for B in args.faces:
    rs = np.random.RandomState(B)
    d = torch.as_tensor(np.concatenate([rs.uniform(-1e4, 1e4, (B, ns)), rs.uniform(-3, 3, (B, ne))], 1).astype(np.float32), device=dev)
    x = d.clone().requires_grad_(True)
    nst = L.fr_geometry_loss_state_bytes(B, ns, ne)
    state = torch.empty((nst,), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    one = torch.ones((), dtype=torch.float32, device=dev)
    gd = torch.empty((B, K), dtype=torch.float32, device=dev)

    def product_fwd_bwd():
        x.grad = None
        g = net.geometry_product(x)
        (g * g).mean().backward(one)

    def gram_fwd_bwd():
        x.grad = None
        net.geometry_loss(x, gram=True).backward(one)

    def gram_kernels():
        L.fr_geometry_loss_forward(h.ptr(d), h.ptr(G), B, N, ns, ne, h.ptr(loss), h.ptr(state), nst, st)
        L.fr_geometry_loss_backward(h.ptr(one), h.ptr(state), nst, B, N, ns, ne, h.ptr(gd), st)

    routes = {"product_fwd_bwd": (product_fwd_bwd, args.calls), "gram_fwd_bwd": (gram_fwd_bwd, args.calls),
              "gram_kernels": (gram_kernels, args.calls), "gram_build": (build, args.build_calls)}
    for fn, _ in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the two routes beside each other on this input (recorded, not asserted; the tests hold both)
    product_fwd_bwd()
    lp, gp = float((net.geometry_product(x.detach()) ** 2).mean()), x.grad.clone()
    gram_fwd_bwd()
    lg, gg = float(net.geometry_loss(x.detach(), gram=True)), x.grad.clone()
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, (fn, calls) in routes.items():
            res[k].append(timed(fn, calls))
    rec = {k: summary(v) for k, v in res.items()}
    rec["product_over_gram_fwd_bwd"] = round(rec["product_fwd_bwd"]["median"] / rec["gram_fwd_bwd"]["median"], 2)
    prod_bytes = B * 3 * N * 4
    image = int(net._basis_nomu.image.numel())
    must = 2 * image + 4 * prod_bytes
    rec["bytes"] = {"packed_image": image, "product_tensor": prod_bytes, "product_route_must_move": must,
                    "product_route_time_at_copy_rate_us": round(must / COPY_RATE * 1e6, 2),
                    "gram_route_moves_at_most": int(B * G.numel() * 8 + 3 * nst + 2 * B * K * 4)}
    rec["loss"] = {"product": lp, "gram": lg, "relative_difference": abs(lp - lg) / abs(lg),
                   "largest_gradient_difference_over_largest_gradient": float((gp - gg).abs().max() / gg.abs().max())}
    rec["peak_bytes"] = {"product": peak_of_get_loss(B), "gram": peak_of_get_loss(B, geometry_gram=True)}
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

geo = (ctypes.c_int * 6)()
L.fr_debug_geometry_gram_geom(N, ns, ne, geo)
basis_bytes = 3 * N * K * 4
gate = out.get("B=64", {}).get("gram_fwd_bwd", {}).get("median")
doc = {"what": "us per call, device events around %d calls per figure (%d for the build), %d alternating rounds, one process, the full "
               "synthetic mesh; product_fwd_bwd = geometry_product -> (g * g).mean() -> backward, gram_fwd_bwd = "
               "geometry_loss(gram=True) -> backward (autograd node), gram_kernels = fr_geometry_loss_forward + _backward through the "
               "raw C ABI, gram_build = fr_geometry_gram_build (load time); peak_bytes = max_memory_allocated of one get_loss + "
               "backward above what was allocated before it" % (args.calls, args.build_calls, args.rounds),
       "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
       "geometry": dict(zip(("rows_per_chunk", "chunks", "Kp", "tile_pairs", "workgroups", "lds_bytes"), geo)),
       "build": {"basis_bytes": basis_bytes, "read_floor_us": round(basis_bytes / COPY_RATE * 1e6, 2), "workspace_bytes": int(nws),
                 "gram_bytes": int(nb)},
       "gate": {"gram_fwd_bwd_at_64_faces_us": gate, "bound_us": 75.0, "holds": bool(gate is not None and gate < 75.0)},
       "results": out}
print(json.dumps(doc))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
