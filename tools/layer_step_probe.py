#!/usr/bin/env python3
"""The decode -> rendering-layer step, one call against the composed chain, in ONE process through the raw C ABI
(modelled on tools/bwd_ab_probe.py): alternating rounds, device events.

  backward  'composed'    = the torch pixel-gradient expression of _RenderingLayerFused.backward -> fr_render_depth_backward_ws
                            -> fr_decode_3dmm_backward_packed (d f from the forward's output: the default autograd route)
            'composed_mu' = the same with fr_decode_3dmm_backward_packed_mu (the chain the fused call is bit-identical to)
            'fused'       = fr_decode_render_backward
  forward   'two_calls'   = fr_decode_3dmm -> fr_rendering_layer_forward_phases(3)      (triangle list packed once)
            'one_call'    = fr_decode_rendering_layer_forward(11)
  autograd  host time of loss.backward() through FaceRecNet.decode_rendering_layer (one node) against
            vertices_transform -> rendering_layer_fused (two nodes): wall clock of the call (enqueue) and of call + synchronize.

--trace: a few calls of each route and nothing else, for a `rocprofv3 --kernel-trace --stats -- python tools/layer_step_probe.py
--trace` run of its own (per-kernel times).  --out FILE: where the JSON goes besides stdout."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--calls", type=int, default=40, help="calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32, 16])
ap.add_argument("--trace", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
H = W = 200
NS, NE = 199, 29


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
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    N, ntri = net.nvert, int(net.tri.shape[1])
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    im = torch.rand((B, H, W, 1), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    net_in, depth_img = torch.empty((B, H, W, 7), **o), torch.empty((B, H, W, 1), **o)
    depth, tri_ind = torch.empty((B, H, W, 1), **o), torch.empty((B, H, W, 1), **o)
    V = torch.empty((B, 3, N), **o)
    nws = L.fr_render_depth_workspace_bytes(B, N, ntri, H, W)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    nh = L.fr_decode_render_vertex_bytes(B, N)
    hand = torch.empty((nh,), dtype=torch.uint8, device=dev)
    outs = [h.ptr(t) for t in (net_in, depth_img, depth, tri_ind)]

    def one_call(ph=11):
        return L.fr_decode_rendering_layer_forward(h.ptr(P), h.ptr(net._basis.image), None, h.ptr(net.tri), h.ptr(net.vertex_code),
                                                   h.ptr(im), B, N, NS, NE, ntri, H, W, 1, 200.0, h.ptr(hand), nh, *outs, h.ptr(ws),
                                                   nws, st, ph)

    def two_calls(ph=3):
        rc = L.fr_decode_3dmm(h.ptr(P), h.ptr(net._basis.image), None, B, N, NS, NE, 200.0, h.ptr(V), st)
        return rc or L.fr_rendering_layer_forward_phases(h.ptr(V), h.ptr(net.tri), h.ptr(net.vertex_code), h.ptr(im), B, N, ntri, H,
                                                         W, 1, *outs, h.ptr(ws), nws, st, ph)
    assert two_calls(7) == 0 and one_call(15) == 0
    torch.cuda.synchronize()

    gd, gi, gn = torch.randn((B, H, W, 1), **o), torch.randn((B, H, W, 1), **o), torch.randn((B, H, W, 7), **o)
    img_t = net._basis.image_t()
    nrw = L.fr_render_depth_backward_workspace_bytes(B, H, W)
    rws = torch.empty((nrw,), dtype=torch.uint8, device=dev)
    ndw = L.fr_decode_backward_workspace_bytes(B, N, NS, NE)
    dws = torch.empty((ndw,), dtype=torch.uint8, device=dev)
    nfw = L.fr_decode_render_backward_workspace_bytes(B, N, NS, NE, H, W)
    fws = torch.empty((nfw,), dtype=torch.uint8, device=dev)
    vg = torch.empty((B, 3, N), **o)
    gp = torch.empty_like(P)

    def composed(mu=False):
        # (the pixel gradient exactly as _RenderingLayerFused.backward forms it: torch elementwise ops, fresh temporaries)
        dg = torch.zeros_like(depth)
        dg = dg + gn[..., 0:1] * im * ((depth >= 1e-6) & (depth <= 1.0)).to(depth.dtype)
        dg = dg + gi * (depth >= 1e-6).to(depth.dtype)
        dg = dg + gd
        dg = dg.contiguous()
        rc = L.fr_render_depth_backward_ws(h.ptr(dg), h.ptr(net.tri), h.ptr(tri_ind), h.ptr(vg), B, N, ntri, H, W, h.ptr(rws), nrw, st)
        if mu:
            return rc or L.fr_decode_3dmm_backward_packed_mu(h.ptr(vg), h.ptr(P), h.ptr(net.mu), h.ptr(img_t), None, B, N, NS, NE,
                                                             200.0, h.ptr(gp), h.ptr(dws), ndw, st)
        return rc or L.fr_decode_3dmm_backward_packed(h.ptr(vg), h.ptr(P), h.ptr(V), h.ptr(img_t), None, B, N, NS, NE, 200.0,
                                                      h.ptr(gp), h.ptr(dws), ndw, st)

    def fused():
        return L.fr_decode_render_backward(h.ptr(gd), h.ptr(gi), h.ptr(gn), h.ptr(im), h.ptr(depth), h.ptr(net.tri), h.ptr(tri_ind),
                                           h.ptr(P), h.ptr(net.mu), h.ptr(img_t), None, B, N, NS, NE, ntri, H, W, 200.0, h.ptr(gp),
                                           h.ptr(fws), nfw, st)
    routes_b = {"composed": lambda: composed(False), "composed_mu": lambda: composed(True), "fused": fused}
    routes_f = {"two_calls": two_calls, "one_call": one_call}
    for fn in list(routes_b.values()) + list(routes_f.values()):
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    if args.trace:
        for fn in list(routes_b.values()) + list(routes_f.values()):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        continue

    res = {k: [] for k in list(routes_b) + list(routes_f)}
    for rnd in range(args.rounds):
        for k, fn in list(routes_b.items()) + list(routes_f.items()):
            res[k].append(timed(fn, args.calls))
    rec = {k: summary(v) for k, v in res.items()}
    for fast, base in (("fused", "composed"), ("fused", "composed_mu"), ("one_call", "two_calls")):
        rec["%s_vs_%s" % (fast, base)] = {
            "median_difference_us": round(rec[fast]["median"] - rec[base]["median"], 2),
            "margin_us": rec[base]["spread_max_minus_min"],
            "within_margin": rec[fast]["median"] <= rec[base]["median"] + rec[base]["spread_max_minus_min"]}

    # the autograd route: host time of one backward, one node against two
    gw7, gw1 = torch.rand((B, H, W, 7), **o), torch.rand((B, H, W, 1), **o)

    def graph(one_node):
        p = P.clone().requires_grad_(True)
        if one_node:
            ni, di = net.decode_rendering_layer(p, im_gray=im)
        else:
            ni, di, _, _ = ops.rendering_layer_fused(net.vertices_transform(p), net.tri, net.vertex_code, im)
        return (ni * gw7).sum() + (di * gw1).sum()
    host = {}
    for name, one_node in (("two_nodes", False), ("one_node", True)):
        enq, tot = [], []
        for i in range(3 + 20):
            loss = graph(one_node)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss.backward()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= 3:
                enq.append((t1 - t0) * 1e6)
                tot.append((t2 - t0) * 1e6)
        host[name] = {"backward_call_us_median": round(statistics.median(enq), 1),
                      "backward_call_plus_sync_us_median": round(statistics.median(tot), 1)}
    rec["autograd_backward_host"] = host
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

if not args.trace:
    doc = {"what": "us per call, device events around %d calls per figure, %d alternating rounds, one process, raw C ABI; "
                   "autograd_backward_host: wall clock of loss.backward() (the loss includes two torch reductions in both routes)"
                   % (args.calls, args.rounds),
           "acceptance": "median(fused) <= median(composed) + (max - min of composed over the rounds)",
           "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(), "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
