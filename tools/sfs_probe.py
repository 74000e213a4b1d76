#!/usr/bin/env python3
"""What the shape-from-shading term costs, in ONE process (modelled on tools/normal_grad_probe.py): alternating rounds, device
events, medians, 64 and 32 faces at 200 x 200 on maps from a real render of the synthetic full-size assets.

  'torch_fwd'        = nets/losses.py::spherical_harmonics_intensity, the stock-torch route (four permutes, a batched matmul,
                       torch.linalg.pinv(hermitian=True) on 40,000 3x3 matrices, two matmuls, a permute back), under no_grad
  'fused_fwd'        = fr_sfs_intensity_forward through the raw C ABI
  'torch_fwd_bwd'    = the torch route with both normal maps requiring grad + backward of a given dL / d intensity
  'fused_fwd_bwd'    = rendering_layer/ops.py::sfs_intensity the same way (autograd node, state tensor allocated per call)
  'fused_bwd'        = fr_sfs_intensity_backward alone, both outputs, raw C ABI

Beside the fused calls: the bytes each direction must move -- forward 40 B per (face, pixel) (two normal maps, two albedos,
im_gray read; intensity written) + 80 B of state per pixel; backward 28 B read + 24 B written per (face, pixel) + 72 B of state read
per pixel -- and the time they take at the measured copy rate of 6.29 TB/s.  The fused forward is also compared with the torch
route on the well-conditioned pixels (recorded, not asserted; the tests hold the kernel to its float64 model).

--alt-lib NAME=PATH (repeatable): a shared library built from csrc/fr_sfs.hip ALONE with another -DFR_SFS_SLICES_MAX (hipcc
--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -DFR_SFS_SLICES_MAX=8 -o PATH fr_sfs.hip): its forward and
backward are timed in the same rounds -- how the batch-slice count of the launch geometry was chosen.
--trace: a few calls of each route and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own.
--out FILE: where the JSON goes besides stdout (default profiles/sfs_intensity.json).

--sharded: instead of the above, the SPLIT route (fr_sfs_moments + fr_sfs_solve_shade, fr_sfs_backward_q + fr_sfs_backward_apply:
one rank's share of a whole-batch solve across ranks) beside the one-call kernels, raw C ABI, same rounds, same process:
  'one_fwd' / 'one_bwd'              = fr_sfs_intensity_forward / fr_sfs_intensity_backward (both normal outputs)
  'split_fwd_p1' / 'split_bwd_p1'    = the two split calls of a direction with ONE part (this rank alone)
  'split_fwd_p8' / 'split_bwd_p8'    = the same with eight parts: this rank's planes written into slot 0 of the stacked buffer, the
                                       other seven slots synthetic remote parts (the sums of the same maps); no collective runs
with the bytes each leg must move: the one-call figure + (1 + nparts) x 72 B per pixel forward (the part written, the stack read),
+ (1 + nparts) x 24 B backward, and what a rank would RECEIVE in the exchange (not timed here: no second GPU).  A library given
with --alt-lib (the parent commit's fr_sfs.hip, say) has its one-call kernels timed in the same rounds, and whether its bits equal
this build's is recorded.  Default --out profiles/sfs_sharded.json."""
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
ap.add_argument("--calls", type=int, default=40, help="fused calls per timed figure")
ap.add_argument("--torch-calls", type=int, default=5, help="torch-route calls per timed figure")
ap.add_argument("--faces", type=int, nargs="+", default=[64, 32])
ap.add_argument("--rcond", type=float, default=1e-6)
ap.add_argument("--alt-lib", action="append", default=[], metavar="NAME=PATH")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--sharded", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "sfs_sharded.json" if args.sharded else "sfs_intensity.json")

if not torch.cuda.is_available():
    raise SystemExit("sfs_probe: needs an MI355X (a measurement path does not fall back)")

h = importlib.import_module("3dfacerecon_amd._lib")
synth = importlib.import_module("3dfacerecon_amd.utils.synth")
netm = importlib.import_module("3dfacerecon_amd.nets.network")
ops = importlib.import_module("3dfacerecon_amd.rendering_layer.ops")
losses = importlib.import_module("3dfacerecon_amd.nets.losses")
L = h.lib()
A = synth.make_assets()
dev = torch.device("cuda:0")
H = W = 200


def bind_alt(path):
    """only the SfS entry points of a library built from fr_sfs.hip alone"""
    return h.bind(ctypes.CDLL(path), ("fr_sfs_intensity_forward", "fr_sfs_intensity_backward", "fr_debug_sfs_geom"))


ALT = {}
for spec in args.alt_lib:
    name, path = spec.split("=", 1)
    ALT[name] = bind_alt(path)


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


def geom_of(lib, B):
    g = (ctypes.c_int * 4)()
    lib.fr_debug_sfs_geom(B, H, W, g)
    return dict(zip(("pixels_per_workgroup", "batch_slices", "workgroups", "lds_bytes"), g))


out = {}
for B in args.faces:
    net = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=200, device=dev)
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=200, beta=0.7), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = dict(dtype=torch.float32, device=dev)
    with torch.no_grad():
        V = net.vertices_transform(P)
        alb, nmap = net.compute_abedo_image(V, net.tri, net.mu_tex)
        tex_new = net.mu_tex + (net.pc_tex @ net.param_tex).reshape(3, -1)
        alb2, nmap2 = net.compute_abedo_image(V, net.tri, tex_new)
    alb, nmap, alb2, nmap2 = (t.contiguous() for t in (alb, nmap, alb2, nmap2))
    im = torch.rand((B, H, W, 1), generator=torch.Generator().manual_seed(1)).to(dev)
    g = torch.randn((B, H, W, 1), generator=torch.Generator().manual_seed(2)).to(dev)
    nst = L.fr_sfs_state_bytes(H, W)
    state = torch.empty((nst // 8,), dtype=torch.float64, device=dev)
    inten = torch.empty((B, H, W, 1), **o)
    gn, gn2 = torch.empty((B, H, W, 3), **o), torch.empty((B, H, W, 3), **o)
    n_req, n2_req = nmap.clone().requires_grad_(True), nmap2.clone().requires_grad_(True)

    def c_fwd(lib):
        return lambda: lib.fr_sfs_intensity_forward(h.ptr(alb), h.ptr(nmap), h.ptr(im), h.ptr(alb2), h.ptr(nmap2), B, H, W, args.rcond,
                                                    h.ptr(inten), h.ptr(state), nst, st)

    def c_bwd(lib):
        return lambda: lib.fr_sfs_intensity_backward(h.ptr(g), h.ptr(alb), h.ptr(im), h.ptr(alb2), h.ptr(nmap2), h.ptr(state), nst,
                                                     B, H, W, h.ptr(gn), h.ptr(gn2), st)

    if args.sharded:
        NP = 8
        npix = H * W
        nm, nq = L.fr_sfs_moments_bytes(H, W), L.fr_sfs_q_bytes(H, W)
        mstack = torch.empty((NP, 9, H, W), dtype=torch.float64, device=dev)   # slot 0: this rank; 1-7: synthetic remote parts
        qstack = torch.empty((NP, 3, H, W), dtype=torch.float64, device=dev)
        state2, inten2 = torch.empty_like(state), torch.empty_like(inten)
        gn_s, gn2_s = torch.empty_like(gn), torch.empty_like(gn2)

        def split_fwd(nparts):
            def run():
                rc = L.fr_sfs_moments(h.ptr(alb), h.ptr(nmap), h.ptr(im), B, H, W, h.ptr(mstack), nm, st)
                return rc or L.fr_sfs_solve_shade(h.ptr(mstack), nparts, h.ptr(alb2), h.ptr(nmap2), B, H, W, args.rcond,
                                                  h.ptr(inten2), h.ptr(state2), nst, st)
            return run

        def split_bwd(nparts):
            def run():
                rc = L.fr_sfs_backward_q(h.ptr(g), h.ptr(alb2), h.ptr(nmap2), B, H, W, h.ptr(qstack), nq, st)
                return rc or L.fr_sfs_backward_apply(h.ptr(g), h.ptr(alb), h.ptr(im), h.ptr(alb2), h.ptr(nmap2), h.ptr(state), nst,
                                                     h.ptr(qstack), nparts, B, H, W, h.ptr(gn_s), h.ptr(gn2_s), None, st)
            return run
        assert c_fwd(L)() == 0 and c_bwd(L)() == 0 and split_fwd(1)() == 0 and split_bwd(1)() == 0
        torch.cuda.synchronize()

        def same(a, b):
            return bool((a.reshape(-1).view(torch.int32) == b.reshape(-1).view(torch.int32)).all())
        bits = {"split_p1_equals_one_call": same(inten2, inten) and same(state2, state) and same(gn_s, gn) and same(gn2_s, gn2)}
        for name, lib in ALT.items():   # the other library's one-call kernels on the same inputs: the same bits?
            keep = [t.clone() for t in (inten, state, gn, gn2)]
            assert c_fwd(lib)() == 0 and c_bwd(lib)() == 0
            torch.cuda.synchronize()
            bits["one_call_equals_" + name] = all(same(a, b) for a, b in zip(keep, (inten, state, gn, gn2)))
        mstack[1:] = mstack[0]
        qstack[1:] = qstack[0]
        routes = {"one_fwd": c_fwd(L), "split_fwd_p1": split_fwd(1), "split_fwd_p8": split_fwd(NP),
                  "one_bwd": c_bwd(L), "split_bwd_p1": split_bwd(1), "split_bwd_p8": split_bwd(NP)}
        for name, lib in ALT.items():
            routes["%s_one_fwd" % name] = c_fwd(lib)
            routes["%s_one_bwd" % name] = c_bwd(lib)
        for fn in routes.values():
            for _ in range(3):
                assert fn() == 0
        torch.cuda.synchronize()
        if args.trace:
            continue
        res = {k: [] for k in routes}
        for rnd in range(args.rounds):
            for k, fn in routes.items():
                res[k].append(timed(fn, args.calls))
        assert c_fwd(L)() == 0   # (the state the backward legs read: left as the one-call forward writes it)
        rec = {k: summary(v) for k, v in res.items()}
        must_f = B * npix * 40 + npix * 80
        must_b = B * npix * 52 + npix * 72
        rec["bytes"] = {"one_fwd": must_f, "one_bwd": must_b}
        for n in (1, NP):
            rec["bytes"]["split_fwd_p%d" % n] = must_f + (1 + n) * npix * 72
            rec["bytes"]["split_bwd_p%d" % n] = must_b + (1 + n) * npix * 24
            rec["bytes"]["exchange_received_fwd_p%d" % n] = (n - 1) * npix * 72
            rec["bytes"]["exchange_received_bwd_p%d" % n] = (n - 1) * npix * 24
        rec["bytes"]["map_gather_received_p%d" % NP] = (NP - 1) * B * npix * 16   # the gather=True torch route: 4 floats per (face, pixel)
        rec["time_at_copy_rate_us"] = {k: round(v / COPY_RATE * 1e6, 2) for k, v in rec["bytes"].items() if not k.startswith(("exch", "map"))}
        for k in ("fwd", "bwd"):
            for n in (1, NP):
                rec["split_%s_p%d_minus_one_call_us" % (k, n)] = round(rec["split_%s_p%d" % (k, n)]["median"] - rec["one_" + k]["median"], 2)
        g6 = (ctypes.c_int * 6)()
        L.fr_debug_sfs_split_geom(B, H, W, g6)
        rec["geometry"] = dict(zip(("pixels_per_workgroup", "batch_slices", "workgroups", "lds_moments", "lds_solve_shade", "lds_q"), g6))
        rec["bits"] = bits
        out["B=%d" % B] = rec
        print("B=%d" % B, json.dumps(rec), flush=True)
        continue

    def torch_fwd():
        with torch.no_grad():
            return losses.spherical_harmonics_intensity(alb, nmap, im, alb2, nmap2, rcond=args.rcond)

    def torch_fwd_bwd():
        n_req.grad = n2_req.grad = None
        losses.spherical_harmonics_intensity(alb, n_req, im, alb2, n2_req, rcond=args.rcond).backward(g)

    def fused_fwd_bwd():
        n_req.grad = n2_req.grad = None
        ops.sfs_intensity(alb, n_req, im, alb2, n2_req, rcond=args.rcond).backward(g)
    routes = {"torch_fwd": (torch_fwd, args.torch_calls), "fused_fwd": (c_fwd(L), args.calls),
              "torch_fwd_bwd": (torch_fwd_bwd, args.torch_calls), "fused_fwd_bwd": (fused_fwd_bwd, args.calls),
              "fused_bwd": (c_bwd(L), args.calls)}
    for name, lib in ALT.items():
        routes["%s_fwd" % name] = (c_fwd(lib), args.calls)
        routes["%s_bwd" % name] = (c_bwd(lib), args.calls)
    for fn, _ in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if args.trace:
        for fn, _ in routes.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        continue
    # the fused forward beside the torch route, on the pixels where the solve is a property of the formula
    assert c_fwd(L)() == 0
    I_t = torch_fwd()
    rank = state.view(10, H, W)[9]
    Y = nmap.permute(1, 2, 3, 0).double()
    sv = torch.linalg.svdvals(Y @ Y.transpose(-1, -2))
    good = sv[..., 2] > 1e-3 * sv[..., 0]
    diff = float((inten - I_t)[:, good].abs().max()) if bool(good.any()) else None
    res = {k: [] for k in routes}
    for rnd in range(args.rounds):
        for k, (fn, calls) in routes.items():
            res[k].append(timed(fn, calls))
    rec = {k: summary(v) for k, v in res.items()}
    npix = H * W
    must_f = B * npix * 40 + npix * 80
    must_b = B * npix * 52 + npix * 72
    rec["bytes"] = {"forward_must_move": must_f, "backward_must_move": must_b,
                    "forward_time_at_copy_rate_us": round(must_f / COPY_RATE * 1e6, 2),
                    "backward_time_at_copy_rate_us": round(must_b / COPY_RATE * 1e6, 2)}
    rec["fused_fwd_fraction_of_copy_rate"] = round(must_f / COPY_RATE * 1e6 / rec["fused_fwd"]["median"], 3)
    rec["fused_bwd_fraction_of_copy_rate"] = round(must_b / COPY_RATE * 1e6 / rec["fused_bwd"]["median"], 3)
    rec["torch_over_fused_fwd"] = round(rec["torch_fwd"]["median"] / rec["fused_fwd"]["median"], 2)
    rec["torch_over_fused_fwd_bwd"] = round(rec["torch_fwd_bwd"]["median"] / rec["fused_fwd_bwd"]["median"], 2)
    rec["geometry"] = geom_of(L, B)
    for name, lib in ALT.items():
        rec["geometry_" + name] = geom_of(lib, B)
    rec["pixels_by_rank"] = [int((rank == k).sum()) for k in range(4)]
    rec["well_conditioned_pixels"] = int(good.sum())
    rec["fused_vs_torch_max_abs_on_them"] = diff
    out["B=%d" % B] = rec
    print("B=%d" % B, json.dumps(rec), flush=True)

if args.sharded and not args.trace:
    doc = {"what": "us per leg, device events around %d repetitions per figure, %d alternating rounds, one process, raw C ABI; maps from "
                   "render_depth of the full-size synthetic mesh at 200 x 200, rcond %g; one_* = the one-call kernels, split_*_pN = the "
                   "two split calls of that direction with N parts (N = 8: this rank's part + seven synthetic remote parts already in "
                   "the stacked buffer; no collective is timed); bytes = what each leg must move, exchange_received_* = what a rank "
                   "would receive in the all-gather, map_gather_received = the same for the gather=True torch route; "
                   "<name>_one_* = the one-call kernels of the library given as --alt-lib <name>=..." % (args.calls, args.rounds, args.rcond),
           "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
           "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
elif not args.trace:
    doc = {"what": "us per call, device events around %d fused / %d torch calls per figure, %d alternating rounds, one process; maps "
                   "from render_depth of the full-size synthetic mesh at 200 x 200, rcond %g; torch_* = the stock-torch "
                   "spherical_harmonics_intensity, fused_fwd / fused_bwd = fr_sfs_intensity_forward / _backward through the raw C ABI, "
                   "fused_fwd_bwd = the autograd operator sfs_intensity + backward (it allocates its state and outputs per call); "
                   "*_must_move = the bytes any scheme moves, fraction_of_copy_rate = (must_move / 6.29 TB/s) / time; any other "
                   "<name>_fwd / <name>_bwd = the same calls from a library built with another batch-slice cap (geometry_<name>)"
                   % (args.calls, args.torch_calls, args.rounds, args.rcond),
           "copy_rate_bytes_per_s": COPY_RATE, "device": torch.cuda.get_device_name(0), "lib": L.fr_version().decode(),
           "results": out}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
