#!/usr/bin/env python3
"""Caller harness for BASELINE.json configs 3-5: CoarseNet (x nIter) around the decode -> render hot path, the depth
rendering layer, FineNet, forward only or the reference's training step, one process per GPU (RCCL all-reduce of the
network gradients through torch DDP).  Shaped like the reference's train loop (trainval.py:79-125: train step, then a
full forward on a validation batch every iteration) with synthetic images / labels.

    python examples/coarse_loop.py --config 3      # presets: 3 = CoarseNet + render forward, batch 32, 1 GPU;
                                                   #          4 = train loop, 256 faces over the ranks (32 per GPU at N = 8);
                                                   #          5 = Coarse + Fine joint forward at 448 x 448, 128 faces over the ranks
    python examples/coarse_loop.py --batch 32 --steps 5                       # config 3 spelled out
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29501 \
        examples/coarse_loop.py --batch 32 --steps 5 --train                  # config 4: 256 faces over 8 GPUs
    ... --im-size 448 --batch 16 --fine                                       # config 5: Coarse + Fine joint forward
    python examples/coarse_loop.py --phase test --batch 64 --steps 20         # the reference's eval loop (trainval.py:192-210):
                                                                              # independent test batches, the depth rendering of
                                                                              # batch k in flight beside the network of batch k+1

The render / decode path needs no collective (the batch is sharded); the only collectives are DDP's gradient all-reduce
and -- with --gather-sfs -- the all-gather that restores the reference's whole-batch lighting estimate of the
shape-from-shading loss (nets/losses.py).  The objective is the reference's (nets/network.py:336-378): pose MSE, geometry
MSE through the basis, SfS, fidelity, Laplacian smoothness; per training forward with nIter = 4 that is 5 decodes + 1
basis product and 7 render_depth calls, as in the reference graph.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def pkg(n):
    return importlib.import_module("3dfacerecon_amd." + n)


_emit = lambda rec: print(json.dumps(rec))   # noqa: E731  (main() points it at the real stdout)


def build_harness(args, dev, rank, world, local):
    """model (DDP-wrapped when training on > 1 rank), optimiser, step() closure."""
    synth, netm, cn, losses = pkg("utils.synth"), pkg("nets.network"), pkg("nets.coarse_net"), pkg("nets.losses")
    cn.apply_miopen_workaround()   # a process setting, applied by the entry point before the first convolution
    torch.manual_seed(1234)  # same initial weights on every rank
    A = synth.make_small_assets() if args.small else synth.make_assets()
    B, S = args.batch, args.im_size
    face = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=dev)
    if args.small:  # the tiny mesh is ~30 px wide: centre it and scale it up a little
        face.init_pred_params[..., 6] = 1e-3 * S / 200.0
    # the reference's graph always holds FineNet (build(), network.py:69-101); the forward-only config 3 is CoarseNet + render
    model = cn.FaceReconModel(face, nIter=args.nIter, fine=args.fine or args.train, fused_step=args.fused_step,
                              pose_grad=args.pose_grad, normal_grad=args.normal_grad,
                              **({"learn_tex": True} if args.sfs_tex_grad else {}),
                              **({"depth_interp": True} if args.depth_interp else {})).to(dev)
    net = model
    if args.train and world > 1:
        net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local] if dev.type == "cuda" else None)
    opt = torch.optim.Adam(model.parameters(), lr=1e-5) if args.train else None  # run_experiment.sh:13

    g = torch.Generator(device="cpu").manual_seed(100 + rank)  # every rank has its own shard of the data
    def batch(seed):
        im = torch.rand((B, S, S, 1), generator=g).to(dev)
        lab = torch.as_tensor(synth.sample_params_batch(B, im_size=S, n_shape=face.ndim_shape, n_exp=face.ndim_exp,
                                                        beta=0.7, seed=seed + rank), device=dev)
        return im, lab
    train_b, val_b = batch(200), batch(300)
    train_s = val_s = None
    if args.synth_data:
        # --synth-data: a fresh batch every step whose image depicts its label (pipeline.SynthBatches: sampled, decoded, rendered
        # and shaded on a side stream); train and validation draw from two streams with disjoint seeds, every rank its own faces
        pipe = pkg("pipeline")
        kw = dict(slots=2, first_face=pipe.synth_face_range(0, rank, world, B)[0], stride=world * B,
                  focal=1e-3 * S / 200.0 if args.small else 1e-3, **({"colour": True} if args.synth_colour else {}))
        if args.landmark_loss:   # the batches also carry the projections of 68 vertices and whether the render shows them
            lm_idx = synth.landmark_ids(A, min(68, face.nvert))
            kw["landmarks"] = lm_idx
        train_s = pipe.SynthBatches(face, B, args.synth_seed, **kw)
        val_s = pipe.SynthBatches(face, B, args.synth_seed + 1, **kw)

    def draw(stream, resident):
        if stream is None:
            return resident
        b = stream.next()
        extra = {}
        if args.photo_loss:   # the batch's own lighting and albedo, and the stream's gain and offset: the image is their shading
            extra.update(photo_light=b["light"], photo_alpha=b["alpha"], photo_gain=stream.gain, photo_offset=stream.offset,
                         lambda_photo=args.photo_lambda)
            if args.synth_colour:   # a colour batch: light is [B,3,9] and the term compares against the colour picture
                extra.update(photo_target_rgb=b["im_rgb"])
        if args.silhouette_loss:   # the batch's ground-truth mask against the soft coverage of the predicted face
            extra.update(silhouette_mask=b["mask"], lambda_silhouette=args.silhouette_lambda)
        if args.landmark_loss:   # the predicted parameters' projections of the same vertices against the batch's, where visible
            extra.update(landmark_target=b["landmarks"], landmark_idx=lm_idx, landmark_weight=b["landmark_visible"],
                         lambda_landmark=args.landmark_lambda)
        if extra:
            return b["im_gray"], b["params"], extra
        return b["im_gray"], b["params"]

    def forward_loss(im, lab, photo={}):
        out = net(im)
        return out, losses.get_loss(face, out["pred_params"], lab, im, out["vertices_proj"], out["coarse_depth_map"],
                                    out["pred_depth_map"], gather_sfs=args.gather_sfs, sfs_normal_grad=args.sfs_grad,
                                    sfs_fused=args.sfs_fused, sfs_rcond=args.sfs_rcond,
                                    **({"sfs_tex_grad": True} if args.sfs_tex_grad else {}),
                                    **({"sfs_fused_gather": True} if args.sfs_fused_gather else {}),
                                    **({"sfs_fine": True} if args.sfs_fine else {}),
                                    **({"geometry_gram": True} if args.geometry_gram else {}),
                                    **({"fine_fused": True} if args.fine_fused else {}),
                                    **({"sfs_alpha_lse": True, "sfs_alpha_ridge": args.sfs_alpha_ridge} if args.sfs_alpha_lse else {}),
                                    **photo)

    def step():
        if not args.train:
            with torch.no_grad():
                return net(*draw(train_s, train_b)[:1]), None
        model.train()
        out, L = forward_loss(*draw(train_s, train_b))
        opt.zero_grad(set_to_none=True)
        L["total_loss"].backward()
        opt.step()
        if args.val:  # trainval.py:96-99: a second full forward on a validation batch every iteration
            model.eval()
            with torch.no_grad():
                forward_loss(*draw(val_s, val_b))
        return out, L

    return model, net, opt, step


class _MeshExport:
    """--export-mesh: the first --export-count faces of the one-at-a-time pass as meshes, coarse and fine.  The fine depth map is
    FineNet's of (im_gray, coarse depth) -- network.py:311-333, untrained here like everything else -- taken back to the vertices by
    FaceRecNet.fine_mesh; rank 0 writes face_%06d_coarse.obj / face_%06d_fine.obj (upright: flip_y), every rank adds its faces'
    squared z errors against the decode of the LABEL parameters (synthetic batches only) over the vertices the lift moved."""

    def __init__(self, args, face, cn, dev, rank):
        self.dir, self.count, self.face, self.rank, self.B = args.export_mesh, max(args.export_count, 0), face, rank, args.batch
        self.fine = cn.FineNet().to(dev).eval()
        self.mesh_io = pkg("utils.mesh_io")
        self.tri = face.tri.cpu().numpy()
        self.done = 0
        self.err = torch.zeros(3, dtype=torch.float64, device=dev)   # squared z error coarse, fine; vertices counted
        self.labelled = False
        if rank == 0:
            os.makedirs(self.dir, exist_ok=True)

    def wants_more(self):
        return self.done < self.count

    def take(self, batch, params, coarse_depth):
        face = self.face
        V = face.vertices_transform(params)
        mesh = face.fine_mesh(V, self.fine(batch["im_gray"], coarse_depth), coarse_depth)
        n = min(self.B, self.count - self.done)
        if "params" in batch:
            self.labelled = True
            moved = (mesh["state"][:n] == 1).double()
            z_lab = face.vertices_transform(batch["params"])[:n, 2].double()
            ec, ef = V[:n, 2].double() - z_lab, mesh["vertices"][:n, 2].double() - z_lab
            self.err.add_(torch.stack([(ec * ec * moved).sum(), (ef * ef * moved).sum(), moved.sum()]))
        if self.rank == 0:
            Vc, Vf, Nf = V[:n].cpu().numpy(), mesh["vertices"][:n].cpu().numpy(), mesh["normals"][:n].cpu().numpy()
            Nc = pkg("rendering_layer.ops").vertex_normals(V[:n], face.tri, face.adjacency()).cpu().numpy()
            for i in range(n):
                stem = os.path.join(self.dir, "face_%06d" % (self.done + i))
                self.mesh_io.write_obj(stem + "_coarse.obj", Vc[i], self.tri, normals=Nc[i], flip_y=face.im_size)
                self.mesh_io.write_obj(stem + "_fine.obj", Vf[i], self.tri, normals=Nf[i], flip_y=face.im_size)
        self.done += n

    def record(self, dist_u, dev):
        rec = {"export_mesh": self.dir, "export_count": self.done}
        if self.labelled:
            sc, sf, cnt = (dist_u.sum_over_ranks(float(v), device=dev) for v in self.err.tolist())
            rec["vertex_rmse_coarse"] = (sc / cnt) ** 0.5 if cnt > 0 else float("nan")
            rec["vertex_rmse_fine"] = (sf / cnt) ** 0.5 if cnt > 0 else float("nan")
            rec["vertex_rmse_vertices"] = int(cnt)
        return rec


def run_test_phase(args, dev, rank, world, local, dist_u):
    """The reference's evaluation loop (trainval.py:192-210: `while True: images = next(generator); pred_depth = sess.run(...);
    write depth * 255`) over INDEPENDENT test batches.  CoarseNet of a batch is a dependent chain (network -> decode -> render ->
    network, nets/network.py:113-116) and runs as such on torch's current stream; the batch's final depth rendering
    (depth_rendering_layer, network.py:300-309: decode + render of the predicted parameters) does not feed anything of the NEXT
    batch, so it goes down `pipeline.BatchesInFlight.submit(pred_params)` -- its own stream, two batches in flight -- and its
    consumer (the reference writes depth * 255 to a jpg; here: the same product, reduced to a checksum) is ordered behind the slot
    with `make_current_stream_wait()` one iteration later, i.e. the render of batch k runs beside the network of batch k + 1."""
    synth, netm, cn, pipe = pkg("utils.synth"), pkg("nets.network"), pkg("nets.coarse_net"), pkg("pipeline")
    cn.apply_miopen_workaround()
    torch.manual_seed(1234)
    A = synth.make_small_assets() if args.small else synth.make_assets()
    B, S = args.batch, args.im_size
    face = netm.FaceRecNet(mesh_data=A, batch_size=B, im_size=S, device=dev)
    if args.small:
        face.init_pred_params[..., 6] = 1e-3 * S / 200.0
    coarse = cn.CoarseNet(face, nIter=args.nIter, fused_step=args.fused_step).to(dev).eval()
    flights = pipe.BatchesInFlight(face, B, S, S, slots=2)
    g = torch.Generator(device="cpu").manual_seed(100 + rank)
    images = [torch.rand((B, S, S, 1), generator=g).to(dev) for _ in range(4)]   # the "test generator": four resident batches
    # --synth-data: the test generator is a pipeline.SynthBatches stream instead -- rendered faces of known parameters, with the
    # ground-truth depth and mask the reference's evaluation never had (trainval.py:204: "TODO: Load ground truth ...")
    n_warm = max(args.warmup, 1)
    synth_kw = dict(slots=2, stride=world * B, focal=1e-3 * S / 200.0 if args.small else 1e-3)
    stream = None
    if args.synth_data:
        stream = pipe.SynthBatches(face, B, args.synth_seed + 2, first_face=pipe.synth_face_range(0, rank, world, B)[0], **synth_kw)
    # squared depth error over the mask, and the mask's pixels
    err = torch.zeros(2, dtype=torch.float64, device=dev) if stream is not None else None

    def draw(k, src=None):
        src = stream if src is None else src
        return src.next() if src is not None else {"im_gray": images[k % len(images)]}

    dumped = []   # --dump-batches: what every timed batch left in its slot (copied out by the CONSUMER, on the current stream)

    def consume(slot, batch, keep=False):
        """trainval.py:196: depth_images = pred_depth * 255.0, one image per face (written to disk there)."""
        slot.make_current_stream_wait()
        if err is not None:   # coarse_depth_map against the ground truth, over the ground truth's mask
            d = (slot.depth.clamp_min(1e-6) - batch["depth"]).double()
            err.add_(torch.stack([(d * d * batch["mask"]).sum(), batch["mask"].sum().double()]))
        if keep:
            dumped.append([t.clone() for t in (slot.params, slot.vertex_proj.contiguous()) + tuple(slot.outputs())])
        return (slot.depth.clamp_min(1e-6) * 255.0).sum(dim=(1, 2, 3))

    def loop(n, keep=False):
        sums, pending = [], None
        with torch.no_grad():
            for k in range(n):
                batch = draw(k)
                params = coarse(batch["im_gray"])                   # the dependent chain of THIS batch (current stream)
                slot = flights.submit(params)                       # its depth rendering: the slot's stream, nothing waits for it yet
                if pending is not None:
                    sums.append(consume(*pending, keep))            # batch k-1's planes, behind ITS slot
                pending = (slot, batch)                             # (a synthetic batch stays valid for two draws)
            sums.append(consume(*pending, keep))
        return sums

    loop(n_warm)
    torch.cuda.synchronize(dev)
    if err is not None:
        err.zero_()
    dist_u.barrier()
    t0 = time.perf_counter()
    sums = loop(args.steps, keep=bool(args.dump_batches))
    torch.cuda.synchronize(dev)
    dt = dist_u.max_over_ranks(time.perf_counter() - t0, device=dev)
    depth_rmse = None
    if stream is not None:
        se, px = (dist_u.sum_over_ranks(float(v), device=dev) for v in err.tolist())
        depth_rmse = (se / px) ** 0.5 if px > 0 else float("nan")
    if args.dump_batches and rank == 0:
        # every timed batch's predicted parameters, vertices and four planes as the consumer saw them: tests/test_programs_gpu.py
        # holds them to the CPU oracle (this program never loads it)
        import numpy as np
        names = ("params", "vertex_proj", "depth", "texture_image", "normal", "tri_ind")
        np.savez(args.dump_batches, steps=len(dumped), mu=A["mu"], pc_shape=A["pc_shape"], pc_exp=A["pc_exp"], tri=A["tri"], vertex=A["vertex"],
                 im_size=S, **({} if depth_rmse is None else {"depth_rmse": depth_rmse}),
                 **{"%s_%d" % (n, k): t.cpu().numpy() for k, rec in enumerate(dumped) for n, t in zip(names, rec)})
    # the same batches one at a time through the plain surface: the in-flight loop must reproduce them bit for bit
    export = _MeshExport(args, face, cn, dev, rank) if args.export_mesh else None
    with torch.no_grad():
        ref = []
        again = None
        if stream is not None:   # the timed loop's faces once more: a face's bits depend on (seed, global face index) alone
            again = pipe.SynthBatches(face, B, args.synth_seed + 2, first_face=pipe.synth_face_range(n_warm, rank, world, B)[0],
                                      **synth_kw)
        for k in range(min(args.steps, len(images))):
            batch = draw(k, again)
            im = batch["im_gray"]
            p = coarse(im)
            d = face.coarse_net_input(face.vertices_transform(p), im_gray=im)[1]
            ref.append((d * 255.0).sum(dim=(1, 2, 3)))
            if export is not None and export.wants_more():
                export.take(batch, p, d)
    same = all(torch.equal(a, b) for a, b in zip(sums, ref))
    dist_info = dist_u.describe(device=dev)
    if rank == 0:
        _emit(dict({"metric": "faces/sec, evaluation loop (trainval.py:192-210): CoarseNet x %d + depth rendering" % args.nIter,
                          "value": world * B * args.steps / dt, "unit": "faces/s", "higher_is_better": True, "data": "synthetic",
                          "dtype": "f32", "phase": "test", "n_gpus": world, "faces_per_gpu": B, "im_size": S, "steps": args.steps,
                          "ms_per_step": 1e3 * dt / args.steps, "batches_in_flight": len(flights.slots),
                          "route": "CoarseNet on torch's current stream; depth_rendering_layer of batch k through "
                                   "pipeline.BatchesInFlight.submit() beside the network of batch k + 1; consumer ordered with "
                                   "make_current_stream_wait()",
                          "depth_identical_to_one_batch_at_a_time": bool(same), "dist": dist_info},
                   **({} if depth_rmse is None else {"data": "synthetic, rendered on the device (pipeline.SynthBatches)",
                                                     "depth_rmse": depth_rmse, "synth_seed": args.synth_seed}),
                   **({} if export is None else export.record(dist_u, dev))))
    dist_u.finalize()
    return 0 if same else 1


# BASELINE.json configs[2..4] as presets; the global batch is cut over the ranks that are present (one process per GPU)
CONFIG_PRESETS = {
    3: dict(label="configs[2]: CoarseNet (ResNet-101) + render_depth end-to-end forward, batch 32, 1 GPU",
            global_batch=32, im_size=200, train=False, val=False, fine=False),
    4: dict(label="configs[3]: CoarseNet train loop, batch 256 sharded over the ranks, RCCL all-reduce",
            global_batch=256, im_size=200, train=True, val=True, fine=True),
    5: dict(label="configs[4]: CoarseNet + FineNet joint forward, 448x448 input, batch 128 over the ranks",
            global_batch=128, im_size=448, train=False, val=False, fine=True),
}


def ddp_bucket_bytes(model, net):
    """Gradient bytes one training step all-reduces: every parameter that requires grad, fp32, once per step (DDP's
    buckets partition exactly this set); 0 when the model is not wrapped (single rank / forward only)."""
    if net is model:
        return 0
    return int(sum(p.numel() * p.element_size() for p in model.parameters() if p.requires_grad))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=sorted(CONFIG_PRESETS), default=None,
                    help="BASELINE.json config preset (3, 4 or 5): sets batch / im-size / train / val / fine; on fewer GPUs "
                         "than the config names each rank runs global_batch / max(world, named GPUs) faces (its shard)")
    ap.add_argument("--shard-gpus", type=int, default=8, help="GPUs configs 4 and 5 are quoted on (their per-GPU shard)")
    ap.add_argument("--batch", type=int, default=32, help="faces per GPU")
    ap.add_argument("--im-size", type=int, default=200)
    ap.add_argument("--nIter", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--val", action="store_true", help="with --train: the reference's per-iteration validation forward")
    ap.add_argument("--fine", action="store_true")
    ap.add_argument("--fused-step", action="store_true",
                    help="decode -> rendering layer as one call and one autograd node per CoarseNet iteration "
                         "(FaceRecNet.decode_rendering_layer); off: the two-step route")
    ap.add_argument("--pose-grad", action="store_true",
                    help="let the render loop's gradient reach the three pose angles (fr_decode_pose_backward / "
                         "fr_decode_render_backward_pose); off: they get 0 from it, as in the reference")
    ap.add_argument("--normal-grad", action="store_true",
                    help="let the normal channels of every CoarseNet input carry their gradient to x, y and z of the vertices "
                         "(fr_render_normal_backward); off: they are constants to autograd, as in the reference")
    ap.add_argument("--depth-interp", action="store_true",
                    help="the coarse depth map (FineNet's input, the fidelity target) is the winners' interpolated depth, with a "
                         "gradient to x, y and z of the vertices (fr_depth_interp_forward / _backward); off: the reference's flat "
                         "per-triangle depth")
    ap.add_argument("--gather-sfs", action="store_true", help="whole-batch SfS lighting estimate across ranks")
    ap.add_argument("--sfs-grad", action="store_true",
                    help="let the shape-from-shading term reach the geometry: its two renders carry the normal map's gradient to "
                         "the vertices (get_loss(sfs_normal_grad=True)); off: the term is a reported scalar with no gradient, as in "
                         "the reference")
    ap.add_argument("--sfs-fused", action="store_true",
                    help="the SfS lighting solve and shading as one kernel pass per direction (fr_sfs_intensity_forward / "
                         "_backward) instead of the stock-torch permutes, matmuls and batched pinv")
    ap.add_argument("--sfs-fused-gather", action="store_true",
                    help="with --gather-sfs and --sfs-fused: the whole-batch lighting estimate on the fused kernels under several "
                         "ranks -- the ranks all-gather nine float64 planes of per-pixel sums forward and three backward instead of "
                         "their maps, and the DDP-averaged gradient equals the single-process one (get_loss(sfs_fused_gather=True)); "
                         "off: --gather-sfs under several ranks stays on the stock-torch route")
    ap.add_argument("--sfs-tex-grad", action="store_true",
                    help="let the shape-from-shading term fit the albedo coefficients: param_tex becomes a parameter of the model "
                         "(FaceReconModel(learn_tex=True)) and the render of the new texture carries the albedo image's gradient to it "
                         "(get_loss(sfs_tex_grad=True), fr_render_texture_backward); off: param_tex is a constant, as in the reference")
    ap.add_argument("--sfs-fine", action="store_true",
                    help="the SfS term shades the normals of the predicted FINE depth map (depth_normals: fr_depth_normals_forward / "
                         "_backward, masked by the render's tri_ind) instead of the coarse mesh's a second time, so the term's gradient "
                         "reaches pred_depth_map (get_loss(sfs_fine=True)); needs --fine; off: as the reference")
    ap.add_argument("--geometry-gram", action="store_true",
                    help="the geometry loss from the Gram matrix of the basis, built once in float64 (fr_geometry_gram_build; "
                         "get_loss(geometry_gram=True)): no pass over the basis per step and no second packed image of it; off: the "
                         "basis product on the decode kernel and its packed backward")
    ap.add_argument("--fine-fused", action="store_true",
                    help="the fidelity and the smoothness term of the fine depth map from one kernel pass per direction "
                         "(fine_depth_losses: fr_fine_losses_forward / _backward; get_loss(fine_fused=True)): float64 sums in a fixed "
                         "association, no convolution; needs --fine; off: mse_loss and a conv2d / abs / sum chain")
    ap.add_argument("--sfs-alpha-lse", action="store_true",
                    help="fit the SfS term's albedo coefficients PER FACE by least squares given the lighting (fr_albedo_lse_forward; "
                         "get_loss(sfs_alpha_lse=True)) instead of the one shared param_tex -- the estimate the reference gave up; "
                         "needs --sfs-fused, excludes --sfs-tex-grad, --gather-sfs and --sfs-fused-gather; off: as the reference")
    ap.add_argument("--sfs-alpha-ridge", type=float, default=1e-6,
                    help="ridge of the per-face albedo fit, relative to the mean diagonal of a face's Gram matrix")
    ap.add_argument("--sfs-rcond", type=float, default=1e-15,
                    help="eigenvalue cutoff of the SfS pseudo-inverse, relative to the largest.  With float64 sums a rank-deficient "
                         "pixel (fewer than three faces cover it, or their normals are parallel) has null eigenvalues near 1e-16 "
                         "of the largest, so the reference's 1e-15 cuts them unpredictably -- as it does in the reference itself.  "
                         "A cutoff such as 1e-6 makes the term well defined everywhere and is the sensible choice once the term "
                         "carries a gradient (--sfs-grad)")
    ap.add_argument("--synth-data", action="store_true",
                    help="train, validate and test on batches made on the device (pipeline.SynthBatches): random parameters, the face "
                         "they decode to rendered with a random per-face albedo and lighting, a fresh batch every step -- the image "
                         "depicts its label.  With --phase test the loop also reports depth_rmse, the RMSE of the coarse depth map "
                         "against the ground-truth depth over its mask; off: random images beside unrelated random labels")
    ap.add_argument("--synth-seed", type=int, default=3456, help="with --synth-data: the seed of the training stream (validation "
                                                                 "takes seed + 1, the test phase seed + 2)")
    ap.add_argument("--photo-loss", action="store_true",
                    help="with --synth-data and --train: add the photometric term (get_loss(photo_light=, photo_alpha=); "
                         "fr_photo_loss_forward / _backward) -- the predicted geometry rendered with the batch's ground-truth albedo "
                         "and lighting against the batch's image; its gradient reaches the vertices (the pose angles too with "
                         "--pose-grad); the record gains photometric_loss; off: no term compares a rendered face with the picture")
    ap.add_argument("--photo-lambda", type=float, default=1.0, help="with --photo-loss: the term's weight in total_loss")
    ap.add_argument("--synth-colour", action="store_true",
                    help="with --synth-data and --train: the synthetic faces are shaded in colour (SynthBatches(colour=True): RGB albedo "
                         "under a second-order lighting per channel; the net takes the gray of that image); with --photo-loss the "
                         "term compares in colour (get_loss(photo_target_rgb=); fr_photo_loss_rgb_forward / _backward)")
    ap.add_argument("--silhouette-loss", action="store_true",
                    help="with --synth-data and --train: add the silhouette term (get_loss(silhouette_mask=); fr_coverage_forward / "
                         "_backward) -- the soft coverage of the predicted face against the batch's ground-truth mask; its gradient "
                         "reaches x and y of the vertices (the pose angles too with --pose-grad); the record's losses gain "
                         "silhouette_loss; off: no term tells the fit where the face is in the picture")
    ap.add_argument("--silhouette-lambda", type=float, default=1.0, help="with --silhouette-loss: the term's weight in total_loss")
    ap.add_argument("--landmark-loss", action="store_true",
                    help="with --synth-data and --train: add the landmark term (get_loss(landmark_target=); fr_landmark_forward / "
                         "_backward) -- the projections of 68 vertices (utils/synth.landmark_ids) under the predicted parameters "
                         "against the batch's own, weighted by their visibility; decoded from a compact image of those vertices' "
                         "basis rows, its gradient reaches the predicted parameters directly, the angles included; the record's "
                         "losses gain landmark_loss")
    ap.add_argument("--landmark-lambda", type=float, default=1.0, help="with --landmark-loss: the term's weight in total_loss")
    ap.add_argument("--small", action="store_true", help="tiny synthetic assets (smoke runs)")
    ap.add_argument("--dump-batches", default=None, metavar="FILE.npz",
                    help="--phase test: save every timed batch's parameters, vertices and planes (as its consumer saw them) for an "
                         "external checker")
    ap.add_argument("--export-mesh", default=None, metavar="DIR",
                    help="--phase test: write the first --export-count faces as DIR/face_%%06d_coarse.obj (the coarse decode) and "
                         "DIR/face_%%06d_fine.obj (FaceRecNet.fine_mesh: FineNet's depth map lifted onto the visible vertices; "
                         "fr_mesh_visible / fr_mesh_lift / fr_mesh_vertex_normals), upright, with vertex normals.  With --synth-data "
                         "the record gains vertex_rmse_coarse and vertex_rmse_fine: the RMS z error against the decode of the label "
                         "parameters over the vertices the lift moved.  The image size must be a multiple of 4 (FineNet); off: no mesh "
                         "is built and the record is unchanged")
    ap.add_argument("--export-count", type=int, default=4, help="with --export-mesh: how many faces to write")
    ap.add_argument("--phase", choices=("train", "test"), default="train",
                    help="trainval.py's phase switch (:223-225).  test = the forward-only evaluation loop over independent batches "
                         "with the depth rendering in flight (run_test_phase); train = everything else this script does")
    return ap


def main():
    ap = build_parser()
    args = ap.parse_args()
    if args.photo_loss and not args.synth_data:
        ap.error("--photo-loss needs --synth-data (the term uses the batch's ground-truth lighting and albedo)")
    if args.synth_colour and not args.synth_data:
        ap.error("--synth-colour needs --synth-data (it is the synthetic batches' shading)")
    if args.silhouette_loss and not args.synth_data:
        ap.error("--silhouette-loss needs --synth-data (the term uses the batch's ground-truth mask)")
    if args.landmark_loss and not args.synth_data:
        ap.error("--landmark-loss needs --synth-data (the term uses the batch's ground-truth landmarks)")
    if args.export_mesh and (args.phase != "test" or args.im_size % 4):
        ap.error("--export-mesh needs --phase test and an image size that is a multiple of 4 (FineNet pools twice)")
    # (ONE line on stdout: RCCL prints a version banner to fd 1 when its first communicator comes up -- from here on fd 1 is
    # stderr and the JSON line goes to the saved real stdout)
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    global _emit
    _emit = lambda rec: os.write(real_stdout, (json.dumps(rec) + "\n").encode())   # noqa: E731
    dist_u = pkg("utils.dist")
    world, rank, local = dist_u.init_from_env()
    if args.phase == "test":
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        sys.exit(run_test_phase(args, dev, rank, world, local, dist_u))
    preset = None
    if args.config is not None:
        preset = CONFIG_PRESETS[args.config]
        named = 1 if args.config == 3 else args.shard_gpus
        args.batch = preset["global_batch"] // max(world, named)
        args.im_size, args.train, args.val, args.fine = preset["im_size"], preset["train"], preset["val"], preset["fine"]
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    model, net, opt, step = build_harness(args, dev, rank, world, local)
    if not args.train:
        model.eval()
    for _ in range(max(args.warmup, 1)):
        step()
    torch.cuda.synchronize(dev)
    dist_u.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out, L = step()
    torch.cuda.synchronize(dev)
    dt = dist_u.max_over_ranks(time.perf_counter() - t0, device=dev)
    dist_info = dist_u.describe(device=dev)   # (a collective: every rank calls it)
    if rank == 0:
        name = "configs[4]" if args.fine and not args.train else ("configs[3]" if args.train else "configs[2]")
        rec = {"metric": "faces/sec, caller config (%s)" % (preset["label"] if preset else name + " coarse_loop"),
               "value": world * args.batch * args.steps / dt, "unit": "faces/s", "higher_is_better": True,
               "data": "synthetic", "dtype": "f32", "scaling": "weak (per-GPU shard fixed)",
               "config": "%s coarse_loop" % name, "n_gpus": world, "faces_per_gpu": args.batch, "im_size": args.im_size,
               "global_batch_this_run": world * args.batch,
               "dist": dist_info,
               "ddp_allreduce_bytes_per_step": ddp_bucket_bytes(model, net),
               "nIter": args.nIter, "train": args.train, "val_forward": args.val, "fine": args.fine or args.train,
               "steps": args.steps, "faces_per_s": world * args.batch * args.steps / dt,
               "ms_per_step": 1e3 * dt / args.steps,
               "params_finite": bool(torch.isfinite(out["pred_params"]).all())}
        if L is not None:
            rec["losses"] = {k: float(v) for k, v in L.items()}
        if args.synth_data:
            rec["data"] = "synthetic, rendered on the device (pipeline.SynthBatches)"
            rec["synth_seed"] = args.synth_seed
        if args.photo_loss and L is not None:
            rec["photometric_loss"] = float(L["photometric_loss"])
        _emit(rec)
    dist_u.finalize()


if __name__ == "__main__":
    main()
