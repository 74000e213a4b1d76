"""GPU: every entry point called from several host threads at once, held to its single-threaded result bit for bit.

include/fr_hotpath.h promises a reentrant C ABI and says which concurrent uses it supports; rendering_layer/ops.py, nets/network.py
and pipeline.py keep host-side caches that threads share.  Every path here is deterministic by design (the forward is bit-exact,
both backwards sum in a fixed order or in fixed point), so each threaded result must EQUAL the job's reference, computed first on
one thread and anchored to the CPU oracle on at least one face: forward planes and decodes bit for bit, backwards within the bounds
of tests/test_backward_gpu.py and tests/test_decode_backward_bounds_gpu.py.  Anything less than equality is a finding.

  A  a fresh child process whose eight threads make their FIRST calls into the library at the same moment, one entry point each;
  B  warm: eight threads on eight streams (more than ops.WS_CACHE_MAX) loop over the Python surface at different shapes;
  C  threads sharing torch's default stream with two triangle lists of one geometry: the packed-table reuse of ops.py;
  D  the phases of one DecodeRenderPlan forward under two strip geometries, and the strip hint's validation;
  E  the decode backward's workspace LRU under six streams.
No graph capture; fixed repetition counts; every wait is bounded."""
import ctypes
import json
import os
import subprocess
import sys
import threading
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import test_decode_backward_bounds_gpu as DB
import threads_cold_child as cold
from conftest import ROOT, pkg
from gpu_util import assert_render_equal, net_mod, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IM = 200
WAIT = 180          # seconds: the bound of every wait on a thread
PLANES = ("depth", "texture_image", "normal", "tri_ind")


def _h():
    return pkg("_lib")


def _pipe():
    return pkg("pipeline")


def _overlap(fns):
    """fns[i]() on thread i, all released at once by a barrier -> their results, in order.  A hang fails the test."""
    barrier = threading.Barrier(len(fns))

    def go(fn):
        barrier.wait(timeout=60)
        return fn()

    ex = ThreadPoolExecutor(max_workers=len(fns))
    try:
        futs = [ex.submit(go, fn) for fn in fns]
        return [f.result(timeout=WAIT) for f in futs]
    finally:
        ex.shutdown(wait=False, cancel_futures=True)


def _bits(t):
    t = t.detach()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _diff(got, want):
    """number of elements whose bits differ (0 = equal)"""
    if tuple(got.shape) != tuple(want.shape):
        return -1
    return int((_bits(got) != _bits(want)).sum())


def _rand_params(rs, B, ns, ne):
    P = np.zeros((B, 7 + ns + ne), np.float32)
    P[:, 0:3] = rs.uniform(-1.5, 1.5, (B, 3))
    P[:, 3:5] = rs.uniform(0, IM, (B, 2))
    P[:, 5] = rs.uniform(-1, 1, B)
    P[:, 6] = rs.uniform(2e-4, 1e-3, B)
    P[:, 7:7 + ns] = rs.uniform(0, 1e4, (B, ns))
    P[:, 7 + ns:] = rs.uniform(-1.5, 1.5, (B, ne))
    return P


def _check_decode_grad(oracle, A, packed, B, P, G, R, V, gp, tag):
    """the decode backward of the faces given (some of a launch of B faces; a face's bits do not depend on its batch), against
    the float64 gradient under the proven bound of tests/test_decode_backward_bounds_gpu.py for that launch"""
    kind = "packed" if packed else "ref"
    rig = types.SimpleNamespace(N=A["mu"].size // 3, ns=A["pc_shape"].shape[1], ne=A["pc_exp"].shape[1])
    ref = DB.Ref(oracle, A, P, G, R=R)
    DB._check(gp.astype(np.float64), ref, DB._depths(kind, rig, B), kind, Vg=V, tag=tag)


def _check_render_grad(oracle, A, G, tind, vg, tag):
    """the render backward against the oracle's, as tests/test_backward_gpu.py holds it"""
    want = oracle.render_depth_grad(G, A["tri"], tind, vg.shape[2])
    assert np.all(vg[:, :2] == 0), tag
    np.testing.assert_allclose(vg[:, 2], want[:, 2], rtol=0, atol=2e-5, err_msg=tag)
    assert np.abs(vg).max() > 0, tag


# ---- A: cold start ------------------------------------------------------------------------------------------------------------------
def test_cold_start_every_entry_point_at_once(oracle, synth, small_assets, tmp_path):
    A = small_assets
    h = _h()
    L = h.lib()
    B, im = 3, 64
    ns, ne = A["pc_shape"].shape[1], A["pc_exp"].shape[1]
    N, ntri = A["mu"].size // 3, A["tri"].shape[1]
    P = synth.sample_params_batch(B, im_size=im, n_shape=ns, n_exp=ne, beta=0.7, seed=5)
    R = oracle.rotation_matrix_batch(P[:, :3])
    V = oracle.decode_3dmm(P, A["mu"], A["pc_shape"], A["pc_exp"], float(im), R=R)
    want = oracle.render_depth(V, A["tri"], A["vertex"][None], im, im)
    rs = np.random.RandomState(11)
    inputs = dict(P=P, R=R, mu=np.asarray(A["mu"], np.float32).reshape(-1), pc_shape=A["pc_shape"], pc_exp=A["pc_exp"], V=V,
                  tri=A["tri"], tex=A["vertex"], im_gray=rs.uniform(0, 1, (B, im, im, 1)), tri_ind=want[3],
                  G_px=rs.standard_normal((B, im, im, 1)), G_v=rs.standard_normal((B, 3, N)))
    inputs = {k: np.ascontiguousarray(v, np.float32) for k, v in inputs.items()}
    S = dict(B=B, N=N, ns=ns, ne=ne, ntri=ntri, H=im, W=im, im=float(im),
             packed_basis_bytes=L.fr_decode_packed_basis_bytes(N, ns, ne),
             q30_image_bytes=L.fr_decode_q30_image_bytes(N, ns, ne), q30_ws_bytes=L.fr_decode_q30_workspace_bytes(ns, ne),
             render_ws_bytes=L.fr_render_depth_workspace_bytes(B, N, ntri, im, im),
             render_bwd_ws_bytes=L.fr_render_depth_backward_workspace_bytes(B, im, im),
             decode_bwd_ws_bytes=L.fr_decode_backward_workspace_bytes(B, N, ns, ne), pitch=L.fr_decode_render_vertex_pitch(N),
             vertex_bytes=L.fr_decode_render_vertex_bytes(B, N))
    assert S["vertex_bytes"] == B * 3 * S["pitch"] * 4, S
    assert all(S[k] > 0 for k in ("packed_basis_bytes", "q30_image_bytes", "q30_ws_bytes", "render_ws_bytes")), S
    np.savez(os.path.join(tmp_path, "inputs.npz"), **inputs)
    json.dump(S, open(os.path.join(tmp_path, "sizes.json"), "w"))

    # the references: the same jobs one after the other on this thread
    T = cold.upload(inputs, DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    qimage = torch.empty((max(S["q30_image_bytes"], 256),), dtype=torch.uint8, device=DEV)
    cold.pack_q30(L, T, S, qimage, st)
    ref = {}
    for j in cold.JOBS:
        out = cold.run_job(L, j, T, S, cold.prepare(j, T, S, DEV), st, qimage)
        torch.cuda.synchronize()
        ref[j] = {k: v.cpu().numpy() for k, v in out.items()}
    # ... anchored to the oracle
    assert (want[3] >= 0).mean() > 0.05
    np.testing.assert_array_equal(ref["decode"]["out"], V)
    np.testing.assert_array_equal(ref["decode_q30"]["out"],
                                  oracle.decode_3dmm_q30(P, A["mu"], A["pc_shape"], A["pc_exp"], float(im), R=R, levels=cold.Q30_LEVELS))
    for j in ("render", "render_phases"):
        assert_render_equal(tuple(ref[j][k] for k in ("depth", "tex_img", "normal", "tri_ind")), want, j)
    np.testing.assert_array_equal(ref["layer"]["depth"], want[0])
    np.testing.assert_array_equal(ref["layer"]["tri_ind"], want[3])
    np.testing.assert_array_equal(ref["layer"]["depth_img"], np.maximum(want[0], np.float32(1e-6)))
    for k in ("vg_ws", "vg"):
        _check_render_grad(oracle, A, inputs["G_px"], want[3], ref["render_bwd"][k], "cold reference " + k)
    _check_decode_grad(oracle, A, False, B, P, inputs["G_v"], R, V, ref["decode_bwd"]["gp"], "cold reference decode_bwd")
    assert np.abs(ref["decode_bwd"]["gp"]).max() > 0
    np.testing.assert_array_equal(ref["decode_render"]["vertex"][:, :, :N], V)
    assert_render_equal(tuple(ref["decode_render"][k] for k in ("depth", "tex_img", "normal", "tri_ind")), want, "decode_render")

    # the child: one at a time, its own process (never an exec of this one)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [cold.__file__, str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "child exit %d:\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    bad = []
    for j in cold.JOBS:
        for k, w in ref[j].items():
            g = np.load(os.path.join(tmp_path, "out_%s_%s.npy" % (j, k)))
            if g.shape != w.shape or not np.array_equal(g.view(np.int32), w.view(np.int32)):
                bad.append("%s.%s: %d elements differ" % (j, k, int((g != w).sum()) if g.shape == w.shape else -1))
    assert not bad, bad


# ---- B: warm, one stream per thread -------------------------------------------------------------------------------------------------
class _Job:
    """One call of the Python surface at one shape.  run(net) launches on torch's current stream and returns its outputs."""

    def __init__(self, oracle, kind, A, B, seed):
        self.kind, self.A, self.B = kind, A, B
        ns, ne = A["pc_shape"].shape[1], A["pc_exp"].shape[1]
        self.N = A["mu"].size // 3
        rs = np.random.RandomState(seed)
        if kind == "decode":
            self.P = _rand_params(rs, B, ns, ne)
            self.G = (rs.standard_normal((B, 3, self.N)) * np.exp(rs.uniform(-3, 3, (B, 3, self.N)))).astype(np.float32)
        else:
            self.P = pkg("utils.synth").sample_params_batch(B, im_size=IM, n_shape=ns, n_exp=ne, beta=0.7, seed=seed)
            self.G = rs.standard_normal((B, IM, IM, 1)).astype(np.float32)
        self.R = oracle.rotation_matrix_batch(self.P[:, :3])
        if kind in ("render", "layer"):
            self.V = oracle.decode_3dmm(self.P, A["mu"], A["pc_shape"], A["pc_exp"], float(IM), R=self.R)
            self.img = rs.uniform(0, 1, (B, IM, IM, 1)).astype(np.float32)
        self.plans = {}

    def tensors(self):
        t = {k: torch.as_tensor(getattr(self, k), device=DEV) for k in ("P", "G", "R")}
        if self.kind in ("render", "layer"):
            t["V"], t["img"] = torch.as_tensor(self.V, device=DEV), torch.as_tensor(self.img, device=DEV)
        return t

    def setup(self, net):
        if self.kind == "plan":   # one plan per (job, net): built here, on the main thread
            self.plans[id(net)] = _pipe().DecodeRenderPlan(net, self.B, IM, IM)

    def run(self, net, t):
        if self.kind == "decode":
            p = t["P"].clone().requires_grad_(True)
            V = net.vertices_transform(p, R=t["R"])
            V.backward(t["G"])
            return [V.detach(), p.grad]
        if self.kind == "render":
            v = t["V"].clone().requires_grad_(True)
            outs = ops().render_depth(v, net.tri, net.vertex_code, torch.zeros((self.B, IM, IM, 3), device=DEV))
            outs[0].backward(t["G"])
            return list(outs) + [v.grad]
        if self.kind == "layer":
            v = t["V"].clone().requires_grad_(True)
            outs = ops().rendering_layer_fused(v, net.tri, net.vertex_code, t["img"])
            outs[2].backward(t["G"])
            return list(outs) + [v.grad]
        plan = self.plans[id(net)]
        return [o.clone() for o in plan.step(t["P"])] + [plan.vertex_proj.clone()]

    def anchor(self, oracle, out):
        """face 0 of the reference against the oracle; and the reference is not trivial"""
        A, tag = self.A, "%s B=%d N=%d" % (self.kind, self.B, self.N)
        o = [x.detach().cpu().numpy() for x in out]
        if self.kind == "decode":
            np.testing.assert_array_equal(o[0][:1], oracle.decode_3dmm(self.P[:1], A["mu"], A["pc_shape"], A["pc_exp"], float(IM),
                                                                       R=self.R[:1]), err_msg=tag)
            _check_decode_grad(oracle, A, self.packed, self.B, self.P[:1], self.G[:1], self.R[:1], o[0][:1], o[1][:1], tag)
            assert np.abs(o[1]).max() > 0, tag
            return
        if self.kind == "plan":
            V = o[4][:1]
            want = oracle.render_depth(V, A["tri"], A["vertex"][None], IM, IM)
            assert_render_equal(tuple(x[:1] for x in o[:4]), want, tag)
            Vo = oracle.decode_3dmm(self.P[:1], A["mu"], A["pc_shape"], A["pc_exp"], float(IM), R=self.R[:1])
            assert np.all(np.abs(V - Vo) <= 2 * np.spacing(np.maximum(np.abs(Vo), np.float32(1.0)))), tag
            assert (want[3] >= 0).mean() > 0.01, tag
            return
        want = oracle.render_depth(self.V[:1], A["tri"], A["vertex"][None], IM, IM)
        if self.kind == "render":
            assert_render_equal(tuple(x[:1] for x in o[:4]), want, tag)
        else:
            np.testing.assert_array_equal(o[2][:1], want[0], err_msg=tag)
            np.testing.assert_array_equal(o[3][:1], want[3], err_msg=tag)
        assert (want[3] >= 0).mean() > 0.01, tag
        _check_render_grad(oracle, A, self.G[:1], want[3], o[-1][:1], tag)


def test_warm_threads_one_stream_each(oracle, synth, full_assets, small_assets):
    meshes = {"full": full_assets, "small": small_assets,
              "s199": synth.make_assets(13, 17, 199, 29, patch=None, seed_basis=221),
              "ragged": synth.make_assets(7, 9, 1, 1, patch=None, seed_basis=63),     # N = 63: < 4 tiles, ragged last tile
              "r65": synth.make_assets(9, 10, 40, 7, patch=None, seed_basis=90),      # 65 faces: a second 64-face pass
              "r130": synth.make_assets(6, 8, 20, 3, patch=None, seed_basis=48)}      # 130 faces: two wide passes + 2
    spec = [[("decode", "full", 1), ("render", "full", 1)],
            [("layer", "full", 2), ("plan", "full", 2), ("decode", "full", 2)],
            [("decode", "s199", 17), ("render", "s199", 5), ("layer", "s199", 5)],
            [("plan", "s199", 8), ("decode", "s199", 8)],
            [("decode", "small", 3), ("render", "small", 3), ("layer", "small", 3), ("plan", "small", 3)],
            [("decode", "ragged", 1), ("decode", "r65", 65)],
            [("decode", "r130", 130), ("render", "small", 8)],
            [("plan", "small", 1), ("layer", "small", 1)]]
    assert len(spec) > ops().WS_CACHE_MAX
    netm = net_mod()
    # the references run on nets of their own: the threads' nets are fresh, so their lazy builds (PackedBasis.image_t, the
    # backward workspaces) happen while other threads launch
    ref_nets = {m: netm.FaceRecNet(mesh_data=A, batch_size=1, im_size=IM) for m, A in meshes.items()}
    nets = {m: netm.FaceRecNet(mesh_data=A, batch_size=1, im_size=IM) for m, A in meshes.items()}
    threads = []
    seed = 100
    for row in spec:
        jobs = []
        for kind, m, B in row:
            seed += 1
            j = _Job(oracle, kind, meshes[m], B, seed)
            j.mesh = m
            j.packed = nets[m]._basis.backward_packed_ok()
            j.setup(ref_nets[m])
            j.setup(nets[m])
            j.t = j.tensors()
            jobs.append(j)
        threads.append(jobs)
    torch.cuda.synchronize()
    for jobs in threads:
        for j in jobs:
            j.ref = j.run(ref_nets[j.mesh], j.t)
            torch.cuda.synchronize()
            j.anchor(oracle, j.ref)
    streams = [torch.cuda.Stream(device=DEV) for _ in threads]
    ITERS = 20

    def worker(i):
        bad = []
        with torch.cuda.stream(streams[i]):
            for it in range(ITERS):
                j = threads[i][it % len(threads[i])]
                out = j.run(nets[j.mesh], j.t)
                streams[i].synchronize()
                for k, (g, w) in enumerate(zip(out, j.ref)):
                    d = _diff(g, w)
                    if d:
                        bad.append("thread %d iter %d %s/%s B=%d output %d: %d differ" % (i, it, j.kind, j.mesh, j.B, k, d))
        return bad

    bad = sum(_overlap([lambda i=i: worker(i) for i in range(len(threads))]), [])
    assert not bad, bad[:10]


# ---- C: one shared stream, two triangle lists of one geometry ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared_scene(oracle, full_assets, synth):
    """the full-size mesh, 2 faces at 200 x 200, and tri2 = a permutation of tri1's columns (other tri_ind, the same ids): a
    wrong table gives wrong planes, never an out-of-bounds read.  Geometries are never mixed on a shared stream."""
    A = full_assets
    B = 2
    net = net_mod().FaceRecNet(mesh_data=A, batch_size=B, im_size=IM)
    P = synth.sample_params_batch(B, im_size=IM, beta=0.7, seed=77)
    R = oracle.rotation_matrix_batch(P[:, :3])
    Vn = oracle.decode_3dmm(P, A["mu"], A["pc_shape"], A["pc_exp"], float(IM), R=R)
    perm = np.random.RandomState(3).permutation(A["tri"].shape[1])
    s = types.SimpleNamespace(A=A, B=B, net=net, V=torch.as_tensor(Vn, device=DEV), tri1=net.tri,
                              tri2=net.tri[:, torch.as_tensor(perm, device=DEV)].contiguous(),
                              img=torch.as_tensor(np.random.RandomState(4).uniform(0, 1, (B, IM, IM, 1)).astype(np.float32), device=DEV))
    s.image = torch.zeros((B, IM, IM, 3), device=DEV)
    o = ops()
    s.call = {"render": lambda tri: o.render_depth(s.V, tri, net.vertex_code, s.image),
              "layer": lambda tri: o.rendering_layer_fused(s.V, tri, net.vertex_code, s.img)}
    o.clear_workspace_cache()
    s.ref = {}
    for name, fn in s.call.items():
        for k, tri in ((1, s.tri1), (2, s.tri2)):
            s.ref[name, k] = [t.clone() for t in fn(tri)]
    torch.cuda.synchronize()
    for k, tri_np in ((1, A["tri"]), (2, np.ascontiguousarray(A["tri"][:, perm]))):
        want = oracle.render_depth(Vn[:1], tri_np, A["vertex"][None], IM, IM)
        assert_render_equal(tuple(t[:1].cpu().numpy() for t in s.ref["render", k]), want, "tri%d" % k)
        np.testing.assert_array_equal(s.ref["layer", k][2][:1].cpu().numpy(), want[0])
        np.testing.assert_array_equal(s.ref["layer", k][3][:1].cpu().numpy(), want[3])
        assert (want[3] >= 0).mean() > 0.2
    assert _diff(s.ref["render", 1][3], s.ref["render", 2][3]) > 1000     # the two lists are told apart by tri_ind
    yield s
    o.clear_workspace_cache()


def _mismatch(s, name, k, out):
    return {n: d for n, d in ((n, _diff(g, w)) for n, g, w in zip(range(4), out, s.ref[name, k])) if d}


@pytest.mark.parametrize("name,fn_name", [("render", "fr_render_depth_forward_phases"),
                                          ("layer", "fr_rendering_layer_forward_phases")])
def test_shared_stream_forced_interleaving(shared_scene, monkeypatch, name, fn_name):
    """C1: thread A (tri1) decides to skip the pack -- the default stream's table came from tri1 -- then thread B (tri2) runs its
    whole call, then A launches.  A must still get tri1's planes.  A's wrapper of the C entry point waits up to 1 s for B's launch
    to return: with the decision, launch and record atomic per workspace entry B cannot launch in between, A's wait times out and
    A goes on."""
    s = shared_scene
    o = ops()
    L = o._host().lib()                        # (the library handle ops.py calls through)
    o.clear_workspace_cache()
    s.call[name](s.tri1)                       # warm the default stream's entry with tri1's table
    torch.cuda.synchronize()
    real = getattr(L, fn_name)
    a_in, b_done = threading.Event(), threading.Event()
    order = []

    def wrapper(*args):
        if args[1].value == s.tri1.data_ptr():    # thread A: it has decided its phases
            a_in.set()
            order.append(("A waits", b_done.wait(timeout=1.0)))
            return real(*args)
        rc = real(*args)
        b_done.set()
        order.append(("B launched",))
        return rc

    monkeypatch.setattr(L, fn_name, wrapper)

    def thread_a():
        out = [t.clone() for t in s.call[name](s.tri1)]
        torch.cuda.synchronize()
        return out

    def thread_b():
        assert a_in.wait(timeout=30)
        out = [t.clone() for t in s.call[name](s.tri2)]
        torch.cuda.synchronize()
        return out

    a, b = _overlap([thread_a, thread_b])
    monkeypatch.undo()
    bad_a, bad_b = _mismatch(s, name, 1, a), _mismatch(s, name, 2, b)
    assert not bad_a and not bad_b, "mismatching elements by output: A (tri1) %s, B (tri2) %s; order %s" % (bad_a, bad_b, order)


def test_shared_stream_unforced(shared_scene):
    """C2: two threads on the default stream, tri1 and tri2, render_depth and the fused layer in turn, 100 calls each."""
    s = shared_scene
    ops().clear_workspace_cache()

    def worker(k):
        bad = []
        tri = s.tri1 if k == 1 else s.tri2
        for it in range(100):
            name = ("render", "layer")[it % 2]
            out = s.call[name](tri)
            mm = _mismatch(s, name, k, out)
            if mm:
                bad.append("tri%d iter %d %s: %s" % (k, it, name, mm))
        torch.cuda.synchronize()
        return bad

    bad = sum(_overlap([lambda: worker(1), lambda: worker(2)]), [])
    assert not bad, bad[:10]


# ---- D: the phases of one plan forward ----------------------------------------------------------------------------------------------
def _geom(B, ntri, rows):
    out = (ctypes.c_int * 4)()
    _h().lib().fr_debug_render_geom(B, ntri, IM, IM, rows, out)
    return dict(rows=out[0], strips=out[1], binned=bool(out[3]))


def test_phase_split_refuses_a_resolve_under_another_geometry(oracle, full_assets, synth):
    """Emit through render_phase(1) under the library's strip height, then change FR_RENDER_ROWS: render_phase(2) must raise
    before it launches anything (the planes keep what they held).  The other height has FEWER strips than the emit's, so a
    library without the check resolves from offsets the emit did write: wrong planes, never an out-of-bounds read."""
    A = full_assets
    h = _h()
    B = 2
    net = net_mod().FaceRecNet(mesh_data=A, batch_size=B, im_size=IM)
    ntri = int(net.tri.shape[1])
    auto = _geom(B, ntri, 0)
    other = auto["rows"] + 3
    og = _geom(B, ntri, other)
    assert auto["binned"] and og["binned"] and og["strips"] < auto["strips"], (auto, og)
    assert h.get_option("FR_RENDER_ROWS") == 0
    P = torch.as_tensor(synth.sample_params_batch(B, im_size=IM, beta=0.7, seed=31), device=DEV)
    plan = _pipe().DecodeRenderPlan(net, B, IM, IM, strip_rows=0)
    ref = [t.clone() for t in plan.step(P)]
    torch.cuda.synchronize()
    want = oracle.render_depth(plan.vertex_proj[:1].contiguous().cpu().numpy(), A["tri"], A["vertex"][None], IM, IM)
    assert_render_equal(tuple(t[:1].cpu().numpy() for t in ref), want, "plan reference")
    assert (want[3] >= 0).mean() > 0.2

    def same(tag):
        torch.cuda.synchronize()
        bad = {n: _diff(g, w) for n, g, w in zip(PLANES, plan.outputs(), ref) if _diff(g, w)}
        assert not bad, "%s: %s" % (tag, bad)

    def refused(tag):
        for t in plan.outputs():
            t.fill_(7.0)
        try:
            plan.render_phase(2)
            raised = False
        except RuntimeError:
            raised = True
        torch.cuda.synchronize()
        written = {n: int((t != 7.0).sum()) for n, t in zip(PLANES, plan.outputs())}
        wrong = {n: _diff(g, w) for n, g, w in zip(PLANES, plan.outputs(), ref)}
        assert raised and not any(written.values()), ("%s: raised %s; elements written %s; elements that differ from the "
                                                      "reference %s" % (tag, raised, written, wrong))

    plan.render_phase(1)
    with h.options(FR_RENDER_ROWS=other):
        refused("emitted at %d rows, resolved at %d" % (auto["rows"], other))
        plan.step()                                            # a whole step under the new height: the reference's bits
        same("step() at %d rows" % other)
        plan.render_phase(1)
        plan.render_phase(2)
        same("emit + resolve at %d rows" % other)
    refused("emitted at %d rows, options restored" % other)
    plan.step()
    same("step() after the change")
    for k in range(3):                                         # resolving again and again after one step (tools/emit_probe.py)
        plan.render_phase(2)
        same("resolve %d after one step" % k)
    fresh = _pipe().DecodeRenderPlan(net, B, IM, IM)
    with pytest.raises(RuntimeError):
        fresh.render_phase(2)                                  # no emit yet


def test_strip_rows_is_validated_and_read_only(small_assets):
    pipe = _pipe()
    B = 4
    net = net_mod().FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=IM)
    plan = pipe.DecodeRenderPlan(net, B, IM, IM, strip_rows=9)
    assert plan.strip_rows == 9
    with pytest.raises(AttributeError):
        plan.strip_rows = 3
    assert plan.strip_rows == 9
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            pipe.DecodeRenderPlan(net, B, IM, IM, strip_rows=bad)
    assert pipe.DecodeRenderPlan(net, B, IM, IM, strip_rows=255).strip_rows == 255
    auto = pipe.BatchesInFlight(net, B, IM, IM, slots=2)
    neg = pipe.BatchesInFlight(net, B, IM, IM, slots=2, strip_rows=-1)   # as bench.py --strip-rows -1: auto
    assert neg.strip_rows == auto.strip_rows == pipe.BatchesInFlight.strip_rows_in_flight(net, B, IM, IM)
    assert all(sl.strip_rows == neg.strip_rows for sl in neg.slots)
    with pytest.raises(AttributeError):
        neg.strip_rows = 3
    neg.synchronize()
    auto.synchronize()


# ---- E: the decode backward's workspace LRU ----------------------------------------------------------------------------------------
def test_decode_backward_workspace_lru_under_six_streams(oracle, synth):
    A = synth.make_assets(13, 17, 199, 29, patch=None, seed_basis=221)
    net = net_mod().FaceRecNet(mesh_data=A, batch_size=1, im_size=IM)
    basis = net._basis
    ns, ne = net.ndim_shape, net.ndim_exp
    NT, ITERS = 6, 30
    jobs = []
    for i in range(NT):
        rs = np.random.RandomState(500 + i)
        B = 2 + i
        P = _rand_params(rs, B, ns, ne)
        G = rs.standard_normal((B, 3, net.nvert)).astype(np.float32)
        R = oracle.rotation_matrix_batch(P[:, :3])
        t = [torch.as_tensor(x, device=DEV) for x in (P, G, R)]
        jobs.append((P, G, R, t))

    def run(t):
        p = t[0].clone().requires_grad_(True)
        V = net.vertices_transform(p, R=t[2])
        V.backward(t[1])
        return V.detach(), p.grad

    refs = []
    for P, G, R, t in jobs:
        V, gp = run(t)
        torch.cuda.synchronize()
        refs.append(gp.clone())
        _check_decode_grad(oracle, A, basis.backward_packed_ok(), P.shape[0], P[:1], G[:1], R[:1], V[:1].cpu().numpy(),
                           gp[:1].cpu().numpy(), "lru reference")
        assert float(gp.abs().max()) > 0
    streams = [torch.cuda.Stream(device=DEV) for _ in range(NT)]

    def worker(i):
        bad = []
        t = jobs[i][3]
        B = t[0].shape[0]
        with torch.cuda.stream(streams[i]):
            for it in range(ITERS):
                _, gp = run(t)
                # the LRU itself, from six threads at once (autograd runs the backwards of one device on one thread)
                for _ in range(4):
                    with basis.backward_workspace(B, DEV) as (nws, buf):
                        assert buf.numel() >= nws
                streams[i].synchronize()
                d = _diff(gp, refs[i])
                if d:
                    bad.append("thread %d iter %d: %d differ" % (i, it, d))
        return bad

    bad = sum(_overlap([lambda i=i: worker(i) for i in range(NT)]), [])
    assert not bad, bad[:10]
    assert len(basis._bwd_ws) <= 4
