"""GPU: synthetic batches (csrc/fr_synth.hip, rendering_layer.ops.synth_*, pipeline.SynthBatches, examples/coarse_loop.py
--synth-data).  The three kernels are held to the numpy model of tests/ref_synth_batch.py bit for bit; the shader also to the
stock-torch composition within a derived bound; every batch of the pipeline to the eager composition of the public operators on
the parameters it returned; the callers run as programs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
from gpu_util import assert_bits_equal, net_mod, ops
import ref_synth_batch as RS
import synth_batch_child as child

pytestmark = pytest.mark.gpu
F = np.float32
LIGHT = ((0.3, 0.7), (-0.4, 0.4), (-0.4, 0.4), (0.2, 0.9))
KEYS = child.KEYS


def _dev():
    return torch.device("cuda:0")


def _alpha_ranges(K):
    return [(-1.0 - 0.125 * k, 0.5 + k) for k in range(K)]


def _cpu(t):
    return t.detach().cpu().numpy()


# ---- sampler ----------------------------------------------------------------------------------------------------------------------------
def _draw(seed, first, B, ns, ne, K, im=200, beta=0.7, focal=1e-3):
    got = ops().synth_params(seed, first, B, ns, ne, K, im, beta=beta, light_ranges=LIGHT, alpha_ranges=_alpha_ranges(K), focal=focal,
                             device=_dev())
    torch.cuda.synchronize()
    assert not any(t.requires_grad for t in got)
    return [_cpu(t) for t in got]


@pytest.mark.parametrize("B, ns, ne, K", [(1, 9, 5, 3), (3, 9, 5, 10), (5, 199, 29, 10), (2, 0, 0, 0)])
@pytest.mark.parametrize("beta", [0.7, 1.0])
def test_sampler_bit_exact_against_the_model(B, ns, ne, K, beta):
    seed, first = 0x1234567890ABCDEF, 11
    got = _draw(seed, first, B, ns, ne, K, beta=beta)
    want = RS.sample(seed, first, B, ns, ne, K, 200, beta, LIGHT, _alpha_ranges(K))
    for g, w, name in zip(got, want, ("params", "light", "alpha")):
        assert_bits_equal(g, w, "%s at %s" % (name, (B, ns, ne, K, beta)))


def test_sampler_counts_faces_globally():
    ns, ne, K = 9, 5, 3
    whole = _draw(7, 0, 8, ns, ne, K)
    part = _draw(7, 5, 3, ns, ne, K)
    for w, p in zip(whole, part):
        assert_bits_equal(w[5:8], p, "rows 5..7 of a batch of 8 against the batch of 3 that starts at face 5")
    # the counter's word boundary: faces 2^32 - 2 .. 2^32 + 1
    first = 2 ** 32 - 2
    got = _draw(7, first, 4, ns, ne, K)
    want = RS.sample(7, first, 4, ns, ne, K, 200, 0.7, LIGHT, _alpha_ranges(K))
    for g, w in zip(got, want):
        assert_bits_equal(g, w, "faces across 2^32")
    assert len({r.tobytes() for r in got[0]}) == 4
    assert_bits_equal(got[0][2:], _draw(7, 2 ** 32, 2, ns, ne, K)[0], "g_hi = 1")
    other = _draw(8, 0, 8, ns, ne, K)
    assert not np.array_equal(whole[0], other[0]) and not np.array_equal(whole[1], other[1])      # two seeds differ


# ---- texture ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 3, 10])
@pytest.mark.parametrize("B", [1, 3])
def test_texture_bit_exact_against_the_model(small_assets, K, B):
    dev = _dev()
    mu, pc = small_assets["mu_tex"], np.ascontiguousarray(small_assets["pc_tex"][:, :K])
    alpha = np.random.RandomState(10 * K + B).uniform(-2, 2, (B, K)).astype(F)
    got = ops().synth_texture(torch.as_tensor(mu, device=dev), torch.as_tensor(pc, device=dev) if K else None,
                              torch.as_tensor(alpha, device=dev))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, 3, mu.shape[1]) and not got.requires_grad
    assert mu.shape[1] % 256 != 0 and mu.shape[1] > 256                  # more than one block, and a ragged last one
    assert_bits_equal(_cpu(got), RS.texture(mu, pc, alpha), "K = %d, B = %d" % (K, B))
    if K == 0:
        assert_bits_equal(_cpu(got), np.repeat(mu[None], B, 0), "K = 0 is the mean texture")


@pytest.mark.parametrize("K", [17, 33])
@pytest.mark.parametrize("B", [8, 9, 17])
def test_texture_bit_exact_across_column_chunks_and_face_groups(K, B):
    """the kernel takes pc_tex 16 columns at a time through LDS and eight faces per workgroup: K = 17 and 33 run the second and
    third chunk (one column each, behind the barrier that lets the tile be rewritten), B = 8, 9 and 17 a full group, a second
    group of one face and a third; N = 2 x 256 + 3 rows leaves a ragged last workgroup"""
    dev = _dev()
    N = 515
    rs = np.random.RandomState(100 * K + B)
    mu = rs.uniform(0, 1, (3, N)).astype(F)
    pc = rs.standard_normal((3 * N, K)).astype(F)
    alpha = rs.uniform(-2, 2, (B, K)).astype(F)
    got = ops().synth_texture(torch.as_tensor(mu, device=dev), torch.as_tensor(pc, device=dev), torch.as_tensor(alpha, device=dev))
    torch.cuda.synchronize()
    assert_bits_equal(_cpu(got), RS.texture(mu, pc, alpha), "K = %d, B = %d" % (K, B))


# ---- shade ------------------------------------------------------------------------------------------------------------------------------
def _hand_planes(B, H, W, seed):
    """planes that reach every branch: n_z < 0, mag <= 1e-6, s < 0, tex < 1e-6, a NaN in tex_img and one in normal, background on
    every border row and column and at scattered inner pixels"""
    rs = np.random.RandomState(seed)
    tex = rs.uniform(-0.2, 1.0, (B, H, W, 3)).astype(F)
    nrm = rs.standard_normal((B, H, W, 3)).astype(F)
    tiny = rs.uniform(size=(B, H, W)) < 0.1
    nrm[tiny] *= F(1e-4)
    ti = rs.randint(0, 500, (B, H, W, 1)).astype(F)
    ti[rs.uniform(size=(B, H, W)) < 0.2] = -1
    ti[:, 0], ti[:, -1], ti[:, :, 0], ti[:, :, -1] = -1, -1, -1, -1
    light = rs.uniform(-1, 1, (B, 4)).astype(F)
    nan_at = []
    if H >= 5 and W >= 5:   # one NaN in tex_img and one in normal, each in a covered inner pixel of its own
        for k, plane in enumerate((tex, nrm)):
            b, y, x = B - 1, 1 + k, 2
            ti[b, y, x, 0] = 3
            plane[b, y, x, 1] = np.nan
            nan_at.append((b, y, x))
    return tex, nrm, ti, light, nan_at


@pytest.mark.parametrize("B, H, W", [(1, 5, 6), (3, 33, 17), (2, 64, 64)])
@pytest.mark.parametrize("bg", ["none", "one", "batch"])
def test_shade_bit_exact_against_the_model(B, H, W, bg):
    dev = _dev()
    tex, nrm, ti, light, nan_at = _hand_planes(B, H, W, seed=H * W + B)
    back = {"none": None, "one": np.random.RandomState(1).uniform(0, 1, (1, H, W, 1)).astype(F),
            "batch": np.random.RandomState(2).uniform(0, 1, (B, H, W, 1)).astype(F)}[bg]
    gain, offset = 1.75, -0.125
    want_im, want_mask = RS.shade(tex, nrm, ti, light, back, gain, offset)
    covered = ti[..., 0] >= 0
    if B * H * W > 500:   # the planes reach every branch (the model's own intermediate values)
        flip = nrm[..., 2] < 0
        mag = (nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1]) + nrm[..., 2] * nrm[..., 2]
        assert (covered & flip).any() and (covered & ~flip).any() and (covered & (mag <= F(1e-6))).any()
        assert (covered & (tex < F(1e-6)).any(-1)).any() and (covered & (want_im[..., 0] == F(offset))).any()    # s < 0: I = 0
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev)   # noqa: E731
    im, mask = ops().synth_shade(t(tex), t(nrm), t(ti), t(light), background=t(back), gain=gain, offset=offset)
    torch.cuda.synchronize()
    assert not im.requires_grad and not mask.requires_grad
    assert_bits_equal(_cpu(im), want_im, "im_gray at %s, background %s" % ((B, H, W), bg))
    assert_bits_equal(_cpu(mask), want_mask, "mask")
    assert np.array_equal(_cpu(mask)[..., 0], covered.astype(F))
    # a NaN stays in its pixel
    nan_px = np.zeros((B, H, W), bool)
    for b, y, x in nan_at:
        nan_px[b, y, x] = True
    assert len(nan_at) == 2 and np.array_equal(np.isnan(_cpu(im)[..., 0]), nan_px)
    # every border row and column is background
    bgv = np.zeros((B, H, W), F) if back is None else np.broadcast_to(back[..., 0], (B, H, W))
    for sl in (np.s_[:, 0], np.s_[:, -1], np.s_[:, :, 0], np.s_[:, :, -1]):
        assert np.array_equal(_cpu(im)[..., 0][sl], bgv[sl]) and not _cpu(mask)[..., 0][sl].any()


@pytest.fixture(scope="module")
def small_render(small_assets):
    """one batch of the small assets at 32 x 32, B = 3, through the public operators: sampled, decoded, textured, rendered"""
    dev, B, S = _dev(), 3, 32
    net = net_mod().FaceRecNet(mesh_data=small_assets, batch_size=B, im_size=S, device=dev)
    K = int(net.pc_tex.shape[1])
    P, light, alpha = ops().synth_params(5, 0, B, net.ndim_shape, net.ndim_exp, K, S, light_ranges=LIGHT, alpha_ranges=1.0,
                                         focal=1e-3 * S / 200.0, device=dev)
    ver = net.vertices_transform(P)
    tex = ops().synth_texture(net.mu_tex, net.pc_tex, alpha)
    depth, tex_img, normal, tri_ind = ops().render_depth(ver, net.tri, tex, torch.zeros((B, S, S, 3), device=dev))
    torch.cuda.synchronize()
    return dict(net=net, light=light, tex_img=tex_img, normal=normal, tri_ind=tri_ind, B=B, S=S)


def test_shade_against_the_stock_torch_composition(small_render):
    r = small_render
    tex_img, normal, tri_ind, light = r["tex_img"], r["normal"], r["tri_ind"], r["light"]
    im, mask = ops().synth_shade(tex_img, normal, tri_ind, light)
    # the compute_abedo_image arithmetic (nets/network.py), then a relu(l . n')
    a = torch.clamp_min(tex_img, 1e-6).mean(dim=-1, keepdim=True)
    n = torch.where(normal[..., 2:3] < 0, -1.0 * normal, normal)
    mag = (n * n).sum(-1)
    mag = torch.where(mag > 1e-6, mag, torch.ones_like(mag))
    nm = n / (torch.sqrt(mag) + 1e-6)[..., None]
    s = light[:, None, None, 0:1] + (light[:, None, None, 1:4] * nm).sum(-1, keepdim=True)
    stock = a * torch.relu(s)
    torch.cuda.synchronize()
    covered = _cpu(tri_ind)[..., 0] >= 0
    assert 0.1 < covered.mean() < 0.95
    assert np.array_equal(_cpu(mask)[..., 0], covered.astype(F))                       # mask IS tri_ind >= 0
    want_im, want_mask = RS.shade(_cpu(tex_img), _cpu(normal), _cpu(tri_ind), _cpu(light))
    assert_bits_equal(_cpu(im), want_im, "im_gray on rendered planes")
    assert (_cpu(im)[..., 0][~covered] == 0).all()
    # about ten roundings per route, each relative 2^-24, on a sum of signed terms
    l64, n64, a64 = _cpu(light).astype(np.float64), _cpu(nm).astype(np.float64), _cpu(a).astype(np.float64)[..., 0]
    terms = np.abs(l64[:, None, None, 0]) + (np.abs(l64[:, None, None, 1:4] * n64)).sum(-1)
    bound = 32 * 2.0 ** -24 * a64 * terms
    diff = np.abs(_cpu(im).astype(np.float64) - _cpu(stock).astype(np.float64))[..., 0]
    print("shade vs stock torch: max |diff| / bound = %.3f over %d covered pixels" % ((diff[covered] / bound[covered]).max(),
                                                                                        covered.sum()))
    assert (diff[covered] <= bound[covered]).all()
    assert (_cpu(im)[..., 0][covered] > 0).mean() > 0.5                                # (lit faces, not a black image)


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------------
SEED, PB, PS = 91, 3, 32


def _clone(b):
    return {k: b[k].clone() for k in KEYS}


@pytest.fixture(scope="module")
def six_batches():
    net, st = child.stream(SEED, PB, PS, slots=2)
    got = []
    for _ in range(6):
        got.append(_clone(st.next()))
    torch.cuda.synchronize()
    return net, got


def test_pipeline_batches_are_the_eager_composition(six_batches):
    net, got = six_batches
    dev = _dev()
    K = int(net.pc_tex.shape[1])
    for n, b in enumerate(got):
        assert set(b) == set(KEYS) and not any(t.requires_grad for t in b.values())
        # the parameters are faces n B .. n B + B of the seed's sequence
        want = RS.sample(SEED, n * PB, PB, net.ndim_shape, net.ndim_exp, K, PS, 0.7, ops().SYNTH_LIGHT_RANGES, [(-1.0, 1.0)] * K,
                         focal=F(1e-3 * PS / 200.0))
        for key, w in zip(("params", "light", "alpha"), want):
            assert_bits_equal(_cpu(b[key]), w, "batch %d: %s" % (n, key))
        ver = net.vertices_transform(b["params"])
        tex = ops().synth_texture(net.mu_tex, net.pc_tex, b["alpha"])
        depth, tex_img, normal, tri_ind = ops().render_depth(ver, net.tri, tex, torch.zeros((PB, PS, PS, 3), device=dev))
        im, mask = ops().synth_shade(tex_img, normal, tri_ind, b["light"])
        depth_img = net.rendering_layer(ver, net.tri, net.vertex_code, im_gray=torch.ones((PB, PS, PS, 1), device=dev))[3]
        torch.cuda.synchronize()
        assert torch.equal(b["tri_ind"], tri_ind) and torch.equal(b["mask"], mask), n
        assert_bits_equal(_cpu(b["im_gray"]), _cpu(im), "batch %d: im_gray" % n)
        assert_bits_equal(_cpu(b["depth"]), _cpu(depth_img), "batch %d: depth" % n)
        assert_bits_equal(_cpu(b["depth"]), _cpu(torch.clamp_min(depth, 1e-6)), "batch %d: depth against render_depth" % n)
        cov = float((tri_ind >= 0).float().mean())
        assert 0.05 < cov < 0.98, (n, cov)
        assert float(b["im_gray"][b["mask"] > 0].mean()) > 0.02
    assert all(not torch.equal(got[0]["params"], g["params"]) for g in got[1:])


def test_a_batch_stays_until_slots_calls_later():
    slots = 2
    _, st = child.stream(SEED, PB, PS, slots=slots)
    first = st.next()
    keep = _clone(first)
    for later in range(1, slots):                  # calls 1 .. slots - 1: the first batch is still the caller's
        st.next()
        st.synchronize()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(first[k], keep[k]), (later, k)
    again = st.next()                              # call `slots`: the first batch's buffers are in the making again
    st.synchronize()
    torch.cuda.synchronize()
    assert again["params"].data_ptr() != first["params"].data_ptr()
    assert not torch.equal(first["params"], keep["params"])
    nxt = st.next()                                # ... and come back as batch slots + 1
    assert nxt["params"].data_ptr() == first["params"].data_ptr()


def test_two_ranks_reproduce_the_single_stream(six_batches):
    pipe = pkg("pipeline")
    net, single = six_batches
    ranks = []
    for rank in range(2):
        first, _ = pipe.synth_face_range(0, rank, 2, PB)
        _, st = child.stream(SEED, PB, PS, first_face=first, stride=2 * PB)
        ranks.append(st)
    for step in range(3):
        for rank in range(2):
            b = _clone(ranks[rank].next())
            torch.cuda.synchronize()
            for k in KEYS:   # the world = 1 stream's batch 2 step + rank holds exactly these faces
                assert torch.equal(b[k], single[2 * step + rank][k]), (step, rank, k)


def test_a_fresh_process_draws_the_same_bits(six_batches):
    _, got = six_batches
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "synth_batch_child.py"), str(SEED), str(PB), str(PS), "3"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("SYNTH_DIGEST ")]
    assert len(lines) == 1 and lines[0].split()[1] == child.digest(got[:3])


# ---- programs ---------------------------------------------------------------------------------------------------------------------------
def _run(cmd, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[-2000:]     # ONE line on stdout, nothing else
    return json.loads(lines[0])


TRAIN = ["examples/coarse_loop.py", "--small", "--train", "--steps", "2", "--warmup", "0"]
TEST = ["examples/coarse_loop.py", "--phase", "test", "--small", "--batch", "3", "--im-size", "32", "--steps", "3", "--warmup", "1"]
# what the programs print without the flag: the parent's records, key for key
TRAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "data", "dtype", "scaling", "config", "n_gpus", "faces_per_gpu", "im_size",
              "global_batch_this_run", "dist", "ddp_allreduce_bytes_per_step", "nIter", "train", "val_forward", "fine", "steps",
              "faces_per_s", "ms_per_step", "params_finite", "losses"}
TEST_KEYS = {"metric", "value", "unit", "higher_is_better", "data", "dtype", "phase", "n_gpus", "faces_per_gpu", "im_size", "steps",
             "ms_per_step", "batches_in_flight", "route", "depth_identical_to_one_batch_at_a_time", "dist"}
DUMP_NAMES = ("params", "vertex_proj", "depth", "texture_image", "normal", "tri_ind")


def test_train_program_on_synthetic_batches():
    d = _run(TRAIN + ["--synth-data"])
    assert d["train"] is True and d["steps"] == 2 and d["params_finite"] is True and d["value"] > 0
    assert "SynthBatches" in d["data"] and d["synth_seed"] == 3456
    assert d["losses"] and all(np.isfinite(v) for v in d["losses"].values()), d["losses"]
    assert set(d) == TRAIN_KEYS | {"synth_seed"}


def test_eval_program_reports_depth_rmse(tmp_path):
    dump = str(tmp_path / "synth.npz")
    d = _run(TEST + ["--synth-data", "--synth-seed", "17", "--dump-batches", dump])
    assert d["phase"] == "test" and d["steps"] == 3 and d["depth_identical_to_one_batch_at_a_time"] is True
    assert np.isfinite(d["depth_rmse"]) and d["depth_rmse"] >= 0 and d["synth_seed"] == 17
    assert set(d) == TEST_KEYS | {"depth_rmse", "synth_seed"}
    z = np.load(dump)
    assert float(z["depth_rmse"]) == d["depth_rmse"] and int(z["steps"]) == 3
    assert all(np.isfinite(z["params_%d" % k]).all() for k in range(3))


def test_programs_without_the_flag_print_the_parents_records(tmp_path):
    dump = str(tmp_path / "plain.npz")
    d = _run(TEST + ["--dump-batches", dump])
    assert set(d) == TEST_KEYS and d["data"] == "synthetic" and d["depth_identical_to_one_batch_at_a_time"] is True
    z = np.load(dump)
    want = {"steps", "mu", "pc_shape", "pc_exp", "tri", "vertex", "im_size"} | {"%s_%d" % (n, k) for n in DUMP_NAMES for k in range(3)}
    assert set(z.files) == want
    # the test generator is the parent's: four resident torch.rand images of a CPU generator seeded 100 + rank, timed batch k taking
    # image k.  Rebuilt here as the parent's program builds it: the dumped parameters are CoarseNet of THOSE images, in that order
    B, S = 3, 32
    netm, cn, dev = net_mod(), pkg("nets.coarse_net"), _dev()
    with torch.random.fork_rng(devices=[0]):
        torch.manual_seed(1234)
        face = netm.FaceRecNet(mesh_data=pkg("utils.synth").make_small_assets(), batch_size=B, im_size=S, device=dev)
        face.init_pred_params[..., 6] = 1e-3 * S / 200.0
        coarse = cn.CoarseNet(face, nIter=4).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(100)
    images = [torch.rand((B, S, S, 1), generator=g).to(dev) for _ in range(4)]
    with torch.no_grad():
        want_p = [_cpu(coarse(im)).reshape(B, -1) for im in images]
    for k in range(3):
        P = z["params_%d" % k]
        # same weights, same image, same kernels in another process: at most the convolution algorithm differs, a reordering of
        # fp32 sums whose effect stays orders of magnitude below 1e-3 of a column's size
        tol = 1e-3 * np.abs(want_p[k]).max(0, keepdims=True) + 1e-12
        dev_k = np.abs(P - want_p[k])
        print("batch %d: max |dumped - recomputed| / tol = %.3g" % (k, (dev_k / tol).max()))
        assert (dev_k <= tol).all(), k
        assert all(not np.array_equal(want_p[k], want_p[j]) for j in range(4) if j != k)
    t = _run(TRAIN)
    assert set(t) == TRAIN_KEYS and t["data"] == "synthetic" and all(np.isfinite(v) for v in t["losses"].values())
