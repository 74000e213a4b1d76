"""CPU: the consumer fuzz (tests/test_fuzz_consumers_gpu.py) is not vacuous.  Over its default 48 seeds -- the oracle and the numpy
models only, no GPU -- the scenes reach every class of input the fuzz exists for.  These are conditions on the INPUTS, not
measurements of the code under test.

Seed base fuzz_scenes.CONSUMER_BASE = 31000: the first base tried, and every condition below holds on it at the default count (the
bases to try next would have been 31100, 31200, ..).  What it gives, in cases of the 48 (all five scene kinds are drawn):
  covered pixels 47; normal backward, a face with non-finite terms 27; interpolated depth, the same 25; den == 0 under a covered
  pixel 34; a covered zero normal 30; a winner naming a vertex twice 23; tex_batch == 1 32; tex_batch == B > 1 16; B == 8 12; more
  than 2,000 vertices 20; an out-of-range id beside covered pixels 9; photo_loss flipped 41 / not 45, unit 30 / not 47, unlit 45 /
  lit 44, texture kept 47 / clamped 0; and in the second pass (below) a pixel naming a triangle whose third id alone is bad 47, a NaN
  tri_ind on a pixel the forward covered 47, a tri_ind >= ntri 45.
The second pass exists because two of the mutations the fuzz was checked with survived on rendered scenes: the rasteriser skips a
triangle with an id outside the mesh and writes whole indices or -1, so no rendered tri_ind names a bad-id triangle or holds a NaN,
and a consumer whose own test of the ids (or of the plane) is wrong goes unseen.  fuzz_scenes.ConsumerCase.altered hands the
consumers such a table and plane; the three conditions above hold it to doing so.
The photometric loss's texture clamp (tex_img < 1e-6 on a covered pixel) is out of the seeds' reach at any base: _scene draws its
textures from (0, 1), and a pixel's value is the mean of three.  fuzz_scenes.clamp_scene is the deterministic hand-made scene for
that class (the GPU file runs it), and it is held here to reaching both sides of every branch on its own."""
import os

import numpy as np
import pytest

import fuzz_scenes as FS
import ref_depth_interp as RD
import ref_normal_backward as RN
import ref_photo_loss as RP

N_RENDER = int(os.environ.get("FR_FUZZ_CASES", "160"))
N_CASES = max(1, N_RENDER * 3 // 10)


def case_stats(case, planes):
    """what one case reaches -> dict of counts / flags (planes: the oracle's depth, tex_img, normal, tri_ind)"""
    c = case
    tind = planes[3].reshape(c.B, -1)
    normal = planes[2].reshape(c.B, -1, 3)
    ids_all = RN.f2i_x86(c.tri)
    s = dict(covered=int((tind >= 0).sum()), B=c.B, nver=c.nver, tex_batch=c.tex_batch, kind=c.kind)
    s["bad_id_table"] = bool(((ids_all < 0) | (ids_all >= c.nver)).any()) and s["covered"] > 0
    s["den0"] = s["zero_normal"] = s["twice"] = 0
    for b in range(c.B):
        px, ids = RN.contributing(c.tri, tind[b], c.nver)
        q = RD.weights(c.ver[b], ids, px, c.W)
        s["den0"] += int(q["flat"].sum())
        s["zero_normal"] += int((normal[b][px] == 0).all(axis=1).sum())
        s["twice"] += int(((ids[0] == ids[1]) | (ids[0] == ids[2]) | (ids[1] == ids[2])).sum())
    s["normal_bad"] = sum(int(F.bad) for mode in (0, 1) for g in c.g_normal
                          for F in RN.model(g, c.ver, c.tri, tind, c.H, c.W, mode).faces)
    s["depth_bad"] = sum(int(F.bad) for g in c.g_depth for F in RD.model(g, c.ver, c.tri, tind, c.H, c.W).faces)
    a, plane = c.altered(tind)                                                 # the second pass: the altered table and plane
    third, t = RN.f2i_x86(a.tri[2]), RN.f2i_x86(tind)
    named = (t >= 0) & (t < a.tri.shape[1])
    s["named_bad_third"] = int((named & ((third < 0) | (third >= c.nver))[np.where(named, t, 0)]).sum())
    s["nan_where_covered"] = int((np.isnan(plane) & (tind >= 0)).sum())
    s["covered_not_counted"] = int(((plane >= 0) & ~(RN.f2i_x86(plane) < a.tri.shape[1])).sum())
    s["branches"] = RP.branches(planes[1], planes[2], planes[3], c.light)
    return s


def seed_set_reaches(stats):
    """the conditions on a seed set's statistics -> dict name -> (count of cases, holds)"""
    n = lambda f: sum(1 for s in stats if f(s))                                # noqa: E731
    need = len(stats) * 40 // 48
    out = {
        "covered pixels": (n(lambda s: s["covered"] > 0), need),
        "normal backward: a face with non-finite terms": (n(lambda s: s["normal_bad"] > 0), 1),
        "interpolated depth: a face with non-finite terms": (n(lambda s: s["depth_bad"] > 0), 1),
        "a covered pixel with den == 0": (n(lambda s: s["den0"] > 0), 1),
        "a covered pixel whose normal is exactly zero": (n(lambda s: s["zero_normal"] > 0), 1),
        "a winning triangle that names a vertex twice": (n(lambda s: s["twice"] > 0), 1),
        "tex_batch == 1": (n(lambda s: s["tex_batch"] == 1), 1),
        "tex_batch == B > 1": (n(lambda s: s["tex_batch"] == s["B"] > 1), 1),
        "B == 8": (n(lambda s: s["B"] == 8), 1),
        "more than 2,000 vertices": (n(lambda s: s["nver"] > 2000), 1),
        "an out-of-range id beside covered pixels": (n(lambda s: s["bad_id_table"]), 1),
        "altered pass: pixels naming a triangle whose third id alone is bad": (n(lambda s: s["named_bad_third"] > 0), 1),
        "altered pass: a NaN tri_ind on a pixel the forward covered": (n(lambda s: s["nan_where_covered"] > 0), 1),
        "altered pass: a tri_ind >= ntri (covered, not counted)": (n(lambda s: s["covered_not_counted"] > 0), 1),
    }
    for name in RP.BRANCHES:
        if not name.startswith("tex clamped"):
            out["photo_loss: " + name] = (n(lambda s: s["branches"][name]), 1)
    return out


@pytest.fixture(scope="module")
def stats(oracle):
    out = []
    for i in range(N_CASES):
        c = FS.ConsumerCase(i)
        out.append(case_stats(c, oracle.render_depth(c.ver, c.tri, c.tex, c.H, c.W)))
    return out


def test_the_seed_set_reaches_every_class(stats):
    table = seed_set_reaches(stats)
    print("; ".join("%s %d" % (k, v[0]) for k, v in table.items()))
    if N_CASES < 48:
        return                                                                 # the conditions are stated for the default count
    short = {k: v for k, v in table.items() if v[0] < v[1]}
    assert not short, short


def test_every_kind_is_drawn(stats):
    if N_CASES < 48:
        return
    assert {s["kind"] for s in stats} == set(range(len(FS.KINDS)))


def test_the_texture_clamp_is_out_of_the_seeds_reach_and_the_hand_made_scene_reaches_it(oracle, stats):
    assert not any(s["branches"]["tex clamped"] for s in stats)               # (0, 1) textures: see the module docstring
    c = FS.clamp_scene()
    planes = oracle.render_depth(c.ver, c.tri, c.tex, c.H, c.W)
    assert all(RP.branches(planes[1], planes[2], planes[3], c.light).values())
    assert (planes[3] >= 0).any() and not (planes[3] >= 0).all()


def test_consumer_scene_is_the_scene_cut_down():
    for seed in (FS.CONSUMER_BASE, FS.CONSUMER_BASE + 7, 1003, 1017):
        ver, tri, tex, H, W, kind, drawn = FS.consumer_scene(seed)
        full = FS._scene(drawn)
        assert (drawn - seed) % FS.CONSUMER_STRIDE == 0 and ver.shape[0] <= FS.CONSUMER_FACES
        assert ver.shape[0] * H * W <= FS.CONSUMER_PIXELS and (H, W) == full[3:]
        assert ver.tobytes() == full[0][:FS.CONSUMER_FACES].tobytes() and tri.tobytes() == full[1].tobytes()
        per_face = full[2].shape[0] == full[0].shape[0]
        assert tex.tobytes() == (full[2][:FS.CONSUMER_FACES] if per_face else full[2]).tobytes()
        assert tex.shape[0] in (1, ver.shape[0])
