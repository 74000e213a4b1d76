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
that class (the GPU file runs it), and it is held here to reaching both sides of every branch on its own.
The soft coverage, the colour shading and the albedo fit joined the fuzz later; their draws come from streams of their own
(fuzz_scenes.ConsumerCase._draw_later_consumers), so the numbers above did not move.  What the same 48 cases give them:
  coverage, rendered pass: an OK / not-OK border 42; a live pair 38 (at least 36 are required: a silent majority of empty cases
  would otherwise go unseen); a record written 36; a soft value 37; Fc == 0 on the winning edge 8; two edges tie on s 4; a zero-area
  winner at a border 30; an OK pixel with a > 1 (clamped to 0) 14; a not-OK pixel with a > 1 (saturated) 4; an inert pair whose
  triangle has area 6; a backward face with non-finite terms, rendered or altered pass, 4; altered pass: an OK pixel beside one that
  is not OK by a bad id alone 46, a pixel covered and not OK 46;
  coverage, poisoned vertices (ConsumerCase.vertex_altered): a non-finite area under a border pixel 42, a poisoned triangle with a
  live pair 33 -- a rendered scene reaches neither, the rasteriser lets no such triangle win;
  coverage, vertices on a segment (ConsumerCase.vertex_on_segment): a tie on s inside (0, 1) with q != 0 on a face of finite terms
  37.  Every tie a scene holds is at s = 0 (a centre on a vertex of the lattice scenes: `open_ties` is empty on all 48), where no
  record is written and either edge gives the forward the same value: a tie rule that keeps the highest k passed every rendered
  and altered case, which is why the pass exists;
  photo_loss_rgb with the case's own lights: flipped 41 / not 45, unit 30 / not 47, lit 47 / 46 / 47 and unlit 18 / 15 / 14 per
  channel, mixed lit 31, an inner uncovered pixel 25, weighted 24, kept 47 per channel / clamped 0 (the clamp scene again, with
  colour lights of both signs); background_rgb None 22, [1,H,W,3] 8, [B,H,W,3] 18;
  albedo fit: K = 1 / 10 / 15 in 17 / 13 / 18 cases; a face with a non-finite moment 9 (a NaN normal, or the NaN and Inf the specials
  kind gets in im_gray); a face with finite moments and at least K + 1 counted pixels 38."""
import os

import numpy as np
import pytest

import fuzz_scenes as FS
import ref_albedo_lse as RA
import ref_coverage as RC
import ref_depth_interp as RD
import ref_normal_backward as RN
import ref_photo_loss as RP
import ref_photo_rgb as RPR

N_RENDER = int(os.environ.get("FR_FUZZ_CASES", "160"))
N_CASES = max(1, N_RENDER * 3 // 10)


def coverage_classes(c, tind, marked=None):
    """What the soft coverage meets on the case's table and vertices with the plane tind [B,npix], by the oracle's walk (ref_coverage's
    pair, edge and OK rule) -> dict of counts.  Pairs are counted once, from their OK pixel: `live`; `fc0` (Fc == 0 on the winning edge:
    the centre lies on it); `tie` (two candidate edges share the smallest s); `zero_area`, `bad_area` (not finite) and `inert_area` (a
    triangle with area and no candidate edge) for the inert ones; `live_marked`: live pairs of a triangle naming a vertex of
    marked [B,nver].  Pixels: `border` (a neighbour of the other state), `soft` (a value in (0, 1)), `ok_clamped` (an OK pixel with
    a > 1: the clamp at 0 acts), `saturated` (a not-OK pixel with a > 1: the clamp at 1 acts).  `open_ties` lists the tied pairs with
    0 < s < 1 -- the ones that write terms, to the winning edge's vertices -- as (face, pixel, neighbour, s)."""
    s = dict.fromkeys(("border", "live", "fc0", "tie", "zero_area", "bad_area", "inert_area", "live_marked", "soft", "ok_clamped",
                       "saturated"), 0)
    s["open_ties"] = []
    H, W = c.H, c.W
    for b in range(c.B):
        okt, tid = RC.ok_triangles(c.tri, tind[b], c.nver)
        for i in RC._border(okt, H, W):
            y, x = divmod(int(i), W)
            me, a = okt[i], 0.0
            s["border"] += 1
            for dx, dy in RC.NEIGHBOURS:
                nx, ny = x + dx, y + dy
                if nx < 0 or nx >= W or ny < 0 or ny >= H or (okt[ny * W + nx] >= 0) == (me >= 0):
                    continue
                t = me if me >= 0 else okt[ny * W + nx]
                cc, nn = ((x, y), (nx, ny)) if me >= 0 else ((nx, ny), (x, y))
                P = RC._tri_xy(c.ver[b], tid, t)
                pr = RC.pair(P, cc, nn)
                if pr is not None:
                    a += max(0.5 - RC.clamp01(pr[1]), 0.0) if me >= 0 else max(RC.clamp01(pr[1]) - 0.5, 0.0)
                if me < 0:
                    continue
                if pr is None:
                    area = RC.edge(P[0][0], P[0][1], P[1][0], P[1][1], P[2][0], P[2][1])
                    s["zero_area" if area == 0 else ("inert_area" if np.isfinite(area) else "bad_area")] += 1
                    continue
                s["live"] += 1
                s["fc0"] += pr[2] == 0
                s["live_marked"] += marked is not None and bool(marked[b][tid[:, t]].any())
                sk = FS.candidate_s(P, cc, nn)
                s["tie"] += sk.count(min(sk)) > 1
                if sk.count(min(sk)) > 1 and 0.0 < pr[1] < 1.0:
                    s["open_ties"].append((b, int(i), ny * W + nx, pr[1]))
            s["soft"] += 0.0 < (max(0.0, 1.0 - a) if me >= 0 else min(1.0, a)) < 1.0
            s["ok_clamped" if me >= 0 else "saturated"] += a > 1.0
    return {k: v if k == "open_ties" else int(v) for k, v in s.items()}


def telling_ties(c, tind):
    """On the vertices of ConsumerCase.vertex_on_segment: the tied pairs with 0 < s < 1 whose q (the header's) is not zero on a
    profile of g_cov under which their face has finite terms only -- where the choice of the edge shows in the result -> count"""
    w = c.vertex_on_segment(tind)
    ties = coverage_classes(w, tind)["open_ties"]
    if not ties:
        return 0
    cov = RC.forward(w.ver, w.tri, tind, c.H, c.W).reshape(c.B, -1)
    count = 0
    for g in w.g_cov:
        R = RC.model(g, cov, w.ver, w.tri, tind, c.H, c.W)
        for b, i, j, sv in ties:
            q = (float(g[b, i]) if sv < 0.5 and cov[b, i] > 0 else 0.0) + (float(g[b, j]) if sv > 0.5 and cov[b, j] < 1 else 0.0)
            count += q != 0 and not R.faces[b].bad
    return count


def coverage_backward_stats(c, tind):
    """-> (faces with a non-finite term over both profiles of g_cov, records written on the first)"""
    cov = RC.forward(c.ver, c.tri, tind, c.H, c.W)
    R = [RC.model(g, cov, c.ver, c.tri, tind, c.H, c.W) for g in c.g_cov]
    return sum(int(F.bad) for M in R for F in M.faces), sum(len(p) for p in R[0].records)


def albedo_stats(c, planes, tind):
    """-> (faces with a non-finite moment, faces with every moment finite and at least K + 1 counted pixels).  A moment is a sum of
    products of the x of the counted pixels, all far from overflow when finite: it is finite iff every x is"""
    x, counted = RA.pixel_x(RA.basis_ref(c.tri, c.pc_tex), tind.reshape(c.B, c.H, c.W, 1), c.lighting, planes[2], c.abedo, c.im_gray)
    finite = np.isfinite(x).all(axis=(1, 2))
    return int((~finite).sum()), int((finite & (counted.sum(1) >= c.K + 1)).sum())


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
    # the soft coverage: the rendered pass, the altered pass, and the pass on poisoned vertices under the oracle's plane
    s["cov"], s["cov_altered"] = coverage_classes(c, tind), coverage_classes(a, plane)
    s["cov_bad"], s["cov_records"] = coverage_backward_stats(c, tind)
    s["cov_bad_altered"], s["cov_records_altered"] = coverage_backward_stats(a, plane)
    v = c.vertex_altered(tind)
    s["cov_vertex"] = coverage_classes(v, tind, marked=(v.ver.view(np.uint32) != c.ver.view(np.uint32)).any(axis=1))
    s["cov_open_ties"], s["cov_telling_ties"] = len(s["cov"]["open_ties"]), telling_ties(c, tind)
    okt = np.stack([RC.ok_triangles(a.tri, plane[b], c.nver)[0] for b in range(c.B)]).reshape(c.B, c.H, c.W)
    named_not_ok = (RN.f2i_x86(plane).reshape(okt.shape) >= 0) & (RN.f2i_x86(plane).reshape(okt.shape) < a.tri.shape[1]) & (okt < 0)
    ok = np.pad(okt >= 0, ((0, 0), (1, 1), (1, 1)))
    s["bad_id_beside_ok"] = int((named_not_ok & (ok[:, 1:-1, :-2] | ok[:, 1:-1, 2:] | ok[:, :-2, 1:-1] | ok[:, 2:, 1:-1])).sum())
    s["covered_not_ok"] = int(((plane.reshape(okt.shape) >= 0) & (okt < 0)).sum())
    # the colour shading, with the case's own lights; the albedo fit, on either plane
    s["branches_rgb"] = RPR.branches(planes[1], planes[2], planes[3], c.light_rgb, c.weight)
    s["bg_kind"], s["K"] = c.bg_kind, c.K
    s["albedo"] = tuple(map(sum, zip(albedo_stats(c, planes, tind), albedo_stats(a, planes, plane))))
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
    cov = lambda key, where="cov": n(lambda s: s[where][key] > 0)            # noqa: E731
    out.update({
        "coverage: a live pair": (cov("live"), len(stats) * 36 // 48),
        "coverage: an OK / not-OK border": (cov("border"), 1),
        "coverage: a record written": (n(lambda s: s["cov_records"] > 0), 1),
        "coverage: a soft value in (0, 1)": (cov("soft"), 1),
        "coverage: Fc == 0 on the winning edge": (cov("fc0"), 1),
        "coverage: two edges tie on s": (cov("tie"), 1),
        "coverage: a zero-area winner at a border": (cov("zero_area"), 1),
        "coverage: an OK pixel clamped to 0": (cov("ok_clamped"), 1),
        "coverage: a not-OK pixel saturated at 1": (cov("saturated"), 1),
        "coverage: an inert pair whose triangle has area": (cov("inert_area"), 1),
        "coverage, either pass: a backward face with non-finite terms": (n(lambda s: s["cov_bad"] + s["cov_bad_altered"] > 0), 1),
        "coverage, poisoned vertices: a non-finite area under a border pixel": (cov("bad_area", "cov_vertex"), 1),
        "coverage, poisoned vertices: a poisoned triangle with a live pair": (cov("live_marked", "cov_vertex"), 1),
        "coverage: a tie on s in (0, 1) on a rendered scene (none is needed: the pass below)": (n(lambda s: s["cov_open_ties"] > 0), 0),
        "coverage, vertices on a segment: a tie on s in (0, 1) whose terms count": (n(lambda s: s["cov_telling_ties"] > 0), 1),
        "coverage, altered pass: an OK pixel beside one that is not OK by a bad id alone": (n(lambda s: s["bad_id_beside_ok"] > 0), 1),
        "coverage, altered pass: a pixel covered (>= 0) and not OK": (n(lambda s: s["covered_not_ok"] > 0), 1),
        "albedo fit: a face with a non-finite moment": (n(lambda s: s["albedo"][0] > 0), 1),
        "albedo fit: a face with finite moments and at least K + 1 counted pixels": (n(lambda s: s["albedo"][1] > 0), 1),
    })
    for name in RPR.BRANCHES:
        if not name.startswith("clamped"):
            out["photo_loss_rgb: " + name] = (n(lambda s: s["branches_rgb"][name]), 1)
    for k in range(3):
        out["background_rgb kind %d" % k] = (n(lambda s: s["bg_kind"] == k), 1)
    for K in FS.ALBEDO_K:
        out["albedo fit: K == %d" % K] = (n(lambda s: s["K"] == K), 1)
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
    assert not any(s["branches_rgb"]["clamped %d" % ch] for s in stats for ch in range(3))
    rgb = RPR.branches(planes[1], planes[2], planes[3], c.light_rgb, c.weight)
    assert tuple(rgb) == RPR.BRANCHES and all(rgb.values()), rgb             # with the scene's own colour lights, of both signs
    assert (planes[3] >= 0).any() and not (planes[3] >= 0).all()


def test_vertex_altered_poisons_border_triangles_and_nothing_else(oracle):
    """up to four different triangles that own an OK pixel beside a not-OK one, one coordinate each; the case itself is untouched"""
    for i in (0, 3, 10, 25):
        c = FS.ConsumerCase(i)
        tind = oracle.render_depth(c.ver, c.tri, c.tex, c.H, c.W)[3].reshape(c.B, -1)
        before = c.ver.copy()
        v = c.vertex_altered(tind)
        assert c.ver.tobytes() == before.tobytes() and v.tri is c.tri and v.g_cov is c.g_cov
        owners = set()
        for b in range(c.B):
            okt, _ = RC.ok_triangles(c.tri, tind[b], c.nver)
            border = RC._border(okt, c.H, c.W)
            owners |= {(b, int(t)) for t in okt[border] if t >= 0}
        assert len(v.poisoned) == (4 if owners else 0)
        assert all((b, t) in owners and vid in RN.f2i_x86(c.tri[:, t]) and row in (0, 1) for b, t, vid, row, _ in v.poisoned)
        assert len({t for _, t, _, _, _ in v.poisoned}) == min(4, len({t for _, t in owners}))
        changed = np.argwhere(v.ver.view(np.uint32) != before.view(np.uint32))
        assert {tuple(x) for x in changed} <= {(b, row, vid) for b, _, vid, row, _ in v.poisoned}
        last = {(b, row, vid): val for b, _, vid, row, val in v.poisoned}      # (a vertex drawn twice holds the later value)
        for (b, row, vid), val in last.items():
            assert np.array_equal(v.ver[b, row, vid], np.float32(val), equal_nan=True)


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
