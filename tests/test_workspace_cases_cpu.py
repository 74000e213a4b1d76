"""CPU: the table of caller-owned buffers (tests/workspace_cases.py) is complete, its "ragged" shapes are ragged against each entry's own
launch geometry, its inputs are not vacuous on the CPU references, and the two comparison helpers of
tests/test_workspace_contract_gpu.py can fail."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
import workspace_cases as WC

CASES = sorted(WC.CASES)


def _declared():
    with open(os.path.join(ROOT, "include", "fr_hotpath.h")) as f:
        return sorted(set(re.findall(r"size_t (fr_\w+_bytes)\(", f.read())))


def test_every_size_function_of_the_header_is_in_the_table():
    declared = _declared()
    assert len(declared) >= 31
    covered = {c.size_fn for c in WC.CASES.values()}
    assert covered <= set(declared), sorted(covered - set(declared))
    for name, reason in WC.EXCLUDED.items():
        assert name in declared and name not in covered, name
        assert isinstance(reason, str) and reason.strip(), "%s is excluded without a reason" % name
    missing = [n for n in declared if n not in covered and n not in WC.EXCLUDED]
    assert not missing, "size functions with neither a case nor a reason in workspace_cases.EXCLUDED: %s" % missing


def test_every_entry_point_that_takes_a_sized_buffer_is_named_by_a_case():
    sigs = pkg("_lib").SIGNATURES
    sized = sorted(n for n, s in sigs.items() if s.startswith("i:") and "z" in s.split(":")[1])
    assert len(sized) >= 45
    named = {"fr_" + tok for name in WC.CASES for tok in re.findall(r"[a-z0-9_]+", name)} & set(sigs)
    for name, reason in WC.UNCASED.items():
        assert name in sized and name not in named, name
        assert isinstance(reason, str) and reason.strip(), "%s is listed without a reason" % name
    missing = [n for n in sized if n not in named and n not in WC.UNCASED]
    assert not missing, "entry points with a sized buffer and neither a case nor a reason in workspace_cases.UNCASED: %s" % missing


def test_the_built_buffers_are_checked_through_their_consumers():
    built = ("fr_decode_packed_basis_bytes", "fr_decode_backward_basis_bytes", "fr_decode_q30_image_bytes", "fr_decode_render_vertex_bytes",
             "fr_geometry_gram_bytes", "fr_albedo_basis_bytes", "fr_albedo_basis_rgb_bytes", "fr_landmark_basis_bytes", "fr_sfs_moments_bytes",
             "fr_sfs_q_bytes")
    for fn in built:
        names = [c.name for c in WC.CASES.values() if c.size_fn == fn]
        assert names and all("->" in n or "hand-off" in n for n in names), (fn, names)


@pytest.mark.parametrize("name", CASES)
def test_sizes_alignment_and_raggedness(name):
    c = WC.CASES[name]
    assert c.align in (16, 128, 256)
    for shape in WC.SHAPES + ("large",):
        n = c.nbytes(shape)
        assert n > 0, (name, shape)
        assert n % 4 == 0, (name, shape, n)
    held = c.ragged("ragged")
    assert held, name
    for what, ok in held:
        assert ok, "%s: the ragged shape is even in '%s'" % (name, what)
    if c.other is not None:
        other, oshape = c.other
        assert other in WC.CASES and oshape in WC.DIM and WC.CASES[other].align == c.align, (name, c.other)


@pytest.mark.parametrize("name", [n for n in CASES if WC.CASES[n].cover is not None and "decode_render_backward" not in n])
def test_inputs_cover_the_image_on_the_cpu_reference(name):
    """(the two fused backwards render their own scene on the GPU: the GPU test holds their coverage)"""
    for shape in WC.SHAPES:
        cov = WC.CASES[name].cover(shape)
        assert 0.30 <= cov < 1.0, (name, shape, cov)


def test_reference_solves_succeed_on_every_unit():
    import ref_albedo_lse as RA
    import ref_photo_solve_rgb as RS
    for shape in WC.SHAPES:
        for K in (1, 9, 15):
            a = WC.albedo_inputs(shape, K)
            stats = RA.fit_ref(a["basis"], a["tri_ind"], a["lighting"], a["normal"], a["abedo"], a["im_gray"], 1e-6)[1]
            assert (stats[:, 3] == 1.0).all(), (shape, K, stats[:, 3])
            s = WC.solve_inputs(shape, K)
            light = RS.light_fit_ref(s["tex"], s["normal"], s["tri_ind"], s["target"])
            alb = RS.albedo_fit_ref(s["basis"], s["tri_ind"], s["normal"], s["light"], s["target"], ridge=1e-6)
            for got in (light, alb):
                st = got[1]
                assert (st[..., 3] == 1.0).all(), (shape, K, st[..., 3])


def test_the_sfs_batches_are_the_smallest_the_reference_model_accepts():
    """tests/ref_sfs.py::inputs asserts the model's eigenvalue-gap condition, which the imported SfS bounds need: it accepts the table's
    three batches, and at the issue's three faces of 17 x 31 it accepts no seed (every draw has a nearly singular pixel)"""
    import ref_sfs as RS
    for shape in WC.DIM:
        d, g = WC.sfs_inputs(shape)
        m = RS.model(*RS.args(d))
        RS.check_gap(m.lam)
        assert np.isfinite(m.intensity).all() and m.intensity.any() and g.any()
    (B, H, W), _ = WC.SFS["ragged"]
    assert (B, H, W) == (9, 17, 31)
    for seed in range(1, 9):
        with pytest.raises(AssertionError, match="gap condition"):
            RS.inputs(3, H, W, seed=seed)


def test_reference_planes_are_finite_and_not_zero():
    import ref_fine_losses as RF
    import ref_photo_loss as RP
    for shape in WC.SHAPES:
        sc = WC.scene(shape)
        for k in ("tex_img", "normal", "tind"):
            assert np.isfinite(sc[k]).all() and sc[k].any(), (shape, k)
        B, H, W = sc["B"], sc["H"], sc["W"]
        z, c, _ = RF.inputs(B, H, W)
        want = RF.forward(z, c)
        assert np.isfinite(want["S_f"]) and want["S_f"] > 0 and want["S_s"] > 0
        p = RP.hand_planes(B, H, W, seed=5 + H)
        sums = RP.forward(*p[:5], p[5], 1.75, -0.125)
        assert np.isfinite(sums).all() and (sums[:, 1] > 0).all()


# ---- the comparison helpers can fail ---------------------------------------------------------------------------------------------------
def test_the_bit_comparator_reports_a_one_bit_difference():
    a = {"x": torch.arange(12, dtype=torch.float32).reshape(3, 4), "s": torch.tensor([1.5, -0.0], dtype=torch.float64)}
    b = {k: v.clone() for k, v in a.items()}
    assert WC.bit_difference(a, b) is None
    b["x"].view(torch.int32)[2, 1] ^= 1                                      # the last mantissa bit of one element
    assert "x: 1 of 12" in WC.bit_difference(a, b)
    b = {k: v.clone() for k, v in a.items()}
    b["s"][1] = 0.0                                                          # +0 against -0: equal under ==, not as bits
    assert bool((a["s"] == b["s"]).all()) and "s: 1 of 2" in WC.bit_difference(a, b)
    n1, n2 = np.array([np.nan], np.float32), np.array([np.nan], np.float32)
    n2.view(np.uint32)[0] ^= 1                                               # another NaN payload
    assert WC.bit_difference({"n": n1}, {"n": n1.copy()}) is None and WC.bit_difference({"n": n1}, {"n": n2}) is not None
    assert WC.bit_difference({"x": a["x"]}, {"x": a["x"].double()}) is not None          # another type
    assert WC.bit_difference({"x": a["x"]}, {"y": a["x"]}) is not None                   # another set of outputs


@pytest.mark.parametrize("align", [16, 128, 256])
def test_the_guard_checker_reports_one_flipped_byte_on_either_side(align):
    nbytes = 1000
    whole, off = WC.place(nbytes, align, device="cpu")
    addr = whole.data_ptr() + off
    assert addr % align == 0 and addr % (2 * align) != 0
    whole[off:off + nbytes] = 0xFF                                           # the buffer itself is the call's to write
    assert WC.guard_damage(whole, off, nbytes) is None
    for at, side in ((off - 1, "before"), (off - WC.GUARD, "before"), (off + nbytes, "behind"), (off + nbytes + WC.GUARD - 1, "behind")):
        whole[at] ^= 1
        msg = WC.guard_damage(whole, off, nbytes)
        assert msg is not None and side in msg, (at, msg)
        whole[at] ^= 1
    assert WC.guard_damage(whole, off, nbytes) is None
