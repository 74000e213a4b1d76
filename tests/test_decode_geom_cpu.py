"""CPU: the decode forward's launch decision (fr_debug_decode_geom: the function fr_launch_decode itself calls) and its work
distribution (fr_debug_decode_walk: the wave_work / tile_walk the kernels call, evaluated on the host).

  * every geometry the launcher can choose -- all FR_DECODE_* knobs, the ring shape and generic shapes, B = 1 .. 200, the model's
    N and small ones, parts of 1 .. 256 compute units -- deals every work item (tile, half) to EXACTLY one wave;
  * the documented boundaries of the decision (the comments of decode_plan_pass in csrc/fr_decode.hip) are what it returns;
  * the same for the Q30 decode (fr_debug_decode_q_geom: the function fr_launch_decode_q calls) and its slot shapes."""
import ctypes

import numpy as np
import pytest

from conftest import pkg

PASS_INTS = 12
FIELDS = ("b0", "cols", "kernel", "nbw", "waves", "mb", "halves", "nt", "prio", "tr", "lds", "grid")
GENERIC, RING = 0, 1
N_MODEL = 53215
KNOBS = [{}, {"FR_DECODE_NT": 0}, {"FR_DECODE_NT": 1}, {"FR_DECODE_NBW": 1}, {"FR_DECODE_NBW": 4}, {"FR_DECODE_WAVES": 8},
         {"FR_DECODE_IMPL": 1}, {"FR_DECODE_WIDE": 0}, {"FR_DECODE_STORE": 1},
         {"FR_DECODE_NBW": 1, "FR_DECODE_WIDE": 0}, {"FR_DECODE_NBW": 4, "FR_DECODE_WIDE": 0},
         {"FR_DECODE_NBW": 1, "FR_DECODE_IMPL": 1}, {"FR_DECODE_NBW": 4, "FR_DECODE_IMPL": 1},
         {"FR_DECODE_WAVES": 8, "FR_DECODE_WIDE": 0}, {"FR_DECODE_STORE": 1, "FR_DECODE_WIDE": 0}]
SHAPES = [(199, 29), (200, 17), (33, 16), (9, 5), (0, 0), (300, 100)]
CUS = (1, 7, 8, 9, 64, 256)


def _h():
    return pkg("_lib")


def geom(B, N, ns, ne, cus):
    """[{field: value} per pass] from fr_debug_decode_geom under the current knobs"""
    out = (ctypes.c_int * (1 + PASS_INTS * ((B + 63) // 64 + 1)))()
    rc = _h().lib().fr_debug_decode_geom(B, N, ns, ne, cus, out)
    assert rc == 0, rc
    return [dict(zip(FIELDS, out[1 + PASS_INTS * i:1 + PASS_INTS * (i + 1)])) for i in range(out[0])]


def walk(tiles, waves, halves, grid):
    v = np.zeros(tiles * halves, np.int32)
    rc = _h().lib().fr_debug_decode_walk(tiles, waves, halves, grid, v.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == 0, rc
    return v.reshape(tiles, halves)


def test_every_launch_geometry_visits_every_item_exactly_once():
    L = _h().lib()
    out = (ctypes.c_int * (1 + PASS_INTS * 5))()
    I_COLS, I_NBW, I_WAVES, I_MB, I_HALVES, I_GRID = (FIELDS.index(f) for f in ("cols", "nbw", "waves", "mb", "halves", "grid"))
    seen = {}
    for knobs in KNOBS:
        with _h().options(**knobs):
            for ns, ne in SHAPES:
                for N in (N_MODEL, 4100, 99, 15):
                    tiles = (N + 15) // 16
                    for cus in CUS:
                        for B in range(1, 201):
                            assert L.fr_debug_decode_geom(B, N, ns, ne, cus, out) == 0
                            b0 = 0
                            for i in range(out[0]):
                                p = out[1 + PASS_INTS * i:1 + PASS_INTS * (i + 1)]
                                cols, nbw, waves, mb, halves, grid = p[I_COLS], p[I_NBW], p[I_WAVES], p[I_MB], p[I_HALVES], p[I_GRID]
                                slots = waves // max(halves, 1)
                                # the passes tile the batch (consecutive, mb columns each, the last one ragged); a pass's halves x NBW
                                # column blocks cover its live columns with less than one item to spare; the grid is one workgroup
                                # per compute unit, or fewer when the tiles run out first
                                if not (p[0] == b0 and cols == min(B - b0, mb) and halves * nbw * 16 >= cols > (halves - 1) * nbw * 16
                                        and slots >= 1 and grid == min(cus, (tiles + slots - 1) // slots)):
                                    raise AssertionError((knobs, ns, ne, N, cus, B, dict(zip(FIELDS, p))))
                                b0 += mb
                                seen.setdefault((tiles, waves, halves, grid), (knobs, ns, ne, N, cus, B))
                            assert b0 >= B
    assert any(k[1] == 16 and k[2] == 3 for k in seen)       # FR_DECODE_NBW=1 at 33-48 columns: a surplus wave
    assert any(k[1] == 12 and k[2] == 2 for k in seen) and any(k[1] == 12 and k[2] == 1 for k in seen)
    assert any(k[1] == 8 for k in seen) and any(k[2] == 4 for k in seen)
    assert any(k[3] % 8 == 0 and k[3] > 8 for k in seen) and any(k[3] % 8 for k in seen)
    for (tiles, waves, halves, grid), first in sorted(seen.items()):
        v = walk(tiles, waves, halves, grid)
        assert v.min() == 1 and v.max() == 1, \
            "tiles %d, %d waves, %d halves, %d workgroups (first reached by %r): visits %d .. %d, %d items not taken once" % (
                tiles, waves, halves, grid, first, v.min(), v.max(), int((v != 1).sum()))


def test_walk_is_exact_for_every_small_launch():
    """beyond what the launcher picks today: every (waves, halves) a kernel exists for, every grid up to 40, ragged tile counts"""
    for waves, halves in ((16, 1), (16, 2), (16, 3), (16, 4), (12, 1), (12, 2), (8, 1), (8, 2)):
        for grid in range(1, 41):
            for tiles in (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 257, 1000):
                v = walk(tiles, waves, halves, grid)
                assert (v == 1).all(), (waves, halves, grid, tiles)


def test_walk_rejects_bad_arguments():
    L = _h().lib()
    v = (ctypes.c_int * 64)()
    assert L.fr_debug_decode_walk(-1, 16, 2, 4, v) == -1
    assert L.fr_debug_decode_walk(4, 16, 0, 4, v) == -1
    assert L.fr_debug_decode_walk(4, 2, 3, 4, v) == -1
    assert L.fr_debug_decode_walk(4, 16, 2, 0, v) == -1
    assert L.fr_debug_decode_walk(4, 16, 2, 4, None) == -1
    assert L.fr_debug_decode_walk(0, 16, 2, 4, None) == 0


def _one(B, ns=199, ne=29, N=N_MODEL, cus=256):
    g = geom(B, N, ns, ne, cus)
    return g


LDS64 = 15 * 16 * 16 * 16 + 64 * 12 * 4 + 64 * 3 * 2 * 8           # 13 + 2 groups, 64 columns
LDS128 = 15 * 16 * 32 * 16 + 128 * 12 * 4 + 128 * 3 * 2 * 8         # ... 128 columns


def _is(p, **kv):
    assert {k: p[k] for k in kv} == kv, p


@pytest.mark.parametrize("ns,ne", [(199, 29), (200, 17)], ids=["199+29", "200+17"])
def test_documented_boundaries_ring_shape(ns, ne):
    """13 + 2 groups (reached by 199 + 29 and by 200 + 17), default knobs, the model's N on 256 compute units"""
    host = _h()
    assert all(host.get_option(k) == d for k, d in (("FR_DECODE_IMPL", 0), ("FR_DECODE_WIDE", 1), ("FR_DECODE_NBW", 0),
                                                    ("FR_DECODE_WAVES", 16), ("FR_DECODE_NT", -1), ("FR_DECODE_STORE", 0)))
    tiles = (N_MODEL + 15) // 16
    (p,) = _one(16, ns, ne)      # one column block: 16-column items, non-temporal stream, equal priorities
    _is(p, b0=0, cols=16, kernel=RING, nbw=1, waves=16, mb=64, halves=1, nt=1, prio=0, tr=0, lds=LDS64, grid=(tiles + 15) // 16)
    (p,) = _one(17, ns, ne)      # two blocks in one item; below 64 faces the default cache policy, ranked waves
    _is(p, cols=17, kernel=RING, nbw=2, waves=16, mb=64, halves=1, nt=0, prio=1, tr=0, lds=LDS64, grid=(tiles + 15) // 16)
    (p,) = _one(32, ns, ne)
    _is(p, cols=32, kernel=RING, nbw=2, halves=1, nt=0, prio=1)
    (p,) = _one(33, ns, ne)      # three blocks: two items per tile, eight tiles per workgroup
    _is(p, cols=33, kernel=RING, nbw=2, waves=16, halves=2, nt=0, prio=1, grid=256)
    (p,) = _one(63, ns, ne)
    _is(p, cols=63, nbw=2, halves=2, nt=0, prio=1)
    (p,) = _one(64, ns, ne)      # the benchmarked pass: non-temporal stream
    _is(p, cols=64, kernel=RING, nbw=2, waves=16, mb=64, halves=2, nt=1, prio=1, tr=0, lds=LDS64, grid=256)
    (p,) = _one(65, ns, ne)      # more than 64 remain: one 128-column pass on 12 waves
    _is(p, b0=0, cols=65, kernel=RING, nbw=4, waves=12, mb=128, halves=2, nt=0, prio=0, tr=0, lds=LDS128, grid=256)
    (p,) = _one(128, ns, ne)
    _is(p, cols=128, nbw=4, waves=12, mb=128, halves=2)
    p, q = _one(129, ns, ne)     # ... and a pass of one face
    _is(p, b0=0, cols=128, mb=128)
    _is(q, b0=128, cols=1, kernel=RING, nbw=1, waves=16, mb=64, halves=1, nt=1)
    p, q = _one(192, ns, ne)     # exactly 64 remain: not wide
    _is(p, b0=0, cols=128, mb=128)
    _is(q, b0=128, cols=64, nbw=2, waves=16, mb=64, halves=2, nt=1, prio=1)
    p, q = _one(193, ns, ne)
    _is(p, b0=0, cols=128, mb=128)
    _is(q, b0=128, cols=65, nbw=4, waves=12, mb=128, halves=2)
    # the knobs
    with host.options(FR_DECODE_STORE=1):
        (p,) = _one(64, ns, ne)
        _is(p, kernel=RING, nbw=2, nt=1, prio=1, tr=1)
        (p,) = _one(63, ns, ne)  # (the default cache policy of a short pass comes first)
        _is(p, tr=0, nt=0)
    with host.options(FR_DECODE_NT=1):
        (p,) = _one(17, ns, ne)
        _is(p, nt=1, prio=1, tr=0)
    with host.options(FR_DECODE_NT=0):
        (p,) = _one(64, ns, ne)
        _is(p, nt=0, prio=1, tr=0)
    with host.options(FR_DECODE_WAVES=8):
        (p,) = _one(64, ns, ne)
        _is(p, kernel=RING, nbw=2, waves=8, halves=2, nt=0, prio=0, grid=256)
    with host.options(FR_DECODE_WIDE=0):
        p, q = _one(70, ns, ne)
        _is(p, cols=64, mb=64, nbw=2, halves=2)
        _is(q, b0=64, cols=6, mb=64, nbw=1, halves=1)
    with host.options(FR_DECODE_NBW=1):
        for B, halves in ((16, 1), (17, 2), (32, 2), (33, 3), (48, 3), (49, 4), (64, 4)):
            (p,) = _one(B, ns, ne)
            _is(p, kernel=RING, nbw=1, waves=16, halves=halves, nt=1, prio=0, grid=min(256, -(-tiles // (16 // halves))))
    with host.options(FR_DECODE_NBW=4):     # the ring schedule has no 4-block form at 64 columns: the generic kernel on 12 waves
        (p,) = _one(64, ns, ne)
        _is(p, kernel=GENERIC, nbw=4, waves=12, mb=64, halves=1, grid=256)
        (p,) = _one(32, ns, ne)
        _is(p, kernel=RING, nbw=2, waves=16, halves=1)
        (p,) = _one(33, ns, ne)
        _is(p, kernel=GENERIC, nbw=4, waves=12, halves=1)
    with host.options(FR_DECODE_IMPL=1):
        p, q = _one(70, ns, ne)
        _is(p, kernel=GENERIC, nbw=2, waves=16, mb=64, halves=2, cols=64)
        _is(q, kernel=GENERIC, nbw=1, waves=16, halves=1, cols=6)


def test_documented_boundaries_generic_shape():
    lds = 4 * 16 * 16 * 16 + 64 * 12 * 4 + 64 * 3 * 2 * 8            # 33 + 16 coefficients: 3 + 1 groups
    for B, nbw, halves in ((16, 1, 1), (17, 2, 1), (32, 2, 1), (33, 2, 2), (64, 2, 2)):
        (p,) = _one(B, 33, 16, N=1000, cus=256)
        _is(p, b0=0, cols=B, kernel=GENERIC, nbw=nbw, waves=16, mb=64, halves=halves, nt=0, prio=0, tr=0, lds=lds,
            grid=-(-63 // (16 // halves)))
    for B in (65, 128, 129, 192, 193):           # never wide: 64 columns per pass
        g = _one(B, 33, 16, N=1000)
        assert [p["b0"] for p in g] == list(range(0, B, 64)) and all(p["mb"] == 64 and p["kernel"] == GENERIC for p in g)
        assert g[-1]["cols"] == B - 64 * (len(g) - 1)
    (p,) = _one(4, 0, 0, N=48)                   # no basis at all
    _is(p, kernel=GENERIC, nbw=1, halves=1, lds=64 * 12 * 4 + 64 * 3 * 2 * 8, grid=1)


def test_unsupported_and_invalid():
    L = _h().lib()
    out = (ctypes.c_int * 64)()
    # the 64-column LDS image: 4 KiB per 16-coefficient group + 6 KiB -- 38 groups fit 160 KiB, 39 do not
    assert L.fr_debug_decode_geom(4, 100, 16 * 38, 0, 256, out) == 0 and out[0] == 1 and out[1 + 10] == 38 * 4096 + 6144
    assert L.fr_debug_decode_geom(4, 100, 16 * 38 + 1, 0, 256, out) == -4 and out[0] == 0
    assert L.fr_debug_decode_geom(4, 100, 16 * 20, 16 * 19, 256, out) == -4
    assert L.fr_debug_decode_geom(0, 100, 5, 3, 256, out) == 0 and out[0] == 0
    assert L.fr_debug_decode_geom(4, 0, 5, 3, 256, out) == 0 and out[0] == 0
    assert L.fr_debug_decode_geom(-1, 100, 5, 3, 256, out) == -1
    assert L.fr_debug_decode_geom(4, 100, 5, -3, 256, out) == -1
    assert L.fr_debug_decode_geom(4, 100, 5, 3, 0, out) == -1
    assert L.fr_debug_decode_geom(4, 100, 5, 3, 256, None) == -1


# ---- the Q30 decode's launch decision (fr_debug_decode_q_geom: the function fr_launch_decode_q itself calls) ----------------------
Q_INTS = 10
Q_FIELDS = ("b0", "cols", "kernel", "nbw", "waves", "h2", "ring", "launches", "lds", "grid")
Q_SLOT_SHAPES = ((8, 1), (16, 2), (12, 2))          # (waves, waves that share a tile) of the ring kernel's instantiations
Q_GRIDS = (1, 2, 3, 7, 8, 16, 256)
Q_STAGE = 4 * 16384 + 64 * 12 * 4 + 64 * 4          # staged parameter image of a 4-k-step shape


def qgeom(B, N, ns, ne, levels, cus=256):
    out = (ctypes.c_int * (1 + Q_INTS * ((B + 63) // 64 + 1)))()
    rc = _h().lib().fr_debug_decode_q_geom(B, N, ns, ne, levels, cus, out)
    assert rc == 0, rc
    return [dict(zip(Q_FIELDS, out[1 + Q_INTS * i:1 + Q_INTS * (i + 1)])) for i in range(out[0])]


def test_walk_is_exact_for_the_q30_slot_shapes():
    """every tile is taken by exactly one slot (and by each of the waves that share it) at the grids a capped part gives and at the
    full part, at tile counts around each multiple of slots x grid: a full last round, one tile short of it, one tile into the next"""
    for waves, h2 in Q_SLOT_SHAPES:
        slots = waves // h2
        for grid in Q_GRIDS:
            per_round = slots * grid
            for tiles in sorted({max(m * per_round + d, 0) for m in range(0, 4) for d in (-1, 0, 1)} | {1, slots - 1, slots, slots + 1}):
                v = walk(tiles, waves, h2, grid)
                assert v.shape == (tiles, h2) and (v == 1).all(), (waves, h2, grid, tiles)


def test_q30_geom_is_consistent_at_every_batch_and_knob():
    host = _h()
    seen = set()
    for knobs in ({}, {"FR_Q30_SCHED": 1}, {"FR_DECODE_IMPL": 1}, {"FR_DECODE_IMPL": 1, "FR_Q30_SCHED": 1}):
        with host.options(**knobs):
            for ns, ne in ((199, 29), (225, 0), (211, 29), (0, 230), (200, 24), (212, 29), (33, 16), (0, 0), (512, 0)):
                KB = max((ns + ne + 15) // 16, 1)
                S = (KB + 3) // 4
                for lv in (7, 5, 4):
                    for N in (N_MODEL, 700, 15):
                        tiles = (N + 15) // 16
                        for cus in (1, 8, 256):
                            for B in list(range(1, 131, 3)) + [16, 17, 32, 33, 48, 49, 64, 65, 128, 129, 192, 193]:
                                g = qgeom(B, N, ns, ne, lv, cus)
                                assert [p["b0"] for p in g] == list(range(0, B, 64))
                                for p in g:
                                    what = (knobs, ns, ne, lv, N, cus, B, p)
                                    nbt = (p["cols"] + 15) // 16
                                    ring = KB == 15 and not knobs.get("FR_DECODE_IMPL")
                                    assert p["cols"] == min(B - p["b0"], 64) and p["kernel"] == int(ring), what
                                    # the pass's column blocks are covered: by one wave, by the two waves of a pair, or by two launches
                                    assert p["nbw"] * p["h2"] * p["launches"] * 16 >= p["cols"], what
                                    slots = p["waves"] // p["h2"]
                                    assert p["grid"] == min(cus, -(-tiles // slots)), what
                                    if ring:
                                        halves = knobs.get("FR_Q30_SCHED") == 1 and nbt >= 3
                                        assert p["h2"] == (2 if halves else 1) and p["launches"] == 1, what
                                        assert p["nbw"] == (2 if halves else {1: 1, 2: 2, 3: 4, 4: 4}[nbt]), what
                                        assert p["waves"] == ((12 if lv == 7 else 16) if halves else 8), what
                                        assert p["ring"] == (8 if halves else 16), what
                                        assert p["lds"] == Q_STAGE + p["waves"] * 256 + p["waves"] * 2 * p["nbw"] * 1024, what
                                    else:
                                        assert (p["nbw"], p["launches"]) == {1: (1, 1), 2: (2, 1), 3: (2, 2), 4: (2, 2)}[nbt], what
                                        assert p["waves"] == 8 and p["h2"] == 1 and p["ring"] == 0, what
                                        assert p["lds"] == S * 16384 + 64 * 12 * 4 + 64 * 4, what
                                    assert p["lds"] <= 160 * 1024, what
                                    seen.add((p["kernel"], p["nbw"], p["waves"], p["h2"], p["launches"]))
    assert seen == {(1, 1, 8, 1, 1), (1, 2, 8, 1, 1), (1, 4, 8, 1, 1), (1, 2, 12, 2, 1), (1, 2, 16, 2, 1),
                    (0, 1, 8, 1, 1), (0, 2, 8, 1, 1), (0, 2, 8, 1, 2)}, seen
    # every reported (waves, h2) is a slot shape whose walk the test above holds exact
    assert {(w, h) for _, _, w, h, _ in seen} == set(Q_SLOT_SHAPES)


def test_q30_geom_documented_boundaries():
    """the model's shape and N on 256 compute units: a wave first takes a second tile where ceil(tiles / slots) passes the grid"""
    host = _h()
    assert host.get_option("FR_Q30_SCHED") == 0 and host.get_option("FR_DECODE_IMPL") == 0 and host.get_option("FR_DECODE_CUS") == 0
    (p,) = qgeom(64, N_MODEL, 199, 29, 4)
    _is(p, b0=0, cols=64, kernel=RING, nbw=4, waves=8, h2=1, ring=16, launches=1, grid=256)
    (p,) = qgeom(64, 256 * 8 * 16, 199, 29, 7)        # 2,048 tiles: exactly one per wave
    assert p["grid"] == 256
    (p,) = qgeom(64, 256 * 8 * 16 - 16, 199, 29, 7)   # one tile fewer: still 256 workgroups (the last one short of a wave)
    assert p["grid"] == 256
    (p,) = qgeom(64, 255 * 8 * 16, 199, 29, 7)
    assert p["grid"] == 255
    with host.options(FR_Q30_SCHED=1):
        (p,) = qgeom(64, N_MODEL, 199, 29, 7)
        _is(p, kernel=RING, nbw=2, waves=12, h2=2, ring=8, grid=256)
        (p,) = qgeom(64, N_MODEL, 199, 29, 5)
        _is(p, kernel=RING, nbw=2, waves=16, h2=2, ring=8, grid=256)
        (p,) = qgeom(32, N_MODEL, 199, 29, 7)         # two live blocks: the whole-tile schedule
        _is(p, kernel=RING, nbw=2, waves=8, h2=1, ring=16)
        p, q = qgeom(97, N_MODEL, 199, 29, 4)         # 33 columns in the second pass: a half-dead pair
        _is(q, b0=64, cols=33, nbw=2, waves=16, h2=2)
    for ns, ne, kernel in ((225, 0, RING), (211, 29, RING), (0, 230, RING), (240, 0, RING), (200, 24, GENERIC), (212, 29, GENERIC)):
        (p,) = qgeom(20, 1000, ns, ne, 7)
        assert p["kernel"] == kernel, (ns, ne, p)
    with host.options(FR_DECODE_IMPL=1):
        (p,) = qgeom(64, N_MODEL, 199, 29, 7)
        _is(p, kernel=GENERIC, nbw=2, waves=8, h2=1, ring=0, launches=2, lds=Q_STAGE, grid=256)


def test_q30_geom_unsupported_and_invalid():
    L = _h().lib()
    out = (ctypes.c_int * 64)()
    assert L.fr_debug_decode_q_geom(4, 100, 512, 0, 7, 256, out) == 0 and out[0] == 1 and out[1 + 8] == 8 * 16384 + 3328
    assert L.fr_debug_decode_q_geom(4, 100, 513, 0, 7, 256, out) == -4 and out[0] == 0
    assert L.fr_debug_decode_q_geom(4, 100, 500, 13, 4, 256, out) == -4
    assert L.fr_debug_decode_q_geom(0, 100, 5, 3, 7, 256, out) == 0 and out[0] == 0
    assert L.fr_debug_decode_q_geom(4, 0, 5, 3, 7, 256, out) == 0 and out[0] == 0
    for lv in (0, 1, 3, 6, 8, -7):
        assert L.fr_debug_decode_q_geom(4, 100, 5, 3, lv, 256, out) == -1
    assert L.fr_debug_decode_q_geom(-1, 100, 5, 3, 7, 256, out) == -1
    assert L.fr_debug_decode_q_geom(4, -1, 5, 3, 7, 256, out) == -1
    assert L.fr_debug_decode_q_geom(4, 100, 5, -3, 7, 256, out) == -1
    assert L.fr_debug_decode_q_geom(4, 100, 5, 3, 7, 0, out) == -1
    assert L.fr_debug_decode_q_geom(4, 100, 5, 3, 7, 256, None) == -1
