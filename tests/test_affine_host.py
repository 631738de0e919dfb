"""Host half of the affine pin (no GPU): the cases of ``tests/affine_cases.py`` reach what they aim at (a census from the exported
launch plan, ``lsr_affine_plan``), the source box each LDS-staged kernel sizes holds every tap it reads (both coverage claims, in
numpy, at the designed thresholds and on random maps), and ``lsr_affine_f32_cpu`` == the restatement (``tests/affine_ref.py``) ==
scipy, bit for bit, on every case.  ``tests/test_affine_edges_gpu.py`` holds the three kernels to the same arrays.
"""

import collections
import functools

import numpy as np
import pytest

from shrimpy_amd import _lib
from tests import affine_cases as C
from tests import affine_ref as R

MODES = R.MODES


def _planar_names():
    return [n for n in C.CASES if C.case(n).path == 1 and not C.case(n).in_pitch]


# ---- the twin ---------------------------------------------------------------------------------------------------------------------


def run_twin(name, mode, threads=1):
    c = C.case(name)
    src = np.ascontiguousarray(C.source(name))
    out = np.full(c.out_shape, np.float32(np.nan), dtype=np.float32)
    _lib.call("lsr_set_host_threads", int(threads))
    try:
        _lib.call("lsr_affine_f32_cpu", src.ctypes.data, *c.shape, out.ctypes.data, *c.out_shape, _lib.matrix12(c.m), float(c.cval),
                  C.MODE_CODE[mode], None)
    finally:
        _lib.call("lsr_set_host_threads", 1)
    return out


@functools.lru_cache(maxsize=None)
def case_twin(name, mode):
    out = run_twin(name, mode)
    out.setflags(write=False)
    return out


def check(got, name, mode, what):
    want = C.expected(name, mode).out
    assert R.same_bits(got, want), f"{name} [{mode}]: {what} differs from the restatement: {R.describe_difference(got, want)}"


@pytest.mark.parametrize("g", C.GROUPS)
def test_twin_equals_the_restatement_bit_for_bit(g):
    for name in C.group(g):
        for mode in MODES:
            check(case_twin(name, mode), name, mode, "lsr_affine_f32_cpu")


def test_twin_on_three_threads_gives_the_same_bits():
    for g in C.GROUPS:
        for name in C.group(g):
            for mode in MODES:
                check(run_twin(name, mode, threads=3), name, mode, "lsr_affine_f32_cpu on 3 threads")


@pytest.mark.parametrize("g", C.GROUPS)
def test_restatement_equals_scipy_bit_for_bit(g):
    from scipy import ndimage

    checked = 0
    for name in C.group(g):
        if not C.is_finite(name):
            continue
        c = C.case(name)
        m = np.array(c.m).reshape(3, 4)
        for mode in MODES:
            with np.errstate(all="ignore"):
                want = ndimage.affine_transform(C.source(name), m[:, :3], offset=m[:, 3], output_shape=c.out_shape, order=1, mode=mode,
                                                cval=c.cval, prefilter=False, output=np.float32)
            got = C.expected(name, mode).out
            assert R.same_bits(got, want), f"{name} [{mode}]: {R.describe_difference(got, want)}"
            checked += 1
    assert checked


def test_non_finite_cases_have_no_voxel_on_the_last_index_and_spread_no_further_than_their_taps():
    """The rule of the header: the LDS-staged kernels read the upper neighbour of a coordinate exactly on ``n - 1`` from a staged
    duplicate (weight 0), so a non-finite volume is compared there only where no coordinate is on ``n - 1``: the cases count zero
    such voxels, nothing is left out.  A NaN or an infinity reaches exactly the voxels one of whose eight taps holds it."""
    seen = 0
    for name in C.group("content"):
        if C.is_finite(name):
            continue
        for mode in MODES:
            e = C.expected(name, mode)
            assert int(e.on_last.sum()) == 0, name
            bad = ~np.isfinite(e.out)
            assert bad.any() and not (bad & ~e.tap_nonfinite).any(), name
            seen += int(bad.sum())
    assert seen > 100


def test_constant_volume_gives_the_constant_wherever_no_tap_is_outside():
    for name in C.group("content"):
        c = C.case(name)
        if c.content != "constant":
            continue
        e = C.expected(name, "constant")
        assert e.inside.any() and (e.out[e.inside] == np.float32(C.CONSTANT)).all(), name
        g = C.expected(name, "grid-constant")
        assert (g.out[e.inside] == np.float32(C.CONSTANT)).all(), name       # (inside under "constant": all eight taps in the volume)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------


def test_plan_agrees_with_the_path_queries_and_names_each_cases_path():
    for name in C.CASES:
        c = C.case(name)
        for mode in MODES:
            p = c.plan(mode)
            assert p[0] == c.path, (name, p)
            assert p[0] == _lib.call_value("lsr_affine_path_pitched", *c.shape, c.pitch, c.plane, _lib.matrix12(c.m), C.MODE_CODE[mode])
            if c.dense:
                assert p[0] == _lib.call_value("lsr_affine_path", *c.shape, _lib.matrix12(c.m), C.MODE_CODE[mode])
                assert (p[0] == 1) == bool(_lib.call_value("lsr_affine_kernel_choice", c.shape[1], c.shape[2], _lib.matrix12(c.m),
                                                           C.MODE_CODE[mode]))
            if p[0] == 2 and c.dense:
                import ctypes

                out6 = (ctypes.c_int * 6)()
                assert _lib.call_value("lsr_affine_box_shape", *c.shape, _lib.matrix12(c.m), out6) == 1
                assert tuple(out6) == p[1:7], name
            forced = c.plan(mode, pitch=c.gather_pitch)
            assert forced[0] == 0 and forced[13] == -(-c.out_shape[2] // forced[3]) * -(-c.out_shape[1] // forced[2]) * c.out_shape[0]


def test_plan_status_is_the_entrys():
    import ctypes

    lib = _lib.load()
    out = (ctypes.c_int64 * 16)()
    m = _lib.matrix12(np.eye(4)[:3])
    assert lib.lsr_affine_plan(4, 8, 8, 8, 64, 4, 8, 8, 8, m, 0, out) == 0 and out[0] == 1
    assert lib.lsr_affine_plan(4, 8, 8, 8, 64, 4, 8, 8, 8, None, 0, out) == -1
    assert lib.lsr_affine_plan(4, 8, 8, 8, 64, 4, 8, 8, 8, m, 0, None) == -1
    assert lib.lsr_affine_plan(4, 8, 8, 7, 64, 4, 8, 8, 8, m, 0, out) == -2            # a pitch smaller than a row
    assert lib.lsr_affine_plan(4, 8, 8, 8, 64, 4, 8, 8, 7, m, 0, out) == -2
    assert lib.lsr_affine_plan(0, 8, 8, 8, 64, 4, 8, 8, 8, m, 0, out) == -3            # (as the pitched entry: no extent of 0)
    assert lib.lsr_affine_plan(4, 8, 8, 8, 64, 4, 8, 8, 8, m, 7, out) == -4
    assert lib.lsr_affine_plan(4, 8, 8, 8, 64, 4, 8, 8, 8, _lib.matrix12(np.full((3, 4), np.nan)), 0, out) == -4


def test_census_planar():
    """Every tile under both wave counts (crossed with exact / f32 and the two borders by the GPU test: all 32 instances), both ring
    depths, both sides of every bisected threshold, the staging limit at equality, more than one patch per axis, ragged patches."""
    tiles, rings, at = set(), set(), collections.defaultdict(set)
    for name in _planar_names():
        c = C.case(name)
        p = c.plan()
        tiles.add((p[1], p[2], p[3]))
        rings.add(p[6])
        assert p[4] * (p[5] // 4) <= 8 * 64 * p[1] and p[7] <= 150 * 1024, name       # what the kernel's staging loop and LDS hold
    assert tiles == {(w, w * nr, 64 * nc) for w in (8, 4) for nr, nc in C.PLANAR_TILES}, sorted(tiles)
    assert rings == {3, 4}
    for name in C.group("planar_tile"):
        c = C.case(name)
        if c.aimed("tile") is not None:
            at[(c.aimed("waves"), c.aimed("tile"))].add((c.aimed("at"), C.planar_tile_index(c.plan(), c.aimed("waves"))))
    for waves in (8, 4):
        for t in range(4):
            seen = at[(waves, t)]
            assert ("last", t) in seen and ("inside", t) in seen, (waves, t, seen)
            assert any(label == "next" and index > t for label, index in seen), (waves, t, seen)   # the next tile, or another kernel
    stage = {C.case(n).aimed("staging"): C.case(n).plan() for n in C.group("planar_tile") if C.case(n).aimed("staging")}
    assert stage["last"][4] * (stage["last"][5] // 4) == 8 * 64 * stage["last"][1], stage          # the staging limit at equality
    assert stage["last"][1:4] == (4, 16, 128) and stage["next"][1:4] != (4, 16, 128), stage
    ring4 = {C.case(n).aimed("ring4"): C.case(n).plan() for n in C.group("planar_tile") if C.case(n).aimed("ring4")}
    assert ring4["last"][6] == 4 and ring4["last"][2:4] == (32, 128) and ring4["next"][2:4] != (32, 128), ring4
    step = {C.case(n).aimed("step"): C.case(n).plan() for n in C.group("planar_tile") if C.case(n).aimed("step")}
    assert step["ynext"][4] == step["ylast"][4] + 1 and step["ynext"][5] == step["ylast"][5], step
    assert step["xnext"][5] == step["xlast"][5] + 4 and step["xnext"][4] == step["xlast"][4], step
    ring = {C.case(n).aimed("ring"): C.case(n).plan() for n in C.group("planar_z") if C.case(n).aimed("ring")}
    assert (ring["3 last"][6], ring["4 first"][6], ring["4 last"][6], ring["4 last"][0], ring["refused"][0]) == (3, 4, 4, 1, 2), ring
    # the z march: chunk edges, chunks of a launch that begin outside and inside the volume, full and ragged tiles in one launch
    zo_seen = {C.case(n).out_shape[0] for n in C.group("planar_z")}
    assert {1, 15, 16, 17, 32, 33} <= zo_seen and {1, 2} <= {C.case(n).shape[0] for n in C.group("planar_z")}
    chunks, mixed = set(), 0
    for name in C.group("planar_z"):
        c = C.case(name)
        p = c.plan()
        if p[0] != 1:
            continue
        chunks.add(p[8])
        full = (c.out_shape[1] // p[2]) * (c.out_shape[2] // p[3])
        mixed += 0 < full < p[9] * p[10]
    assert 16 in chunks and mixed >= 5
    # patches: more than one along y and along x, ragged last ones, under each patch shape; both block -> tile decodes
    seen = collections.defaultdict(set)
    for name in C.group("planar_map"):
        c = C.case(name)
        p = c.plan()
        assert p[0] == 1 and "%d,%d" % (p[11], p[12]) == c.aimed("patch"), (name, p)          # the switch reached the launcher
        py, px = -(-p[9] // p[11]), -(-p[10] // p[12])
        seen[c.aimed("patch")].add((py > 1, px > 1, p[9] % p[11] != 0 or p[10] % p[12] != 0))
        assert p[13] % 8 == 0 and p[13] >= py * px * 64 * -(-c.out_shape[0] // p[8])
        assert c.plan(f32=True)[13] == p[9] * p[10] * -(-c.out_shape[0] // p[8])
    for patch in ("8,8", "1,64", "64,1"):      # (a patch of one row has no second patch along x below 65 tile columns, and vice versa)
        assert patch == "64,1" or any(y and r for y, x, r in seen[patch]), (patch, seen[patch])
        assert patch == "1,64" or any(x and r for y, x, r in seen[patch]), (patch, seen[patch])
    assert any(y and x for y, x, r in seen["8,8"])


def test_census_box():
    """Every block shape, every compiled walk, the step of the box on each axis, the last map the kernel takes, both block orders
    with more than four blocks per axis, and the three kinds of block in one launch with each predicate met on its value."""
    blocks, walks = set(), set()
    for name in C.CASES:
        c = C.case(name)
        p = c.plan()
        if p[0] == 2:
            blocks.add(p[1:4])
            walks.add((p[1], C.box_walk(c.m)))
            assert p[7] <= 150 * 1024 and -(-(p[7] // 16) // 256) <= 20, name
    assert blocks == set(C.BOX_BLOCKS), f"block shapes not reached: {sorted(set(C.BOX_BLOCKS) - blocks)}"
    assert walks == {(tz, dep) for tz in (8, 16) for dep in (3, 5, 7)}, sorted(walks)
    step = collections.defaultdict(list)
    for name in C.group("box_shape"):
        if C.case(name).aimed("step"):
            step[C.case(name).aimed("step")].append(C.case(name).plan())
    for i, axis in enumerate("zyx"):
        for a, b in zip(step[axis + "last"], step[axis + "next"]):
            grown = tuple(v + (4 if axis == "x" else 1) * (j == i) for j, v in enumerate(a[4:7]))
            assert a[1:4] == b[1:4] and b[4:7] == grown, (axis, a, b)
    limit = {C.case(n).aimed("limit"): C.case(n).plan() for n in C.group("box_shape") if C.case(n).aimed("limit")}
    assert limit["last"][0] == 2 and limit["next"][0] == 0 and -(-(limit["last"][7] // 16) // 256) == 20, limit
    linear = {C.case(n).aimed("linear"): C.case(n).plan() for n in C.group("box_shape") if C.case(n).aimed("linear") is not None}
    assert linear[0][11] == 0 and linear[1][11] == 1, linear                                       # the switch reached the launcher
    assert min(linear[0][8:11]) > 4, linear                                                        # more than one patch along each axis
    # whole-number maps and padded strides go through every kernel
    assert {C.case(n).path for n in C.group("grid_points")} == {0, 1, 2} and {C.case(n).path for n in C.group("strides")} == {0, 1, 2}
    assert {C.case(n).path for n in C.group("content")} == {0, 1, 2}
    # exact and f32 mode number the blocks differently unless told otherwise
    some = C.case(C.group("box_kind")[0])
    assert some.plan()[11] == 0 and some.plan(f32=True)[11] == 1
    all_three = 0
    flips = collections.defaultdict(dict)
    for name in C.group("box_kind"):
        c = C.case(name)
        p = c.plan()
        for mode in MODES:
            kinds = C.block_kinds(c.m, p, c.out_shape, c.shape, mode == "grid-constant")
            all_three += all(kinds.values())
        flips[(c.aimed("axis"), c.aimed("which"), c.aimed("value"))][c.aimed("at")] = c.aimed("corner")
    assert all_three >= 12
    assert len(flips) == 18
    for (axis, which, value), corners in flips.items():
        assert corners["on"] == value and corners["the double below"] < value < corners["the double above"], (axis, which, value, corners)
        assert corners["the double below"] >= np.nextafter(value, -np.inf) - 1e-14 and corners["the double above"] <= value + 1e-14


# ---- the coverage claims ----------------------------------------------------------------------------------------------------------


def _staged_columns(xlo, box_x, xi):
    """Source column held by each float of a staged row: whole 16-byte chunks, clamped into the rows as the kernels clamp them."""
    j = np.arange(box_x)
    return np.clip(xlo + 4 * (j // 4), 0, ((xi + 3) & ~3) - 4) + j % 4


def _axis_taps(c, n, grid):
    """``(i0, live0, live1, ok)`` of one axis: the lower tap as the kernels index it, which of the two taps must hold the source
    voxel of their index (inside the volume and of non-zero weight), and whether the sample exists at all."""
    fl = np.floor(c)
    w0 = 1.0 - (c - fl)
    w1 = 1.0 - w0
    if grid:
        i0 = np.clip(fl, -2.0, n + 1.0).astype(np.int64)
        ok = np.ones(c.shape, dtype=bool)
        return i0, (i0 >= 0) & (i0 < n), (i0 + 1 >= 0) & (i0 + 1 < n), ok
    ok = (c >= 0.0) & (c <= n - 1.0)
    i0 = np.where(ok, fl, 0.0).astype(np.int64)
    return i0, ok, ok & ((i0 + 1 < n) | (w1 != 0.0)), ok


def planar_coverage(m, plan, shape, out_shape, grid):
    """Every tile of a planar launch: the taps of every sample lie inside the box the plan reports -- the kernel's clamps move no
    index -- and the staged box holds, at each tap that counts, the source voxel the rule names.  Returns the taps checked."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    (b, c, ty), (d, e, tx) = (m[1, 1], m[1, 2], m[1, 3]), (m[2, 1], m[2, 2], m[2, 3])
    yi, xi = shape[1], shape[2]
    tile_y, tile_x, box_y, box_x = plan[2], plan[3], plan[4], plan[5]
    coord = lambda yo, xo, m1, m2, sh: (yo * m1 + xo * m2) + sh                       # noqa: E731
    checked = 0
    for y0 in range(0, out_shape[1], tile_y):
        for x0 in range(0, out_shape[2], tile_x):
            y1, x1 = min(y0 + tile_y, out_shape[1]) - 1, min(x0 + tile_x, out_shape[2]) - 1
            yo = np.arange(y0, y1 + 1, dtype=np.float64).reshape(-1, 1)
            xo = np.arange(x0, x1 + 1, dtype=np.float64).reshape(1, -1)
            cy, cx = coord(yo, xo, b, c, ty), coord(yo, xo, d, e, tx)
            cy_min = coord(float(y1 if b < 0.0 else y0), float(x1 if c < 0.0 else x0), b, c, ty)
            cx_min = coord(float(y1 if d < 0.0 else y0), float(x1 if e < 0.0 else x0), d, e, tx)
            assert cy_min == cy.min() and cx_min == cx.min()                         # the corner IS the smallest coordinate
            for low in ((-1.0, 0.0) if not grid else (-1.0,)):                      # both values of kLow hold an inside pixel's taps
                ylo = int(min(max(np.floor(cy_min), low), yi - 1.0))
                xlo = int(min(max(np.floor(cx_min), low), xi - 1.0)) & ~3
                iy0, ly0, ly1, oky = _axis_taps(cy, yi, grid)
                ix0, lx0, lx1, okx = _axis_taps(cx, xi, grid)
                ok = oky & okx
                if not grid:
                    ly0, ly1, lx0, lx1 = ly0 & ok, ly1 & ok, lx0 & ok, lx1 & ok
                    assert (iy0 - ylo)[ok].min(initial=0) >= 0 and (iy0 - ylo)[ok].max(initial=0) <= box_y - 2, (y0, x0, low)
                    assert (ix0 - xlo)[ok].min(initial=0) >= 0 and (ix0 - xlo)[ok].max(initial=0) <= box_x - 2, (y0, x0, low)
                by0, bx0 = np.clip(iy0 - ylo, 0, box_y - 2), np.clip(ix0 - xlo, 0, box_x - 2)
                rows = np.clip(ylo + np.arange(box_y), 0, yi - 1)
                cols = _staged_columns(xlo, box_x, xi)
                for dy, live_y in ((0, ly0), (1, ly1)):
                    assert (rows[by0 + dy] == iy0 + dy)[live_y].all(), (y0, x0, low, dy)
                    checked += int(live_y.sum())
                for dx, live_x in ((0, lx0), (1, lx1)):
                    assert (cols[bx0 + dx] == ix0 + dx)[live_x].all(), (y0, x0, low, dx)
                    checked += int(live_x.sum())
    return checked


def box_coverage(m, plan, shape, out_shape, grid):
    """The same for every block of a box-kernel launch, on the three axes."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    block, box = plan[1:4], plan[4:7]
    checked = 0
    for bz in range(plan[8]):
        for by in range(plan[9]):
            for bx in range(plan[10]):
                lo = [i * t for i, t in zip((bz, by, bx), block)]
                hi = [min(l + t, n) - 1 for l, t, n in zip(lo, block, out_shape)]
                corners = C.block_corners(m, plan, out_shape, (bz, by, bx))
                last = [n - 1.0 for n in shape]
                if grid:
                    blind = any(not (h > -1.0) or not (l < n + 1.0) for (l, h), n in zip(corners, last))
                else:
                    blind = any(h < 0.0 or l > n for (l, h), n in zip(corners, last))
                if blind:
                    continue
                zo = np.arange(lo[0], hi[0] + 1, dtype=np.float64).reshape(-1, 1, 1)
                yo = np.arange(lo[1], hi[1] + 1, dtype=np.float64).reshape(1, -1, 1)
                xo = np.arange(lo[2], hi[2] + 1, dtype=np.float64).reshape(1, 1, -1)
                taps, ok = [], True
                for axis in range(3):
                    r = m[axis]
                    c = ((zo * r[0] + yo * r[1]) + xo * r[2]) + r[3]
                    c = np.broadcast_to(c, (hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1))
                    assert corners[axis] == (c.min(), c.max())                       # the corners ARE the extremes, exactly
                    taps.append(_axis_taps(c, shape[axis], grid))
                    ok = ok & taps[-1][3]
                for axis in range(3):
                    i0, l0, l1, _ = taps[axis]
                    n = shape[axis]
                    origin = int(min(max(np.floor(corners[axis][0]), -1.0 if grid else 0.0), n - 1.0))
                    if axis == 2:
                        origin &= ~3
                    if not grid:
                        l0, l1 = l0 & ok, l1 & ok
                        assert (i0 - origin)[ok].min(initial=0) >= 0 and (i0 - origin)[ok].max(initial=0) <= box[axis] - 2, (bz, by, bx, axis)
                    held = _staged_columns(origin, box[axis], n) if axis == 2 else np.clip(origin + np.arange(box[axis]), 0, n - 1)
                    at = i0 - origin
                    for d, live in ((0, l0), (1, l1)):
                        assert ((at + d >= 0) & (at + d < box[axis]))[live].all(), (bz, by, bx, axis, d)
                        assert (held[np.clip(at + d, 0, box[axis] - 1)] == i0 + d)[live].all(), (bz, by, bx, axis, d)
                        checked += int(live.sum())
    return checked


def test_planar_box_covers_every_tap_of_every_tile_at_the_designed_thresholds():
    checked = 0
    for name in C.group("planar_tile") + C.group("planar_map") + C.group("grid_points") + C.group("strides"):
        c = C.case(name)
        p = c.plan()
        if p[0] != 1:
            continue
        for grid in (False, True):
            checked += planar_coverage(c.m, p, c.shape, c.out_shape, grid)
    assert checked > 1_000_000


def test_planar_box_covers_every_tap_of_every_tile_for_random_maps():
    rng = np.random.default_rng(2024)
    shape, out_shape = (3, 200, 304), (1, 70, 300)
    done, tiles = 0, set()
    for i in range(400):
        th = np.deg2rad(rng.uniform(-45, 45))
        s = np.exp(rng.uniform(np.log(0.3), np.log(2.6), 2)) * rng.choice([1.0, -1.0], 2)
        rows = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(th), -np.sin(th)], [0.0, np.sin(th), np.cos(th)]]) @ np.diag([1.0, s[0], s[1]])
        rows[1, 2] += rng.uniform(-0.2, 0.2)
        m = C.fit(rows, out_shape, keep=rng.uniform(0.5, 1.2))[1]
        m[:, 3] += rng.uniform(-3, 3, 3)
        with C.switched((("LSR_PLANAR_WAVES", "4"),) if i % 2 else ()):
            p = C.raw_plan(shape, shape[2], shape[1] * shape[2], out_shape, out_shape[2], m, 0)
        if p[0] != 1:
            continue
        tiles.add(p[1:4])
        planar_coverage(m, p, shape, out_shape, bool(i % 3 == 0))
        done += 1
    assert done > 300 and len(tiles) >= 6, (done, tiles)


def test_box_kernel_box_covers_every_tap_of_every_block_at_the_designed_thresholds():
    checked = 0
    for name in C.group("box_shape") + C.group("box_kind")[::3] + C.group("grid_points") + C.group("strides"):
        c = C.case(name)
        p = c.plan()
        if p[0] != 2:
            continue
        for grid in (False, True):
            checked += box_coverage(c.m, p, c.shape, c.out_shape, grid)
    assert checked > 1_000_000
