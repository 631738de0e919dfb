"""The fused deskew on the host: the restated rule (``tests/deskew_ref.py``) against scipy (``oracle.cpu_ref``) bit for bit on every
finite case, the twins ``lsr_deskew_*_cpu`` against the restatement on every case they answer, the launch plan
(``lsr_deskew_plan``) against the slab it has to fit -- no kernel runs here -- and a census: every tile width, staging pass, slab
position, extent, sign, offset, border, fill value, entry and content the cases aim at is reached, computed from the plan and the
restatement and never from a result.

Cases: ``tests/deskew_cases.py``.
"""

import functools
import math

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from shrimpy_amd import _lib
from shrimpy_amd import deskew as D
from tests import deskew_cases as C
from tests import deskew_ref as R


# ---- running the twin -------------------------------------------------------------------------------------------------------------


def run_twin(name, u16=False):
    """``(window, padding kept, window written)`` of the twin on a case; raises what the twin answers."""
    c = C.case(name)
    data = np.array(C.raw_u16(name) if u16 else C.raw(name), order="C")
    buf = C.output_buffer(c)
    flat = C.flat(name)
    pattern = None if flat is None else np.array(flat[0], order="C")
    mean = None if flat is None else np.array([flat[1]], dtype=np.float32)
    cv = C.fill(name)
    cval = None if cv is None else np.array([cv], dtype=np.float32)
    entry, args = C.entry_args(c, u16, data.ctypes.data, buf.ctypes.data, None if pattern is None else pattern.ctypes.data,
                               None if mean is None else mean.ctypes.data, None if cval is None else cval.ctypes.data, None, cpu=True)
    _lib.call(entry, *args)
    return (np.array(C.window(c, buf)),) + C.padding_intact(c, buf)


def twin_answers(name):
    c = C.case(name)
    return c.mode == "constant" and c.flat is None


@functools.lru_cache(maxsize=None)
def case_twin(name):
    """The twin's result on a case it answers, computed once (read-only; tests/test_deskew_edges_gpu.py holds the device to it)."""
    out, _, _ = run_twin(name)
    out.setflags(write=False)
    return out


def check(got, name, what):
    want = C.expected(name)
    assert R.same_bits(got, want), f"{what} on {name!r}: {R.describe_difference(got, want)}"


# ---- the restatement against scipy ------------------------------------------------------------------------------------------------


def oracle(name):
    c = C.case(name)
    cv = C.fill(name)
    m = np.array(c.matrix, dtype=np.float64).reshape(3, 4)
    pre = cpu_ref.affine_apply(R.corrected(C.raw(name), C.flat(name)), m[:, :3], m[:, 3], c.pre_shape,
                               cval=0.0 if cv is None else float(cv), mode=c.mode)
    return cpu_ref.average_slices(pre, c.avg)


@pytest.mark.parametrize("g", C.GROUPS)
def test_the_restatement_is_scipy_and_the_oracle_mean_bit_for_bit(g):
    """Every case whose samples are all finite (``+-3e38`` and the denormals among them), no voxel left out, the sign of a zero
    included.  The two places where the oracle is not the rule are in ``tests/deskew_ref.py``'s docstring."""
    compared = 0
    for name in C.group(g):
        c = C.case(name)
        if not C.is_finite(name):
            continue
        assert R.oracle_comparable_plane(c.Yo, c.Xo, c.avg), name
        want = oracle(name)
        assert R.same_bits(C.expected(name), want), f"{name}: {R.describe_difference(C.expected(name), want)}"
        compared += 1
    assert compared == sum(C.is_finite(n) for n in C.group(g)) >= len(C.group(g)) // 2


def test_the_oracle_mean_is_pairwise_on_a_single_voxel_plane():
    """Why a (1, 1) plane with ``avg >= 8`` is held to the restatement alone: ``numpy.mean`` does not add in plane order there."""
    pre = C.average_input(24, 8, (1, 1))
    assert not R.oracle_comparable_plane(1, 1, 8) and R.oracle_comparable_plane(1, 2, 8) and R.oracle_comparable_plane(1, 1, 7)
    seq = R.average(pre, 8)
    want = np.array([[[np.float32(sum(float(v) for v in pre[8 * g:8 * g + 8, 0, 0]) / 8)]] for g in range(3)])
    assert np.allclose(seq, want, rtol=1e-6)
    assert R.same_bits(R.average(pre[:21], 7), cpu_ref.average_slices(np.array(pre[:21]), 7))


def test_the_rule_by_hand():
    f = np.float32
    raw = np.arange(4, dtype=np.float32).reshape(4, 1, 1) * f(10.0)                       # 0, 10, 20, 30 along z
    m = R.shear(0.0, 0.5, -1.25, 1, 0, 1, 0)                                              # z_in = -1.25, -0.75, ..., 3.25
    got = R.pre_average(raw, m, (1, 1, 10), "constant", 7.0)[0, 0]
    assert got.tolist() == [7.0, 7.0, 7.0, 2.5, 7.5, 12.5, 17.5, 22.5, 27.5, 7.0]
    got = R.pre_average(raw, m, (1, 1, 10), "grid-constant", 8.0)[0, 0]
    assert got.tolist() == [8.0, 6.0, 2.0, 2.5, 7.5, 12.5, 17.5, 22.5, 27.5, 24.5]     # 0.75 * 8 + 0.25 * 0, ..., 0.75 * 30 + 0.25 * 8
    whole = R.shear(0.0, 1.0, -1.0, 1, 0, 1, 0)                                           # z_in = -1, 0, 1, 2, 3, 4
    assert R.pre_average(raw, whole, (1, 1, 6), "constant", 7.0)[0, 0].tolist() == [7.0, 0.0, 10.0, 20.0, 30.0, 7.0]
    assert R.pre_average(raw, whole, (1, 1, 6), "grid-constant", 7.0)[0, 0].tolist() == [7.0, 0.0, 10.0, 20.0, 30.0, 7.0]
    # a row or a column outside the stack is the fill value under either border
    assert R.pre_average(raw, R.shear(0.0, 1.0, 0.0, 1, 1, 1, 0), (1, 1, 2), "grid-constant", 7.0).tolist() == [[[7.0, 7.0]]]
    assert R.pre_average(raw, R.shear(0.0, 1.0, 0.0, 1, 0, -1, -1), (1, 1, 2), "constant", 7.0).tolist() == [[[7.0, 7.0]]]
    # the clamped neighbour of an infinity at z = Z - 1 multiplies it by zero; scipy mirrors instead
    top = raw.copy()
    top[3] = np.inf
    assert np.isnan(R.pre_average(top, whole, (1, 1, 6), "constant", 7.0)[0, 0, 4])
    # the mean: a float32 sum from the first plane on, the last group edge-padded, one division
    pre = np.array([1.0, 2.0 ** 24, 1.0, 5.0], dtype=np.float32).reshape(4, 1, 1)
    assert R.average(pre, 3).ravel().tolist() == [float(f(f(f(1.0) + f(2.0 ** 24)) + f(1.0)) / f(3.0)), 5.0]
    assert R.average(pre, 1) is not pre and R.average(pre, 1).tobytes() == pre.tobytes()
    assert R.tile_rows(R.shear(0.0, 1.0, 0.5, 1, 0, 1, 0), 100, 0, 0, 64) == (65, 0.0, 64.0)
    assert R.tile_rows(R.shear(0.0, 1.0, -70.0, 1, 0, 1, 0), 100, 0, 0, 64)[0] == 0 and staged_rows(0.0, 1.0, -70.0, 0, 0, 64, 100) == 0


# ---- the plan and the slab --------------------------------------------------------------------------------------------------------


def staged_rows(a, b, c, zd, xo0, n_xo, z_extent):
    """The kernel's row count, restated: ``floor(max z) + 1 - floor(min z) + 1`` over the tile's two end columns, clamped to the scan
    (Python floats: every product and sum rounded on its own)."""
    z0 = ((float(zd) * a + 0.0 * 0.0) + float(xo0) * b) + c
    z1 = ((float(zd) * a + 0.0 * 0.0) + float(xo0 + n_xo - 1) * b) + c
    lo, hi = math.floor(min(z0, z1)), math.floor(max(z0, z1)) + 1
    if hi < 0 or lo > z_extent - 1:
        return 0
    return min(max(hi, 0), z_extent - 1) - min(max(lo, 0), z_extent - 1) + 1


def threshold_values(w):
    """The ``|b|`` around the edge of a tile width: the threshold and the doubles either side (the width 1 has no upper edge)."""
    if w == 1:
        return [C.next_up(C.threshold(2)), 300.0, 2.0 ** 30]
    t = C.threshold(w)
    return [C.next_down(t), t, C.next_up(t)]


SWEEP_BASES = (0.0, -3.0, -1000.0) + C.SLAB_BASES


@functools.lru_cache(maxsize=None)
def admitted_rows(w, sign):
    """The most rows a tile of width ``w`` stages at its threshold, ``b`` of this sign, over the offsets the slab cases are chosen
    from (a scan without ends)."""
    v = C.threshold(w) if w > 1 else 300.0
    return max(staged_rows(0.0, sign * v, c, 0, 0, w, 2 ** 40) for c in C.slab_offsets(w, sign * v))


def test_the_plan_halves_the_tile_at_each_threshold_and_refuses_nothing():
    assert (C.TILE_Y, C.SLAB_ROWS, C.PASS_ROWS) == (64, 68, 24)
    assert [C.tile_width(b) for b in (0.0, 2.0 ** -40, -0.3, 0.755, -1.0)] == [64] * 5
    for w in C.WIDTHS[:-1]:
        t = C.threshold(w)
        assert [C.tile_width(s * v) for v in (t, C.next_up(t)) for s in (1, -1)] == [w, w, w // 2, w // 2], w
        assert abs(t * (w - 1) - (C.SLAB_ROWS - 3)) < 1e-9, "the rule: |b| (w - 1) + 3 rows fit the slab"
    assert [C.tile_width(b) for b in (65.5, -300.0, 2.0 ** 30, -1e300)] == [1] * 4
    # tiles, blocks and the launched grid
    m = R.shear(0.0, 0.3, 0.0, -1, 0, -1, 0)
    assert C.plan(3, 65, 129, m) == (64, 64, 68, 24, 3, 2, 18, 24)
    assert C.plan(1, 1, 1, m)[4:] == (1, 1, 1, 8) and C.plan(2, 64, 128, m)[4:] == (2, 1, 4, 8)
    assert C.plan(1, 10, 9, R.shear(0.0, 9.0, 0.0, -1, 0, -1, 0))[:5] == (8, 64, 68, 24, 2)
    # the statuses of the deskew entries for the same arguments
    for bad, kind in ((R.shear(0.0, 1.0, 0.0, -1, 0.5, -1, 0), _lib.LsrUnsupported), (R.shear(0.0, 1.0, 0.0, 2, 0, -1, 0), _lib.LsrUnsupported),
                      (R.shear(0.0, float("nan"), 0.0, -1, 0, -1, 0), _lib.LsrError), ([0.0, 0.1] + m[2:], _lib.LsrUnsupported)):
        with pytest.raises(kind):
            C.plan(1, 1, 1, bad)
    with pytest.raises(_lib.LsrError):
        C.plan(0, 1, 1, m)
    with pytest.raises(_lib.LsrError):
        C.plan(2 ** 31, 1, 1, m)


def test_the_plan_follows_the_swizzle_switch(monkeypatch):
    m = R.shear(0.0, 0.3, 0.0, -1, 0, -1, 0)
    monkeypatch.setenv("LSR_DESKEW_SWIZZLE", "0")
    assert C.plan(3, 65, 129, m)[6:] == (18, 18)
    monkeypatch.setenv("LSR_DESKEW_SWIZZLE", "1")
    assert C.plan(3, 65, 129, m)[6:] == (18, 24)


@pytest.mark.parametrize("w", C.WIDTHS)
def test_the_staged_rows_always_fit_the_slab(w):
    """At the threshold of every tile width and the doubles either side, both signs, tiles at several offsets along X' and a sweep of
    ``c`` that includes offsets just below a whole number: the rows the kernel's formula counts never pass the slab the plan reports.
    (One row more is silent corruption of the workgroup's LDS, not a fault.)"""
    worst = 0
    for v in threshold_values(w):
        for s in (1.0, -1.0):
            b = s * v
            tile, _, slab = C.plan(1, 1, 1, R.shear(0.0, b, 0.0, -1, 0, -1, 0))[:3]
            assert tile == (w if v <= (C.threshold(w) if w > 1 else math.inf) else w // 2)
            for xo0 in (0, tile, 5 * tile, 1023 * tile):
                for a, zd in ((0.0, 0), (-b * C.COS30, 7), (0.37, 170)):
                    for base in SWEEP_BASES:
                        for f in C.FRACTIONS:
                            rows = staged_rows(a, b, base + f, zd, xo0, tile, 2 ** 40)
                            assert rows <= slab, (w, b, a, zd, xo0, base + f, rows)
                            assert rows == R.tile_rows(R.shear(a, b, base + f, -1, 0, -1, 0), 2 ** 40, zd, xo0, tile)[0]
                            worst = max(worst, rows)
    print(f"tile width {w}: at most {worst} of {C.SLAB_ROWS} rows")
    assert worst >= max(admitted_rows(w, 1.0), admitted_rows(w, -1.0)) and (w == 1 or worst >= C.SLAB_ROWS - 1), "the sweep reaches the rows the rule is there for"


# ---- the census -------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def facts(name):
    """What a case reaches, from the plan and the restatement's coordinates."""
    c = C.case(name)
    m = c.matrix
    w, _, _, per_pass, tiles_x, tiles_y, blocks, _ = c.plan
    y_in, y_ok = R.y_rows(m, c.Zd, c.Y)
    x_in, x_ok = R.x_cols(m, c.Yo, c.X)
    rows, positions = set(), set()
    for zd in np.flatnonzero(y_ok):
        for tx in range(tiles_x):
            n = min(w, c.Xo - tx * w)
            count, lo_d, hi_d = R.tile_rows(m, c.Z, int(zd), tx * w, n)
            assert count == staged_rows(c.a, c.b, c.c, int(zd), tx * w, n, c.Z) and count <= C.SLAB_ROWS, name
            rows.add(count)
            z = R.z_coords(m, [zd], range(tx * w, tx * w + n))[0]
            if z.max() < 0:
                positions.add("below")
            elif z.min() > c.Z - 1:
                positions.add("above")
            else:
                positions |= ({"straddles z < 0"} if z.min() < 0 else set()) | ({"straddles z > Z - 1"} if z.max() > c.Z - 1 else set())
                if z.min() >= 0 and z.max() <= c.Z - 1:
                    positions.add("inside")
            if count == 0:
                positions.add("nothing staged")
    z_all = R.z_coords(m, np.flatnonzero(y_ok), range(c.Xo))
    z_flags = {label for label, hit in (("0", z_all == 0), ("Z - 1", z_all == c.Z - 1), ("(-1, 0)", (z_all > -1) & (z_all < 0)),
                                        ("(Z - 1, Z)", (z_all > c.Z - 1) & (z_all < c.Z)), ("-1", z_all == -1), ("Z", z_all == c.Z))
               if hit.any()}
    row_kinds = set()
    for zo in range(c.Zo):
        out = [not y_ok[min(zo * c.avg + k, c.Zd - 1)] for k in range(c.avg)]
        n_out = sum(out)
        if n_out == 0:
            continue
        if n_out == c.avg:
            row_kinds.add("a whole group")
        elif all(out[:n_out]):
            row_kinds.add("the first of a group")
        elif all(out[-n_out:]):
            row_kinds.add("the last of a group")
    row_kinds = {"every row"} if not y_ok.any() else (row_kinds or {"no row"})
    col_kinds = set()
    for ty in range(tiles_y):
        out = (~x_ok[ty * C.TILE_Y:(ty + 1) * C.TILE_Y]).tolist()
        n_out = sum(out)
        if n_out == 0:
            continue
        if n_out == len(out):
            if len(out) == C.TILE_Y:
                col_kinds.add("a whole tile")
        elif all(out[:n_out]):
            col_kinds.add("the first of a tile")
        elif all(out[-n_out:]):
            col_kinds.add("the last of a tile")
    col_kinds = {"every column"} if not x_ok.any() else (col_kinds or {"no column"})
    return dict(w=w, rows=frozenset(rows), passes=frozenset(-(-r // per_pass) for r in rows if r), positions=frozenset(positions),
                z=frozenset(z_flags), row_kinds=frozenset(row_kinds), col_kinds=frozenset(col_kinds), blocks=blocks)


def _cases_of(g=None, **match):
    return [C.case(n) for n in (C.group(g) if g else C.CASES) if all(getattr(C.case(n), k) == v for k, v in match.items())]


def test_the_cases_reach_every_tile_width_and_its_edges():
    for w in C.WIDTHS:
        mine = [c for c in _cases_of("tile") if facts(c.name)["w"] == w]
        bs = {c.b for c in mine}
        want = {s * C.inside_b(w) for s in (1, -1)}
        if w > 1:
            want |= {C.threshold(w), -C.threshold(w)}
        if w < 64:
            want |= {s * C.next_up(C.threshold(2 * w)) for s in (1, -1)}
        assert want <= bs, (w, sorted(want - bs))
        assert {c.Xo for c in mine} >= {x for x in (1, w - 1, w, w + 1, 2 * w + 1) if x >= 1}, w
        kinds = {"0" if c.a == 0 else "0.37" if c.a == 0.37 else "-b cos 30" if c.a == -c.b * C.COS30 else "?" for c in mine}
        assert kinds == {"0", "0.37", "-b cos 30"}, w
        assert {c.mode for c in mine} == set(R.MODES)
        # the most rows the host rule admits for this width, in a tile wholly inside the scan
        for sign in (1.0, -1.0):
            most = max(max(facts(c.name)["rows"], default=0) for c in _cases_of() if facts(c.name)["w"] == w and c.b * sign > 0)
            assert most == admitted_rows(w, sign), (w, sign, most, admitted_rows(w, sign))
    assert {0.0, 2.0 ** -40, 0.3, 0.755, 1.0} <= {c.b for c in _cases_of("tile") if facts(c.name)["w"] == 64}
    assert {facts(n)["w"] for n in C.CASES} == set(C.WIDTHS)
    assert any(c.b < 0 for c in _cases_of()) and any(c.b == 0 for c in _cases_of())


def test_the_cases_reach_every_staging_pass_and_slab_position():
    for mode in R.MODES:
        mine = _cases_of(mode=mode)
        assert set().union(*(facts(c.name)["passes"] for c in mine)) == {1, 2, 3}, mode
        assert {0, 1, 2, 24, 25, 48, 49} & set().union(*(facts(c.name)["rows"] for c in mine)) >= {0, 1, 2}
        five = [c for c in mine if c.name.startswith("position: five tiles")]
        assert len(five) == 2 and {c.b > 0 for c in five} == {True, False}
        for c in five:
            assert facts(c.name)["positions"] >= {"below", "straddles z < 0", "inside", "straddles z > Z - 1", "above", "nothing staged"}
        reached = set().union(*(facts(c.name)["z"] for c in mine))
        assert reached >= {"0", "Z - 1", "(-1, 0)", "(Z - 1, Z)", "-1", "Z"}, (mode, reached)
        for z in (1, 2, 3):
            small = [c for c in mine if c.Z == z]
            assert set().union(*(facts(c.name)["z"] for c in small)) >= {"0", "Z - 1", "(-1, 0)", "(Z - 1, Z)"}, (mode, z)
    assert max(max(facts(n)["rows"], default=0) for n in C.CASES) >= C.SLAB_ROWS - 1


def test_the_cases_reach_every_extent_and_block_count():
    ext = _cases_of("extent")
    assert [(c.Zd, c.avg) for c in ext] == C.ZD_AVG and {c.Yo for c in ext} == set(C.YO_LIST) == {1, 63, 64, 65, 129}
    blocks = [facts(c.name)["blocks"] for c in ext]
    assert {b % 8 for b in blocks} == set(range(8)) and {1, 7} <= set(blocks) and max(blocks) > 8
    assert all(c.swizzle_off for c in ext)
    off = [facts(n)["blocks"] for n in C.SWIZZLE_CASES]
    assert {b % 8 for b in off} == set(range(8)) and min(off) < 8 < max(off)
    assert {facts(n)["w"] for n in C.SWIZZLE_CASES} >= {64, 8, 1}
    # strides: dense, rows padded by 1 .. 3 floats, planes with spare rows
    assert {c.pitch_pad for c in _cases_of()} == {0, 1, 2, 3} and {c.spare_rows for c in _cases_of()} == {0, 1, 2}
    assert any(c.pitch_pad == 0 and c.spare_rows for c in _cases_of()) and any(c.pitch_pad and not c.spare_rows for c in _cases_of())
    assert all(c.plane >= c.Yo * c.pitch for c in _cases_of())


def test_the_cases_reach_every_sign_and_offset():
    for sy in (-1, 1):
        for sx in (-1, 1):
            mine = _cases_of("sign", sy=sy, sx=sx)
            assert [next(iter(facts(c.name)["row_kinds"])) for c in mine] == C.ROW_KINDS, (sy, sx)
            assert sorted(k for c in mine for k in facts(c.name)["col_kinds"]) == sorted(C.COL_KINDS), (sy, sx)
            assert all(len(facts(c.name)["row_kinds"]) == 1 == len(facts(c.name)["col_kinds"]) for c in mine)
    assert all(c.avg == 3 and c.Yo > 2 * C.TILE_Y for c in _cases_of("sign"))
    # ... and the product's own geometry is among the rest
    assert any((c.sy, c.oy, c.sx, c.ox) == (-1, c.Y - 1, -1, c.X - 1) and c.b > 0 for c in _cases_of("tile"))


def test_the_cases_reach_every_border_fill_entry_and_content():
    fills = {(c.mode, c.cval) for c in _cases_of("fill")}
    assert fills == {(mode, cval) for mode in R.MODES for cval in C.FILLS} and float(np.float32(132.8)) in C.FILLS and 132.8 not in C.FILLS
    for c in _cases_of("fill"):
        assert facts(c.name)["row_kinds"] == {"the last of a group"} and facts(c.name)["col_kinds"] == {"the last of a tile"}
        assert C.raw(c.name).min() > 100, "a minimum that is not the default fill value"
    entries = {C.entry_name(c, u16) for c in _cases_of() for u16 in ((False, True) if c.has_u16 else (False,))}
    assert entries == set(C.ENTRIES)
    for mode in R.MODES:
        assert {(c.family, c.flat is not None, u16) for c in _cases_of(mode=mode) for u16 in ((False, True) if c.has_u16 else (False,))} >= \
            {(f, fl, u) for f in ("border", "cval") for fl in (False, True) for u in (False, True)}, mode
    assert {c.flat for c in _cases_of()} == {None, "generic", "zero", "nan"}
    for c in _cases_of():
        if c.has_u16:
            v = C.raw_u16(c.name)
            assert v.dtype == np.uint16 and (c.content != "counts" or ((v == 0).any() and (v == 65535).any())), c.name
        if c.flat in ("zero", "nan"):
            pat = C.flat(c.name)[0]
            assert ((pat == 0).sum() if c.flat == "zero" else np.isnan(pat).sum()) == 1 and not C.is_finite(c.name)
    contents = {c.content for c in _cases_of("content")}
    assert contents == {"uniform", "counts", "huge", "denormal", "nonfinite interior", "nonfinite top"}
    assert (C.raw("content: uniform constant") < 0).any() and (np.abs(C.raw("content: huge constant")) == np.float32(3e38)).any()
    tiny = C.raw("content: denormal constant")
    assert (np.abs(tiny[tiny != 0]) < np.finfo(np.float32).tiny).all()
    # the non-finite stacks: at an interior voxel; at z = Z - 1 where z_in == Z - 1; as the zero-weight upper neighbour
    seen = set()
    for c in _cases_of("content"):
        if not c.content.startswith("nonfinite"):
            continue
        v = C.raw(c.name)
        at = np.argwhere(~np.isfinite(v))
        assert [tuple(r) for r in at.tolist()] == sorted(C.nonfinite_at(c)) and len(at) == 3 and np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
        y_in, _ = R.y_rows(c.matrix, c.Zd, c.Y)
        for z, y, x in at:
            for zd in np.flatnonzero(y_in == y):
                z_in = R.z_coords(c.matrix, [zd], range(c.Xo))[0]
                if 0 < z < c.Z - 1 and ((z_in > z - 1) & (z_in < z + 1) & (z_in != np.floor(z_in))).any():
                    seen.add((c.mode, "interior"))
                if z == c.Z - 1 and (z_in == c.Z - 1).any():
                    seen.add((c.mode, "top"))
                if (z_in == z - 1).any():
                    seen.add((c.mode, "zero-weight neighbour"))
        assert np.isnan(C.expected(c.name)).any()
    assert seen == {(mode, k) for mode in R.MODES for k in ("interior", "top", "zero-weight neighbour")}, seen
    assert sorted(n for g in C.GROUPS for n in C.group(g)) == sorted(C.CASES), "the groups the tests run hold every case once"
    print(f"{len(C.CASES)} cases")


def test_the_average_and_fallback_cases():
    assert [(zd, avg) for zd, avg, plane in C.AVERAGE_CASES if plane == (5, 70)] == C.ZD_AVG
    assert (24, 8, (1, 1)) in C.AVERAGE_CASES
    zd, avg, plane = C.AVERAGE_CASES[-1]
    assert -(-zd // avg) * plane[0] * plane[1] > 8192 * 256, "past the grid cap: the grid-stride loop runs twice"
    with pytest.raises(_lib.LsrUnsupported):
        C.plan(1, 1, 1, np.array(C.GENERAL_MATRIX).ravel().tolist())


# ---- the twin against the restatement -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("g", C.GROUPS)
def test_twin_equals_the_restatement_bit_for_bit(g):
    """Every ``"constant"`` case without a flat-field, the non-finite stacks included (a NaN by position), float32 and uint16; the
    padding keeps its bits.  The other cases are refused."""
    for name in C.group(g):
        c = C.case(name)
        if not twin_answers(name):
            with pytest.raises(_lib.LsrUnsupported):
                run_twin(name)
            continue
        for u16 in ((False, True) if c.has_u16 else (False,)):
            out, kept, written = run_twin(name, u16)
            check(out, name, "the uint16 twin" if u16 else "the twin")
            assert kept and written, f"{name}: a word of the padding was written, or one of the window left"
            assert R.same_bits(out, case_twin(name))


def test_twin_average_equals_the_restatement():
    for zd, avg, plane in C.AVERAGE_CASES:
        pre = C.average_input(zd, avg, plane)
        got = D.average_n_slices(torch.from_numpy(np.array(pre)), avg).numpy()
        assert R.same_bits(got, R.average(pre, avg)), (zd, avg, plane)
        if R.oracle_comparable_plane(plane[0], plane[1], avg):
            assert R.same_bits(got, cpu_ref.average_slices(np.array(pre), avg)), (zd, avg, plane)


def general_expected():
    m = np.array(C.GENERAL_MATRIX, dtype=np.float64)
    return R.average(cpu_ref.affine_apply(C.general_raw(), m[:, :3], m[:, 3], C.GENERAL_PRE), C.GENERAL_AVG)


def test_twin_general_matrix_falls_back_to_resample_then_average():
    got = D.deskew_with_matrix(torch.from_numpy(np.array(C.general_raw())), C.GENERAL_MATRIX, C.GENERAL_PRE, C.GENERAL_AVG).numpy()
    assert R.same_bits(got, general_expected())


AVG17 = dict(ls_angle_deg=30.0, px_to_scan_ratio=0.755, keep_overhang=False, average_n_slices=17)


@functools.lru_cache(maxsize=None)
def avg17_case():
    raw = np.random.default_rng(17).uniform(-50.0, 150.0, (60, 40, 9)).astype(np.float32)
    want = cpu_ref.deskew(raw, 30.0, 0.755, False, 17)
    raw.setflags(write=False)
    return raw, want


def test_average_of_17_slices_on_a_cpu_tensor():
    """The twin takes what the device takes (it refused more than 16)."""
    raw, want = avg17_case()
    got = D.fast_deskew_zyx(torch.from_numpy(np.array(raw)), **AVG17).numpy()
    assert got.shape == (3, 9, want.shape[2]) and R.same_bits(got, want)
    pre = np.zeros((4097, 1, 2), dtype=np.float32)
    assert D.average_n_slices(torch.from_numpy(pre), 4096).shape == (2, 1, 2)
    with pytest.raises(_lib.LsrError):
        D.average_n_slices(torch.from_numpy(pre), 4097)
