"""The sliding-window passes at their dispatch edges, on the host twins: every case of ``tests/morphology_edge_cases.py`` --
grey morphology (``lsr_grey_morph_f32_cpu``) against ``scipy.ndimage`` element for element and the restated rule byte for byte,
the peak test of bead detection (``lsr_local_max_candidates_f32_cpu``) against an oracle that does not share the row kernel's
doubling spans, the box smoothing (``lsr_box_smooth_f32_cpu``) against scipy in float64 -- and the check that the cases still aim
at the edges the launches branch on (``test_the_cases_aim_at_the_dispatch``: a retuned constant fails there instead of moving
the edges away in silence).  ``tests/test_morphology_edges_gpu.py`` runs the same cases on the device.

The twins share the rule, the plan and ``walk_host`` with the kernels but neither the read-ahead of the strided walk, nor the row
kernel, nor the late mask of the peak sink: what this file pins is the rule at these shapes and the oracles themselves.
"""

import numpy as np
import pytest

from shrimpy_amd import _lib, psf
from shrimpy_amd import morphology as M
from tests import morphology_cases as C
from tests import morphology_edge_cases as E
from tests import psf_ref
from tests import test_morphology_host as H
from tests import test_psf_host as PH

GUARD = H.GUARD
POISON = -7

# one scratch buffer for every call of this module, never cleared between them (and poisoned to begin with)
SCRATCH = np.full(E.scratch_bytes_of_the_cases(), 0xA5, dtype=np.uint8)


def twin_morph(vol, r, op):
    """``test_morphology_host.twin_morph`` with this module's scratch (sized for the large case): (out, guard)."""
    z, y, x = vol.shape
    assert vol.dtype == np.float32 and vol.flags.c_contiguous
    assert 0 < _lib.call_value("lsr_grey_morph_scratch_bytes", z, y, x) <= SCRATCH.nbytes
    out = np.full(vol.size + GUARD, H.FILL, dtype=np.float32)
    before = vol.tobytes()
    _lib.call("lsr_grey_morph_f32_cpu", vol.ctypes.data, out.ctypes.data, z, y, x, *r, C.OPS.index(op), SCRATCH.ctypes.data, None)
    assert vol.tobytes() == before, "the input was written"
    return out[:vol.size].reshape(vol.shape), out[vol.size:]


# ---- grey morphology ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch", list(E.BATCHES))
def test_twin_equals_scipy_and_the_restatement_at_the_edges(batch):
    for case in E.BATCHES[batch]:
        for content in case.contents:
            vol = E.volume(case.shape, content)
            for op in case.ops:
                out, guard = twin_morph(vol, case.r, op)
                H.check_buffer(out, guard)
                E.check(case, content, op, out)


def test_the_digests_tell_what_the_comparisons_tell():
    a = np.array([0.0, -0.0, 1.0, np.nan, np.inf], dtype=np.float32)
    b = a.copy()
    b.view(np.uint32)[3] = 0xFFC00001                                    # another NaN: equal under both
    assert E.bytes_digest(a) == E.bytes_digest(b) and E.value_digest(a) == E.value_digest(b)
    b[0], b[1] = -0.0, 0.0                                               # the zeros swapped: equal values, other bytes
    assert E.bytes_digest(a) != E.bytes_digest(b) and E.value_digest(a) == E.value_digest(b)
    b[2] = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert E.value_digest(a) != E.value_digest(b)
    b = a.copy()
    b[3] = 5.0                                                           # a number where the NaN was
    assert E.bytes_digest(a) != E.bytes_digest(b) and E.value_digest(a) != E.value_digest(b)


def test_the_cases_aim_at_the_dispatch():
    """Recomputed here from ``tiling()`` and ``dispatch()`` alone: which instantiation of the strided walk each case selects,
    how many segments a row has, how many rows the busiest workgroup takes."""
    cap, columns, segment, _ = M.tiling()
    narrow, static, groups, *depths = M.dispatch()
    assert 1 < narrow and narrow + 1 < static and static + 1 < cap and len(set(depths)) == 3 and groups > 1
    assert (cap, columns, segment) == (E.CAP, E.COLUMNS, E.SEGMENT)

    def depth(r):
        return depths[0] if r <= narrow else (depths[1] if r <= static else depths[2])

    def segments(x):
        seg = -(-(-(-x // -(-x // segment))) // columns) * columns
        return -(-x // seg)

    def walked(case):                                      # (half-width, line length) of the case's one strided axis
        axis = 0 if case.r[0] else 1
        return case.r[axis], case.shape[axis]

    # every width of the row kernel and of the walk; the borders of the instantiations along y
    rows = [c for c in E.CASES if c.group == "rows-every-width"]
    assert {c.r[2] for c in rows if c.shape[2] == 2 * cap + 3} == set(range(1, cap + 1))
    narrow_row = {c.r[2] for c in rows if c.shape[2] == 5}
    assert {1, 2, 3, 4, 5, cap - 1, cap} <= narrow_row and all(c.r[:2] == (0, 0) for c in rows)
    assert all(any(v == 2 ** k + d for k in range(1, 12) for d in (-1, 0, 1)) for v in narrow_row)
    walks = [c for c in E.CASES if c.group == "walk-every-width"]
    assert {c.r[0] for c in walks if c.r[0]} == set(range(1, cap + 1))
    assert {c.r[1] for c in walks if c.r[1]} >= {narrow, narrow + 1, static, static + 1, cap}
    assert all(c.shape[2] == columns + 1 for c in walks), "a second workgroup with one live lane"
    per_depth = {u: sorted({walked(c)[0] for c in walks if depth(walked(c)[0]) == u}) for u in depths}
    for u, rs in per_depth.items():
        print(f"walk-every-width: {u} rows ahead at half-widths {rs[0]} .. {rs[-1]} ({len(rs)} of them)")
    assert [per_depth[u][0] for u in depths] == [1, narrow + 1, static + 1]
    assert [per_depth[u][-1] for u in depths] == [narrow, static, cap]

    # the read-ahead: per instantiation its first and last half-width, and the lengths around its depth and around w
    ahead = [c for c in E.CASES if c.group == "read-ahead"]
    seen = {}
    for c in ahead:
        r, n = walked(c)
        seen.setdefault((depth(r), "zy"[0 if c.r[0] else 1], r), set()).add(n)
        assert c.ops == tuple(C.OPS) and c.shape[2] == (columns + 1 if c.r[0] else 1)
    for (u, axis, r), lengths in sorted(seen.items()):
        print(f"read-ahead: {u} rows ahead, {axis}, half-width {r}: lengths {sorted(lengths)}")
        w = 2 * r + 1
        assert lengths >= {1, u - 1, u, u + 1, 2 * u - 1, 2 * u, 2 * u + 1, w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1} - {0}
    assert {(u, axis) for u, axis, _ in seen} == {(u, axis) for u in depths for axis in "zy"}
    assert {r for _, _, r in seen} == {1, narrow, narrow + 1, static, static + 1, cap}
    for batch, cases in E.BATCHES.items():
        if batch.startswith("read-ahead"):
            assert len({depth(walked(c)[0]) for c in cases}) == 1, f"{batch}: one instantiation per test"
    nan = E.volume((2 * cap + 1, 1, columns + 1), "nan")
    assert np.isnan(nan).sum() > 100 and len(set(nan.view(np.uint32)[np.isnan(nan)].tolist())) == 2

    # the row kernel: segments per row, rows per workgroup
    for c in (c for c in E.CASES if c.group in ("row-segments", "row-stride")):
        rows_in_group = -(-(c.shape[0] * c.shape[1]) // groups)
        print(f"{c.group} {c.shape} rx={c.r[2]}: {segments(c.shape[2])} segments per row, {rows_in_group} rows in the busiest workgroup")
        assert (segments(c.shape[2]), rows_in_group) == (E.segments(c.shape[2]), E.rows_of_the_busiest_workgroup(c.shape))
    assert {segments(c.shape[2]) for c in E.CASES if c.group == "row-segments"} == {1, 2, 3}
    assert {c.r[2] for c in E.CASES if c.group == "row-segments"} == {1, cap}
    stride = [c for c in E.CASES if c.group == "row-stride"]
    assert {-(-(c.shape[0] * c.shape[1]) // groups) for c in stride} == {1, 2, 3}
    second_row_of_two_segments = [c for c in stride if segments(c.shape[2]) == 2 and c.shape[0] * c.shape[1] > groups]
    assert {c.r[2] for c in second_row_of_two_segments} == {1, cap}
    assert all({"grey_erosion", "white_tophat", "black_tophat"} <= set(c.ops) for c in second_row_of_two_segments)
    assert sum(int(np.prod(c.shape)) > 70000 for c in E.CASES) == len(second_row_of_two_segments) == 4, "one large shape"
    assert all(c.restate for c in E.CASES if c not in second_row_of_two_segments), "... and it alone is held to scipy alone"

    # the box smoothing: one axis at the mirror's limit, the greatest tap count the entry takes
    assert max(E.BOX_TAPS) == 2 * psf.MAX_HALF_WIDTH + 1 and all(min(E.box_shape(b)) == b // 2 + 1 for b in E.BOX_TAPS)


# ---- the peak sink --------------------------------------------------------------------------------------------------------------


def twin_peaks(s, r, threshold, capacity):
    """The twin through the C ABI into poisoned index and value buffers with 64 guard words behind each."""
    index = np.full(capacity + GUARD, POISON, dtype=np.int64)
    value = np.full(capacity + GUARD, POISON, dtype=np.float32)
    count = np.full(1, 12345, dtype=np.uint64)
    before = s.tobytes()
    _lib.call("lsr_local_max_candidates_f32_cpu", s.ctypes.data, *s.shape, *r, threshold, index.ctypes.data, value.ctypes.data,
              capacity, count.ctypes.data, None, None)
    assert s.tobytes() == before, "the input was written"
    return int(count[0]), index, value


def hold_peaks(run, case):
    """Shared with the device test: the peak set, the values and the count equal the oracle's exactly -- once with the buffers
    exactly full, once with one slot too few (the count runs over, nothing is written past the capacity)."""
    s = E.peak_volume(case.shape, case.content)
    want = E.expected_peaks(case)
    n = len(want)
    count, index, value = run(s, case.r, case.threshold, max(n, 1))
    assert count == n, f"{case}: {count} peaks, the oracle has {n}"
    order = np.argsort(index[:n])
    assert np.array_equal(index[:n][order], want), case
    assert value[:n][order].tobytes() == s.ravel()[want].tobytes(), case
    assert np.all(index[n:] == POISON) and np.all(value[n:] == POISON), f"{case}: written past the last peak"
    if n >= 2:
        count, index, value = run(s, case.r, case.threshold, n - 1)
        assert count == n, f"{case}: the count must run over the capacity"
        got = index[:n - 1]
        assert len(set(got.tolist())) == n - 1 and np.isin(got, want).all(), case
        assert value[:n - 1].tobytes() == s.ravel()[got].tobytes(), case
        assert np.all(index[n - 1:] == POISON) and np.all(value[n - 1:] == POISON), f"{case}: written past the capacity"
    return n


@pytest.mark.parametrize("batch", list(E.PEAK_BATCHES))
def test_twin_peaks_equal_an_independent_oracle(batch):
    _lib.call("lsr_set_host_threads", 4)
    found = [hold_peaks(twin_peaks, case) for case in E.PEAK_BATCHES[batch]]
    assert sum(n >= 2 for n in found) > len(found) // 2, "most cases must reach the overflow run"


@pytest.mark.parametrize("batch", list(E.PEAK_BATCHES))
def test_the_scipy_peak_oracle_agrees_with_the_literal_one(batch):
    small = [c for c in E.PEAK_BATCHES[batch] if E.peak_oracle_is_literal(c.shape)]
    assert len(small) >= len(E.PEAK_BATCHES[batch]) // 2
    for case in small:
        mask = E.peak_mask_scipy(E.peak_volume(case.shape, case.content), case.r, case.threshold)
        assert np.array_equal(np.flatnonzero(mask), E.expected_peaks(case)), case


def test_the_peak_cases_aim_at_the_late_mask():
    narrow, static, _, *depths = M.dispatch()

    def depth(r):
        return depths[0] if r <= narrow else (depths[1] if r <= static else depths[2])

    # the peak sink: both instantiations it meets, the z walk alone and behind the x and y passes, every late bit
    assert max(E.PEAK_RZ) <= psf.MAX_HALF_WIDTH
    assert {depth(rz) for rz in E.PEAK_RZ} == set(depths[:2]) and {0, narrow, narrow + 1} <= set(E.PEAK_RZ)
    for rz in E.PEAK_RZ:
        u = depth(rz)
        print(f"peak-sink: rz {rz}: {u} rows ahead, lengths {E.peak_lengths(rz)}")
        assert set(E.peak_lengths(rz)) >= {1, u, u + 1, 2 * u + 1, 2 * rz + 3}
    assert {c.r[1:] for c in E.PEAK_CASES} == {(0, 0), (1, 2)} and {c.shape[1] for c in E.PEAK_CASES} == {1, 3}
    for c in E.PEAK_CASES:
        lin = E.expected_peaks(c)
        z = np.unravel_index(lin, c.shape)[0]
        u = depth(c.r[0])
        if c.content == "constant":                      # every voxel passes maximum(): every bit of every group is set
            at = np.indices(c.shape)
            first = np.all([at[a] == 0 for a in range(3) if c.r[a]] or [np.ones(c.shape, dtype=bool)], axis=0)
            assert np.array_equal(lin, np.flatnonzero(first)), c
        if c.content == "staircase" and c.threshold == 0.0 and c.r[1:] == (0, 0) and c.shape[0] >= u:
            assert len(lin) == c.shape[1] * c.shape[2], "a peak per column"
            assert {int(v) % u for v in z + c.r[0]} == set(range(u)), f"{c}: a peak at every bit of the late mask"
    assert any(len(E.expected_peaks(c)) >= 2 for c in E.PEAK_CASES if c.content == "inf" and c.threshold == np.inf)
    assert sum(not E.peak_oracle_is_literal(c.shape) for c in E.PEAK_CASES) >= 20, "the scipy oracle is in use"


# ---- the box smoothing ----------------------------------------------------------------------------------------------------------


def hold_box_smoothing(device):
    """Shared with the device test.  Every figure is printed before anything is asserted; returns the smoothed volumes."""
    worst, out = {}, {}
    for b in E.BOX_TAPS:
        shape = E.box_shape(b)
        v = PH.noisy(shape, b)
        assert v.min() > 0.0
        got = psf.smooth(PH._t(v, device), b).cpu().numpy()
        want = psf_ref.smooth(v, b)
        worst[b] = float((np.abs(got.astype(np.float64) - want) / np.abs(want)).max() / PH.U)
        print(f"{b} taps on {shape}: smoothing off by {worst[b]:.3f} units of 2^-24 relative")
        out[b] = got
    assert max(worst.values()) <= PH.SMOOTH_BOUND_U, worst
    return out


def test_twin_box_smoothing_at_the_mirrors_limit():
    _lib.call("lsr_set_host_threads", 4)
    hold_box_smoothing(PH.CPU)
