"""The host twins of the two mutual-information kernels against ``tests/mi_ref.py`` on every case of
``tests/mi_edge_cases.py``, and the checks of the cases themselves: the integer proofs of the exact cases and what each
case must contain (sample counts against the launch size, kinds of u, cells, waves, coordinates on the keep limits).
``test_mi_fp64_gpu.py`` runs the same cases on the device.

Exact and edge cases: equal histograms and counts, bit-equal gradient sums.  Bound cases: the histogram within the
existing 2 n units, the gradient within ``mi_ref.gradient_bound``.  Measured worst fraction of that bound for the twin:
8.5e-5, 2.5e-4, 8.7e-5 on the three general cases (bins 8, 32, 64), 1.6e-5 on the two-trip scene, the same with
``hist=None`` and with the restatement's histogram; every histogram of a bound case came out equal cell for cell."""

import numpy as np
import pytest

from tests import mi_edge_cases as cases
from tests import mi_ref as ref

_ID = dict(ids=lambda c: c.name)


def _t(a):
    import torch

    return torch.as_tensor(np.array(a, dtype=np.float32))


def _twin_histogram(mov, tgt, m, stride, bins, ranges):
    from shrimpy_amd.estimate import joint_histogram

    return joint_histogram(_t(mov), _t(tgt), m, stride, bins, ranges)


def _twin_rows(mov, tgt, case, ranges):
    """The twin's raw (blocks, 12) rows at the synthetic ``dl``, written into a NaN-filled buffer."""
    import torch

    partial = torch.full((cases.blocks(), 12), float("nan"), dtype=torch.float64)
    dl = torch.as_tensor(cases.synthetic_dl(case.bins))
    cases.raw_gradient(_t(mov), _t(tgt), case.m, case.stride, case.centre, cases.SCALE, case.bins, ranges, dl, partial)
    return partial.numpy()


# ---------------------------------------------------------------------------------------------------- the cases themselves


def test_sample_counts_sit_on_the_launch_edges():
    t = cases.launch_threads()
    by_name = {c.name: c.grid_samples for c in cases.EXACT_CASES}
    want = {"one-sample": 1, "wave-less-one": 63, "one-wave": 64, "wave-plus-one": 65, "workgroup-less-one": 255,
            "one-workgroup": 256, "workgroup-plus-one": 257, "every-thread-but-one": t - 1, "every-thread-once": t,
            "one-sample-on-the-second-trip": t + 1, "second-trip-of-workgroup-0": t + 256}
    assert {k: by_name[k] for k in want} == want
    assert 2 * t < by_name["ragged-third-trip"] < 3 * t and by_name["ragged-third-trip"] % cases.THREADS != 0
    assert all(5 * t < by_name[f"five-trips-bins-{b}"] <= 700_000 for b in cases.ALL_BINS)
    assert max(by_name.values()) <= 700_000
    assert by_name["band-outside"] < t
    # strides: none divides its axis; one exceeds its axis; three different ones
    for c in cases.STRIDE_CASES[:2]:
        assert len(set(c.stride)) == 3
    assert all(n % s for n, s in zip(cases.BIG_TARGET, cases.STRIDE_CASES[0].stride))
    assert cases.STRIDE_CASES[1].stride[0] > cases.BIG_TARGET[0] and cases.STRIDE_CASES[2].stride[1] > cases.BIG_TARGET[1]
    # every bin count on a multi-trip case, the smallest and the largest the entries accept among them
    assert {c.bins for c in cases.EXACT_CASES if c.grid_samples > t} >= set(cases.ALL_BINS)


@pytest.mark.parametrize("case", cases.EXACT_CASES, **_ID)
def test_exact_case_is_exact_and_holds_what_it_is_for(case):
    """The integer proof: u, the weights and every gradient term are float64 without rounding, and no partial sum in any
    order needs more than 53 bits.  Then the properties the case exists for, from the restatement alone."""
    mov, tgt = cases.inputs(case)
    assert mov.shape == case.moving_shape and tgt.shape == case.target_shape
    assert np.array_equal(mov, np.rint(mov)) and np.array_equal(tgt, np.rint(tgt)) and np.abs(mov).max() <= 20
    assert np.array_equal(case.m * 8, np.rint(case.m * 8))
    r = cases.rows(case)
    n = r.tv.size
    assert len(r.keep) == case.grid_samples and n == r.keep.sum()
    # values: multiples of 2^-9 (three lerps by eighths); u and f * 65536: exact in float64 because they are exact in
    # extended precision as well
    assert np.array_equal(r.mval * 512, np.rint(r.mval * 512))
    a, b0, u_raw, f = ref.bin_rule(r.tv, r.mval, case.bins, cases.RANGES)
    wide = (r.mval.astype(np.longdouble) - cases.M_RANGE[0]) * (case.bins - 1) / (cases.M_RANGE[1] - cases.M_RANGE[0])
    assert np.array_equal(wide, u_raw.astype(np.longdouble))
    assert np.array_equal(f * 65536.0, np.rint(f * 65536.0))
    hist, n_hist = cases.expected_histogram(case)
    assert n_hist == n and int(hist.sum()) == 65536 * n
    if case.gradient:
        t = cases.expected_terms(case)
        sums, bits = ref.exact_integer_terms(t.terms, cases.EXACT_BITS)
        assert np.array_equal(sums, t.sums), case.name
        # three more orders: forwards, backwards, by owner
        assert np.array_equal(t.terms.sum(axis=0), sums) and np.array_equal(t.terms[::-1].cumsum(axis=0)[-1], sums)
        assert np.array_equal(ref.sums_by_owner(t.terms, t.index, cases.blocks()).sum(axis=0), sums)
        assert np.any(sums != 0)
        kinds = ref.u_kinds(u_raw, case.bins)
        print(f"{case.name}: n {n} of {case.grid_samples}, widest sum {bits} bits, {kinds}")
        if case.kinds:
            assert min(kinds[k] for k in ("below", "zero", "inside", "top", "above")) > 0 and kinds["nan"] == 0, kinds
            # a sample exactly on an end of the range has a gradient to lose
            gsum = np.abs(r.g).sum(axis=0)
            assert np.any((u_raw == 0) & (gsum > 0)) and np.any((u_raw == case.bins - 1) & (gsum > 0))
            # dl differs along both axes where the samples are: a wrong row stride would show
            used = np.zeros((case.bins, case.bins - 1), bool)
            used[a[t.inside], b0[t.inside]] = True
            assert used.sum() >= min(case.bins, 8)
    if case.trips is not None:
        assert (r.index.max() // cases.launch_threads()) + 1 == case.trips      # a KEPT sample on the last trip
    if case.bins == 64 and case.grid_samples > cases.launch_threads():
        assert hist[63, 63] > 0 and hist[0, 0] > 0
        assert np.any(t.inside & (a == 63) & (b0 == 62)), "the last dL entry is never read"


def test_band_case_has_idle_waves_partial_waves_an_idle_workgroup_and_the_keep_limits():
    case = next(c for c in cases.GEOMETRY_CASES if c.name == "band-outside")
    r = cases.rows(case)
    assert case.moving_shape != case.target_shape
    keep = np.concatenate([r.keep, np.zeros(-len(r.keep) % cases.WAVE, bool)]).reshape(-1, cases.WAVE).sum(axis=1)
    full_waves = len(r.keep) // cases.WAVE
    assert (keep[:full_waves] == 0).any() and ((keep[:full_waves] > 0) & (keep[:full_waves] < cases.WAVE)).any()
    assert (keep == cases.WAVE).any()
    own = ref.owner(np.arange(len(r.keep)), cases.blocks())
    has, kept = np.bincount(own, minlength=cases.blocks()), np.bincount(own, weights=r.keep, minlength=cases.blocks())
    assert ((has == cases.THREADS) & (kept == 0)).any(), "no workgroup whose 256 samples are all outside"
    for axis, size in enumerate(case.moving_shape):
        others = np.ones(len(r.keep), bool)
        for k, other in enumerate(case.moving_shape):
            if k != axis:
                others &= (r.coord[k] >= 0) & (r.coord[k] < other - 1)
        assert (r.keep & (r.coord[axis] == 0.0)).any(), f"axis {axis}: no kept sample at exactly 0"
        assert (others & (r.coord[axis] == size - 1) & ~r.keep).any(), f"axis {axis}: no sample at exactly n - 1"


def test_contention_cases_put_a_wave_in_one_cell_and_in_64_cells():
    one, many = cases.CONTENTION_CASES
    for case, distinct in ((one, 1), (many, cases.WAVE)):
        r = cases.rows(case)
        assert r.keep.all() and len(r.keep) % cases.WAVE == 0
        a, b0, _, f = ref.bin_rule(r.tv, r.mval, case.bins, cases.RANGES)
        cell = (a * case.bins + b0).reshape(-1, cases.WAVE)
        assert all(len(set(row)) == distinct for row in cell.tolist()), case.name
        if distinct == 1:
            w1 = np.floor(f * 65536.0 + 0.5)
            assert np.all((w1 > 0) & (w1 < 65536))            # both adds of every lane land on contended cells
            assert len(set(cell[:, 0].tolist())) > 1


@pytest.mark.parametrize("case", cases.EDGE_CASES, **_ID)
def test_edge_case_holds_what_it_is_for(case):
    launch, tgt, expect = cases.edge_inputs(case)
    r = cases.edge_rows(case)
    hist, n, t = cases.edge_expected(case)
    if case.n is not None:
        assert n == case.n
    assert int(hist.sum()) == 65536 * n
    sums, _ = ref.exact_integer_terms(t.terms, cases.EXACT_BITS)
    assert np.array_equal(sums, t.sums)
    bad = [w for w, v in case.moving_at if not np.isfinite(v)]
    if case.launch_only:
        touched = np.zeros(case.moving_shape, bool)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    touched[r.cell[0] + dz, r.cell[1] + dy, r.cell[2] + dx] = True
        assert bad and not any(touched[w] for w in bad) and not np.isfinite(launch).all() and np.isfinite(expect).all()
    elif bad:
        # every value that is not finite is a tap of a sample with fx == 0 -- as the far tap, which 0 multiplies -- and of
        # a sample with fx != 0
        for (z, y, x) in bad:
            inside_zy = (r.cell[0] <= z) & (z <= r.cell[0] + 1) & (r.cell[1] <= y) & (y <= r.cell[1] + 1)
            assert (inside_zy & (r.cell[2] + 1 == x) & (r.frac[2] == 0)).any(), (case.name, "fx == 0")
            assert (inside_zy & (r.cell[2] + 1 == x) & (r.frac[2] != 0)).any(), (case.name, "fx != 0")
        assert np.isnan(r.mval).any()
        assert hist[:, 0].sum() > 0
    if case.name == "target-nan-inf-zero-and-range-ends":
        a, _, _, _ = ref.bin_rule(r.tv, r.mval, case.bins, case.ranges)
        lookup = {tuple(int(v) for v in r.idx[:, k]): int(a[k]) for k in range(n)}
        got = [lookup[w] for w, _ in case.target_at]
        assert got == [0, case.bins - 1, 0, 0, 0, case.bins - 1, 0, case.bins - 1]
    if case.name == "negative-zero":
        assert np.signbit(launch).any() and np.signbit(tgt).any()


# ---------------------------------------------------------------------------------------------------- twins against mi_ref


@pytest.mark.parametrize("case", cases.EXACT_CASES, **_ID)
def test_twins_equal_the_restatement_on_an_exact_case(case):
    mov, tgt = cases.inputs(case)
    want, n_want = cases.expected_histogram(case)
    got, n = _twin_histogram(mov, tgt, case.m, case.stride, case.bins, cases.RANGES)
    assert n == n_want
    assert np.array_equal(got, want), (case.name, np.argwhere(got != want)[:4].tolist())
    if case.gradient:
        t = cases.expected_terms(case)
        part = _twin_rows(mov, tgt, case, cases.RANGES)
        assert not np.isnan(part).any()
        assert np.array_equal(part.sum(axis=0), t.sums), (case.name, part.sum(axis=0), t.sums)


@pytest.mark.parametrize("case", cases.EDGE_CASES, **_ID)
def test_twins_equal_the_restatement_on_an_edge_case(case):
    launch, tgt, _ = cases.edge_inputs(case)
    want, n_want, t = cases.edge_expected(case)
    got, n = _twin_histogram(launch, tgt, case.m, case.stride, case.bins, case.ranges)
    assert n == n_want
    assert np.array_equal(got, want), (case.name, np.argwhere(got != want)[:4].tolist())
    part = _twin_rows(launch, tgt, case, case.ranges)
    assert not np.isnan(part).any()
    assert np.array_equal(part.sum(axis=0), t.sums), (case.name, part.sum(axis=0), t.sums)
    if n == 0:
        assert not got.any() and not part.any()


@pytest.mark.parametrize("case", cases.BOUND_CASES, **_ID)
def test_twins_are_within_the_a_priori_bound(case):
    from shrimpy_amd.estimate import mi_gradient

    mov, tgt, m, ranges, centre, scale = cases.bound_inputs(case)
    r = cases.bound_rows(case)
    want_hist, n = cases.histogram_of(r, case.bins, ranges)
    hist, n_twin = _twin_histogram(mov, tgt, m, case.stride, case.bins, ranges)
    assert n_twin == n and n > 500
    off = int(np.abs(hist.astype(np.int64) - want_hist.astype(np.int64)).sum())
    assert off <= 2 * n
    for label, given, used in (("hist=None", None, hist), ("the restatement's hist", want_hist, want_hist)):
        want, bound = cases.bound_expected(case, used)
        got = mi_gradient(_t(mov), _t(tgt), m, case.stride, case.bins, ranges, given, centre, scale)
        fraction = ref.worst_fraction(got, want, bound)
        print(f"{case.name}, {label}: n {n}, histogram off by {off} units, worst fraction of the a-priori bound {fraction:.3e}")
        assert np.abs(want).max() > 0
        assert fraction <= 1.0
