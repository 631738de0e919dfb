"""The DynaTrack estimator entries without a GPU: the blur dispatch query (``lsr_blur_reflect_form``) against the case
table, and every table of ``tests/estimators_ref.py`` through the host twins (``csrc/estimators_host.hip``) against the
float64 / exact restatements -- the assertions ``test_estimators_fp64_gpu.py`` makes of the kernels.  (``lsr_minmax_u16``
has no twin: its table is checked against the restatement alone.)
"""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import dynatrack as d
from tests import estimators_ref as R
from tests.estimators_backends import Twin, _f, form_of


@pytest.fixture(scope="module")
def twin():
    return Twin()


# ---------------------------------------------------------------------------------------------- the dispatch query
def test_blur_cases_reach_every_form_and_each_has_the_form_its_name_claims():
    reached = {}
    for case in R.BLUR_CASES:
        code = form_of(case)
        assert 0 <= code < len(R.FORMS), (case["name"], code)
        assert R.FORMS[code] == case["form"], f"{case['name']}: the launcher takes the {R.FORMS[code]} form"
        reached[R.FORMS[code]] = reached.get(R.FORMS[code], 0) + 1
    print("blur forms reached:", reached)
    assert set(reached) == set(R.FORMS)
    assert len({c["name"] for c in R.BLUR_CASES}) == len(R.BLUR_CASES)
    # the limits of each form, on both sides
    q = lambda *a: R.FORMS[_lib.call_value("lsr_blur_reflect_form", *a)]  # noqa: E731
    assert [q(40, 4, 64, 0, r, 0, 0) for r in (12, 13, 28, 29)] == ["marching", "packed", "packed", "tiled-64"]
    assert [q(200, 4, 64, 0, r, 0, 0) for r in (28, 29, 60, 61, 64)] == ["packed", "tiled-128", "tiled-128", "tiled-64", "tiled-64"]
    assert [q(L, 4, 64, 0, 12, 0, 0) for L in (31, 32)] == ["tiled-64", "marching"]
    assert [q(L, 4, 64, 0, 20, 0, 0) for L in (32, 33)] == ["tiled-64", "packed"]
    assert [q(L, 1, 63, 0, 20, 0, 0) for L in (64, 65)] == ["tiled-64", "tiled-128"]
    # alignment: the address modulo 16 of either array, or the alignment it is known to have
    assert [q(90, 6, 134, 0, 20, a, 0) for a in (0, 4, 8, 12, 16)] == ["packed", "tiled-128", "packed", "tiled-128", "packed"]
    assert q(90, 6, 134, 0, 20, 0, 4) == "tiled-128"
    assert q(3, 3, 3, 2, 2, 4, 4) == "contiguous"


def test_the_form_query_refuses_what_the_launcher_refuses():
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    lib = _lib.load()
    # Every argument set below must be one the launcher REFUSES: it is called with host pointers, and an accepted set
    # would launch a kernel on host memory.  Arguments that are accepted belong in R.BLUR_CASES, never here.
    for shape, axis, r in (((8, 9, 10), 0, 8), ((8, 9, 10), 1, 9), ((8, 9, 10), 2, 10), ((100, 100, 100), 0, 65),
                           ((8, 9, 10), 3, 1), ((8, 9, 10), -1, 1), ((8, 9, 10), 0, -1), ((0, 9, 10), 1, 1),
                           ((1 << 30, 4, 4), 1, 1)):
        code = _lib.call_value("lsr_blur_reflect_form", *shape, axis, r, 0, 0)
        assert code < 0, (shape, axis, r, code)
        # the launcher answers a refusal before its first HIP call (the pointers are host memory: nothing reads them)
        assert lib.lsr_blur_reflect_f32(p, p + 64, *shape, axis, p, r, _f(0), _f(0), None) == code, (shape, axis, r)
        # ... and the twin makes the same checks
        assert lib.lsr_blur_reflect_f32_cpu(p, p + 64, *shape, axis, p, r, _f(0), _f(0), None) == code, (shape, axis, r)
    assert _lib.call_value("lsr_blur_reflect_form", 8, 9, 10, 0, 7, 0, 0) >= 0


# ---------------------------------------------------------------------------------------------- twins vs restatements
@pytest.mark.parametrize("n", R.FLAT_N)
def test_minmax_f32(twin, n):
    for offset in R.FLAT_OFFSETS:
        R.check_minmax_f32(twin, n, offset)


@pytest.mark.parametrize("n", R.FLAT_N)
def test_histogram(twin, n):
    for nbins in R.HIST_BINS:
        for offset in R.FLAT_OFFSETS:
            R.check_histogram(twin, n, offset, nbins)


def test_histogram_rules(twin):
    R.check_histogram_rules(twin)


@pytest.mark.parametrize("n", R.U16_N)
def test_minmax_u16_table_against_the_restatement(n):
    """No twin to run: the restatement itself must see the planted extremes where the table says they are."""

    class Restated:
        def minmax_u16(self, x, offset):
            s = np.sort(x.astype(np.int64))
            return np.array([s[0], s[-1]], np.float32)

    names = R.u16_positions(n)
    assert names["first"] == 0 and names["last"] == n - 1
    if n >= 8:
        assert names["low_half"] % 2 == 0 and names["high_half"] % 2 == 1 and max(names["low_half"], names["high_half"]) < n // 8 * 8
    if n % 8 and n > 8:
        assert names["tail"] >= n // 8 * 8
    for offset in R.U16_OFFSETS:
        R.check_minmax_u16(Restated(), n, offset)


@pytest.mark.parametrize("kind", R.CENTROID_KINDS)
@pytest.mark.parametrize("shape", R.CENTROID_SHAPES, ids=str)
def test_centroid_sums(twin, shape, kind):
    print(f"{kind} {shape}: worst |got - fsum| / (N 2^-53 fsum) = {R.check_centroid(twin, shape, kind):.3g}")


@pytest.mark.parametrize("form", R.FORMS)
def test_blur(twin, form):
    cases = [c for c in R.BLUR_CASES if c["form"] == form]
    worst = max(R.check_blur(twin, c) for c in cases)
    print(f"{form}: {len(cases)} cases, worst |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("si,so", R.MATCH_CASES, ids=str)
def test_match_shape(twin, si, so):
    R.check_match(twin, si, so)


def test_match_shape_refuses_one_more_than_the_largest_pad(twin):
    with pytest.raises(_lib.LsrError, match="reflect-pad"):
        twin.match(np.zeros((5, 6, 7), np.float32), (14, 16, 19))


@pytest.mark.parametrize("into_b", (False, True))
@pytest.mark.parametrize("n", R.CROSS_N)
def test_cross_power(twin, n, into_b):
    print(f"n={n} into_b={into_b}: worst error / bound = {R.check_cross(twin, n, into_b):.3f}")


@pytest.mark.parametrize("shape", R.PEAK_SHAPES, ids=str)
def test_peak(twin, shape):
    R.check_peak(twin, shape)


# ---------------------------------------------------------------------------------------------- no finite sample
def test_a_volume_without_a_finite_sample(twin):
    """All NaN: the peak entry answers ~0 (-1) and ``lsr_minmax_f32`` (+inf, -inf) -- no sample ever replaces the
    starting values.  Neither reached the caller as such before: ``_percentile`` returned +inf as a percentile,
    ``_multiotsu_threshold`` got as far as the histogram entry's "range is empty", ``_binary_mask`` took the volume for
    a flat one, and ``_phase_cross_corr`` (which decodes the index of both the peak kernel and ``fft3.correlation_peak``)
    failed inside ``np.unravel_index``.  ``_minmax`` and ``_phase_cross_corr`` now raise a ValueError that names the cause."""
    nan = np.full((3, 4, 5), np.nan, np.float32)
    assert twin.peak(nan, 0) == -1 and twin.peak(nan, 1) == -1
    got = twin.minmax_f32(nan, 0)
    assert got[0] == np.inf and got[1] == -np.inf and np.array_equal(got, R.minmax(nan))
    vol = torch.from_numpy(nan)
    for call in (lambda: d._minmax(vol), lambda: d._percentile(vol, 50.0), lambda: d._multiotsu_threshold(vol),
                 lambda: d._binary_mask(vol, sigma=1.0), lambda: d._multiotsu_center_of_mass(vol, vol, sigma=1.0),
                 lambda: d._intensity_center_of_mass_to_roi_center(vol, background_percentile=50.0)):
        with pytest.raises(ValueError, match="no sample that is not NaN"):
            call()
    with pytest.raises(ValueError, match="no finite peak"):
        d._phase_cross_corr(vol, vol)
    ok = torch.ones(3, 4, 5)
    with pytest.raises(ValueError, match="no finite peak"):
        d._phase_cross_corr(ok, vol)
    # an infinite sample is a sample: the range is reported as it is
    assert d._minmax(torch.tensor([[[np.inf, 1.0, np.nan]]])) == (1.0, np.inf)
