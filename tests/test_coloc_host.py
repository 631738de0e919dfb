"""Colocalization on the CPU: the host twins (``lsr_label_coloc_f32_cpu`` / ``_u16_cpu``) against the numpy restatement
(``tests/coloc_ref.py``) on every case of ``tests/coloc_cases.py`` at every threshold and grid cap -- uint16 byte for byte, float32
exactly in the counts and within ``m 2^-53 sum|terms|`` in the sums; guards and the entry checks; ``coefficients`` against exact
rational arithmetic and scipy; a scene with known answers; Costes' thresholds against the restatement.  PARITY UNPINNED: the rule
of ``csrc/coloc.hpp`` is the specification."""

import fractions
import math

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import colocalize as K
from tests import coloc_cases as C
from tests import coloc_ref as R

GUARD = 64
FILL = -7
WORDS = 16                            # a record in 64-bit words
E_ARG, E_UNSUPPORTED = -4, -3         # include/lsrecon.h
LDS_SLOTS, DEFAULT_BLOCKS = K.coloc_geometry()
U = 2.0 ** -53


def guarded(n):
    """``n`` zeroed records between two guards of 64 words of -7."""
    buf = np.full((2 * GUARD + WORDS * n,), FILL, dtype=np.int64)
    buf[GUARD:GUARD + WORDS * n] = 0
    return buf


def split(buf, n, dtype):
    return buf[GUARD:GUARD + WORDS * n].view(dtype), np.concatenate([buf[:GUARD], buf[GUARD + WORDS * n:]])


def twin_coloc(labels, a, b, n, thresholds=(0.0, 0.0), max_blocks=0):
    """The twin through the C ABI, by the channels' type: (records, guards).  ``labels`` may be None."""
    z, y, x = a.shape
    f32 = a.dtype == np.float32
    buf = guarded(n)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    labels = None if labels is None else np.ascontiguousarray(labels)
    _lib.call("lsr_label_coloc_f32_cpu" if f32 else "lsr_label_coloc_u16_cpu", None if labels is None else labels.ctypes.data,
              a.ctypes.data, b.ctypes.data, z, y, x, n, thresholds[0], thresholds[1], buf[GUARD:].ctypes.data, max_blocks, None)
    return split(buf, n, K.COLOC_DTYPE_F32 if f32 else K.COLOC_DTYPE_U16)


def entry_check_calls(labels_ptr, a_ptr, b_ptr, table_ptr):
    """``(what, status, arguments)`` of every call the entry must refuse, for a (2, 3, 4) volume and a table of 8 records.  Every
    pointer is valid for the stated shape, except where the shape itself is what is refused before anything is read."""
    ok = dict(labels=labels_ptr, a=a_ptr, b=b_ptr, Z=2, Y=3, X=4, n=8, ta=0.0, tb=0.0, table=table_ptr, max_blocks=0)
    bad = [("a is NULL", E_ARG, dict(a=None)), ("b is NULL", E_ARG, dict(b=None)), ("table is NULL", E_ARG, dict(table=None)),
           ("an empty shape", E_ARG, dict(Z=0)), ("a negative extent", E_ARG, dict(X=-1)), ("n -1", E_ARG, dict(n=-1)),
           ("no labels and n 8", E_ARG, dict(labels=None)), ("no labels and n 0", E_ARG, dict(labels=None, n=0)),
           ("ta is NaN", E_ARG, dict(ta=math.nan)), ("tb is NaN", E_ARG, dict(tb=math.nan)),
           ("max_blocks -1", E_ARG, dict(max_blocks=-1)),
           ("table is labels", E_ARG, dict(table=labels_ptr)), ("table inside labels", E_ARG, dict(table=labels_ptr + 16)),
           ("table is a", E_ARG, dict(table=a_ptr)), ("table inside a", E_ARG, dict(table=a_ptr + 8)),
           ("table is b", E_ARG, dict(table=b_ptr)), ("table inside b", E_ARG, dict(table=b_ptr + 8)),
           ("2^31 voxels", E_UNSUPPORTED, dict(Z=1 << 11, Y=1 << 10, X=1 << 10))]
    for what, status, change in bad:
        k = dict(ok, **change)
        yield what, status, (k["labels"], k["a"], k["b"], k["Z"], k["Y"], k["X"], k["n"], k["ta"], k["tb"], k["table"],
                             k["max_blocks"])


# ---------------------------------------------------------------- the ABI


def test_the_records_are_128_bytes_and_the_geometry_is_sane():
    assert K.COLOC_DTYPE_F32.itemsize == 128 and K.COLOC_DTYPE_U16.itemsize == 128
    assert K.COLOC_DTYPE_F32 == R.DTYPE_F32 and K.COLOC_DTYPE_U16 == R.DTYPE_U16
    assert K.COLOC_DTYPE_F32.names == R.FIELDS == K.COLOC_FIELDS
    assert [K.COLOC_DTYPE_F32.fields[f][1] // 8 for f in R.COUNTS] == [0, 6, 12, 13]
    assert LDS_SLOTS >= 64 and LDS_SLOTS & (LDS_SLOTS - 1) == 0 and DEFAULT_BLOCKS >= 1
    for name in ("COLOC_DTYPE_F32", "COLOC_DTYPE_U16", "coloc_geometry", "pair_table", "coefficients", "costes_thresholds"):
        assert name in K.__all__


def test_census_of_the_cases():
    """The label side is what ``tests/moments_cases.py`` claims at THIS kernel's slots, and the value side is what it claims."""
    for shape, content in C.MANY_LABELS:
        labels, n = C.labels_of(shape, content, LDS_SLOTS)
        assert n == 4 * LDS_SLOTS
        for cap in C.CAPS:
            flat = labels.ravel()
            distinct = [len(np.unique(flat[a:b][flat[a:b] > 0])) for a, b in C.M.spans(flat.size, cap, DEFAULT_BLOCKS)]
            assert max(distinct) > LDS_SLOTS, f"{shape} cap {cap}: no span holds more labels than the LDS table has slots"
    # whole wave steps of one label (the register path), of no label, and of several runs all occur
    for shape, content, least_uniform, least_mixed in (((3, 7, 1030), "one-label", 300, 0), ((3, 7, 1030), "runs", 30, 100),
                                                       ((3, 7, 1030), "random-0..5", 0, 300)):
        labels, n = C.labels_of(shape, content, LDS_SLOTS)
        flat = np.r_[labels.ravel(), np.zeros(-labels.size % 64, np.int32)].reshape(-1, 64)
        uniform = (flat == flat[:, :1]).all(axis=1) & (flat[:, 0] != 0)
        assert uniform.sum() >= least_uniform and (~uniform).sum() >= least_mixed, (content, uniform.sum(), (~uniform).sum())
    shape, content = C.ROW_CROSSING[2]
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    a, b = C.pair_f32(shape, content, LDS_SLOTS, "non-finite")
    assert np.isnan(a).sum() == 1 and np.isinf(a).sum() == 2 and len(np.unique(labels[~np.isfinite(a)])) == 1
    assert np.isfinite(b).all()
    a, b = C.pair_f32(shape, content, LDS_SLOTS, "signed-zeros")
    assert not a.any() and not b.any() and np.signbit(a).any() and not np.signbit(b).all()
    a, b = (v.astype(np.float64) for v in C.pair_f32(shape, content, LDS_SLOTS, "cancelling"))
    assert abs(a.sum()) <= 1e-6 * np.abs(a).sum() and abs(b.sum()) <= 1e-2 * np.abs(b).sum() and (a * b < 0).any() and (a * b > 0).any()
    # "at-value": both thresholds occur, so `>` and `>=` differ
    for a, b in (C.pair_f32(shape, content, LDS_SLOTS, "independent"), C.pair_u16(shape, content, "random")):
        ta, tb = C.thresholds_of(a, b, "at-value")
        assert (a == ta).any() and (b == tb).any() and 0 < (a > ta).sum() < a.size
    a, b = C.pair_u16(shape, content, "equal")
    assert np.array_equal(a, b) and len(np.unique(a)) > 1000


# ---------------------------------------------------------------- the table


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_u16_equals_the_restatement(shape, content):
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    for kind in C.PAIRS_U16:
        a, b = C.pair_u16(shape, content, kind)
        for name in C.THRESHOLDS_U16:
            want = C.want_u16(shape, content, LDS_SLOTS, kind, name)
            for cap in C.CAPS:
                rows, guards = twin_coloc(labels, a, b, n, C.thresholds_of(a, b, name), cap)
                assert np.all(guards == FILL), f"{kind}, {name}, cap {cap}: the twin wrote outside the table"
                assert rows.tobytes() == want.tobytes(), f"{kind}, {name}, cap {cap}"


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_f32_is_within_the_bound_of_the_restatement(shape, content):
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    worst = 0.0
    for kind in C.PAIRS_F32:
        a, b = C.pair_f32(shape, content, LDS_SLOTS, kind)
        for name in C.THRESHOLDS_F32:
            want = C.want_f32(shape, content, LDS_SLOTS, kind, name)
            rows, guards = twin_coloc(labels, a, b, n, C.thresholds_of(a, b, name))
            assert np.all(guards == FILL), f"{kind}, {name}: the twin wrote outside the table"
            worst = max(worst, C.check_f32(rows, want, f"{kind}, {name}"))
    print(f"worst error / bound = {worst:.3g}")


def test_the_strict_comparison_and_the_extreme_thresholds():
    shape, content = (5, 9, 130), "random-0..5"
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    for a, b in (C.pair_f32(shape, content, LDS_SLOTS, "independent"), C.pair_u16(shape, content, "random")):
        inside = (labels >= 1) & (labels <= n)
        ta, tb = float(a[inside][0]), float(b[inside][-1])              # values that occur inside the objects
        rows, _ = twin_coloc(labels, a, b, n, (ta, tb))
        assert rows["count_A"].sum() == (inside & (a > ta)).sum() < (inside & (a >= ta)).sum()
        assert rows["count_B"].sum() == (inside & (b > tb)).sum() < (inside & (b >= tb)).sum()
        rows, _ = twin_coloc(labels, a, b, n, (-np.inf, -np.inf))
        for f, g in (("count_both", "count"), ("both_ab", "sum_ab"), ("a_where_B", "sum_a"), ("b_where_A", "sum_b")):
            assert np.array_equal(rows[f], rows[g])
        rows, _ = twin_coloc(labels, a, b, n, (np.inf, 0.0))
        for f in ("count_both", "count_A", "both_a", "both_ab", "b_where_A"):
            assert not rows[f].any()
        assert rows["count_B"].sum() == (inside & (b > 0)).sum() and rows["a_where_B"].any()


def test_non_finite_voxels_stay_in_their_object():
    """``+inf``, ``-inf`` and a NaN in channel a of one object: its sums of a are NaN, its sums of b alone are finite, where the
    NaN is masked out (it is never above a threshold) the sum follows the infinities alone; every other object is finite."""
    shape, content = C.ROW_CROSSING[2]
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    a, b = C.pair_f32(shape, content, LDS_SLOTS, "non-finite")
    hit = int(labels[np.isnan(a)][0]) - 1
    rows, _ = twin_coloc(labels, a, b, n, (-np.inf, -np.inf))
    got = C.sums_of(rows)
    others = np.arange(n) != hit
    assert np.isfinite(got[others]).all()
    for f in ("sum_a", "sum_aa", "sum_ab", "a_where_B"):
        assert np.isnan(rows[f][hit]), f
    for f in ("sum_b", "sum_bb", "both_b", "both_bb", "b_where_A"):
        assert np.isfinite(rows[f][hit]), f
    # above -inf: +inf is, -inf and the NaN are not, so the sums over "both" hold +inf alone
    assert rows["both_a"][hit] == np.inf and rows["both_aa"][hit] == np.inf
    assert rows["count_A"][hit] == rows["count"][hit] - 2


def test_no_objects():
    labels = np.ones((2, 3, 4), dtype=np.int32)
    for dtype in (np.float32, np.uint16):
        a = np.ones((2, 3, 4), dtype)
        rows, guards = twin_coloc(labels, a, a.copy(), 0)
        assert len(rows) == 0 and np.all(guards == FILL)
        assert len(K.pair_table(torch.from_numpy(labels), 0, torch.from_numpy(a), torch.from_numpy(a.copy()))) == 0


# ---------------------------------------------------------------- the entry checks


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_entry_checks(u16):
    labels = np.ones((2, 3, 4), dtype=np.int32)
    a = np.ones((2, 3, 4), dtype=np.uint16 if u16 else np.float32)
    b = a.copy()
    table = np.zeros((8 * WORDS,), dtype=np.int64)
    entry = "lsr_label_coloc_u16_cpu" if u16 else "lsr_label_coloc_f32_cpu"
    for what, status, args in entry_check_calls(labels.ctypes.data, a.ctypes.data, b.ctypes.data, table.ctypes.data):
        with pytest.raises(_lib.LsrError) as err:
            _lib.call(entry, *args, None)
        assert err.value.code == status, what
        assert not table.any(), f"{what}: something was written"
    assert (labels == 1).all() and (a == 1).all() and (b == 1).all()


def test_python_argument_checks():
    labels = torch.ones((2, 3, 4), dtype=torch.int32)
    a = torch.ones((2, 3, 4), dtype=torch.float32)
    with pytest.raises(TypeError):
        K.pair_table(labels.to(torch.int64), 1, a, a)
    with pytest.raises(TypeError):
        K.pair_table(labels, 1, a, a.to(torch.uint16))
    with pytest.raises(TypeError):
        K.pair_table(labels, 1, a.to(torch.float64), a.to(torch.float64))
    with pytest.raises(TypeError):
        K.pair_table(labels, 1, a.numpy(), a)
    with pytest.raises(ValueError):
        K.pair_table(labels, -1, a, a)
    with pytest.raises(ValueError):
        K.pair_table(None, 2, a, a)
    with pytest.raises(ValueError):
        K.pair_table(labels, 1, a, a[:, :2])
    with pytest.raises(ValueError):
        K.pair_table(labels, 1, a, a, thresholds=(0.0, math.nan))
    with pytest.raises(ValueError):
        K.costes_thresholds(labels, 1, a, a, region="object")
    with pytest.raises(ValueError):
        K.costes_thresholds(None, 1, a, a, region="labelled")
    with pytest.raises(TypeError):
        K.coefficients(np.zeros((3,), np.float64))


# ---------------------------------------------------------------- the coefficients


def _tensor(arr):
    return None if arr is None else torch.from_numpy(np.array(arr))


@pytest.mark.parametrize("shape,content", [((5, 9, 130), "random-0..5"), ((3, 7, 1030), "random-0..5"), ((3, 7, 1030), "no-labels")],
                         ids=["small", "long-rows", "no-labels"])
@pytest.mark.parametrize("kind", ["random", "equal"])
def test_pearson_of_uint16_data_against_exact_arithmetic_and_scipy(shape, content, kind):
    """Within ``8 2^-53 |r|`` of the exact rational value (three roundings of exact integers, one product, one square root, one
    division: 4.5 units), and of scipy's ``pearsonr`` within that plus scipy's own measured distance from the rational value."""
    from scipy import stats

    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    a, b = C.pair_u16(shape, content, kind)
    table = K.pair_table(_tensor(labels), n, _tensor(a), _tensor(b))
    got = K.coefficients(table)
    assert list(got) == list(K.COEFFICIENTS) and all(v.dtype == np.float64 and v.shape == (n,) for v in got.values())
    for k in range(n):
        inside = np.ones(shape, bool) if labels is None else labels == k + 1
        va, vb = a[inside].astype(np.int64), b[inside].astype(np.int64)
        exact = R.pearson_exact(len(va), *(int(v) for v in (va.sum(), vb.sum(), (va * va).sum(), (vb * vb).sum(), (va * vb).sum())))
        ours = fractions.Fraction(float(got["pearson"][k]))
        allowed = fractions.Fraction(8 * U) * abs(exact)
        print(f"object {k + 1}: r = {float(exact):.17g}, ours off by {float(abs(ours - exact) / (fractions.Fraction(U) * abs(exact))):.3g} "
              f"units of 2^-53 |r|")
        assert abs(ours - exact) <= allowed
        theirs = fractions.Fraction(float(stats.pearsonr(va.astype(np.float64), vb.astype(np.float64))[0]))
        assert abs(ours - theirs) <= allowed + abs(theirs - exact)
        if kind == "equal":
            assert got["pearson"][k] == 1.0 and got["overlap"][k] == 1.0 and got["k1"][k] == 1.0


@pytest.mark.parametrize("kind", C.WELL_CONDITIONED)
def test_pearson_of_float32_data_is_within_the_propagated_bound(kind):
    """Against r of the restatement's exact sums, in rational arithmetic: within the first-order propagation of the sums' bounds
    through the formula, doubled (``coloc_ref.pearson_bound_f32``)."""
    for shape, content in (((5, 9, 130), "random-0..5"), ((3, 7, 1030), "runs"), ((3, 7, 1030), "no-labels")):
        labels, n = C.labels_of(shape, content, LDS_SLOTS)
        a, b = C.pair_f32(shape, content, LDS_SLOTS, kind)
        want = C.want_f32(shape, content, LDS_SLOTS, kind, "zero")
        got = K.coefficients(K.pair_table(_tensor(labels), n, _tensor(a), _tensor(b)))
        for k in range(n):
            count = int(want["counts"][k, 0])
            assert count > 100
            exact = R.pearson_exact(count, *(float(v) for v in want["sums"][k, :5]))
            allowed = R.pearson_bound_f32(count, want["sums"][k, :5], want["bound"][k, :5])
            error = abs(fractions.Fraction(float(got["pearson"][k])) - exact)
            print(f"{kind}, {content}, object {k + 1}: r = {float(exact):.6f}, error / bound = {float(error) / allowed:.3g}")
            assert error <= allowed
            assert abs(float(exact)) < 0.2 if kind == "independent" else float(exact) > 0.8


def test_coefficients_are_nan_where_they_have_no_meaning():
    table = np.zeros((4,), K.COLOC_DTYPE_U16)
    table[1] = (1, 5, 7, 25, 49, 35, 1, 5, 7, 25, 49, 35, 1, 1, 5, 7)               # one voxel
    table[2] = (3, 15, 6, 75, 14, 30, 0, 0, 0, 0, 0, 0, 0, 3, 15, 0)                # a constant, nothing above ta
    table[3] = (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)                     # two voxels of zeros
    got = K.coefficients(table)
    for name in K.COEFFICIENTS:
        assert np.isnan(got[name][0]) and np.isnan(got[name][1]), name               # count < 2
    assert np.isnan(got["pearson"][2]) and np.isnan(got["pearson_above"][2]) and np.isnan(got["a_in_b"][2])
    assert got["manders_m1"][2] == 1.0 and got["manders_m2"][2] == 0.0 and got["fraction_both"][2] == 0.0
    assert got["b_in_a"][2] == 0.0 and got["k1"][2] == 30 / 75
    assert all(np.isnan(got[name][3]) for name in K.COEFFICIENTS if name != "fraction_both") and got["fraction_both"][3] == 0.0
    same = K.coefficients(table.astype(K.COLOC_DTYPE_F32))
    for name in K.COEFFICIENTS:
        assert np.array_equal(np.isnan(same[name]), np.isnan(got[name])), name
        assert np.allclose(same[name], got[name], rtol=1e-15, atol=0, equal_nan=True), name


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_two_shifted_boxes_have_the_known_answers(dtype):
    """a = 3 in a box, b = 5 in the box shifted by half its width: half of a's mass lies where b is and the other way round; as
    two indicators with p = 192/1200 and p11 = 96/1200, r = (p11 - p^2) / (p (1 - p)) = 17/42."""
    a, b, box, overlap = C.shifted_boxes(dtype)
    table = K.pair_table(None, 1, _tensor(a), _tensor(b))
    got = K.coefficients(table)
    assert table["count"][0] == a.size == 1200 and table["count_both"][0] == overlap and table["count_A"][0] == box
    assert got["manders_m1"][0] == 0.5 and got["manders_m2"][0] == 0.5
    assert got["fraction_both"][0] == overlap / a.size and got["a_in_b"][0] == 0.5 and got["b_in_a"][0] == 0.5
    assert got["pearson"][0] == pytest.approx(17 / 42, rel=8 * U if dtype == np.uint16 else 1e-13, abs=0)
    assert np.isnan(got["pearson_above"][0])                                       # constant where both are above
    assert got["overlap"][0] == pytest.approx(0.5, rel=4 * U) and got["k1"][0] == pytest.approx(5 / 6, rel=2 * U)
    # split at the end of a's box: object 1 holds a's box and the overlap, object 2 the rest of b's box
    labels = np.full(a.shape, 1, np.int32)
    labels[:, :, 12:] = 2
    both = K.coefficients(K.pair_table(_tensor(labels), 2, _tensor(a), _tensor(b)))
    assert both["manders_m1"][0] == 0.5 and both["manders_m2"][0] == 1.0                # all of b's half lies in a's box
    assert np.isnan(both["manders_m1"][1]) and both["manders_m2"][1] == 0.0             # no a at all; none of b where a is


# ---------------------------------------------------------------- Costes' thresholds


def _above(a, b, thresholds):
    return (a.astype(np.float32) > np.float32(thresholds["ta"])) & (b.astype(np.float32) > np.float32(thresholds["tb"]))


@pytest.mark.parametrize("dtype_name", ["uint16", "float32"])
def test_costes_thresholds_separate_the_structure_from_the_background(dtype_name):
    """On the scene of ``coloc_cases.costes_scene``: every structure voxel is above both thresholds and at most 1 % of the
    background is -- first the restatement alone, then the package; for uint16 data the two agree exactly."""
    a, b, structure = C.costes_scene(dtype_name)
    want = C.costes_want(dtype_name, "volume")
    assert want["status"] == "ok" and _above(a, b, want)[structure].all() and _above(a, b, want)[~structure].mean() <= 0.01
    got = K.costes_thresholds(None, 1, _tensor(a), _tensor(b))
    print(f"{dtype_name}: ta = {got['ta']!r}, tb = {got['tb']!r} (restatement {want['ta']!r}, {want['tb']!r}), "
          f"{got['launches']} launches; above: structure {_above(a, b, got)[structure].mean():.4f}, "
          f"background {_above(a, b, got)[~structure].mean():.4f}")
    assert got["status"] == "ok" and got["launches"] <= 34 and got["slope"] > 0
    assert _above(a, b, got)[structure].all() and _above(a, b, got)[~structure].mean() <= 0.01
    if dtype_name == "uint16":
        assert (got["ta"], got["tb"]) == (want["ta"], want["tb"])
        # the labelled region: the structure and a margin of background around it
        labels = np.zeros(a.shape, np.int32)
        labels[0:6, 2:18, 4:36] = 1
        labels[:, :, 20:] *= 2
        region = K.costes_thresholds(_tensor(labels), 2, _tensor(a), _tensor(b), region="labelled")
        restated = R.costes(labels, a, b, 2, "labelled")
        assert (region["ta"], region["tb"], region["status"]) == (restated["ta"], restated["tb"], "ok")


@pytest.mark.parametrize("dtype_name", ["uint16", "float32"])
def test_costes_on_independent_channels_is_uncorrelated(dtype_name):
    """Two independent draws have a sample covariance of either sign, and the rule calls the pair ``uncorrelated`` where it is not
    positive: the second channel is mirrored about 2000 where the draw happened to give a positive one (it stays independent of
    the first).  A constant channel (a variance of 0) and an anticorrelated pair are ``uncorrelated`` too."""
    rng = np.random.default_rng(3)
    a, b = (rng.normal(1000.0, 50.0, (4, 10, 33)).astype(dtype_name) for _ in range(2))
    fa, fb = a.astype(np.float64), b.astype(np.float64)
    if ((fa - fa.mean()) * (fb - fb.mean())).sum() > 0:
        b = (2000 - fb).astype(dtype_name)
    fb = b.astype(np.float64)
    assert abs(np.corrcoef(fa.ravel(), fb.ravel())[0, 1]) < 0.1
    for c, d in ((a, b), (a, np.full_like(a, 7)), (a, (3000 - fa).astype(dtype_name))):
        got = K.costes_thresholds(None, 1, _tensor(c), _tensor(d))
        assert got["status"] == "uncorrelated" and math.isnan(got["ta"]) and math.isnan(got["tb"]) and got["launches"] == 1
        assert R.costes(None, c, d, 1)["status"] == "uncorrelated"
