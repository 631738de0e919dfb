"""The float64 restatement of the SSD normal-equations kernel (``tests/estimate_ref.py``) pinned without a GPU: the
exactness proof of every exact and edge case in integers, the closed-form sample counts, agreement with the numpy oracle
within the a-priori bound, and the host helpers of ``shrimpy_amd.estimate`` around the kernel.  The kernel itself is held
to the restatement in ``test_estimate_fp64_gpu.py``."""

from fractions import Fraction

import numpy as np
import pytest

from oracle import cpu_ref as o
from tests import estimate_ref as ref

ALL_EXACT = ref.EXACT_CASES + ref.EDGE_CASES


def _packed(h, b, sse, n):
    return np.concatenate([h[np.triu_indices(14)], b, [sse, float(n)]])


def test_case_table_covers_the_launch_sizes():
    """Grid samples (``nz ny nx``) of the exact cases: one sample, less than a wave, ragged inside a workgroup, every
    thread once, one workgroup on a second trip, a ragged second trip, seven trips; the per-axis strides of the largest."""
    grid = {c.name: c.grid_samples for c in ref.EXACT_CASES}
    assert grid["one-sample"] == 1 and grid["less-than-a-wave"] == 30 and 64 < grid["ragged-workgroup-gain-0"] < 256
    assert grid["every-thread-once"] == ref.N_THREADS and grid["second-trip-of-workgroup-0"] == ref.N_THREADS + 256
    assert grid["ragged-second-trip"] == 104448 and grid["seven-trips"] == 419331 and -(-419331 // ref.N_THREADS) == 7
    big = {c.strides for c in ref.EXACT_CASES if c.target_shape == (33, 97, 131)}
    assert big == {(1, 1, 1), (4, 2, 1), (1, 3, 7), (64, 1, 1)}
    assert {c.gain for c in ref.EXACT_CASES} == {0.5, -1.5, 0.0, 1.0}
    assert grid["strides-1-3-7"] == 33 * 33 * 19 and grid["strides-64-1-1"] == 1 * 97 * 131      # ceil_div, stride > axis


@pytest.mark.parametrize("case", ALL_EXACT, ids=lambda c: c.name)
def test_exact_cases_are_exact_in_integers(case):
    """``J 2^12`` and ``r 2^12`` are integers, the widest sum of magnitudes stays below 2^53 in units of 2^-24 (so every
    partial sum in any order is a float64), and the restatement's sums equal the int64 ones bit for bit -- also after a
    random permutation of the samples."""
    h, b, sse, n, rows = ref.expectation(case)
    want, bits = ref.exact_integer_sums(rows)
    assert bits <= 53
    assert np.array_equal(_packed(h, b, sse, n), want)
    assert np.array_equal(h, h.T)
    if 0 < n <= 120000:       # (the largest cases: the integer sums above already are order-free)
        perm = np.random.default_rng(3).permutation(n)
        assert np.array_equal(ref.packed_sums(rows.J[perm], rows.r[perm]), want)
        assert np.array_equal(_packed(rows.J.T @ rows.J, rows.J.T @ rows.r, float(rows.r @ rows.r), n), want)   # plain float64
    # the inputs are what the docstring of the module says they are
    launch, tgt, mov = ref.volumes(case)
    assert np.array_equal(mov, np.rint(mov)) and mov.min() >= 0 and mov.max() <= 15 and tgt.max() <= 15
    eps = 2.0 ** -40
    m4 = case.m * 4
    assert all(v == np.rint(v) or abs(v) == 4 * eps for v in m4.ravel())
    assert case.gain in (0.5, -1.5, 0.0, 1.0) and case.offset == int(case.offset)
    assert np.log2(case.scale) == int(np.log2(case.scale)) and case.scale <= 64 and np.array_equal(2 * case.centre, np.rint(2 * case.centre))
    if case.n is not None:
        assert n == case.n
    if case.sse is not None:
        assert sse == case.sse
    if case.late_kept:
        late = rows.index >= ref.N_THREADS
        assert late.sum() >= 200, "samples of the later trips must be kept"
        assert rows.index.max() >= (case.grid_samples - 1) // ref.N_THREADS * ref.N_THREADS      # ... of the LAST trip too


def test_edge_case_counts_are_the_closed_forms():
    by_name = {c.name: c for c in ref.EDGE_CASES}
    assert ref.expectation(by_name["identity-2-2-2"])[3] == 1
    assert ref.expectation(by_name["identity-5-6-7"])[3] == 4 * 5 * 6
    h, b, sse, n, rows = ref.expectation(by_name["nothing-kept"])
    assert n == 0 and sse == 0.0 and not h.any() and not b.any() and not np.isnan(h).any()
    for case in ref.EDGE_CASES:
        if "dropped" not in case.extra:
            continue
        h, b, sse, n, rows = ref.expectation(case)
        axis, shape = case.extra["axis"], case.target_shape
        keep = rows.keep.reshape(shape)
        want = np.ones(shape, bool)
        for k in range(3):       # the identity rule on the other axes: the last plane is out
            sl = [slice(None)] * 3
            sl[k] = [shape[k] - 1] if k != axis else case.extra["dropped"]
            want[tuple(sl)] = False
        assert np.array_equal(keep, want), case.name
        assert n == case.n == int(want.sum())
    # the four coordinates of the issue, on every axis: 0 - 2^-40 out, 0 in, (n - 1) - 2^-40 in, n - 1 out
    for axis in range(3):
        below = ref.expectation(by_name[f"ulp-below-axis-{axis}"])[4]
        ident = ref.expectation(by_name["identity-5-6-7"])[4]
        c, ci = below.coord[axis], ident.coord[axis]
        n_a = by_name["identity-5-6-7"].moving_shape[axis]
        assert c.min() == -2.0 ** -40 and not below.keep[c < 0].any()
        assert c.max() == (n_a - 1) - 2.0 ** -40 and c.max() < n_a - 1 and below.keep[c == c.max()].any()
        assert ci.min() == 0.0 and ident.keep[ci == 0].any() and ci.max() == n_a - 1 and not ident.keep[ci == n_a - 1].any()


def test_nan_outside_the_kept_taps_changes_nothing():
    case = next(c for c in ref.EDGE_CASES if c.nan_at is not None)
    launch, tgt, mov = ref.volumes(case)
    h, b, sse, n, rows = ref.expectation(case)
    assert np.isnan(launch[case.nan_at]) and not rows.touched[case.nan_at] and rows.touched.sum() == 4 ** 3
    again = ref.normal_equations_f64(launch, tgt, case.m, case.gain, case.offset, case.strides, case.centre, case.scale)
    assert np.array_equal(_packed(*again), _packed(h, b, sse, n))
    inside = launch.copy()
    inside[1, 1, 1] = np.nan             # ... and one that a kept sample does touch is seen
    assert np.isnan(ref.normal_equations_f64(inside, tgt, case.m, case.gain, case.offset, case.strides, case.centre,
                                             case.scale)[2])


@pytest.mark.parametrize("case", ref.BOUND_CASES, ids=lambda c: c.name)
def test_restatement_agrees_with_the_oracle_within_the_a_priori_bound(case):
    """The oracle takes its coordinates from a matrix product: the bound carries the coordinate term (12 roundings)."""
    mov, tgt, m = ref.bound_inputs(case)
    h, b, sse, n, rows = ref.bound_expectation(case)
    want = o.affine_normal_equations(mov, tgt, m[:3], case.gain, case.offset, case.strides, np.array(case.centre), case.scale)
    assert n == want[3] and n > 500
    if case.name == "multi-trip-stride-1-1-1":
        assert (rows.index >= ref.N_THREADS).sum() > 30000
    bh, bb, bs = ref.apriori_bound(rows, coordinate_roundings=12)
    plain = ref.apriori_bound(rows)
    fr = [ref.worst_fraction(g, w, bd) for g, w, bd in zip((h, b, sse), want[:3], (bh, bb, bs))]
    print(f"{case.name}: n {n}, worst fraction of the bound H {fr[0]:.3g} b {fr[1]:.3g} sse {fr[2]:.3g}; "
          f"the coordinate term is {float(np.max(bh / plain[0])) - 1:.3g} of the plain bound at most")
    assert max(fr) <= 1.0
    assert np.array_equal(h, h.T) and np.all(np.linalg.eigvalsh(h) > 0)


def test_unpack_and_stride3():
    from shrimpy_amd import estimate as e

    case = ref.EXACT_CASES[2]
    h, b, sse, n, rows = ref.expectation(case)
    row = ref.packed_sums(rows.J, rows.r)
    got = e._unpack(row)
    assert np.array_equal(got[0], h) and np.array_equal(got[1], b) and got[2] == sse and got[3] == n
    assert np.array_equal(got[0], got[0].T)
    assert e._stride3(3) == (3, 3, 3) and e._stride3((2, 8, 8)) == (2, 8, 8) and e._stride3(np.int64(2)) == (2, 2, 2)
    with pytest.raises(ValueError, match="stride"):
        e._stride3((2, 2))
    # a zero stride keeps its shape in ``_stride3``; the entry refuses it on the host, before anything is launched
    import ctypes

    from shrimpy_amd import _lib

    assert e._stride3((2, 0, 2)) == (2, 0, 2)
    mov, tgt = np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32)
    centre, partial = np.zeros(3), np.zeros((256, 121))
    for bad in ((2, 0, 2), (0, 0, 0), (1, 1, -1)):
        with pytest.raises(_lib.LsrError, match="strides must be >= 1"):
            _lib.call("lsr_affine_normal_equations_f32", mov.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 4, 4, 4,
                      tgt.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 4, 4, 4, _lib.matrix12(np.eye(4)[:3]),
                      ctypes.c_double(1.0), ctypes.c_double(0.0), (ctypes.c_int * 3)(*e._stride3(bad)), e._f64p(centre),
                      ctypes.c_double(2.0), partial.ctypes.data, None)


def test_keep_rule_follows_the_written_order_not_a_fused_product():
    """A z row for which ``((m0 z + m1 y) + m2 x) + m3`` is exactly 9 = n - 1 at target index (4, 7, 3) (dropped), while a
    fused accumulation of the same row -- how a BLAS matrix product evaluates it, emulated here in exact rationals with
    one rounding per fused step -- gives 9 - 2^-49 (kept).  The restatement, like the kernel, follows the written order."""
    row = [float.fromhex(v) for v in ("0x1.1b44159b2223ap-1", "0x1.55adb22f2cab3p-2", "0x1.dc3ae5b68a67dp-2",
                                      "0x1.872dd85722df8p+1")]
    z, y, x = 4, 7, 3
    t = float(Fraction(row[0]) * z)
    t = float(Fraction(row[1]) * y + Fraction(t))
    t = float(Fraction(row[2]) * x + Fraction(t))
    fused = t + row[3]
    written = ((row[0] * z + row[1] * y) + row[2] * x) + row[3]
    assert written == 9.0 and fused == 9.0 - 2.0 ** -49
    m = np.array([row, [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
    rng = np.random.default_rng(0)
    mov, tgt = rng.integers(0, 16, (10, 10, 10)).astype(np.float32), rng.integers(0, 16, (8, 8, 8)).astype(np.float32)
    h, b, sse, n, rows = ref.normal_equations_f64(mov, tgt, m, 1.0, 0.0, 1, [3.5, 3.5, 3.5], 4.0, rows=True)
    s = (z * 8 + y) * 8 + x
    assert rows.coord[0][s] == 9.0 and not rows.keep[s]
    # nothing else about this sample keeps it out, and no other sample sits on the limit
    assert 0 <= rows.coord[1][s] < 9 and 0 <= rows.coord[2][s] < 9 and (rows.coord[0] == 9.0).sum() == 1
    with_fused = rows.keep.copy()
    with_fused[s] = True
    assert n == rows.keep.sum() == with_fused.sum() - 1
