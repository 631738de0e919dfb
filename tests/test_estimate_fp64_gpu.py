"""The SSD normal-equations kernel (``affine_normal_kernel``, ``csrc/estimate_affine.hip``) against its float64 restatement
(``tests/estimate_ref.py``, pinned on the host by ``test_estimate_host.py``) at every dispatch edge: one sample, less than a
wave, a ragged workgroup, every thread once, a second trip of one workgroup, ragged and many trips of the grid-stride loop,
per-axis strides that do not divide the axis or exceed it, the keep rule to the ulp, nothing kept, a NaN outside the taps.

Exact and edge cases: every per-sample quantity and every partial sum is a float64 (proved in integers on the host), so the
kernel must return the restatement's bits whatever its summation order.  Bound cases (generic float32 scenes, tilted
matrices): within ``(n + 52) 2^-53 sum J^_i J^_j`` (derived in ``estimate_ref``'s docstring).  Measured on an MI355X: all
26 exact and edge cases equal; worst fraction of the bound 1.3e-4 for ``H``, 4.4e-6 for ``b``, 3.5e-6 for ``sse``."""

import ctypes

import numpy as np
import pytest

from tests import estimate_ref as ref

pytestmark = pytest.mark.gpu


def _launch(device, mov, tgt, case_args):
    import torch

    from shrimpy_amd.estimate import normal_equations

    return normal_equations(torch.as_tensor(np.array(mov), device=device),
                            torch.as_tensor(np.array(tgt), device=device), *case_args)


def _partial_rows(device, mov, tgt, matrix, gain, offset, strides, centre, scale, poison=False):
    """The raw ``(256, 121)`` workgroup rows: the same ``_lib.call`` as ``normal_equations``, without the host's sum.
    ``poison``: the output holds NaN before the launch instead of whatever ``torch.empty`` left there."""
    import torch

    from shrimpy_amd import _lib
    from shrimpy_amd.estimate import _f64p, _stride3
    from shrimpy_amd.geometry import as_matrix_3x4

    dm = torch.as_tensor(np.array(mov), device=device)
    dt = torch.as_tensor(np.array(tgt), device=device)
    c = np.ascontiguousarray(centre, dtype=np.float64)
    rows, width = _lib.call_value("lsr_affine_normal_blocks"), _lib.call_value("lsr_affine_normal_size")
    assert (rows, width) == (256, 121)
    partial = torch.empty((rows, width), dtype=torch.float64, device=device)
    if poison:
        partial.fill_(float("nan"))
    with torch.cuda.device(device):
        _lib.call("lsr_affine_normal_equations_f32", dm.data_ptr(), *(int(v) for v in dm.shape), dt.data_ptr(),
                  *(int(v) for v in dt.shape), _lib.matrix12(as_matrix_3x4(matrix)), ctypes.c_double(float(gain)),
                  ctypes.c_double(float(offset)), (ctypes.c_int * 3)(*_stride3(strides)), _f64p(c),
                  ctypes.c_double(float(scale)), partial.data_ptr(), _lib.stream_ptr(device))
    return partial.cpu().numpy()


def _args(case):
    return (case.m, case.gain, case.offset, case.strides, case.centre, case.scale)


def _assert_bits(got, want, name):
    assert got[3] == want[3], (name, got[3], want[3])
    assert np.array_equal(got[0], want[0]), (name, "H", np.argwhere(got[0] != want[0])[:4].tolist())
    assert np.array_equal(got[1], want[1]), (name, "b", np.flatnonzero(got[1] != want[1]).tolist())
    assert got[2] == want[2], (name, "sse", got[2], want[2])


@pytest.mark.parametrize("case", ref.EXACT_CASES + ref.EDGE_CASES, ids=lambda c: c.name)
def test_kernel_equals_the_restatement_bit_for_bit(device, case):
    launch, tgt, _ = ref.volumes(case)
    want = ref.expectation(case)
    got = _launch(device, launch, tgt, _args(case))
    _assert_bits(got, want, case.name)
    if case.n is not None:
        assert got[3] == case.n
    if case.n == 0:
        assert not got[0].any() and not got[1].any() and got[2] == 0.0       # 0.0, not NaN
    if case.sse is not None:
        assert got[2] == case.sse


@pytest.mark.parametrize("case", ref.BOUND_CASES, ids=lambda c: c.name)
def test_kernel_is_within_the_a_priori_bound(device, case):
    """Worst measured fraction of the bound on an MI355X over the cases: H 1.3e-4 (legacy-stride-3-3-3), b 4.4e-6, sse 3.5e-6."""
    mov, tgt, m = ref.bound_inputs(case)
    h, b, sse, n, rows = ref.bound_expectation(case)
    args = (m, case.gain, case.offset, case.strides, np.array(case.centre), case.scale)
    got = _launch(device, mov, tgt, args)
    bounds = ref.apriori_bound(rows)
    fr = [ref.worst_fraction(g, w, bd) for g, w, bd in zip(got[:3], (h, b, sse), bounds)]
    print(f"{case.name}: n {got[3]} (want {n}), worst fraction of the a-priori bound: H {fr[0]:.3e} b {fr[1]:.3e} sse {fr[2]:.3e}")
    assert got[3] == n
    assert max(fr) <= 1.0
    assert np.array_equal(got[0], got[0].T)
    again = _launch(device, mov, tgt, args)
    _assert_bits(again, got, case.name)                                      # fixed summation order


def test_partial_rows_of_a_small_launch(device):
    """Fewer than 256 grid samples: workgroup 0 owns them all, the other 255 rows are written and are exactly zero."""
    for case in ref.EXACT_CASES[:3]:
        assert case.grid_samples < 256
        launch, tgt, _ = ref.volumes(case)
        h, b, sse, n, _ = ref.expectation(case)
        part = _partial_rows(device, launch, tgt, *_args(case))
        assert part.shape == (256, 121) and not part[1:].any()
        assert np.array_equal(part[0], np.concatenate([h[np.triu_indices(14)], b, [sse, float(n)]])), case.name


def test_partial_rows_of_the_second_trip(device):
    """65 792 grid samples: the samples 65 536 .. 65 791 are workgroup 0's second trip.  Every row's ``n`` column is
    the number of kept samples that workgroup owns, and the rows add up to the restatement's sums."""
    case = next(c for c in ref.EXACT_CASES if c.name == "second-trip-of-workgroup-0")
    launch, tgt, _ = ref.volumes(case)
    h, b, sse, n, rows = ref.expectation(case)
    part = _partial_rows(device, launch, tgt, *_args(case))
    owner = (rows.index // 256) % 256
    assert np.array_equal(part[:, 120], np.bincount(owner, minlength=256).astype(np.float64))
    assert part[:, 120].sum() == n and (rows.index >= ref.N_THREADS).sum() == 256
    assert np.array_equal(part.sum(axis=0), np.concatenate([h[np.triu_indices(14)], b, [sse, float(n)]]))


def test_every_row_is_written_by_the_launch(device):
    """The output of ``normal_equations`` is ``torch.empty``.  First the entry itself on a buffer that holds NaN in every
    row; then ``normal_equations`` right after a NaN-filled block of the output's size was freed, which the caching
    allocator hands to the next request of that size (reported, since an allocator may be configured otherwise)."""
    import torch

    from shrimpy_amd.estimate import normal_equations

    for case in (ref.EXACT_CASES[0], ref.EXACT_CASES[2], next(c for c in ref.EDGE_CASES if c.name == "nothing-kept")):
        launch, tgt, _ = ref.volumes(case)
        h, b, sse, n, _ = ref.expectation(case)
        part = _partial_rows(device, launch, tgt, *_args(case), poison=True)
        assert not np.isnan(part).any() and not part[1:].any()
        assert np.array_equal(part[0], np.concatenate([h[np.triu_indices(14)], b, [sse, float(n)]])), case.name
        dm, dt = torch.as_tensor(np.array(launch), device=device), torch.as_tensor(np.array(tgt), device=device)
        poison = torch.full((256, 121), float("nan"), dtype=torch.float64, device=device)
        where = poison.data_ptr()
        torch.cuda.synchronize(device)
        del poison
        probe = torch.empty((256, 121), dtype=torch.float64, device=device)
        reused = probe.data_ptr() == where and bool(torch.isnan(probe).all())
        del probe
        got = normal_equations(dm, dt, *_args(case))
        print(f"{case.name}: the NaN-filled block was handed back to the next allocation: {reused}")
        _assert_bits(got, ref.expectation(case), case.name)
