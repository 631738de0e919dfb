"""The band-power kernels (``csrc/focus.hip``) against float64 transforms at EVERY window length they accept.

``focus.hip`` restates the row-transform wrappers of ``csrc/rfft_rows.hip`` for its x leg and adds a complex column
transform with a full twiddle table, the only complex LDS transform beyond N = 256.  ``tests/test_fft_kernels_fp64_gpu.py``
pins the originals at every length; here every row length Xc (with a small Yc) and every column length Yc = 2 .. 2048
(with a small Xc) runs through ``lsr_band_power_f32`` raw, the window inside a larger, NaN-surrounded plane at offsets
that rotate (an odd x0: the 4-byte-aligned pair gather), on three planes: standard normal, a 2-D tone at one bin under
test, an impulse at the window's last voxel (``tests/transform_cases.py``).

The tables are built here, not by ``lsr_band_power_plan``: "full" (every column 0 .. M with [0, N / 2]; the scratch then
holds the whole x leg, held row by row to float64 ``rfft`` with the FFT sweep's check and constants) and one-bin tables
(one column with a = b = m, every other column empty) at (0, 0), (N / 2, M), (N / 2, 0), (0, M), (1, 1) and a
pseudo-random bin: both self-paired columns, both self-mirrored rows and their crossings.  For every table and plane

    |P_got - P_ref| <= 32 u (log2 Xc + log2 Yc) W sqrt(Yc Xc) rms(plane),        u = 2^-24,

``W`` the weighted bin count of THAT table and ``P_ref`` from float64 ``fft2`` over the full-spectrum mask of the table
(and, independently, by the half-spectrum weight rule).  With one bin ``W <= 4``: the bound is about 1e-5 of a typical
coefficient, so one wrong bin, weight or mirror shows.  The tone's power is also held to its closed form ``A Yc Xc`` on its
own bin and to nothing on the others.  Two calls return the same bits, and the host twin agrees within twice the bound.

Corners: the default 800 x 800 window with the band of ``lsr_band_power_plan``, and the longest pair (2048, 4096), where
both legs launch at their LDS maximum (139 KB and 147 KB: the dynamic-LDS opt-ins).

Worst ratios observed on an MI355X (``WORST``): x leg l2 0.882, max 8.30 (of 2.5 and 32); power / bound: full 4.3e-3, one
bin 0.540, the default window 9.6e-4; device against twin (of 2): full 4.3e-3, one bin 0.540.  The 0.540 is the tone on
its own self-paired bin at (1500, 12): P = 18000 comes back one float32 ulp high (pocketfft in single returns the same
bits) -- a tone puts all of ``A Yc Xc`` into one coefficient while the bound grows with ``sqrt(Yc Xc)``.
"""
import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import focus as F
from tests import focus_ref as R
from tests import transform_cases as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PARTS = T.slices(T.FOCUS_ROW_CASES) + T.slices(T.FOCUS_COL_CASES)

# the worst ratio seen per family in this process (the FFT sweep's dict: read back when the constants are re-measured)
WORST = T.WORST


def _raw_call(vol_d, window, table, dev=DEV):
    """``lsr_band_power_f32`` with NaN-filled output and scratch buffers (``test_focus_gpu._raw_call`` with the table as an
    argument): (power, spec, partial)."""
    z, y, x = vol_d.shape
    yc, xc, y0, x0 = window
    k_hi = table.shape[0] - 1
    sb, pb = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.call("lsr_band_power_scratch_bytes", z, yc, k_hi, ctypes.byref(sb), ctypes.byref(pb))
    spec = torch.full((sb.value // 4,), float("nan"), dtype=torch.float32, device=dev)
    partial = torch.full((pb.value // 8,), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full((z,), float("nan"), dtype=torch.float64, device=dev)
    half, full = F._row_twiddles(xc, dev)
    tw_y = F._column_twiddles(yc, dev)
    tab = torch.as_tensor(np.ascontiguousarray(table, dtype=np.int32), device=dev)
    _lib.call("lsr_band_power_f32", vol_d.data_ptr(), z, y, x, y0, x0, yc, xc, half.data_ptr(), full.data_ptr(),
              tw_y.data_ptr(), tab.data_ptr(), k_hi, spec.data_ptr(), partial.data_ptr(), out.data_ptr(), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy(), spec, partial


def _sweep_case(case, twin=True):
    yc, xc = case.yc, case.xc
    window = (yc, xc, case.y0, case.x0)
    vol_d = torch.as_tensor(np.ascontiguousarray(case.vol), device=DEV)
    planes = case.vol.shape[0]
    case.check_reference()
    for kind, b, table, weighted, ref, bound in case.tables:
        got, spec, partial = _raw_call(vol_d, window, table)
        assert not torch.isnan(partial).any(), f"{kind} {b}: a partial was not written"
        if kind == "full":
            assert not torch.isnan(spec).any(), "the x leg left a coefficient unwritten"
            rows = spec.cpu().numpy().view(np.complex64).reshape(planes, xc // 2 + 1, yc).transpose(0, 2, 1)
            T.check_x_leg("focus x leg", rows, case.rows, xc)
        case.check_power("focus power", got, kind, b, weighted, ref, bound)
        again, _, _ = _raw_call(vol_d, window, table)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), f"{kind} {b}: a second call returns other bits"
        if not twin:
            continue
        host = T.host_twin_power(case, table)
        ratio = np.abs(got - host) / bound
        T._record(f"focus power against the twin {kind}", ratio.max())
        assert np.all(ratio <= 2.0), f"{kind} {b}: device {got}, host twin {host}, bound {bound}"


def test_the_sweep_covers_every_length_the_kernels_accept():
    assert len(T.ROW_X) == 86 and len(T.COL_Y) == 109
    assert [x for x in range(0, 4101) if _lib.call_value("lsr_rfft_rows_supported", x)] == T.ROW_X
    assert [y for y in range(0, 2100) if _lib.call_value("lsr_band_power_supported", y, 8)] == T.COL_Y
    assert sorted({c[1] for c in T.FOCUS_ROW_CASES}) == T.ROW_X and sorted({c[0] for c in T.FOCUS_COL_CASES}) == T.COL_Y


@pytest.mark.parametrize("part", PARTS, ids=T.slice_id)
def test_band_power_every_length(part):
    for yc, xc, index in part:
        with T.at(f"(Yc, Xc) = ({yc}, {xc})"):
            _sweep_case(T.FocusCase(yc, xc, index))


def test_the_default_window():
    """Planes (2, 800, 800) -- the default ``center_crop_xy``, never transformed elsewhere in the suite -- with the band of
    ``lsr_band_power_plan`` at ``focus_ref.OPTICS`` and the default fractions, against ``focus_ref.power`` and
    ``focus_ref.bound``."""
    vol = np.random.default_rng(800).standard_normal((2, 800, 800)).astype(np.float32)
    assert F.focus_grid(vol.shape) == (800, 800, 0, 0)
    lo, hi = F.band_limits(R.OPTICS["NA_det"], R.OPTICS["lambda_ill"], R.FRACTIONS)
    table, k_hi, weighted = F.band_table(800, 800, R.OPTICS["pixel_size"], lo, hi)
    assert 0 < k_hi < 400 and weighted == int(R.band_mask(800, 800, **R.OPTICS).sum())
    ref, bound = R.power(vol, **R.OPTICS), R.bound(vol, **R.OPTICS)
    vol_d = torch.as_tensor(vol, device=DEV)
    got, spec, partial = _raw_call(vol_d, (800, 800, 0, 0), table[:k_hi + 1])
    assert not torch.isnan(partial).any() and not torch.isnan(spec).any()
    ratio = np.abs(got - ref) / bound
    T._record("focus power default window", ratio.max())
    assert np.all(np.isfinite(got)) and np.all(ratio <= 1.0), f"|P - P_ref| / bound = {ratio}"
    again, _, _ = _raw_call(vol_d, (800, 800, 0, 0), table[:k_hi + 1])
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    public = F.midband_power(vol_d, **R.OPTICS)
    assert np.array_equal(public.cpu().numpy().view(np.uint64), got.view(np.uint64))


def test_the_longest_pair():
    """The longest window ``lsr_band_power_supported`` accepts, one plane, "full" and two one-bin tables: both legs at their
    LDS maximum in one launch, the column transform at the length where its butterfly index arithmetic stops being
    exact.  (The host twin, eight million points in plain loops, is left to the sweep's lengths.)"""
    yc, xc = T.longest_pair(lambda y, x: _lib.call_value("lsr_band_power_supported", y, x))
    assert (yc, xc) == (T.COL_Y[-1], T.ROW_X[-1]) == (2048, 4096)
    bins = [(yc // 2, xc // 2), T.one_bins(yc, xc)[-1]]
    _sweep_case(T.FocusCase(yc, xc, 1, planes=1, bins=bins), twin=False)
