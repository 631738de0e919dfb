"""Focus measure of a z stack: the mid-band spectral power of every plane, and the plane where it peaks.

This is what biahub's ``estimate-stabilization`` uses for the z drift of a time-lapse: waveorder's
``focus_from_transverse_band``.  Neither package is vendored or installed: PARITY IS UNPINNED.  The rule below is this
package's own statement -- [RECALLED] where it follows waveorder from memory -- and ``tests/focus_ref.py`` restates it in
float64 NumPy as the test oracle.

**Band power of a plane** ``v`` of shape ``(Yc, Xc)``, pixel size ``p``: ``F = fft2(v)`` unnormalised [RECALLED],
``cutoff = 2 NA_det / lambda_ill``, and ::

    r(ky, kx) = sqrt((min(ky, Yc - ky) / (Yc p))^2 + (min(kx, Xc - kx) / (Xc p))^2)         (float64)
    P = sum of |F(ky, kx)| over the bins with  cutoff f0 < r < cutoff f1                      (both strict)

``midband_fractions = (f0, f1)``, default ``(0.125, 0.25)`` [RECALLED].  On the half spectrum ``kx <= Xc / 2`` the columns
``0 < kx < Xc / 2`` count twice.  The power of a volume is the float64 vector ``P[z]``.

**Transform window** (:func:`focus_grid`).  No padding: every plane is centre-cropped (start ``d // 2``, as
``dynatrack._match_shape`` crops) to ``(Yc, Xc)``; ``Xc`` is the largest length ``<= min(X, center_crop_xy[1])`` the row
kernels take (``lsr_rfft_rows_supported``: a multiple of 4 whose half is 5-smooth, 8 .. 4096), ``Yc`` the largest 5-smooth
length ``<= min(Y, center_crop_xy[0])`` in 2 .. 2048 (one tile of eight columns of the y leg in a CU's LDS, and the range the
LDS transforms' index arithmetic is exact for).  ``center_crop_xy`` defaults to ``(800, 800)``.

**Focus index** (:func:`focus_from_transverse_band`): ``argmax P`` (``mode="min"``: ``argmin``; the first extremum wins a
tie), kept when the peak's full width at half prominence -- ``scipy.signal.peak_widths(P, [peak], rel_height=0.5)``,
restated here in NumPy (:func:`peak_width`) -- is at least ``threshold_FWHM``, else ``None``.  ``Z == 1`` is index 0.

On a HIP device ``P`` is three launches of ``csrc/focus.hip`` (``lsr_band_power_f32``): the x transform of the window's rows
straight from the uncropped volume, keeping only the columns that hold band bins; the y transform of eight columns per
workgroup in LDS with the masked sum of magnitudes as its epilogue; a fixed-order sum per plane.  Neither the cropped volume
nor the y-transformed spectrum is written.  CPU tensors and arrays take the host twin (``lsr_band_power_f32_cpu``).  The
strict inequalities are decided once, in float64 on the host (:func:`band_table`), for kernels and twin alike.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

__all__ = ["focus_grid", "band_limits", "band_table", "midband_power", "peak_width", "focus_from_transverse_band",
           "MAX_YC", "DEFAULT_CENTER_CROP_XY", "DEFAULT_MIDBAND_FRACTIONS"]

MAX_YC = 2048                                # csrc/focus.hpp: kMaxY
DEFAULT_CENTER_CROP_XY = (800, 800)
DEFAULT_MIDBAND_FRACTIONS = (0.125, 0.25)


def _smooth5(n: int) -> bool:
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def focus_grid(shape_zyx, center_crop_xy=DEFAULT_CENTER_CROP_XY) -> tuple[int, int, int, int]:
    """``(Yc, Xc, y0, x0)``: the transform window of a ``(Z, Y, X)`` volume and its first row and column (module docstring)."""
    _, y, x = (int(v) for v in shape_zyx)
    cy, cx = (int(v) for v in center_crop_xy)
    if min(y, x, cy, cx) <= 0:
        raise ValueError(f"shape_zyx {tuple(shape_zyx)} and center_crop_xy {tuple(center_crop_xy)} must be positive")
    xc = min(x, cx) // 4 * 4
    while xc >= 8 and not _lib.call_value("lsr_rfft_rows_supported", xc):
        xc -= 4
    yc = min(y, cy, MAX_YC)
    while yc >= 2 and not _smooth5(yc):
        yc -= 1
    if xc < 8 or yc < 2:
        raise ValueError(f"a ({y}, {x}) plane cropped to {(cy, cx)} is too small for the focus measure: the window needs "
                         "at least 2 rows and 8 columns")
    return yc, xc, (y - yc) // 2, (x - xc) // 2


def band_limits(NA_det: float, lambda_ill: float, midband_fractions=DEFAULT_MIDBAND_FRACTIONS) -> tuple[float, float]:
    """``(cutoff f0, cutoff f1)`` in cycles per unit length, ``cutoff = 2 NA_det / lambda_ill``."""
    f0, f1 = (float(v) for v in midband_fractions)
    if not (0.0 <= f0 < f1 and np.isfinite(f1)):
        raise ValueError(f"midband_fractions {tuple(midband_fractions)} must satisfy 0 <= f0 < f1")
    if not (float(NA_det) > 0 and float(lambda_ill) > 0):
        raise ValueError("NA_det and lambda_ill must be positive")
    cutoff = 2.0 * float(NA_det) / float(lambda_ill)
    return cutoff * f0, cutoff * f1


def band_table(yc: int, xc: int, pixel_size: float, band_lo: float, band_hi: float):
    """``(table, k_hi, weighted_bins)``: for every column ``kx <= xc / 2`` of the half spectrum the closed interval
    ``table[kx] = (a, b)`` of ``min(ky, yc - ky)`` with ``band_lo < r < band_hi`` (``a > b``: none), int32 ``(xc / 2 + 1, 2)``;
    ``k_hi`` the last column that holds a bin (``-1``: the band is empty); ``weighted_bins`` the number of bins of the full
    spectrum inside the band.  Float64 on the host (``lsr_band_power_plan``)."""
    yc, xc = int(yc), int(xc)
    table = np.zeros((xc // 2 + 1, 2), dtype=np.int32)
    k_hi, weighted = ctypes.c_int64(-1), ctypes.c_int64(0)
    _lib.call("lsr_band_power_plan", yc, xc, float(pixel_size), float(band_lo), float(band_hi), table.ctypes.data,
              ctypes.byref(k_hi), ctypes.byref(weighted))
    return table, int(k_hi.value), int(weighted.value)


_twiddles: dict = {}


def _column_twiddles(n: int, device):
    """``exp(-2 pi i k / n)``, ``k < n``, complex64 on ``device`` (cached per length, as ``fft3._row_twiddles``)."""
    import torch

    key = (int(n), device.index)
    t = _twiddles.get(key)
    if t is None:
        if len(_twiddles) >= 16:
            _twiddles.pop(next(iter(_twiddles)))
        k = np.arange(n, dtype=np.float64)
        t = _twiddles[key] = torch.as_tensor(np.exp(-2j * np.pi * k / n).astype(np.complex64), device=device)
    return t


_tables: dict = {}


def _device_table(key, table, k_hi, device):
    import torch

    key = key + (device.index,)
    t = _tables.get(key)
    if t is None:
        if len(_tables) >= 16:
            _tables.pop(next(iter(_tables)))
        t = _tables[key] = torch.as_tensor(np.ascontiguousarray(table[:k_hi + 1]), device=device)
    return t


def midband_power(volume, NA_det: float, lambda_ill: float, pixel_size: float,
                  midband_fractions=DEFAULT_MIDBAND_FRACTIONS, center_crop_xy=DEFAULT_CENTER_CROP_XY):
    """``P[z]`` of a ``(Z, Y, X)`` volume (module docstring): a float64 tensor of ``Z`` on the volume's device for a
    ``torch.Tensor``, a float64 array for a NumPy array.  ``uint16`` input is widened to float32 first.  An empty band --
    no bin of the window satisfies the inequalities -- is a ``ValueError``."""
    import torch

    as_numpy = not isinstance(volume, torch.Tensor)
    vol = torch.from_numpy(np.ascontiguousarray(volume).astype(np.float32, copy=False)) if as_numpy else volume
    if vol.dim() != 3 or min(vol.shape) <= 0:
        raise ValueError(f"volume must be (Z, Y, X), got shape {tuple(vol.shape)}")
    vol = vol.to(torch.float32).contiguous()
    z, y, x = (int(v) for v in vol.shape)
    if not (float(pixel_size) > 0 and np.isfinite(float(pixel_size))):
        raise ValueError(f"pixel_size must be positive, got {pixel_size}")
    yc, xc, y0, x0 = focus_grid((z, y, x), center_crop_xy)
    lo, hi = band_limits(NA_det, lambda_ill, midband_fractions)
    table, k_hi, _ = band_table(yc, xc, pixel_size, lo, hi)
    if k_hi < 0:
        raise ValueError(f"the band {lo * float(pixel_size):.6g} < r < {hi * float(pixel_size):.6g} cycles per pixel holds no "
                         f"bin of the ({yc}, {xc}) window: check NA_det, lambda_ill, pixel_size and midband_fractions")
    out = torch.empty((z,), dtype=torch.float64, device=vol.device)
    if vol.device.type == "cuda":
        dev = vol.device
        with torch.cuda.device(dev):
            half, full = _row_twiddles(xc, dev)
            tw_y = _column_twiddles(yc, dev)
            tab = _device_table((yc, xc, float(pixel_size), lo, hi), table, k_hi, dev)
            spec_bytes, partial_bytes = ctypes.c_int64(0), ctypes.c_int64(0)
            _lib.call("lsr_band_power_scratch_bytes", z, yc, k_hi, ctypes.byref(spec_bytes), ctypes.byref(partial_bytes))
            spec = torch.empty((spec_bytes.value // 8,), dtype=torch.complex64, device=dev)
            partial = torch.empty((partial_bytes.value // 8,), dtype=torch.float64, device=dev)
            _lib.call("lsr_band_power_f32", vol.data_ptr(), z, y, x, y0, x0, yc, xc, half.data_ptr(), full.data_ptr(),
                      tw_y.data_ptr(), tab.data_ptr(), k_hi, spec.data_ptr(), partial.data_ptr(), out.data_ptr(),
                      _lib.stream_ptr(dev))
    else:
        _lib.call("lsr_band_power_f32_cpu", vol.data_ptr(), z, y, x, y0, x0, yc, xc, None, None, None, table.ctypes.data,
                  k_hi, None, None, out.data_ptr(), None)
    return out.numpy() if as_numpy else out


def _row_twiddles(xc: int, device):
    from . import fft3

    return fft3._row_twiddles(xc, device)


def peak_width(power, peak: int, rel_height: float = 0.5) -> float:
    """``scipy.signal.peak_widths(power, [peak], rel_height)[0][0]`` in NumPy: the peak's prominence (its height above the
    higher of the two lowest points between it and the next higher sample -- or the end -- on either side), then the
    distance between the linear interpolations of the crossings of ``power[peak] - prominence * rel_height`` on both sides."""
    x = np.asarray(power, dtype=np.float64)
    n, peak = x.size, int(peak)
    if not 0 <= peak < n:
        raise ValueError(f"peak {peak} is not an index of a curve of {n} points")
    # prominence: walk outwards until a higher sample, keep the minimum on the way
    i, left_min = peak, x[peak]
    while i >= 0 and x[i] <= x[peak]:
        left_min = min(left_min, x[i])
        i -= 1
    i, right_min = peak, x[peak]
    while i < n and x[i] <= x[peak]:
        right_min = min(right_min, x[i])
        i += 1
    prominence = x[peak] - max(left_min, right_min)
    height = x[peak] - prominence * float(rel_height)
    # the bases' positions: the left-most / right-most points of those minima, as scipy's _peak_prominences records them
    i, left_base, m = peak, peak, x[peak]
    while i >= 0 and x[i] <= x[peak]:
        if x[i] < m:
            m, left_base = x[i], i
        i -= 1
    i, right_base, m = peak, peak, x[peak]
    while i < n and x[i] <= x[peak]:
        if x[i] < m:
            m, right_base = x[i], i
        i += 1
    i = peak
    while left_base < i and height < x[i]:
        i -= 1
    left_ip = float(i)
    if x[i] < height:
        left_ip += (height - x[i]) / (x[i + 1] - x[i])
    i = peak
    while i < right_base and height < x[i]:
        i += 1
    right_ip = float(i)
    if x[i] < height:
        right_ip -= (height - x[i]) / (x[i - 1] - x[i])
    return right_ip - left_ip


def focus_from_transverse_band(zyx, NA_det: float, lambda_ill: float, pixel_size: float,
                               midband_fractions=DEFAULT_MIDBAND_FRACTIONS, mode: str = "max", threshold_FWHM: float = 0,
                               return_statistics: bool = False, center_crop_xy=DEFAULT_CENTER_CROP_XY,
                               polynomial_fit_order=None, enable_subpixel_precision: bool = False, plot_path=None):
    """The in-focus plane of a ``(Z, Y, X)`` stack (module docstring): an int, or ``None`` when the peak is narrower than
    ``threshold_FWHM``; with ``return_statistics`` a pair ``(index, {"peak_index", "peak_FWHM", "midband_power"})``.
    ``polynomial_fit_order``, ``enable_subpixel_precision`` and ``plot_path`` are waveorder's [RECALLED] and not built."""
    if polynomial_fit_order is not None:
        raise NotImplementedError("polynomial_fit_order (a polynomial fit of the power curve) is not built")
    if enable_subpixel_precision:
        raise NotImplementedError("enable_subpixel_precision (a sub-plane focus index) is not built")
    if plot_path is not None:
        raise NotImplementedError("plot_path (plotting the power curve) is not built")
    if mode not in ("max", "min"):
        raise ValueError(f"mode must be 'max' or 'min', got {mode!r}")
    if len(zyx.shape) != 3:
        raise ValueError(f"zyx must be (Z, Y, X), got shape {tuple(zyx.shape)}")
    if int(zyx.shape[0]) == 1:
        stats = {"peak_index": 0, "peak_FWHM": None, "midband_power": None}
        return (0, stats) if return_statistics else 0
    power = midband_power(zyx, NA_det, lambda_ill, pixel_size, midband_fractions, center_crop_xy)
    curve = power.cpu().numpy() if hasattr(power, "cpu") else np.asarray(power)
    peak = int(np.argmax(curve) if mode == "max" else np.argmin(curve))
    width = peak_width(curve, peak, 0.5)
    index = peak if width >= float(threshold_FWHM) else None
    if return_statistics:
        return index, {"peak_index": peak, "peak_FWHM": float(width), "midband_power": curve}
    return index
