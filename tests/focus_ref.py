"""Float64 NumPy model of the focus measure and the drift rule (``shrimpy_amd/focus.py``, ``shrimpy_amd/stabilize.py``):
the test oracle of ``test_focus_*`` and ``test_stabilize_*``.  waveorder and biahub are not installed: PARITY UNPINNED, the
rule is the package's own and this file restates it independently -- ``np.fft.fft2`` in float64, the band's mask from ``r``
directly (not from the interval table, so the table is checked too), ``scipy.signal.peak_widths`` for the width.
"""

from __future__ import annotations

import warnings

import numpy as np

from scipy.ndimage import gaussian_filter
from scipy.signal import peak_widths

from shrimpy_amd.focus import focus_grid

# cutoff * pixel_size = 1.4 cycles per pixel with the default fractions: a band of 0.175 .. 0.35 cycles per pixel
OPTICS = dict(NA_det=0.7, lambda_ill=1.0, pixel_size=1.0)
FRACTIONS = (0.125, 0.25)

# (Z, Y, X, z0)
CASES = [(5, 12, 16, 3), (7, 30, 40, 2), (9, 64, 72, 6), (6, 50, 100, 1), (11, 128, 160, 4)]


def stack(Z, Y, X, z0, seed=None):
    """Plane z = 100 + 400 gaussian_filter(U(0,1) texture, 0.6 |z - z0|, wrap), Poisson noise, float32; seed Z Y X."""
    rng = np.random.default_rng(Z * Y * X if seed is None else seed)
    tex = rng.uniform(0, 1, (Y, X))
    vol = np.stack([100 + 400 * gaussian_filter(tex, 0.6 * abs(z - z0), mode="wrap") for z in range(Z)]).astype(np.float32)
    return rng.poisson(vol).astype(np.float32)


# name -> (volume arguments, keyword arguments of the power call beyond OPTICS)
def extra_cases():
    return {
        # a crop with non-zero offsets: (50, 100) planes, window (32, 48) at (9, 26)
        "crop": ((6, 50, 100, 1), dict(center_crop_xy=(32, 48))),
        # an odd-factor window: (46, 62) planes -> Yc = 45, Xc = 60
        "odd": ((5, 46, 62, 2), dict()),
        # a band that reaches the column X / 2 (weight 1): cutoff f1 p = 0.56 > 0.5
        "nyquist": ((5, 24, 32, 2), dict(midband_fractions=(0.2, 0.4))),
    }


EMPTY_BAND = ((3, 12, 16, 1), dict(midband_fractions=(0.0001, 0.0002)))


def window(volume, center_crop_xy=(800, 800)):
    yc, xc, y0, x0 = focus_grid(volume.shape, center_crop_xy)
    return np.asarray(volume)[:, y0:y0 + yc, x0:x0 + xc]


def band_mask(Y, X, NA_det, lambda_ill, pixel_size, midband_fractions=FRACTIONS):
    """Boolean (Y, X): cutoff f0 < r < cutoff f1 on the full spectrum."""
    cutoff = 2.0 * float(NA_det) / float(lambda_ill)
    ky, kx = np.arange(Y), np.arange(X)
    fy = np.minimum(ky, Y - ky) / (float(Y) * float(pixel_size))
    fx = np.minimum(kx, X - kx) / (float(X) * float(pixel_size))
    r = np.sqrt(fy[:, None] * fy[:, None] + fx[None, :] * fx[None, :])
    return (r > cutoff * float(midband_fractions[0])) & (r < cutoff * float(midband_fractions[1]))


def power(volume, NA_det, lambda_ill, pixel_size, midband_fractions=FRACTIONS, center_crop_xy=(800, 800), dtype=np.float64):
    """P[z], float64 (``dtype=np.complex64``-style evaluation: pass ``np.float32`` to have pocketfft work in single)."""
    import scipy.fft as sf

    win = window(volume, center_crop_xy)
    mask = band_mask(win.shape[1], win.shape[2], NA_det, lambda_ill, pixel_size, midband_fractions)
    if not mask.any():
        raise ValueError("the band holds no bin")
    return np.array([np.abs(sf.fft2(plane.astype(dtype))).astype(np.float64)[mask].sum() for plane in win])


def bound(volume, NA_det, lambda_ill, pixel_size, midband_fractions=FRACTIONS, center_crop_xy=(800, 800)):
    """Per plane: 32 u (log2 Xc + log2 Yc) W sqrt(Yc Xc) rms(v), u = 2^-24 -- the per-coefficient constant the LDS
    transforms carry in tests/test_fft_kernels_fp64_gpu.py, per leg, times the number of bins that are added up."""
    win = window(volume, center_crop_xy).astype(np.float64)
    yc, xc = win.shape[1:]
    w = int(band_mask(yc, xc, NA_det, lambda_ill, pixel_size, midband_fractions).sum())
    rms = np.sqrt(np.mean(win * win, axis=(1, 2)))
    return 32.0 * 2.0 ** -24 * (np.log2(xc) + np.log2(yc)) * w * np.sqrt(yc * xc) * rms


def width(curve, peak):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (a peak of prominence 0 -- mode="min" -- makes scipy warn)
        return float(peak_widths(np.asarray(curve, dtype=np.float64), [int(peak)], rel_height=0.5)[0][0])


def focus_index(curve, mode="max", threshold_FWHM=0.0):
    curve = np.asarray(curve, dtype=np.float64)
    if curve.size == 1:
        return 0
    peak = int(np.argmax(curve) if mode == "max" else np.argmin(curve))
    return peak if width(curve, peak) >= threshold_FWHM else None


def fill_forward(indices):
    """A ``None`` takes the previous valid index, leading ones the first valid one; all ``None`` is an error."""
    valid = [i for i in indices if i is not None]
    if not valid:
        raise ValueError("no timepoint has a focus index")
    out, last = [], valid[0]
    for i in indices:
        last = last if i is None else i
        out.append(last)
    return out


def pcc_model(ref, mov):
    """The integer shift s with mov = roll(ref, s): argmax of the circular cross-correlation, float64."""
    f = np.fft.fftn(np.asarray(mov, dtype=np.float64)) * np.conj(np.fft.fftn(np.asarray(ref, dtype=np.float64)))
    corr = np.fft.ifftn(f).real
    peak = np.unravel_index(int(np.argmax(corr)), corr.shape)
    return tuple(int(p) if p <= n // 2 else int(p) - n for p, n in zip(peak, corr.shape))


def drift_series(volumes, method, kind, t_reference="first", threshold_FWHM=0.0):
    """List of 4x4 matrices, one per timepoint (the drift rule of the issue, restated)."""
    volumes = [np.asarray(v) for v in volumes]
    T = len(volumes)
    shifts = np.zeros((T, 3))
    if method == "focus-finding":
        f = fill_forward([focus_index(power(v, **OPTICS), threshold_FWHM=threshold_FWHM) for v in volumes])
        shifts[:, 0] = [i - f[0] for i in f]
    if method == "phase-cross-corr" or kind == "xyz":
        if t_reference == "first":
            s = np.array([pcc_model(volumes[0], v) for v in volumes], dtype=np.float64)
        else:
            steps = [(0, 0, 0)] + [pcc_model(volumes[t - 1], volumes[t]) for t in range(1, T)]
            s = np.cumsum(np.array(steps, dtype=np.float64), axis=0)
        if method == "phase-cross-corr":
            shifts[:] = s
            if kind == "xy":
                shifts[:, 0] = 0
        else:
            shifts[:, 1:] = s[:, 1:]
    out = []
    for t in range(T):
        m = np.eye(4)
        m[:3, 3] = shifts[t]
        out.append(m)
    return out
