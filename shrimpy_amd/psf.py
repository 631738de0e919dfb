"""Measure the PSF from a bead volume: detect beads, cut patches, average and characterise them.

The step between ``deskew`` and ``deconvolve --psf-dirpath``: ``DeconvolveSettings.psf_path`` reads "an averaged bead
volume as the PSF-characterisation tools around the reference write them"; this module produces one.  The reference does
it in ``scripts/measure_psf.py`` through biahub's ``_characterize_psf`` (``:17, 194-203, 253-263``), which is not vendored
and whose arithmetic is therefore not available: **PARITY UNPINNED**.  Only the field names of the settings follow the
reference's call sites (``scripts/measure_psf.py:20-50``); the rule below is this package's own, restated in NumPy /
float64 by ``tests/psf_ref.py``.

Detection (exact, integer result).  The volume is smoothed with ``blur_kernel_size`` equal taps per axis (1 = no
smoothing; ``lsr_box_smooth_f32``: one pass per axis with float64 sums and float64 results between the passes, rounded to
float32 once -- three chained float32 passes of ``lsr_blur_reflect_f32`` drift up to 3 units of 2^-24 from the float64
filter, beyond the 2 this stage is held to); voxel ``p`` of the smoothed volume ``s`` is a peak iff ``s(p) >=
threshold_abs``, ``s(p) >= s(q)`` for every in-volume ``q`` within ``min_distance`` of it per axis and ``s(p) > s(q)`` for
every such ``q`` of smaller linear index (of tied maxima in reach of each other the first in C order wins; a NaN is never
a peak and leaves none within its reach).  The full-volume work -- smoothing and the separable running maximum fused with
the test -- runs where the volume lives (``csrc/peaks.hip`` on a HIP device, the host twins on a CPU tensor); only the
peak list crosses to the host, which orders it (value descending, linear index ascending) and applies ``exclude_border``,
the isolation test and ``max_num_peaks``.

Averaging.  Patches are centred on the integer peak; per bead ``B`` = the mean of the patch's six faces and ``S =
sum(patch - B)``, the PSF is the mean of ``(patch - B) / S`` over the isolated beads with ``S > 0`` (float64, list order:
the same bits on the device and on the host).  It is not clipped (``DeconvolveSettings.load_psf`` clips on use).
The FWHM always reported is the linearly interpolated width of ``patch - B`` at half its peak along each axis through
the peak voxel.

Gaussian fits (``gaussian_fit``, :func:`fit_beads`; ``csrc/psf_fit.hip``, one workgroup per bead, or its host twin).  On
the patch around each peak, ``r`` the voxel offset from the peak voxel, ``m(r) = B + A exp(-(r - mu)^T W (r - mu) / 2)`` with a
symmetric 3 x 3 precision ``W`` is fitted by unweighted least squares: Levenberg-Marquardt with Marquardt's diagonal
scaling in float64, ``lambda`` from 1e-3, / 10 on an accepted step (trial cost <= cost), * 10 on a rejected one.  Start:
``B0`` the face mean, ``A0 = d(0) - B0``, ``mu0`` and a diagonal ``W0`` from the moments of ``g = max(d - B0 - A0 / 2, 0)``,
the part of the bead above its half maximum: ``mu0 = sum(g r) / sum(g)``, ``sigma0_i^2 = max(var_i(g) / c, 1 / 4)`` with ``c
= 0.18887`` the second moment of a unit Gaussian cut at its half maximum (``csrc/psf_fit.hpp``).  The fit has converged
when a step moves every ``mu`` by less than 1e-9 voxel and the cost by at most 1e-12 of itself (an accepted step, or a
rejected one: ``theta`` is kept); it gives up after ``fit_max_iter`` trial cost evaluations.  Status per bead: 0 converged,
1 iteration limit, 2 a system or the final ``W`` not positive definite, 3 some ``|mu_i| >= 1``, 4 ``A <= 0``, 5 a
non-finite voxel or a patch that does not fit; parameters are NaN unless the status is 0.  Widths on the host in float64:
``2 sqrt(2 ln 2) / sqrt(W_ii)`` along each axis through the centre, and ``2 sqrt(2 ln 2) / sqrt(eigenvalue)`` along the
principal axes of ``W`` (``numpy.linalg.eigh``), widest first.  Device and twin agree to rounding, not to the bit.

Sub-voxel alignment (``alignment="subvoxel"``, :func:`average_psf_aligned`).  Each patch ``patch - B`` is moved by its
fitted ``mu`` with the periodic-sinc (Fourier) shift before it is added: three separable circulant passes, x, y, z, with
the Dirichlet weights ``w[k] = D_N(k + mu)``, ``D_N(t) = sin(pi t) / (N sin(pi t / N))`` of an axis of ``N`` voxels --
exact for band-limited data, where integer alignment averages the PSF with a one-voxel box and linear or cubic resampling
flattens the peak (DESIGN section 4 has the numbers).  The weights are computed here in float64 and handed to the kernel,
which adds the shifted patches over ``S`` in list order in float64: the same bits on the device and on the host.  The
beads averaged are the isolated ones whose fit has status 0 (the others are listed as ``unfit``) and whose ``S > 0``.
"""

from __future__ import annotations

import ctypes

from dataclasses import dataclass

import numpy as np

from . import _lib

__all__ = ["MAX_HALF_WIDTH", "PsfCharacterization", "BeadFits", "smooth", "local_maxima", "detect_peaks", "isolated_mask",
           "average_psf", "fit_beads", "shift_weights", "average_psf_aligned", "fwhm_vox", "characterize_psf"]

MAX_HALF_WIDTH = 64            # csrc/peaks.hpp kMaxHalfWidth
DEFAULT_CAPACITY = 1 << 20     # peaks the device buffer holds (12 bytes each)


def _is_host(t) -> bool:
    return t.device.type == "cpu"


def _check_volume(volume):
    import torch

    if not isinstance(volume, torch.Tensor):
        raise TypeError(f"volume must be a torch.Tensor, got {type(volume).__name__}")
    if volume.dtype != torch.float32:
        raise TypeError(f"volume must be float32, got {volume.dtype}")
    if volume.dim() != 3:
        raise ValueError(f"volume must be (Z, Y, X), got shape {tuple(volume.shape)}")
    if not volume.is_contiguous():
        raise ValueError("volume must be contiguous")
    if volume.device.type not in ("cpu", "cuda"):
        raise ValueError(f"volume is on {volume.device}: a HIP device or the CPU")
    return volume


def _call(volume, name, *args):
    """Entry point ``name`` on the volume's device (stream last), or its host twin."""
    import torch

    if _is_host(volume):
        from .host import _threads

        _threads()
        _lib.call(name + "_cpu", *args, None)
    else:
        with torch.cuda.device(volume.device):
            _lib.call(name, *args, _lib.stream_ptr(volume.device))


def _half_widths(min_distance) -> tuple[int, int, int]:
    r = (min_distance,) * 3 if np.isscalar(min_distance) else tuple(min_distance)
    if len(r) != 3 or any(int(v) != v or v < 0 for v in r):
        raise ValueError(f"min_distance must be a non-negative integer or three of them, got {min_distance!r}")
    r = tuple(int(v) for v in r)
    if max(r) > MAX_HALF_WIDTH:
        raise ValueError(f"min_distance {r}: the window half-widths are limited to {MAX_HALF_WIDTH} per axis")
    return r


def smooth(volume, blur_kernel_size: int = 3):
    """The smoothed volume detection runs on: ``blur_kernel_size`` (odd) equal taps ``float32(1 / b)`` per axis,
    mirrored borders, float64 sums rounded to float32 once (``lsr_box_smooth_f32``); ``1`` returns ``volume`` itself."""
    import torch

    vol = _check_volume(volume)
    b = int(blur_kernel_size)
    if b != blur_kernel_size or b < 1 or b % 2 == 0:
        raise ValueError(f"blur_kernel_size must be a positive odd integer, got {blur_kernel_size!r}")
    if b == 1:
        return vol
    r = b // 2
    if r > MAX_HALF_WIDTH or r >= min(vol.shape):
        raise ValueError(f"blur_kernel_size {b} needs every extent of the volume {tuple(vol.shape)} above {r} (and b <= 129)")
    z, y, x = (int(v) for v in vol.shape)
    out = torch.empty_like(vol)
    scratch = None
    if not _is_host(vol):
        nbytes = ctypes.c_int64(0)
        _lib.call("lsr_box_smooth_scratch_bytes", z, y, x, ctypes.byref(nbytes))
        scratch = torch.empty(nbytes.value // 8, dtype=torch.float64, device=vol.device)
    _call(vol, "lsr_box_smooth_f32", vol.data_ptr(), out.data_ptr(), z, y, x, b, ctypes.c_float(np.float32(1.0 / b)),
          None if scratch is None else scratch.data_ptr())
    return out


def local_maxima(smoothed, min_distance, threshold_abs: float, capacity: int = DEFAULT_CAPACITY):
    """Every peak of ``smoothed`` under the rule above, unordered: ``(linear indices int64, values float32)`` as NumPy
    arrays.  ``capacity``: the peaks the buffers hold; more than that is a ``ValueError`` (raise ``threshold_abs``)."""
    import torch

    s = _check_volume(smoothed)
    rz, ry, rx = _half_widths(min_distance)
    thr = float(threshold_abs)
    if np.isnan(thr):
        raise ValueError("threshold_abs is NaN")
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError("capacity must be positive")
    z, y, x = (int(v) for v in s.shape)
    dev = s.device
    index = torch.empty(capacity, dtype=torch.int64, device=dev)
    value = torch.empty(capacity, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = None
    if not _is_host(s):
        nbytes = ctypes.c_int64(0)
        _lib.call("lsr_local_max_scratch_bytes", z, y, x, ctypes.byref(nbytes))
        scratch = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
    _call(s, "lsr_local_max_candidates_f32", s.data_ptr(), z, y, x, rz, ry, rx, ctypes.c_float(thr), index.data_ptr(),
          value.data_ptr(), capacity, count.data_ptr(), None if scratch is None else scratch.data_ptr())
    n = int(count.item())          # (the one synchronisation: the counter, then the n candidates)
    if n > capacity:
        raise ValueError(f"{n} voxels are local maxima at or above threshold_abs = {thr:g}, the buffer holds {capacity}: "
                         "raise threshold_abs (or min_distance)")
    return index[:n].cpu().numpy(), value[:n].cpu().numpy()


def isolated_mask(coords, shape, patch_shape_zyx) -> np.ndarray:
    """Per peak: the patch around it fits ``shape`` and no other peak of ``coords`` lies within ``2 * (patch // 2)`` of it
    on all three axes."""
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    half = np.asarray([int(n) // 2 for n in patch_shape_zyx], dtype=np.int64)
    fits = np.all((coords >= half) & (coords + half < np.asarray(shape, dtype=np.int64)), axis=1)
    order = np.argsort(coords[:, 0], kind="stable")
    zs = coords[order, 0]
    crowded = np.zeros(len(coords), dtype=bool)
    for k, i in enumerate(order):      # only the peaks within 2 h of it along z are looked at
        lo, hi = np.searchsorted(zs, zs[k] - 2 * half[0], "left"), np.searchsorted(zs, zs[k] + 2 * half[0], "right")
        near = order[lo:hi]
        d = np.abs(coords[near, 1:] - coords[i, 1:])
        crowded[i] = np.count_nonzero(np.all(d <= 2 * half[1:], axis=1)) > 1      # (itself is one of them)
    return fits & ~crowded


def _find(volume, min_distance, threshold_abs, blur_kernel_size, exclude_border, max_num_peaks, patch_shape_zyx, capacity):
    vol = _check_volume(volume)
    border = (exclude_border,) * 3 if np.isscalar(exclude_border) else tuple(exclude_border)
    if len(border) != 3 or any(int(v) != v or v < 0 for v in border):
        raise ValueError(f"exclude_border must be three non-negative integers, got {exclude_border!r}")
    if max_num_peaks is not None and (int(max_num_peaks) != max_num_peaks or max_num_peaks < 1):
        raise ValueError(f"max_num_peaks must be a positive integer or None, got {max_num_peaks!r}")
    s = smooth(vol, blur_kernel_size)
    lin, val = local_maxima(s, min_distance, threshold_abs, capacity)
    shape = np.asarray(vol.shape, dtype=np.int64)
    order = np.lexsort((lin, -val.astype(np.float64)))          # value descending, then linear index ascending
    lin, val = lin[order], val[order]
    coords = np.stack(np.unravel_index(lin, tuple(vol.shape)), axis=1).astype(np.int64).reshape(-1, 3)
    e = np.asarray([int(v) for v in border], dtype=np.int64)
    keep = np.all((coords >= e) & (coords <= shape - 1 - e), axis=1)
    coords, val = coords[keep], val[keep]
    iso = isolated_mask(coords, shape, patch_shape_zyx) if patch_shape_zyx is not None else None
    if max_num_peaks is not None:
        n = int(max_num_peaks)
        coords, val, iso = coords[:n], val[:n], (None if iso is None else iso[:n])
    return coords, val.astype(np.float32), iso


def detect_peaks(volume, *, min_distance, threshold_abs, blur_kernel_size: int = 3, exclude_border=(0, 0, 0),
                 max_num_peaks=None, capacity: int = DEFAULT_CAPACITY):
    """Bead positions in ``volume`` (float32 ``(Z, Y, X)``, HIP device or CPU): ``(coords int64 (N, 3), values float32
    (N,))`` as CPU tensors, ordered by smoothed value descending, then linear index ascending.

    ``min_distance``: the window half-widths (one integer or ``(rz, ry, rx)``, each <= 64); ``threshold_abs``: the least
    smoothed value of a peak; ``blur_kernel_size``: odd, the box smoothing (1 = none); ``exclude_border``: peaks closer
    than ``(ez, ey, ex)`` voxels to a face are dropped; ``max_num_peaks``: keep the first N."""
    import torch

    coords, val, _ = _find(volume, min_distance, threshold_abs, blur_kernel_size, exclude_border, max_num_peaks, None, capacity)
    return torch.from_numpy(np.ascontiguousarray(coords)), torch.from_numpy(np.ascontiguousarray(val))


def _patch_shape(patch_shape_zyx, shape) -> tuple[int, int, int]:
    p = tuple(patch_shape_zyx)
    if len(p) != 3 or any(int(n) != n or n < 1 or int(n) % 2 == 0 for n in p):
        raise ValueError(f"patch_shape_zyx must be three odd positive integers, got {patch_shape_zyx!r}")
    p = tuple(int(n) for n in p)
    if max(p) > 129:
        raise ValueError(f"patch_shape_zyx {p}: at most 129 per axis (what psf_shape_zyx takes)")
    if any(n > s for n, s in zip(p, shape)):
        raise ValueError(f"patch_shape_zyx {p} is larger than the volume {tuple(int(s) for s in shape)}")
    return p


def average_psf(volume, peaks, patch_shape_zyx, return_stats: bool = False):
    """The average PSF over the beads at ``peaks`` ((N, 3) integer ZYX positions, every patch inside the volume):
    ``(psf, skipped)`` -- a float32 ``patch_shape_zyx`` tensor on the volume's device and the indices (into ``peaks``) of
    the beads left out because their background-subtracted flux ``S`` is not positive.  ``return_stats``: also the
    ``(N, 2)`` float64 array of ``(B, S)`` per bead."""
    import torch

    vol = _check_volume(volume)
    shape = tuple(int(v) for v in vol.shape)
    pz, py, px = _patch_shape(patch_shape_zyx, shape)
    coords = np.asarray(peaks.cpu().numpy() if isinstance(peaks, torch.Tensor) else peaks, dtype=np.int64).reshape(-1, 3)
    if len(coords) == 0:
        raise ValueError("no beads to average")
    half = np.array([pz // 2, py // 2, px // 2])
    if not np.all((coords >= half) & (coords + half < np.asarray(shape))):
        raise ValueError(f"a {pz}x{py}x{px} patch around one of the peaks does not fit the volume {shape}")
    lin = np.ravel_multi_index(tuple(coords.T), shape).astype(np.int64)
    centres = torch.from_numpy(lin).to(vol.device)
    stats = torch.empty((len(lin), 2), dtype=torch.float64, device=vol.device)
    psf = torch.empty((pz, py, px), dtype=torch.float32, device=vol.device)
    _call(vol, "lsr_psf_accumulate_f32", vol.data_ptr(), *shape, centres.data_ptr(), len(lin), pz, py, px, stats.data_ptr(),
          psf.data_ptr())
    stats_h = stats.cpu().numpy()
    skipped = np.flatnonzero(~(stats_h[:, 1] > 0)).astype(np.int64)
    if len(skipped) == len(lin):
        raise ValueError("no bead has a positive background-subtracted flux: nothing to average")
    return (psf, skipped, stats_h) if return_stats else (psf, skipped)


FWHM_PER_SIGMA = 2.0 * np.sqrt(2.0 * np.log(2.0))
FIT_STATUS = {0: "converged", 1: "iteration limit", 2: "not positive definite", 3: "centre a voxel or more off the peak",
              4: "no positive amplitude", 5: "non-finite voxel or the patch does not fit"}


@dataclass
class BeadFits:
    """Result of :func:`fit_beads`: one row per bead, NaN where ``status != 0`` (-1: the bead was not fitted)."""

    background: np.ndarray              # (N,) B
    amplitude: np.ndarray               # (N,) A
    offset_zyx: np.ndarray              # (N, 3) mu: the centre's offset from the peak voxel, voxels
    centre_zyx: np.ndarray              # (N, 3) peak + mu, voxels
    precision: np.ndarray               # (N, 3, 3) W, ZYX order
    cost: np.ndarray                    # (N,) final sum of squared residuals
    status: np.ndarray                  # (N,) int32, FIT_STATUS
    fwhm_axis_zyx: np.ndarray           # (N, 3) 2 sqrt(2 ln 2) / sqrt(W_ii): the cut along each axis through the centre
    fwhm_principal: np.ndarray          # (N, 3) along the principal axes of W, widest first
    principal_axes: np.ndarray          # (N, 3, 3) principal_axes[i, k] = the unit ZYX vector of fwhm_principal[i, k]

    def __len__(self) -> int:
        return len(self.status)


def principal_widths(precision, zyx_scale=(1.0, 1.0, 1.0)):
    """``(fwhm (N, 3) widest first, axes (N, 3, 3) as rows)`` of the Gaussians with precisions ``precision`` (N, 3, 3) in
    voxels, measured in units of ``zyx_scale`` per voxel; NaN rows stay NaN."""
    w = np.asarray(precision, dtype=np.float64).reshape(-1, 3, 3)
    inv = 1.0 / np.asarray(zyx_scale, dtype=np.float64)
    fwhm, axes = np.full((len(w), 3), np.nan), np.full((len(w), 3, 3), np.nan)
    for i, m in enumerate(w):
        if not np.isfinite(m).all():
            continue
        val, vec = np.linalg.eigh(m * inv[:, None] * inv[None, :])         # ascending eigenvalues: widest first
        if val[0] > 0:
            fwhm[i], axes[i] = FWHM_PER_SIGMA / np.sqrt(val), vec.T
    return fwhm, axes


def _bead_fits(theta, status, coords) -> BeadFits:
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, 12)
    w = np.empty((len(theta), 3, 3))
    for (i, j), k in {(0, 0): 5, (1, 1): 6, (2, 2): 7, (0, 1): 8, (0, 2): 9, (1, 2): 10}.items():
        w[:, i, j] = w[:, j, i] = theta[:, k]
    with np.errstate(invalid="ignore", divide="ignore"):
        axis = FWHM_PER_SIGMA / np.sqrt(np.stack([theta[:, 5], theta[:, 6], theta[:, 7]], axis=1))
    fwhm, axes = principal_widths(w)
    mu = theta[:, 2:5].copy()
    return BeadFits(background=theta[:, 0].copy(), amplitude=theta[:, 1].copy(), offset_zyx=mu,
                    centre_zyx=np.asarray(coords, dtype=np.float64).reshape(-1, 3) + mu, precision=w, cost=theta[:, 11].copy(),
                    status=np.asarray(status, dtype=np.int32), fwhm_axis_zyx=axis, fwhm_principal=fwhm, principal_axes=axes)


def _centres(coords, shape):
    """Linear indices of ``coords``; -1 for a position outside the volume (the kernels leave such a bead out)."""
    inside = np.all((coords >= 0) & (coords < np.asarray(shape, dtype=np.int64)), axis=1)
    lin = (coords[:, 0] * shape[1] + coords[:, 1]) * shape[2] + coords[:, 2]
    return np.where(inside, lin, -1).astype(np.int64)


def _fit(vol, coords, patch, max_iter):
    """``lsr_bead_fit_f32`` over ``coords``: the kernel's ``(theta (N, 12), status (N,))`` as NumPy arrays."""
    import torch

    shape = tuple(int(v) for v in vol.shape)
    centres = torch.from_numpy(_centres(coords, shape)).to(vol.device)
    fit = torch.empty((len(coords), 12), dtype=torch.float64, device=vol.device)
    status = torch.empty(len(coords), dtype=torch.int32, device=vol.device)
    _call(vol, "lsr_bead_fit_f32", vol.data_ptr(), *shape, centres.data_ptr(), len(coords), *patch, int(max_iter),
          fit.data_ptr(), status.data_ptr())
    return fit.cpu().numpy(), status.cpu().numpy()


def fit_beads(volume, peaks, patch_shape_zyx, max_iter: int = 100) -> BeadFits:
    """Fit a 3-D Gaussian on a constant background to the ``patch_shape_zyx`` patch around each of ``peaks`` ((N, 3)
    integer ZYX positions) -- the rule of the module docstring, ``lsr_bead_fit_f32`` where the volume lives.  A bead whose
    patch does not fit the volume gets status 5; nothing raises for a bead that cannot be fitted."""
    import torch

    vol = _check_volume(volume)
    patch = _patch_shape(patch_shape_zyx, tuple(int(v) for v in vol.shape))
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    coords = np.asarray(peaks.cpu().numpy() if isinstance(peaks, torch.Tensor) else peaks, dtype=np.int64).reshape(-1, 3)
    if len(coords) == 0:
        raise ValueError("no beads to fit")
    return _bead_fits(*_fit(vol, coords, patch, max_iter), coords)


def shift_weights(offsets, n: int) -> np.ndarray:
    """Dirichlet weights of the periodic-sinc shift along an axis of ``n`` (odd) voxels: row ``i`` holds ``w[k] = D_n(k +
    offsets[i])``, ``D_n(t) = sin(pi t) / (n sin(pi t / n))``, float64.  ``sin(pi (k + mu))`` is taken as ``(-1)^k sin(pi
    mu)``, so an offset of exactly 0 gives exactly the delta ``(1, 0, ..., 0)``."""
    mu = np.asarray(offsets, dtype=np.float64).reshape(-1, 1)
    k = np.arange(int(n), dtype=np.float64)[None, :]
    sign = np.where(np.arange(int(n)) % 2 == 0, 1.0, -1.0)[None, :]
    den = n * np.sin(np.pi * ((k + mu) / n))
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(den == 0.0, 1.0, sign * np.sin(np.pi * mu) / den)
    return w + 0.0                     # (-0.0 -> 0.0)


def _average_shifted(vol, coords, mu, patch):
    """The shifted average over ``coords`` with offsets ``mu`` (a NaN row leaves its bead out): ``(psf, stats, used)``."""
    import torch

    shape = tuple(int(v) for v in vol.shape)
    pz, py, px = patch
    weights = np.ascontiguousarray(np.concatenate([shift_weights(mu[:, a], n) for a, n in enumerate(patch)], axis=1))
    centres = torch.from_numpy(_centres(coords, shape)).to(vol.device)
    w = torch.from_numpy(weights).to(vol.device)
    stats = torch.empty((len(coords), 2), dtype=torch.float64, device=vol.device)
    psf = torch.empty(patch, dtype=torch.float32, device=vol.device)
    scratch = None
    if not _is_host(vol):
        nbytes = ctypes.c_int64(0)
        _lib.call("lsr_psf_shift_scratch_bytes", len(coords), pz, py, px, ctypes.byref(nbytes))
        scratch = torch.empty(nbytes.value // 8, dtype=torch.float64, device=vol.device)
    _call(vol, "lsr_psf_accumulate_shifted_f32", vol.data_ptr(), *shape, centres.data_ptr(), len(coords), pz, py, px,
          stats.data_ptr(), w.data_ptr(), None if scratch is None else scratch.data_ptr(), psf.data_ptr())
    stats_h = stats.cpu().numpy()
    used = (stats_h[:, 1] > 0) & np.isfinite(weights).all(axis=1)
    return psf, stats_h, used


def average_psf_aligned(volume, peaks, centre_zyx, patch_shape_zyx, return_stats: bool = False):
    """:func:`average_psf` with every patch moved onto its sub-voxel centre first: ``centre_zyx`` ((N, 3) float, voxels,
    e.g. ``fit_beads(...).centre_zyx``) is where each bead really sits, ``mu = centre_zyx - peaks`` the offset the
    periodic-sinc shift takes out (``|mu_i| < 1``, anything else is a ``ValueError``).  Returns ``(psf, skipped)`` as
    :func:`average_psf` does; with ``mu = 0`` everywhere the same bits."""
    import torch

    vol = _check_volume(volume)
    shape = tuple(int(v) for v in vol.shape)
    patch = _patch_shape(patch_shape_zyx, shape)
    coords = np.asarray(peaks.cpu().numpy() if isinstance(peaks, torch.Tensor) else peaks, dtype=np.int64).reshape(-1, 3)
    if len(coords) == 0:
        raise ValueError("no beads to average")
    half = np.array([n // 2 for n in patch])
    if not np.all((coords >= half) & (coords + half < np.asarray(shape))):
        raise ValueError(f"a {patch[0]}x{patch[1]}x{patch[2]} patch around one of the peaks does not fit the volume {shape}")
    centre = np.asarray(centre_zyx.cpu().numpy() if isinstance(centre_zyx, torch.Tensor) else centre_zyx, dtype=np.float64)
    if centre.shape != coords.shape:
        raise ValueError(f"centre_zyx must have the shape of peaks {coords.shape}, got {centre.shape}")
    mu = centre - coords
    if not np.all(np.abs(mu) < 1.0):
        raise ValueError("centre_zyx must lie within one voxel of its peak on every axis (|mu| < 1, finite)")
    psf, stats, used = _average_shifted(vol, coords, mu, patch)
    skipped = np.flatnonzero(~used).astype(np.int64)
    if len(skipped) == len(coords):
        raise ValueError("no bead has a positive background-subtracted flux: nothing to average")
    return (psf, skipped, stats) if return_stats else (psf, skipped)


def _shell_mean(patch: np.ndarray) -> float:
    shell = np.ones(patch.shape, dtype=bool)
    if min(patch.shape) > 2:
        shell[1:-1, 1:-1, 1:-1] = False
    return float(patch[shell].mean())


def _fwhm_1d(p: np.ndarray) -> float:
    c = len(p) // 2
    if not p[c] > 0:
        return float("nan")
    half = p[c] / 2
    width = 0.0
    for step in (-1, 1):
        i = c
        while 0 <= i + step < len(p) and p[i + step] >= half:
            i += step
        if not 0 <= i + step < len(p):
            return float("nan")
        width += abs(i - c) + (p[i] - half) / (p[i] - p[i + step])
    return float(width)


def fwhm_vox(patch, background: float | None = None) -> np.ndarray:
    """FWHM in voxels along z, y, x through the centre voxel of ``patch``: the linearly interpolated half-maximum
    crossings of ``patch - background`` on either side (float64; NaN where a crossing is missing inside the patch).
    ``background`` defaults to the mean of the patch's six faces."""
    p = np.asarray(patch, dtype=np.float64)
    p = p - (_shell_mean(p) if background is None else float(background))
    c = tuple(n // 2 for n in p.shape)
    return np.array([_fwhm_1d(p[:, c[1], c[2]]), _fwhm_1d(p[c[0], :, c[2]]), _fwhm_1d(p[c[0], c[1], :])])


@dataclass
class PsfCharacterization:
    """Result of :func:`characterize_psf`."""

    psf: "object"                       # float32 (pz, py, px) tensor on the volume's device, unclipped
    peaks: np.ndarray                   # (N, 3) int64 ZYX, ordered as detect_peaks orders them
    values: np.ndarray                  # (N,) float32 smoothed value at each peak
    isolated: np.ndarray                # (N,) bool: the beads whose patches are averaged
    skipped: np.ndarray                 # indices into `peaks` of isolated beads left out (flux S <= 0)
    fwhm_vox_zyx: np.ndarray            # (N, 3) float64 per bead, NaN for beads that are not isolated
    psf_fwhm_vox_zyx: np.ndarray        # (3,) of the average
    patch_shape_zyx: tuple
    zyx_scale: tuple
    # only when the Gaussian fit ran (settings.gaussian_fit, or alignment == "subvoxel" which implies it)
    fit: "BeadFits | None" = None       # one row per peak: the isolated beads' fits, NaN (status -1) elsewhere
    psf_fit: "BeadFits | None" = None   # one row: the same fit of the averaged PSF
    unfit: "np.ndarray | None" = None   # subvoxel alignment: indices into `peaks` of isolated beads left out for their fit status
    alignment: str = "voxel"

    @property
    def n_averaged(self) -> int:
        return int(np.count_nonzero(self.isolated)) - len(self.skipped) - (0 if self.unfit is None else len(self.unfit))

    def report(self) -> dict:
        """Counts and mean / median FWHM in voxels and physical units (plain Python numbers)."""
        used = self.isolated.copy()
        used[self.skipped] = False
        if self.unfit is not None:
            used[self.unfit] = False
        f = self.fwhm_vox_zyx[used]
        scale = np.asarray(self.zyx_scale, dtype=np.float64)

        def stat(fn):
            with np.errstate(all="ignore"):
                v = np.array([fn(col[np.isfinite(col)]) if np.isfinite(col).any() else np.nan for col in f.T]) if len(f) else np.full(3, np.nan)
            return v

        mean, median = stat(np.mean), stat(np.median)

        def lst(a):
            return [None if not np.isfinite(v) else float(v) for v in a]
        out = {"n_peaks": int(len(self.peaks)), "n_isolated": int(np.count_nonzero(self.isolated)),
               "n_skipped": int(len(self.skipped)), "n_averaged": self.n_averaged,
               "patch_shape_zyx": [int(n) for n in self.patch_shape_zyx], "zyx_scale": [float(v) for v in scale],
               "fwhm_mean_vox_zyx": lst(mean), "fwhm_median_vox_zyx": lst(median),
               "fwhm_mean_zyx": lst(mean * scale), "fwhm_median_zyx": lst(median * scale),
               "psf_fwhm_vox_zyx": lst(self.psf_fwhm_vox_zyx), "psf_fwhm_zyx": lst(self.psf_fwhm_vox_zyx * scale)}
        if self.fit is None:
            return out
        good = used & (self.fit.status == 0)

        def med(a):
            return lst(np.median(a[good], axis=0)) if good.any() else [None] * 3
        out.update(fit_fwhm_axis_median_vox_zyx=med(self.fit.fwhm_axis_zyx), fit_fwhm_axis_median_zyx=med(self.fit.fwhm_axis_zyx * scale),
                   fit_fwhm_principal_median_vox=med(self.fit.fwhm_principal),
                   fit_fwhm_principal_median=med(principal_widths(self.fit.precision, scale)[0]),
                   n_unfit=0 if self.unfit is None else int(len(self.unfit)), alignment=self.alignment)
        if self.psf_fit is not None:
            p = self.psf_fit
            out.update(psf_fit_status=int(p.status[0]), psf_fit_fwhm_axis_vox_zyx=lst(p.fwhm_axis_zyx[0]),
                       psf_fit_fwhm_axis_zyx=lst(p.fwhm_axis_zyx[0] * scale), psf_fit_fwhm_principal_vox=lst(p.fwhm_principal[0]),
                       psf_fit_fwhm_principal=lst(principal_widths(p.precision, scale)[0][0]),
                       psf_fit_principal_axes=[lst(row) for row in p.principal_axes[0]])
        return out


def characterize_psf(volume, settings, zyx_scale=(1.0, 1.0, 1.0), capacity: int = DEFAULT_CAPACITY) -> PsfCharacterization:
    """Detect the beads of ``volume`` with ``settings`` (:class:`shrimpy_amd.settings.CharacterizeSettings`), average
    the patches of the isolated ones and measure their widths.  ``zyx_scale``: the voxel size ``patch_size`` is
    converted with (and the report's physical units)."""
    vol = _check_volume(volume)
    shape = tuple(int(v) for v in vol.shape)
    patch = _patch_shape(settings.patch_shape_zyx(zyx_scale), shape)
    coords, values, iso = _find(vol, settings.min_distance, settings.threshold_abs, settings.blur_kernel_size,
                                settings.exclude_border, settings.max_num_peaks, patch, capacity)
    if not iso.any():
        raise ValueError(f"{len(coords)} peaks, none isolated for a {patch} patch in the {shape} volume: lower threshold_abs, "
                         "shrink patch_size or use a sparser bead sample")
    chosen = np.flatnonzero(iso)
    alignment = getattr(settings, "alignment", "voxel")
    fit_on = bool(getattr(settings, "gaussian_fit", False)) or alignment == "subvoxel"
    theta, status = _fit(vol, coords[chosen], patch, settings.fit_max_iter) if fit_on else (None, None)
    unfit = None
    if alignment == "subvoxel":
        good = status == 0
        if not good.any():
            raise ValueError(f"none of the {len(chosen)} isolated beads could be fitted (statuses {sorted(set(status.tolist()))}: "
                             f"{FIT_STATUS}): use alignment='voxel' or another patch_size")
        # (an unfit bead's NaN offsets give it NaN weights: the kernel leaves it out and still reports its B and S)
        psf, stats, used = _average_shifted(vol, coords[chosen], theta[:, 2:5], patch)
        unfit = chosen[~good]
        skipped = np.flatnonzero(good & ~used)
        if not used.any():
            raise ValueError("no fitted bead has a positive background-subtracted flux: nothing to average")
    else:
        psf, skipped, stats = average_psf(vol, coords[chosen], patch, return_stats=True)
    half = [n // 2 for n in patch]
    fwhm = np.full((len(coords), 3), np.nan)
    for k, i in enumerate(chosen):       # a few hundred small patches: host-side float64
        z, y, x = (int(v) for v in coords[i])
        cut = vol[z - half[0]:z + half[0] + 1, y - half[1]:y + half[1] + 1, x - half[2]:x + half[2] + 1].cpu().numpy()
        fwhm[i] = fwhm_vox(cut, stats[k, 0])
    extra = {}
    if fit_on:
        all_theta, all_status = np.full((len(coords), 12), np.nan), np.full(len(coords), -1, dtype=np.int32)
        all_theta[chosen], all_status[chosen] = theta, status
        extra = dict(fit=_bead_fits(all_theta, all_status, coords), unfit=unfit, alignment=alignment,
                     psf_fit=fit_beads(psf, [[n // 2 for n in patch]], patch, settings.fit_max_iter))
    return PsfCharacterization(psf=psf, peaks=coords, values=values, isolated=iso, skipped=chosen[skipped],
                               fwhm_vox_zyx=fwhm, psf_fwhm_vox_zyx=fwhm_vox(psf.cpu().numpy()),
                               patch_shape_zyx=patch, zyx_scale=tuple(float(v) for v in zyx_scale), **extra)
