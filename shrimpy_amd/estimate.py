"""Estimate the affine that registers one volume onto another (label-free <-> light-sheet) on MI355X.

The "estimate" half of the registration step; ``register.apply_affine_transform_zyx`` is the "apply"
half.  The reference ships neither ("algorithms for deconvolution and registration ... are being
developed", ``docs/data_structure.md:58-62``); SURVEY.md section 8 f-4 lists the estimation as the row that
closes the register loop end to end.  What is estimated is exactly what ``RegisterSettings`` stores and
the apply kernels consume: ``affine_transform_zyx``, a 4x4 in ZYX voxel units mapping a TARGET index to
the MOVING coordinate (the ``scipy.ndimage.affine_transform`` convention).

Method: Gauss-Newton on the sum of squared differences with a linear intensity map,

    minimise  sum_x ( gain * M(A x + t) + offset - T(x) )^2 ,

coarse to fine (Gaussian blur + strided sampling of the target grid).  Each iteration is ONE launch of
``lsr_affine_normal_equations_f32`` (``csrc/estimate_affine.hip``: trilinear taps, analytic gradient,
the 14 x 14 normal equations accumulated in fp64 registers) and a 14 x 14 solve on the host; an
optional phase cross-correlation (the DynaTrack kernels) supplies the starting translation.
The SSD estimate runs on a HIP device only (its host side is a 14 x 14 solve; no host twin of the normal-equations kernel).

``metric="mi"`` replaces the criterion by Mattes-style mutual information for two channels whose intensities follow no
linear map (quantitative phase against fluorescence): a joint histogram of target intensity against interpolated moving
intensity (``lsr_affine_joint_histogram_f32``, ``csrc/estimate_mi.hip``: zero-order target bins, a linear Parzen window
on the moving value, integer weights -- the same bits on every run) and its analytic gradient
(``lsr_affine_mi_gradient_f32``), climbed by a regular-step (BFGS-directed) ascent on the same pyramid, with a
pattern search at the end of the finest level.  Both entries have host
twins, and so have the blur and the steps of the phase correlation: ``metric="mi"`` runs end to end on CPU tensors too.
No upstream implementation exists to compare against: parity unpinned, the recovery tests are the contract.
"""

from __future__ import annotations

import ctypes
import logging

from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .geometry import as_matrix_3x4

logger = logging.getLogger(__name__)

__all__ = ["RegistrationEstimate", "normal_equations", "estimate_affine_zyx", "default_levels", "joint_histogram",
           "mutual_information", "mi_gradient"]

N_PARAMS = 14          # 12 affine + gain + offset
MODELS = ("translation", "affine")
METRICS = ("ssd", "mi")
MI_WEIGHT_ONE = 65536  # one sample in the joint histogram's units


@dataclass
class RegistrationEstimate:
    """Result of :func:`estimate_affine_zyx`."""

    affine_transform_zyx: np.ndarray      # 4x4, target index -> moving coordinate
    gain: float
    offset: float
    rms: float                            # residual RMS on the finest level, in target intensity units
    n_samples: int
    iterations: int
    converged: bool
    history: list = field(default_factory=list)   # (stride, iteration, rms -- "mi": MI --, step in voxels) per accepted step
    metric: str = "ssd"
    mi: float = float("nan")              # "mi": the mutual information (nats) on the finest level

    def to_settings_dict(self, **extra) -> dict:
        """The ``RegisterSettings`` YAML mapping for this estimate."""
        return {"affine_transform_zyx": [[float(v) for v in row] for row in self.affine_transform_zyx], **extra}


def _f64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _unpack(row: np.ndarray):
    """(H 14x14 symmetric, b 14, sse, n) from one 121-entry row of sums."""
    h = np.zeros((N_PARAMS, N_PARAMS))
    h[np.triu_indices(N_PARAMS)] = row[:105]
    h = h + np.triu(h, 1).T
    return h, row[105:119].copy(), float(row[119]), int(round(row[120]))


def _stride3(stride) -> tuple[int, int, int]:
    if np.isscalar(stride):
        return (int(stride),) * 3
    st = tuple(int(v) for v in stride)
    if len(st) != 3:
        raise ValueError(f"stride must be an int or three ints, got {stride!r}")
    return st


def normal_equations(moving, target, matrix, gain: float = 1.0, offset: float = 0.0, stride=1,
                     centre=None, scale: float | None = None):
    """One launch of the normal-equations kernel: ``(H, b, sse, n)`` of the Gauss-Newton step at
    ``matrix`` (3x4 / 4x4, target index -> moving coordinate) over the target grid sampled every
    ``stride`` voxels (an int, or one per axis).  Parameter order: the 3x4 matrix row by row IN
    CENTRED, SCALED target coordinates ``((x - centre) / scale, 1)``, then gain, offset."""
    import torch

    mov = _lib.require_device_f32(moving, "moving")
    tgt = _lib.require_device_f32(target, "target")
    if mov.dim() != 3 or tgt.dim() != 3 or mov.device != tgt.device:
        raise ValueError("moving and target must be (Z, Y, X) tensors on the same device")
    m = as_matrix_3x4(matrix)
    shape = tuple(int(v) for v in tgt.shape)
    c = np.ascontiguousarray(centre if centre is not None else [(n - 1) / 2 for n in shape], dtype=np.float64)
    s = float(scale if scale is not None else max(shape) / 2)
    st = (ctypes.c_int * 3)(*_stride3(stride))
    n_out = _lib.call_value("lsr_affine_normal_size")
    n_blocks = _lib.call_value("lsr_affine_normal_blocks")
    partial = torch.empty((n_blocks, n_out), dtype=torch.float64, device=tgt.device)
    with torch.cuda.device(tgt.device):
        _lib.call("lsr_affine_normal_equations_f32", mov.data_ptr(), *(int(v) for v in mov.shape), tgt.data_ptr(),
                  *shape, _lib.matrix12(m), ctypes.c_double(float(gain)), ctypes.c_double(float(offset)), st,
                  _f64p(c), ctypes.c_double(s), partial.data_ptr(), _lib.stream_ptr(tgt.device))
    # the 256 workgroup rows are added in row order on the host: the same sums on every run
    return _unpack(partial.cpu().numpy().sum(axis=0))


def _to_normalised(m: np.ndarray, c: np.ndarray, s: float) -> np.ndarray:
    """3x4 in voxel units -> 3x4 acting on ((x - c) / s, 1)."""
    q = np.empty((3, 4))
    q[:, :3] = m[:, :3] * s
    q[:, 3] = m[:, :3] @ c + m[:, 3]
    return q


def _from_normalised(q: np.ndarray, c: np.ndarray, s: float) -> np.ndarray:
    m = np.empty((3, 4))
    m[:, :3] = q[:, :3] / s
    m[:, 3] = q[:, 3] - m[:, :3] @ c
    return m


def _corner_motion(a: np.ndarray, b: np.ndarray, shape) -> float:
    """Largest displacement (voxels) of the target volume's corners between two 3x4 maps."""
    corners = np.array([[z, y, x, 1.0] for z in (0, shape[0] - 1) for y in (0, shape[1] - 1) for x in (0, shape[2] - 1)])
    return float(np.abs(corners @ (a - b).T).max())


def default_levels(shape, max_stride: int = 32, min_samples: int = 8):
    """Coarse-to-fine schedule ``[(strides zyx, sigmas zyx), ...]`` for a target of ``shape``: strides
    halve from the coarsest level -- per axis the largest power of two (<= ``max_stride``) that still
    leaves ``min_samples`` samples along that axis -- down to 1; sigma = stride / 2 (0 at stride 1).  A
    Gauss-Newton step only sees displacements of a few sigma: the coarsest level has to span the
    largest misalignment at the volume's corners (a 2 % scale error is 20 voxels at 1024)."""
    top = []
    for n in shape:
        s = 1
        while s * 2 <= max_stride and n // (s * 2) >= min_samples:
            s *= 2
        top.append(s)
    levels = []
    k = max(top)
    while k >= 1:
        strides = tuple(min(k, t) for t in top)
        levels.append((strides, tuple(st / 2 if st > 1 else 0.0 for st in strides)))
        k //= 2
    return levels


def _blur_axes(vol, sigmas):
    """Separable Gaussian blur with a sigma per axis (reflect padding; the kernel of DESIGN.md 4.7)."""
    import torch

    if not any(sg > 0 for sg in sigmas):
        return vol
    z, y, x = (int(v) for v in vol.shape)
    src = vol
    if vol.device.type == "cpu":    # the blur's host twin (metric="mi" on CPU tensors)
        from .dynatrack import _run

        for axis, (n, sg) in enumerate(zip((z, y, x), sigmas)):
            r = min(int(4 * sg + 0.5), n - 1) if sg > 0 else 0
            if r < 1:
                continue
            xs = torch.arange(-r, r + 1, dtype=torch.float32)
            k1d = torch.exp(-0.5 * (xs / float(sg)) ** 2)
            k1d = (k1d / k1d.sum()).contiguous()
            dst = torch.empty_like(vol)
            _run(vol.device, "lsr_blur_reflect_f32", src.data_ptr(), dst.data_ptr(), z, y, x, axis, k1d.data_ptr(), r,
                 ctypes.c_float(0.0), ctypes.c_float(0.0))
            src = dst
        return src
    with torch.cuda.device(vol.device):
        stream = _lib.stream_ptr(vol.device)
        for axis, (n, sg) in enumerate(zip((z, y, x), sigmas)):
            if sg <= 0:
                continue
            r = min(int(4 * sg + 0.5), n - 1)
            if r < 1:
                continue
            xs = torch.arange(-r, r + 1, device=vol.device, dtype=torch.float32)
            k1d = torch.exp(-0.5 * (xs / float(sg)) ** 2)
            k1d = (k1d / k1d.sum()).contiguous()
            dst = torch.empty_like(vol)
            _lib.call("lsr_blur_reflect_f32", src.data_ptr(), dst.data_ptr(), z, y, x, axis, k1d.data_ptr(), r,
                      ctypes.c_float(0.0), ctypes.c_float(0.0), stream)
            src = dst
    return src


# ---------------------------------------------------------------------------------------------- mutual information


def _mi_operands(moving, target):
    """The two volumes of a mutual-information call: both on one HIP device (the kernels) or both CPU tensors (the host
    twins).  A CPU tensor beside a device tensor is refused (:class:`LsrError`), as everywhere else."""
    import torch

    from . import host

    if isinstance(moving, torch.Tensor) and isinstance(target, torch.Tensor) and host.is_host(moving) and host.is_host(target):
        mov, tgt = host._f32(moving, "moving"), host._f32(target, "target")
    else:
        mov, tgt = _lib.require_device_f32(moving, "moving"), _lib.require_device_f32(target, "target")
    if mov.dim() != 3 or tgt.dim() != 3 or mov.device != tgt.device:
        raise ValueError("moving and target must be (Z, Y, X) tensors on the same device")
    return mov, tgt


def _mi_ranges(mov, tgt, ranges):
    """``((t_lo, t_hi), (m_lo, m_hi))`` as four floats; ``None`` = the volumes' own min / max."""
    if ranges is None:
        from .dynatrack import _minmax

        ranges = (_minmax(tgt), _minmax(mov))
    (t_lo, t_hi), (m_lo, m_hi) = ranges
    return float(t_lo), float(t_hi), float(m_lo), float(m_hi)


def _mi_call(entry: str, mov, tgt, *args):
    """``entry`` on the volumes' device: the kernel on the current stream, or the host twin (no stream argument)."""
    import torch

    head = (mov.data_ptr(), *(int(v) for v in mov.shape), tgt.data_ptr(), *(int(v) for v in tgt.shape))
    if tgt.device.type == "cpu":
        from . import host

        host._threads()
        _lib.call(entry + "_cpu", *head, *args)
        return
    with torch.cuda.device(tgt.device):
        _lib.call(entry, *head, *args, _lib.stream_ptr(tgt.device))


def joint_histogram(moving, target, matrix, stride=1, bins: int = 32, ranges=None):
    """One launch of the joint-histogram kernel (CPU tensors: its host twin): ``(hist, n)`` at ``matrix`` (3x4 / 4x4,
    target index -> moving coordinate) over the target grid sampled every ``stride`` voxels.  ``hist`` is a uint64
    ``[bins, bins]`` array (rows: target bins, zero order; columns: moving bins, linear Parzen window) in units of
    2^-16 sample, so ``hist.sum() == 65536 * n``; ``n`` counts the samples whose moving coordinate lies inside the
    moving volume.  ``ranges = ((t_lo, t_hi), (m_lo, m_hi))``, default the volumes' min / max; values outside are
    clamped into the edge bins.  The sums are integer: the same array on every run, from the kernel and from the twin."""
    import torch

    mov, tgt = _mi_operands(moving, target)
    m = as_matrix_3x4(matrix)
    t_lo, t_hi, m_lo, m_hi = _mi_ranges(mov, tgt, ranges)
    bins = int(bins)
    st = (ctypes.c_int * 3)(*_stride3(stride))
    cells = max(bins, 0) ** 2
    out = torch.zeros((cells + 1,), dtype=torch.int64, device=tgt.device)     # the histogram, then the sample count
    _mi_call("lsr_affine_joint_histogram_f32", mov, tgt, _lib.matrix12(m), st, bins, ctypes.c_double(t_lo),
             ctypes.c_double(t_hi), ctypes.c_double(m_lo), ctypes.c_double(m_hi), out.data_ptr(),
             out.data_ptr() + 8 * cells)
    host = out.cpu().numpy().view(np.uint64)
    return host[:cells].reshape(bins, bins).copy(), int(host[cells])


def mutual_information(hist) -> float:
    """Mutual information (nats) of a joint histogram: ``sum P log(P / (P_t P_m))`` over its non-empty cells, in
    float64 on the host (at most 64 x 64 cells)."""
    h = np.asarray(hist, dtype=np.float64)
    total = h.sum()
    if not total > 0:
        return 0.0
    p = h / total
    outer = p.sum(axis=1)[:, None] * p.sum(axis=0)[None, :]
    nz = p > 0
    return float((p[nz] * np.log(p[nz] / outer[nz])).sum())


def _mi_dl(hist) -> np.ndarray:
    """``dL[a, b] = L[a, b + 1] - L[a, b]`` with ``L = log(P / P_m)`` (0 in empty cells): what the gradient kernel reads."""
    h = np.asarray(hist, dtype=np.float64)
    pm = h.sum(axis=0)
    big_l = np.zeros_like(h)
    nz = h > 0
    big_l[nz] = np.log((h / np.where(pm > 0, pm, 1.0)[None, :])[nz])
    return np.ascontiguousarray(big_l[:, 1:] - big_l[:, :-1])


def mi_gradient(moving, target, matrix, stride=1, bins: int = 32, ranges=None, hist=None, centre=None,
                scale: float | None = None) -> np.ndarray:
    """Gradient of the mutual information with respect to the 3x4 matrix row by row IN CENTRED, SCALED target
    coordinates ``((x - centre) / scale, 1)`` (12 values): one launch of the gradient kernel (CPU tensors: its host
    twin) with ``dL`` from ``hist`` (default: one :func:`joint_histogram` launch at the same arguments), its
    workgroup rows added in row order on the host and divided by the sample count.  Samples whose moving value is
    clamped -- or lies exactly on an end of the moving range -- contribute nothing."""
    import torch

    mov, tgt = _mi_operands(moving, target)
    m = as_matrix_3x4(matrix)
    ranges = _mi_ranges(mov, tgt, ranges)
    if hist is None:
        hist, _ = joint_histogram(mov, tgt, m, stride, bins, (ranges[:2], ranges[2:]))
    hist = np.asarray(hist)
    bins = int(bins)
    if hist.shape != (bins, bins):
        raise ValueError(f"hist must be ({bins}, {bins}), got {hist.shape}")
    n = float(hist.sum(dtype=np.float64)) / MI_WEIGHT_ONE
    if not n > 0:
        return np.zeros(12)
    shape = tuple(int(v) for v in tgt.shape)
    c = np.ascontiguousarray(centre if centre is not None else [(k - 1) / 2 for k in shape], dtype=np.float64)
    s = float(scale if scale is not None else max(shape) / 2)
    st = (ctypes.c_int * 3)(*_stride3(stride))
    dl = torch.as_tensor(_mi_dl(hist)).to(tgt.device)
    rows, width = _lib.call_value("lsr_affine_mi_gradient_blocks"), _lib.call_value("lsr_affine_mi_gradient_size")
    partial = torch.empty((rows, width), dtype=torch.float64, device=tgt.device)
    _mi_call("lsr_affine_mi_gradient_f32", mov, tgt, _lib.matrix12(m), st, _f64p(c), ctypes.c_double(s), bins,
             *(ctypes.c_double(v) for v in ranges), dl.data_ptr(), partial.data_ptr())
    # the rows are added in row order on the host: the same sums on every run
    return partial.cpu().numpy().sum(axis=0) / n


def _estimate_mi(mov, tgt, m, model, levels, max_iterations, tol, init_translation, initial_given, bins, c, s, shape):
    """The ``metric="mi"`` body of :func:`estimate_affine_zyx`: regular-step ascent of the mutual information in the
    normalised parameters.  A step moves the target volume's worst corner by at most ``length`` voxels (starting at the
    level's largest stride); one that lowers the MI or loses more than half the samples is rejected and halves the
    length; a stage ends when the length falls below ``tol * max(stride)``.  The direction is the gradient, or -- once
    two gradients are known -- the gradient through a BFGS estimate of the inverse Hessian (dropped again whenever it
    proposes a step that is refused).  One histogram launch per trial, one gradient launch per accepted step.  The
    finest level ends with a pattern search over the free parameters (two histogram launches per parameter and sweep):
    the piecewise interpolant and window leave sub-voxel ripples in the MI that stall a gradient short of the peak."""
    from .dynatrack import _minmax, _phase_cross_corr

    def measure(level, trial):
        hist, n = joint_histogram(level[0], level[1], trial, level[2], bins, level[3])
        return mutual_information(hist), n, hist

    if init_translation == "pcc" and not initial_given and tuple(mov.shape) == shape:
        shift = np.array(_phase_cross_corr(tgt, mov), dtype=np.float64)
        if np.any(shift):
            # the correlation's sign convention is settled by the data: keep whichever direction (or neither) has the
            # larger mutual information
            probe = (mov, tgt, tuple(max(2, v) for v in levels[0][0]), (_minmax(tgt), _minmax(mov)))
            best = None
            for sign in (0.0, 1.0, -1.0):
                trial = m.copy()
                trial[:, 3] += sign * shift
                value, n, _ = measure(probe, trial)
                if n > 0.25 * tgt.numel() / np.prod(probe[2]) and (best is None or value > best[0]):
                    best = (value, trial)
            if best is not None:
                m = best[1]

    history, total_iters, converged = [], 0, False
    value, n_used = float("nan"), 0
    for li, (strides, sigmas) in enumerate(levels):
        bm, bt = _blur_axes(mov, sigmas), _blur_axes(tgt, sigmas)
        level = (bm, bt, strides, (_minmax(bt), _minmax(bm)))
        value, n, hist = measure(level, m)
        if n < 64:
            raise _lib.LsrError("estimate_affine_zyx", -1, f"only {n} target samples fall inside the moving volume "
                                "at the starting transform: give a better `initial`")
        # the coarsest level settles the translation before it frees the linear part
        stages = (["translation", model] if (li == 0 and model == "affine" and len(levels) > 1) else [model])
        for kind in stages:
            free = np.zeros(12, dtype=bool)
            free[[3, 7, 11]] = True
            if kind == "affine":
                free[:] = True
            length, converged = float(max(strides)), False
            floor_length = tol * max(strides)
            grad = np.where(free, mi_gradient(level[0], level[1], m, strides, bins, level[3], hist, c, s), 0.0)
            inv_h = None             # BFGS estimate of the inverse Hessian of -MI over the free parameters (None: identity)
            for it in range(int(max_iterations)):
                q = _to_normalised(m, c, s)
                step = None
                while length >= floor_length:
                    direction = grad if inv_h is None else np.where(free, inv_h @ grad, 0.0)
                    if inv_h is not None and not direction @ grad > 0:
                        inv_h = None     # not an ascent direction: back to the gradient
                        continue
                    unit = _corner_motion(_from_normalised(q + direction.reshape(3, 4), c, s), m, shape)
                    if not unit > 0:
                        break            # a zero gradient: nowhere to go at this level
                    # the plain gradient carries no length of its own: it takes the full step; a quasi-Newton direction
                    # is cut to it
                    alpha = length / unit if inv_h is None else min(1.0, length / unit)
                    delta = alpha * direction
                    m_new = _from_normalised(q + delta.reshape(3, 4), c, s)
                    v2, n2, h2 = measure(level, m_new)
                    if n2 >= 0.5 * n and v2 > value:
                        step = (m_new, v2, n2, h2, delta, alpha * unit)
                        break
                    if inv_h is not None:
                        inv_h = None     # the curvature estimate misled: try the gradient at this length first
                    else:
                        length /= 2
                total_iters += 1
                if step is None:
                    converged = True    # no uphill step left at this level
                    break
                m, value, n, hist, delta, moved = step
                g_new = np.where(free, mi_gradient(level[0], level[1], m, strides, bins, level[3], hist, c, s), 0.0)
                y = grad - g_new         # change of the gradient of -MI along the step
                sy = float(delta @ y)
                if sy > 1e-12 * np.linalg.norm(delta) * np.linalg.norm(y):
                    if inv_h is None:
                        inv_h = np.eye(12) * (sy / float(y @ y))
                    rho = 1.0 / sy
                    left = np.eye(12) - rho * np.outer(delta, y)
                    inv_h = left @ inv_h @ left.T + rho * np.outer(delta, delta)
                else:
                    inv_h = None
                grad = g_new
                history.append((strides, it, value, moved))
            if li == len(levels) - 1 and kind == model:
                # the finest level ends with a pattern search: the interpolant and the window are piecewise, so the MI
                # has ripples of a fraction of a voxel that a gradient cannot see across.  Each free parameter in turn
                # moves the worst corner by +- length (from half a sampling pitch down to the tolerance).
                length = max(strides) / 2
                while length >= floor_length:
                    improved = False
                    for k in np.flatnonzero(free):
                        q = _to_normalised(m, c, s)
                        axis = np.zeros(12)
                        axis[k] = 1.0
                        unit = _corner_motion(_from_normalised(q + axis.reshape(3, 4), c, s), m, shape)
                        for sign in (1.0, -1.0):
                            m_new = _from_normalised(q + (sign * length / unit) * axis.reshape(3, 4), c, s)
                            v2, n2, h2 = measure(level, m_new)
                            if n2 >= 0.5 * n and v2 > value:
                                m, value, n, hist, improved = m_new, v2, n2, h2, True
                                history.append((strides, total_iters, value, length))
                                break
                    total_iters += 1
                    if not improved:
                        length /= 2
                converged = True
        n_used = n
        logger.info("estimate_affine (mi): strides %s sigmas %s -> MI %.5g on %d samples", strides, sigmas, value, n)
    out = np.eye(4)
    out[:3] = m
    return RegistrationEstimate(out, 1.0, 0.0, float("nan"), n_used, total_iters, converged, history, "mi", float(value))


def estimate_affine_zyx(moving, target, *, initial=None, model: str = "affine", intensity: bool = True,
                        levels=None, max_iterations: int = 40, tol: float = 2e-3,
                        init_translation: str | None = "pcc", metric: str = "ssd",
                        bins: int = 32) -> RegistrationEstimate:
    """Estimate ``affine_transform_zyx`` (target index -> moving coordinate) between two device volumes.

    Parameters
    ----------
    moving, target : (Z, Y, X) float32 device tensors (the result resamples ``moving`` onto ``target``'s grid).
    initial : 4x4 / 3x4 starting map; default identity (plus ``init_translation``).
    model : ``"affine"`` (12 parameters) or ``"translation"`` (3).
    intensity : also fit ``gain`` / ``offset`` of the linear intensity map (two modalities or exposures).
    levels : ``(stride, sigma)`` per resolution level, coarse to fine, each an int / float or one per
        axis: both volumes are blurred with a Gaussian of ``sigma`` voxels and the target grid is sampled
        every ``stride`` voxels.  Default: :func:`default_levels` of the target shape.
    tol : stop a level when a step moves no corner of the target volume by more than ``tol`` voxels.
    init_translation : ``"pcc"`` = whole-voxel shift from the phase cross-correlation, ``None`` = none.
    metric : ``"ssd"`` (the default: the method above) or ``"mi"``: mutual information with ``bins`` bins per axis
        (4 .. 64), for two channels whose intensities follow no linear map.  The same pyramid and blur; per level the
        intensity ranges are the min / max of the blurred volumes; ``gain`` / ``offset`` are not fitted (``intensity``
        is ignored; 1.0 and 0.0 are returned), ``rms`` is nan and ``mi`` holds the final value.  ``tol`` then bounds
        the step length: a level ends when no step of ``tol * max(stride)`` voxels at the worst corner raises the MI.
        ``max_iterations`` bounds the accepted steps of a stage.  ``"mi"`` also takes two CPU tensors (host twins).
    """
    from .dynatrack import _phase_cross_corr

    if model not in MODELS:
        raise ValueError(f"model must be one of {MODELS}, got {model!r}")
    if init_translation not in (None, "pcc"):
        raise ValueError("init_translation must be 'pcc' or None")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if metric == "mi":
        mov, tgt = _mi_operands(moving, target)
    else:
        mov = _lib.require_device_f32(moving, "moving")
        tgt = _lib.require_device_f32(target, "target")
    if mov.dim() != 3 or tgt.dim() != 3:
        raise ValueError("moving and target must be (Z, Y, X)")
    shape = tuple(int(v) for v in tgt.shape)
    if levels is None:
        levels = default_levels(shape)
    levels = [(_stride3(st), tuple(float(v) for v in (np.full(3, sg) if np.isscalar(sg) else sg))) for st, sg in levels]
    c = np.array([(n - 1) / 2 for n in shape])
    s = max(shape) / 2
    m = as_matrix_3x4(initial if initial is not None else np.eye(4)).copy()
    if metric == "mi":
        return _estimate_mi(mov, tgt, m, model, levels, max_iterations, tol, init_translation, initial is not None,
                            int(bins), c, s, shape)
    gain, offset = 1.0, 0.0
    if intensity:   # moments give the starting intensity map
        sm, st_ = float(mov.std()), float(tgt.std())
        if sm > 0 and st_ > 0:
            gain = st_ / sm
            offset = float(tgt.mean()) - gain * float(mov.mean())

    def free_mask(kind):
        free = np.zeros(N_PARAMS, dtype=bool)
        free[[3, 7, 11]] = True
        if kind == "affine":
            free[:12] = True
        if intensity:
            free[12:] = True
        return free

    if init_translation == "pcc" and initial is None and tuple(mov.shape) == shape:
        shift = np.array(_phase_cross_corr(tgt, mov), dtype=np.float64)
        if np.any(shift):
            # the correlation's sign convention is settled by the data: keep whichever direction
            # (or neither) has the smaller residual
            probe = tuple(max(2, v) for v in levels[0][0])
            best = None
            for sign in (0.0, 1.0, -1.0):
                trial = m.copy()
                trial[:, 3] += sign * shift
                _, _, sse, n = normal_equations(mov, tgt, trial, gain, offset, probe, c, s)
                if n > 0.25 * tgt.numel() / np.prod(probe) and (best is None or sse / n < best[0]):
                    best = (sse / n, trial)
            if best is not None:
                m = best[1]

    history, total_iters, converged = [], 0, False
    rms, n_used = float("nan"), 0
    for li, (strides, sigmas) in enumerate(levels):
        level = (_blur_axes(mov, sigmas), _blur_axes(tgt, sigmas), strides)
        h, b, sse, n = normal_equations(level[0], level[1], m, gain, offset, strides, c, s)
        if n < 64:
            raise _lib.LsrError("estimate_affine_zyx", -1, f"only {n} target samples fall inside the moving volume "
                                "at the starting transform: give a better `initial`")
        # the coarsest level settles the translation before it frees the linear part
        stages = (["translation", model] if (li == 0 and model == "affine" and len(levels) > 1) else [model])
        for kind in stages:
            free = free_mask(kind)
            lam, converged = 1e-3, False
            for it in range(int(max_iterations)):
                hf, bf = h[np.ix_(free, free)], b[free]
                step = None
                for _ in range(8):   # Levenberg-Marquardt: raise the damping until the residual goes down
                    try:
                        delta = np.linalg.solve(hf + lam * np.diag(np.diag(hf)) + 1e-12 * np.eye(hf.shape[0]), -bf)
                    except np.linalg.LinAlgError:
                        lam *= 10
                        continue
                    full = np.zeros(N_PARAMS)
                    full[free] = delta
                    q = _to_normalised(m, c, s) + full[:12].reshape(3, 4)
                    m_new = _from_normalised(q, c, s)
                    g_new, o_new = gain + full[12], offset + full[13]
                    h2, b2, sse2, n2 = normal_equations(level[0], level[1], m_new, g_new, o_new, strides, c, s)
                    if n2 >= 0.5 * n and sse2 / max(n2, 1) <= sse / n * (1 + 1e-12):
                        step = (m_new, g_new, o_new, h2, b2, sse2, n2)
                        lam = max(lam / 3, 1e-9)
                        break
                    lam *= 10
                total_iters += 1
                if step is None:
                    converged = True    # no downhill step left at this level
                    break
                moved = _corner_motion(step[0], m, shape)
                m, gain, offset, h, b, sse, n = step
                history.append((strides, it, float(np.sqrt(sse / n)), moved))
                if moved < tol * max(strides):
                    converged = True
                    break
        rms, n_used = float(np.sqrt(sse / n)), n
        logger.info("estimate_affine: strides %s sigmas %s -> rms %.4g on %d samples", strides, sigmas, rms, n)
    out = np.eye(4)
    out[:3] = m
    return RegistrationEstimate(out, float(gain), float(offset), rms, n_used, total_iters, converged, history)
