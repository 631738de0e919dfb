"""Time-lapse stabilization: one translation per timepoint, estimated from the series and applied volume by volume.

biahub's ``estimate-stabilization`` / ``stabilize`` pair [RECALLED]; biahub is not vendored or installed -- PARITY
UNPINNED, the rule is this package's own and ``tests/focus_ref.py::drift_series`` restates it.

For one position, the channel ``stabilization_estimation_channel`` and timepoints ``0 .. T - 1`` with volumes ``V[t]``:

* ``focus-finding`` (``stabilization_type`` ``"z"`` or ``"xyz"``): ``f[t]`` = the focus index of ``V[t]``
  (:func:`shrimpy_amd.focus.focus_from_transverse_band`); a timepoint whose index is ``None`` takes the previous valid one,
  leading ones the first valid one, and a series without any is a ``ValueError``; ``dz[t] = f[t] - f[0]``.  For ``"xyz"``
  the y and x components come from the phase cross-correlation below (its z component is discarded).
* ``phase-cross-corr`` (``"xy"`` or ``"xyz"``): ``s = dynatrack._phase_cross_corr(ref, mov, maximum_shift)`` on the volumes
  centre-cropped in y and x to ``center_crop_xy`` (start ``d // 2``; z uncropped), in the reference's sign:
  ``mov = roll(ref, s)`` gives ``s``.  ``t_reference="first"``: ``s[t] = pcc(V[0], V[t])``; ``"previous"``: the running sum
  of ``pcc(V[t - 1], V[t])``.  ``"xy"`` zeroes the z component.

The matrix of timepoint ``t`` is the 4x4 identity with the shift in ``[0:3, 3]`` (ZYX): scipy's output -> input convention,
so ``out[i] = V[t][i + s]`` and the plane in focus at ``t`` lands on ``f[0]`` -- what ``apply_affine_transform_zyx`` takes.
An integer translation goes through its exact path: every output voxel is an input voxel or the fill value.
"""

from __future__ import annotations

import numpy as np

__all__ = ["estimate_stabilization", "apply_stabilization", "fill_missing"]


def fill_missing(indices):
    """``None`` entries take the previous valid value, leading ones the first valid one (module docstring)."""
    valid = [i for i in indices if i is not None]
    if not valid:
        raise ValueError("focus finding found no plane in focus at any timepoint (every peak is narrower than "
                         "threshold_FWHM): the z drift cannot be estimated")
    out, last = [], valid[0]
    for i in indices:
        if i is not None:
            last = i
        out.append(last)
    return out


def _center_crop_yx(volume, center_crop_xy):
    z, y, x = (int(v) for v in volume.shape)
    cy, cx = min(y, int(center_crop_xy[0])), min(x, int(center_crop_xy[1]))
    if (cy, cx) == (y, x):
        return volume
    y0, x0 = (y - cy) // 2, (x - cx) // 2
    return volume[:, y0:y0 + cy, x0:x0 + cx].contiguous()


def estimate_stabilization(volumes, settings, pixel_size: float) -> list:
    """One 4x4 float64 matrix per timepoint from an iterable of ``(Z, Y, X)`` volumes (tensors on any device, or arrays),
    one per timepoint of the estimation channel.  The iterable is consumed as a stream: beside the volume at hand only the
    (cropped) correlation reference is kept.  ``settings``: :class:`~shrimpy_amd.settings.EstimateStabilizationSettings`
    (or its dict); ``pixel_size``: the y, x pixel size in the units of ``lambda_ill``."""
    import torch

    from .dynatrack import _phase_cross_corr
    from .focus import focus_from_transverse_band
    from .settings import EstimateStabilizationSettings

    if not isinstance(settings, EstimateStabilizationSettings):
        settings = EstimateStabilizationSettings(**settings)
    method, kind = settings.stabilization_method, settings.stabilization_type
    ff, pc = settings.focus_finding_settings, settings.phase_cross_corr_settings
    want_focus = method == "focus-finding"
    want_pcc = method == "phase-cross-corr" or kind == "xyz"

    focus, steps = [], []
    reference = None
    for t, vol in enumerate(volumes):
        if not isinstance(vol, torch.Tensor):
            vol = torch.from_numpy(np.ascontiguousarray(vol))
        vol = vol.to(torch.float32)
        if vol.dim() != 3:
            raise ValueError(f"timepoint {t}: expected a (Z, Y, X) volume, got shape {tuple(vol.shape)}")
        if want_focus:
            focus.append(focus_from_transverse_band(vol, ff.NA_det, ff.lambda_ill, pixel_size, ff.midband_fractions,
                                                    threshold_FWHM=ff.threshold_FWHM, center_crop_xy=ff.center_crop_xy))
        if want_pcc:
            moving = _center_crop_yx(vol, pc.center_crop_xy).contiguous()
            if reference is None:
                steps.append((0, 0, 0))
                reference = moving
            else:
                steps.append(tuple(int(v) for v in _phase_cross_corr(reference, moving, pc.maximum_shift)))
                if pc.t_reference == "previous":
                    reference = moving
            del moving
        del vol
    n = max(len(focus), len(steps))
    if n == 0:
        raise ValueError("the series holds no timepoint")
    shifts = np.zeros((n, 3), dtype=np.float64)
    if want_focus:
        f = fill_missing(focus)
        shifts[:, 0] = [i - f[0] for i in f]
    if want_pcc:
        s = np.asarray(steps, dtype=np.float64)
        if pc.t_reference == "previous":
            s = np.cumsum(s, axis=0)
        if method == "phase-cross-corr":
            shifts[:] = s
            if kind == "xy":
                shifts[:, 0] = 0.0
        else:
            shifts[:, 1:] = s[:, 1:]
    out = []
    for t in range(n):
        m = np.eye(4, dtype=np.float64)
        m[:3, 3] = shifts[t]
        out.append(m)
    return out


def apply_stabilization(volume, matrix):
    """``volume`` ((Z, Y, X) tensor) moved by one timepoint's matrix onto its own grid, zero outside."""
    from .register import apply_affine_transform_zyx

    return apply_affine_transform_zyx(volume, np.asarray(matrix, dtype=np.float64), tuple(int(v) for v in volume.shape),
                                      mode="constant", cval=0.0)
