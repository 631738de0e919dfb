"""Flat grey-scale morphology under a box window, and what sits on it: top-hat background subtraction and hole filling.

``csrc/morphology.hip`` runs on the device (one van Herk / Gil-Werman pass per axis, about three comparisons per voxel at any
window width), ``csrc/host_twins.hip`` on the CPU over the same plan and the same walk (``csrc/morphology.hpp``).  The rule,
for half-widths ``(rz, ry, rx)`` and the window ``2r + 1`` per axis:

* ``erode(v)(p)`` is the least and ``dilate(v)(p)`` the greatest ``v(q)`` over the in-volume ``q`` of the box around ``p``.
  Voxels outside the volume do not compete -- ``scipy.ndimage``'s default ``reflect`` border for centred odd boxes -- and a
  half-width may exceed the axis.  ``-0.0`` sorts below ``+0.0``, ``+-inf`` are ordinary values, and the result is the bit
  pattern of the chosen element.  A window that holds a NaN gives the canonical quiet NaN (scipy is not pinned there).
* ``open = dilate(erode)``, ``close = erode(dilate)``, ``white_tophat = v - open(v)``, ``black_tophat = close(v) - v``.
* An axis with half-width 0 gets no pass.

Element for element ``scipy.ndimage.grey_erosion`` / ``grey_dilation`` / ``grey_opening`` / ``grey_closing`` /
``white_tophat`` / ``black_tophat`` with ``size = 2r + 1`` on NaN-free volumes (``tests/morphology_ref.py``).

* :func:`subtract_background` -- the white top-hat under a window given in physical units: what is left of a volume once
  everything wider than the window is taken away (out-of-focus haze, the light sheet's profile).
* :func:`fill_holes` -- ``scipy.ndimage.binary_fill_holes`` with its default structure, on the labelling kernels.

Not built: ball or other non-box structuring elements, rolling-ball, uint16 kernels, multi-GPU or slab morphology, one launch
for the two z passes of an opening or closing.
"""

from __future__ import annotations

import ctypes
import math

from . import _lib
from .segment import _check_volume, _run, _scratch, _shape3

__all__ = ["tiling", "dispatch", "max_half_width", "grey_erosion", "grey_dilation", "grey_opening", "grey_closing", "white_tophat",
           "black_tophat", "half_widths_of", "subtract_background", "fill_holes"]

OPS = {"grey_erosion": 0, "grey_dilation": 1, "grey_opening": 2, "grey_closing": 3, "white_tophat": 4, "black_tophat": 5}


def tiling() -> tuple[int, int, int, int]:
    """``(greatest half-width per axis, columns per workgroup of the y and z passes, outputs per staged row segment of the x
    pass, threads per workgroup of the x pass)`` (``lsr_grey_morph_tiling``)."""
    out = (ctypes.c_int * 4)()
    _lib.call("lsr_grey_morph_tiling", out)
    return tuple(out)


def dispatch() -> tuple[int, int, int, int, int, int]:
    """The edges at which the launches choose their code (``lsr_grey_morph_dispatch``): ``(greatest half-width of the narrow
    instantiation of the y and z walk, greatest half-width whose strip fits static LDS, workgroups of the x pass at most, rows
    read ahead by the narrow, the static-LDS and the dynamic-LDS instantiation)``.  For tests that aim at those edges."""
    out = (ctypes.c_int * 6)()
    _lib.call("lsr_grey_morph_dispatch", out)
    return tuple(out)


def max_half_width() -> int:
    """The greatest half-width the kernels take on an axis."""
    return tiling()[0]


def _half_widths(half_widths, cap=None) -> tuple[int, int, int]:
    try:
        r = tuple(half_widths)
    except TypeError as exc:
        raise TypeError(f"half_widths must be three integers (z, y, x), got {half_widths!r}") from exc
    if len(r) != 3 or any(isinstance(v, bool) or int(v) != v for v in r):
        raise ValueError(f"half_widths must be three integers (z, y, x), got {half_widths!r}")
    r = tuple(int(v) for v in r)
    if min(r) < 0:
        raise ValueError(f"half_widths must not be negative, got {r}")
    cap = max_half_width() if cap is None else cap
    if max(r) > cap:
        raise ValueError(f"half_widths {r}: at most {cap} per axis")
    return r


def _morph(name: str, vol, half_widths):
    import torch

    vol = _check_volume(vol, "vol", torch.float32)
    z, y, x = _shape3(vol, "vol")
    rz, ry, rx = _half_widths(half_widths)
    scratch = _scratch("lsr_grey_morph_scratch_bytes", z, y, x, vol.device)
    out = torch.empty((z, y, x), dtype=torch.float32, device=vol.device)
    _run(vol.device, "lsr_grey_morph_f32", vol.data_ptr(), out.data_ptr(), z, y, x, rz, ry, rx, OPS[name], scratch.data_ptr())
    return out


def grey_erosion(vol, half_widths):
    """The least value of ``vol`` ((Z, Y, X) float32) in the box of ``half_widths = (rz, ry, rx)`` around each voxel: a new
    float32 tensor on ``vol``'s device."""
    return _morph("grey_erosion", vol, half_widths)


def grey_dilation(vol, half_widths):
    """The greatest value of ``vol`` in the box around each voxel."""
    return _morph("grey_dilation", vol, half_widths)


def grey_opening(vol, half_widths):
    """The dilation of the erosion: what of ``vol`` a box of this size fits under."""
    return _morph("grey_opening", vol, half_widths)


def grey_closing(vol, half_widths):
    """The erosion of the dilation."""
    return _morph("grey_closing", vol, half_widths)


def white_tophat(vol, half_widths):
    """``vol - grey_opening(vol)``: the bright structures narrower than the window, the subtraction fused into the last pass."""
    return _morph("white_tophat", vol, half_widths)


def black_tophat(vol, half_widths):
    """``grey_closing(vol) - vol``: the dark structures narrower than the window."""
    return _morph("black_tophat", vol, half_widths)


def half_widths_of(radius, sampling=(1, 1, 1), cap=None) -> tuple[int, int, int]:
    """Half-widths in voxels of a ``radius`` in the units of ``sampling = (sz, sy, sx)``: ``floor(radius / s + 0.5)`` per axis.
    ``radius`` is one number for every axis or a ``(z, y, x)`` triple; a component 0 means no window on that axis.  A
    half-width above the kernels' cap (``cap``: another family's, ``shrimpy_amd/rank.py``) is a ``ValueError`` that names the
    cap."""
    try:
        s = tuple(float(v) for v in sampling)
    except TypeError as exc:
        raise TypeError(f"sampling must be three numbers (z, y, x), got {sampling!r}") from exc
    if len(s) != 3 or not all(math.isfinite(v) and v > 0.0 for v in s):
        raise ValueError(f"sampling must be three positive finite numbers (z, y, x), got {sampling!r}")
    try:
        r = tuple(float(v) for v in radius)
    except TypeError:
        r = (float(radius),) * 3
    if len(r) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in r):
        raise ValueError(f"radius must be a non-negative finite number or three of them (z, y, x), got {radius!r}")
    quotients = tuple(a / b for a, b in zip(r, s))
    cap = max_half_width() if cap is None else cap
    if any(q + 0.5 >= cap + 1 for q in quotients):
        raise ValueError(f"radius {radius!r} at sampling {s} is a half-width of {tuple(round(q, 3) for q in quotients)} voxels: "
                         f"at most {cap} per axis")
    return tuple(int(math.floor(q + 0.5)) for q in quotients)


def subtract_background(vol, radius, sampling=(1, 1, 1)):
    """``white_tophat(vol, half_widths_of(radius, sampling))``: ``vol`` without everything that is wider than ``2 * radius``."""
    return white_tophat(vol, half_widths_of(radius, sampling))


def fill_holes(mask):
    """``scipy.ndimage.binary_fill_holes(mask)`` with its default structure, for a (Z, Y, X) bool tensor: a new bool tensor on
    ``mask``'s device.  The complement is labelled with connectivity 6; a component whose bounding box touches a face of the
    volume is connected to the outside and stays background (a component that touches a face has a voxel on it, so its
    bounding box does), every other one is a hole and joins the foreground."""
    import numpy as np
    import torch

    from .segment import label_volume, region_table

    mask = _check_volume(mask, "mask", torch.bool)
    z, y, x = _shape3(mask, "mask")
    labels, n = label_volume((~mask).to(torch.float32), 0.5, 6)
    if n == 0:
        return mask.clone()
    bbox = region_table(labels, n)["bbox"]
    outside = (bbox[:, :3] == 0).any(axis=1) | (bbox[:, 3:] == np.array([z, y, x])).any(axis=1)
    hole = np.zeros((n + 1,), dtype=np.bool_)
    hole[1:] = ~outside
    if not hole.any():
        return mask.clone()
    return mask | torch.from_numpy(hole).to(mask.device)[labels.long()]
