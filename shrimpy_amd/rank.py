"""Rank filters under a box window: rank, median, percentile, and the removal of outliers on the median.

``csrc/rank.hip`` runs on the device (one launch: a workgroup stages the codes of its tile and a halo in LDS and every voxel
bisects the 32 bits of the code of its window's ``rank``-th element), ``csrc/host_twins.hip`` on the CPU over the same fold, the
same codes, the same bisection and the same fused op (``csrc/rank.hpp``).  The rule, for half-widths ``(rz, ry, rx)``, each at
most :func:`max_half_width`, and the window ``2r + 1`` per axis with ``n`` elements:

* the border is ``scipy.ndimage``'s ``reflect`` (``d c b a | a b c d``); a half-width may exceed the axis, and reflected voxels
  count as often as they fall in the window;
* ``m(p)`` is the ``rank``-th smallest value (from 0) of the window around ``p``.  ``-0.0`` sorts below ``+0.0``, ``+-inf`` are
  ordinary values, a NaN is the greatest and comes back as the canonical quiet NaN (scipy is not pinned there); the result is
  the bit pattern of the chosen element;
* the outlier removal keeps a voxel ``v`` unless it stands out from the median ``m`` by more than a threshold ``t``:
  ``v - m > t`` (bright), ``m - v > t`` (dark) or either (both), one float32 subtraction each, fused into the kernel's store.
  ImageJ's "Remove Outliers".

By value ``scipy.ndimage.rank_filter`` / ``median_filter`` / ``percentile_filter`` with ``size = 2r + 1`` and ``mode="reflect"``
on NaN-free volumes, the conventions for ranks and percentiles included (``tests/rank_ref.py``).

Not built: other border modes, non-box footprints, half-widths above the cap, uint16 kernels, multi-GPU or slab filtering.
"""

from __future__ import annotations

import ctypes
import math

from . import _lib
from . import morphology
from .segment import _check_volume, _run, _shape3

__all__ = ["tiling", "max_half_width", "rank_filter", "median_filter", "percentile_filter", "remove_outliers", "half_widths_of"]

OPS = {"value": 0, "remove_bright": 1, "remove_dark": 2, "remove_both": 3}
WHICH = {"bright": "remove_bright", "dark": "remove_dark", "both": "remove_both"}


def tiling() -> tuple[int, int, int, int]:
    """``(greatest half-width per axis, tile z, tile y, tile x)``: the outputs a workgroup takes (``lsr_rank_filter_tiling``)."""
    out = (ctypes.c_int * 4)()
    _lib.call("lsr_rank_filter_tiling", out)
    return tuple(out)


def max_half_width() -> int:
    """The greatest half-width the kernel takes on an axis."""
    return tiling()[0]


def _half_widths(half_widths) -> tuple[int, int, int]:
    return morphology._half_widths(half_widths, cap=max_half_width())


def window_size(half_widths) -> int:
    """The number of elements of the window."""
    rz, ry, rx = _half_widths(half_widths)
    return (2 * rz + 1) * (2 * ry + 1) * (2 * rx + 1)


def rank_of(rank, n: int) -> int:
    """scipy's convention for ``rank_filter``: a negative rank counts from the greatest element (``+ n``); outside
    ``0 .. n - 1`` after that is a ``ValueError``."""
    if isinstance(rank, bool) or int(rank) != rank:
        raise ValueError(f"rank must be an integer, got {rank!r}")
    rank = int(rank)
    if rank < 0:
        rank += n
    if not 0 <= rank < n:
        raise ValueError(f"rank out of range for a window of {n} elements")
    return rank


def rank_of_percentile(percentile, n: int) -> int:
    """scipy's convention for ``percentile_filter``: a negative percentile gets ``+ 100``; 100 is the greatest element,
    anything else ``int(float(n) * percentile / 100.0)``; outside ``0 .. 100`` after that is a ``ValueError``."""
    p = float(percentile)
    if p < 0.0:
        p += 100.0
    if not 0.0 <= p <= 100.0:               # (a NaN too)
        raise ValueError(f"percentile {percentile!r} out of range")
    return n - 1 if p == 100.0 else int(float(n) * p / 100.0)


def _filter(vol, half_widths, rank: int, op: str, threshold: float = 0.0, variant: int = 0):
    import torch

    vol = _check_volume(vol, "vol", torch.float32)
    z, y, x = _shape3(vol, "vol")
    rz, ry, rx = _half_widths(half_widths)
    out = torch.empty((z, y, x), dtype=torch.float32, device=vol.device)
    _run(vol.device, "lsr_rank_filter_f32", vol.data_ptr(), out.data_ptr(), z, y, x, rz, ry, rx, rank, OPS[op],
         ctypes.c_float(threshold), variant)
    return out


def rank_filter(vol, rank, half_widths):
    """The ``rank``-th smallest value (from 0; negative: from the greatest) of ``vol`` ((Z, Y, X) float32) in the box of
    ``half_widths = (rz, ry, rx)`` around each voxel: a new float32 tensor on ``vol``'s device."""
    return _filter(vol, half_widths, rank_of(rank, window_size(half_widths)), "value")


def median_filter(vol, half_widths):
    """The median of the box around each voxel: rank ``n // 2``."""
    return _filter(vol, half_widths, window_size(half_widths) // 2, "value")


def percentile_filter(vol, percentile, half_widths):
    """The ``percentile``-th percentile of the box around each voxel, by :func:`rank_of_percentile`."""
    return _filter(vol, half_widths, rank_of_percentile(percentile, window_size(half_widths)), "value")


def remove_outliers(vol, half_widths, threshold, which="bright"):
    """``vol`` with every voxel that stands out from the median of its box by more than ``threshold`` replaced by that median:
    ``which`` ``"bright"`` (``v - m > t``), ``"dark"`` (``m - v > t``) or ``"both"``.  Every other voxel keeps its bytes."""
    if which not in WHICH:
        raise ValueError(f"which must be one of {sorted(WHICH)}, got {which!r}")
    threshold = float(threshold)
    if math.isnan(threshold):
        raise ValueError("threshold is NaN")
    return _filter(vol, half_widths, window_size(half_widths) // 2, WHICH[which], threshold)


def half_widths_of(radius, sampling=(1, 1, 1)) -> tuple[int, int, int]:
    """Half-widths in voxels of a ``radius`` in the units of ``sampling``: ``floor(radius / s + 0.5)`` per axis
    (``morphology.half_widths_of``), against this module's cap."""
    return morphology.half_widths_of(radius, sampling, cap=max_half_width())
