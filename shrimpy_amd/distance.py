"""The exact Euclidean distance transform and what sits on it: label expansion.

``csrc/edt.hip`` runs on the device (the nearest site of each row from wave ballots, then the lower envelope of the parabolas of
every y line and every z line, float64 costs), ``csrc/host_twins.hip`` on the CPU over the same row rule and line pass
(``csrc/edt.hpp``).  The rule:

* ``nearest[v]`` (``int32``): the linear index of a site that minimises ``(sz dz)^2 + (sy dy)^2 + (sx dx)^2``; among equals the
  smallest linear index wins (this package's rule, pinned by brute force: scipy's ``return_indices`` breaks ties otherwise).
* ``dist[v]`` (``float32``): the float64 distance to ``nearest[v]``, rounded.  ``scipy.ndimage.distance_transform_edt(mask,
  sampling=...)`` bit for bit for integer and dyadic spacings, within one float32 ulp otherwise (``tests/edt_ref.py``).
* With no site anywhere ``dist`` is ``+inf`` and ``nearest`` is ``-1`` at every voxel -- scipy measures from index -1 there.

* :func:`distance_transform` -- of a float32 volume: the sites are the background ``!(vol > threshold)`` (NaN is background, as in
  ``segment.label_volume``), so the result is scipy's ``distance_transform_edt(vol > threshold)``; ``invert`` swaps the roles.
* :func:`distance_transform_labels` -- of an int32 label volume: the sites are ``labels != 0``, with ``invert`` ``labels == 0``.
* :func:`expand_labels` -- ``skimage.segmentation.expand_labels(labels, distance, spacing=sampling)`` up to the tie rule.

Not built: a stand-alone ``distance`` command, a float distance channel in an output store, multi-GPU or slab transforms,
volumes above ``2^31 - 1`` voxels.
"""

from __future__ import annotations

import ctypes

from . import _lib
from .segment import _check_volume, _run, _scratch, _shape3

__all__ = ["tiling", "distance_transform", "distance_transform_labels", "expand_labels"]


def tiling() -> tuple[int, int, int, int]:
    """``(voxels per step of the x pass, lines per workgroup of the y and z passes, rows the x pass holds at once, lines a y or z
    pass holds at once)`` (``lsr_edt_tiling``)."""
    out = (ctypes.c_int * 4)()
    _lib.call("lsr_edt_tiling", out)
    return tuple(out)


def _sampling(sampling):
    import math

    try:
        s = tuple(float(v) for v in sampling)
    except TypeError as exc:
        raise TypeError(f"sampling must be three numbers (z, y, x), got {sampling!r}") from exc
    if len(s) != 3:
        raise ValueError(f"sampling must be three numbers (z, y, x), got {sampling!r}")
    if not all(math.isfinite(v) and v > 0.0 for v in s):
        raise ValueError(f"sampling must be positive and finite, got {s}")
    return s, (ctypes.c_double * 3)(*s)


def _transform(entry: str, vol, head: tuple, invert: bool, sampling, return_indices: bool, want_dist: bool = True):
    import torch

    z, y, x = _shape3(vol, "the volume")
    _, c_sampling = _sampling(sampling)
    scratch = _scratch("lsr_edt_scratch_bytes", z, y, x, vol.device)
    dist = torch.empty((z, y, x), dtype=torch.float32, device=vol.device) if want_dist else None
    nearest = torch.empty((z, y, x), dtype=torch.int32, device=vol.device) if return_indices else None
    _run(vol.device, entry, vol.data_ptr(), z, y, x, *head, int(bool(invert)), c_sampling,
         None if dist is None else dist.data_ptr(), None if nearest is None else nearest.data_ptr(), scratch.data_ptr())
    return (dist, nearest) if return_indices else dist


def distance_transform(vol, threshold: float, sampling=(1, 1, 1), invert: bool = False, return_indices: bool = False):
    """The distance of every voxel of ``vol`` ((Z, Y, X) float32) to the nearest background voxel ``!(vol > threshold)``, in units
    of ``sampling = (sz, sy, sx)``: a new float32 tensor on ``vol``'s device, 0 on the background.  With ``invert`` the distance
    to the nearest foreground voxel.  With ``return_indices`` also the int32 ``nearest`` (linear indices, ``-1`` without a site)."""
    import torch

    vol = _check_volume(vol, "vol", torch.float32)
    return _transform("lsr_edt_f32", vol, (ctypes.c_float(float(threshold)),), invert, sampling, return_indices)


def distance_transform_labels(labels, sampling=(1, 1, 1), invert: bool = False, return_indices: bool = False):
    """The distance of every voxel to the nearest labelled voxel (``labels != 0``; (Z, Y, X) int32), 0 on the objects; with
    ``invert`` to the nearest background voxel, 0 on the background: the depth inside each object."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    return _transform("lsr_edt_labels_i32", labels, (), invert, sampling, return_indices)


def expand_labels(labels, distance: float, sampling=(1, 1, 1)):
    """Grow every label of ``labels`` ((Z, Y, X) int32) into the background by at most ``distance`` (in units of ``sampling``)
    without overlap: a background voxel takes the label of its nearest labelled voxel where that is within ``distance`` (ties:
    the labelled voxel of the smallest linear index).  A new int32 tensor; ``distance = 0`` returns a copy."""
    import math

    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    z, y, x = _shape3(labels, "labels")
    distance = float(distance)
    if math.isnan(distance) or distance < 0.0:
        raise ValueError(f"distance must not be negative, got {distance}")
    _, c_sampling = _sampling(sampling)
    _, nearest = _transform("lsr_edt_labels_i32", labels, (), False, sampling, True, want_dist=False)
    out = torch.empty_like(labels)
    _run(labels.device, "lsr_label_expand_i32", labels.data_ptr(), nearest.data_ptr(), z, y, x, c_sampling, ctypes.c_double(distance),
         out.data_ptr())
    return out
