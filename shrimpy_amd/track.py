"""Tracking labelled objects over time: the overlap table of two label volumes, a linking rule, tracks and lineages.

``csrc/overlap.hip`` fills the table on the device, ``csrc/host_twins.hip`` on the CPU over the same rule
(``csrc/overlap.hpp``).  PINNED (to numpy): the table is integer arithmetic, so device, twin and ``np.unique`` of the packed
pairs (``tests/track_ref.py``) agree exactly, as sets of ``(a, b, count)``.  PARITY UNPINNED: the linking and track rules
below are the specification -- biahub's ``track`` step runs ultrack, which is not a dependency and not a GPU path.

The rules.

* Table: for every voxel ``v`` with ``u = v + shift`` inside the volume, ``a[v] > 0`` and ``b[u] > 0``, the pair
  ``(a[v], b[u])`` gains 1.  Labels ``<= 0`` are background.
* Link (host, numpy, deterministic): a pair is a *candidate* when ``count >= min_overlap_voxels`` and ``count >= min_iou *
  (va + vb - count)`` in float64.  Every object ``b`` of the later frame takes as ``parent[b]`` the candidate ``a`` of
  greatest ``count``, ties to the smaller ``a``; 0 without a candidate.
* Tracks: ids ``1, 2, ...`` in order of ``(t, label)`` at birth.  The children of ``a`` are the ``b`` with ``parent[b] == a``.
  With ``divisions`` (the convention of the Cell Tracking Challenge) an ``a`` with exactly one child hands its track on; an
  ``a`` with two or more ends, and every child starts a track whose ``parent_track`` is ``a``'s.  Without, the child of
  greatest ``count`` (ties: the smaller label) continues the track and the others start tracks with ``parent_track = 0``.
  An object without a parent starts a track with ``parent_track = 0``; a track whose object has no child ends.  Tracks are
  contiguous in time.

* :func:`label_overlaps` -- ``{"a", "b", "count"}`` sorted by ``(a, b)``.
* :func:`label_volumes` -- voxels per label, exact, counted where the labels are.
* :func:`link_frames` -- ``(parent, overlap, iou)`` per label of the later frame.
* :class:`Tracker`, :func:`track_frames` -- the track of every object, the track table and the per-object links.
* :func:`relabel_by_track` -- a label volume with every voxel's track id.

Not built: gap closing (re-finding an object after a frame without it), motion models, global (ILP / Hungarian) assignment,
reading a stabilization file for the shifts, multi-GPU tracking of one position, volumes above ``2^31 - 1`` voxels.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .segment import _check_volume, _fill_pair_table, _run, _same_volume, _shape3

__all__ = ["OVERLAP_DTYPE", "MAX_CAPACITY", "overlap_geometry", "label_overlaps", "label_volumes", "link_frames", "Tracker",
           "track_frames", "relabel_by_track"]

# one record of the overlap table (csrc/overlap.hpp ``Overlap``)
OVERLAP_DTYPE = np.dtype([("pair", "<u8"), ("count", "<u8")])
assert OVERLAP_DTYPE.itemsize == 16
# the ceiling of label_overlaps' retries: 2^30 slots, 16 GiB
MAX_CAPACITY = 1 << 30


def overlap_geometry() -> tuple[int, int]:
    """``(LDS table slots per workgroup, default cap of the grid)`` of the kernel (``lsr_label_overlap_geometry``)."""
    out = (ctypes.c_int * 2)()
    _lib.call("lsr_label_overlap_geometry", out)
    return int(out[0]), int(out[1])


def _frames(a, b):
    import torch

    a = _check_volume(a, "a", torch.int32)
    b = _check_volume(b, "b", torch.int32)
    _same_volume(a, b, "a", "b")
    return a, b, _shape3(a, "a")


def _shift(shift):
    s = [int(v) for v in shift]
    if len(s) != 3 or any(int(v) != v for v in shift):
        raise ValueError(f"shift must be three integers (z, y, x), got {shift!r}")
    if any(not -2 ** 31 <= v <= 2 ** 31 - 1 for v in s):
        raise ValueError(f"shift {shift!r} is out of the int32 range")
    return (ctypes.c_int32 * 3)(*s)


def label_overlaps(a, b, shift=(0, 0, 0), _capacity: int | None = None, _max_blocks: int = 0) -> dict:
    """The contingency table of two label volumes ((Z, Y, X) int32, contiguous, one shape, one device -- CPU or HIP):
    ``{"a", "b", "count"}``, int64 numpy arrays sorted by ``(a, b)``; ``count`` is the number of voxels ``v`` that are ``a``
    in the first volume while ``v + shift`` is ``b`` in the second.

    The device fills an open-addressing table; its first capacity is the power of two at or above ``4 * bound + 1024`` with
    ``bound = min(max(a) + max(b), voxels)``, and while a contribution finds no slot the capacity doubles and the pass runs
    again, up to ``MAX_CAPACITY`` slots (then :class:`RuntimeError`).  ``_capacity`` sets the first capacity (a power of two;
    tests force the retry with it), ``_max_blocks`` caps the grid (0: the kernel's default; the result does not depend on it)."""
    a, b, (z, y, x) = _frames(a, b)
    c_shift = _shift(shift)
    if _capacity is not None:
        capacity = int(_capacity)
    else:
        bound = min(max(int(a.max()), 0) + max(int(b.max()), 0), z * y * x)
        capacity = 1 << int(4 * bound + 1024 - 1).bit_length()
    if capacity <= 0 or capacity & (capacity - 1) or capacity > MAX_CAPACITY:
        raise ValueError(f"_capacity must be a power of two up to 2^30, got {capacity}")

    def launch(capacity, table_ptr, counts_ptr):
        _run(a.device, "lsr_label_overlap_i32", a.data_ptr(), b.data_ptr(), z, y, x, c_shift, capacity, table_ptr, counts_ptr,
             int(_max_blocks))

    rows = _fill_pair_table(a.device, OVERLAP_DTYPE, capacity, MAX_CAPACITY, "label_overlaps: {} voxels", launch)
    return {"a": (rows["pair"] >> np.uint64(32)).astype(np.int64), "b": (rows["pair"] & np.uint64(0xFFFFFFFF)).astype(np.int64),
            "count": rows["count"].astype(np.int64)}


def label_volumes(labels) -> np.ndarray:
    """Voxels per label of a (Z, Y, X) int32 tensor: an int64 numpy array indexed by label, ``max(label) + 1`` entries (entry 0
    counts the background, labels ``<= 0``).  An exact integer count, made where the labels are (``torch.bincount``)."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    if labels.numel() == 0:
        return np.zeros((1,), dtype=np.int64)
    return torch.bincount(labels.reshape(-1).clamp_min(0)).cpu().numpy().astype(np.int64)


def link_frames(overlaps: dict, volumes_a, volumes_b, min_overlap_voxels: int = 1, min_iou: float = 0.0):
    """Link the objects of the later frame to those of the earlier one: ``(parent, overlap, iou)``, arrays indexed by the
    later frame's label (``len(volumes_b)`` entries, entry 0 unused and 0) -- ``parent`` (int64: the earlier frame's label,
    0 without one), ``overlap`` (int64: the voxels shared with it) and ``iou`` (float64: ``overlap / (va + vb - overlap)``).

    ``overlaps`` is :func:`label_overlaps`' table, ``volumes_a`` and ``volumes_b`` are indexed by label
    (:func:`label_volumes`).  Host code, numpy, deterministic."""
    va = np.asarray(volumes_a, dtype=np.int64)
    vb = np.asarray(volumes_b, dtype=np.int64)
    a = np.asarray(overlaps["a"], dtype=np.int64)
    b = np.asarray(overlaps["b"], dtype=np.int64)
    count = np.asarray(overlaps["count"], dtype=np.int64)
    min_overlap_voxels, min_iou = int(min_overlap_voxels), float(min_iou)
    if min_overlap_voxels < 1:
        raise ValueError(f"min_overlap_voxels must be at least 1, got {min_overlap_voxels}")
    if not 0.0 <= min_iou <= 1.0:
        raise ValueError(f"min_iou must be in [0, 1], got {min_iou}")
    n = max(len(vb), 1)
    parent = np.zeros((n,), dtype=np.int64)
    overlap = np.zeros((n,), dtype=np.int64)
    iou = np.zeros((n,), dtype=np.float64)
    if len(a) == 0:
        return parent, overlap, iou
    if a.max() >= len(va) or b.max() >= len(vb):
        raise ValueError("the overlap table names a label that the volumes do not cover")
    union = (va[a] + vb[b] - count).astype(np.float64)
    keep = (count >= min_overlap_voxels) & (count.astype(np.float64) >= min_iou * union)
    a, b, count, union = a[keep], b[keep], count[keep], union[keep]
    order = np.lexsort((a, -count, b))                      # by b, then the greatest count, then the smaller a
    a, b, count, union = a[order], b[order], count[order], union[order]
    first = np.ones((len(b),), dtype=bool)
    first[1:] = b[1:] != b[:-1]
    parent[b[first]] = a[first]
    overlap[b[first]] = count[first]
    iou[b[first]] = count[first].astype(np.float64) / union[first]
    return parent, overlap, iou


class Tracker:
    """The tracks of a time-lapse, one frame at a time.  :meth:`step` takes the next frame's labels (a (Z, Y, X) int32 tensor,
    CPU or HIP) and returns the track id of each of its labels; the frame stays where it is until the next one has been
    linked to it, so every volume is uploaded once.  ``settings``: anything with ``min_overlap_voxels``, ``min_iou`` and
    ``divisions`` (:class:`~shrimpy_amd.settings.TrackSettings`)."""

    def __init__(self, settings):
        self.min_overlap_voxels = int(settings.min_overlap_voxels)
        self.min_iou = float(settings.min_iou)
        self.divisions = bool(settings.divisions)
        self.t = 0
        self._prev = None                       # the previous frame's labels, its volumes and its labels' tracks
        self._volumes = None
        self._track_of = None
        self._begin, self._end, self._parent_track = [], [], []
        self._objects = []                      # (t, label, track, parent_label, overlap, iou)

    def _new_track(self, parent_track: int) -> int:
        self._begin.append(self.t)
        self._end.append(self.t)
        self._parent_track.append(int(parent_track))
        return len(self._begin)

    def step(self, labels, shift=(0, 0, 0)) -> np.ndarray:
        """Link ``labels`` to the previous frame (``shift``: the integer ``(z, y, x)`` offset of this frame's voxels against the
        previous frame's, ignored at the first) and return ``track_of`` (int32, indexed by label, entry 0 is 0; 0 for a label
        that no voxel carries)."""
        volumes = label_volumes(labels)
        n = len(volumes)
        track_of = np.zeros((n,), dtype=np.int32)
        present = volumes > 0
        present[0] = False
        parent = np.zeros((n,), dtype=np.int64)
        overlap = np.zeros((n,), dtype=np.int64)
        iou = np.zeros((n,), dtype=np.float64)
        if self._prev is not None:
            if tuple(labels.shape) != tuple(self._prev.shape):
                raise ValueError(f"frame {self.t} has shape {tuple(labels.shape)}, the frame before {tuple(self._prev.shape)}")
            table = label_overlaps(self._prev, labels, shift)
            parent, overlap, iou = link_frames(table, self._volumes, volumes, self.min_overlap_voxels, self.min_iou)
        # who continues its parent's track?
        heir = {}                               # earlier label -> the later label that takes its track on
        children = {}
        for b in np.flatnonzero(present & (parent > 0)).tolist():
            children.setdefault(int(parent[b]), []).append(b)
        for a, kids in children.items():
            if self.divisions:
                if len(kids) == 1:
                    heir[a] = kids[0]
            else:
                heir[a] = min(kids, key=lambda k: (-int(overlap[k]), k))
        for b in np.flatnonzero(present).tolist():
            a = int(parent[b])
            if a > 0 and heir.get(a) == b:
                track = int(self._track_of[a])
                self._end[track - 1] = self.t
            else:
                track = self._new_track(int(self._track_of[a]) if a > 0 and self.divisions else 0)
            track_of[b] = track
            self._objects.append((self.t, b, track, a, int(overlap[b]), float(iou[b])))
        self._prev, self._volumes, self._track_of = labels, volumes, track_of
        self.t += 1
        return track_of

    def tracks(self) -> dict:
        """The track table so far: ``track_id``, ``t_begin``, ``t_end``, ``parent_track_id`` (int64 arrays, one row per track),
        and under ``"objects"`` one row per object: ``t``, ``label``, ``track_id``, ``parent_label``, ``overlap_voxels`` (int64)
        and ``iou`` (float64)."""
        cols = list(zip(*self._objects)) if self._objects else [()] * 6
        objects = {name: np.asarray(cols[k], dtype=np.float64 if name == "iou" else np.int64)
                   for k, name in enumerate(("t", "label", "track_id", "parent_label", "overlap_voxels", "iou"))}
        return {"track_id": np.arange(1, len(self._begin) + 1, dtype=np.int64), "t_begin": np.asarray(self._begin, dtype=np.int64),
                "t_end": np.asarray(self._end, dtype=np.int64), "parent_track_id": np.asarray(self._parent_track, dtype=np.int64),
                "objects": objects}


def track_frames(frames, settings, shifts=None):
    """Track the objects of ``frames`` (an iterable of (Z, Y, X) int32 label tensors, one per timepoint):
    ``(track_of, tracks)`` -- ``track_of[t]`` maps frame ``t``'s labels to track ids (:meth:`Tracker.step`), ``tracks`` is
    :meth:`Tracker.tracks`.  ``shifts[t]`` is the integer ``(z, y, x)`` shift between frame ``t`` and ``t + 1`` (the voxel ``v``
    of frame ``t`` is compared with ``v + shift`` of frame ``t + 1``); zero by default."""
    tracker = Tracker(settings)
    track_of = []
    for t, labels in enumerate(frames):
        shift = (0, 0, 0) if shifts is None or t == 0 else shifts[t - 1]
        track_of.append(tracker.step(labels, shift))
    return track_of, tracker.tracks()


def relabel_by_track(labels, track_of_label):
    """A new int32 tensor with ``track_of_label[labels[v]]`` at every voxel (0 on the background and for a label outside the
    map), through ``lsr_label_remap_i32``; ``labels`` is not changed."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    lut = np.ascontiguousarray(track_of_label, dtype=np.int32)
    if lut.ndim != 1 or len(lut) < 1 or lut[0] != 0:
        raise ValueError("track_of_label must be a 1-D map with entry 0 (the background's) equal to 0")
    out = labels.clone()
    if out.numel() == 0:
        return out
    d_lut = torch.from_numpy(lut).to(out.device)
    _run(out.device, "lsr_label_remap_i32", out.data_ptr(), out.numel(), d_lut.data_ptr(), len(lut))
    _lib.mark_written(out)
    return out
