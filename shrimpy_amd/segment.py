"""Segmentation: connected-component labels of a thresholded volume, one table row per object, and a filter.

``csrc/label.hip`` labels on the device (a block-based union-find rooted at the smallest linear index, so that the
numbering is a prefix count), ``csrc/host_twins.hip`` on the CPU; both equal ``scipy.ndimage.label`` element for element
(``tests/label_ref.py``): foreground is ``vol > threshold`` (NaN and the threshold itself are background), labels are
``1 .. N`` in raster order of each component's first voxel.

* :func:`label_volume` -- ``(labels, n)``: an ``int32`` torch tensor on the volume's device and the object count.
* :func:`region_table` -- per label: volume, bounding box (half-open), centroid, and with an intensity volume its sum,
  mean, minimum, maximum and the intensity-weighted centroid.  The integer columns and the intensity range are exact; the
  float64 sums are atomic adds on the device (within ``n_k * 2^-53 * sum|terms|`` of the exact sum, not bit-reproducible).
* :func:`filter_objects` -- drop small objects or keep the largest; the kept labels stay consecutive, in their old order.
* :func:`moment_table` -- per label the exact integer sums of the coordinates and of their products (``csrc/moments.hip``: one
  launch, runs of equal labels reduced in closed form, a table in LDS per workgroup; the twin in ``csrc/host_twins.hip``).
* :func:`shape_table` -- axis lengths and the major axis from those moments, exposed faces, staircase surface area, contact
  area, neighbours and ``touches_border``; :func:`contact_table` -- the pairs of labels that share a face.  PARITY UNPINNED
  (skimage is not a dependency): the rules in :func:`shape_table`'s docstring are the specification,
  ``tests/moments_ref.py`` restates them in plain numpy.
* :func:`segment_zyx` -- on request take the median under a small box (``shrimpy_amd/rank.py``), subtract the background (the white top-hat of ``shrimpy_amd/morphology.py``), threshold (a
  number or multi-Otsu, after an optional Gaussian blur), on request fill the holes of the mask, label, on request split the
  touching objects by a watershed of their depth map (``shrimpy_amd/watershed.py``), measure, filter, and on request grow the
  labels by a distance and measure each object's inscribed radius (``shrimpy_amd/distance.py``).

* :func:`intensity_table` -- per label what another volume (float32 or uint16) holds: count, sum, sum of squares, mean,
  standard deviation, extremes and the intensity-weighted first moments (``csrc/intensity.hip``: the moment kernel's form with
  the run sums reduced inside the wave and float64 LDS adds; PARITY UNPINNED, ``tests/intensity_ref.py``); :func:`shell_labels`
  -- a ring of local background around every object.  The ``measure`` command applies both to any label store and any channel.

Not built: seeded watersheds, multi-GPU or slab labelling, label pyramids, volumes above ``2^31 - 1`` voxels, ball-shaped or
rolling-ball background windows (the window is a box), per-object percentiles, :func:`region_table` on the intensity kernel
(sums over two channels -- Pearson / Manders colocalization per object -- are ``shrimpy_amd/colocalize.py``).  Labels are
numbered from 1 at every timepoint; linking them over time is ``shrimpy_amd/track.py`` (the ``track`` command), where gap
closing, motion models and a global assignment are not built.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

__all__ = ["REGION_DTYPE", "MOMENTS_DTYPE", "tile_shape", "launch_geometry", "label_volume", "region_table", "filter_objects", "moments_geometry",
           "moment_table", "shape_table", "contact_table", "segment_zyx", "INTENSITY_DTYPE_F32", "INTENSITY_DTYPE_U16",
           "intensity_geometry", "intensity_table", "shell_labels"]

# one record of the object table (csrc/label.hpp ``Region``)
REGION_DTYPE = np.dtype([("volume", "<i8"), ("sum_zyx", "<i8", (3,)), ("sum_v", "<f8"), ("sum_vzyx", "<f8", (3,)),
                         ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("v_min", "<f4"), ("v_max", "<f4")])
assert REGION_DTYPE.itemsize == 96
# one record of the moment table (csrc/moments.hpp ``Moments``)
MOMENT_FIELDS = ("volume", "s_z", "s_y", "s_x", "m_zz", "m_yy", "m_xx", "m_zy", "m_zx", "m_yx")
MOMENTS_DTYPE = np.dtype([(f, "<i8") for f in MOMENT_FIELDS])
assert MOMENTS_DTYPE.itemsize == 80
# one record of the intensity table for float32 and for uint16 values (csrc/intensity.hpp ``RecordF32``, ``RecordU16``)
INTENSITY_SUMS = ("sum_v", "sum_vv", "sum_vz", "sum_vy", "sum_vx")
INTENSITY_DTYPE_F32 = np.dtype([("count", "<i8")] + [(f, "<f8") for f in INTENSITY_SUMS]
                               + [("v_min", "<f4"), ("v_max", "<f4"), ("pad", "<u4", (2,))])
INTENSITY_DTYPE_U16 = np.dtype([("count", "<i8")] + [(f, "<u8") for f in INTENSITY_SUMS]
                               + [("v_min", "<u4"), ("v_max", "<u4"), ("pad", "<u4", (2,))])
assert INTENSITY_DTYPE_F32.itemsize == 64 and INTENSITY_DTYPE_U16.itemsize == 64


def _tile_shape(entry: str) -> tuple[int, int, int]:
    zyx = (ctypes.c_int * 3)()
    _lib.call(entry, zyx)
    return tuple(zyx)


def tile_shape() -> tuple[int, int, int]:
    """The ``(z, y, x)`` tile one workgroup labels in LDS (``lsr_label_tile_shape``)."""
    return _tile_shape("lsr_label_tile_shape")


def _launch_geometry(entry: str) -> tuple[int, int, int, int, int]:
    out = (ctypes.c_int64 * 5)()
    _lib.call(entry, out)
    return tuple(int(v) for v in out)


def launch_geometry() -> tuple[int, int, int, int, int]:
    """``(threads per workgroup, voxels per workgroup of the numbering launches, threads of the scan's one workgroup, cap of
    the grid-stride launches' grids, cap of the local launch's grid)`` of ``csrc/label.hip`` (``lsr_label_launch_geometry``)."""
    return _launch_geometry("lsr_label_launch_geometry")


def _run(device, entry: str, *args) -> None:
    import torch

    if device.type == "cpu":
        _lib.call(entry + "_cpu", *args, None)
        return
    with torch.cuda.device(device):
        _lib.call(entry, *args, _lib.stream_ptr(device))


def _check_volume(t, name: str, dtype):
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() != 3:
        raise ValueError(f"{name} must be (Z, Y, X), got shape {tuple(t.shape)}")
    if t.device.type not in ("cpu", "cuda"):
        raise ValueError(f"{name} is on {t.device}: a HIP device or the CPU")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


# ---- shared with distance.py, watershed.py and track.py --------------------------------------------------------------------------

def _shape3(t, name: str) -> tuple[int, int, int]:
    """``(z, y, x)`` of a checked volume that must not be empty."""
    z, y, x = (int(v) for v in t.shape)
    if min(z, y, x) <= 0:
        raise ValueError(f"{name} must not be empty, got shape {(z, y, x)}")
    return z, y, x


def _same_volume(a, b, name_a: str, name_b: str) -> None:
    """``b`` has ``a``'s shape and sits on ``a``'s device."""
    if b.shape != a.shape or b.device != a.device:
        raise ValueError(f"{name_b} {tuple(b.shape)} on {b.device} does not match {name_a} {tuple(a.shape)} on {a.device}")


def _connectivity(connectivity) -> int:
    if connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    return int(connectivity)


def _scratch(entry: str, z: int, y: int, x: int, device):
    """The scratch buffer ``entry`` (a ``*_scratch_bytes``) asks for at this shape, as a uint8 tensor on ``device``."""
    import torch

    scratch_bytes = _lib.call_value(entry, z, y, x)
    if scratch_bytes < 0:
        _lib.call(entry, z, y, x)       # (raises with the library's message)
    return torch.empty((max(scratch_bytes, 4),), dtype=torch.uint8, device=device)


def _fill_pair_table(device, dtype: np.dtype, capacity: int, ceiling: int, what: str, launch) -> np.ndarray:
    """The claimed records of an open-addressing pair table (``csrc/pair_table.hpp``) as a host array of ``dtype``, sorted by
    ``pair``.  ``launch(capacity, table_ptr, counts_ptr)`` fills a zeroed table of ``capacity`` records and sets ``counts =
    (claimed, lost)``; while a contribution is lost the capacity doubles and the pass runs again, up to ``ceiling`` slots
    (then :class:`RuntimeError`, which begins with ``what.format(lost)``: the caller's name and what was lost)."""
    import torch

    while True:
        table = torch.zeros((capacity * dtype.itemsize,), dtype=torch.uint8, device=device)   # the host zeroes it
        counts = torch.empty((2,), dtype=torch.int32, device=device)
        launch(capacity, table.data_ptr(), counts.data_ptr())
        claimed, lost = (int(v) for v in counts.cpu().tolist())
        if lost == 0:
            break
        del table
        if capacity >= ceiling:
            raise RuntimeError(f"{what.format(lost)} found no slot in a table of {capacity} slots ({claimed} claimed), the ceiling")
        capacity *= 2
    rows = table.cpu().numpy().view(dtype)
    rows = rows[rows["pair"] != 0]
    rows = rows[np.argsort(rows["pair"], kind="stable")]
    assert len(rows) == claimed
    return rows


def label_volume(vol, threshold: float, connectivity: int = 6):
    """Label the components of ``vol > threshold`` ((Z, Y, X) float32): ``(labels, n)``.

    ``labels`` is a new ``int32`` tensor on ``vol``'s device (0 on the background, ``1 .. n`` in raster order of each
    component's first voxel); ``n`` is a Python int (one small device-to-host copy).  ``connectivity`` is 6 (scipy's
    default), 18 or 26."""
    import torch

    vol = _check_volume(vol, "vol", torch.float32)
    connectivity = _connectivity(connectivity)
    z, y, x = _shape3(vol, "vol")
    scratch = _scratch("lsr_label_scratch_bytes", z, y, x, vol.device)
    labels = torch.empty((z, y, x), dtype=torch.int32, device=vol.device)
    count = torch.empty((1,), dtype=torch.int32, device=vol.device)
    _run(vol.device, "lsr_label_f32", vol.data_ptr(), z, y, x, ctypes.c_float(float(threshold)), connectivity,
         labels.data_ptr(), count.data_ptr(), scratch.data_ptr())
    return labels, int(count.cpu().item())


def _raw_table(labels, n: int, intensity=None) -> np.ndarray:
    """The ``n`` records of ``lsr_label_regions_f32`` as a host structured array (``REGION_DTYPE``)."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    n = int(n)
    if n < 0:
        raise ValueError(f"n must not be negative, got {n}")
    if intensity is not None:
        intensity = _check_volume(intensity, "intensity", torch.float32)
        _same_volume(labels, intensity, "labels", "intensity")
    if n == 0:
        return np.zeros((0,), dtype=REGION_DTYPE)
    z, y, x = (int(v) for v in labels.shape)
    table = torch.zeros((n * REGION_DTYPE.itemsize,), dtype=torch.uint8, device=labels.device)     # the host zeroes it
    _run(labels.device, "lsr_label_regions_f32", labels.data_ptr(), None if intensity is None else intensity.data_ptr(),
         z, y, x, n, table.data_ptr())
    return table.cpu().numpy().view(REGION_DTYPE).copy()


def region_table(labels, n: int, intensity=None) -> dict:
    """One row per label ``1 .. n``, as a dict of numpy arrays of length ``n``:

    ``label``, ``volume`` (voxels), ``bbox`` ((n, 6): z0, y0, x0, z1, y1, x1, half-open), ``sum_zyx`` ((n, 3) int64),
    ``centroid`` ((n, 3) float64, in voxels); with ``intensity`` also ``intensity_sum``, ``intensity_mean``,
    ``intensity_min``, ``intensity_max``, ``intensity_sum_zyx`` (sum of v * coordinate) and ``weighted_centroid``
    (NaN where an object's intensities sum to zero)."""
    raw = _raw_table(labels, n, intensity)
    vol = raw["volume"].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {
            "label": np.arange(1, len(raw) + 1, dtype=np.int32),
            "volume": vol,
            "bbox": np.concatenate([raw["lo"], raw["hi"]], axis=1).astype(np.int32).reshape(len(raw), 6),
            "sum_zyx": raw["sum_zyx"].astype(np.int64).reshape(len(raw), 3),
            "centroid": raw["sum_zyx"].reshape(len(raw), 3) / vol[:, None].astype(np.float64),
        }
        if intensity is not None:
            out.update({
                "intensity_sum": raw["sum_v"].astype(np.float64),
                "intensity_mean": raw["sum_v"] / vol.astype(np.float64),
                "intensity_min": raw["v_min"].astype(np.float32),
                "intensity_max": raw["v_max"].astype(np.float32),
                "intensity_sum_zyx": raw["sum_vzyx"].astype(np.float64).reshape(len(raw), 3),
                "weighted_centroid": raw["sum_vzyx"].reshape(len(raw), 3) / raw["sum_v"][:, None],
            })
    return out


def filter_map(volumes, min_volume: int = 0, keep_largest: bool = False) -> np.ndarray:
    """``map`` (int32, ``len(volumes) + 1`` entries, ``map[0] == 0``) of :func:`filter_objects`: label ``k`` becomes
    ``map[k]`` -- 0 if dropped, otherwise its rank among the kept labels."""
    volumes = np.asarray(volumes, dtype=np.int64)
    keep = volumes >= int(min_volume)
    if keep_largest and keep.any():
        best = int(np.argmax(np.where(keep, volumes, -1)))          # (argmax: the first of equals, the lowest label)
        keep = np.zeros_like(keep)
        keep[best] = True
    out = np.zeros((len(volumes) + 1,), dtype=np.int32)
    out[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return out


def filter_objects(labels, table: dict, min_volume: int = 0, keep_largest: bool = False):
    """Drop the objects of fewer than ``min_volume`` voxels and, with ``keep_largest``, all but the one of greatest volume
    among the rest (ties: the lowest label).  The kept labels are renumbered ``1 .. M`` in their old order, IN PLACE in
    ``labels`` (the host builds the map from the table, the device applies it).  Returns ``(labels, table_of_the_kept, M)``."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    lut = filter_map(table["volume"], min_volume, keep_largest)
    kept = lut[1:] > 0
    if not kept.all():
        d_lut = torch.from_numpy(lut).to(labels.device)
        _run(labels.device, "lsr_label_remap_i32", labels.data_ptr(), labels.numel(), d_lut.data_ptr(), len(lut))
        _lib.mark_written(labels)
    out = {k: v[kept] for k, v in table.items()}
    out["label"] = np.arange(1, int(kept.sum()) + 1, dtype=np.int32)
    return labels, out, int(kept.sum())


def moments_geometry() -> tuple[int, int]:
    """``(LDS table slots per workgroup, default cap of the grid)`` of the moment kernel (``lsr_label_moments_geometry``)."""
    out = (ctypes.c_int * 2)()
    _lib.call("lsr_label_moments_geometry", out)
    return int(out[0]), int(out[1])


def _raw_moments(labels, n: int, _max_blocks: int = 0) -> np.ndarray:
    """The ``n`` records of ``lsr_label_moments_i32`` as a host structured array (``MOMENTS_DTYPE``)."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    n = int(n)
    if n < 0:
        raise ValueError(f"n must not be negative, got {n}")
    z, y, x = _shape3(labels, "labels")
    if n == 0:
        return np.zeros((0,), dtype=MOMENTS_DTYPE)
    table = torch.zeros((n * MOMENTS_DTYPE.itemsize,), dtype=torch.uint8, device=labels.device)     # the host zeroes it
    _run(labels.device, "lsr_label_moments_i32", labels.data_ptr(), z, y, x, n, table.data_ptr(), int(_max_blocks))
    return table.cpu().numpy().view(MOMENTS_DTYPE).copy()


def moment_table(labels, n: int, _max_blocks: int = 0) -> dict:
    """The integer moments of the labels ``1 .. n`` of a (Z, Y, X) int32 tensor (CPU or HIP), as a dict of int64 numpy arrays of
    length ``n``: ``volume``, ``s_z``, ``s_y``, ``s_x`` (sums of the coordinates) and ``m_zz``, ``m_yy``, ``m_xx``, ``m_zy``,
    ``m_zx``, ``m_yx`` (sums of their products), in absolute voxel indices.  Exact: pure integer arithmetic on the device and in
    the host twin (``csrc/moments.hpp``).  Labels outside ``1 .. n`` are ignored, a label that no voxel carries has a zero row.
    ``_max_blocks`` caps the grid (0: the kernel's default; the result does not depend on it)."""
    raw = _raw_moments(labels, n, _max_blocks)
    return {f: np.ascontiguousarray(raw[f], dtype=np.int64) for f in MOMENT_FIELDS}


def intensity_geometry() -> tuple[int, int]:
    """``(LDS table slots per workgroup, default cap of the grid)`` of the intensity kernel (``lsr_label_intensity_geometry``)."""
    out = (ctypes.c_int * 2)()
    _lib.call("lsr_label_intensity_geometry", out)
    return int(out[0]), int(out[1])


def _raw_intensity(labels, n: int, values, _max_blocks: int = 0) -> np.ndarray:
    """The ``n`` records of ``lsr_label_intensity_f32`` / ``_u16`` as a host structured array (``INTENSITY_DTYPE_F32`` /
    ``INTENSITY_DTYPE_U16``, by ``values``' type)."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    n = int(n)
    if n < 0:
        raise ValueError(f"n must not be negative, got {n}")
    if not isinstance(values, torch.Tensor) or values.dtype not in (torch.float32, torch.uint16):
        raise TypeError(f"values must be a float32 or uint16 torch.Tensor, got {getattr(values, 'dtype', type(values).__name__)}")
    values = _check_volume(values, "values", values.dtype)
    _same_volume(labels, values, "labels", "values")
    z, y, x = _shape3(labels, "labels")
    entry, dtype = (("lsr_label_intensity_f32", INTENSITY_DTYPE_F32) if values.dtype == torch.float32
                    else ("lsr_label_intensity_u16", INTENSITY_DTYPE_U16))
    if n == 0:
        return np.zeros((0,), dtype=dtype)
    table = torch.zeros((n * dtype.itemsize,), dtype=torch.uint8, device=labels.device)     # the host zeroes it
    _run(labels.device, entry, labels.data_ptr(), values.data_ptr(), z, y, x, n, table.data_ptr(), int(_max_blocks))
    return table.cpu().numpy().view(dtype).copy()


def intensity_table(labels, n: int, values, _max_blocks: int = 0) -> dict:
    """What the labels ``1 .. n`` of a (Z, Y, X) int32 tensor hold in ``values``, a float32 or uint16 tensor of the same shape on
    the same device (CPU or HIP), one row per label, as a dict of numpy arrays of length ``n`` (``csrc/intensity.hip``: one pass
    over both volumes, runs of equal labels reduced inside the wave, a table in LDS per workgroup; the twins in
    ``csrc/host_twins.hip``; the rule in ``csrc/intensity.hpp``):

    ``label``, ``count`` (int64), ``sum`` and ``sum_sq`` (float64 for float32 values, uint64 and exact for uint16 values),
    ``mean``, ``std`` (the population standard deviation in float64: ``sqrt(max(sum_sq / n - mean^2, 0))``), ``min`` and ``max``
    (``values``' type), ``sum_zyx`` ((n, 3): the sums of ``v z``, ``v y``, ``v x`` in absolute voxel indices) and
    ``weighted_centroid`` ((n, 3) float64 = ``sum_zyx / sum``, NaN where ``sum`` is 0).

    ``count``, ``min`` and ``max`` are exact; -0.0 sorts below +0.0 and a NaN is an object's ``max`` or ``min`` by its sign bit,
    as in :func:`region_table`.  A float64 sum is within ``2 n_k 2^-53 sum|terms|`` of the exact sum (atomic adds: not
    bit-reproducible on the device); uint16 sums are integers.  Labels outside ``1 .. n`` are ignored; a label that no voxel
    carries has zeros and a NaN ``mean``, ``std`` and ``weighted_centroid``.  ``_max_blocks`` caps the grid (0: the kernel's
    default)."""
    raw = _raw_intensity(labels, n, values, _max_blocks)
    count = raw["count"].astype(np.int64)
    sum_zyx = np.stack([raw["sum_vz"], raw["sum_vy"], raw["sum_vx"]], axis=1) if len(raw) else np.zeros((0, 3), raw["sum_vz"].dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        total = raw["sum_v"].astype(np.float64)
        mean = total / count.astype(np.float64)
        variance = raw["sum_vv"].astype(np.float64) / count.astype(np.float64) - mean * mean
        # (a NaN variance stays NaN: an object that holds a NaN or an infinity has no standard deviation)
        std = np.sqrt(np.where(variance < 0.0, 0.0, variance))
        centroid = sum_zyx.astype(np.float64) / np.where(total == 0.0, np.nan, total)[:, None]
    return {
        "label": np.arange(1, len(raw) + 1, dtype=np.int32), "count": count,
        "sum": np.ascontiguousarray(raw["sum_v"]), "sum_sq": np.ascontiguousarray(raw["sum_vv"]), "mean": mean, "std": std,
        "min": np.ascontiguousarray(raw["v_min"]).astype(np.float32 if raw.dtype == INTENSITY_DTYPE_F32 else np.uint16),
        "max": np.ascontiguousarray(raw["v_max"]).astype(np.float32 if raw.dtype == INTENSITY_DTYPE_F32 else np.uint16),
        "sum_zyx": np.ascontiguousarray(sum_zyx), "weighted_centroid": centroid,
    }


def shell_labels(labels, distance: float, gap: float = 0.0, sampling=(1, 1, 1)):
    """A ring of local background around every object of ``labels`` ((Z, Y, X) int32): a voxel within ``gap`` of an object (the
    objects included) is 0, a voxel farther than that and within ``gap + distance`` carries the label of its nearest object, in
    units of ``sampling`` -- ``expand_labels(labels, gap + distance)`` where ``expand_labels(labels, gap) == 0``, else 0.  A new
    int32 tensor.  The rings of neighbouring objects do not overlap, because ``distance.expand_labels`` does not."""
    import torch

    from . import distance as D

    distance, gap = float(distance), float(gap)
    if not (np.isfinite(distance) and distance >= 0 and np.isfinite(gap) and gap >= 0):
        raise ValueError(f"distance and gap must be finite and not negative, got {distance!r} and {gap!r}")
    inner = D.expand_labels(labels, gap, sampling)
    outer = D.expand_labels(labels, gap + distance, sampling)
    return torch.where(inner == 0, outer, torch.zeros_like(outer))


def _sampling3(sampling) -> tuple[float, float, float]:
    s = tuple(float(v) for v in sampling)
    if len(s) != 3 or not all(np.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"sampling must be three positive numbers (z, y, x), got {sampling!r}")
    return s


def _face_areas(sampling) -> np.ndarray:
    """The area of one face perpendicular to z, to y and to x."""
    sz, sy, sx = sampling
    return np.asarray([sy * sx, sz * sx, sz * sy], dtype=np.float64)


def _self_overlaps(labels, n: int) -> list[dict]:
    """Per axis ``c`` the overlap table of ``labels`` with itself under the unit shift along ``c`` (``track.label_overlaps``),
    restricted to the labels ``1 .. n``: every face-adjacent pair of voxels of the volume, once."""
    from . import track         # (track imports this module)

    tables = []
    for c in range(3):
        shift = [0, 0, 0]
        shift[c] = 1
        t = track.label_overlaps(labels, labels, tuple(shift))
        keep = (t["a"] <= n) & (t["b"] <= n)
        tables.append({k: v[keep] for k, v in t.items()})
    return tables


def _pair_faces(overlaps: list[dict]):
    """``(a, b, faces_zyx)`` of the pairs ``a < b`` that share a face, sorted by ``(a, b)``: the contact of ``a < b`` along ``c``
    is ``n_ab(c) + n_ba(c)``."""
    keys, counts, axes = [], [], []
    for c, t in enumerate(overlaps):
        off = t["a"] != t["b"]
        a, b = t["a"][off], t["b"][off]
        keys.append(np.minimum(a, b) << 32 | np.maximum(a, b))
        counts.append(t["count"][off])
        axes.append(np.full((int(off.sum()),), c, dtype=np.int64))
    pairs, inverse = np.unique(np.concatenate(keys), return_inverse=True)
    faces = np.zeros((len(pairs), 3), dtype=np.int64)
    np.add.at(faces, (inverse.reshape(-1), np.concatenate(axes)), np.concatenate(counts))
    return (pairs >> 32).astype(np.int64), (pairs & 0xFFFFFFFF).astype(np.int64), faces


def contact_table(labels, sampling=(1, 1, 1)) -> dict:
    """The pairs of labels that share a face: ``{"a", "b", "faces_zyx", "area"}`` with ``a < b``, sorted by ``(a, b)`` --
    ``faces_zyx`` ((P, 3) int64) counts the shared faces perpendicular to z, to y and to x, exactly; ``area`` (float64) is
    ``faces_z * sy * sx + faces_y * sz * sx + faces_x * sz * sy`` under ``sampling = (sz, sy, sx)``.  Labels ``<= 0`` are
    background.  Built from three :func:`shrimpy_amd.track.label_overlaps` calls, on the device the labels are on."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    _shape3(labels, "labels")
    sampling = _sampling3(sampling)
    a, b, faces = _pair_faces(_self_overlaps(labels, 2 ** 31 - 1))
    return {"a": a, "b": b, "faces_zyx": faces, "area": faces.astype(np.float64) @ _face_areas(sampling)}


def _covariances(m: dict, sampling) -> np.ndarray:
    """``(n, 3, 3)`` float64: ``C_ab = s_a s_b (N m_ab - S_a S_b) / N^2`` with the numerator in exact integers (int64 where
    ``N * m`` stays below 2^62, Python integers otherwise) and rounded once, plus ``s_a^2 / 12`` on the diagonal; NaN where
    ``N == 0``."""
    vol = m["volume"]
    n = len(vol)
    sums = (m["s_z"], m["s_y"], m["s_x"])
    second = {(0, 0): m["m_zz"], (1, 1): m["m_yy"], (2, 2): m["m_xx"], (0, 1): m["m_zy"], (0, 2): m["m_zx"], (1, 2): m["m_yx"]}
    # (S_a^2 <= N m_aa, so the diagonal bounds every term of every numerator)
    wide = n > 0 and max(float(np.max(vol.astype(np.float64) * second[(a, a)].astype(np.float64))) for a in range(3)) >= 2.0 ** 62
    as_int = (lambda v: v.astype(object)) if wide else (lambda v: v)
    cov = np.full((n, 3, 3), np.nan, dtype=np.float64)
    live = vol > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_n2 = 1.0 / (vol.astype(np.float64) * vol.astype(np.float64))
        for (a, b), mab in second.items():
            numerator = as_int(vol) * as_int(mab) - as_int(sums[a]) * as_int(sums[b])
            value = numerator.astype(np.float64) * (sampling[a] * sampling[b]) * inv_n2
            if a == b:
                value = value + sampling[a] * sampling[a] / 12.0
            cov[:, a, b] = cov[:, b, a] = np.where(live, value, np.nan)
    return cov


def shape_table(labels, n: int, sampling=(1, 1, 1), bbox=None) -> dict:
    """The shape and the contacts of the labels ``1 .. n`` ((Z, Y, X) int32, CPU or HIP), one row per label, as a dict of numpy
    arrays.  ``sampling = (sz, sy, sx)`` is the voxel spacing; lengths and areas are in its units.

    The rules.

    * Moments: :func:`moment_table` (exact integers); its ten columns are returned as they are.
    * ``covariance`` ((n, 3, 3) float64): ``C_ab = s_a s_b (N m_ab - S_a S_b) / N^2``, the numerator in exact integers and
      rounded once, plus ``s_a^2 / 12`` on the diagonal -- a voxel counts as a uniform cell, so that a box of ``L`` voxels has
      exactly the continuous box's variance ``(L s)^2 / 12`` and a single voxel is not degenerate.
    * ``eigenvalues`` ((n, 3), ``l0 >= l1 >= l2``): ``numpy.linalg.eigh`` of ``C``, clipped at 0.  ``axis_lengths`` ((n, 3):
      major, mid, minor) ``= 2 sqrt(5 l)``: the full axes of the solid ellipsoid with these second moments.
    * ``major_axis`` ((n, 3), z y x): the unit eigenvector of ``l0``, its first non-zero component positive (a component of
      magnitude below ``1e-12`` counts as zero and is returned as 0).
    * Faces: for the axis ``c`` let ``n_ab(c)`` be the overlap table of the labels with themselves under the unit shift along
      ``c`` (``track.label_overlaps``).  The exposed faces of ``k`` perpendicular to ``c`` are ``2 volume_k - 2 n_kk(c)``
      (``faces_zyx``, (n, 3) int64): faces against the background, against another label and against the border of the volume
      alike.  The contact of ``a < b`` along ``c`` is ``n_ab(c) + n_ba(c)``; ``contact_faces_zyx`` sums a label's contacts,
      ``n_neighbours`` counts the distinct labels it touches.  All exact.
    * ``surface_area = faces_z sy sx + faces_y sz sx + faces_x sz sy``: the STAIRCASE area of the voxel surface, which does not
      converge to a smooth surface's (it is about 1.5 times a sphere's), so no sphericity is derived from it.
      ``contact_area`` is the same sum over ``contact_faces_zyx``.
    * ``touches_border`` (bool): the bounding box reaches a face of the volume.  ``bbox`` ((n, 6), :func:`region_table`'s) is
      measured here unless it is handed in.

    A label that no voxel carries has zero counts, NaN lengths and ``touches_border`` False.

    Not built: a smoothed (Crofton-weight) area estimator and sphericity, ``label_regions_kernel`` on the moment kernel's form
    (:func:`intensity_table` has it; :func:`region_table` has not been moved), multi-GPU tables."""
    import torch

    labels = _check_volume(labels, "labels", torch.int32)
    shape = _shape3(labels, "labels")
    sampling = _sampling3(sampling)
    n = int(n)
    moments = moment_table(labels, n)
    vol = moments["volume"]
    cov = _covariances(moments, sampling)
    live = vol > 0
    eigenvalues = np.full((n, 3), np.nan, dtype=np.float64)
    major = np.full((n, 3), np.nan, dtype=np.float64)
    if live.any():
        w, v = np.linalg.eigh(cov[live])                           # ascending
        eigenvalues[live] = np.clip(w[:, ::-1], 0.0, None)
        axis = v[:, :, 2]
        axis = np.where(np.abs(axis) < 1e-12, 0.0, axis)
        first = np.take_along_axis(axis, np.argmax(axis != 0.0, axis=1)[:, None], axis=1)
        major[live] = axis * np.where(first < 0.0, -1.0, 1.0)
    overlaps = _self_overlaps(labels, n)
    faces = np.zeros((n, 3), dtype=np.int64)
    for c, t in enumerate(overlaps):
        same = t["a"] == t["b"]
        inner = np.zeros((n,), dtype=np.int64)
        inner[t["a"][same] - 1] = t["count"][same]
        faces[:, c] = 2 * vol - 2 * inner
    a, b, pair_faces = _pair_faces(overlaps)
    contact_faces = np.zeros((n, 3), dtype=np.int64)
    np.add.at(contact_faces, a - 1, pair_faces)
    np.add.at(contact_faces, b - 1, pair_faces)
    neighbours = np.bincount(np.concatenate([a, b]) - 1, minlength=n).astype(np.int64) if n > 0 else np.zeros((0,), np.int64)
    if bbox is None:
        bbox = region_table(labels, n)["bbox"]
    bbox = np.asarray(bbox).reshape(n, 6)
    areas = _face_areas(sampling)
    return {
        "label": np.arange(1, n + 1, dtype=np.int32), **moments,
        "covariance": cov, "eigenvalues": eigenvalues, "axis_lengths": 2.0 * np.sqrt(5.0 * eigenvalues), "major_axis": major,
        "faces_zyx": faces, "contact_faces_zyx": contact_faces,
        "surface_area": faces.astype(np.float64) @ areas, "contact_area": contact_faces.astype(np.float64) @ areas,
        "n_neighbours": neighbours,
        "touches_border": live & ((bbox[:, :3] <= 0).any(axis=1) | (bbox[:, 3:] >= np.asarray(shape)).any(axis=1)),
    }


# what `shape: true` adds to segment_zyx's table
SHAPE_COLUMNS = ("axis_lengths", "major_axis", "surface_area", "contact_area", "n_neighbours", "touches_border", "faces_zyx",
                 "contact_faces_zyx", "eigenvalues", "covariance") + MOMENT_FIELDS[1:]


def segment_zyx(vol, settings, sampling=(1, 1, 1)):
    """Threshold, label, measure and filter one (Z, Y, X) float32 volume by a :class:`~shrimpy_amd.settings.SegmentSettings`:
    ``(labels, table, n)``.  With ``sigma > 0`` the blurred volume is thresholded; with ``threshold: otsu`` the threshold is
    the multi-Otsu one of what is thresholded (a constant volume has no objects), with ``threshold: {percentile: p}`` its
    ``p``-th percentile (``stats.quantiles``).  The table's intensities are ``vol``'s.
    With ``background_radius > 0`` the white top-hat of ``vol`` under a box of that radius (in the units of ``sampling``,
    ``shrimpy_amd/morphology.py``) is what is blurred and thresholded; with ``fill_holes`` the mask ``work > threshold`` is
    filled (``scipy.ndimage.binary_fill_holes``) before it is labelled, for every ``connectivity``.  With ``median_radius > 0``
    the median of ``vol`` under a box of that radius (``shrimpy_amd/rank.py``) takes ``vol``'s place before all of that.  With
    ``enhance`` the multi-scale Hessian response of what those two left (``shrimpy_amd/hessian.py``) is what is blurred and
    thresholded.

    ``sampling = (sz, sy, sx)`` is the voxel spacing the distance settings measure in (``shrimpy_amd/distance.py``).  With
    ``split`` the labelled objects are split before anything else sees them (``watershed.split_touching``: the watershed of
    each object's depth map, blurred by ``split_sigma`` voxels, basins shallower than ``split_min_depth`` merged), so the
    table, ``min_volume`` and ``keep_largest`` act on the split objects.  With
    ``expand_distance > 0`` the labels that survive the filter grow into the background by at most that distance (a dropped
    speck claims no space) and the table is that of the grown labels.  With ``inscribed_radius`` the table gains the column
    ``inscribed_radius``: per object the greatest distance of one of its voxels to the nearest background voxel, of the final
    labels (``+inf`` where the volume has no background).  With ``shape`` the final labels -- after the filter and the
    expansion, where ``inscribed_radius`` is measured -- go through :func:`shape_table` and the table gains its columns
    (``SHAPE_COLUMNS``).  ``contacts`` is the ``segment`` command's: it writes :func:`contact_table` of the returned labels."""
    import torch

    from . import dynatrack as D

    vol = _check_volume(vol, "vol", torch.float32)
    work = vol
    radius = settings.median_radius
    if any(float(r) > 0 for r in (radius if isinstance(radius, (tuple, list)) else (radius,))):
        from . import rank

        work = rank.median_filter(work, rank.half_widths_of(radius, sampling))
    radius = settings.background_radius
    if any(float(r) > 0 for r in (radius if isinstance(radius, (tuple, list)) else (radius,))):
        from . import morphology

        work = morphology.subtract_background(work, radius, sampling)
    if settings.enhance is not None:
        from . import hessian

        sigmas, grid = settings.enhance.scales(sampling)
        work = hessian.enhance(work, settings.enhance.measure, sigmas, grid, settings.enhance.dark)
    work = D._gaussian_blur_3d(work, float(settings.sigma)) if settings.sigma > 0 else work
    if settings.threshold == "otsu":
        threshold = D._multiotsu_threshold(work, int(settings.otsu_component))
    elif hasattr(settings.threshold, "percentile"):
        from . import stats

        threshold = stats.quantiles(work, [float(settings.threshold.percentile) / 100.0])[0]
    else:
        threshold = float(settings.threshold)
    if settings.fill_holes:
        from . import morphology

        # (the filled mask as a volume of 0 and 1: its components under `connectivity` are the filled objects)
        labels, n = label_volume(morphology.fill_holes(work > threshold).to(torch.float32), 0.5, int(settings.connectivity))
    else:
        labels, n = label_volume(work, threshold, int(settings.connectivity))
    if settings.split and n > 0:
        from . import watershed

        labels, n = watershed.split_touching(labels, sampling, float(settings.split_sigma), float(settings.split_min_depth),
                                             int(settings.connectivity))
    table = region_table(labels, n, vol)
    if settings.min_volume > 0 or settings.keep_largest:
        labels, table, n = filter_objects(labels, table, int(settings.min_volume), bool(settings.keep_largest))
    if settings.expand_distance > 0 or settings.inscribed_radius:
        from . import distance

        if settings.expand_distance > 0:
            labels = distance.expand_labels(labels, float(settings.expand_distance), sampling)
            table = region_table(labels, n, vol)
        if settings.inscribed_radius:
            depth = distance.distance_transform_labels(labels, sampling, invert=True)
            table["inscribed_radius"] = (region_table(labels, n, depth)["intensity_max"] if n > 0
                                         else np.zeros((0,), dtype=np.float32))
    if settings.shape:
        measured = shape_table(labels, n, sampling, bbox=table["bbox"])
        table.update({k: measured[k] for k in SHAPE_COLUMNS})
    return labels, table, n
