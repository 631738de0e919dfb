"""Splitting touching objects: a watershed by steepest ascent on a surface, and a merge of its basins by depth.

``csrc/watershed.hip`` runs on the device, ``csrc/host_twins.hip`` on the CPU over the same rule (``csrc/watershed.hpp``).
PARITY UNPINNED: no upstream is pinned -- ``skimage`` is not a dependency, and ``scipy.ndimage.watershed_ift`` breaks ties by
queue order, which no parallel algorithm reproduces.  The rule below is the specification; ``tests/watershed_ref.py`` restates
it in numpy, and device, twin and restatement agree element for element.

The rule.  ``objects`` is int32 (values ``<= 0`` are background), ``surface`` float32, ``connectivity`` 6, 18 or 26.

* Surface values compare by the order-preserving integer image of a float (``lsr::label::float_key``): a total order in which
  ``-0.0`` sorts below ``+0.0`` and ``+inf`` is an ordinary value.  NaN is unsupported (but cannot hang or fault anything).
* ``N(v)``: the neighbours of ``v`` inside the volume with ``objects[u] == objects[v]`` -- a split never joins two objects.
* ``up(v)``: the element of ``N(v) + {v}`` with the greatest (surface, then the SMALLER linear index): a strict total order, so
  plateaus need no special case; ``up(v) == v`` exactly at a basin's summit.
* Basins: the connected components of the edges ``{v, up(v)}``, numbered ``1 .. B`` in raster order of each basin's smallest
  linear index (``segment.label_volume``'s numbering); ``B`` is the number of summits.
* Saddles: for neighbours ``v, u`` of one object in different basins ``a < b``, ``pass = min(surface[v], surface[u])``;
  ``saddle(a, b)`` is the greatest pass.  ``peak(a)`` is the greatest surface value of basin ``a``.
* Merge (host, float64): the saddle edges sorted by saddle descending, then ``a``, then ``b`` ascending, go through a union-find
  over the basins rooted at the smallest label; a cluster's peak is the greatest of its members'.  For an edge whose ends are
  in different clusters ``depth = 0`` where the saddle equals the lower of the two cluster peaks bit for bit (``inf`` against
  ``inf``), else ``min(peak) - saddle``; the clusters merge iff ``depth <= min_depth``.  Clusters are renumbered ``1 .. M`` by
  their smallest basin label.  ``min_depth = 0`` merges exactly the summits that the index tie-break split; ``min_depth =
  +inf`` returns the connected components of the objects.

* :func:`watershed_basins` -- ``(basins, B)``.
* :func:`basin_saddles` -- ``{"a", "b", "saddle"}`` sorted by ``(a, b)``.
* :func:`merge_map` -- the look-up table of the merge.
* :func:`split_labels` -- basins, peaks, saddles, merge, relabel: ``(labels, M)``.
* :func:`split_touching` -- the depth map of a label volume (the exact Euclidean distance to the background), blurred, then
  :func:`split_labels`: what ``SegmentSettings.split`` runs.

Not built: seeded (marker) watersheds, a compact-watershed term, watershed lines, multi-GPU or slab splitting, volumes above
``2^31 - 1`` voxels.
"""

from __future__ import annotations

import numpy as np

from . import _lib
from .segment import (_check_volume, _connectivity, _fill_pair_table, _launch_geometry, _run, _same_volume, _scratch, _shape3,
                      _tile_shape, region_table)

__all__ = ["SADDLE_DTYPE", "MAX_CAPACITY", "tile_shape", "launch_geometry", "watershed_basins", "basin_saddles", "merge_map", "split_labels",
           "split_touching"]

# one slot of the saddle table (csrc/watershed.hpp ``Saddle``)
SADDLE_DTYPE = np.dtype([("pair", "<u8"), ("key", "<u4"), ("unused", "<u4")])
assert SADDLE_DTYPE.itemsize == 16
# the ceiling of basin_saddles' retries: 2^28 slots, 4 GiB
MAX_CAPACITY = 1 << 28


def tile_shape() -> tuple[int, int, int]:
    """The ``(z, y, x)`` tile one workgroup stages in LDS (``lsr_watershed_tile_shape``)."""
    return _tile_shape("lsr_watershed_tile_shape")


def launch_geometry() -> tuple[int, int, int, int, int]:
    """:func:`shrimpy_amd.segment.launch_geometry` of ``csrc/watershed.hip``, which compiles its own copy of the numbering
    launches (``lsr_watershed_launch_geometry``)."""
    return _launch_geometry("lsr_watershed_launch_geometry")


def _key_to_float(keys: np.ndarray) -> np.ndarray:
    """The float32 values whose ``float_key`` the uint32 ``keys`` are."""
    keys = np.asarray(keys, dtype=np.uint32)
    bits = np.where(keys & np.uint32(0x80000000), keys & np.uint32(0x7FFFFFFF), ~keys).astype(np.uint32)
    return bits.view(np.float32)


def _float_to_key(values: np.ndarray) -> np.ndarray:
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def _pair(objects, surface):
    import torch

    objects = _check_volume(objects, "objects", torch.int32)
    surface = _check_volume(surface, "surface", torch.float32)
    _same_volume(objects, surface, "objects", "surface")
    return objects, surface, _shape3(objects, "objects")


def watershed_basins(objects, surface, connectivity: int = 6):
    """The basins of ``surface`` ((Z, Y, X) float32) inside each object of ``objects`` (int32, same shape and device):
    ``(basins, B)`` -- a new int32 tensor (0 on the background, ``1 .. B`` in raster order of each basin's first voxel) and the
    basin count as a Python int (one small device-to-host copy)."""
    import torch

    objects, surface, (z, y, x) = _pair(objects, surface)
    connectivity = _connectivity(connectivity)
    scratch = _scratch("lsr_watershed_scratch_bytes", z, y, x, objects.device)
    basins = torch.empty((z, y, x), dtype=torch.int32, device=objects.device)
    count = torch.empty((1,), dtype=torch.int32, device=objects.device)
    _run(objects.device, "lsr_watershed_f32", objects.data_ptr(), surface.data_ptr(), z, y, x, connectivity, basins.data_ptr(),
         count.data_ptr(), scratch.data_ptr())
    return basins, int(count.cpu().item())


def basin_saddles(objects, basins, n_basins: int, surface, connectivity: int = 6, _capacity: int | None = None) -> dict:
    """The saddles between the basins: ``{"a", "b"}`` (int32, ``a < b``) and ``"saddle"`` (float32), sorted by ``(a, b)``.

    The device fills an open-addressing table; its first capacity is the power of two at or above ``4 * n_basins + 1024``, and
    while a neighbour pair finds no slot the capacity doubles and the pass runs again, up to ``MAX_CAPACITY`` slots (then
    :class:`RuntimeError`).  ``_capacity`` sets the first capacity (a power of two; tests force the retry with it)."""
    import torch

    objects, surface, (z, y, x) = _pair(objects, surface)
    basins = _check_volume(basins, "basins", torch.int32)
    _same_volume(objects, basins, "objects", "basins")
    connectivity = _connectivity(connectivity)
    empty = {"a": np.zeros((0,), np.int32), "b": np.zeros((0,), np.int32), "saddle": np.zeros((0,), np.float32)}
    if int(n_basins) < 2:
        return empty
    capacity = int(_capacity) if _capacity is not None else 1 << int(4 * int(n_basins) + 1024 - 1).bit_length()
    if capacity <= 0 or capacity & (capacity - 1):
        raise ValueError(f"_capacity must be a power of two, got {capacity}")

    def launch(capacity, table_ptr, counts_ptr):
        _run(objects.device, "lsr_watershed_saddles_f32", objects.data_ptr(), basins.data_ptr(), surface.data_ptr(), z, y, x,
             connectivity, capacity, table_ptr, counts_ptr)

    rows = _fill_pair_table(objects.device, SADDLE_DTYPE, capacity, MAX_CAPACITY, "basin_saddles: {} neighbour pairs", launch)
    return {"a": (rows["pair"] >> np.uint64(32)).astype(np.int32), "b": (rows["pair"] & np.uint64(0xFFFFFFFF)).astype(np.int32),
            "saddle": _key_to_float(rows["key"])}


def merge_map(peaks, a, b, saddle, min_depth: float) -> np.ndarray:
    """The look-up table of the merge (int32, ``len(peaks) + 1`` entries, ``map[0] == 0``): basin ``k`` becomes ``map[k]``, the
    rank of its cluster among the clusters in order of their smallest basin label.  ``peaks[k - 1]`` is the peak of basin ``k``
    (float32), ``a, b, saddle`` the saddle edges.  Plain host code: the basin graph is small beside the volume."""
    peaks = np.ascontiguousarray(peaks, dtype=np.float32)
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    saddle = np.ascontiguousarray(saddle, dtype=np.float32)
    min_depth = float(min_depth)
    if np.isnan(min_depth) or min_depth < 0.0:
        raise ValueError(f"min_depth must not be negative, got {min_depth}")
    n = len(peaks)
    parent = list(range(n + 1))
    peak = [np.float32(0)] + list(peaks)                    # of the cluster rooted here
    peak_key = [0] + _float_to_key(peaks).tolist()
    saddle_bits = saddle.view(np.uint32).tolist()

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    order = np.lexsort((b, a, -saddle.astype(np.float64)))
    for e in order.tolist():
        ra, rb = find(int(a[e])), find(int(b[e]))
        if ra == rb:
            continue
        low = ra if peak_key[ra] <= peak_key[rb] else rb          # the lower of the two cluster peaks
        if int(np.float32(peak[low]).view(np.uint32)) == saddle_bits[e]:
            depth = 0.0
        else:
            depth = float(peak[low]) - float(saddle[e])
        if not depth <= min_depth:
            continue
        lo, hi = (ra, rb) if ra < rb else (rb, ra)
        top = ra if peak_key[ra] >= peak_key[rb] else rb
        parent[hi] = lo
        peak[lo], peak_key[lo] = peak[top], peak_key[top]
    roots = np.array([find(k) for k in range(n + 1)], dtype=np.int64)
    is_root = roots == np.arange(n + 1)
    is_root[0] = False
    rank = np.cumsum(is_root)
    out = rank[roots].astype(np.int32)
    out[0] = 0
    return out


def split_labels(objects, surface, connectivity: int = 6, min_depth: float = 0.0):
    """Split every object of ``objects`` along the watersheds of ``surface`` and merge the basins whose depth is at most
    ``min_depth`` (in the units of ``surface``): ``(labels, M)`` -- a new int32 tensor, ``1 .. M`` in raster order of each
    label's first voxel, 0 on the background.  No label spans two objects."""
    import torch

    basins, n = watershed_basins(objects, surface, connectivity)
    if n == 0:
        return basins, 0
    peaks = region_table(basins, n, surface)["intensity_max"]
    edges = basin_saddles(objects, basins, n, surface, connectivity)
    lut = merge_map(peaks, edges["a"], edges["b"], edges["saddle"], min_depth)
    m = int(lut.max())
    if m != n:
        d_lut = torch.from_numpy(lut).to(basins.device)
        _run(basins.device, "lsr_label_remap_i32", basins.data_ptr(), basins.numel(), d_lut.data_ptr(), len(lut))
        _lib.mark_written(basins)
    return basins, m


def split_touching(labels, sampling=(1, 1, 1), sigma: float = 1.0, min_depth: float = 0.0, connectivity: int = 6):
    """Split the touching objects of a label volume ((Z, Y, X) int32): the surface is the depth of every labelled voxel -- its
    exact Euclidean distance to the nearest background voxel in units of ``sampling`` (``distance.distance_transform_labels``
    with ``invert``) -- blurred by a Gaussian of ``sigma`` voxels where ``sigma > 0`` (``dynatrack._gaussian_blur_3d``:
    bit-reproducible), and the split is :func:`split_labels` of it with ``min_depth`` in the same units.  ``(labels, M)``."""
    from . import distance
    from . import dynatrack as D

    sigma = float(sigma)
    if not sigma >= 0.0:
        raise ValueError(f"sigma must not be negative, got {sigma}")
    depth = distance.distance_transform_labels(labels, sampling, invert=True)
    if sigma > 0:
        depth = D._gaussian_blur_3d(depth, sigma)
    return split_labels(labels, depth, connectivity, min_depth)
