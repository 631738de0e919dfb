"""Stitching: the overlapping fields of view of a well placed on one canvas and blended.

biahub's ``estimate-stitch`` / ``stitch`` pair [RECALLED]; biahub is not vendored or installed -- **PARITY UNPINNED**, the
rule is this package's own (``csrc/stitch.hpp``; ``tests/stitch_ref.py`` restates it in float64).  Field names are biahub's
where recalled (``total_translation``, ``blending_exponent``, ``percent_overlap``).

``K`` tiles, each a contiguous float32 ``(Zk, Yk, Xk)``, one float64 translation ``t_k = (tz, ty, tx)`` per tile in canvas
voxels: tile voxel ``i`` sits at canvas coordinate ``i + t_k``.

* Canvas: ``origin = floor(min_k t_k)``, ``shape = ceil(max_k (t_k + n_k)) - origin`` (:func:`canvas_geometry`).
* Per tile and axis ``ti = floor(t)``, ``tf = t - ti``; for the absolute canvas index ``c`` put ``j = c - ti``.  ``tf == 0``:
  one tap ``i = j``, covered iff ``0 <= j <= n - 1``.  Otherwise two taps ``j - 1`` and ``j`` with the float32 weights
  ``float32(tf)`` and ``float32(1 - tf)``, covered iff ``1 <= j <= n - 1``.  A tile covers a voxel iff all three axes are
  covered; nothing is ever interpolated against the fill value.
* Sample ``s_k``: the tile voxel itself, or the linear interpolation over the fractional axes only (x, then y, then z).
* Weight ``w_k = (dy dx)^p`` (``p = blending_exponent`` in ``0 .. 4``, repeated float32 multiplication),
  ``d = min(l + 1, n - l)`` with ``l = c - t``: 1 on a tile's edge, growing towards its middle.  ``p = 0`` is the plain mean,
  ``p = 1`` a linear feather towards the tile edges; z only decides coverage.
* Output: ``cval`` where no tile covers the voxel; ``s_k`` itself where exactly one does (an integer placement copies the
  non-overlapping interior bit for bit); otherwise ``(sum w_k s_k) / (sum w_k)`` in float32, in ascending tile index.

A HIP tensor runs ``csrc/stitch.hip`` on the current stream -- a gather: every canvas voxel is written once from the tile
voxels under it -- a CPU tensor the host twin (the same bits).  Per-tile flips, rotations and affine placement, intensity
equalisation between tiles, multi-GPU compositing and uint16 output are not built.
"""

from __future__ import annotations

import ctypes
import logging

import numpy as np

from . import _lib

__all__ = ["canvas_geometry", "stitch_tiles", "band_plan", "stitch_banded", "grid_placement", "overlap_pairs",
           "solve_placement", "estimate_translations"]

logger = logging.getLogger("shrimpy_amd")
_I64P = ctypes.POINTER(ctypes.c_int64)
_F64P = ctypes.POINTER(ctypes.c_double)


def _geometry_arrays(shapes, translations):
    shp = np.ascontiguousarray(np.asarray(shapes, dtype=np.int64).reshape(-1, 3))
    tr = np.ascontiguousarray(np.asarray(translations, dtype=np.float64).reshape(-1, 3))
    if len(shp) != len(tr) or len(shp) == 0:
        raise ValueError(f"{len(shp)} shapes for {len(tr)} translations: one (z, y, x) of each per tile, at least one tile")
    return shp, tr


def canvas_geometry(shapes, translations):
    """``(shape, origin)`` of the canvas that holds every tile: ``origin = floor(min t)``,
    ``shape = ceil(max (t + n)) - origin``, both ``(z, y, x)`` tuples of ints."""
    shp, tr = _geometry_arrays(shapes, translations)
    origin, shape = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    _lib.call("lsr_stitch_canvas", shp.ctypes.data_as(_I64P), tr.ctypes.data_as(_F64P), len(shp), origin, shape)
    return tuple(int(v) for v in shape), tuple(int(v) for v in origin)


def _check_tiles(tiles):
    import torch

    tiles = list(tiles)
    if not tiles:
        raise ValueError("no tiles")
    for k, t in enumerate(tiles):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"tile {k} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"tile {k} must be float32, got {t.dtype}")
        if t.dim() != 3:
            raise ValueError(f"tile {k} must be (Z, Y, X), got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"tile {k} must be contiguous")
        if t.device != tiles[0].device:
            raise ValueError(f"tile {k} is on {t.device}, tile 0 on {tiles[0].device}")
    if tiles[0].device.type not in ("cpu", "cuda"):
        raise ValueError(f"the tiles are on {tiles[0].device}: a HIP device or the CPU")
    return tiles


def _host_table(tiles, translations):
    """The tile table in host memory (``lsr_stitch_prepare_table``: the float64 split is done there, once)."""
    shp, tr = _geometry_arrays([tuple(t.shape) for t in tiles], translations)
    if len(tr) != len(tiles):
        raise ValueError(f"{len(tr)} translations for {len(tiles)} tiles")
    nbytes = _lib.call_value("lsr_stitch_table_bytes", len(tiles))
    table = np.zeros(max(nbytes, 1), dtype=np.uint8)
    ptrs = (ctypes.c_void_p * len(tiles))(*[t.data_ptr() for t in tiles])
    _lib.call("lsr_stitch_prepare_table", ptrs, shp.ctypes.data_as(_I64P), tr.ctypes.data_as(_F64P), len(tiles),
              table.ctypes.data)
    return table


def stitch_tiles(tiles, translations, blending_exponent: int = 1, cval: float = 0.0, out=None, box=None):
    """The canvas of ``tiles`` (float32 ``(Z, Y, X)`` tensors on one device) at ``translations`` (``(z, y, x)`` per tile,
    canvas voxels), or its ``box = (origin, shape)`` in absolute canvas coordinates -- the whole canvas by default.  Returns a
    float32 tensor of the box's shape on the tiles' device (``out``, when given, is filled and returned).  A tile outside the
    box contributes nothing."""
    import torch

    tiles = _check_tiles(tiles)
    table = _prepare_table(tiles, translations)
    if box is None:
        shape, origin = canvas_geometry([tuple(t.shape) for t in tiles], translations)
    else:
        origin, shape = (tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1]))
        if len(origin) != 3 or len(shape) != 3:
            raise ValueError(f"box must be ((z, y, x) origin, (z, y, x) shape), got {box!r}")
    device = tiles[0].device
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    return _launch(table, len(tiles), device, out, origin, shape, blending_exponent, cval)


def _prepare_table(tiles, translations):
    """The tile table where the launch reads it: host memory (a NumPy array) for CPU tiles, a device tensor for HIP tiles --
    one pageable host-to-device copy, so a caller with several boxes of the same tiles prepares it once."""
    import torch

    table = _host_table(tiles, translations)
    if tiles[0].device.type == "cpu":
        return table
    with torch.cuda.device(tiles[0].device):
        return torch.from_numpy(table).to(tiles[0].device)


def _launch(table, n_tiles: int, device, out, origin, shape, blending_exponent, cval):
    """One box into ``out`` from a prepared table (``_prepare_table``), on the current stream of ``device``."""
    import torch

    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) \
            or not out.is_contiguous() or out.device != device:
        raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(shape)} on {device}")
    o3, s3 = (ctypes.c_int64 * 3)(*origin), (ctypes.c_int64 * 3)(*shape)
    p, cval = int(blending_exponent), float(cval)
    if device.type == "cpu":
        from .host import _threads

        _threads()
        _lib.call("lsr_stitch_f32_cpu", table.ctypes.data, n_tiles, out.data_ptr(), o3, s3, p, cval, None)
    else:
        with torch.cuda.device(device):     # (the table tensor is freed stream-ordered: behind the launches that read it)
            _lib.call("lsr_stitch_f32", table.data_ptr(), n_tiles, out.data_ptr(), o3, s3, p, cval, _lib.stream_ptr(device))
    _lib.mark_written(out)
    return out


def band_plan(shapes, translations, band_rows: int):
    """``[(y0, y1, [tile indices])]``: the canvas cut along y into bands of ``band_rows`` rows (absolute rows ``y0 .. y1 - 1``;
    the last band takes what is left), each with the tiles whose rows reach into it, in ascending index.  A tile's rows are
    taken as ``floor(ty) .. floor(ty) + n - 1``: with a fractional ``ty`` the first of them is not covered, which at most
    lists a tile one band early -- it contributes nothing there."""
    shp, tr = _geometry_arrays(shapes, translations)
    band_rows = int(band_rows)
    if band_rows <= 0:
        raise ValueError(f"band_rows must be positive, got {band_rows}")
    (_, ny, _), (_, oy, _) = canvas_geometry(shp, tr)
    first = np.floor(tr[:, 1]).astype(np.int64)
    last = first + shp[:, 1] - 1
    plan = []
    for y0 in range(oy, oy + ny, band_rows):
        y1 = min(y0 + band_rows, oy + ny)
        plan.append((y0, y1, [k for k in range(len(shp)) if first[k] < y1 and last[k] >= y0]))
    return plan


def _plan_peak_bytes(plan, shapes) -> int:
    return max(sum(4 * int(np.prod(shapes[k])) for k in ks) for _, _, ks in plan)


def stitch_banded(load_tile, shapes, translations, blending_exponent: int = 1, cval: float = 0.0,
                  max_resident_bytes: int | None = None, band_rows: int | None = None, out=None):
    """The canvas composed in bands along y, for tiles that do not fit beside it all at once.  ``load_tile(k)`` returns tile
    ``k`` as a contiguous float32 tensor on the target device; it is called once per tile, when the first band that the tile
    reaches into comes up, and the tile is released after the last.  Each band's launch gets only its own tiles, in ascending
    index, so every voxel sees the tiles it would see in one launch in the same order: the result is bit-identical.

    ``band_rows``: rows per band; left out, the largest power-of-two fraction of the canvas whose bands keep the canvas plus
    the resident tiles within ``max_resident_bytes`` (``ValueError`` when single rows do not).  With neither, one band."""
    import torch

    shp, tr = _geometry_arrays(shapes, translations)
    shape, origin = canvas_geometry(shp, tr)
    if band_rows is None:
        band_rows = shape[1]
        if max_resident_bytes is not None:
            budget = int(max_resident_bytes) - 4 * int(np.prod(shape))
            while _plan_peak_bytes(band_plan(shp, tr, band_rows), shp) > budget:
                if band_rows == 1:
                    raise ValueError(f"a canvas of {shape} and the tiles under one of its rows need more than "
                                     f"max_resident_bytes = {int(max_resident_bytes)}")
                band_rows = max(1, band_rows // 2)
    plan = band_plan(shp, tr, band_rows)
    last_use = {k: b for b, (_, _, ks) in enumerate(plan) for k in ks}
    resident: dict = {}
    for b, (y0, y1, ks) in enumerate(plan):
        for k in ks:
            if k not in resident:
                tile = load_tile(k)
                if tuple(tile.shape) != tuple(int(v) for v in shp[k]):
                    raise ValueError(f"load_tile({k}) returned shape {tuple(tile.shape)}, expected {tuple(shp[k])}")
                resident[k] = tile
        if out is None:
            ref = resident[ks[0]] if ks else load_tile(0)
            out = torch.empty(shape, dtype=torch.float32, device=ref.device)
        band = out[:, y0 - origin[1]:y1 - origin[1], :]
        sub = [resident[k] for k in ks]
        if not ks:                       # (a canvas is spanned by its tiles' floors: every band has a tile; kept for safety)
            band.fill_(float(cval))
        elif band.is_contiguous():       # one band, or a canvas of one plane
            stitch_tiles(sub, tr[ks], blending_exponent, cval, out=band,
                         box=((origin[0], y0, origin[2]), (shape[0], y1 - y0, shape[2])))
        else:
            # the kernel writes a contiguous box; a y band of a (Z, Y, X) canvas is one such box per plane
            # (one launch per plane, all from the band's one table)
            table = _prepare_table(_check_tiles(sub), tr[ks])
            for z in range(shape[0]):
                _launch(table, len(sub), sub[0].device, band[z:z + 1], (origin[0] + z, y0, origin[2]),
                        (1, y1 - y0, shape[2]), blending_exponent, cval)
        for k in [k for k in resident if last_use[k] == b]:
            del resident[k]
    return out


# ---- placement ----------------------------------------------------------------------------------------------------------


def grid_placement(shapes, grid_columns: int, percent_overlap: float):
    """Nominal translations of tiles laid out row-major on a grid with ``grid_columns`` columns, neighbours overlapping by
    ``percent_overlap`` per cent of a tile's extent: tile ``k`` at ``(0, (k // columns) * Y * (1 - f), (k % columns) * X *
    (1 - f))`` with the extents of tile 0."""
    shp = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    cols = int(grid_columns)
    if cols <= 0 or not 0.0 <= float(percent_overlap) < 100.0:
        raise ValueError("grid_columns must be positive and percent_overlap in [0, 100)")
    step = 1.0 - float(percent_overlap) / 100.0
    return [(0.0, (k // cols) * float(shp[0, 1]) * step, (k % cols) * float(shp[0, 2]) * step) for k in range(len(shp))]


def _round_half_up(v):
    return np.floor(np.asarray(v, dtype=np.float64) + 0.5).astype(np.int64)


def overlap_pairs(shapes, initial, min_overlap_voxels: int):
    """``[(i, j, lo, hi)]`` for ``i < j``: the pairs whose boxes under the ROUNDED initial placement share at least
    ``min_overlap_voxels`` per axis; ``lo`` / ``hi`` the shared box in canvas coordinates (int64, ``hi`` exclusive)."""
    shp = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    pos = _round_half_up(np.asarray(initial, dtype=np.float64).reshape(-1, 3))
    out = []
    for i in range(len(shp)):
        for j in range(i + 1, len(shp)):
            lo, hi = np.maximum(pos[i], pos[j]), np.minimum(pos[i] + shp[i], pos[j] + shp[j])
            if np.all(hi - lo >= int(min_overlap_voxels)):
                out.append((i, j, lo, hi))
    return out


def solve_placement(n_tiles: int, anchors, measurements, outlier_threshold_voxels: float):
    """Least squares over pairwise measurements ``(i, j, d_ij)`` (``t_j - t_i ~ d_ij``, float64 ``(z, y, x)``): minimises
    ``sum |(t_j - t_i) - d_ij|^2`` with tile 0 pinned to ``anchors[0]`` (``numpy.linalg.lstsq``).  While a residual
    exceeds ``outlier_threshold_voxels`` the pair with the largest one is dropped and the rest solved again.  A group of tiles that no pair
    connects to tile 0 has its lowest tile pinned to that tile's anchor instead.  Returns ``(t, kept, pinned)``: the
    ``(n_tiles, 3)`` solution, the surviving measurements and the pinned tiles other than 0."""
    anchors = np.asarray(anchors, dtype=np.float64).reshape(n_tiles, 3)
    kept = list(measurements)
    while True:
        # connected groups over the surviving pairs; the lowest tile of each is pinned
        group = list(range(n_tiles))

        def find(a):
            while group[a] != a:
                group[a] = group[group[a]]
                a = group[a]
            return a

        for i, j, _ in kept:
            a, b = find(i), find(j)
            group[max(a, b)] = min(a, b)
        pinned = sorted({find(k) for k in range(n_tiles)})
        free = [k for k in range(n_tiles) if k not in pinned]
        col = {k: c for c, k in enumerate(free)}
        t = anchors.copy()
        if kept and free:
            a_mat = np.zeros((len(kept), len(free)), dtype=np.float64)
            rhs = np.zeros((len(kept), 3), dtype=np.float64)
            for r, (i, j, d) in enumerate(kept):
                rhs[r] = np.asarray(d, dtype=np.float64)
                if j in col:
                    a_mat[r, col[j]] = 1.0
                else:
                    rhs[r] -= anchors[j]
                if i in col:
                    a_mat[r, col[i]] = -1.0
                else:
                    rhs[r] += anchors[i]
            sol = np.linalg.lstsq(a_mat, rhs, rcond=None)[0]
            for k, c in col.items():
                t[k] = sol[c]
        resid = [float(np.linalg.norm((t[j] - t[i]) - np.asarray(d, dtype=np.float64))) for i, j, d in kept]
        if not kept or max(resid) <= float(outlier_threshold_voxels):
            return t, kept, [k for k in pinned if k != 0]
        # one gross outlier spreads its error over every pair of its loops: the worst pair goes first, the rest is re-solved
        kept.pop(int(np.argmax(resid)))


def estimate_translations(tiles_or_loader, shapes, initial, settings) -> dict:
    """The translation of every tile from the phase cross-correlation of its overlaps: ``{name: (z, y, x)}``.

    ``initial``: ``{name: (z, y, x)}``, the nominal placement (its order is the tile order; the first tile is pinned to its
    initial value).  ``shapes``: ``{name: (Z, Y, X)}`` (or a sequence in that order).  ``tiles_or_loader``: ``{name: volume}``
    (tensors on any device, or arrays) or a callable ``(name, (slice_z, slice_y, slice_x)) -> volume`` that returns that crop
    of tile ``name`` -- only the overlaps are ever asked for, all of one tile before the next tile's.  ``settings``:
    :class:`~shrimpy_amd.settings.EstimateStitchSettings` (or its dict).

    For every pair of tiles whose boxes under the rounded initial placement share at least ``min_overlap_voxels`` per axis the
    shared box is cropped from both and ``r = dynatrack._phase_cross_corr(crop_j, crop_i, maximum_shift)`` taken (the sign of
    ``stabilize.py``: ``mov = roll(ref, r)`` gives ``r``; with tile ``j`` as the reference ``r`` is what ``t_j - t_i`` is off by).
    A pair is dropped when a crop is constant (nothing to correlate) or ``|r|`` reaches ``maximum_shift_voxels`` on an axis.
    The rest is solved by :func:`solve_placement` with ``d_ij = round(initial_j) - round(initial_i) + r_ij`` (the crops were
    cut at the rounded placement).  A tile left without any pair keeps its initial placement, with a warning that names it.
    ``round_to_integer`` rounds the solution (half up), so that ``stitch`` copies voxels instead of interpolating."""
    import torch

    from .dynatrack import _phase_cross_corr
    from .settings import EstimateStitchSettings

    if not isinstance(settings, EstimateStitchSettings):
        settings = EstimateStitchSettings(**settings)
    names = list(initial)
    if not names:
        raise ValueError("no tiles")
    shp = [tuple(int(v) for v in (shapes[n] if isinstance(shapes, dict) else shapes[k])) for k, n in enumerate(names)]
    init = np.asarray([initial[n] for n in names], dtype=np.float64).reshape(-1, 3)
    pos = _round_half_up(init)

    def crop(k, lo, hi):
        sl = tuple(slice(int(a - o), int(b - o)) for a, b, o in zip(lo, hi, pos[k]))
        vol = tiles_or_loader(names[k], sl) if callable(tiles_or_loader) else tiles_or_loader[names[k]][sl]
        if not isinstance(vol, torch.Tensor):
            vol = torch.from_numpy(np.ascontiguousarray(vol))
        return vol.to(torch.float32).contiguous()

    # every crop of a tile is asked for before the next tile's: a loader that reads whole volumes reads each one once
    pairs = overlap_pairs(shp, init, settings.min_overlap_voxels)
    crops = {(k, n): crop(k, lo, hi) for k in range(len(names)) for n, (i, j, lo, hi) in enumerate(pairs) if k in (i, j)}
    measurements = []
    for n, (i, j, lo, hi) in enumerate(pairs):
        mov, ref = crops.pop((i, n)), crops.pop((j, n))
        if float(ref.max() - ref.min()) == 0.0 or float(mov.max() - mov.min()) == 0.0:
            logger.info("stitch: pair (%s, %s) rejected: a featureless overlap", names[i], names[j])
            continue
        r = np.asarray(_phase_cross_corr(ref, mov, settings.maximum_shift), dtype=np.float64)
        if np.any(np.abs(r) >= settings.maximum_shift_voxels):
            logger.info("stitch: pair (%s, %s) rejected: shift %s reaches maximum_shift_voxels", names[i], names[j], r.tolist())
            continue
        measurements.append((i, j, (pos[j] - pos[i]).astype(np.float64) + r))
    t, kept, pinned = solve_placement(len(names), init, measurements, settings.outlier_threshold_voxels)
    paired = {k for i, j, _ in kept for k in (i, j)}
    for k in range(len(names)):
        if k not in paired and len(names) > 1:
            logger.warning("stitch: tile %s is left without a pair: it keeps its initial placement %s", names[k],
                           init[k].tolist())
    for k in pinned:
        if k in paired:
            logger.warning("stitch: no pair connects tile %s to tile %s: its group is placed from its own initial placement",
                           names[k], names[0])
    if settings.round_to_integer:
        t = _round_half_up(t).astype(np.float64)
    return {n: tuple(float(v) for v in t[k]) for k, n in enumerate(names)}
