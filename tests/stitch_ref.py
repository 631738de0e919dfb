"""Float64 restatement of the stitching rule (``shrimpy_amd/stitch.py``, ``csrc/stitch.hpp``) -- the oracle of
tests/test_stitch_host.py and tests/test_stitch_gpu.py, and the cases and fixtures the two share; nothing here is imported
by the package.  biahub is not installed:
PARITY IS UNPINNED, the rule is the package's own and this file states it a second time, in NumPy float64.

Tile voxel ``i`` of tile ``k`` sits at canvas coordinate ``i + t_k``.  Per tile and axis ``ti = floor(t)``, ``tf = t - ti``,
``j = c - ti`` for the absolute canvas index ``c``; ``tf == 0``: tap ``j``, covered iff ``0 <= j <= n - 1``; else taps ``j - 1``
and ``j`` with weights ``tf`` and ``1 - tf``, covered iff ``1 <= j <= n - 1``.  Sample: interpolation over the fractional axes
only.  Weight ``(dy dx)^p``, ``d = min(l + 1, n - l)``, ``l = c - t``.  Output: ``cval`` (no tile), the sample (one tile),
``sum(w s) / sum(w)`` (several).

The a-priori bound of the float32 result (``bound_f32``), from the operation count of ``csrc/stitch.hpp``.  Write
``u = 2^-24`` and ``gamma(m) = m u / (1 - m u)``: a product of ``m`` factors ``(1 + d)^(+-1)``, ``|d| <= u``, differs from 1
by at most ``gamma(m)`` (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  Every float32 operation below
is one such factor on each term it touches; all weights are positive, so factors on the terms of a sum stay per term.

* Sample.  Per fractional axis ``lerp = fl(fl(w0 a0) + fl(w1 a1))`` with ``w0 = fl(tf)``, ``w1 = fl(1 - tf)``: each tile voxel
  that enters picks up 3 factors (its weight's rounding, the product, the sum).  With ``f`` fractional axes: ``3 f`` factors, so
  ``|s~ - s| <= gamma(3 f) a``, ``a`` the same interpolation of ``|v|``.  ``f = 0``: the voxel itself, exact.
* Weight.  ``d = min(fl(float(j) + w1), fl(float(n - j) + w0))``: the conversion (exact below 2^24), the weight's rounding and
  the sum are 3 factors on a sum of two non-negative terms -- no cancellation -- and taking the float32 minimum of two such
  values is within the same factors of the exact minimum.  ``dy dx``: 3 + 3 + 1 = 7 factors; ``(dy dx)^p`` by ``p - 1`` further
  products (``1 * b`` is exact): ``E = 8 p - 1`` factors for ``p >= 1``, none for ``p = 0`` (``w = 1``).
* Blend of ``n >= 2`` tiles.  Numerator term ``k``: ``3 f + E`` factors from ``s~`` and ``w~``, one from the product, at most
  ``n - 1`` from the sums: ``3 f + E + n``.  Denominator: ``E + (n - 1)`` factors on every term, all positive, so on the sum.  The
  division: 1.  Each tile voxel's contribution to the result is therefore multiplied by at most
  ``M = (3 f + E + n) + (E + n - 1) + 1 = 3 f + 2 E + 2 n`` factors:
  ``|out~ - out| <= gamma(3 f + 2 E + 2 n) * sum(w_k a_k) / sum(w_k)`` -- the form ``(c0 + c1 n_cover) 2^-24 sum(w |s|) / sum(w)``
  with ``c0 = 3 f + 2 E``, ``c1 = 2``, ``|s_k|`` read as the interpolation of ``|v|`` (equal to ``|s_k|`` at integer placement)
  and ``f`` the largest count of fractional axes among the covering tiles.
* One tile: ``gamma(3 f) a``; none: ``cval`` exactly.
"""

from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


def split(t):
    ti = np.floor(np.asarray(t, dtype=np.float64))
    return ti.astype(np.int64), np.asarray(t, dtype=np.float64) - ti


def canvas_geometry(shapes, translations):
    shp = np.asarray(shapes, dtype=np.float64).reshape(-1, 3)
    tr = np.asarray(translations, dtype=np.float64).reshape(-1, 3)
    origin = np.floor(tr.min(axis=0)).astype(np.int64)
    shape = np.ceil((tr + shp).max(axis=0)).astype(np.int64) - origin
    return tuple(int(v) for v in shape), tuple(int(v) for v in origin)


def _axis(v, axis, j, tf):
    """``v`` resampled along ``axis`` at the indices ``j`` (clipped: uncovered ones are masked by the caller)."""
    n = v.shape[axis]
    v1 = np.take(v, np.clip(j, 0, n - 1), axis=axis)
    if tf == 0.0:
        return v1
    return tf * np.take(v, np.clip(j - 1, 0, n - 1), axis=axis) + (1.0 - tf) * v1


def stitch_f64(tiles, translations, p: int, cval: float, box=None):
    """``(out, bound, n_cover)`` over the box (default: the whole canvas), all float64 / int arrays of the box's shape."""
    shapes = [t.shape for t in tiles]
    if box is None:
        shape, origin = canvas_geometry(shapes, translations)
    else:
        origin, shape = tuple(box[0]), tuple(box[1])
    num, den, nabs, single = (np.zeros(shape) for _ in range(4))
    single_abs = np.zeros(shape)
    n_cover = np.zeros(shape, dtype=np.int64)
    f_max = np.zeros(shape, dtype=np.int64)
    for tile, t in zip(tiles, translations):
        ti, tf = split(t)
        v = np.asarray(tile, dtype=np.float64)
        a = np.abs(v)
        cov, dist = [], []
        for ax in (2, 1, 0):                                   # x, then y, then z
            c = origin[ax] + np.arange(shape[ax], dtype=np.int64)
            j = c - ti[ax]
            n = tile.shape[ax]
            v, a = _axis(v, ax, j, tf[ax]), _axis(a, ax, j, tf[ax])
            cov.append((j >= (1 if tf[ax] != 0.0 else 0)) & (j <= n - 1))
            l = c.astype(np.float64) - float(t[ax])
            dist.append(np.minimum(l + 1.0, n - l))
        cx, cy, cz = cov
        covered = cz[:, None, None] & cy[None, :, None] & cx[None, None, :]
        w = np.broadcast_to((dist[1][None, :, None] * dist[0][None, None, :]) ** int(p), shape)
        with np.errstate(invalid="ignore"):
            num += np.where(covered, w * v, 0.0)
            single += np.where(covered, v, 0.0)
        den += np.where(covered, w, 0.0)
        nabs += np.where(covered, w * a, 0.0)
        single_abs += np.where(covered, a, 0.0)
        n_cover += covered
        f_max = np.maximum(f_max, np.where(covered, int(np.count_nonzero(tf)), 0))
    e = 8 * int(p) - 1 if p >= 1 else 0
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(n_cover == 0, float(cval), np.where(n_cover == 1, single, num / den))
        bound = np.where(n_cover == 0, 0.0, np.where(n_cover == 1, gamma(3 * f_max) * single_abs,
                                                    gamma(3 * f_max + 2 * e + 2 * n_cover) * nabs / den))
    return out, bound, n_cover


def bound_f32(tiles, translations, p: int, box=None):
    return stitch_f64(tiles, translations, p, 0.0, box)[1]


def f32_tile(shape, seed: int) -> np.ndarray:
    """100 N(0, 1) + 50: mixed sign."""
    rng = np.random.default_rng(seed)
    return (100.0 * rng.standard_normal(shape) + 50.0).astype(np.float32)


def make_case(case: dict):
    """``(tiles, translations)`` of a case: float32 arrays, seeded by the case's position-independent content."""
    tiles = [f32_tile(s, seed=1000 * k + sum(s)) for k, s in enumerate(case["shapes"])]
    return tiles, [tuple(float(v) for v in t) for t in case["translations"]]


def _case(name, shapes, translations, p, cval=-7.5, box=None):
    return {"name": name, "shapes": [tuple(s) for s in shapes], "translations": [tuple(t) for t in translations], "p": p,
            "cval": cval, "box": box}


LONG = (2, 3, 4099)      # an odd X: the row starts fall on every 4-byte phase of a 16-byte line
CASES = [
    # tiles of different shapes, a single voxel among them, rows that span workgroups (1030 > 1024 voxels per run)
    _case("three_shapes", [(3, 5, 7), (1, 1, 1), (2, 6, 1030)], [(0, 0, 0), (1, 2, 3), (1, 3, -20)], 1),
    _case("phase0", [LONG, LONG], [(0, 0, 0), (0, 1, 0)], 1),
    _case("phase1", [LONG, LONG], [(0, 0, 0), (0, 1, 1)], 1),
    _case("phase2", [LONG, LONG], [(0, 0, 0), (0, 1, 2)], 0),
    _case("phase3", [LONG, LONG], [(0, 0, 0), (1, 1, 3)], 4),
    # ... and the five-float reads of a fractional x placement at every phase (rows 4099 floats apart: phases 0, 3, 2, 1)
    _case("phase_frac_x", [LONG, LONG], [(0, 0, 0), (0, 1, 2.5)], 1),
    _case("negative", [(3, 5, 7), (3, 5, 7)], [(-2, -3, -5), (-1, -1, -1)], 0),
    _case("frac_x", [(2, 6, 1030), (2, 6, 1030)], [(0, 0, 0), (0, 3, 500.5)], 1),
    _case("frac_y", [(3, 6, 40), (3, 6, 40)], [(0, 0, 0), (0, 2.25, 30)], 1),
    _case("frac_z", [(3, 6, 40), (3, 6, 40)], [(0, 0, 0), (0.75, 2, 30)], 4),
    _case("frac_zyx", [(3, 6, 40), (3, 7, 1100)], [(0, 0.5, 0.125), (0.5, 2.25, 17.75)], 1),
    _case("five_cover", [(2, 8, 9)] * 5, [(0, 0, 0), (0, 1, 2), (0, 2, 1), (1, 3, 3), (0, 0.5, 1.5)], 4),
    _case("inside", [(4, 10, 20), (2, 3, 5)], [(0, 0, 0), (1, 4, 6)], 1),
    # a strict sub-box of the canvas, with the third tile wholly outside it
    _case("sub_box", [(3, 8, 40), (3, 8, 40), (2, 2, 2)], [(0, 0, 0), (0, 4, 30), (0, 20, 100)], 1,
          box=((1, 2, 5), (2, 7, 50))),
    _case("single_p0", [(1, 1, 1)], [(5, -6, 7)], 0),
]
GPU_CASES = CASES


# ---- a scene cut into tiles, for the placement estimate ------------------------------------------------------------------


def scene(shape, seed: int) -> np.ndarray:
    """Smooth blobs plus noise: the noise belongs to the scene, so two tiles see the same texture where they overlap.  The
    correlation of ``dynatrack._phase_cross_corr`` is not normalised, so broad blobs alone pull its peak towards zero shift
    in a 16-voxel overlap; the voxel-scale texture (sigma 25 against blobs of 20 .. 60) is what pins it."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    vol = np.zeros(shape)
    for _ in range(40):
        c = rng.uniform(0, 1, 3) * np.asarray(shape)
        s = rng.uniform(2.0, 5.0)
        vol += rng.uniform(20, 60) * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    return (vol + 100.0 + 25.0 * rng.standard_normal(shape)).astype(np.float32)


def grid_tiles(rows: int, cols: int, seed: int, tile=(12, 56, 56), step=40, jitter=3):
    """``(names, tiles, nominal, true)``: a ``rows x cols`` grid of tiles cut from one scene at the nominal grid positions
    ``(1, r * step + jitter, c * step + jitter)`` moved by integer jitters of up to ``+-jitter`` in y and x and ``+-1`` in z."""
    rng = np.random.default_rng(seed)
    shape = (tile[0] + 2, (rows - 1) * step + tile[1] + 2 * jitter, (cols - 1) * step + tile[2] + 2 * jitter)
    vol = scene(shape, seed)
    names, tiles, nominal, true = [], {}, {}, {}
    for r in range(rows):
        for c in range(cols):
            name = f"A/1/{r * cols + c:03d}"
            nom = np.array([1, r * step + jitter, c * step + jitter], dtype=np.int64)
            off = nom + np.array([rng.integers(-1, 2), rng.integers(-jitter, jitter + 1), rng.integers(-jitter, jitter + 1)])
            names.append(name)
            nominal[name] = tuple(float(v) for v in nom)
            true[name] = tuple(int(v) for v in off)
            tiles[name] = np.ascontiguousarray(vol[off[0]:off[0] + tile[0], off[1]:off[1] + tile[1], off[2]:off[2] + tile[2]])
    return names, tiles, nominal, true


# ---- shared by the host and the device tests -------------------------------------------------------------------------------

ESTIMATE = dict(channel="GFP", maximum_shift_voxels=10, min_overlap_voxels=8, outlier_threshold_voxels=1.5)


@functools.lru_cache(maxsize=None)
def grid(rows, cols):
    """``grid_tiles`` of a ``rows x cols`` grid, cut once."""
    return grid_tiles(rows, cols, seed=7 * rows + cols)


@functools.lru_cache(maxsize=None)
def twin_case(index):
    """``(tiles, translations, host twin's output)`` of ``CASES[index]``, computed once and read-only."""
    import torch

    from shrimpy_amd import stitch as S

    case = CASES[index]
    tiles, tr = make_case(case)
    got = S.stitch_tiles([torch.from_numpy(a) for a in tiles], tr, case["p"], case["cval"], box=case["box"]).numpy()
    for a in tiles + [got]:
        a.setflags(write=False)
    return tiles, tr, got
