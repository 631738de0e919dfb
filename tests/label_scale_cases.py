"""Shared case builders of the labelling tests AT SCALE, sized from the exported launch geometry
``G = (T, C, S, B, TB)`` (``lsr_label_launch_geometry``: threads per workgroup, voxels per numbering workgroup, threads of the
scan's one workgroup, the cap of the grid-stride launches, the cap of the local launch) and the tile of the local launch, so
that a changed cap moves the cases with it.  ``tests/label_cases.py`` stays below every one of these numbers; here every case
goes past one:

* ``scan_exact``         ``ceil(n / C) == S``: one count per scan thread, every scan thread busy.
* ``scan_plus_one``      ``ceil(n / C) == S + 1``: two counts per thread, thread ``S / 2`` holds one, every later one is idle.
* ``merge_wrap``         ``Z Y ceil(X / T) > B`` with one piece per row: the merge launch goes round its grid.
* ``merge_wrap_pieces``  the same with two pieces per row: the unit -> (row, piece) split past the wrap.
* ``voxel_wrap``         ``ceil(n / T) > B``: flatten, final, the table, the relabelling and the expansion go round.
* ``tile_wrap``          a column of ``TB + 2`` tiles: the local launch goes round (and the merge: one unit per voxel).

The noise cases are ``rng.random(shape, dtype=float32)`` with foreground ``value > 1 - p`` as ``label_cases``' ``noise_p*``,
with ``p`` BELOW the percolation threshold of the connectivity it is labelled with (``P``); the column's foreground is
``index % 11 < 7``: runs of 7 that start at every phase of the tile's z edge.

A hard rule: NO CASE HERE MAY HOLD A LONG COMPONENT (``MAX_COMPONENT``).  The device's ``find`` does not compress paths across a
launch: a foreground column or a solid volume of this size builds parent chains millions of links long that every thread of
``flatten`` walks.  ``tests/test_label_scale_host.py`` asserts the rule on the scipy reference and the GPU tests check it again
before they launch anything.

A case is ``dict(name, vol (float32), thresholds {connectivity: threshold}, connectivities)``.  The volumes and the references
are built once, on first use, and must not be modified.
"""

import functools

import numpy as np

from shrimpy_amd import segment as S
from tests import label_ref as R

G = S.launch_geometry()
T, C, S_, B, TB = G
TZ, TY, TX = S.tile_shape()

# foreground density per connectivity: below the site-percolation thresholds 0.3116 (6), 0.137 (18) and 0.0976 (26) of the cubic lattice
P = {6: 0.2, 18: 0.12, 26: 0.05}
MAX_COMPONENT = 4096
NOISE = ("scan_exact", "scan_plus_one", "merge_wrap", "merge_wrap_pieces", "voxel_wrap")
NAMES = NOISE + ("tile_wrap",)


def ceil_div(a, b):
    return -(-a // b)


def _round_up(a, m):
    return ceil_div(a, m) * m


def _shape_of_blocks(blocks, chunk, tile):
    """The first ``(z, y, x)`` -- z from 2 tz + 1, y from 4 ty + 6, x ascending -- with ``ceil(z y x / chunk) == blocks`` and no
    extent a multiple of its tile extent."""
    tz, ty, tx = tile
    for z in range(2 * tz + 1, 8 * tz):
        for y in range(4 * ty + 6, 8 * ty):
            if z % tz == 0 or y % ty == 0:
                continue
            for x in range(chunk * (blocks - 1) // (z * y) + 1, chunk * blocks // (z * y) + 1):
                if x % tx and ceil_div(z * y * x, chunk) == blocks:
                    return z, y, x
    raise AssertionError(f"no shape of {blocks} numbering blocks")


def shapes_for(geometry, tile):
    """name -> (z, y, x) for a launch geometry and a tile (``tests/watershed_scale_cases.py`` sizes its own from watershed.hip's);
    with (256, 4096, 1024, 2^16, 2^22) and a tile 4 deep: merge_wrap (33, 2000, 70), merge_wrap_pieces (2, 17000, 260),
    voxel_wrap (65, 2000, 130), tile_wrap (2^24 + 5, 1, 1)."""
    t, c, s, b, tb = geometry
    return {
        "scan_exact": _shape_of_blocks(s, c, tile),
        "scan_plus_one": _shape_of_blocks(s + 1, c, tile),
        # one piece per row (X < T), more rows than B
        "merge_wrap": (33, _round_up(ceil_div(b + 1, 33), 100), 70),
        # two pieces per row (T < X <= 2 T), more units than B
        "merge_wrap_pieces": (2, _round_up(ceil_div(b + 1, 2 * 2), 1000), t + 4),
        # more voxels than B workgroups of T threads hold
        "voxel_wrap": (65, _round_up(ceil_div(b * t + 1, 65 * 130), 100), 130),
        # TB + 2 tiles on top of one another, the last one partial
        "tile_wrap": (tile[0] * tb + 5, 1, 1),
    }


@functools.lru_cache(maxsize=None)
def shapes():
    return shapes_for(G, (TZ, TY, TX))


def shape(name):
    return shapes()[name]


def crossings(name):
    """What the launches of ``name`` come to: dict(n, blocks, per, units, pieces, voxel_groups, tiles)."""
    z, y, x = shape(name)
    n = z * y * x
    blocks = ceil_div(n, C)
    pieces = ceil_div(x, T)
    return dict(n=n, blocks=blocks, per=ceil_div(blocks, S_), units=z * y * pieces, pieces=pieces, voxel_groups=ceil_div(n, T),
                tiles=ceil_div(z, TZ) * ceil_div(y, TY) * ceil_div(x, TX))


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "tile_wrap":
        n = shape(name)[0]
        vol = (np.arange(n, dtype=np.int64) % 11 < 7).astype(np.float32).reshape(n, 1, 1)
        c = dict(name=name, vol=vol, thresholds={6: 0.5, 26: 0.5}, connectivities=(6, 26))
    else:
        rng = np.random.default_rng(2000 + NAMES.index(name))
        # values in (0, 1): foreground is value > 1 - p
        c = dict(name=name, vol=rng.random(shape(name), dtype=np.float32), thresholds={k: float(np.float32(1.0 - p)) for k, p in P.items()},
                 connectivities=(6, 18, 26))
    c["vol"].setflags(write=False)
    return c


PARAMS = [(name, k) for name in NAMES for k in ((6, 26) if name == "tile_wrap" else (6, 18, 26))]
PARAM_IDS = [f"{n}-{k}" for n, k in PARAMS]


@functools.lru_cache(maxsize=None)
def case_labels(name, connectivity):
    """``scipy.ndimage.label`` of a case, computed once and shared (read-only): ``(labels, n, voxels of the largest component)``."""
    c = case(name)
    labels, n = R.label(c["vol"], c["thresholds"][connectivity], connectivity)
    labels.setflags(write=False)
    return labels, n, int(np.bincount(labels.ravel())[1:].max())


def safe_labels(name, connectivity):
    """:func:`case_labels` of a case that keeps the rule: what every launch at scale asks for first."""
    labels, n, largest = case_labels(name, connectivity)
    assert 0 < largest < MAX_COMPONENT, f"{name}-{connectivity}: a component of {largest} voxels must not reach the device"
    return labels, n


# ---- synthetic labels on the voxel_wrap shape: the table, the filter and the expansion past the cap --------------------------------

N_SYNTHETIC = 52


@functools.lru_cache(maxsize=None)
def synthetic_labels():
    """``1 + (z // 5) * 4 + (y // 500)`` on the foreground of voxel_wrap's noise at p = 0.2, 0 elsewhere: 52 objects of about
    65 000 voxels in runs along x, so that the per-object loops of ``label_ref.table`` stay short.  The last of them (z >= 60)
    hold voxels on both sides of voxel ``B T``, where the launches begin their second trip.  (labels int32, 52), read-only."""
    c = case("voxel_wrap")
    z, y, x = np.indices(c["vol"].shape, dtype=np.int32, sparse=True)
    labels = np.where(c["vol"] > np.float32(c["thresholds"][6]), 1 + (z // 5) * 4 + (y // 500) + 0 * x, 0).astype(np.int32)
    labels.setflags(write=False)
    return labels, int(labels.max())


@functools.lru_cache(maxsize=None)
def synthetic_intensity():
    rng = np.random.default_rng(2999)
    out = (rng.standard_normal(shape("voxel_wrap"), dtype=np.float32) * np.float32(100.0)).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synthetic_table():
    """``label_ref.table`` of the synthetic labels with the synthetic intensities, once."""
    labels, n = synthetic_labels()
    return R.table(labels, n, synthetic_intensity())


PLAIN_KEYS = ("label", "volume", "bbox", "sum_zyx", "centroid")

# the expansion: every voxel's own index with x rounded down to a multiple of 3 as its `nearest`, so that the offsets are 0, 1
# and 2 voxels along x; under EXPAND_SAMPLING they measure 0, 0.75 and 1.5, and EXPAND_DISTANCE admits the first two
EXPAND_SAMPLING = (2.0, 0.5, 0.75)
EXPAND_DISTANCE = 1.0


@functools.lru_cache(maxsize=None)
def expand_nearest():
    zs, ys, xs = shape("voxel_wrap")
    z, y, x = np.indices((zs, ys, xs), dtype=np.int32, sparse=True)
    out = ((z * ys + y) * xs + (x - x % 3)).astype(np.int32)
    out.setflags(write=False)
    return out


def expand_restatement(labels, nearest, sampling, distance):
    """``lsr_label_expand_i32`` in float64 numpy: ``labels[nearest[v]]`` where the rule's distance from v to it is at most
    ``distance``, 0 elsewhere (``sqrt(((sz dz)^2 + (sy dy)^2) + (sx dx)^2)``, csrc/edt.hpp)."""
    zs, ys, xs = labels.shape
    z, y, x = np.indices(labels.shape, dtype=np.int64, sparse=True)
    site = nearest.astype(np.int64)
    dz, dy, dx = z - site // xs // ys, y - site // xs % ys, x - site % xs
    sz, sy, sx = (np.float64(v) for v in sampling)
    d = np.sqrt(((sz * dz) * (sz * dz) + (sy * dy) * (sy * dy)) + (sx * dx) * (sx * dx))
    return np.where((site >= 0) & (d <= np.float64(distance)), labels.ravel()[np.clip(site, 0, labels.size - 1)], 0).astype(np.int32)
