"""Shared case builders of the watershed tests AT SCALE.  ``csrc/watershed.hip`` compiles its own copy of the numbering launches
(flatten, count, scan, rank, final: ``label_uf.hpp``) into its own code object, so the shapes come from ITS exported launch
geometry (``lsr_watershed_launch_geometry``) through ``tests/label_scale_cases.py``'s formulas:

* ``merge_wrap``  ``ceil(n / C) > S``: the scan of this code object gives every thread two counts (connectivities 6 and 26).
* ``voxel_wrap``  ``ceil(n / T) > B``: flatten, final and ``watershed_saddles_kernel`` go round their grids (connectivity 6).

``surface`` is standard normal float32: an ascent in white noise ends after a few steps, so NO BASIN IS LONG
(``MAX_BASIN``; the rule of ``label_scale_cases`` and its reason hold here, and the ``ties``, ``constant``, ``inf`` and
``serpentine`` surfaces of ``watershed_cases`` have no place at this size).  ``objects`` is ``watershed_cases``' "bernoulli":
scipy's labelling at connectivity 6 of ``random < 0.7``, half of the rest set to -1.

Not crossed here: ``watershed_local_kernel``'s tile wrap needs a column of ``8 * 2^22`` voxels and ``watershed_merge_kernel``'s
wrap ``n > 2^26``: tens of millions of voxels under a slow reference.  Their loops have the form of the labelling's, which
``tests/test_label_scale_gpu.py`` pins.

A case is ``dict(name, objects (int32), surface (float32))``, built once on first use and read-only.
"""

import functools

import numpy as np
from scipy import ndimage

from shrimpy_amd import watershed as W
from tests import label_scale_cases as LC
from tests import watershed_ref as R

G = W.launch_geometry()
T, C, S_, B, TB = G
TILE = W.tile_shape()
MAX_BASIN = 4096
NAMES = ("merge_wrap", "voxel_wrap")
PARAMS = [("merge_wrap", 6), ("merge_wrap", 26), ("voxel_wrap", 6)]
PARAM_IDS = [f"{n}-{k}" for n, k in PARAMS]


@functools.lru_cache(maxsize=None)
def shapes():
    every = LC.shapes_for(G, TILE)
    return {name: every[name] for name in NAMES}


def shape(name):
    return shapes()[name]


def crossings(name):
    """dict(n, blocks, per, voxel_groups, merge_groups, tiles) of the launches of ``name``."""
    z, y, x = shape(name)
    n = z * y * x
    blocks = LC.ceil_div(n, C)
    return dict(n=n, blocks=blocks, per=LC.ceil_div(blocks, S_), voxel_groups=LC.ceil_div(n, T), merge_groups=LC.ceil_div(LC.ceil_div(n, 4), T),
                tiles=LC.ceil_div(z, TILE[0]) * LC.ceil_div(y, TILE[1]) * LC.ceil_div(x, TILE[2]))


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(3000 + NAMES.index(name))
    s = shape(name)
    surface = rng.standard_normal(s, dtype=np.float32)
    labels, _ = ndimage.label(rng.random(s) < 0.7)                        # scipy's default structure: connectivity 6
    objects = labels.astype(np.int32)
    objects[(objects == 0) & (rng.random(s) < 0.5)] = -1
    c = dict(name=name, surface=np.ascontiguousarray(surface), objects=np.ascontiguousarray(objects))
    c["surface"].setflags(write=False)
    c["objects"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case_basins(name, connectivity):
    """The numpy restatement of a case, computed once and shared (read-only): ``(basins, B, summits, voxels of the largest basin)``."""
    c = case(name)
    labels, count, summits = R.basins(c["objects"], c["surface"], connectivity)
    labels.setflags(write=False)
    return labels, count, summits, int(np.bincount(labels.ravel())[1:].max())


def safe_basins(name, connectivity):
    """:func:`case_basins` of a case that keeps the rule: what every launch at scale asks for first."""
    labels, count, summits, largest = case_basins(name, connectivity)
    assert 0 < largest < MAX_BASIN, f"{name}-{connectivity}: a basin of {largest} voxels must not reach the device"
    return labels, count, summits


@functools.lru_cache(maxsize=None)
def case_saddles(name, connectivity):
    c = case(name)
    return R.saddles(c["objects"], case_basins(name, connectivity)[0], c["surface"], connectivity)
