"""Shared case builders of the watershed tests, sized from the exported tile ``(tz, ty, tx)`` of the local launch
(``lsr_watershed_tile_shape``) so that every face and every partial tile is crossed.  Every case is a few ten thousand voxels.

A case is ``dict(name, objects (int32), surface (float32))``: the cross of four shapes, six surfaces and four object volumes.
``CASES`` lists them, ``case(name)`` finds one.  The arrays are built once and must not be modified.
"""

import functools

import numpy as np
from scipy import ndimage

from shrimpy_amd import watershed as W

CONNECTIVITIES = (6, 18, 26)
T = W.tile_shape()
TZ, TY, TX = T

SHAPES = {"one": (1, 1, 1), "row": (1, 1, 3 * TX + 5), "tile+1": (TZ + 1, TY + 1, TX + 1), "tiles": (2 * TZ + 1, TY + 2, 2 * TX + 3)}
SURFACES = ("random", "ties", "constant", "inf", "zeros", "serpentine")
OBJECTS = ("solid", "bernoulli", "diagonal", "background")


def serpentine_path(shape):
    """The voxels of a one-voxel-wide path through ``shape``, in order: along x on the even rows of an even plane (turning through
    one voxel of the odd row at the row's end), through one voxel of the odd plane at the plane's end, and back the same way on
    the next even plane.  Under connectivity 6 a voxel of the path touches no other voxel of it than the one before and the one
    behind; under 18 and 26 a turn can be cut by one step."""
    Z, Y, X = shape
    plane = []
    for k, y in enumerate(range(0, Y, 2)):
        xs = list(range(X)) if k % 2 == 0 else list(range(X - 1, -1, -1))
        plane += [(y, x) for x in xs]
        if y + 2 < Y:
            plane.append((y + 1, xs[-1]))
    path = []
    for k, z in enumerate(range(0, Z, 2)):
        walk = plane if k % 2 == 0 else plane[::-1]
        path += [(z, y, x) for y, x in walk]
        if z + 2 < Z:
            path.append((z + 1, *walk[-1]))
    return path


def _surface(kind, shape, rng):
    if kind == "random":
        return rng.standard_normal(shape).astype(np.float32)                     # no ties worth speaking of
    if kind == "ties":
        return rng.integers(0, 3, size=shape).astype(np.float32)                 # ties everywhere: the index rule
    if kind == "constant":
        return np.full(shape, 1.5, dtype=np.float32)
    if kind == "inf":
        return np.full(shape, np.inf, dtype=np.float32)
    if kind == "zeros":
        return np.where(rng.random(shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    # a ramp along the serpentine, -1 off it: from the path's start the ascent walks the whole path, across every tile face
    out = np.full(shape, -1.0, dtype=np.float32)
    for k, p in enumerate(serpentine_path(shape)):
        out[p] = k
    return out


def _objects(kind, shape, rng):
    if kind == "solid":
        return np.ones(shape, dtype=np.int32)
    if kind == "background":
        return np.where(rng.random(shape) < 0.5, 0, -3).astype(np.int32)          # (every value <= 0 is background)
    if kind == "bernoulli":
        labels, _ = ndimage.label(rng.random(shape) < 0.7)                        # scipy's default structure: connectivity 6
        labels = labels.astype(np.int32)
        labels[(labels == 0) & (rng.random(shape) < 0.5)] = -1
        return labels
    # two blocks that share no face: they touch along an edge or at a corner only (one block where an extent is 1)
    h = tuple((n + 1) // 2 for n in shape)
    out = np.zeros(shape, dtype=np.int32)
    out[:h[0], :h[1], :h[2]] = 1
    out[h[0]:, h[1]:, h[2]:] = 2
    return out


@functools.lru_cache(maxsize=None)
def _all():
    cases = []
    for si, (sname, shape) in enumerate(SHAPES.items()):
        for fi, fname in enumerate(SURFACES):
            for oi, oname in enumerate(OBJECTS):
                rng = np.random.default_rng(10000 + 100 * si + 10 * fi + oi)
                c = dict(name=f"{sname}-{fname}-{oname}", shape_name=sname, surface_name=fname, objects_name=oname,
                         surface=np.ascontiguousarray(_surface(fname, shape, rng)),
                         objects=np.ascontiguousarray(_objects(oname, shape, rng)))
                c["surface"].setflags(write=False)
                c["objects"].setflags(write=False)
                cases.append(c)
    return tuple(cases)


CASES = _all()
NAMES = [c["name"] for c in CASES]
PARAMS = [(c["name"], k) for c in CASES for k in CONNECTIVITIES]
PARAM_IDS = [f"{n}-{k}" for n, k in PARAMS]
# the saddles, the merge and the relabelling: the two shapes with more than one tile, every surface, the objects with voxels
GRAPH_PARAMS = [(c["name"], k) for c in CASES for k in CONNECTIVITIES
                if c["shape_name"] in ("row", "tiles") and c["objects_name"] != "background"]
GRAPH_IDS = [f"{n}-{k}" for n, k in GRAPH_PARAMS]
TIE_HEAVY = "tiles-ties-solid"


def case(name):
    return CASES[NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def touching_balls():
    """Two balls of radius 10 with centres 18 apart, one object: ``objects`` (int32), read-only."""
    z, y, x = np.indices((25, 25, 43))
    mask = ((z - 12) ** 2 + (y - 12) ** 2 + (x - 12) ** 2 <= 100) | ((z - 12) ** 2 + (y - 12) ** 2 + (x - 30) ** 2 <= 100)
    out = mask.astype(np.int32)
    out.setflags(write=False)
    return out
