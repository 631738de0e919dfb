"""Oracles of the distance-transform tests.

* distances: ``scipy.ndimage.distance_transform_edt(mask, sampling=s).astype(float32)``; with no site anywhere the rule's own
  ``+inf`` (scipy measures from index -1 there);
* ``nearest``: a chunked numpy brute force over all sites, ``argmin`` taking the first of equals in raster order -- the smallest
  linear index (scipy's ``return_indices`` breaks ties another way), on the cases of at most ``edt_cases.BRUTE_VOXELS`` voxels;
* ``expand_labels`` restated from the brute-force ``nearest``.

Every result is computed once per (case, sampling, invert), shared and read-only.
"""

import functools

import numpy as np
import scipy.ndimage as ndi

from tests import edt_cases as C


def rule_distance(shape, nearest, sampling):
    """The rule's float64 distance from every voxel to ``nearest`` (linear indices; ``+inf`` where it is negative)."""
    z, y, x = np.indices(shape)
    n = np.where(nearest < 0, 0, nearest).astype(np.int64)
    nz, ny, nx = n // (shape[1] * shape[2]), n // shape[2] % shape[1], n % shape[2]
    sz, sy, sx = (np.float64(v) for v in sampling)
    a, b, c = sz * (z - nz), sy * (y - ny), sx * (x - nx)
    d = np.sqrt((a * a + b * b) + c * c)
    return np.where(nearest < 0, np.inf, d)


def edt(sites, sampling):
    """float32 distances to the nearest True voxel of ``sites``."""
    if not sites.any():
        return np.full(sites.shape, np.inf, dtype=np.float32)
    return ndi.distance_transform_edt(~sites, sampling=sampling).astype(np.float32)


def brute_nearest(sites, sampling, chunk=256):
    """int32 linear index of the nearest site, the smallest among equals; -1 everywhere without a site."""
    shape = sites.shape
    if not sites.any():
        return np.full(shape, -1, dtype=np.int32)
    pos = np.argwhere(sites).astype(np.int64)               # raster order
    lin = pos @ np.array([shape[1] * shape[2], shape[2], 1], dtype=np.int64)
    vox = np.argwhere(np.ones(shape, dtype=bool)).astype(np.int64)
    s = [np.float64(v) for v in sampling]
    out = np.empty(len(vox), dtype=np.int32)
    for lo in range(0, len(vox), chunk):
        d = vox[lo:lo + chunk, None, :] - pos[None, :, :]
        t = [s[a] * d[..., a] for a in range(3)]
        sq = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
        out[lo:lo + chunk] = lin[np.argmin(sq, axis=1)]     # the first of equals
    return out.reshape(shape)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case_edt(name, sampling, invert):
    return _frozen(edt(C.sites(name, invert), sampling))


@functools.lru_cache(maxsize=None)
def case_nearest(name, sampling, invert):
    assert C.case(name)["brute"], name
    return _frozen(brute_nearest(C.sites(name, invert), sampling))


def expand(labels, nearest, sampling, distance):
    """``expand_labels`` restated: the label of the nearest labelled voxel within ``distance``, 0 elsewhere."""
    d = rule_distance(labels.shape, nearest, sampling)
    taken = labels.ravel()[np.where(nearest < 0, 0, nearest)]
    return np.where((nearest >= 0) & (d <= distance), taken, 0).astype(np.int32)


def ulps(a, b):
    """The distance of two arrays of non-negative float32 in units in the last place (equal infinities: 0)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check(name, sampling, invert, dist, nearest):
    """The assertions every route shares (twin, kernels, profile entry): ``dist`` against scipy -- bit for bit under the exact
    samplings, within one float32 ulp otherwise, no voxel excluded --, ``nearest`` a site whose rule distance reproduces ``dist``
    exactly, and on the brute-force cases under the exact samplings ``nearest`` itself."""
    site = C.sites(name, invert)
    want = case_edt(name, sampling, invert)
    exact = sampling in C.EXACT
    worst = int(ulps(dist, want).max())
    print(f"{name} {sampling} invert={invert}: worst distance error {worst} ulp")
    if exact:
        assert dist.tobytes() == want.tobytes(), f"distances differ from scipy by up to {worst} ulp"
    else:
        assert worst <= 1, f"distances differ from scipy by up to {worst} ulp"
    if not site.any():
        assert np.all(nearest == -1) and np.all(np.isposinf(dist))
        return
    assert nearest.min() >= 0 and nearest.max() < site.size and np.all(site.ravel()[nearest]), "nearest is not a site"
    assert np.array_equal(nearest[site], np.flatnonzero(site)), "a site is not its own nearest"
    assert rule_distance(site.shape, nearest, sampling).astype(np.float32).tobytes() == dist.tobytes()
    if exact and C.case(name)["brute"]:
        assert np.array_equal(nearest, case_nearest(name, sampling, invert)), "the tie rule: smallest linear index"
