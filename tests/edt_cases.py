"""Shared case builders of the distance-transform tests, sized from the exported tiling (``lsr_edt_tiling``): the 64-voxel step
of the x pass, the 256 lines a workgroup of the y and z passes takes, and the rows and lines beyond which a wave or a lane takes
a second one.

A case is ``dict(name, vol (float32), threshold, brute)``: the foreground is ``vol > threshold``, the sites are the background
(``invert = False``) or the foreground (``invert = True``); ``brute`` says that the case is small enough for the brute-force
oracle of ``nearest``.  ``PARAMS`` lists ``(name, sampling, invert)``.  The volumes are built once and must not be modified.
"""

import functools
import itertools

import numpy as np

from shrimpy_amd import distance as D

CHUNK, TILE, ROWS_AT_ONCE, LINES_AT_ONCE = D.tiling()

EXACT = ((1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (1.5, 0.5, 0.25))     # every cost is exact in float64
INEXACT = (0.4, 0.116, 0.116)
SAMPLINGS = EXACT + (INEXACT,)
BRUTE_VOXELS = 8000
X_EXTENTS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7)
LINE_EXTENTS = (1, 2, TILE + 1)


def _f(foreground):
    return np.ascontiguousarray(foreground, dtype=np.float32)


def _noise(shape, p, seed):
    """Bernoulli foreground at ``p`` as values in (0, 1) against the threshold 1 - p: the mask is not the data."""
    rng = np.random.default_rng(seed)
    return rng.random(shape, dtype=np.float32), float(np.float32(1.0 - p))


def _corner(shape, corner):
    fg = np.ones(shape, dtype=bool)
    fg[tuple(-c for c in corner)] = False                  # (index 0 or -1 on every axis)
    return fg


def _threshold_semantics(shape):
    tiny = np.float32(1e-45)        # the smallest subnormal
    vals = np.array([0.0, np.nan, -np.nan, np.inf, -np.inf, -0.0, tiny, -tiny, 1.0, -1.0, 2.0], dtype=np.float32)
    return vals[np.random.default_rng(77).integers(0, len(vals), size=shape)]


@functools.lru_cache(maxsize=None)
def _all():
    small = (5, 9, CHUNK + 6)
    cases = []
    for k, x in enumerate(X_EXTENTS):
        vol, thr = _noise((3, 5, x), 0.9, 100 + k)
        cases.append(dict(name=f"extent_x{x}", vol=vol, threshold=thr))
    for k, y in enumerate(LINE_EXTENTS):
        vol, thr = _noise((2, y, CHUNK + 6), 0.97, 200 + k)
        cases.append(dict(name=f"extent_y{y}", vol=vol, threshold=thr))
    for k, z in enumerate(LINE_EXTENTS):
        vol, thr = _noise((z, 3, CHUNK + 6), 0.97, 300 + k)
        cases.append(dict(name=f"extent_z{z}", vol=vol, threshold=thr))
    cases.append(dict(name="single_site", vol=_f(np.zeros((1, 1, 1))), threshold=0.5))
    cases.append(dict(name="all_sites", vol=_f(np.zeros((3, 9, CHUNK + 6))), threshold=0.5))
    for corner in itertools.product((0, 1), repeat=3):     # one site: pure geometry, the longest distances, empty lines and planes
        cases.append(dict(name="corner_" + "".join(map(str, corner)), vol=_f(_corner(small, corner)), threshold=0.5))
    cases.append(dict(name="no_site", vol=_f(np.ones(small)), threshold=0.5))
    plane = np.ones(small, dtype=bool)
    plane[2] = np.random.default_rng(5).random(small[1:]) < 0.5
    cases.append(dict(name="one_plane", vol=_f(plane), threshold=0.5))
    row = np.ones(small, dtype=bool)
    row[1, 4] = np.random.default_rng(6).random(small[2]) < 0.7
    cases.append(dict(name="one_row", vol=_f(row), threshold=0.5))
    for k, p in enumerate((0.5, 0.9, 0.99)):               # (6, 19, 70): more lines than one workgroup takes, in both passes
        vol, thr = _noise((6, 19, CHUNK + 6), p, 400 + k)
        cases.append(dict(name=f"noise_p{p}", vol=vol, threshold=thr))
    cases.append(dict(name="checkerboard", vol=_f(np.indices((5, 9, CHUNK + 3)).sum(axis=0) % 2 == 0), threshold=0.5))
    mirror = np.ones((5, 9, CHUNK + 1), dtype=bool)         # odd extents, a site in every corner: the middle planes tie
    for corner in itertools.product((0, -1), repeat=3):
        mirror[corner] = False
    cases.append(dict(name="mirror_corners", vol=_f(mirror), threshold=0.5))
    pairs = np.ones((3, 7, CHUNK + 1), dtype=bool)          # pairs of sites mirrored about the middle of every row
    pairs[:, :, 3] = pairs[:, :, -4] = False
    cases.append(dict(name="mirror_pairs", vol=_f(pairs), threshold=0.5))
    cases.append(dict(name="threshold_semantics", vol=_threshold_semantics((3, 7, CHUNK + 5)), threshold=0.0))
    # more rows than the x pass holds at once, more lines than the y pass and the z pass hold at once
    vol, thr = _noise((3, ROWS_AT_ONCE // 3 + 11, 2), 0.9, 500)
    cases.append(dict(name="second_rows", vol=vol, threshold=thr, samplings=((1.0, 1.0, 1.0), INEXACT)))
    vol, thr = _noise((1, 2, LINES_AT_ONCE + CHUNK + 6), 0.9, 501)
    cases.append(dict(name="second_lines_y", vol=vol, threshold=thr, samplings=((1.0, 1.0, 1.0), INEXACT)))
    vol, thr = _noise((2, 1, LINES_AT_ONCE + CHUNK + 6), 0.9, 502)
    cases.append(dict(name="second_lines_z", vol=vol, threshold=thr, samplings=((1.0, 1.0, 1.0), INEXACT)))
    for c in cases:
        c.setdefault("samplings", SAMPLINGS)
        c["brute"] = c["vol"].size <= BRUTE_VOXELS
        c["vol"].setflags(write=False)
    return tuple(cases)


CASES = _all()
NAMES = [c["name"] for c in CASES]
INVERTED = ("noise_p0.5", "checkerboard", "threshold_semantics", "one_row", "no_site", "all_sites")
PARAMS = [(c["name"], s, False) for c in CASES for s in c["samplings"]] + \
         [(n, s, True) for n in INVERTED for s in ((1.5, 0.5, 0.25), INEXACT)]
PARAM_IDS = [f"{n}-{'x'.join(f'{v:g}' for v in s)}{'-inverted' if inv else ''}" for n, s, inv in PARAMS]


def case(name):
    return CASES[NAMES.index(name)]


def sites(name, invert):
    """The boolean site mask of a case: the background of ``vol > threshold``, with ``invert`` the foreground."""
    c = case(name)
    with np.errstate(invalid="ignore"):
        fg = c["vol"] > np.float32(c["threshold"])
    return fg if invert else ~fg


def label_volume(name):
    """An int32 label volume for the entries that take one: the case's foreground, numbered 1 .. 5 by position."""
    fg = sites(name, True)
    idx = np.arange(fg.size, dtype=np.int64).reshape(fg.shape)
    return np.where(fg, 1 + idx % 5, 0).astype(np.int32)
