"""Shared case builders of the labelling tests, sized from the exported tile ``t = (tz, ty, tx)`` of the local launch
(``lsr_label_tile_shape``) so that they aim at its faces.  Every case is a few hundred thousand voxels at most.

A case is ``dict(name, vol (float32), threshold, connectivities)``; ``CASES`` lists them, ``case(name)`` finds one.  The
volumes are built once and must not be modified.
"""

import functools
import itertools

import numpy as np

from shrimpy_amd import segment as S

CONNECTIVITIES = (6, 18, 26)
T = S.tile_shape()
TZ, TY, TX = T

# the 13 neighbour directions whose first non-zero component is positive
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]
assert len(DIRECTIONS) == 13


def _f(mask):
    return np.ascontiguousarray(mask, dtype=np.float32)


def _runs(n):
    """Alternating foreground / background runs of lengths 1, 2, 3, ... along ``n`` voxels, foreground first."""
    out, pos, k = np.zeros(n, dtype=bool), 0, 1
    while pos < n:
        out[pos:pos + k] = (k % 2 == 1)
        pos, k = pos + k, k + 1
    return out


def _straddle_pair(d):
    """Two voxels a, a + d on a 2 x 2 x 2 arrangement of tiles, on different sides of the tile boundary along every axis on which
    d moves, and hard against the boundary on the others."""
    vol = np.zeros((2 * TZ, 2 * TY, 2 * TX), dtype=bool)
    a = tuple(t - 1 if c >= 0 else t for t, c in zip(T, d))
    vol[a] = True
    vol[tuple(p + c for p, c in zip(a, d))] = True
    return vol


def _corner_chain(d):
    """Three voxels c - d, c, c + d through the corner the eight tiles share (d a body diagonal)."""
    vol = np.zeros((2 * TZ, 2 * TY, 2 * TX), dtype=bool)
    c = tuple(t if s > 0 else t - 1 for t, s in zip(T, d))
    for k in (-1, 0, 1):
        vol[tuple(p + k * s for p, s in zip(c, d))] = True
    return vol


def _mixed_chain():
    """Across the common corner by a face step, then an edge step: 2 objects under 6, 1 under 18 and 26."""
    vol = np.zeros((2 * TZ, 2 * TY, 2 * TX), dtype=bool)
    vol[TZ - 1, TY - 1, TX - 1] = vol[TZ - 1, TY - 1, TX] = vol[TZ, TY, TX] = True
    return vol


def _serpentine():
    """A one-voxel-wide path through (3, 2 ty + 3, 2 tx + 5): along x on the even rows of plane 0, turning at the row ends, up
    through one voxel of plane 1 at the plane's end, and back the same way on plane 2.  One component under every
    connectivity; planes 0 and 2 are half path, plane 1 is the turn (the path is a third of the volume)."""
    Z, Y, X = 3, 2 * TY + 3, 2 * TX + 5
    plane = np.zeros((Y, X), dtype=bool)
    plane[0::2, :] = True
    for k, y in enumerate(range(1, Y, 2)):
        plane[y, X - 1 if k % 2 == 0 else 0] = True
    vol = np.zeros((Z, Y, X), dtype=bool)
    vol[0] = vol[2] = plane
    last_row = Y - 1                                    # (Y is odd: the last row is a path row)
    n_turns = len(range(1, Y, 2))
    end_x = 0 if n_turns % 2 == 1 else X - 1            # where the path leaves the last row
    vol[1, last_row, end_x] = True
    return vol


def _nested_us():
    """U shapes open towards low x: two arms along x in different tiles, joined only by a bar at their high-x end, nested three
    voxels apart.  The root of each (the first voxel of its upper arm) is far from where the arms are found equal."""
    Y, X = 2 * TY + 3, 2 * TX + 5
    vol = np.zeros((1, Y, X), dtype=bool)
    for k in range(4):
        lo, hi, bar = 3 * k, Y - 1 - 3 * k, X - 1 - 3 * k
        vol[0, lo, 3 * k:bar + 1] = vol[0, hi, 3 * k:bar + 1] = True
        vol[0, lo:hi + 1, bar] = True
    return vol


def _nested_vs():
    """... and open towards low y: the arms run along y and meet on a bar at their high-y end."""
    Y, X = 2 * TY + 3, 2 * TX + 5
    vol = np.zeros((1, Y, X), dtype=bool)
    for k in range(4):
        lo, hi, bar = 3 * k, X - 1 - 3 * k, Y - 1 - 3 * k
        vol[0, 3 * k:bar + 1, lo] = vol[0, 3 * k:bar + 1, hi] = True
        vol[0, bar, lo:hi + 1] = True
    return vol


def _spiral():
    """A square spiral, one voxel wide with one voxel between its turns, over (3 ty + 2, 3 tx + 2): more than 3 x 3 tiles.
    Walked from the outside: straight on while the voxel ahead is free and the one behind it is too, else a right turn."""
    Y, X = 3 * TY + 2, 3 * TX + 2
    seen = np.zeros((Y, X), dtype=bool)

    def free(y, x, dy, dx):
        ahead, beyond = (y + dy, x + dx), (y + 2 * dy, x + 2 * dx)
        if not (0 <= ahead[0] < Y and 0 <= ahead[1] < X) or seen[ahead]:
            return False
        return not (0 <= beyond[0] < Y and 0 <= beyond[1] < X and seen[beyond])

    turns, k, y, x = ((0, 1), (1, 0), (0, -1), (-1, 0)), 0, 0, 0
    seen[0, 0] = True
    while True:
        if not free(y, x, *turns[k]):
            k = (k + 1) % 4
            if not free(y, x, *turns[k]):
                break
        y, x = y + turns[k][0], x + turns[k][1]
        seen[y, x] = True
    return seen[None]


def _comb():
    """Teeth on every other column, joined only by a spine on the LAST row."""
    Y, X = 2 * TY + 3, 2 * TX + 5
    vol = np.zeros((1, Y, X), dtype=bool)
    vol[0, :, 0::2] = True
    vol[0, Y - 1, :] = True
    return vol


def _threshold_semantics():
    """The threshold itself, NaN, +-inf, -0.0 and the numbers next to zero, against threshold 0."""
    tiny = np.float32(1e-45)        # the smallest subnormal
    vals = np.array([0.0, np.nan, -np.nan, np.inf, -np.inf, -0.0, tiny, -tiny, 1.0, -1.0, 2.0], dtype=np.float32)
    rng = np.random.default_rng(77)
    return vals[rng.integers(0, len(vals), size=(3, TY + 3, TX + 5))]


@functools.lru_cache(maxsize=None)
def _all():
    big = (2 * TZ + 1, 2 * TY + 1, 2 * TX + 1)
    cases = [
        dict(name="single_fg", vol=_f(np.ones((1, 1, 1))), threshold=0.5),
        dict(name="single_bg", vol=_f(np.zeros((1, 1, 1))), threshold=0.5),
        dict(name="runs_x", vol=_f(_runs(2 * TX + 3).reshape(1, 1, -1)), threshold=0.5),
        dict(name="runs_y", vol=_f(_runs(2 * TY + 3).reshape(1, -1, 1)), threshold=0.5),
        dict(name="runs_z", vol=_f(_runs(2 * TZ + 3).reshape(-1, 1, 1)), threshold=0.5),
        dict(name="all_fg", vol=_f(np.ones(big)), threshold=0.5),
        dict(name="checkerboard", vol=_f(np.indices(big).sum(axis=0) % 2 == 0), threshold=0.5),
    ]
    for d in DIRECTIONS:
        cases.append(dict(name="pair_" + "".join("m0p"[c + 1] for c in d), vol=_f(_straddle_pair(d)), threshold=0.5, direction=d))
    for d in DIRECTIONS:
        if all(d):
            cases.append(dict(name="chain_" + "".join("m0p"[c + 1] for c in d), vol=_f(_corner_chain(d)), threshold=0.5))
    cases += [
        dict(name="chain_mixed", vol=_f(_mixed_chain()), threshold=0.5),
        dict(name="serpentine", vol=_f(_serpentine()), threshold=0.5),
        dict(name="nested_us", vol=_f(_nested_us()), threshold=0.5),
        dict(name="nested_vs", vol=_f(_nested_vs()), threshold=0.5),
        dict(name="spiral", vol=_f(_spiral()), threshold=0.5),
        dict(name="comb", vol=_f(_comb()), threshold=0.5),
    ]
    for seed, p in enumerate((0.05, 0.2, 0.3, 0.5, 0.9)):
        rng = np.random.default_rng(1000 + seed)
        # values in (0, 1): foreground is value > 1 - p, so the threshold is not 0.5 and the mask is not the data
        cases.append(dict(name=f"noise_p{p}", vol=rng.random((9, 70, 1030), dtype=np.float32), threshold=float(np.float32(1.0 - p))))
    cases.append(dict(name="threshold_semantics", vol=_threshold_semantics(), threshold=0.0))
    for c in cases:
        c.setdefault("connectivities", CONNECTIVITIES)
        c["vol"].setflags(write=False)
    return tuple(cases)


CASES = _all()
NAMES = [c["name"] for c in CASES]
PARAMS = [(c["name"], k) for c in CASES for k in c["connectivities"]]
PARAM_IDS = [f"{n}-{k}" for n, k in PARAMS]


def case(name):
    return CASES[NAMES.index(name)]


def expected_count(name, connectivity):
    """The object count where the construction fixes it (None otherwise)."""
    level = {6: 1, 18: 2, 26: 3}[connectivity]
    c = case(name)
    if name.startswith("pair_"):
        return 1 if sum(1 for v in c["direction"] if v) <= level else 2
    if name.startswith("chain_") and name != "chain_mixed":
        return 1 if level == 3 else 3
    fixed = {"single_fg": 1, "single_bg": 0, "all_fg": 1, "serpentine": 1, "nested_us": 4, "nested_vs": 4, "spiral": 1, "comb": 1,
             "chain_mixed": 2 if level == 1 else 1}
    if name == "checkerboard":
        return int(c["vol"].sum()) if level == 1 else 1
    return fixed.get(name)


def ramp(shape):
    """Intensities for the table: a ramp with a sign change, exactly representable, different in every voxel."""
    n = int(np.prod(shape))
    return (np.arange(n, dtype=np.float32) * np.float32(0.25) - np.float32(n // 8)).reshape(shape)


def intensities(name):
    """The intensity volume a case's table is measured with (all_fg: a ramp; the others: reproducible noise)."""
    shape = case(name)["vol"].shape
    if name == "all_fg":
        return ramp(shape)
    rng = np.random.default_rng(NAMES.index(name))
    return (rng.standard_normal(shape) * 100.0).astype(np.float32)
