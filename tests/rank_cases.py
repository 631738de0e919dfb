"""The cases of the rank-filter tests (``tests/test_rank_host.py``, ``tests/test_rank_gpu.py``), sized from the exported tiling
(``lsr_rank_filter_tiling``): with ``(tz, ty, tx)`` the tile of outputs of a workgroup and ``R`` the greatest half-width,

* shapes: per axis ``1``, ``2``, ``t - 1``, ``t``, ``t + 1`` and ``2t + 1``, crossed sparingly -- the diagonal, and three mixed
  ones; ``(2tz + 1, 2ty + 1, 2tx + 1)``, the largest, is three tiles on every axis, the last with one live plane, row and lane;
* half-widths: the seven triples of ``{0, 1}^3`` that have a kernel of their own, none, 2 on one axis, ``(1, 1, 2)`` (the first
  window past the register dispatch), the cap on every axis, ``(3, 0, 1)``, and ``(2, 3, 1)``; on the shapes ``(1, 1, 1)`` and
  ``(2, 2, 2)`` the windows of half-width 2 and 3 are wider than the axis and the fold repeats;
* contents: noise, small integers (heavy ties), a mix of ``-0.0`` and ``+0.0``, ``+-inf`` at 10 %, a constant, a ramp, isolated
  spikes of ``+-9`` on noise of 0.1 (``THRESHOLD`` splits them from the noise), NaN at 10 % (two payloads; restatement only);
* ranks: ``0, 1, n // 2, n - 2, n - 1``, de-duplicated; ops: all four at the median.

Every array is read-only: the tests share them.
"""

import functools

import numpy as np

from shrimpy_amd import rank as K

R, TZ, TY, TX = K.tiling()

SHAPES = [(1, 1, 1), (2, 2, 2), (TZ - 1, TY - 1, TX - 1), (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1), (2 * TZ + 1, 2 * TY + 1, 2 * TX + 1),
          (1, 2 * TY + 1, 2), (2 * TZ + 1, 2, TX), (2, 1, 2 * TX + 1)]

REGISTER = [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
HALF_WIDTHS = REGISTER + [(0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 2), (R, R, R), (R, 0, 1), (2, R, 1)]

CONTENTS = ["noise", "small_integers", "zeros", "inf", "constant", "ramp", "spikes", "nan"]
NAN_FREE = [c for c in CONTENTS if c != "nan"]
OPS = ["value", "remove_bright", "remove_dark", "remove_both"]
THRESHOLD = 0.75                            # between the noise of the spike scene (sigma 0.1) and its spikes (+-9); splits the
#                                             small integers' differences too (1 and more pass, 0 does not)

PARAMS = [(shape, r) for shape in SHAPES for r in HALF_WIDTHS]
PARAM_IDS = ["x".join(map(str, s)) + "-r" + "_".join(map(str, r)) for s, r in PARAMS]


def window_size(r):
    return (2 * r[0] + 1) * (2 * r[1] + 1) * (2 * r[2] + 1)


def ranks_of(r):
    n = window_size(r)
    return sorted({k for k in (0, 1, n // 2, n - 2, n - 1) if 0 <= k < n})


def calls_of(r):
    """``(content, rank, op)`` of every call of a (shape, half-widths) pair."""
    n = window_size(r)
    out = []
    for content in CONTENTS:
        out += [(content, k, "value") for k in ranks_of(r)]
        out += [(content, n // 2, op) for op in OPS[1:]]
    return out


@functools.lru_cache(maxsize=None)
def volume(shape, content):
    """The float32 volume of a case (read-only)."""
    rng = np.random.default_rng([SHAPES.index(shape), CONTENTS.index(content)])
    if content == "noise":
        v = rng.normal(size=shape)
    elif content == "small_integers":
        v = rng.integers(-2, 3, size=shape)
    elif content == "zeros":
        v = np.where(rng.random(size=shape) < 0.5, -0.0, 0.0)
    elif content == "inf":
        v = rng.normal(size=shape)
        u = rng.random(size=shape)
        v[u < 0.05] = np.inf
        v[u > 0.95] = -np.inf
    elif content == "constant":
        v = np.full(shape, 2.5)
    elif content == "ramp":
        z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
        v = 0.25 * x - 0.5 * y + 3.0 * z - 3.0
    elif content == "spikes":
        v = 0.1 * rng.normal(size=shape)
        u = rng.random(size=shape)
        v[u < 0.03] += 9.0
        v[u > 0.97] -= 9.0
    elif content == "nan":
        v = rng.normal(size=shape).astype(np.float32)
        u = rng.random(size=shape)
        bits = v.view(np.uint32)
        bits[u < 0.05] = 0x7FC00000
        bits[u > 0.95] = 0xFFC00001                                # a negative NaN with a payload
        v = bits.view(np.float32)
    else:
        raise KeyError(content)
    v = np.ascontiguousarray(v, dtype=np.float32)
    v.setflags(write=False)
    return v


# ---- the scenes of the outlier and segmentation tests ------------------------------------------------------------------------------

SPIKE_SHAPE = (6, 20, 24)
SPIKE_COUNT = 40
SPIKE_HEIGHT = 3000.0
SPIKE_THRESHOLD = 200.0


@functools.lru_cache(maxsize=None)
def spike_scene():
    """``100 + 10 N(0, 1)`` with 40 voxels raised by 3000, no two of them in one (1, 3, 3) window: ``(volume, flat indices)``."""
    rng = np.random.default_rng(7)
    vol = (100.0 + 10.0 * rng.normal(size=SPIKE_SHAPE)).astype(np.float32)
    chosen = []
    for e in rng.permutation(vol.size).tolist():
        z, y, x = np.unravel_index(e, SPIKE_SHAPE)
        if all(not (z == a and abs(y - b) <= 2 and abs(x - c) <= 2) for a, b, c in chosen):
            chosen.append((z, y, x))
        if len(chosen) == SPIKE_COUNT:
            break
    at = np.sort(np.ravel_multi_index(tuple(np.array(chosen).T), SPIKE_SHAPE))
    vol.flat[at] += np.float32(SPIKE_HEIGHT)
    vol.setflags(write=False)
    at.setflags(write=False)
    return vol, at


BALL_SHAPE = (12, 32, 48)
BALL_THRESHOLD = 50.0


@functools.lru_cache(maxsize=None)
def speckled_balls():
    """Two balls of amplitude 100 and radius 4 on a background of 0 with 1 % of the voxels raised by 1000: the unfiltered
    labelling finds the speckle as objects of its own, the median under a (1, 1, 1) box does not."""
    z, y, x = np.ogrid[:BALL_SHAPE[0], :BALL_SHAPE[1], :BALL_SHAPE[2]]
    vol = np.zeros(BALL_SHAPE, dtype=np.float32)
    for c in ((6, 10, 12), (6, 20, 34)):
        vol[(z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= 16] = 100.0
    vol[np.random.default_rng(11).random(BALL_SHAPE) < 0.01] += 1000.0
    vol.setflags(write=False)
    return vol
