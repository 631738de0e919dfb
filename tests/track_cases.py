"""The cases of the tracking tests: label-volume pairs for the overlap table (sizes derived from the kernel's geometry) and
the synthetic time-lapse of the linking tests.  Everything is built once and handed out read-only."""

import functools

import numpy as np
import scipy.ndimage

INT32_MIN = -2 ** 31
INT32_MAX = 2 ** 31 - 1

SHAPES = [(1, 1, 1), (3, 5, 7), (2, 3, 64), (2, 3, 65), (5, 9, 130)]
CONTENTS = ["one-pair", "random-0..3", "random-0..1000", "runs", "background-values", "int32-max"]
PARAMS = [(shape, content) for shape in SHAPES for content in CONTENTS]
PARAM_IDS = ["x".join(map(str, shape)) + "-" + content for shape, content in PARAMS]
RUNS_SHAPE = (1, 67, 130)          # 8710 voxels: every run length 1 .. 130 fits (8515)
MANY_PAIRS = ((5, 9, 130), "random-0..1000")


def runs_flat(n: int):
    """Runs of equal pairs of lengths 1, 2, .. 130, 1, 2, .. along the linear index; neighbouring runs differ in a."""
    a, b = np.zeros((n,), np.int32), np.zeros((n,), np.int32)
    starts, at, k = [], 0, 0
    while at < n:
        length = k % 130 + 1
        starts.append(at)
        a[at:at + length] = k % 3 + 1
        b[at:at + length] = k % 4 + 1
        at, k = at + length, k + 1
    return a, b, starts + [n]


def _frozen(*arrays):
    for arr in arrays:
        arr.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pair(shape, content):
    """``(a, b)``: two read-only int32 volumes."""
    n = int(np.prod(shape))
    rng = np.random.default_rng(1000 * n + CONTENTS.index(content))
    if content == "one-pair":
        a, b = np.ones(shape, np.int32), np.ones(shape, np.int32)
    elif content == "random-0..3":
        a, b = rng.integers(0, 4, shape).astype(np.int32), rng.integers(0, 4, shape).astype(np.int32)
    elif content == "random-0..1000":
        a, b = rng.integers(1, 1001, shape).astype(np.int32), rng.integers(1, 1001, shape).astype(np.int32)
        a[rng.random(shape) < 0.5] = 0
        b[rng.random(shape) < 0.5] = 0
    elif content == "runs":
        a, b, _ = runs_flat(n)
        a, b = a.reshape(shape), b.reshape(shape)
    elif content == "background-values":
        values = np.array([0, -1, INT32_MIN, 1, 2, -7, 3], dtype=np.int32)
        a, b = values[rng.integers(0, len(values), shape)], values[rng.integers(0, len(values), shape)]
    elif content == "int32-max":
        values = np.array([0, 1, INT32_MAX, INT32_MAX - 1], dtype=np.int32)
        a, b = values[rng.integers(0, len(values), shape)], values[rng.integers(0, len(values), shape)]
        a.flat[0] = b.flat[0] = INT32_MAX
    else:
        raise KeyError(content)
    return _frozen(np.ascontiguousarray(a), np.ascontiguousarray(b))


@functools.lru_cache(maxsize=None)
def distinct_pairs(lds_slots: int):
    """``a = arange + 1`` against ``b = reversed arange + 1`` on a shape of more than ``2 * lds_slots`` voxels: every voxel is a
    pair of its own, so one workgroup's LDS table overflows."""
    x = 130
    y = (2 * lds_slots) // x + 2
    shape = (1, y, x)
    n = y * x
    assert n > 2 * lds_slots
    a = (np.arange(n, dtype=np.int32) + 1).reshape(shape)
    b = (np.arange(n, dtype=np.int32)[::-1] + 1).reshape(shape)
    return _frozen(np.ascontiguousarray(a), np.ascontiguousarray(b))


# ---- the time-lapse of the linking tests: (12, 24, 48) over t = 0 .. 4 ----

SCENE_SHAPE = (12, 24, 48)
SCENE_T = 5


def _balls(t):
    balls = [((6, 6, 6 + 2 * t), 3)]                                   # A
    if t <= 1:
        balls += [((6, 17, 24), 4), ((3, 6, 40), 2)]                   # B, C
    else:
        d = 3 + (t - 2)
        balls += [((6, 17, 24 - d), 2), ((6, 17, 24 + d), 2)]          # B's daughters
    if t >= 3:
        balls.append(((9, 20, 42), 2))                                 # D
    return balls


def scene_mask(t):
    z, y, x = np.indices(SCENE_SHAPE)
    mask = np.zeros(SCENE_SHAPE, dtype=bool)
    for (cz, cy, cx), r in _balls(t):
        mask |= (z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    return mask


@functools.lru_cache(maxsize=None)
def scene():
    """The five label volumes (``scipy.ndimage.label``, 6-connectivity), read-only."""
    frames = []
    for t in range(SCENE_T):
        labels, _ = scipy.ndimage.label(scene_mask(t))
        frames.append(np.ascontiguousarray(labels, dtype=np.int32))
    return _frozen(*frames)


SCENE_VOLUMES = [[33, 257, 123], [33, 257, 123], [123, 33, 33], [123, 33, 33, 33], [123, 33, 33, 33]]
SCENE_TABLES = [{(1, 1, 33), (2, 2, 257), (3, 3, 69)}, {(2, 2, 24), (2, 3, 24), (3, 1, 69)}, {(1, 1, 69), (2, 2, 20), (3, 3, 20)}]
SCENE_TABLE_SHIFTED = {(1, 1, 11), (2, 2, 163), (3, 3, 123)}          # t0 -> t1 with shift (0, 0, 2): A is fully re-aligned
SCENE_TRACKS_DIVISIONS = [(1, 0, 1, 0), (2, 0, 1, 0), (3, 0, 4, 0), (4, 2, 4, 2), (5, 2, 4, 2), (6, 3, 4, 0)]
SCENE_TRACKS_NO_DIVISIONS = [(1, 0, 1, 0), (2, 0, 4, 0), (3, 0, 4, 0), (4, 2, 4, 0), (5, 3, 4, 0)]


def boxes(shape, *specs):
    """A label volume with the box ``(label, z0, z1, y0, y1, x0, x1)`` of every spec."""
    out = np.zeros(shape, dtype=np.int32)
    for label, z0, z1, y0, y1, x0, x1 in specs:
        out[z0:z1, y0:y1, x0:x1] = label
    return out
