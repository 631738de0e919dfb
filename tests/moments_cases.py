"""The cases of the moment tests: label volumes sized from the kernel's geometry (``segment.moments_geometry()``: ``S`` LDS slots
per workgroup), built once and handed out read-only, and the scenes of the shape tests."""

import functools

import numpy as np

INT32_MIN = -2 ** 31
INT32_MAX = 2 ** 31 - 1
STEP = 1024          # voxels one workgroup takes per stride of its span (csrc/moments.hpp kStep)

# X = 130 and 1030 make runs cross wave steps (64 voxels) and row ends
SHAPES = [(1, 1, 1), (1, 1, 65), (2, 3, 130), (5, 9, 130), (3, 7, 1030)]
CONTENTS = ["one-label", "background", "random-0..5", "random-0..4S", "runs", "distinct", "ignored-values", "n-above"]
PARAMS = [(shape, content) for shape in SHAPES for content in CONTENTS]
PARAM_IDS = ["x".join(map(str, shape)) + "-" + content for shape, content in PARAMS]
CAPS = (1, 2, 0)     # max_blocks: one workgroup, two, the default
MANY_LABELS = [((5, 9, 130), "random-0..4S"), ((3, 7, 1030), "random-0..4S")]
ROW_CROSSING = [((2, 3, 130), "runs"), ((5, 9, 130), "runs"), ((3, 7, 1030), "runs")]


def _frozen(arr):
    arr = np.ascontiguousarray(arr, dtype=np.int32)
    arr.setflags(write=False)
    return arr


def runs_flat(n: int) -> np.ndarray:
    """Runs of lengths 1, 2, .. 130, 1, 2, .. along the linear index, labelled 1, 2, 3, 1, ..: neighbouring runs differ, and a
    run that lies over a row end continues with the same label in the next row."""
    out = np.zeros((n,), np.int32)
    at, k = 0, 0
    while at < n:
        length = k % 130 + 1
        out[at:at + length] = k % 3 + 1
        at, k = at + length, k + 1
    return out


@functools.lru_cache(maxsize=None)
def case(shape, content, slots):
    """``(labels, n)``: a read-only int32 volume and the number of objects the entry is told."""
    voxels = int(np.prod(shape))
    rng = np.random.default_rng(1000 * voxels + CONTENTS.index(content))
    if content == "one-label":
        labels, n = np.ones(shape, np.int32), 1
    elif content == "background":
        labels, n = np.zeros(shape, np.int32), 3
    elif content == "random-0..5":
        labels, n = rng.integers(0, 6, shape), 5
    elif content == "random-0..4S":
        labels, n = rng.integers(0, 4 * slots + 1, shape), 4 * slots
    elif content == "runs":
        labels, n = runs_flat(voxels).reshape(shape), 3
    elif content == "distinct":
        labels, n = (np.arange(voxels) + 1).reshape(shape), voxels
    elif content == "ignored-values":
        n = 2
        values = np.array([0, 1, 2, -1, INT32_MIN, n + 1, INT32_MAX], dtype=np.int64)
        labels = values[rng.integers(0, len(values), shape)]
        labels.flat[:len(values)] = values[:voxels]
    elif content == "n-above":
        labels, n = rng.integers(0, 6, shape), 9
    else:
        raise KeyError(content)
    return _frozen(labels), n


def spans(voxels: int, cap: int, default_cap: int):
    """``(first, last)`` of every workgroup's span under ``max_blocks = cap`` (the entry's arithmetic)."""
    cap = cap if cap > 0 else default_cap
    steps = -(-voxels // STEP)
    span = -(-steps // min(steps, cap)) * STEP
    return [(first, min(first + span, voxels)) for first in range(0, voxels, span)]


# ---- the scenes of the shape tests ----


def ellipsoid(shape, semi_zyx, turn_yx_degrees=0.0):
    """The voxels whose centres lie inside the ellipsoid of these semi-axes about the centre of ``shape``, turned about z."""
    z, y, x = (c - (s - 1) / 2.0 for c, s in zip(np.indices(shape), shape))
    t = np.deg2rad(turn_yx_degrees)
    u, v = np.cos(t) * x + np.sin(t) * y, -np.sin(t) * x + np.cos(t) * y        # u along the turned x, v along the turned y
    a, b, c = semi_zyx
    return _frozen((z / a) ** 2 + (v / b) ** 2 + (u / c) ** 2 <= 1.0)


def two_balls():
    """Two balls of radius 10 whose centres are 18 apart along x, as a float32 volume of 0 and 1."""
    z, y, x = np.indices((24, 24, 44))
    mask = ((z - 11.5) ** 2 + (y - 11.5) ** 2 + (x - 12.0) ** 2 <= 100.0) | ((z - 11.5) ** 2 + (y - 11.5) ** 2 + (x - 30.0) ** 2 <= 100.0)
    return np.ascontiguousarray(mask, dtype=np.float32)
