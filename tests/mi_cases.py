"""Inputs shared by the mutual-information tests (``test_mi_host.py``: the host twins against ``mi_ref``;
``test_mi_gpu.py``: the kernels against the twins)."""

import functools

import numpy as np

from oracle import cpu_ref as o
from tests.test_estimate import _scene, _tilted

MOVING_SHAPE, TARGET_SHAPE = (20, 37, 51), (18, 40, 45)     # different on purpose
BINS = (8, 32, 64)
STRIDES = (1, 2, (1, 2, 3))
CENTRE, SCALE = np.array([8.5, 19.5, 22.0]), 22.5

# every entry a multiple of 1/8: coordinates, fractions and the trilinear value are exact in float64
EIGHTHS = np.array([[1.0, 0.0, 0.125, 0.5],
                    [0.0, 0.875, 0.0, 1.25],
                    [-0.125, 0.0, 1.0, 3.0]])


@functools.lru_cache(maxsize=None)
def exact_pair():
    """Integer-valued volumes in 0 .. 255: with ``EIGHTHS`` and power-of-two bin scales float64 rounding cannot matter."""
    rng = np.random.default_rng(42)
    return (rng.integers(0, 256, MOVING_SHAPE).astype(np.float32), rng.integers(0, 256, TARGET_SHAPE).astype(np.float32))


def exact_ranges(bins):
    """Target scale bins / 256 and moving scale (bins - 1) / (32 (bins - 1)) = 1 / 32: both exact powers of two."""
    return ((0.0, 256.0), (0.0, 32.0 * (bins - 1)))


@functools.lru_cache(maxsize=None)
def general_pair():
    """The volumes and the transform of the normal-equations test, the ranges their min / max."""
    mov, tgt = _scene(5, MOVING_SHAPE), _scene(6, TARGET_SHAPE)
    m = _tilted(TARGET_SHAPE, tilt=4.0, shift=(1.5, -2.0, 3.0))
    ranges = ((float(tgt.min()), float(tgt.max())), (float(mov.min()), float(mov.max())))
    return mov, tgt, m, ranges


def non_monotone(v):
    """The intensity map of the recovery cases: no linear gain / offset describes it."""
    return 150.0 * np.sin(np.pi * np.asarray(v, dtype=np.float64) / 160.0) ** 2 + 5.0


@functools.lru_cache(maxsize=None)
def recovery_pair(shape):
    """A bead scene, the tilted truth and the target made from the warped scene by the non-monotone map."""
    mov = _scene(3, shape) if shape == (24, 40, 48) else _scene(7, shape, n=60)
    true = _tilted(shape)
    tgt = non_monotone(o.affine_apply_4x4(mov, true, shape)).astype(np.float32)
    return mov, tgt, true


def corner_error(a, b, shape):
    """Largest displacement (voxels) of the target volume's corners between two maps."""
    corners = np.array([[z, y, x, 1.0] for z in (0, shape[0] - 1) for y in (0, shape[1] - 1) for x in (0, shape[2] - 1)])
    return float(np.abs(corners @ (np.asarray(a)[:3] - np.asarray(b)[:3]).T).max())
