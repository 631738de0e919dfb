"""Float64 / integer restatement of one pyramid level (``shrimpy_amd/pyramid.py``, ``csrc/pyramid.hpp``) -- the oracle
of tests/test_pyramid_host.py and tests/test_pyramid_gpu.py; nothing here is imported by the package.

Output voxel (z, y, x) is the mean over the input voxels (fz z + a, 2 y + b, 2 x + c), a < fz, b < 2, c < 2, that lie
inside the volume; the output has ceil(n / f) voxels per axis, a window 1, 2, 4 or 8 voxels.

The a-priori bound of the float32 result: the window sum is a pairwise sum of at most eight values, three additions
deep, each rounding at most 2^-24 of its own partial sum, and every partial sum is at most sum|v|; the division by the
count, a power of two, is exact.  So |got - exact| <= 3 * 2^-24 * sum|v| / count = 3 * 2^-24 * mean|v| of the window
(first order; the second-order terms are 2^-48 and no case here comes near the first).
"""

from __future__ import annotations

import numpy as np

U = 2.0 ** -24

# (Z, Y, X): degenerate extents, odd and even ones, one with rows longer than a wavefront's 256 inputs
SHAPES = [(1, 1, 1), (1, 3, 2), (3, 1, 5), (2, 2, 2), (5, 7, 9), (4, 6, 8), (7, 33, 67)]
# on the device also: rows that split across workgroups, and an odd X that puts every second row off 16-byte alignment
GPU_SHAPES = SHAPES + [(3, 5, 1030), (2, 3, 4099)]
FZ = [1, 2]


def out_shape(shape, fz):
    z, y, x = shape
    return (-(-z // fz), -(-y // 2), -(-x // 2))


def window_sums(volume: np.ndarray, fz: int):
    """(sum, count) per output voxel: ``volume`` zero-padded to whole windows and added up in its own dtype's widest
    sibling (float64 / int64); ``count`` is the number of in-volume voxels of each window."""
    v = np.asarray(volume)
    acc = np.int64 if v.dtype.kind in "ui" else np.float64
    zo, yo, xo = out_shape(v.shape, fz)
    pad = np.zeros((zo * fz, yo * 2, xo * 2), dtype=acc)
    pad[:v.shape[0], :v.shape[1], :v.shape[2]] = v
    inside = np.zeros(pad.shape, dtype=np.int64)
    inside[:v.shape[0], :v.shape[1], :v.shape[2]] = 1
    fold = lambda a: a.reshape(zo, fz, yo, 2, xo, 2).sum(axis=(1, 3, 5))   # noqa: E731
    return fold(pad), fold(inside)


def downsample2_f64(volume: np.ndarray, fz: int) -> np.ndarray:
    s, n = window_sums(np.asarray(volume, dtype=np.float64), fz)
    return s / n


def bound_f32(volume: np.ndarray, fz: int) -> np.ndarray:
    """3 * 2^-24 * mean|v| per window."""
    s, n = window_sums(np.abs(np.asarray(volume, dtype=np.float64)), fz)
    return 3.0 * U * s / n


def downsample2_u16(volume: np.ndarray, fz: int) -> np.ndarray:
    """(sum + (count >> 1)) >> log2(count): round half up."""
    s, n = window_sums(np.asarray(volume, dtype=np.uint16), fz)
    k = np.round(np.log2(n)).astype(np.int64)
    assert np.array_equal(1 << k, n), "a window count that is no power of two"
    return ((s + (n >> 1)) >> k).astype(np.uint16)


def f32_volume(shape, seed: int) -> np.ndarray:
    """100 N(0, 1) + 50: mixed sign."""
    rng = np.random.default_rng(seed)
    return (100.0 * rng.standard_normal(shape) + 50.0).astype(np.float32)


def u16_volume(shape, seed: int) -> np.ndarray:
    """The full range, with a block of 65535 (a window of eight needs the 32-bit sum) and one of zeros."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 65536, shape, dtype=np.uint16)
    z, y, x = shape
    v[: max(1, z // 2), : max(1, y // 2), : max(1, x // 2)] = 65535
    v[z - 1, y - 1, : max(1, x // 3)] = 0
    return v
