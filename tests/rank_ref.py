"""The rank-filter rule (``csrc/rank.hpp``) restated in NumPy, and the oracle ``scipy.ndimage``.

Rule: the window of half-widths ``(rz, ry, rx)`` around ``p`` under scipy's ``reflect`` border (index ``i`` of an axis of length
``L`` reads ``m = i mod 2L``, then ``m < L ? m : 2L - 1 - m``; reflected voxels count as often as they fall in the window);
``m(p)`` is the element of rank ``rank`` of the window's values under the order-preserving integer image of a float (``-0.0``
below ``+0.0``, ``+-inf`` ordinary, a NaN the greatest and returned as the canonical quiet NaN ``0x7fc00000``).  The ops compare
``v - m`` and ``m - v`` (one float32 subtraction each) with a threshold; a comparison with a NaN is false.

The restatement gathers the window into a stack and SORTS it (the kernel bisects): independent of the kernel's method.  scipy is
pinned on NaN-free volumes only and may return either zero on ``+-0.0`` ties: it is compared by value, the restatement by bytes.
"""

import functools

import numpy as np
import scipy.ndimage as ndi

from tests import rank_cases as C

QUIET_NAN = np.uint32(0x7FC00000)
NAN_CODE = np.uint32(0xFFFFFFFF)


def float_key(v):
    """``label::float_key``: uint32 keys that order like the floats."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def key_float(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def fold(i, length):
    m = np.mod(i, 2 * length)
    return np.where(m < length, m, 2 * length - 1 - m)


def sorted_windows(v, r):
    """``(n, Z, Y, X)`` uint32: the codes of every voxel's window, sorted along axis 0."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    code = np.where(np.isnan(v), NAN_CODE, float_key(v))
    index = [fold(np.arange(-ra, n + ra), n) for ra, n in zip(r, v.shape)]
    padded = code[np.ix_(*index)]
    z, y, x = v.shape
    stack = [padded[dz:dz + z, dy:dy + y, dx:dx + x] for dz in range(2 * r[0] + 1) for dy in range(2 * r[1] + 1)
             for dx in range(2 * r[2] + 1)]
    return np.sort(np.stack(stack), axis=0)


def decode(code):
    bits = key_float(code).view(np.uint32).copy()
    bits[code == NAN_CODE] = QUIET_NAN
    return bits.view(np.float32)


def apply_op(m, v, op, threshold):
    """The fused op in float32: ``m`` the selected element, ``v`` the volume."""
    if op == "value":
        return m
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        bright, dark = (v - m) > t, (m - v) > t
    take = {"remove_bright": bright, "remove_dark": dark, "remove_both": bright | dark}[op]
    return np.where(take, m, v)


def restated(v, r, rank, op="value", threshold=0.0):
    """The rule on a float32 volume: a new float32 array."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    return apply_op(decode(sorted_windows(v, r)[rank]), v, op, threshold)


@functools.lru_cache(maxsize=2)
def _case_sorted(shape, content, r):
    return sorted_windows(C.volume(shape, content), r)


@functools.lru_cache(maxsize=None)
def case_restated(shape, content, r, rank, op):
    """The restatement on a case of ``tests/rank_cases.py``, computed once (read-only)."""
    v = C.volume(shape, content)
    out = np.ascontiguousarray(apply_op(decode(_case_sorted(shape, content, r)[rank]), v, op, C.THRESHOLD))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_scipy(shape, content, r, rank, op):
    """scipy's answer on a NaN-free case, computed once (read-only): ``rank_filter``, and ``np.where`` on it for the ops."""
    assert content != "nan"
    v = C.volume(shape, content)
    m = ndi.rank_filter(v, rank, size=tuple(2 * k + 1 for k in r), mode="reflect")
    assert m.dtype == np.float32
    out = np.ascontiguousarray(apply_op(m, v, op, C.THRESHOLD))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_scipy_named(shape, content, r, rank):
    """On a NaN-free case, scipy's ``median_filter`` where ``rank`` is the median and its ``percentile_filter`` at 0 and 100
    where ``rank`` is the least or the greatest: a list, empty at any other rank."""
    assert content != "nan"
    v, size, n = C.volume(shape, content), tuple(2 * k + 1 for k in r), C.window_size(r)
    out = []
    if rank == n // 2:
        out.append(ndi.median_filter(v, size=size, mode="reflect"))
    if rank == 0:
        out.append(ndi.percentile_filter(v, 0, size=size, mode="reflect"))
    if rank == n - 1:
        out.append(ndi.percentile_filter(v, 100, size=size, mode="reflect"))
    return out


def same_bytes(a, b):
    """Byte for byte, all NaNs counting as equal."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def check(shape, content, r, rank, op, got):
    """``got`` against the restatement (bytes, NaNs as a mask; a NaN of op ``value`` is the canonical one) and, on a NaN-free
    case, against ``scipy.ndimage.rank_filter`` by value with no voxel excluded -- and against ``median_filter`` at the median and
    ``percentile_filter`` at 0 and 100 at the two ends."""
    what = f"{shape} {content} r={r} rank={rank} {op}"
    want = case_restated(shape, content, r, rank, op)
    assert same_bytes(got, want), f"{what}: differs from the restatement at {int((got.view(np.uint32) != want.view(np.uint32)).sum())} voxels"
    if op == "value":
        assert np.all(got.view(np.uint32)[np.isnan(got)] == QUIET_NAN), f"{what}: a NaN that is not the canonical one"
    if content != "nan":
        assert not np.isnan(got).any()
        assert np.array_equal(got, case_scipy(shape, content, r, rank, op)), f"{what}: differs from scipy"
        if op == "value":
            for ref in case_scipy_named(shape, content, r, rank):
                assert np.array_equal(got, ref), f"{what}: differs from scipy's median_filter / percentile_filter"
