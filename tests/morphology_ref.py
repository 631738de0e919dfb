"""The grey-morphology rule (``csrc/morphology.hpp``) restated in NumPy, the oracle ``scipy.ndimage`` and a brute force.

Rule: ``erode(v)(p)`` is the least and ``dilate(v)(p)`` the greatest ``v(q)`` over the in-volume ``q`` of the box of half-widths
``(rz, ry, rx)`` around ``p``; voxels outside the volume do not compete.  Values compare by the order-preserving integer image of
a float (``-0.0`` below ``+0.0``, ``+-inf`` ordinary) and the result is the chosen element's bit pattern; a window that holds a
NaN gives the canonical quiet NaN ``0x7fc00000``.  ``open = dilate(erode)``, ``close = erode(dilate)``, the top-hats are one
float32 subtraction.  An axis with half-width 0 gets no pass: with all three at 0 the first four ops copy ``v`` bit for bit.

scipy is pinned on NaN-free volumes only (its comparisons give an order-dependent answer on NaN) and does not tell ``-0.0``
from ``+0.0``: ``np.array_equal`` takes them for equal, the restatement pins the bits.
"""

import functools

import numpy as np
import scipy.ndimage as ndi

from tests import morphology_cases as C

QUIET_NAN = np.uint32(0x7FC00000)
SCIPY = {"grey_erosion": ndi.grey_erosion, "grey_dilation": ndi.grey_dilation, "grey_opening": ndi.grey_opening,
         "grey_closing": ndi.grey_closing, "white_tophat": ndi.white_tophat, "black_tophat": ndi.black_tophat}


def float_key(v):
    """``label::float_key``: uint32 keys that order like the floats."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def key_float(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _extreme(v, r, greatest):
    """Erosion or dilation: per axis, the extreme key over the offsets -r .. r that stay inside the volume."""
    if not any(r):
        return v.copy()
    key, nan = float_key(v), np.isnan(v)
    pick = np.maximum if greatest else np.minimum
    for axis, ra in enumerate(r):
        n = v.shape[axis]
        out_key, out_nan = key.copy(), nan.copy()
        for d in range(1, min(ra, n - 1) + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
            lo, hi = tuple(lo), tuple(hi)
            out_key[lo] = pick(out_key[lo], key[hi])          # the neighbour at +d
            out_key[hi] = pick(out_key[hi], key[lo])          # ... and at -d
            out_nan[lo] |= nan[hi]
            out_nan[hi] |= nan[lo]
        key, nan = out_key, out_nan
    bits = key_float(key).view(np.uint32).copy()
    bits[nan] = QUIET_NAN
    return bits.view(np.float32)


def erode(v, r):
    return _extreme(v, r, False)


def dilate(v, r):
    return _extreme(v, r, True)


def restated(v, r, op):
    """The rule on a float32 volume: a new float32 array."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        if op == "grey_erosion":
            return erode(v, r)
        if op == "grey_dilation":
            return dilate(v, r)
        if op == "grey_opening":
            return dilate(erode(v, r), r)
        if op == "grey_closing":
            return erode(dilate(v, r), r)
        if op == "white_tophat":
            return v - dilate(erode(v, r), r)
        if op == "black_tophat":
            return erode(dilate(v, r), r) - v
    raise KeyError(op)


def brute(v, r, greatest):
    """Erosion or dilation by the definition: a loop over the voxels, the extreme of the clipped box by the key."""
    out = np.empty(v.shape, dtype=np.uint32)
    key = float_key(v)
    for p in np.ndindex(*v.shape):
        box = tuple(slice(max(0, c - ra), c + ra + 1) for c, ra in zip(p, r))
        if np.isnan(v[box]).any():
            out[p] = QUIET_NAN
        else:
            k = key[box].max() if greatest else key[box].min()
            out[p] = key_float(np.array([k]))[0].view(np.uint32)
    return out.view(np.float32)


@functools.lru_cache(maxsize=512)
def case_restated(shape, content, r, op):
    """The restatement on a case of ``tests/morphology_cases.py``, computed once (read-only)."""
    out = restated(C.volume(shape, content), r, op)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=512)
def case_scipy(shape, content, r, op):
    """scipy's answer on a NaN-free case, computed once (read-only)."""
    assert content != "nan"
    with np.errstate(invalid="ignore"):
        out = SCIPY[op](C.volume(shape, content), size=tuple(2 * k + 1 for k in r))
    assert out.dtype == np.float32
    out.setflags(write=False)
    return out


def same_bytes(a, b):
    """Byte for byte, all NaNs counting as equal."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def check(shape, content, r, op, got):
    """``got`` against the restatement (bytes, NaNs as a mask; a NaN of an erosion .. closing with a window is the canonical one)
    and, on a NaN-free case, against scipy (``np.array_equal``, no voxel excluded; the NaNs an ``inf - inf`` makes must sit
    where scipy's do)."""
    want = case_restated(shape, content, r, op)
    assert same_bytes(got, want), f"{shape} {content} r={r} {op}: differs from the restatement at {int((got.view(np.uint32) != want.view(np.uint32)).sum())} voxels"
    if any(r) and not op.endswith("tophat"):
        assert np.all(got.view(np.uint32)[np.isnan(got)] == QUIET_NAN), "a NaN that is not the canonical one"
    if content != "nan":
        ref = case_scipy(shape, content, r, op)
        assert np.array_equal(got, ref, equal_nan=True), f"{shape} {content} r={r} {op}: differs from scipy"
        if content != "inf":
            assert not np.isnan(got).any()
