"""The restatement of the intensity rule (``csrc/intensity.hpp``) in plain numpy.  PARITY UNPINNED: no upstream is vendored; this
file and the rule say the same thing in two ways.

uint16 values: ``np.add.at`` in uint64, the records byte for byte.  float32 values: the count, the extremes (through a numpy
restatement of ``csrc/label.hpp``'s ``float_key``) and, per sum, the exact sum of the exact products (``math.fsum`` of float64
products, which are exact: ``v * v`` has 48 bits, ``v * c`` at most 24 + 29) with the sum of their magnitudes for the bound."""

import math

import numpy as np

SUMS = ("sum_v", "sum_vv", "sum_vz", "sum_vy", "sum_vx")
DTYPE_U16 = np.dtype([("count", "<i8")] + [(f, "<u8") for f in SUMS] + [("v_min", "<u4"), ("v_max", "<u4"), ("pad", "<u4", (2,))])
DTYPE_F32 = np.dtype([("count", "<i8")] + [(f, "<f8") for f in SUMS] + [("v_min", "<f4"), ("v_max", "<f4"), ("pad", "<u4", (2,))])


def _kept(labels: np.ndarray, n: int):
    """``(record index, z, y, x, linear index)`` of the voxels whose label lies in ``1 .. n``."""
    labels = np.asarray(labels)
    z, y, x = (c.ravel().astype(np.int64) for c in np.indices(labels.shape))
    flat = labels.ravel().astype(np.int64)
    keep = (flat >= 1) & (flat <= n)
    return flat[keep] - 1, z[keep], y[keep], x[keep], np.flatnonzero(keep)


def intensity_u16(labels: np.ndarray, values: np.ndarray, n: int) -> np.ndarray:
    """``n`` records (``DTYPE_U16``): ``np.add.at`` of every voxel's gains in uint64, ``np.minimum.at`` / ``np.maximum.at``."""
    k, z, y, x, at = _kept(labels, n)
    v = np.asarray(values).ravel()[at].astype(np.uint64)
    out = np.zeros((n,), dtype=DTYPE_U16)
    gains = dict(sum_v=v, sum_vv=v * v, sum_vz=v * z.astype(np.uint64), sum_vy=v * y.astype(np.uint64), sum_vx=v * x.astype(np.uint64))
    count = np.zeros((n,), dtype=np.int64)
    np.add.at(count, k, 1)
    out["count"] = count
    for f in SUMS:
        column = np.zeros((n,), dtype=np.uint64)
        np.add.at(column, k, gains[f])
        out[f] = column
    lo, hi = np.full((n,), 2 ** 32 - 1, dtype=np.uint64), np.zeros((n,), dtype=np.uint64)
    np.minimum.at(lo, k, v)
    np.maximum.at(hi, k, v)
    out["v_min"] = np.where(count > 0, lo, 0)
    out["v_max"] = hi
    return out


def float_key(values: np.ndarray) -> np.ndarray:
    """``csrc/label.hpp``'s order-preserving uint32 image of a float32."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def key_float(keys: np.ndarray) -> np.ndarray:
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    return np.where(keys & np.uint32(0x80000000), keys & np.uint32(0x7FFFFFFF), ~keys).astype(np.uint32).view(np.float32)


def _ieee_sum(terms: np.ndarray) -> float:
    """The exact sum of finite float64 terms, correctly rounded; with non-finite terms what IEEE addition gives in any order."""
    if np.isnan(terms).any() or (np.isposinf(terms).any() and np.isneginf(terms).any()):
        return math.nan
    if np.isposinf(terms).any():
        return math.inf
    if np.isneginf(terms).any():
        return -math.inf
    return math.fsum(terms.tolist())


def intensity_f32(labels: np.ndarray, values: np.ndarray, n: int) -> dict:
    """Per record: ``count`` (int64), ``v_min`` / ``v_max`` (float32, zero where the count is), ``sums`` ((n, 5) float64: the
    exact sums of the exact products in ``SUMS`` order, rounded once) and ``magnitudes`` ((n, 5): the sums of their absolute
    values, NaN or inf where a term is not finite)."""
    k, z, y, x, at = _kept(labels, n)
    v32 = np.asarray(values, dtype=np.float32).ravel()[at]
    v = v32.astype(np.float64)
    count = np.bincount(k, minlength=n).astype(np.int64)
    keys = float_key(v32).astype(np.int64)
    lo, hi = np.full((n,), 2 ** 32, dtype=np.int64), np.full((n,), -1, dtype=np.int64)
    np.minimum.at(lo, k, keys)
    np.maximum.at(hi, k, keys)
    live = count > 0
    v_min, v_max = np.zeros((n,), np.float32), np.zeros((n,), np.float32)
    v_min[live] = key_float(lo[live].astype(np.uint32))
    v_max[live] = key_float(hi[live].astype(np.uint32))
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.stack([v, v * v, v * z, v * y, v * x], axis=1)          # (inf * 0 is NaN, as in the kernel and the twin)
    order = np.argsort(k, kind="stable")
    bounds = np.r_[0, np.cumsum(count)]
    sums, magnitudes = np.zeros((n, 5)), np.zeros((n, 5))
    terms = terms[order]
    for r in np.flatnonzero(live):
        part = terms[bounds[r]:bounds[r + 1]]
        for c in range(5):
            sums[r, c] = _ieee_sum(part[:, c])
            magnitudes[r, c] = _ieee_sum(np.abs(part[:, c]))
    return {"count": count, "v_min": v_min, "v_max": v_max, "sums": sums, "magnitudes": magnitudes}


def bound(ref: dict) -> np.ndarray:
    """``2 n_k 2^-53 sum|terms|`` per record and sum ((n, 5))."""
    return 2.0 * ref["count"][:, None].astype(np.float64) * 2.0 ** -53 * ref["magnitudes"]
