"""The rule of ``csrc/stats.hpp`` restated in numpy: keys, digit tables, order statistics by sorting the keys, exact moments,
the quantile interpolation and the rescale.  The checker of tests/test_stats_host.py and tests/test_stats_gpu.py, never the
product."""

import math

import numpy as np


def key_bits(dtype) -> int:
    return 32 if np.dtype(dtype) == np.float32 else 16


def keys_of(arr) -> np.ndarray:
    """uint32 keys of a float32 / uint16 array (NaNs included: drop them first)."""
    arr = np.ascontiguousarray(arr).reshape(-1)
    if arr.dtype == np.uint16:
        return arr.astype(np.uint32)
    b = arr.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def values_of(keys, dtype) -> np.ndarray:
    k = np.asarray(keys, dtype=np.uint32)
    if np.dtype(dtype) == np.uint16:
        return k.astype(np.uint16)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def non_nan(arr) -> np.ndarray:
    arr = np.ascontiguousarray(arr).reshape(-1)
    return arr if arr.dtype == np.uint16 else arr[~np.isnan(arr)]


def sorted_keys(arrs) -> np.ndarray:
    return np.sort(np.concatenate([keys_of(non_nan(a)) for a in arrs]))


def order_statistics(arrs, ranks) -> np.ndarray:
    return values_of(sorted_keys(arrs)[np.asarray(ranks, dtype=np.int64)], arrs[0].dtype)


def prefix_of(key: int, pass_index: int, bits: int, kbits: int) -> int:
    return 0 if pass_index == 0 else int(key) >> (kbits - bits * pass_index)


def digit_tables(arr, pass_index: int, prefixes, table_of_rank, bits: int) -> np.ndarray:
    """uint64 [k, bins]: what one call adds to zeroed tables."""
    kbits, bins = key_bits(arr.dtype), 1 << bits
    keys = keys_of(non_nan(arr)).astype(np.uint64)
    shift = max(kbits - bits * (pass_index + 1), 0)
    digit = (keys >> np.uint64(shift)) & np.uint64(bins - 1)
    prefix = keys >> np.uint64(shift + bits) if pass_index else np.zeros_like(keys)
    out = np.zeros((len(prefixes), bins), dtype=np.uint64)
    for p, t in set(zip(prefixes, table_of_rank)):
        out[t] += np.bincount(digit[prefix == np.uint64(p)].astype(np.int64), minlength=bins).astype(np.uint64)
    return out


def moments(arrs) -> dict:
    """count, nan_count, the extremes by key, and the exact sums: Python integers for uint16, ``math.fsum`` of the exact float64
    terms (and the sums of their magnitudes) for float32."""
    dtype = arrs[0].dtype
    kept = np.concatenate([non_nan(a) for a in arrs])
    total = sum(int(np.asarray(a).size) for a in arrs)
    out = {"count": int(kept.size), "nan_count": total - int(kept.size)}
    if kept.size:
        ks = keys_of(kept)
        out["min"], out["max"] = values_of([ks.min()], dtype)[0], values_of([ks.max()], dtype)[0]
    if dtype == np.uint16:
        v = kept.astype(object)
        out["sum"], out["sum_sq"] = int(v.sum()) if kept.size else 0, int((v * v).sum()) if kept.size else 0
    else:
        v = kept.astype(np.float64)
        finite = bool(np.all(np.isfinite(v)))
        out["finite"] = finite
        if finite:
            out["sum"], out["sum_abs"] = math.fsum(v), math.fsum(np.abs(v))
            out["sum_sq"] = out["sum_sq_abs"] = math.fsum(v * v)          # (v * v is exact in float64)
    return out


def interpolate(a, b, g) -> float:
    a, b, g = np.float64(a), np.float64(b), np.float64(g)
    with np.errstate(all="ignore"):
        return float(b - (b - a) * (np.float64(1) - g) if g >= 0.5 else a + (b - a) * g)


def bracket(q: float, n: int):
    h = np.float64(q) * np.float64(n - 1)
    j = int(np.floor(h))
    return j, min(j + 1, n - 1), float(h - np.float64(j))


def rescale(v, sub, div, clip=None) -> np.ndarray:
    with np.errstate(all="ignore"):
        o = (v.astype(np.float32) - np.float32(sub)) / np.float32(div)
        return o if clip is None else np.clip(o, np.float32(clip[0]), np.float32(clip[1]))
