"""The flat-field rule, restated in numpy (``csrc/flatfield.hip``, ``flat_pattern_cpu`` of ``csrc/host_twins.hip``); nothing here
calls the library.

* ``key(v)``: the order-preserving uint32 image of a float32 -- ``-0.0`` sorts below ``+0.0``, ``+-inf`` are ordinary values.
* ``pattern(vol)``: per pixel, the column sorted by ``key``; ``a = s[(Z - 1) // 2]``, ``b = s[Z // 2]``; an odd ``Z`` gives ``a``, an
  even one ``b - (b - a) * 0.5`` with the difference rounded to float32 and the rest ONE rounding (``fma(-(b - a), 0.5, b)``,
  what ``torch.quantile`` computes on the host); a column holding a NaN gives the canonical quiet NaN ``0x7fc00000``.
* ``mean(pattern)``: ``math.fsum`` over the pattern divided by its size, float64.
* ``apply(vol, pattern, mean)``: ``float32(vol) / pattern * mean``, two float32 roundings, the division first.
* ``split_level`` and ``takes_count_mode`` say which path of the kernel a column and a workgroup take, from the definition.
"""

import math

from fractions import Fraction

import numpy as np

CANONICAL_NAN = 0x7FC00000
COUNT_LIMIT_BITS = 0x47800000               # the bits of 65536.0f: a count is an integer v with bits(v) < this (so not -0.0)


def key(v):
    """The order-preserving uint32 image of float32 values."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def value(k):
    """The float32 of a key."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def middle(vol):
    """``(a, b)``: the order statistics ``(Z - 1) // 2`` and ``Z // 2`` of every column under ``key`` (NaNs sort as their keys)."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    z = vol.shape[0]
    s = np.sort(key(vol), axis=0)
    return value(s[(z - 1) // 2]), value(s[z // 2])


def _round_to_f32(q):
    """The float32 nearest to the Fraction ``q`` (ties to the even mantissa)."""
    c = np.float32(float(q))                                      # within an ulp or two of the answer
    best = None
    for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - q)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    assert best is not None and abs(q) < Fraction(float(np.finfo(np.float32).max)), "overflow is not a case of the tests"
    return np.float32(best[1])


def lerp_half(a, b):
    """``float32(b - float32(b - a) * 0.5)``: the product and the outer subtraction exact, rounded once."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (b - a).astype(np.float32)                            # the one rounding of the difference
        x = b.astype(np.float64)
        y = -(d.astype(np.float64) * 0.5)                         # exact: a float32 halved is a float64
        s = x + y
        t = s - x
        e = (x - (s - t)) + (y - t)                               # TwoSum: s + e == x + y exactly
        out = np.array(s, dtype=np.float32)                       # one rounding where e == 0 (signed zeros as IEEE adds them)
    inexact = np.isfinite(s) & (e != 0)
    for i in np.argwhere(inexact):
        i = tuple(i)
        out[i] = _round_to_f32(Fraction(float(x[i])) + Fraction(float(y[i])))
    return out


def pattern(vol):
    """The median over axis 0 under the rule; the volume may be float32 or uint16."""
    vol = np.ascontiguousarray(vol).astype(np.float32)
    a, b = middle(vol)
    out = a.copy() if vol.shape[0] % 2 else lerp_half(a, b)
    bits = out.view(np.uint32)
    bits[np.isnan(vol).any(axis=0)] = CANONICAL_NAN
    return out


def same_bits(got, want):
    """Bit for bit, except that a NaN the arithmetic itself made (``inf - inf``) is "a NaN at this position"."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def mean(p):
    """``fsum(p) / size`` in float64 (NaN or an infinity if the pattern holds one)."""
    p = np.asarray(p, dtype=np.float32).ravel().astype(np.float64)
    if not np.isfinite(p).all():
        with np.errstate(invalid="ignore"):
            return float(p.sum() / p.size)
    return math.fsum(p.tolist()) / p.size


def mean_bound(p):
    """``2^-24 |m| + n 2^-53 mean|p|``: the float32 rounding of the result plus n float64 roundings of terms of the mean size.
    Below the normal range a float32 rounds to half a denormal step, ``2^-150``, whatever ``m`` is: the first term is at least that
    (the same bound wherever ``|m| >= 2^-126``)."""
    p = np.asarray(p, dtype=np.float32).ravel().astype(np.float64)
    return max(2.0 ** -24 * abs(mean(p)), 2.0 ** -150) + p.size * 2.0 ** -53 * (math.fsum(np.abs(p).tolist()) / p.size)


def apply(vol, p, m):
    """``float32(vol) / pattern * mean``: two float32 roundings, the division first."""
    with np.errstate(all="ignore"):
        q = (np.ascontiguousarray(vol).astype(np.float32) / np.asarray(p, dtype=np.float32)[None]).astype(np.float32)
        return (q * np.float32(m)).astype(np.float32)


def is_count(v):
    """The kernel's predicate: an integer in [+0, 65536) -- ``bits(v) < bits(65536.0)`` and ``v == trunc(v)``."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (v.view(np.uint32) < COUNT_LIMIT_BITS) & (v == np.trunc(v))


def takes_count_mode(vol, cols):
    """Per workgroup of ``cols`` consecutive pixels: whether every sample of its pixels is a count."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    ok = is_count(vol).reshape(vol.shape[0], -1).all(axis=0)
    return np.array([bool(ok[i:i + cols].all()) for i in range(0, ok.size, cols)])


def split_level(column, count=False):
    """For an even ``Z`` the index (0 is the most significant) of the first key byte in which the two middle elements differ;
    ``None`` when they are equal or ``Z`` is odd.  With ``count`` the key is the integer itself (its two low bytes: levels 2, 3)."""
    column = np.ascontiguousarray(column, dtype=np.float32).ravel()
    if column.size % 2:
        return None
    a, b = middle(column[:, None])
    ka, kb = (int(a[0]), int(b[0])) if count else (int(key(a)[0]), int(key(b)[0]))
    for level in range(4):
        shift = 24 - 8 * level
        if (ka >> shift) & 255 != (kb >> shift) & 255:
            return level
    return None


def select_keys(column, count=False):
    """``(keys, ka, kb)`` as Python integers: the keys the select works on -- the integer itself in the count mode -- of every
    sample and of the two middle elements."""
    column = np.ascontiguousarray(column, dtype=np.float32).ravel()
    a, b = middle(column[:, None])
    if count:
        return column.astype(np.int64), int(a[0]), int(b[0])
    return key(column).astype(np.int64), int(key(a)[0]), int(key(b)[0])


def bin_at(k, level):
    """Byte ``level`` of a key (0 is the most significant): the bin of the histogram pass of that level."""
    return (k >> (24 - 8 * level)) & 255


def prefix_at(k, level):
    """The bytes of a key above byte ``level``: what a sample shares with the selected element to be counted at that level."""
    return k >> (32 - 8 * level)
