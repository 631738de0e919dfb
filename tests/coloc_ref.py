"""The restatement of the colocalization rule (``csrc/coloc.hpp``) and of Costes' threshold rule (``shrimpy_amd/colocalize.py``)
in plain numpy.  PARITY UNPINNED: no upstream is vendored; this file and the rule say the same thing in two ways.

uint16 values: ``np.add.at`` in uint64, the records byte for byte.  float32 values: the four counts and, per sum, the exact sum of
the exact terms (``math.fsum`` of float64 products, which are exact: 48 bits) with the sum of their magnitudes and the number of
terms for the bound ``m 2^-53 sum|terms|``."""

import fractions
import math

import numpy as np

from tests.intensity_ref import _ieee_sum

COUNTS = ("count", "count_both", "count_A", "count_B")
SUMS = ("sum_a", "sum_b", "sum_aa", "sum_bb", "sum_ab", "both_a", "both_b", "both_aa", "both_bb", "both_ab", "a_where_B", "b_where_A")
FIELDS = ("count",) + SUMS[:5] + ("count_both",) + SUMS[5:10] + ("count_A", "count_B") + SUMS[10:]
DTYPE_U16 = np.dtype([(f, "<i8" if f in COUNTS else "<u8") for f in FIELDS])
DTYPE_F32 = np.dtype([(f, "<i8" if f in COUNTS else "<f8") for f in FIELDS])
# the count that numbers the terms of each sum, in SUMS order
TERMS_OF = ("count",) * 5 + ("count_both",) * 5 + ("count_B", "count_A")
U = 2.0 ** -53


def _kept(labels, shape, n):
    """``(record index, linear index)`` of the voxels that count: every voxel for object 1 without labels."""
    if labels is None:
        assert n == 1
        size = int(np.prod(shape))
        return np.zeros((size,), np.int64), np.arange(size)
    flat = np.asarray(labels).ravel().astype(np.int64)
    keep = (flat >= 1) & (flat <= n)
    return flat[keep] - 1, np.flatnonzero(keep)


def _masks(a, b, ta, tb):
    """``A = float32(a) > ta``, ``B = float32(b) > tb`` with float32 thresholds: strictly above, a NaN is not."""
    with np.errstate(invalid="ignore"):
        return a.astype(np.float32) > np.float32(ta), b.astype(np.float32) > np.float32(tb)


def pair_u16(labels, a, b, n, ta=0.0, tb=0.0):
    """``n`` records (``DTYPE_U16``): ``np.add.at`` of every voxel's gains in uint64."""
    k, at = _kept(labels, a.shape, n)
    va, vb = a.ravel()[at], b.ravel()[at]
    A, B = _masks(va, vb, ta, tb)
    va, vb = va.astype(np.uint64), vb.astype(np.uint64)
    both = A & B
    zero = np.uint64(0)
    gains = dict(count=np.ones_like(k), count_both=both.astype(np.int64), count_A=A.astype(np.int64), count_B=B.astype(np.int64),
                 sum_a=va, sum_b=vb, sum_aa=va * va, sum_bb=vb * vb, sum_ab=va * vb)
    for f in SUMS[:5]:
        gains["both" + f[3:]] = np.where(both, gains[f], zero)
    gains["a_where_B"], gains["b_where_A"] = np.where(B, va, zero), np.where(A, vb, zero)
    out = np.zeros((n,), dtype=DTYPE_U16)
    for f in FIELDS:
        column = np.zeros((n,), dtype=DTYPE_U16[f])
        np.add.at(column, k, gains[f].astype(DTYPE_U16[f]))
        out[f] = column
    return out


def pair_f32(labels, a, b, n, ta=0.0, tb=0.0):
    """Per record: ``counts`` ((n, 4) int64 in ``COUNTS`` order), ``sums`` ((n, 12) float64 in ``SUMS`` order: the exact sums of
    the exact terms, rounded once; NaN or an infinity where IEEE addition gives one in any order), ``magnitudes`` ((n, 12): the
    sums of the terms' absolute values) and ``terms`` ((n, 12) int64: the number of terms of each sum)."""
    k, at = _kept(labels, a.shape, n)
    a32, b32 = np.asarray(a, np.float32).ravel()[at], np.asarray(b, np.float32).ravel()[at]
    A, B = _masks(a32, b32, ta, tb)
    both = A & B
    va, vb = a32.astype(np.float64), b32.astype(np.float64)
    counts = np.stack([np.bincount(k, weights=w, minlength=n).astype(np.int64) for w in (np.ones(len(k)), both, A, B)], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        five = [va, vb, va * va, vb * vb, va * vb]                    # (inf * 0 is NaN, as in the kernel and the twin)
    # a term that its mask keeps out is not there at all: it is 0 here, whatever the voxel holds
    columns = five + [np.where(both, t, 0.0) for t in five] + [np.where(B, va, 0.0), np.where(A, vb, 0.0)]
    terms = np.stack(columns, axis=1)
    order = np.argsort(k, kind="stable")
    terms = terms[order]
    bounds = np.r_[0, np.cumsum(counts[:, 0])]
    sums, magnitudes = np.zeros((n, 12)), np.zeros((n, 12))
    for r in np.flatnonzero(counts[:, 0] > 0):
        part = terms[bounds[r]:bounds[r + 1]]
        if len(part) == 1:
            sums[r], magnitudes[r] = part[0], np.abs(part[0])
            continue
        if np.isfinite(part).all():
            columns = part.T.tolist()
            sums[r] = [math.fsum(column) for column in columns]
            magnitudes[r] = [math.fsum(map(abs, column)) for column in columns]
            continue
        for c in range(12):
            sums[r, c] = _ieee_sum(part[:, c])
            magnitudes[r, c] = _ieee_sum(np.abs(part[:, c]))
    number = np.stack([counts[:, COUNTS.index(f)] for f in TERMS_OF], axis=1)
    return {"counts": counts, "sums": sums, "magnitudes": magnitudes, "terms": number}


def bound(ref: dict) -> np.ndarray:
    """``m 2^-53 sum|terms|`` per record and sum ((n, 12)), ``m`` the number of terms of that sum."""
    return ref["terms"].astype(np.float64) * U * ref["magnitudes"]


# ---- the coefficients ----


def exact_sqrt(q: fractions.Fraction) -> fractions.Fraction:
    """The square root of a non-negative rational to a relative 2^-120."""
    if q == 0:
        return fractions.Fraction(0)
    shift = 240 + 2 * max(0, q.denominator.bit_length() - q.numerator.bit_length())
    return fractions.Fraction(math.isqrt((q.numerator << shift) // q.denominator), 1 << (shift // 2))


def pearson_exact(n, sa, sb, saa, sbb, sab) -> fractions.Fraction:
    """Pearson's r of exact sums (integers, or floats taken as the rationals they are), to a relative 2^-120."""
    n, sa, sb, saa, sbb, sab = (fractions.Fraction(v) for v in (n, sa, sb, saa, sbb, sab))
    num, da, db = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    assert da > 0 and db > 0
    return num / exact_sqrt(da * db)


def pearson_bound_f32(n, sums, bounds) -> float:
    """How far Pearson's r of sums that lie within ``bounds`` of ``sums`` (``sum_a, sum_b, sum_aa, sum_bb, sum_ab``) can lie
    from r of ``sums``: the first-order propagation through ``r = num / sqrt(da db)``, ``num = N Sab - Sa Sb``, ``da = N Saa -
    Sa^2``, ``db = N Sbb - Sb^2``, doubled for the neglected second-order terms."""
    sa, sb, saa, sbb, sab = (float(v) for v in sums)
    ea, eb, eaa, ebb, eab = (float(v) for v in bounds)
    num, da, db = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    e_num = n * eab + abs(sb) * ea + abs(sa) * eb
    e_da, e_db = n * eaa + 2 * abs(sa) * ea, n * ebb + 2 * abs(sb) * eb
    root = math.sqrt(da * db)
    return 2.0 * (e_num / root + abs(num / root) * (e_da / (2 * da) + e_db / (2 * db)))


# ---- Costes' thresholds ----


def _region_sums(a, b, keep, exact):
    """``(N, Sa, Sb, Saa, Sbb, Sab)`` over ``keep``: Python integers for uint16 data, ``math.fsum`` of exact products else."""
    va, vb = a[keep], b[keep]
    if exact:
        va, vb = [int(v) for v in va.tolist()], [int(v) for v in vb.tolist()]
        return (len(va), sum(va), sum(vb), sum(v * v for v in va), sum(v * v for v in vb), sum(p * q for p, q in zip(va, vb)))
    va, vb = va.astype(np.float64), vb.astype(np.float64)
    return (len(va),) + tuple(math.fsum(t.tolist()) for t in (va, vb, va * va, vb * vb, va * vb))


def costes(labels, a, b, n, region="volume", steps=32):
    """The rule of ``colocalize.costes_thresholds`` over plain arrays: ``{"ta", "tb", "status"}``."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    exact = a.dtype == np.uint16
    if region == "volume":
        keep = np.ones(a.shape, bool)
    else:
        flat = np.asarray(labels).ravel()
        keep = (flat >= 1) & (flat <= n)
    N, sa, sb, saa, sbb, sab = _region_sums(a, b, keep, exact)
    nothing = {"ta": math.nan, "tb": math.nan, "status": "uncorrelated"}
    if N < 2:
        return nothing
    cov_n, va_n, vb_n = N * sab - sa * sb, N * saa - sa * sa, N * sbb - sb * sb
    if not (cov_n > 0 and va_n > 0 and vb_n > 0):
        return nothing
    cov, var_a, var_b = cov_n / (N * N), va_n / (N * N), vb_n / (N * N)
    d = var_b - var_a
    m = (d + math.sqrt(d * d + 4.0 * cov * cov)) / (2.0 * cov)
    c = sb / N - m * (sa / N)

    def thresholds(t):
        ta = np.float32(t)
        return ta, np.float32(m * float(ta) + c)

    def predicate(t):
        ta, tb = thresholds(t)
        A, B = _masks(a, b, ta, tb)
        below = keep & ~(A & B)
        Nb, ua, ub, uaa, ubb, uab = _region_sums(a, b, below, exact)
        if not exact:
            # all minus both, as the rule states it (the float64 sums are subtracted, not summed afresh)
            _, wa, wb, waa, wbb, wab = _region_sums(a, b, keep & A & B, exact)
            ua, ub, uaa, ubb, uab = sa - wa, sb - wb, saa - waa, sbb - wbb, sab - wab
        return Nb * uaa - ua * ua > 0 and Nb * ubb - ub * ub > 0 and Nb * uab - ua * ub > 0

    lo, hi = float(a[keep].min()), float(a[keep].max())
    for _ in range(steps):
        mid = float(np.float32((lo + hi) / 2.0))
        if mid == lo or mid == hi:
            break
        if predicate(mid):
            hi = mid
        else:
            lo = mid
    ta, tb = thresholds(lo)
    return {"ta": float(ta), "tb": float(tb), "status": "ok"}
