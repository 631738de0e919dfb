"""Colocalization of two channels, per object and per volume (``csrc/coloc.hip``; the rule in ``csrc/coloc.hpp``).

* :func:`pair_table` -- one pass over a label volume (or none: the whole volume is object 1) and two value volumes of one type
  (float32 or uint16) with two thresholds: per object the count, the five sums ``a, b, a^2, b^2, a b``, the same where both
  channels are above their thresholds, the counts above each threshold and the sums of each channel where the other is above.
  uint16 sums are exact integers; float64 sums are within ``m 2^-53 sum|terms|`` of the exact sum.  On CPU tensors the host
  twin runs (``csrc/host_twins.hip``).  PARITY UNPINNED: the rule is the specification, ``tests/coloc_ref.py`` restates it.
* :func:`coefficients` -- Pearson (all voxels, and the voxels above both thresholds), Manders' M1 and M2, the overlap
  coefficient with k1 and k2, and the fractions of voxels above the thresholds, per record.
* :func:`costes_thresholds` -- Costes' automatic thresholds as a stated rule: a bisection along the orthogonal-regression line
  for the point below which the two channels stop being positively correlated, one kernel launch per step.

Not built: the 2-D cytofluorogram, Costes' randomisation test, Spearman's rank correlation and the ICQ, thresholds per object,
two channels of different types, multi-GPU tables."""

from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from .segment import _check_volume, _run, _same_volume, _shape3

__all__ = ["COLOC_DTYPE_F32", "COLOC_DTYPE_U16", "COLOC_FIELDS", "COEFFICIENTS", "coloc_geometry", "pair_table", "coefficients",
           "costes_thresholds"]

# one record of the table for float32 and for uint16 values (csrc/coloc.hpp ``RecordF32``, ``RecordU16``)
COLOC_COUNTS = ("count", "count_both", "count_A", "count_B")
COLOC_FIELDS = ("count", "sum_a", "sum_b", "sum_aa", "sum_bb", "sum_ab", "count_both", "both_a", "both_b", "both_aa", "both_bb",
                "both_ab", "count_A", "count_B", "a_where_B", "b_where_A")
COLOC_DTYPE_F32 = np.dtype([(f, "<i8" if f in COLOC_COUNTS else "<f8") for f in COLOC_FIELDS])
COLOC_DTYPE_U16 = np.dtype([(f, "<i8" if f in COLOC_COUNTS else "<u8") for f in COLOC_FIELDS])
assert COLOC_DTYPE_F32.itemsize == 128 and COLOC_DTYPE_U16.itemsize == 128
# the columns of :func:`coefficients`, in order
COEFFICIENTS = ("pearson", "pearson_above", "manders_m1", "manders_m2", "overlap", "k1", "k2", "fraction_both", "a_in_b", "b_in_a")
COSTES_STEPS = 32


def coloc_geometry() -> tuple[int, int]:
    """``(LDS table slots per workgroup, default cap of the grid)`` of the kernel (``lsr_label_coloc_geometry``)."""
    out = (ctypes.c_int * 2)()
    _lib.call("lsr_label_coloc_geometry", out)
    return int(out[0]), int(out[1])


def _check_pair(labels, n, a, b):
    """The checked arguments of a launch: ``(labels or None, n, a, b, (z, y, x))``."""
    import torch

    n = int(n)
    if n < 0:
        raise ValueError(f"n must not be negative, got {n}")
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.uint16):
            raise TypeError(f"{name} must be a float32 or uint16 torch.Tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if a.dtype != b.dtype:
        raise TypeError(f"a is {a.dtype} and b is {b.dtype}: the two channels must have one type")
    a, b = _check_volume(a, "a", a.dtype), _check_volume(b, "b", b.dtype)
    _same_volume(a, b, "a", "b")
    if labels is not None:
        labels = _check_volume(labels, "labels", torch.int32)
        _same_volume(a, labels, "a", "labels")
    elif n != 1:
        raise ValueError(f"without labels the whole volume is object 1: n must be 1, got {n}")
    return labels, n, a, b, _shape3(a, "a")


def _thresholds(thresholds) -> tuple[float, float]:
    ta, tb = (float(np.float32(v)) for v in thresholds)
    if math.isnan(ta) or math.isnan(tb):
        raise ValueError(f"a threshold is NaN: {thresholds!r}")
    return ta, tb


def pair_table(labels, n: int, a, b, thresholds=(0.0, 0.0), _max_blocks: int = 0) -> np.ndarray:
    """The ``n`` records of ``lsr_label_coloc_f32`` / ``_u16`` as a host structured array (``COLOC_DTYPE_F32`` /
    ``COLOC_DTYPE_U16``, by the channels' type).

    ``labels`` is a (Z, Y, X) int32 tensor or ``None`` (then ``n`` must be 1 and every voxel belongs to object 1); ``a`` and
    ``b`` are two tensors of that shape and of one type, float32 or uint16, on the same device (CPU or HIP).  ``thresholds =
    (ta, tb)`` are rounded to float32; a voxel is above where ``float32(a) > ta`` (strictly; a NaN is not above).  Record
    ``label - 1`` holds ``count``; ``sum_a, sum_b, sum_aa, sum_bb, sum_ab``; ``count_both`` and ``both_a .. both_ab`` over the
    voxels above both thresholds; ``count_A``, ``count_B``; ``a_where_B`` and ``b_where_A``.  Labels outside ``1 .. n`` are
    ignored; a label that no voxel carries has zeros.  ``_max_blocks`` caps the grid (0: the kernel's default)."""
    import torch

    labels, n, a, b, (z, y, x) = _check_pair(labels, n, a, b)
    ta, tb = _thresholds(thresholds)
    entry, dtype = (("lsr_label_coloc_f32", COLOC_DTYPE_F32) if a.dtype == torch.float32 else ("lsr_label_coloc_u16", COLOC_DTYPE_U16))
    if n == 0:
        return np.zeros((0,), dtype=dtype)
    table = torch.zeros((n * dtype.itemsize,), dtype=torch.uint8, device=a.device)     # the host zeroes it
    _run(a.device, entry, None if labels is None else labels.data_ptr(), a.data_ptr(), b.data_ptr(), z, y, x, n,
         ctypes.c_float(ta), ctypes.c_float(tb), table.data_ptr(), int(_max_blocks))
    return table.cpu().numpy().view(dtype).copy()


def _moments(n, sa, sb, saa, sbb, sab):
    """``(numerator of cov, of var_a, of var_b)`` over ``N^2``: exact integers from integers, float64 arithmetic from floats."""
    return n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb


def _ratio(num, den) -> float:
    """``num / den`` rounded once (Python's integer division is correctly rounded), NaN where ``den`` is 0."""
    return num / den if den != 0 else math.nan


def _pearson_exact(n, sa, sb, saa, sbb, sab) -> float:
    """Pearson's r from integer sums: numerator and the two bracketed denominators exact, each rounded once; then one product,
    one square root and one division."""
    num, da, db = _moments(n, sa, sb, saa, sbb, sab)
    if da <= 0 or db <= 0:
        return math.nan
    return float(num) / math.sqrt(float(da) * float(db))


def coefficients(table: np.ndarray) -> dict:
    """The colocalization coefficients of every record of a :func:`pair_table`, as a dict of float64 arrays (``COEFFICIENTS``):

    ``pearson = (N Sab - Sa Sb) / sqrt((N Saa - Sa^2)(N Sbb - Sb^2))`` over all voxels of the object, ``pearson_above`` the same
    over the voxels above both thresholds (the ``both_*`` sums and ``count_both``); ``manders_m1 = a_where_B / sum_a``,
    ``manders_m2 = b_where_A / sum_b``; ``overlap = Sab / sqrt(Saa Sbb)``, ``k1 = Sab / Saa``, ``k2 = Sab / Sbb``;
    ``fraction_both = count_both / count``, ``a_in_b = count_both / count_A``, ``b_in_a = count_both / count_B``.

    A column is NaN where its denominator is 0 or ``count < 2``.  For a uint16 table the numerators and the bracketed
    denominators are formed in Python integers (exact) and rounded once, so Pearson of uint16 data carries only the roundings
    of one square root, one product and one division; for a float32 table everything is float64 arithmetic on the sums."""
    table = np.asarray(table)
    if table.dtype not in (COLOC_DTYPE_F32, COLOC_DTYPE_U16):
        raise TypeError("table must be a COLOC_DTYPE_F32 or COLOC_DTYPE_U16 array (pair_table's result)")
    table = table.ravel()
    out = {name: np.full((len(table),), np.nan, dtype=np.float64) for name in COEFFICIENTS}
    if table.dtype == COLOC_DTYPE_U16:
        for i, r in enumerate(table.tolist()):
            (n, sa, sb, saa, sbb, sab, nb, ba, bb, baa, bbb, bab, na, nbb, awb, bwa) = (int(v) for v in r)
            if n < 2:
                continue
            out["pearson"][i] = _pearson_exact(n, sa, sb, saa, sbb, sab)
            out["pearson_above"][i] = _pearson_exact(nb, ba, bb, baa, bbb, bab)
            out["manders_m1"][i] = _ratio(awb, sa)
            out["manders_m2"][i] = _ratio(bwa, sb)
            out["overlap"][i] = float(sab) / math.sqrt(float(saa) * float(sbb)) if saa > 0 and sbb > 0 else math.nan
            out["k1"][i] = _ratio(sab, saa)
            out["k2"][i] = _ratio(sab, sbb)
            out["fraction_both"][i] = _ratio(nb, n)
            out["a_in_b"][i] = _ratio(nb, na)
            out["b_in_a"][i] = _ratio(nb, nbb)
        return out

    def column(f):
        return np.ascontiguousarray(table[f]).astype(np.float64)

    def pearson(n, sa, sb, saa, sbb, sab):
        da, db = n * saa - sa * sa, n * sbb - sb * sb
        return _divide(n * sab - sa * sb, np.sqrt(np.where((da > 0) & (db > 0), da * db, np.nan)))

    def _divide(num, den):
        return num / np.where(den == 0, np.nan, den)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        n = column("count")
        out["pearson"] = pearson(n, *(column(f) for f in ("sum_a", "sum_b", "sum_aa", "sum_bb", "sum_ab")))
        out["pearson_above"] = pearson(column("count_both"), *(column(f) for f in ("both_a", "both_b", "both_aa", "both_bb", "both_ab")))
        out["manders_m1"] = _divide(column("a_where_B"), column("sum_a"))
        out["manders_m2"] = _divide(column("b_where_A"), column("sum_b"))
        saa, sbb, sab = column("sum_aa"), column("sum_bb"), column("sum_ab")
        out["overlap"] = _divide(sab, np.sqrt(saa * sbb))
        out["k1"], out["k2"] = _divide(sab, saa), _divide(sab, sbb)
        out["fraction_both"] = _divide(column("count_both"), n)
        out["a_in_b"] = _divide(column("count_both"), column("count_A"))
        out["b_in_a"] = _divide(column("count_both"), column("count_B"))
        for name in COEFFICIENTS:
            out[name] = np.where(n < 2, np.nan, out[name])
    return out


def _totals(table: np.ndarray) -> dict:
    """The sums of all records, field by field: Python integers for a uint16 table, ``math.fsum`` for a float32 table."""
    integer = table.dtype == COLOC_DTYPE_U16
    out = {}
    for f in COLOC_FIELDS:
        column = np.ascontiguousarray(table[f])
        out[f] = sum(int(v) for v in column.tolist()) if integer or f in COLOC_COUNTS else _fsum(column)
    return out


def _fsum(column: np.ndarray) -> float:
    return math.fsum(column.tolist()) if np.isfinite(column).all() else float(np.sum(column))


def regression_line(totals: dict):
    """``(slope, intercept)`` of the orthogonal regression of b on a from the region's total sums, or ``None`` where the
    covariance is not positive or a variance is zero (or not a number): the first step of :func:`costes_thresholds`."""
    n = totals["count"]
    if n < 2:
        return None
    cov_n, va_n, vb_n = _moments(n, totals["sum_a"], totals["sum_b"], totals["sum_aa"], totals["sum_bb"], totals["sum_ab"])
    if not (cov_n > 0 and va_n > 0 and vb_n > 0):
        return None
    nn = n * n
    cov, var_a, var_b = cov_n / nn, va_n / nn, vb_n / nn
    if not (cov > 0.0 and math.isfinite(var_a) and math.isfinite(var_b)):
        return None
    d = var_b - var_a
    m = (d + math.sqrt(d * d + 4.0 * cov * cov)) / (2.0 * cov)
    c = totals["sum_b"] / n - m * (totals["sum_a"] / n)
    return m, c


def below_is_correlated(totals: dict, at: dict) -> bool:
    """Costes' predicate: over the voxels that are NOT above both thresholds (all minus both) both variances and the covariance
    are positive -- for uint16 data the signs of exact integers."""
    n = totals["count"] - at["count_both"]
    sa, sb = totals["sum_a"] - at["both_a"], totals["sum_b"] - at["both_b"]
    saa, sbb, sab = totals["sum_aa"] - at["both_aa"], totals["sum_bb"] - at["both_bb"], totals["sum_ab"] - at["both_ab"]
    cov_n, va_n, vb_n = _moments(n, sa, sb, saa, sbb, sab)
    return bool(va_n > 0 and vb_n > 0 and cov_n > 0)


def line_thresholds(t: float, m: float, c: float) -> tuple[float, float]:
    """``ta = float32(T)``, ``tb = float32(m ta + c)`` as Python floats."""
    ta = float(np.float32(t))
    with np.errstate(over="ignore"):
        return ta, float(np.float32(m * ta + c))


def costes_thresholds(labels, n: int, a, b, region: str = "volume") -> dict:
    """Costes' automatic thresholds for the channels ``a`` and ``b`` over ``region``: ``"volume"`` (every voxel; ``labels`` may be
    ``None``) or ``"labelled"`` (the voxels whose label lies in ``1 .. n``).  Returns ``{"ta", "tb", "status", "slope",
    "intercept", "launches"}``; ``status`` is ``"ok"`` or ``"uncorrelated"`` (then the thresholds are NaN).

    The rule.  From the region's total sums form ``var_a``, ``var_b`` and ``cov`` (the numerators over ``N^2``; exact integers
    for uint16 data).  If ``cov <= 0`` or a variance is 0 the channels are ``uncorrelated``.  Otherwise the orthogonal-regression
    line is ``m = (var_b - var_a + sqrt((var_b - var_a)^2 + 4 cov^2)) / (2 cov)``, ``c = mean_b - m mean_a``.  For a candidate
    ``T``: ``ta = float32(T)``, ``tb = float32(m ta + c)``; the sums "below" are all minus both-above; ``P(T)`` is true where
    both below-variances and the below-covariance are positive.  Bisection with ``lo = min(a)``, ``hi = max(a)`` over the region
    (``segment.intensity_table``): ``mid = float32((lo + hi) / 2)``; stop when ``mid`` equals an end or after 32 steps; ``P(mid)``
    true moves ``hi`` to ``mid``, false moves ``lo``.  The result is ``lo`` with its ``tb``.  ``P`` need not be monotone: the
    rule is this bisection.  Every evaluation is one launch of the kernel (at most 34 launches in all, the extremes included);
    ``"labelled"`` sums the per-object records on the host."""
    import torch

    from .segment import intensity_table

    if region not in ("volume", "labelled"):
        raise ValueError(f"region must be 'volume' or 'labelled', got {region!r}")
    if region == "labelled" and labels is None:
        raise ValueError("region 'labelled' needs labels")
    labels, n, a, b, _ = _check_pair(labels, n if labels is not None else 1, a, b)
    launches = 0

    def sums(thresholds):
        nonlocal launches
        launches += 1
        if region == "volume":
            return _totals(pair_table(None, 1, a, b, thresholds))
        return _totals(pair_table(labels, n, a, b, thresholds))

    result = {"ta": math.nan, "tb": math.nan, "status": "uncorrelated", "slope": math.nan, "intercept": math.nan}
    totals = sums((0.0, 0.0))
    line = regression_line(totals)
    if line is None:
        return dict(result, launches=launches)
    m, c = line
    if region == "volume":
        extremes = intensity_table(torch.ones(a.shape, dtype=torch.int32, device=a.device), 1, a)
    else:
        extremes = intensity_table(labels, n, a)
    launches += 1
    live = extremes["count"] > 0
    lo, hi = float(extremes["min"][live].min()), float(extremes["max"][live].max())
    for _ in range(COSTES_STEPS):
        mid = float(np.float32((lo + hi) / 2.0))
        if mid == lo or mid == hi:
            break
        if below_is_correlated(totals, sums(line_thresholds(mid, m, c))):
            hi = mid
        else:
            lo = mid
    ta, tb = line_thresholds(lo, m, c)
    return {"ta": ta, "tb": tb, "status": "ok", "slope": m, "intercept": c, "launches": launches}
