"""What the intensities of a volume are: exact order statistics, quantiles, moments and the rescale (``csrc/stats.hip``; the
rule is stated in ``csrc/stats.hpp``, ``tests/stats_ref.py`` restates it in numpy).

A quantile of 8e8 voxels is a radix select: pass ``d`` histograms digit ``d`` of the keys that carry the prefix a rank has
reached (``lsr_digit_histogram_f32`` / ``_u16``, up to ``K`` ranks a pass), the tables come to the host, and the walk from the
tables to the next prefixes is integer work here -- one synchronisation per pass.  Pass 0 has the empty prefix, so it is run
once for any number of ranks and also accumulates the moment record.  The counters are not zeroed by the entry: a set of
volumes is walked once per pass and pools into one multiset.

CPU tensors run the host twins, HIP tensors the kernels; there is no torch fallback.
"""

from __future__ import annotations

import collections
import ctypes
import math

import numpy as np

from . import _lib

FORM_RUNS = 0
FORM_PLAIN = 1
RECORD_WORDS = 5

# (pass, form) -> launches since the module was loaded, ("flush", form) -> those with a flush period: what the tests' census reads
CENSUS: collections.Counter = collections.Counter()


def geometry() -> dict:
    """The kernels' constants (``lsr_volume_stats_geometry``): ``digit_bits``, ``bins``, ``K`` (ranks a pass serves),
    ``threads``, ``wave_step`` and ``step`` (voxels a wave / a workgroup takes per stride), ``default_grid_cap``, ``lds_bytes``,
    ``passes_f32`` and ``passes_u16``."""
    out = (ctypes.c_int64 * 8)()
    _lib.call("lsr_volume_stats_geometry", out)
    bits, bins, k, threads, wave_step, cap, lds, passes = (int(v) for v in out)
    return {"digit_bits": bits, "bins": bins, "K": k, "threads": threads, "wave_step": wave_step, "step": wave_step * threads // 64,
            "default_grid_cap": cap, "lds_bytes": lds, "passes_f32": passes, "passes_u16": -(-16 // bits)}


class _Pool:
    """``vols`` as a re-iterable of flat, contiguous, aligned float32 / uint16 tensors of one type on one device (empty ones
    dropped).  A tensor is a pool of one; a list or any other re-iterable is walked again by every pass and only ever holds
    the volume it is at (a store can be pooled without being resident); a one-shot iterator is kept as a list.  ``dtype`` and
    ``device`` are those of the first volume, known once a walk has begun; ``total`` counts the voxels of the last walk."""

    def __init__(self, vols):
        import torch

        if isinstance(vols, torch.Tensor):
            vols = [vols]
        elif iter(vols) is vols:
            vols = list(vols)
        self._vols, self.dtype, self.device, self.total = vols, None, None, 0

    def __iter__(self):
        import torch

        self.total = 0
        for v in self._vols:
            if not isinstance(v, torch.Tensor) or v.dtype not in (torch.float32, torch.uint16):
                raise TypeError(f"a volume must be a float32 or uint16 torch.Tensor, got {getattr(v, 'dtype', type(v).__name__)}")
            if self.dtype is None:
                self.dtype, self.device = v.dtype, v.device
            if v.dtype != self.dtype or v.device != self.device:
                raise ValueError("pooled volumes must share one dtype and one device")
            if v.numel() == 0:
                continue
            v = v.contiguous().reshape(-1)
            if v.data_ptr() % 16:
                v = v.clone()                   # (a view that starts inside an allocation: the kernels load 16 bytes at once)
            self.total += v.numel()
            yield v

    @property
    def np_dtype(self):
        import torch

        return np.uint16 if self.dtype == torch.uint16 else np.float32

    @property
    def passes(self) -> int:
        g = geometry()
        return g["passes_u16"] if self.np_dtype == np.uint16 else g["passes_f32"]


def digit_histogram(vol, pass_index: int, prefixes, table_of_rank, tables, moments=None, grid_cap: int = 0, form: int = FORM_RUNS,
                    flush_strides: int = 0) -> None:
    """The raw entry: one digit pass over ``vol`` (a flat float32 / uint16 tensor) into ``tables`` (an int64 tensor of
    ``len(prefixes) * bins`` words on ``vol``'s device, NOT zeroed here) and, in pass 0, into ``moments`` (an int64 tensor of 5
    words, not zeroed either).  ``prefixes`` and ``table_of_rank`` are host integers, one per rank.  ``flush_strides`` makes a
    workgroup flush its LDS tables every so many strides (the tests' way to that flush)."""
    import torch

    k = len(prefixes)
    pre = np.ascontiguousarray(prefixes, dtype=np.uint32)
    tab = np.ascontiguousarray(table_of_rank, dtype=np.int32)
    if len(tab) != k:
        raise ValueError("prefixes and table_of_rank must have one entry per rank")
    entry = "lsr_digit_histogram_f32" if vol.dtype == torch.float32 else "lsr_digit_histogram_u16"
    args = (vol.data_ptr(), vol.numel(), int(pass_index), pre.ctypes.data, tab.ctypes.data, k, tables.data_ptr(),
            None if moments is None else moments.data_ptr(), int(grid_cap), int(form) | int(flush_strides) << 8)
    CENSUS[(int(pass_index), int(form))] += 1
    if flush_strides:
        CENSUS[("flush", int(form))] += 1
    if vol.device.type == "cpu":
        _lib.call(entry + "_cpu", *args, None)
        return
    with torch.cuda.device(vol.device):
        _lib.call(entry, *args, _lib.stream_ptr(vol.device))


def _words(t) -> np.ndarray:
    """A device or host int64 tensor as host uint64 words (on a device this is the pass's one synchronisation)."""
    return t.cpu().numpy().view(np.uint64).copy()


def _pass0(pool: _Pool, grid_cap: int = 0, form: int = FORM_RUNS):
    """Pass 0 over every volume: the one table (uint64[bins]) and the pooled raw moment record (uint64[5]); zeros for a pool
    without a voxel."""
    import torch

    g = geometry()
    tables = record = None
    for v in pool:
        if tables is None:
            tables = torch.zeros((g["bins"],), dtype=torch.int64, device=v.device)
            record = torch.zeros((RECORD_WORDS,), dtype=torch.int64, device=v.device)
        if v.dtype == torch.uint16 and pool.total > (2**64 - 1) // 65535**2:
            raise _lib.LsrUnsupported("stats", _lib.E_UNSUPPORTED, "65535^2 n must stay below 2^64 for the pooled uint16 sums to fit")
        digit_histogram(v, 0, [0], [0], tables, record, grid_cap, form)
    if tables is None:
        return np.zeros(g["bins"], np.uint64), np.zeros(RECORD_WORDS, np.uint64)
    return _words(tables), _words(record)


def _walk(table: np.ndarray, rank: int) -> tuple[int, int]:
    """The digit whose bin holds 0-based ``rank`` of the table's multiset, and the rank inside that bin."""
    below = 0                                               # (Python integers: exact at any count)
    for digit, held in enumerate(table.tolist()):
        if rank < below + held:
            return digit, rank - below
        below += held
    raise ValueError(f"rank {rank} lies outside a table of {below} keys")


def _select(pool: _Pool, ranks: list[int], table0: np.ndarray, grid_cap: int = 0, form: int = FORM_RUNS) -> dict[int, int]:
    """rank -> key for every rank of ``ranks`` (distinct, inside the multiset), continuing from pass 0's table."""
    import torch

    g = geometry()
    passes, bins, K = pool.passes, g["bins"], g["K"]
    keys: dict[int, int] = {}
    ranks = sorted(set(ranks))
    for at in range(0, len(ranks), K):
        group = ranks[at:at + K]
        state = [_walk(table0, r) for r in group]            # (prefix, rank inside the prefix) per rank
        for p in range(1, passes):
            distinct = sorted({prefix for prefix, _ in state})
            table_of = [distinct.index(prefix) for prefix, _ in state]
            tables = torch.zeros((len(group) * bins,), dtype=torch.int64, device=pool.device)
            for v in pool:
                digit_histogram(v, p, [prefix for prefix, _ in state], table_of, tables, None, grid_cap, form)
            words = _words(tables).reshape(len(group), bins)
            nxt = []
            for (prefix, r), t in zip(state, table_of):
                digit, r = _walk(words[t], r)
                nxt.append((prefix << g["digit_bits"] | digit, r))
            state = nxt
        for r, (key, _) in zip(group, state):
            keys[r] = key
    return keys


def key_values(keys, dtype) -> np.ndarray:
    """Keys back to values: ``dtype`` float32 (``label.hpp``'s ``key_float``) or uint16 (the key itself)."""
    k = np.asarray(keys, dtype=np.uint64).astype(np.uint32)
    if np.dtype(dtype) == np.uint16:
        return k.astype(np.uint16)
    bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return bits.view(np.float32)


def _decode_record(record: np.ndarray, dtype) -> dict:
    """The raw record as count, nan_count, sum, sum_sq (float64 or exact Python integers), min, max, mean, std."""
    count, nans = int(record[0]), int(record[1])
    if np.dtype(dtype) == np.float32:
        total, total_sq = (float(v) for v in record[2:4].view(np.float64))
    else:
        total, total_sq = int(record[2]), int(record[3])
    out = {"count": count, "nan_count": nans, "sum": total, "sum_sq": total_sq}
    if count == 0:
        out.update(min=math.nan, max=math.nan, mean=math.nan, std=math.nan)
        return out
    codes = record[4:5].view(np.uint32)
    lo, hi = key_values([int(~codes[0])], dtype)[0], key_values([int(codes[1])], dtype)[0]
    with np.errstate(all="ignore"):
        mean = np.float64(total) / np.float64(count)
        variance = np.float64(total_sq) / np.float64(count) - mean * mean
        std = np.sqrt(variance if not variance < 0.0 else np.float64(0.0))
    out.update(min=lo.item(), max=hi.item(), mean=float(mean), std=float(std))
    return out


def moments(vols, _grid_cap: int = 0, _form: int = FORM_RUNS) -> dict:
    """``count`` (non-NaN voxels), ``nan_count``, ``sum``, ``sum_sq``, ``min``, ``max``, ``mean = sum / n`` and the population
    ``std = sqrt(max(sum_sq / n - mean^2, 0))`` of one tensor or a pooled set: one pass.  NaNs are counted and nothing else."""
    pool = _Pool(vols)
    _, record = _pass0(pool, _grid_cap, _form)
    return _decode_record(record, pool.np_dtype)


def order_statistics(vols, ranks, _grid_cap: int = 0, _form: int = FORM_RUNS) -> np.ndarray:
    """The elements at the 0-based ``ranks`` of the sorted multiset of every non-NaN voxel of ``vols`` (one float32 / uint16
    tensor, or a re-iterable of them: pooled), as a numpy array of the volumes' type.  Exact: bit for bit what sorting the keys
    gives (-0.0 below +0.0).  Any number of ranks, served in groups of ``K``; each pass walks ``vols`` once."""
    pool = _Pool(vols)
    ranks = [int(r) for r in ranks]
    table0, _ = _pass0(pool, _grid_cap, _form)
    if not ranks:
        return np.zeros((0,), pool.np_dtype)
    n = int(table0.astype(object).sum())
    if n == 0:
        raise ValueError("no non-NaN voxel: there is no order statistic")
    if min(ranks) < 0 or max(ranks) >= n:
        raise ValueError(f"ranks must lie in 0 .. {n - 1} (the non-NaN voxels), got {min(ranks)} .. {max(ranks)}")
    keys = _select(pool, ranks, table0, _grid_cap, _form)
    return key_values([keys[r] for r in ranks], pool.np_dtype)


def interpolate(a: float, b: float, g: float) -> float:
    """numpy's ``linear`` rule between the bracketing order statistics in float64: ``a + (b - a) g``, and
    ``b - (b - a)(1 - g)`` where ``g >= 0.5``."""
    a, b, g = np.float64(a), np.float64(b), np.float64(g)
    with np.errstate(all="ignore"):
        d = b - a
        return float(b - d * (np.float64(1.0) - g) if g >= 0.5 else a + d * g)


def _bracket(q: float, n: int) -> tuple[int, int, float]:
    h = np.float64(q) * np.float64(n - 1)
    j = int(np.floor(h))
    return j, min(j + 1, n - 1), float(h - np.float64(j))


def _quantiles_from(pool: _Pool, qs, table0, grid_cap, form) -> tuple[list[float], dict]:
    n = int(table0.astype(object).sum())
    qs = [float(q) for q in qs]
    if any(not 0.0 <= q <= 1.0 for q in qs):
        raise ValueError(f"quantiles must lie in [0, 1], got {qs}")
    if n == 0:
        return [math.nan] * len(qs), {}
    brackets = [_bracket(q, n) for q in qs]
    keys = _select(pool, [r for j, j1, _ in brackets for r in (j, j1)], table0, grid_cap, form)
    dtype = pool.np_dtype
    value = {r: key_values([k], dtype)[0].item() for r, k in keys.items()}
    return [interpolate(value[j], value[j1], g) for j, j1, g in brackets], value


def quantiles(vols, qs, _grid_cap: int = 0, _form: int = FORM_RUNS) -> list[float]:
    """numpy's default (``linear``) quantiles of the non-NaN voxels of ``vols`` (pooled), in float64 on the host from the two
    exact bracketing order statistics.  Every quantile of a set without a non-NaN voxel is NaN, after one pass."""
    pool = _Pool(vols)
    table0, _ = _pass0(pool, _grid_cap, _form)
    return _quantiles_from(pool, qs, table0, _grid_cap, _form)[0]


def summary(vols, qs=(), _grid_cap: int = 0, _form: int = FORM_RUNS) -> dict:
    """:func:`moments` and ``quantiles`` ({q: value} for ``qs`` and 0.25, 0.5, 0.75), ``median`` and ``iqr = q75 - q25`` from
    one shared pass 0."""
    pool = _Pool(vols)
    qs = sorted({float(q) for q in qs} | {0.25, 0.5, 0.75})
    table0, record = _pass0(pool, _grid_cap, _form)
    out = _decode_record(record, pool.np_dtype)
    out["quantiles"] = dict(zip(qs, _quantiles_from(pool, qs, table0, _grid_cap, _form)[0]))
    out["median"] = out["quantiles"][0.5]
    out["iqr"] = out["quantiles"][0.75] - out["quantiles"][0.25]
    return out


def rescale(vol, sub: float, div: float, clip=None, out=None):
    """``(float32(vol) - sub) / div`` as a float32 tensor, with ``clip = (lo, hi)`` clamped to it; a NaN stays a NaN.  One
    float32 rounding per step: bit for bit ``np.clip((v.astype(f32) - f32(sub)) / f32(div), lo, hi)``.  ``vol`` is float32 or
    uint16; ``out`` may be ``vol`` itself for a float32 volume (in place)."""
    import torch

    if not isinstance(vol, torch.Tensor) or vol.dtype not in (torch.float32, torch.uint16):
        raise TypeError(f"vol must be a float32 or uint16 torch.Tensor, got {getattr(vol, 'dtype', type(vol).__name__)}")
    if not vol.is_contiguous():
        raise ValueError("vol must be contiguous")
    if out is None:
        out = torch.empty(vol.shape, dtype=torch.float32, device=vol.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == vol.device and out.shape == vol.shape
              and out.is_contiguous()):
        raise ValueError("out must be a contiguous float32 tensor of vol's shape on vol's device")
    if vol.numel() == 0:
        return out
    lo, hi = (0.0, 0.0) if clip is None else (float(clip[0]), float(clip[1]))
    entry = "lsr_rescale_f32" if vol.dtype == torch.float32 else "lsr_rescale_u16"
    args = (vol.data_ptr(), vol.numel(), float(sub), float(div), int(clip is not None), lo, hi, out.data_ptr())
    if vol.device.type == "cpu":
        _lib.call(entry + "_cpu", *args, None)
    else:
        with torch.cuda.device(vol.device):
            _lib.call(entry, *args, _lib.stream_ptr(vol.device))
    _lib.mark_written(out)
    return out


def normalization(vols, method: str, lower_percentile: float = 1.0, upper_percentile: float = 99.9) -> tuple[float, float, bool]:
    """``(sub, div, degenerate)`` of a method from the statistics of ``vols``: ``percentile`` (``sub = q_lo``,
    ``div = q_hi - q_lo``), ``zscore`` (mean and std) or ``robust`` (median and iqr).  A divisor that is 0 or not finite becomes
    1 and ``degenerate`` is True."""
    if method == "percentile":
        lo, hi = quantiles(vols, [lower_percentile / 100.0, upper_percentile / 100.0])
        sub, div = lo, hi - lo
    elif method == "zscore":
        m = moments(vols)
        sub, div = m["mean"], m["std"]
    elif method == "robust":
        s = summary(vols)
        sub, div = s["median"], s["iqr"]
    else:
        raise ValueError(f"method must be 'percentile', 'zscore' or 'robust', got {method!r}")
    degenerate = not (math.isfinite(div) and div != 0.0 and math.isfinite(sub))
    if not (math.isfinite(div) and div != 0.0):
        div = 1.0
    if not math.isfinite(sub):
        sub = 0.0
    return float(sub), float(div), degenerate


def normalize(vol, method: str = "percentile", lower_percentile: float = 1.0, upper_percentile: float = 99.9, clip: bool = False,
              out=None):
    """``vol`` rescaled by its own statistics (:func:`normalization`, then :func:`rescale`); with ``method='percentile'`` and
    ``clip`` the result is clamped to [0, 1].  Returns ``(tensor, {"sub", "div", "degenerate"})``."""
    if clip and method != "percentile":
        raise ValueError("clip goes with method='percentile' (it clamps to [0, 1])")
    sub, div, degenerate = normalization(vol, method, lower_percentile, upper_percentile)
    return rescale(vol, sub, div, (0.0, 1.0) if clip else None, out), {"sub": sub, "div": div, "degenerate": degenerate}
