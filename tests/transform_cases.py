"""Lengths, inputs, tables and float64 references shared by the per-length pins of the phase and focus transform kernels
(``tests/test_phase_lengths_gpu.py``, ``tests/test_focus_lengths_gpu.py``) and their host counterparts
(``tests/test_phase_host.py``, ``tests/test_focus_host.py``).

``csrc/phase.hip`` and ``csrc/focus.hip`` restate the row-transform wrappers of ``csrc/rfft_rows.hip``; ``focus.hip`` adds a
complex column transform with a full twiddle table.  The originals are pinned at every length in
``tests/test_fft_kernels_fp64_gpu.py``; the lengths, the structured inputs, the row check and its constants are taken from
there, so the copies are held to exactly what the originals are.

Nothing here needs a GPU.  References are float64 NumPy; a table is whatever the test builds -- ``lsr_band_power_f32``
takes any table of closed intervals -- so single bins, self-paired columns and self-mirrored rows can be isolated.
"""

import math

import numpy as np

from tests import phase_ref
from tests.test_fft_kernels_fp64_gpu import (C_L2_ROWS, C_MAX_ROWS, ROW_X, U, WORST, _check_rows, _record,  # noqa: F401
                                             _row_inputs, _smooth)

COL_Y = [n for n in range(2, 2049) if _smooth(n)]            # the rule lsr_band_power_supported states for Yc

SLICE = 25                                                   # lengths per parametrised test


def slices(items):
    return [items[i:i + SLICE] for i in range(0, len(items), SLICE)]


def slice_id(part):
    return f"{part[0]}..{part[-1]}" if not isinstance(part[0], tuple) else f"{part[0][:2]}..{part[-1][:2]}"


class at:
    """``with at(f"X = {x}"):`` -- an assertion that fails inside names the length it failed at."""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        return self

    def __exit__(self, kind, err, tb):
        if kind is not None and issubclass(kind, AssertionError):
            raise AssertionError(f"{self.what}: {err}") from err
        return False


def check_rows(family, got, want, n, scale=None):
    """``_check_rows`` of the FFT sweep with its constants; a set of nothing but zero rows (one sample of a sine) must come
    out zero."""
    if not np.any(want):
        assert np.array_equal(np.asarray(got), np.zeros_like(got)), f"{family}: a zero row is not zero"
        return
    _check_rows(family, got, want, n, C_L2_ROWS, C_MAX_ROWS, scale)


# ---------------------------------------------------------------- phase: geometry and rows


def phase_geometry(i, x):
    """``(Zi, Yi, Xi), (Z, Y, X)`` of the ``i``-th row length: the volume's width rotates over no padding, an odd width,
    padding shorter than the volume, about half, a third (the clamp: the padding is longer than twice the volume) and one
    sample; y over ragged second and third tiles and padding longer than the volume; z likewise."""
    xi = (x, x - 1, x - 3, x // 2 + 1, max(1, x // 3), 1)[i % 6]
    yi, y = ((1, 1), (7, 8), (9, 9), (8, 9), (3, 17))[i % 5]
    zi, z = ((1, 1), (2, 3), (1, 4), (3, 3))[(i // 3) % 4]
    return (zi, yi, xi), (z, y, x)


def row_sets(x_len, width, rows_per_set, rng):
    """The rows of ``_row_inputs`` (impulses, tones, Hermitian-spectrum rows, zero-mean normal rows) dealt into sets of
    ``rows_per_set`` rows: as many sets as it takes to hold all twelve structured rows, ``(sets, rows_per_set, width)``."""
    sets = max(1, -(-12 // rows_per_set))
    return _row_inputs(x_len, width, sets * rows_per_set, rng).reshape(sets, rows_per_set, width)


def phase_volumes(i, x):
    """``(volumes float32 (sets, Zi, Yi, Xi), shape, grid)`` of the ``i``-th row length."""
    shape, grid = phase_geometry(i, x)
    zi, yi, xi = shape
    vols = row_sets(x, xi, zi * yi, np.random.default_rng(x))
    return vols.reshape((-1,) + shape), shape, grid


def phase_grid_rows(i, x):
    """Known rows of the whole grid for the inverse kernel: ``(rows float32 (sets, Z, Y, X), spectrum complex64 in the
    kernel's [Z][XC][Y] layout (sets, Z, XC, Y), shape, grid)`` -- the float64 spectrum rounded to complex64."""
    shape, grid = phase_geometry(i, x)
    z, y, _ = grid
    rows = row_sets(x, x, z * y, np.random.default_rng(5000 + x)).reshape((-1,) + grid)
    spec = np.fft.rfft(rows.astype(np.float64), axis=-1).astype(np.complex64)
    return rows, np.ascontiguousarray(spec.transpose(0, 1, 3, 2)), shape, grid


def forward_reference(vol, grid):
    """float64 ``(Z, Y, XC)``: the DFT of every mirror-extended row of the grid."""
    return np.fft.rfft(phase_ref.extend(vol, grid), axis=2)


def inverse_reference(spec_t, grid, mean):
    """float64 ``(Z, Y, X)`` from a ``[Z][XC][Y]`` complex64 spectrum: ``irfft / (Z Y mean)`` (``irfft`` divides by X)."""
    z, y, x = grid
    return np.fft.irfft(spec_t.transpose(0, 2, 1).astype(np.complex128), n=x, axis=2) / (z * y * mean)


def whole_rows(got, want, shape):
    """The bound is on whole rows of the grid: the cropped part of a row carries no more than the whole, so the columns
    the kernel does not store are taken from the reference."""
    z, y, x = shape
    out = want[:z, :y].copy()
    out[:, :, :x] = np.asarray(got, dtype=np.float64).reshape(shape)
    return out


def mirror_literal(i, n, g):
    """The header of ``csrc/phase.hip``, word for word: ``i < n`` is the sample itself; behind it, with ``a = i - n`` and
    ``b = g - 1 - i``, sample ``n - 1 - min(a, n - 1)`` if ``a <= b``, else sample ``min(b, n - 1)``."""
    if i < n:
        return i
    a, b = i - n, g - 1 - i
    if a <= b:
        return n - 1 - min(a, n - 1)
    return min(b, n - 1)


def mirror_by_padding(v, g):
    """The same extension said another way: the first half (rounded up) of the padding is the volume's end mirrored behind
    it, the rest its beginning mirrored in front of the wrap-around, each continued with the edge value."""
    n = v.shape[0]
    behind, front = -(-(g - n) // 2), (g - n) // 2
    tail = np.pad(np.pad(v, (0, min(behind, n)), mode="symmetric"), (0, max(behind - n, 0)), mode="edge")[n:]
    head = np.pad(np.pad(v, (min(front, n), 0), mode="symmetric"), (max(front - n, 0), 0), mode="edge")[:front]
    return np.concatenate([v, tail, head])


# ---------------------------------------------------------------- focus: geometry, planes, tables

SMALL_Y = (2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16)
SMALL_X = (8, 12, 16, 20, 24, 40)
OFFSETS = ((0, 0), (3, 5), (1, 1), (2, 4))
FOCUS_Z = 3
TONE_AMPLITUDE = 1.0

# (Yc, Xc, index): every row length with a small column, every column length with a small row
FOCUS_ROW_CASES = [(SMALL_Y[i % len(SMALL_Y)], x, i) for i, x in enumerate(ROW_X)]
FOCUS_COL_CASES = [(y, SMALL_X[j % len(SMALL_X)], j) for j, y in enumerate(COL_Y)]


def one_bins(yc, xc):
    """The bins ``(m, kx)`` of the one-bin tables: both self-paired columns, both self-mirrored rows, their crossings, an
    interior bin and a pseudo-random one (seeded by the lengths); duplicates dropped."""
    n, m = yc, xc // 2
    rng = np.random.default_rng(yc * 4099 + xc)
    bins = [(0, 0), (n // 2, m), (n // 2, 0), (0, m), (1, 1), (int(rng.integers(0, n // 2 + 1)), int(rng.integers(0, m + 1)))]
    return list(dict.fromkeys(bins))


def full_table(yc, xc):
    t = np.zeros((xc // 2 + 1, 2), dtype=np.int32)
    t[:, 1] = yc // 2
    return t


def one_bin_table(m, kx):
    """Columns ``0 .. kx``; only the last holds a bin: ``a = b = m`` (the others ``a = 0, b = -1``: empty)."""
    t = np.zeros((kx + 1, 2), dtype=np.int32)
    t[:, 1] = -1
    t[kx] = (m, m)
    return t


def focus_tables(yc, xc):
    """``[(kind, bin or None, table)]``: "full", then the one-bin tables."""
    return [("full", None, full_table(yc, xc))] + [("one bin", b, one_bin_table(*b)) for b in one_bins(yc, xc)]


def tone_bin(yc, xc, index):
    bins = one_bins(yc, xc)
    return bins[index % len(bins)]


def focus_volume(yc, xc, index, planes=FOCUS_Z):
    """``(volume float32 (planes, Yc + 3, Xc + 5) with NaN outside the window, y0, x0, tone bin)``.  Plane 0: standard
    normal; plane 1: ``cos(2 pi (m y / Yc + kx x / Xc))`` at one of the bins under test; plane 2: an impulse at the window's
    last voxel.  Nothing outside the window may be read, so it holds NaN."""
    y0, x0 = OFFSETS[index % len(OFFSETS)]
    rng = np.random.default_rng(yc * 8191 + xc)
    vol = np.full((planes, yc + 3, xc + 5), np.nan, dtype=np.float32)
    win = np.zeros((planes, yc, xc))
    win[0] = rng.standard_normal((yc, xc))
    m, kx = tone_bin(yc, xc, index)
    if planes > 1:
        yy, xx = np.arange(yc)[:, None], np.arange(xc)[None, :]
        win[1] = TONE_AMPLITUDE * np.cos(2 * np.pi * (m * yy / yc + kx * xx / xc))
    if planes > 2:
        win[2, -1, -1] = 1.0
    vol[:, y0:y0 + yc, x0:x0 + xc] = win
    return vol, y0, x0, (m, kx)


def table_mask(table, yc, xc):
    """Boolean ``(Yc, Xc)`` on the FULL spectrum: every bin ``(+-m, +-kx)`` of the table's intervals."""
    mask = np.zeros((yc, xc), dtype=bool)
    for kx, (a, b) in enumerate(np.asarray(table).tolist()):
        m = np.arange(max(a, 0), min(b, yc // 2) + 1)
        ky = np.concatenate([m, (yc - m) % yc])
        mask[ky, kx] = mask[ky, (xc - kx) % xc] = True
    return mask


def power_from_mask(mag, mask):
    """``P[z]``: the magnitudes ``mag`` (planes, Yc, Xc) of the full spectrum added up over the mask."""
    return mag[:, mask].sum(axis=1)


def power_by_weights(mag, table):
    """``P[z]`` on the half spectrum by the weight rule, stated independently of the kernel: a column counts twice for
    ``0 < kx < M`` and once otherwise; a row's mirror ``Yc - m`` is added except at ``m = 0`` and ``2 m = Yc``."""
    planes, yc, xc = mag.shape
    half = xc // 2
    total = np.zeros(planes)
    for kx, (a, b) in enumerate(np.asarray(table).tolist()):
        weight = 2.0 if 0 < kx < half else 1.0
        m = np.arange(max(a, 0), min(b, yc // 2) + 1)
        mirrored = m[(m != 0) & (2 * m != yc)]
        total += weight * (mag[:, m, kx].sum(axis=1) + mag[:, yc - mirrored, kx].sum(axis=1))
    return total


def power_bound(win, weighted):
    """Per plane: ``32 u (log2 Xc + log2 Yc) W sqrt(Yc Xc) rms(plane)`` -- the per-coefficient constant of the LDS
    transforms, per leg, times the weighted number of bins that are added up (``tests/focus_ref.py: bound``)."""
    win = np.asarray(win, dtype=np.float64)
    yc, xc = win.shape[1:]
    rms = np.sqrt(np.mean(win * win, axis=(1, 2)))
    return C_MAX_ROWS * U * (math.log2(xc) + math.log2(yc)) * weighted * math.sqrt(yc * xc) * rms


def tone_allowance(weighted, yc, xc):
    """What rounding the tone to float32 can move its closed form ``A Yc Xc`` by: every sample by at most ``2^-25 A``, so
    every bin by at most ``2^-25 A Yc Xc``, times the weighted bins that are added up."""
    return weighted * 2.0 ** -25 * TONE_AMPLITUDE * yc * xc


class FocusCase:
    """One (Yc, Xc): the volume, its window, the float64 spectrum and, per table, the reference power and the bound."""

    def __init__(self, yc, xc, index, planes=FOCUS_Z, bins=None):
        self.yc, self.xc, self.index = yc, xc, index
        self.vol, self.y0, self.x0, self.tone = focus_volume(yc, xc, index, planes)
        self.win = self.vol[:, self.y0:self.y0 + yc, self.x0:self.x0 + xc]
        assert np.isfinite(self.win).all()
        self.rows = np.fft.rfft(self.win.astype(np.float64), axis=2)             # the x leg: (planes, Yc, M + 1)
        self.mag = np.abs(np.fft.fft2(self.win.astype(np.float64)))
        tables = focus_tables(yc, xc)
        if bins is not None:
            tables = [tables[0]] + [("one bin", b, one_bin_table(*b)) for b in bins]
        self.tables = []
        for kind, b, table in tables:
            mask = table_mask(table, yc, xc)
            weighted = int(mask.sum())
            ref = power_from_mask(self.mag, mask)
            self.tables.append((kind, b, table, weighted, ref, power_bound(self.win, weighted)))

    def check_reference(self):
        """The two statements of the reference agree, the one-bin tables weigh at most four bins, and the tone's power is
        its closed form on its own bin and nothing on the others."""
        assert self.tables[0][3] == self.yc * self.xc
        for kind, b, table, weighted, ref, bound in self.tables:
            by_weights = power_by_weights(self.mag, table)
            assert np.all(np.abs(by_weights - ref) <= 1e-12 * self.mag.sum(axis=(1, 2))), (kind, b)
            if kind == "one bin":
                assert 1 <= weighted <= 4
                if self.win.shape[0] > 1:
                    closed = TONE_AMPLITUDE * self.yc * self.xc if b == self.tone else 0.0
                    assert abs(ref[1] - closed) <= tone_allowance(weighted, self.yc, self.xc), (b, ref[1], closed)

    def check_power(self, family, got, kind, b, weighted, ref, bound, factor=1.0):
        """``|P_got - P_ref| <= factor * bound`` on every plane; on the tone plane also against the closed form."""
        got = np.asarray(got, dtype=np.float64)
        assert np.isfinite(got).all(), f"{kind} {b}: non-finite power"
        ratio = np.abs(got - ref) / bound
        _record(f"{family} {kind}", ratio.max())
        assert np.all(ratio <= factor), f"{kind} {b}: |P - P_ref| / bound = {ratio} (P {got}, P_ref {ref})"
        if kind == "one bin" and got.shape[0] > 1:
            closed = TONE_AMPLITUDE * self.yc * self.xc if b == self.tone else 0.0
            off = abs(got[1] - closed)
            assert off <= factor * bound[1] + tone_allowance(weighted, self.yc, self.xc), \
                f"{kind} {b}: the tone at {self.tone} gives {got[1]}, closed form {closed}"


def check_x_leg(family, got, want, xc):
    """Rows of the x leg (last axis: the kept columns) against the float64 ``rfft`` of the window's rows; the scale is the
    whole reference row's norm."""
    want = np.asarray(want)
    check_rows(family, got, want, xc, scale=np.linalg.norm(want.reshape(-1, want.shape[-1]), axis=1))


def host_twin_power(case, table):
    """``lsr_band_power_f32_cpu`` on the case's volume with the given table."""
    from shrimpy_amd import _lib

    vol = np.ascontiguousarray(case.vol)
    z, y, x = vol.shape
    tab = np.ascontiguousarray(table, dtype=np.int32)
    out = np.full((z,), np.nan)
    _lib.call("lsr_band_power_f32_cpu", vol.ctypes.data, z, y, x, case.y0, case.x0, case.yc, case.xc, None, None, None,
              tab.ctypes.data, tab.shape[0] - 1, None, None, out.ctypes.data, None)
    return out


def longest_pair(supported):
    """The longest (Yc, Xc) ``supported`` accepts, walking the two lists down from (2048, 4096)."""
    return next((y, x) for y in reversed(COL_Y) for x in reversed(ROW_X) if supported(y, x))
