"""Float64 / exact-integer restatements of the DynaTrack estimator kernels (``csrc/estimators.hip``, host twins in
``csrc/estimators_host.hip``), the case tables that reach every branch of their dispatch, and the assertions both the
host suite (``test_estimators_host.py``: the ``_cpu`` twins) and the device suite (``test_estimators_fp64_gpu.py``)
make.  Plain numpy / scipy, written from the rules in the kernel file's comments; nothing here imports ``shrimpy_amd``.

A *backend* is what a check function drives: numpy arrays in, numpy arrays out, one method per entry point
(``minmax_f32``, ``minmax_u16``, ``histogram``, ``centroid``, ``blur``, ``match``, ``cross``, ``peak``).  ``offset`` is
the number of elements the input view is displaced from a 16-byte aligned allocation (``out_offset``: the output's).

Bounds (none is measured):

* blur: ``2r + 1`` FMAs in ascending tap order on float32 operands: ``|got - ref| <= gamma_n * sum |w| |v|`` with
  ``gamma_n = n u / (1 - n u) <= (n + 1) u`` for ``n (n + 1) u <= 1``, ``u = 2^-24``, ``n = 2r + 1``.
* cross power: two rounded products and one rounded sum per component: ``(2 u + u^2) (|p1| + |p2|) < 3 u (...)``.
* centroid sums: non-negative terms whose products ``w * index`` are exact in a double (24 x 30 bits), added in fp64 in
  any order: relative error ``< N * 2^-53`` of the exact sum, ``N = Z Y X`` (every path from a term to the total passes
  fewer than ``N`` roundings, the one of ``row_sum * z`` included; for the shapes with ``N <= 3`` the count is 0 or 1).
"""

from __future__ import annotations

import functools
import math

import numpy as np

from oracle.cpu_ref import dt_histc

U24 = 2.0 ** -24
U53 = 2.0 ** -53

FORMS = ("contiguous", "marching", "packed", "tiled-128", "tiled-64")     # the codes of lsr_blur_reflect_form
BLUR_MAX_R = 64


# ------------------------------------------------------------------------------------------------ restatements
def minmax(x) -> np.ndarray:
    """{min, max} over the samples that are not NaN (fminf / fmaxf skip a NaN operand); none at all: (+inf, -inf)."""
    x = np.asarray(x).ravel()
    x = x[~np.isnan(x)] if x.dtype.kind == "f" else x
    if x.size == 0:
        return np.array([np.inf, -np.inf], np.float32)
    return np.array([x.min(), x.max()]).astype(np.float32)


def histogram(x, nbins, vmin, vmax) -> np.ndarray:
    """``torch.histc`` in its float32 arithmetic (``oracle.cpu_ref.dt_histc``) as integer counts."""
    with np.errstate(invalid="ignore"):
        return dt_histc(x, nbins, vmin, vmax).astype(np.int64)


def in_range_count(x, vmin, vmax) -> int:
    x = np.asarray(x, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero((x >= np.float32(vmin)) & (x <= np.float32(vmax))))


def centroid_sums(vol, param, mask: bool) -> np.ndarray:
    """{sum w, sum w z, sum w y, sum w x}: w in float32 as the kernel forms it, the sums exact (``math.fsum``)."""
    vol = np.asarray(vol, np.float32)
    p = np.float32(param)
    w = (vol > p).astype(np.float32) if mask else np.maximum(vol - p, np.float32(0)).astype(np.float32)
    w = w.astype(np.float64)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in vol.shape), indexing="ij", sparse=True)
    return np.array([math.fsum(w.ravel()), math.fsum((w * z).ravel()), math.fsum((w * y).ravel()),
                     math.fsum((w * x).ravel())])


def blur(vol, axis, taps, sub=0.0, div=0.0):
    """(ref, bound operand): the float32 map ``(v - sub) / div`` (``div != 0``), then the mirror correlation in float64,
    and ``correlate1d(|v|, |taps|)``."""
    from scipy import ndimage

    v = np.asarray(vol, np.float32)
    if div != 0.0:
        v = ((v - np.float32(sub)) / np.float32(div)).astype(np.float32)
    v64, t64 = v.astype(np.float64), np.asarray(taps, np.float32).astype(np.float64)
    return (ndimage.correlate1d(v64, t64, axis=axis, mode="mirror"),
            ndimage.correlate1d(np.abs(v64), np.abs(t64), axis=axis, mode="mirror"))


def match_shape(vol, shape):
    """Per axis: reflect-pad with ``d // 2`` on the left, or crop the centre starting at ``d // 2``."""
    out = np.asarray(vol)
    for ax, (ni, no) in enumerate(zip(out.shape, shape)):
        if no > ni:
            pad = [(0, 0)] * out.ndim
            pad[ax] = ((no - ni) // 2, (no - ni) - (no - ni) // 2)
            out = np.pad(out, pad, mode="reflect")
        elif no < ni:
            start = (ni - no) // 2
            out = np.take(out, np.arange(start, start + no), axis=ax)
    return np.ascontiguousarray(out)


def cross_power(a, b):
    """``a * conj(b)`` in complex128 and the two bound operands (real part, imaginary part)."""
    a, b = np.asarray(a, np.complex64).astype(np.complex128), np.asarray(b, np.complex64).astype(np.complex128)
    return (a * np.conj(b), np.abs(a.real * b.real) + np.abs(a.imag * b.imag),
            np.abs(a.imag * b.real) + np.abs(a.real * b.imag))


def peak(vol) -> int:
    """``argmax(fftshift(|v|))``: the first maximum in fftshift order.  (No NaN: numpy's argmax would pick it.)"""
    return int(np.argmax(np.fft.fftshift(np.abs(np.asarray(vol, np.float32)))))


# ------------------------------------------------------------------------------------------------ flat reductions
GRID_THREADS = 2048 * 256          # kBlocks * kThreads: the thread count of a saturated grid
FLAT_N = [1, 3, 4, 5, 255, 1024, 1025, GRID_THREADS * 4 - 1, GRID_THREADS * 4, GRID_THREADS * 4 + 1,
          4 * (4 * GRID_THREADS + 1000) + 3]
FLAT_OFFSETS = (0, 1)
HIST_BINS = (1, 17, 256, 4096)


def flat_positions(n) -> dict:
    """Named elements of a flat array of n floats at which an extreme is planted (aligned walk: vectors of four, four
    vectors ``nthreads`` apart per unrolled step, then single vectors, then a scalar tail)."""
    pos = {"first": 0, "last": n - 1, "middle": n // 2}
    if n % 4 and n > 4:
        pos["tail"] = (n // 4) * 4
    if n // 4 > 3 * GRID_THREADS:           # every thread runs the unrolled step
        t = 12345
        for k, lane in enumerate((0, 3, 1, 2)):
            pos[f"unrolled_{k}"] = 4 * (t + k * GRID_THREADS) + lane
        pos["single"] = 4 * (4 * GRID_THREADS + 777) + 2
    return {k: v for k, v in pos.items() if 0 <= v < n}


def flat_data(n, seed=0) -> np.ndarray:
    return (np.random.default_rng(1000 + seed + n % 9973).random(n, dtype=np.float32) * 600 + 100).astype(np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_minmax_f32(backend, n, offset):
    """Extremes planted at every named position in turn, bit for bit; -0.0, +-inf, scattered NaN."""
    base = flat_data(n)
    names = list(flat_positions(n).items())
    for k, (name, p) in enumerate(names):
        q_name, q = names[(k + 1) % len(names)]
        x = base.copy()
        x[q] = 7777.0
        x[p] = -5.0
        got = backend.minmax_f32(x, offset)
        want = minmax(x)
        assert np.array_equal(_bits(got), _bits(want)), f"n={n} offset={offset} min at {name}, max at {q_name}: {got} != {want}"
        if p != q:
            assert want[0] == -5.0 and want[1] == 7777.0
    p, q = names[-1][1], names[0][1]
    for lo, hi in ((-0.0, None), (None, -0.0), (-np.inf, np.inf)):
        x = base.copy() if lo is not None else -base
        if lo is not None:
            x[p] = lo
        if hi is not None and (q != p or lo is None):
            x[q] = hi
        got = backend.minmax_f32(x, offset)
        assert np.array_equal(_bits(got), _bits(minmax(x))), f"n={n} offset={offset} planted ({lo}, {hi}): {got}"
    x = base.copy()
    rng = np.random.default_rng(n)
    x[rng.random(n) < 0.3] = np.nan
    x[[0, n - 1]] = np.nan
    if n > 4:
        x[n // 3] = -9.0        # at least one sample survives
    got = backend.minmax_f32(x, offset)
    assert np.array_equal(_bits(got), _bits(minmax(x))), f"n={n} offset={offset} with NaN: {got} != {minmax(x)}"


def hist_data(n, vmin, vmax) -> np.ndarray:
    """Samples over [vmin - 10%, vmax + 10%] with vmin, vmax, their float32 neighbours, NaN and +-inf planted."""
    rng = np.random.default_rng(2000 + n % 9973)
    span = vmax - vmin
    x = (rng.random(n) * 1.2 * span + (vmin - 0.1 * span)).astype(np.float32)
    lo, hi = np.float32(vmin), np.float32(vmax)
    special = [hi, lo, np.nextafter(hi, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf)),
               np.nextafter(hi, np.float32(-np.inf)), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]
    where = np.unique(rng.integers(0, n, len(special)))
    x[where] = special[:len(where)]
    if n >= 2:
        x[n - 1] = hi       # the last element (a tail element of the aligned walk) decides the last bin
    return x


@functools.lru_cache(maxsize=4)
def _hist_case(n, nbins, vmin, vmax):
    x = hist_data(n, vmin, vmax)
    x.setflags(write=False)
    return x, histogram(x, nbins, vmin, vmax)


def check_histogram(backend, n, offset, nbins, vmin=100.0, vmax=700.0):
    x, want = _hist_case(n, nbins, vmin, vmax)
    got = backend.histogram(x, offset, vmin, vmax, nbins).astype(np.int64)
    assert got.shape == (nbins,)
    assert np.array_equal(got, want), f"n={n} offset={offset} nbins={nbins}: bins {np.flatnonzero(got != want)[:8]} differ"
    assert int(got.sum()) == in_range_count(x, vmin, vmax), "the counts do not add up to the in-range samples"


def check_histogram_rules(backend):
    """What does not lean on ``dt_histc``: v == vmax lands in the last bin, NaN / +-inf / out-of-range samples are
    dropped, and samples at bin centres give ``np.histogram``'s float64 counts."""
    nbins, vmin, vmax = 17, -3.0, 14.0
    x = np.full(1031, vmax, np.float32)
    got = backend.histogram(x, 0, vmin, vmax, nbins)
    assert got[-1] == x.size and got[:-1].sum() == 0, "v == vmax must fall in the last bin"
    x = np.array([np.nan, np.inf, -np.inf, vmin - 1e-3, vmax + 1e-3, 1e30, -1e30] * 33, np.float32)
    assert backend.histogram(x, 0, vmin, vmax, nbins).sum() == 0, "NaN, +-inf and out-of-range samples are dropped"
    rng = np.random.default_rng(5)
    centres = (vmin + (np.arange(nbins) + 0.5) * (vmax - vmin) / nbins).astype(np.float32)    # exact: width 1
    x = centres[rng.integers(0, nbins, 5003)]
    want = np.histogram(x.astype(np.float64), bins=nbins, range=(vmin, vmax))[0]
    assert np.array_equal(backend.histogram(x, 1, vmin, vmax, nbins).astype(np.int64), want)
    assert np.array_equal(histogram(x, nbins, vmin, vmax), want)


U16_N = [1, 7, 8, 9, 4097, 2097160 + 5]
U16_OFFSETS = (0, 1, 4)


def u16_positions(n) -> dict:
    """Named elements of n uint16 counts: the low / high half of a 32-bit word of a 16-byte load, and the scalar tail."""
    pos = {"first": 0, "last": n - 1}
    if n >= 8:
        pos.update(low_half=((n // 8 // 2) * 8 + 2) % ((n // 8) * 8), high_half=((n // 8 // 2) * 8 + 5) % ((n // 8) * 8))
    if n % 8 and n > 8:
        pos["tail"] = (n // 8) * 8 + (n % 8) // 2
    return {k: v for k, v in pos.items() if 0 <= v < n}


def check_minmax_u16(backend, n, offset):
    base = np.random.default_rng(3000 + n % 9973).integers(100, 60000, n).astype(np.uint16)
    names = list(u16_positions(n).items())
    for k, (name, p) in enumerate(names):
        q_name, q = names[(k + 1) % len(names)]
        x = base.copy()
        x[q] = 65535
        x[p] = 0
        got = backend.minmax_u16(x, offset)
        want = minmax(x)
        assert np.array_equal(_bits(got), _bits(want)), f"n={n} offset={offset} 0 at {name}, 65535 at {q_name}: {got} != {want}"
        if p != q:
            assert tuple(want) == (0.0, 65535.0)
    got = backend.minmax_u16(base, offset)
    assert np.array_equal(_bits(got), _bits(minmax(base))), f"n={n} offset={offset}: {got} != {minmax(base)}"


# ------------------------------------------------------------------------------------------------ centroids
CENTROID_SHAPES = [(1, 1, 1), (1, 3, 1), (1, 5, 255), (2, 2, 256), (3, 3, 257), (1, 8193, 3), (3, 2731, 5), (9, 33, 300)]
CENTROID_KINDS = ("weighted", "mask")


def centroid_data(shape) -> np.ndarray:
    return (np.random.default_rng(4000 + sum(shape)).random(shape) * 800 + 100).astype(np.float32)


def check_centroid(backend, shape, kind):
    """Each of the four sums within N * 2^-53 (relative) of the exact sum; a parameter above the data: four zeros."""
    vol = centroid_data(shape)
    n = vol.size
    worst = 0.0
    inside = float(vol.min()) + 0.37 * float(vol.max() - vol.min()) if n > 1 else float(vol.min()) - 1.0
    for param in (inside, float(vol.max()) + 1.0):
        got = backend.centroid(kind, vol, param)
        want = centroid_sums(vol, param, kind == "mask")
        err = np.abs(got - want)
        bound = n * U53 * want
        assert np.all(err <= bound), f"{kind} {shape} param={param}: sums {got} against {want} (bound {bound})"
        worst = max([worst] + [e / b for e, b in zip(err, bound) if b > 0])
        if param > vol.max():
            assert np.array_equal(got, np.zeros(4)), "all-zero weights"
        else:
            assert want[0] > 0
    return worst


# ------------------------------------------------------------------------------------------------ blur
# (form, input offset, output offset, [(shape, axis, r), ...]): a flat list; test_estimators_host.py asks lsr_blur_reflect_form
# whether each case takes the form it is listed under
_BLUR_TABLE = [
    # the contiguous axis: lengths around the 1024-output row segment (L = 1023, 1024, 1025, 2050), radii around the 8-tap
    # blocks (7, 8, 9), r = 0, r = L - 1, L < 4; last, more (row, segment) items than the 16384 workgroups (the item loop)
    ("contiguous", 0, 0, [
        ((2, 3, 1), 2, 0), ((2, 3, 3), 2, 0), ((2, 3, 3), 2, 1), ((2, 3, 3), 2, 2), ((2, 3, 9), 2, 0),
        ((2, 3, 9), 2, 1), ((2, 3, 9), 2, 7), ((2, 3, 9), 2, 8), ((2, 3, 1023), 2, 0), ((2, 3, 1023), 2, 1),
        ((2, 3, 1023), 2, 7), ((2, 3, 1023), 2, 8), ((2, 3, 1023), 2, 9), ((2, 3, 1023), 2, 28), ((2, 3, 1023), 2, 64),
        ((2, 3, 1024), 2, 0), ((2, 3, 1024), 2, 1), ((2, 3, 1024), 2, 7), ((2, 3, 1024), 2, 8), ((2, 3, 1024), 2, 9),
        ((2, 3, 1024), 2, 28), ((2, 3, 1024), 2, 64), ((2, 3, 1025), 2, 0), ((2, 3, 1025), 2, 1), ((2, 3, 1025), 2, 7),
        ((2, 3, 1025), 2, 8), ((2, 3, 1025), 2, 9), ((2, 3, 1025), 2, 28), ((2, 3, 1025), 2, 64), ((2, 3, 2050), 2, 0),
        ((2, 3, 2050), 2, 1), ((2, 3, 2050), 2, 7), ((2, 3, 2050), 2, 8), ((2, 3, 2050), 2, 9), ((2, 3, 2050), 2, 28),
        ((2, 3, 2050), 2, 64), ((130, 130, 8), 2, 3),
    ]),
    # marching: r <= 12 and L >= 32, on both strided axes; inner = 255, 256, 257 (partial 256-column strips; on axis 0
    # inner = Y * X); one segment (L <= 768) and 512-long segments (L = 769, 1030)
    ("marching", 0, 0, [
        ((32, 5, 51), 0, 0), ((2, 32, 255), 1, 0), ((32, 2, 128), 0, 0), ((2, 32, 256), 1, 0), ((32, 1, 257), 0, 0),
        ((2, 32, 257), 1, 0), ((32, 5, 51), 0, 12), ((2, 32, 255), 1, 12), ((32, 2, 128), 0, 12), ((2, 32, 256), 1, 12),
        ((32, 1, 257), 0, 12), ((2, 32, 257), 1, 12), ((33, 5, 51), 0, 0), ((2, 33, 255), 1, 0), ((33, 2, 128), 0, 0),
        ((2, 33, 256), 1, 0), ((33, 1, 257), 0, 0), ((2, 33, 257), 1, 0), ((33, 5, 51), 0, 12), ((2, 33, 255), 1, 12),
        ((33, 2, 128), 0, 12), ((2, 33, 256), 1, 12), ((33, 1, 257), 0, 12), ((2, 33, 257), 1, 12),
        ((768, 5, 51), 0, 0), ((2, 768, 256), 1, 0), ((768, 1, 257), 0, 12), ((2, 768, 255), 1, 12),
        ((769, 1, 257), 0, 0), ((2, 769, 255), 1, 0), ((769, 2, 128), 0, 12), ((2, 769, 257), 1, 12),
        ((1030, 2, 128), 0, 0), ((2, 1030, 257), 1, 0), ((1030, 5, 51), 0, 12), ((2, 1030, 256), 1, 12),
    ]),
    # packed: 13 <= r <= 28 (its 64 KB of LDS), even inner (2, 128, 130), L > 32 (33, 64, 65, 129)
    ("packed", 0, 0, [
        ((33, 2, 1), 0, 13), ((2, 33, 128), 1, 13), ((33, 2, 65), 0, 13), ((2, 64, 2), 1, 13), ((64, 2, 64), 0, 13),
        ((2, 64, 130), 1, 13), ((65, 2, 1), 0, 13), ((2, 65, 128), 1, 13), ((65, 2, 65), 0, 13), ((2, 129, 2), 1, 13),
        ((129, 2, 64), 0, 13), ((2, 129, 130), 1, 13), ((33, 2, 1), 0, 28), ((2, 33, 128), 1, 28), ((33, 2, 65), 0, 28),
        ((2, 64, 2), 1, 28), ((64, 2, 64), 0, 28), ((2, 64, 130), 1, 28), ((65, 2, 1), 0, 28), ((2, 65, 128), 1, 28),
        ((65, 2, 65), 0, 28), ((2, 129, 2), 1, 28), ((129, 2, 64), 0, 28), ((2, 129, 130), 1, 28),
    ]),
    # the packed shapes with L <= 64 through an input view one float off 16 bytes: tiled-64
    ("tiled-64", 1, 0, [
        ((33, 2, 1), 0, 13), ((2, 33, 128), 1, 13), ((33, 2, 65), 0, 13), ((2, 64, 2), 1, 13), ((64, 2, 64), 0, 13),
        ((2, 64, 130), 1, 13), ((33, 2, 1), 0, 28), ((2, 33, 128), 1, 28), ((33, 2, 65), 0, 28), ((2, 64, 2), 1, 28),
        ((64, 2, 64), 0, 28), ((2, 64, 130), 1, 28),
    ]),
    # ... and those with L > 64: tiled-128
    ("tiled-128", 1, 0, [
        ((65, 2, 1), 0, 13), ((2, 65, 128), 1, 13), ((65, 2, 65), 0, 13), ((2, 129, 2), 1, 13), ((129, 2, 64), 0, 13),
        ((2, 129, 130), 1, 13), ((65, 2, 1), 0, 28), ((2, 65, 128), 1, 28), ((65, 2, 65), 0, 28), ((2, 129, 2), 1, 28),
        ((129, 2, 64), 0, 28), ((2, 129, 130), 1, 28),
    ]),
    # packed shapes with only the output one float off: tiled-64 (L <= 64)
    ("tiled-64", 0, 1, [
        ((33, 2, 65), 0, 13), ((2, 64, 130), 1, 13), ((33, 2, 65), 0, 28), ((2, 64, 130), 1, 28),
    ]),
    # ... and tiled-128 (L > 64)
    ("tiled-128", 0, 1, [
        ((65, 2, 65), 0, 13), ((2, 129, 130), 1, 13), ((65, 2, 65), 0, 28), ((2, 129, 130), 1, 28),
    ]),
    # tiled-128 (L > 64, r <= 60): r = 13, 28 with odd inner (1, 63, 65); r = 29, 60 with inner 64 and 65, L = 65, 128, 129, 200
    ("tiled-128", 0, 0, [
        ((65, 1, 1), 0, 13), ((2, 65, 63), 1, 13), ((65, 1, 65), 0, 13), ((2, 129, 1), 1, 13), ((129, 1, 63), 0, 13),
        ((2, 129, 65), 1, 13), ((65, 1, 1), 0, 28), ((2, 65, 63), 1, 28), ((65, 1, 65), 0, 28), ((2, 129, 1), 1, 28),
        ((129, 1, 63), 0, 28), ((2, 129, 65), 1, 28), ((65, 1, 64), 0, 29), ((2, 65, 65), 1, 29), ((2, 128, 64), 1, 29),
        ((128, 1, 65), 0, 29), ((2, 129, 64), 1, 29), ((129, 1, 65), 0, 29), ((200, 1, 64), 0, 29),
        ((2, 200, 65), 1, 29), ((2, 65, 64), 1, 60), ((65, 1, 65), 0, 60), ((128, 1, 64), 0, 60), ((2, 128, 65), 1, 60),
        ((129, 1, 64), 0, 60), ((2, 129, 65), 1, 60), ((2, 200, 64), 1, 60), ((200, 1, 65), 0, 60),
    ]),
    # tiled-64: r = 61, 64 (L = 65, 200; inner 1, 63, 64, 65); axes too short for the marching form (L = 1, 2, 31 at
    # r = min(12, L - 1)); 13 <= r < L <= 64 where the packed form does not apply
    ("tiled-64", 0, 0, [
        ((65, 1, 1), 0, 61), ((2, 65, 63), 1, 61), ((2, 65, 64), 1, 61), ((65, 1, 65), 0, 61), ((2, 200, 1), 1, 61),
        ((200, 1, 63), 0, 61), ((200, 1, 64), 0, 61), ((2, 200, 65), 1, 61), ((2, 65, 1), 1, 64), ((65, 1, 63), 0, 64),
        ((65, 1, 64), 0, 64), ((2, 65, 65), 1, 64), ((200, 1, 1), 0, 64), ((2, 200, 63), 1, 64), ((2, 200, 64), 1, 64),
        ((200, 1, 65), 0, 64), ((1, 1, 1), 0, 0), ((2, 1, 63), 1, 0), ((2, 1, 64), 1, 0), ((1, 1, 65), 0, 0),
        ((2, 2, 1), 1, 1), ((2, 1, 63), 0, 1), ((2, 1, 64), 0, 1), ((2, 2, 65), 1, 1), ((2, 31, 1), 1, 12),
        ((31, 1, 63), 0, 12), ((31, 1, 64), 0, 12), ((2, 31, 65), 1, 12), ((14, 1, 64), 0, 13), ((2, 64, 63), 1, 13),
        ((32, 1, 64), 0, 20), ((2, 64, 64), 1, 63), ((33, 1, 64), 0, 29), ((2, 32, 130), 1, 13), ((29, 1, 1), 0, 28),
        ((2, 64, 65), 1, 30),
    ]),
]


def _blur_cases():
    cases = []
    for form, offset, out_offset, rows in _BLUR_TABLE:
        for shape, axis, r in rows:
            name = f"{form} {shape} axis {axis} r={r}" + (" offset view" if offset else "") + (" offset output" if out_offset else "")
            cases.append(dict(name=name, form=form, shape=shape, axis=axis, r=r, offset=offset, out_offset=out_offset))
    return cases


BLUR_CASES = _blur_cases()


def blur_inputs(case):
    """(volume, taps): positive samples on a camera-like offset, random positive taps."""
    rng = np.random.default_rng(5000 + sum(case["shape"]) + 7 * case["axis"] + case["r"])
    vol = (rng.random(case["shape"]) * 900 + 100).astype(np.float32)
    taps = (rng.random(2 * case["r"] + 1) + 0.05).astype(np.float32)
    return vol, taps


def check_blur(backend, case) -> float:
    """With and without the fused map: |got - ref| <= (2r + 2) 2^-24 correlate1d(|v|, |taps|); returns the worst ratio."""
    vol, taps = blur_inputs(case)
    worst = 0.0
    for sub, div in ((0.0, 0.0), (float(vol.min()), float(np.float32(vol.max()) - np.float32(vol.min())))):
        if div == 0.0 and sub != 0.0:
            continue        # a one-voxel volume: no range to map
        got = backend.blur(vol, case["axis"], taps, case["r"], sub, div, case["offset"], case["out_offset"])
        ref, operand = blur(vol, case["axis"], taps, sub, div)
        bound = (2 * case["r"] + 2) * U24 * operand
        err = np.abs(got.astype(np.float64) - ref)
        bad = err > bound
        assert not bad.any(), (f"{case['name']} map={div != 0.0}: {int(bad.sum())} voxels beyond the bound, first at "
                               f"{tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r}, want {ref[bad][0]!r}")
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
    return worst


# ------------------------------------------------------------------------------------------------ match shape
MATCH_CASES = [((5, 6, 7), (8, 4, 7)), ((5, 6, 7), (9, 11, 13)), ((5, 6, 7), (13, 16, 19)), ((5, 6, 7), (5, 6, 7)),
               ((5, 6, 7), (12, 3, 8)), ((1, 1, 1), (1, 1, 1)), ((3, 4, 300), (2, 7, 515)), ((300, 230, 3), (301, 231, 2))]
# ((5, 6, 7) -> (13, 16, 19) is the largest pad (so - si + 1) / 2 < si allows on every axis: so = 3 si - 2)


def check_match(backend, si, so):
    vol = np.random.default_rng(6000 + sum(si) + sum(so)).standard_normal(si).astype(np.float32)
    got = backend.match(vol, so)
    want = match_shape(vol, so)
    assert got.shape == tuple(so) == want.shape
    assert np.array_equal(_bits(got), _bits(want)), f"{si} -> {so}: first difference at {tuple(np.argwhere(got != want)[0])}"


# ------------------------------------------------------------------------------------------------ cross power
CROSS_N = [1, 255, 256, 2097152 + 77]


def check_cross(backend, n, into_b) -> float:
    rng = np.random.default_rng(7000 + n % 9973)
    a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    b = (rng.standard_normal(n) * 30 + 1j * rng.standard_normal(n)).astype(np.complex64)
    a_after, b_after = backend.cross(a, b, into_b)
    got, kept, kept_before = (b_after, a_after, a) if into_b else (a_after, b_after, b)
    assert np.array_equal(_bits(kept.view(np.float32)), _bits(kept_before.view(np.float32))), "the other operand changed"
    ref, op_re, op_im = cross_power(a, b)
    err_re, err_im = np.abs(got.real.astype(np.float64) - ref.real), np.abs(got.imag.astype(np.float64) - ref.imag)
    assert np.all(err_re <= 3 * U24 * op_re) and np.all(err_im <= 3 * U24 * op_im), f"n={n} into_b={into_b}"
    return float(max(np.max(err_re / (3 * U24 * op_re)), np.max(err_im / (3 * U24 * op_im))))


# ------------------------------------------------------------------------------------------------ peak
PEAK_SHAPES = [(1, 1, 1), (1, 1, 7), (1, 5, 8), (3, 4, 5), (4, 6, 12), (2, 3000, 4), (5, 7, 515), (6, 9, 516)]


def peak_patterns(shape):
    """name -> [(position, value)]: the volumes of one shape.  Ties are equal |v| of both signs, placed so that the
    raw order and the fftshift order disagree."""
    Z, Y, X = shape
    zw, yw, xw = Z - Z // 2, Y - Y // 2, X - X // 2          # the first index the shift sends to 0
    mid = (Z // 3, Y // 2, (2 * X) // 3)
    out = {"unique": [(mid, 2.0)], "negative": [(mid, 2.0), ((Z - 1, Y - 1, X // 4), -3.0)], "zeros": None}

    def ties(name, positions):
        positions = list(dict.fromkeys(p for p in positions if all(0 <= i < n for i, n in zip(p, shape))))
        if len(positions) >= 2:
            out[name] = [(p, 2.0 if k % 2 else -2.0) for k, p in enumerate(positions)]

    ties("tie same row", [(Z // 2, Y // 2, 0), (Z // 2, Y // 2, X - 1)])
    ties("tie x wrap", [(0, 0, xw - 1), (0, 0, xw)])
    ties("tie rows of different blocks", [(0, 0, X // 2), (Z - 1, Y - 1, X // 2), (Z // 2, 0, X // 2)])
    ties("tie z wrap", [(zw - 1, Y // 3, 1 % X), (zw, Y // 3, 1 % X)])
    ties("tie y wrap", [(0, yw - 1, X - 1), (0, yw, X - 1)])
    ties("tie z and y wrap", [(zw - 1, yw - 1, X // 2), (zw - 1, yw, X // 2), (zw, yw - 1, X // 2), (zw, yw, X // 2)])
    return out


def peak_volume(shape, pattern) -> np.ndarray:
    if pattern is None:
        return np.zeros(shape, np.float32)
    rng = np.random.default_rng(8000 + sum(shape))
    vol = ((rng.random(shape) * 0.5) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    for p, v in pattern:
        vol[p] = v
    return vol


def check_peak(backend, shape):
    """Every pattern of the shape, aligned and -- so that rows of 4 n floats also take the scalar form -- one float off."""
    for name, pattern in peak_patterns(shape).items():
        vol = peak_volume(shape, pattern)
        want = peak(vol)
        if pattern is not None and name.startswith("tie"):
            raw_first = min(np.ravel_multi_index(p, shape) for p, _ in pattern)
            shifted = np.unravel_index(want, shape)
            back = tuple((s - n // 2) % n for s, n in zip(shifted, shape))
            assert np.ravel_multi_index(back, shape) != raw_first, f"{shape} {name}: the case does not tell the orders apart"
        for offset in (0, 1):
            got = backend.peak(vol, offset)
            assert got == want, f"{shape} {name} offset={offset}: index {got}, want {want}"
