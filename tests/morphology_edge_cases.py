"""The cases that aim at the dispatch edges of the sliding-window passes (``csrc/morphology.hpp``, ``csrc/morphology.hip``,
``csrc/peaks.hip``), for ``tests/test_morphology_edges_host.py`` and ``tests/test_morphology_edges_gpu.py``.  Everything is sized
from ``morphology.tiling()`` and ``morphology.dispatch()``: ``R`` the greatest half-width, ``c`` the columns per workgroup of the
strided walk, ``S`` the row segment, ``N`` the last half-width of the narrow instantiation, ``D`` the last one with static LDS,
``G`` the row-workgroup cap, ``ahead(r)`` the rows the instantiation that ``r`` selects reads ahead (``U`` below), ``w = 2r + 1``.

* ``rows-every-width``  every ``rx`` in ``1 .. R`` on a row of ``2R + 3``, and ``2^k - 1, 2^k, 2^k + 1`` on a row of 5 (a window
  wider than the row): the doubling spans of the row kernel at every width.
* ``walk-every-width``  every ``rz`` in ``1 .. R`` on ``(67, 1, c + 1)``; ``ry`` at the borders of the three instantiations on
  ``(2, 67, c + 1)`` (outer slabs, two column tiles per slab).
* ``read-ahead``  per instantiation the first and the last half-width; line lengths ``1, 2, U - 1 .. U + 1, 2U - 1 .. 2U + 1,
  w - 1 .. w + 1, 2w - 1 .. 2w + 1`` along z on ``(L, 1, c + 1)`` and along y on ``(2, L, 1)`` (one live lane); all six ops.
* ``row-segments``  rows of ``S - 1, S, S + 1, 2S, 2S + 1`` at ``rx`` 1 and ``R``: one, two and three staged segments.
* ``row-stride``  ``G``, ``G + 1`` and ``3G`` rows of 3: a workgroup's first, second and third row; and ``G + 1`` rows of
  ``S + 1``, two segments each -- the one large case (it cannot be smaller: the cap fixes the row count, two segments the row
  length), held to scipy alone because the restatement loops over ``r`` offsets of the whole volume.
* ``peak-sink``  ``lsr_local_max_candidates_f32`` at ``rz`` of 0, 1, ``N``, ``N + 1`` and 64, with and without the x and y
  passes, at line lengths around the read-ahead depth: a constant (every late bit of every group set), a staircase (a peak at
  every bit position), small integers, signed zeros, a ``+inf`` plateau.
* ``box-smooth``  ``lsr_box_smooth_f32`` at 5, 9, 127 and 129 taps with one axis of exactly ``r + 1``: the mirror's limit.

Oracles.  Morphology: ``scipy.ndimage`` element for element and ``morphology_ref.restated`` byte for byte (NaNs as a mask); both
are kept as digests of their canonical bytes, so that the host and the device tests share one computation without holding every
array.  Peaks: ``psf_ref.peak_mask_literal`` up to 8000 voxels, above that two ``scipy.ndimage.maximum_filter`` calls (the box, and
the window's voxels of smaller C-order index) -- neither shares the doubling scheme of the row kernel, which
``psf_ref._window_max`` does.  Every array is read-only.
"""

import collections
import functools
import hashlib

import numpy as np
import scipy.ndimage as ndi

from shrimpy_amd import morphology as M
from tests import morphology_cases as C
from tests import morphology_ref as R
from tests import psf_ref

CAP, COLUMNS, SEGMENT, _ = M.tiling()
NARROW, STATIC, ROW_GROUPS, AHEAD_NARROW, AHEAD_STATIC, AHEAD_DYNAMIC = M.dispatch()
AHEADS = (AHEAD_NARROW, AHEAD_STATIC, AHEAD_DYNAMIC)

ERODE_DILATE = ("grey_erosion", "grey_dilation")
PLAIN_AND_FUSED = ("grey_erosion", "grey_dilation", "white_tophat", "black_tophat")
TIES = ("noise", "small_integers")


def ahead(r):
    """The rows read ahead by the instantiation of the strided walk that half-width ``r`` selects (``launch_strided``)."""
    return AHEAD_NARROW if r <= NARROW else (AHEAD_STATIC if r <= STATIC else AHEAD_DYNAMIC)


def segments(x):
    """The staged segments of a row of ``x`` in the x pass (``launch_pass``): equal lengths, a multiple of the wavefront."""
    want = -(-x // SEGMENT)
    seg = -(-(-(-x // want)) // COLUMNS) * COLUMNS
    return -(-x // seg)


def rows_of_the_busiest_workgroup(shape):
    rows = shape[0] * shape[1]
    return -(-rows // min(rows, ROW_GROUPS))


# ---- the morphology cases -------------------------------------------------------------------------------------------------------

# restate: also held to morphology_ref.restated (everything but the large row-stride case)
Case = collections.namedtuple("Case", "group shape r ops contents restate")


def powers_of_two_and_neighbours():
    out, k = set(), 1
    while 2 ** k - 1 <= CAP:
        out |= {v for v in (2 ** k - 1, 2 ** k, 2 ** k + 1) if 1 <= v <= CAP}
        k += 1
    return sorted(out)


def line_lengths(r):
    u, w = ahead(r), 2 * r + 1
    return sorted({n for n in (1, 2, u - 1, u, u + 1, 2 * u - 1, 2 * u, 2 * u + 1, w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1)
                   if n > 0})


READ_AHEAD_PAIRS = ((1, NARROW), (NARROW + 1, STATIC), (STATIC + 1, CAP))
READ_AHEAD_CONTENTS = ("noise", "small_integers", "ramp_up", "ramp_down", "inf", "nan", "zeros")
Y_BORDERS = sorted({1, NARROW - 1, NARROW, NARROW + 1, STATIC - 1, STATIC, STATIC + 1, CAP - 1, CAP})
LARGE_SHAPE = (1, ROW_GROUPS + 1, SEGMENT + 1)


def _batches():
    """id -> the cases one parametrized test runs: a group, or a part of it that stays at a few seconds."""
    out = collections.OrderedDict()
    wide, short = (1, 2, 2 * CAP + 3), (1, 2, 5)
    out["rows-every-width/" + "x".join(map(str, wide))] = [Case("rows-every-width", wide, (0, 0, rx), ERODE_DILATE, TIES, True)
                                                           for rx in range(1, CAP + 1)]
    out["rows-every-width/" + "x".join(map(str, short))] = [Case("rows-every-width", short, (0, 0, rx), ERODE_DILATE, TIES, True)
                                                            for rx in powers_of_two_and_neighbours()]
    for u in AHEADS:
        out[f"walk-every-width/z-ahead{u}"] = [Case("walk-every-width", (67, 1, COLUMNS + 1), (rz, 0, 0), ERODE_DILATE, TIES, True)
                                               for rz in range(1, CAP + 1) if ahead(rz) == u]
    out["walk-every-width/y"] = [Case("walk-every-width", (2, 67, COLUMNS + 1), (0, ry, 0), ERODE_DILATE, TIES, True)
                                 for ry in Y_BORDERS]
    for pair in READ_AHEAD_PAIRS:
        for axis in "zy":
            for content in READ_AHEAD_CONTENTS:
                name = content + "_" + axis if content.startswith("ramp") else content
                cases = []
                for r in pair:
                    for n in line_lengths(r):
                        shape, rr = ((n, 1, COLUMNS + 1), (r, 0, 0)) if axis == "z" else ((2, n, 1), (0, r, 0))
                        cases.append(Case("read-ahead", shape, rr, tuple(C.OPS), (name,), True))
                out[f"read-ahead/ahead{ahead(pair[0])}-{axis}-{content}"] = cases
    for rx in (1, CAP):
        out[f"row-segments/rx{rx}"] = [Case("row-segments", (1, 2, x), (0, 0, rx), tuple(C.OPS), TIES, True)
                                       for x in (SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT, 2 * SEGMENT + 1)]
    out["row-stride/rows-of-3"] = [Case("row-stride", shape, (0, 0, rx), tuple(C.OPS), TIES, True)
                                   for shape in ((1, ROW_GROUPS, 3), (1, ROW_GROUPS + 1, 3), (3, ROW_GROUPS, 3)) for rx in (1, 2)]
    for rx in (1, CAP):
        for content in TIES:              # the large case: scipy alone (the restatement loops over r offsets of 8.4 M voxels)
            out[f"row-stride/two-segments-rx{rx}-{content}"] = [Case("row-stride", LARGE_SHAPE, (0, 0, rx), PLAIN_AND_FUSED,
                                                                     (content,), False)]
    return out


BATCHES = _batches()
CASES = [case for cases in BATCHES.values() for case in cases]


def scratch_bytes_of_the_cases():
    from shrimpy_amd import _lib

    return max(_lib.call_value("lsr_grey_morph_scratch_bytes", *shape) for shape in {case.shape for case in CASES})


@functools.lru_cache(maxsize=None)
def _small_volume(shape, content):
    return C.filled(shape, content, np.random.default_rng([*shape, C.CONTENTS.index(content)]))


@functools.lru_cache(maxsize=2)
def _large_volume(shape, content):
    return C.filled(shape, content, np.random.default_rng([*shape, C.CONTENTS.index(content)]))


def volume(shape, content):
    """The float32 volume of a case (read-only, cached; of the one large shape only the two last used)."""
    return (_large_volume if shape == LARGE_SHAPE else _small_volume)(shape, content)


def _digest(bits):
    return hashlib.blake2b(np.ascontiguousarray(bits).tobytes(), digest_size=16).digest()


def bytes_digest(a):
    """What ``morphology_ref.same_bytes`` compares: the bytes, every NaN as the canonical one."""
    bits = np.array(a, dtype=np.float32).view(np.uint32)
    bits[np.isnan(a)] = R.QUIET_NAN
    return _digest(bits)


def value_digest(a):
    """What ``np.array_equal(..., equal_nan=True)`` compares: the values, ``-0.0`` as ``+0.0`` and every NaN as one."""
    with np.errstate(invalid="ignore"):
        return bytes_digest(np.asarray(a, dtype=np.float32) + np.float32(0.0))


def scipy_answer(shape, content, r, op):
    with np.errstate(invalid="ignore"):
        out = R.SCIPY[op](volume(shape, content), size=tuple(2 * k + 1 for k in r))
    assert out.dtype == np.float32
    return out


@functools.lru_cache(maxsize=None)
def expected_digests(shape, content, r, op):
    """``(bytes_digest of the restatement, value_digest of scipy's answer or None on the NaN case)``, computed once."""
    return (bytes_digest(R.restated(volume(shape, content), r, op)),
            None if content == "nan" else value_digest(scipy_answer(shape, content, r, op)))


def check(case, content, op, got):
    """``got`` against the case's oracles, as ``morphology_ref.check`` holds the cases of ``tests/morphology_cases.py``: scipy
    element for element (no voxel excluded; the NaNs an ``inf - inf`` makes must sit where scipy's do), the restatement byte for
    byte with NaNs as a mask, a NaN of an erosion .. closing the canonical one."""
    shape, r = case.shape, case.r
    what = f"{case.group} {shape} {content} r={r} {op}"
    assert got.shape == shape and got.dtype == np.float32
    if not case.restate:
        assert content != "nan"
        assert np.array_equal(got, scipy_answer(shape, content, r, op), equal_nan=True), f"{what}: differs from scipy"
        assert not np.isnan(got).any()
        return
    want_bytes, want_values = expected_digests(shape, content, r, op)
    if bytes_digest(got) != want_bytes:
        want = R.restated(volume(shape, content), r, op)
        assert R.same_bytes(got, want), f"{what}: differs from the restatement at {int((got.view(np.uint32) != want.view(np.uint32)).sum())} voxels"
    if any(r) and not op.endswith("tophat"):
        assert np.all(got.view(np.uint32)[np.isnan(got)] == R.QUIET_NAN), f"{what}: a NaN that is not the canonical one"
    if content != "nan":
        if value_digest(got) != want_values:
            assert np.array_equal(got, scipy_answer(shape, content, r, op), equal_nan=True), f"{what}: differs from scipy"
        if content != "inf":
            assert not np.isnan(got).any(), what


# ---- the peak sink --------------------------------------------------------------------------------------------------------------

PEAK_RZ = (0, 1, NARROW, NARROW + 1, 64)
PEAK_RYX = ((0, 0), (1, 2))
PEAK_CONTENTS = ("constant", "staircase", "small_integers", "zeros", "inf")
LITERAL_VOXELS = 8000
# per content: (a threshold equal to a value of the volume -- the `>=` edge --, a threshold below every value)
PEAK_THRESHOLDS = {"constant": (2.5, 0.0), "staircase": (0.0, -1.0e6), "small_integers": (1.0, -3.0), "zeros": (0.0, -1.0),
                   "inf": (float("inf"), -3.0)}

PeakCase = collections.namedtuple("PeakCase", "shape r content threshold")


def peak_lengths(rz):
    u = ahead(rz)
    return sorted({1, u, u + 1, 2 * u + 1, 2 * rz + 3})


def _peak_batches():
    out = collections.OrderedDict()
    for rz in PEAK_RZ:
        for ry, rx in PEAK_RYX:
            out[f"peak-sink/rz{rz}-ry{ry}-rx{rx}"] = [PeakCase((n, y, COLUMNS + 1), (rz, ry, rx), content, thr)
                                                      for n in peak_lengths(rz) for y in (1, 3) for content in PEAK_CONTENTS
                                                      for thr in PEAK_THRESHOLDS[content]]
    return out


PEAK_BATCHES = _peak_batches()
PEAK_CASES = [case for cases in PEAK_BATCHES.values() for case in cases]


@functools.lru_cache(maxsize=None)
def peak_volume(shape, content):
    """``constant``: 2.5.  ``staircase``: column ``k = y * X + x`` falls off by one per voxel from its single strict maximum 0 at
    ``z = k mod Z``.  ``inf``: small integers with two ``+inf`` pairs, neighbours along z and along x (in reach of each other
    wherever that axis has a window).  ``small_integers`` and ``zeros`` as in ``tests/morphology_cases.py``."""
    nz, ny, nx = shape
    if content == "staircase":
        k = np.arange(ny * nx).reshape(1, ny, nx)
        v = -np.abs(np.arange(nz).reshape(nz, 1, 1) - k % nz).astype(np.float32)
    elif content == "inf":
        v = np.array(peak_volume(shape, "small_integers"))
        v[0, 0, 5] = v[min(1, nz - 1), 0, 5] = np.inf
        v[nz - 1, ny - 1, 10] = v[nz - 1, ny - 1, 11] = np.inf
    else:
        v = np.array(C.filled(shape, content, np.random.default_rng([*shape, len(content)])))
        if content == "constant":
            assert np.all(v == np.float32(2.5))
    v = np.ascontiguousarray(v, dtype=np.float32)
    v.setflags(write=False)
    return v


def peak_mask_scipy(s, r, threshold):
    """The detection rule of ``tests/psf_ref.py`` with scipy's filters: the greatest value of the box clipped to the volume
    (outside does not compete: ``-inf``), and the greatest over the window's voxels of smaller C-order index -- a footprint
    that is the first half of the flattened box.  For NaN-free volumes without ``-inf``."""
    s = np.asarray(s, dtype=np.float32)
    clipped = [min(k, n - 1) for k, n in zip(r, s.shape)]
    size = tuple(2 * k + 1 for k in clipped)
    box = ndi.maximum_filter(s, size=size, mode="constant", cval=-np.inf)
    before = np.zeros(size, dtype=bool)
    before.flat[:before.size // 2] = True                        # (the centre of an odd box is its middle element)
    mask = (s >= np.float32(threshold)) & (s >= box)
    if before.any():
        mask &= ~(ndi.maximum_filter(s, footprint=before, mode="constant", cval=-np.inf) >= s)
    return mask


def peak_oracle_is_literal(shape):
    return int(np.prod(shape)) <= LITERAL_VOXELS


@functools.lru_cache(maxsize=None)
def expected_peaks(case):
    """The linear indices of the case's peaks, ascending (read-only): by the definition's triple loop on a small volume, by
    scipy's filters on a larger one."""
    s = peak_volume(case.shape, case.content)
    assert not np.isnan(s).any() and not np.isneginf(s).any()
    mask = (psf_ref.peak_mask_literal if peak_oracle_is_literal(case.shape) else peak_mask_scipy)(s, case.r, case.threshold)
    lin = np.flatnonzero(mask).astype(np.int64)
    lin.setflags(write=False)
    return lin


# ---- the box smoothing ----------------------------------------------------------------------------------------------------------

BOX_TAPS = (5, 9, 127, 129)


def box_shape(taps):
    r = taps // 2
    return (r + 1, r + 2, r + 1 + COLUMNS)
