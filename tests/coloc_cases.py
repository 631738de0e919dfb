"""The cases of the colocalization tests: the label volumes of ``tests/moments_cases.py`` (by import: its shapes from (1, 1, 1) to
(3, 7, 1030) and its eight contents, sized from the kernel's LDS slots), and the form without labels on the same shapes, crossed
with pairs of value volumes and with thresholds; built once and handed out read-only, with their restatement
(``tests/coloc_ref.py``) computed once."""

import functools

import numpy as np

from tests import coloc_ref as R
from tests import intensity_cases as I
from tests import moments_cases as M

SHAPES, CONTENTS, CAPS = M.SHAPES, M.CONTENTS, M.CAPS
NO_LABELS = "no-labels"                   # labels = None, n = 1
PARAMS = M.PARAMS + [(shape, NO_LABELS) for shape in SHAPES]
PARAM_IDS = ["x".join(map(str, shape)) + "-" + content for shape, content in PARAMS]
MANY_LABELS, ROW_CROSSING = M.MANY_LABELS, M.ROW_CROSSING
PAIRS_F32 = ["independent", "linear", "offset", "cancelling", "signed-zeros", "non-finite"]
WELL_CONDITIONED = ("independent", "linear")
PAIRS_U16 = ["zeros", "full", "random", "equal"]
# thresholds by name; "at-value" is a pair of values that occur in the two volumes, which pins the strict `>`
THRESHOLDS_F32 = ["zero", "at-value", "everything", "nothing"]
THRESHOLDS_U16 = THRESHOLDS_F32 + ["half"]


def labels_of(shape, content, slots):
    """``(labels or None, n)``."""
    if content == NO_LABELS:
        return None, 1
    return M.case(shape, content, slots)


def _frozen(arr, dtype):
    arr = np.ascontiguousarray(arr, dtype=dtype)
    arr.setflags(write=False)
    return arr


def _index(content):
    return (CONTENTS + [NO_LABELS]).index(content)


@functools.lru_cache(maxsize=None)
def pair_f32(shape, content, slots, kind):
    """Two read-only float32 volumes.  ``non-finite`` puts ``+inf``, ``-inf`` and a NaN into channel a of ONE object
    (``intensity_cases.values_f32``'s volume; without labels into the first voxels); channel b stays finite."""
    voxels = int(np.prod(shape))
    rng = np.random.default_rng(55 * voxels + 5 * _index(content) + PAIRS_F32.index(kind))
    if kind == "independent":
        a, b = rng.standard_normal(shape), rng.standard_normal(shape)
    elif kind == "linear":
        a = rng.standard_normal(shape)
        b = 0.5 * a + 0.25 * rng.standard_normal(shape)
    elif kind == "offset":
        a, b = 1e4 + rng.standard_normal(shape), 1e4 + rng.standard_normal(shape)
    elif kind == "cancelling":
        # pairs +v, -v along the linear index in both channels, b's pairs shifted by one voxel: the products cancel too
        v = np.repeat(rng.uniform(1.0, 1e3, (voxels + 1) // 2), 2)[:voxels]
        w = np.repeat(rng.uniform(1.0, 1e3, (voxels + 2) // 2), 2)[1:voxels + 1]
        a = (v * np.where(np.arange(voxels) % 2 == 0, 1.0, -1.0)).reshape(shape)
        flip = np.where((np.arange(voxels) + 1) // 2 % 2 == 0, 1.0, -1.0)          # every other pair of b the other way round
        b = (w * flip * np.where(np.arange(voxels) % 2 == 1, 1.0, -1.0)).reshape(shape)
    elif kind == "signed-zeros":
        a = np.where(rng.integers(0, 2, shape) == 0, 0.0, -0.0)
        b = np.where(rng.integers(0, 2, shape) == 0, 0.0, -0.0)
    elif kind == "non-finite":
        if content == NO_LABELS:
            a = rng.standard_normal(shape).astype(np.float32)
            a.ravel()[:3] = np.array([np.inf, -np.inf, np.nan], np.float32)[:min(3, voxels)]
        else:
            a = I.values_f32(shape, content, slots, "non-finite")
        b = rng.standard_normal(shape)
    else:
        raise KeyError(kind)
    return _frozen(a, np.float32), _frozen(b, np.float32)


@functools.lru_cache(maxsize=None)
def pair_u16(shape, content, kind):
    voxels = int(np.prod(shape))
    rng = np.random.default_rng(66 * voxels + 6 * _index(content) + PAIRS_U16.index(kind))
    if kind == "zeros":
        a, b = np.zeros(shape, np.uint16), np.zeros(shape, np.uint16)
    elif kind == "full":
        a, b = np.full(shape, 65535, np.uint16), np.full(shape, 65535, np.uint16)
    elif kind == "random":
        a, b = rng.integers(0, 65536, shape), rng.integers(0, 65536, shape)
    elif kind == "equal":
        a = rng.integers(0, 65536, shape)
        b = a
    else:
        raise KeyError(kind)
    return _frozen(a, np.uint16), _frozen(b, np.uint16)


def thresholds_of(a, b, name):
    """``(ta, tb)`` as Python floats (exact float32 values)."""
    if name == "zero":
        return 0.0, 0.0
    if name == "at-value":
        # the middle of the finite values that occur: voxels equal to it are NOT above
        fa, fb = a[np.isfinite(a)], b[np.isfinite(b)]
        return (float(np.sort(fa, axis=None)[fa.size // 2]) if fa.size else 0.0,
                float(np.sort(fb, axis=None)[fb.size // 2]) if fb.size else 0.0)
    if name == "everything":
        return -np.inf, -np.inf
    if name == "nothing":
        return np.inf, 0.0
    if name == "half":
        return -1.0, 32767.5
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def want_f32(shape, content, slots, kind, threshold):
    """``coloc_ref.pair_f32`` of the case, with its ``bound``; computed once and not to be changed."""
    labels, n = labels_of(shape, content, slots)
    a, b = pair_f32(shape, content, slots, kind)
    ref = R.pair_f32(labels, a, b, n, *thresholds_of(a, b, threshold))
    ref["bound"] = R.bound(ref)
    for arr in ref.values():
        arr.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def want_u16(shape, content, slots, kind, threshold):
    labels, n = labels_of(shape, content, slots)
    a, b = pair_u16(shape, content, kind)
    ref = R.pair_u16(labels, a, b, n, *thresholds_of(a, b, threshold))
    ref.setflags(write=False)
    return ref


def sums_of(rows: np.ndarray) -> np.ndarray:
    return np.stack([rows[f] for f in R.SUMS], axis=1) if len(rows) else np.zeros((0, 12))


def check_f32(rows: np.ndarray, ref: dict, what: str) -> float:
    """``rows`` (``COLOC_DTYPE_F32``) against the restatement: the four counts exactly, every sum within ``m 2^-53 sum|terms|`` of
    the exact sum, or NaN / the same infinity where the terms say so.  Returns the worst error over its bound."""
    for j, f in enumerate(R.COUNTS):
        assert np.array_equal(rows[f], ref["counts"][:, j]), f"{what}: {f}"
    got, want, bound = sums_of(rows), ref["sums"], ref["bound"]
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN sums"
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), f"{what}: infinite sums"
    error = np.abs(got[finite] - want[finite])
    worst = np.max(error - bound[finite], initial=-np.inf)
    ratio = float(np.max(error / np.where(bound[finite] > 0, bound[finite], 1.0), initial=0.0))
    assert worst <= 0.0, f"{what}: a sum is {worst:.3g} outside its bound"
    return ratio


# ---- scenes with known answers ----


def shifted_boxes(dtype):
    """Channel a is 3 in a box of (4, 6, 8) voxels, channel b is 5 in the same box shifted by half its width along x, in a
    (6, 10, 20) volume; both 0 elsewhere.  ``(a, b, box voxels, overlap voxels)``."""
    a, b = np.zeros((6, 10, 20), dtype), np.zeros((6, 10, 20), dtype)
    a[1:5, 2:8, 4:12] = 3
    b[1:5, 2:8, 8:16] = 5
    return _frozen(a, dtype), _frozen(b, dtype), 4 * 6 * 8, 4 * 6 * 4


@functools.lru_cache(maxsize=None)
def costes_scene(dtype_name):
    """A (6, 20, 48) scene: two independent noisy backgrounds around 100 and 120 (sigma 5), and one block of shared signal 400 to
    2000 with ``b = 0.8 a`` and a little noise.  ``(a, b, structure mask)``."""
    rng = np.random.default_rng(20)
    shape = (6, 20, 48)
    a, b = rng.normal(100.0, 5.0, shape), rng.normal(120.0, 5.0, shape)
    structure = np.zeros(shape, bool)
    structure[1:5, 4:16, 8:32] = True
    signal = rng.uniform(400.0, 2000.0, shape)
    a = np.where(structure, signal, a)
    b = np.where(structure, 0.8 * signal + rng.normal(0.0, 4.0, shape), b)
    if dtype_name == "uint16":
        a, b = np.rint(a), np.rint(b)
    structure.setflags(write=False)
    return _frozen(a, np.dtype(dtype_name)), _frozen(b, np.dtype(dtype_name)), structure


@functools.lru_cache(maxsize=None)
def costes_want(dtype_name, region):
    a, b, structure = costes_scene(dtype_name)
    return R.costes(structure.astype(np.int32), a, b, 1, region)
