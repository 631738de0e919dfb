"""The cases of the intensity tests: the label volumes of ``tests/moments_cases.py`` (by import: its shapes from (1, 1, 1) to
(3, 7, 1030) and its eight contents, sized from the kernel's LDS slots) crossed with value volumes, built once and handed out
read-only, with their restatement (``tests/intensity_ref.py``) computed once."""

import functools

import numpy as np

from tests import intensity_ref as R
from tests import moments_cases as M

SHAPES, CONTENTS, PARAMS, PARAM_IDS, CAPS = M.SHAPES, M.CONTENTS, M.PARAMS, M.PARAM_IDS, M.CAPS
MANY_LABELS, ROW_CROSSING = M.MANY_LABELS, M.ROW_CROSSING
VALUES_F32 = ["constant", "normal", "offset", "cancelling", "signed-zeros", "non-finite"]
VALUES_U16 = ["zeros", "full", "random"]


def labels_of(shape, content, slots):
    return M.case(shape, content, slots)


def _frozen(arr, dtype):
    arr = np.ascontiguousarray(arr, dtype=dtype)
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def values_f32(shape, content, slots, kind):
    """A read-only float32 volume.  ``non-finite`` puts ``+inf``, ``-inf`` and a NaN into voxels of ONE object (the object of the
    first voxel whose label counts), or into the first voxels where no label counts (they must then touch nothing)."""
    voxels = int(np.prod(shape))
    rng = np.random.default_rng(77 * voxels + 7 * CONTENTS.index(content) + VALUES_F32.index(kind))
    if kind == "constant":
        v = np.full(shape, 3.25, np.float32)
    elif kind == "normal":
        v = rng.standard_normal(shape)
    elif kind == "offset":
        v = 1e4 + rng.standard_normal(shape)
    elif kind == "cancelling":
        # pairs +a, -a along the linear index: inside a run and inside most objects the sum cancels to (nearly) nothing
        a = np.repeat(rng.uniform(1.0, 1e3, (voxels + 1) // 2), 2)[:voxels]
        v = (a * np.where(np.arange(voxels) % 2 == 0, 1.0, -1.0)).reshape(shape)
    elif kind == "signed-zeros":
        v = np.where(rng.integers(0, 2, shape) == 0, 0.0, -0.0)
    elif kind == "non-finite":
        labels, n = M.case(shape, content, slots)
        v = rng.standard_normal(shape).astype(np.float32)
        flat = labels.ravel()
        counted = np.flatnonzero((flat >= 1) & (flat <= n))
        at = np.flatnonzero(flat == flat[counted[0]])[:3] if len(counted) else np.arange(min(3, voxels))
        v.ravel()[at] = np.array([np.inf, -np.inf, np.nan], np.float32)[:len(at)]
    else:
        raise KeyError(kind)
    return _frozen(v, np.float32)


@functools.lru_cache(maxsize=None)
def values_u16(shape, content, kind):
    voxels = int(np.prod(shape))
    rng = np.random.default_rng(99 * voxels + 9 * CONTENTS.index(content) + VALUES_U16.index(kind))
    if kind == "zeros":
        v = np.zeros(shape, np.uint16)
    elif kind == "full":
        v = np.full(shape, 65535, np.uint16)
    elif kind == "random":
        v = rng.integers(0, 65536, shape)
    else:
        raise KeyError(kind)
    return _frozen(v, np.uint16)


@functools.lru_cache(maxsize=None)
def want_f32(shape, content, slots, kind):
    """``intensity_ref.intensity_f32`` of the case, with its ``bound``; computed once and not to be changed."""
    labels, n = M.case(shape, content, slots)
    ref = R.intensity_f32(labels, values_f32(shape, content, slots, kind), n)
    ref["bound"] = R.bound(ref)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def want_u16(shape, content, slots, kind):
    labels, n = M.case(shape, content, slots)
    ref = R.intensity_u16(labels, values_u16(shape, content, kind), n)
    ref.setflags(write=False)
    return ref


def check_f32(rows: np.ndarray, ref: dict, what: str) -> None:
    """``rows`` (``INTENSITY_DTYPE_F32``) against the restatement: count and extremes bit for bit (NaNs and signed zeros
    included), every sum within ``2 n_k 2^-53 sum|terms|`` of the exact sum, or NaN / the same infinity where the terms say so;
    the pad zero."""
    assert np.array_equal(rows["count"], ref["count"]), f"{what}: count"
    for f in ("v_min", "v_max"):
        assert np.array_equal(np.ascontiguousarray(rows[f]).view(np.uint32), ref[f].view(np.uint32)), f"{what}: {f}"
    assert not rows["pad"].any(), f"{what}: the pad was written"
    got = np.stack([rows[f] for f in R.SUMS], axis=1) if len(rows) else np.zeros((0, 5))
    want, bound = ref["sums"], ref["bound"]
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN sums"
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), f"{what}: infinite sums"
    error = np.abs(got[finite] - want[finite])
    worst = np.max(error - bound[finite], initial=-np.inf)
    print(f"{what}: worst error / bound = {np.max(error / np.where(bound[finite] > 0, bound[finite], 1.0), initial=0.0):.3g}")
    assert worst <= 0.0, f"{what}: a sum is {worst:.3g} outside its bound"
