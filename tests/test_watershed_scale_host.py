"""The watershed AT SCALE on the host (``tests/watershed_scale_cases.py``): that the cases cross what they say they cross, asserted
from ``csrc/watershed.hip``'s own exported launch geometry; that no basin is long (the GPU tests rely on it); the twins against
the numpy restatement (``tests/watershed_ref.py``) at these sizes.

The basins of every case are compared with ``watershed_ref.basins`` in full (1.6 s, 2.2 s and 4.9 s of numpy for
``merge_wrap`` under 6 and 26 and ``voxel_wrap`` under 6).  The saddles of ``merge_wrap`` under 6 are compared with
``watershed_ref.saddles`` in full (3.3 s); under 26 that takes 13.5 s and on ``voxel_wrap`` about as long, so for those two the
twin is compared with the restatement on a SUB-VOLUME of the same arrays here, and ``tests/test_watershed_scale_gpu.py`` holds the
kernel to the twin.

Not crossed: ``watershed_local_kernel``'s tile wrap needs a column of ``8 * 2^22`` voxels and ``watershed_merge_kernel``'s wrap
``n > 2^26`` -- tens of millions of voxels under a slow reference; their loops have the form of the labelling's, which
``tests/test_label_scale_gpu.py`` pins.  PARITY UNPINNED: the restatement is the reference.
"""

import functools

import numpy as np
import pytest

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from shrimpy_amd import watershed as W
from tests import label_scale_cases as LC
from tests import watershed_cases as SMALL
from tests import watershed_ref as R
from tests import watershed_scale_cases as C

GUARD = 64
FILL = -7
# the saddles: (case, connectivity, the sub-volume the twin meets the restatement on -- None: the whole volume)
SADDLE_PARAMS = [("merge_wrap", 6, None), ("merge_wrap", 26, (slice(None), slice(0, 400), slice(None))),
                 ("voxel_wrap", 6, (slice(0, 9), slice(0, 1500), slice(None)))]
SADDLE_IDS = [f"{n}-{k}" for n, k, _ in SADDLE_PARAMS]


@functools.lru_cache(maxsize=None)
def scratch():
    """One scratch buffer of the module's own for every call, poisoned and never cleared: ``chunks * 4 + n`` bytes of the largest case."""
    need = max(_lib.call_value("lsr_watershed_scratch_bytes", *C.shape(name)) for name in C.NAMES)
    n = max(C.crossings(name)["n"] for name in C.NAMES)
    assert need == LC.ceil_div(n, C.C) * 4 + LC.ceil_div(n, 4) * 4
    return np.full(need, 0xA5, dtype=np.uint8)


def twin_watershed(objects, surface, connectivity):
    """The twin through the C ABI into a buffer pre-filled with -7 with 64 guard words behind it: (basins, B, guard)."""
    objects = np.ascontiguousarray(objects, dtype=np.int32)
    surface = np.ascontiguousarray(surface, dtype=np.float32)
    z, y, x = objects.shape
    assert 0 < _lib.call_value("lsr_watershed_scratch_bytes", z, y, x) <= scratch().nbytes
    buf = np.full(objects.size + GUARD, FILL, dtype=np.int32)
    count = np.full(1, FILL, dtype=np.int32)
    _lib.call("lsr_watershed_f32_cpu", objects.ctypes.data, surface.ctypes.data, z, y, x, connectivity, buf.ctypes.data,
              count.ctypes.data, scratch().ctypes.data, None)
    return buf[:objects.size].reshape(objects.shape), int(count[0]), buf[objects.size:]


def saddle_capacity(pairs):
    """The power of two the small tests size their table with."""
    return 1 << int(2 * pairs + 16).bit_length()


def twin_saddles(objects, basins, surface, connectivity, capacity):
    """The twin's table (``capacity`` zeroed slots between two guards of 64 words of -7): (records, counts, guards)."""
    objects = np.ascontiguousarray(objects, dtype=np.int32)
    basins = np.ascontiguousarray(basins, dtype=np.int32)
    surface = np.ascontiguousarray(surface, dtype=np.float32)
    z, y, x = objects.shape
    buf = np.full(2 * GUARD + 4 * capacity, FILL, dtype=np.int32)
    buf[GUARD:GUARD + 4 * capacity] = 0
    counts = np.full(2 + GUARD, FILL, dtype=np.int32)
    _lib.call("lsr_watershed_saddles_f32_cpu", objects.ctypes.data, basins.ctypes.data, surface.ctypes.data, z, y, x, connectivity,
              capacity, buf[GUARD:].ctypes.data, counts.ctypes.data, None)
    return buf[GUARD:GUARD + 4 * capacity].view(W.SADDLE_DTYPE), counts[:2].tolist(), np.concatenate(
        [buf[:GUARD], buf[GUARD + 4 * capacity:], counts[2:]])


def sorted_records(rows):
    """The claimed slots of a table as ``(pair uint64 ascending, key uint32)`` (and a check that no pair sits in two slots): the
    set of records, in arrays -- a dictionary of millions of tuples is slow and large."""
    rows = rows[rows["pair"] != 0]
    assert not rows["unused"].any()
    order = np.argsort(rows["pair"], kind="stable")
    pair, key = np.ascontiguousarray(rows["pair"][order]), np.ascontiguousarray(rows["key"][order])
    assert np.all(pair[1:] != pair[:-1]), "a pair claimed two slots"
    return pair, key


def sorted_dictionary(table):
    """``watershed_ref.saddles``' dictionary in the form of :func:`sorted_records`."""
    ab = np.array(list(table.keys()), dtype=np.uint64).reshape(len(table), 2)
    pair = ab[:, 0] << np.uint64(32) | ab[:, 1]
    key = np.fromiter(table.values(), dtype=np.int64, count=len(table)).astype(np.uint32)
    order = np.argsort(pair, kind="stable")
    return np.ascontiguousarray(pair[order]), np.ascontiguousarray(key[order])


@functools.lru_cache(maxsize=None)
def reference_saddles(name, connectivity):
    """``(basins, pair, key, what they are)`` of a whole case, once: the restatement where it can be afforded; where it cannot,
    the twins (which this module holds to the restatement: the basins in full, the saddles on a sub-volume)."""
    c = C.case(name)
    if [s for n, k, s in SADDLE_PARAMS if (n, k) == (name, connectivity)][0] is None:
        basins = C.safe_basins(name, connectivity)[0]
        return (basins,) + sorted_dictionary(R.saddles(c["objects"], basins, c["surface"], connectivity)) + ("the restatement",)
    basins, n, _ = twin_watershed(c["objects"], c["surface"], connectivity)
    assert 0 < np.bincount(basins.ravel())[1:].max() < C.MAX_BASIN, "a long basin must not reach the device"
    capacity = saddle_capacity(2 * n)
    while True:                                                 # (a table that is too small says so: come back with a larger one)
        rows, counts, guards = twin_saddles(c["objects"], basins, c["surface"], connectivity, capacity)
        assert np.all(guards == FILL)
        if counts[1] == 0:
            break
        capacity *= 2
    pair, key = sorted_records(rows)
    assert len(pair) == counts[0]
    basins.setflags(write=False)
    return basins, pair, key, "the twin"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------


def test_the_cases_cross_the_scan_edge_and_the_cap():
    T, CH, SC, B, TB = C.G
    assert C.G == W.launch_geometry() and min(C.G) >= 1
    assert C.G == S.launch_geometry(), "the two code objects are compiled from one header today"
    small = max(c["objects"].size for c in SMALL.CASES)
    assert LC.ceil_div(small, CH) < SC and LC.ceil_div(small, T) < B
    merge, voxel = C.crossings("merge_wrap"), C.crossings("voxel_wrap")
    # merge_wrap: two counts per scan thread in THIS code object, the last threads idle; nothing else goes round
    assert merge["blocks"] > SC and merge["per"] == 2 and merge["per"] * (SC - 1) > merge["blocks"] and merge["voxel_groups"] <= B
    # voxel_wrap: flatten, final and the saddles go round
    assert voxel["voxel_groups"] > B and voxel["per"] >= 2
    # out of scope, and it shows: the merge walks words of four voxels and the local launch tiles -- neither goes round
    assert voxel["merge_groups"] <= B and voxel["tiles"] <= TB
    for name in C.NAMES:
        c = C.case(name)
        assert c["objects"].shape == c["surface"].shape == C.shape(name) and (c["objects"] == -1).any() and (c["objects"] > 0).any()
    # the sub-volumes of the saddle checks are sub-volumes, with several tiles along every axis that has them
    for name, _, sub in SADDLE_PARAMS:
        if sub is not None:
            shape = C.case(name)["objects"][sub].shape
            assert 0 < np.prod(shape) < C.crossings(name)["n"] and all(n > t for n, t in zip(shape, C.TILE))


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_basins_equal_the_restatement_at_scale_and_no_basin_is_long(name, connectivity):
    case = C.case(name)
    want, n_want, summits, largest = C.case_basins(name, connectivity)
    assert 0 < largest < C.MAX_BASIN
    assert n_want > 4 * C.C and (name != "voxel_wrap" or n_want > 10 ** 6)
    got, n, guard = twin_watershed(case["objects"], case["surface"], connectivity)
    assert np.all(guard == FILL), "the twin wrote behind its output"
    assert not np.any(got == FILL), "a voxel was not written"
    assert n == n_want == summits
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name,connectivity,sub", SADDLE_PARAMS, ids=SADDLE_IDS)
def test_twin_saddles_equal_the_restatement_at_scale(name, connectivity, sub):
    case = C.case(name)
    if sub is None:
        objects, surface = case["objects"], case["surface"]
        basins, *want = reference_saddles(name, connectivity)[:3]
    else:
        objects, surface = np.ascontiguousarray(case["objects"][sub]), np.ascontiguousarray(case["surface"][sub])
        basins, _, _ = R.basins(objects, surface, connectivity)
        want = sorted_dictionary(R.saddles(objects, basins, surface, connectivity))
    rows, counts, guards = twin_saddles(objects, basins, surface, connectivity, saddle_capacity(len(want[0])))
    assert np.all(guards == FILL), "the twin wrote outside the table"
    assert counts == [len(want[0]), 0] and len(want[0]) > 10 ** 5
    got = sorted_records(rows)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
