"""The watershed kernels (``csrc/watershed.hip``) on the device: the numpy restatement of the rule (``tests/watershed_ref.py``)
element for element on every case of ``tests/watershed_cases.py`` (sized from the tile of the local launch), every voxel
written and nothing behind the buffer, the same bytes from two calls and from the twin, one uncleared scratch buffer for every
call; the saddle table as a set of records, bit for bit; the merge and the relabelling; ``segment_zyx`` with ``split``.
Every test is a handful of launches on a few ten thousand voxels.  PARITY UNPINNED: the restatement is the reference.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import watershed as W
from tests import test_watershed_host as H
from tests import watershed_cases as C
from tests import watershed_ref as R

pytestmark = pytest.mark.gpu

GUARD = H.GUARD
FILL = H.FILL
_SCRATCH = {}


def _scratch(device):
    """One poisoned scratch buffer for every call of this module, never cleared between them."""
    if device not in _SCRATCH:
        _SCRATCH[device] = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device=device)
    return _SCRATCH[device]


def _d(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)


def device_watershed(objects, surface, connectivity, device, entry="lsr_watershed_f32", extra=()):
    """The kernels through the C ABI into a buffer pre-filled with -7 with 64 guard words behind it: (basins, B, guard)."""
    z, y, x = objects.shape
    scratch = _scratch(device)
    assert 0 < _lib.call_value("lsr_watershed_scratch_bytes", z, y, x) <= scratch.numel()
    d_objects, d_surface = _d(objects, device), _d(surface, device)
    buf = torch.full((objects.size + GUARD,), FILL, dtype=torch.int32, device=device)
    count = torch.full((1,), FILL, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.call(entry, d_objects.data_ptr(), d_surface.data_ptr(), z, y, x, connectivity, buf.data_ptr(), count.data_ptr(),
                  scratch.data_ptr(), *extra, _lib.stream_ptr(device))
    host = buf.cpu().numpy()
    return host[:objects.size].reshape(objects.shape), int(count.cpu().item()), host[objects.size:]


def device_saddles(objects, basins, surface, connectivity, capacity, device):
    """The kernel's table (``capacity`` zeroed slots between two guards of 64 words of -7): (records, counts, guards)."""
    z, y, x = objects.shape
    buf = torch.full((2 * GUARD + 4 * capacity,), FILL, dtype=torch.int32, device=device)
    buf[GUARD:GUARD + 4 * capacity] = 0
    counts = torch.full((2 + GUARD,), FILL, dtype=torch.int32, device=device)
    d_objects, d_basins, d_surface = _d(objects, device), _d(basins, device), _d(surface, device)
    with torch.cuda.device(device):
        _lib.call("lsr_watershed_saddles_f32", d_objects.data_ptr(), d_basins.data_ptr(), d_surface.data_ptr(), z, y, x,
                  connectivity, capacity, buf[GUARD:].data_ptr(), counts.data_ptr(), _lib.stream_ptr(device))
    host, c = buf.cpu().numpy(), counts.cpu().numpy()
    return host[GUARD:GUARD + 4 * capacity].view(W.SADDLE_DTYPE), c[:2].tolist(), np.concatenate(
        [host[:GUARD], host[GUARD + 4 * capacity:], c[2:]])


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_kernels_equal_the_restatement_and_the_twin(name, connectivity, device):
    case = C.case(name)
    want, n_want, summits = R.case_basins(name, connectivity)
    got, n, guard = device_watershed(case["objects"], case["surface"], connectivity, device)
    assert np.all(guard == FILL), "the kernels wrote behind their output"
    assert not np.any(got == FILL), "a voxel was not written"
    assert n == n_want == summits
    assert np.array_equal(got, want)
    again, n2, _ = device_watershed(case["objects"], case["surface"], connectivity, device)
    assert n2 == n and got.tobytes() == again.tobytes()
    twin, n_twin, _ = H.twin_watershed(case["objects"], case["surface"], connectivity)
    assert n_twin == n and got.tobytes() == twin.tobytes()


def test_a_second_case_on_the_same_uncleared_scratch(device):
    first, second = C.case("tiles-random-bernoulli"), C.case("tile+1-serpentine-solid")    # many directions, then few, in the same bytes
    device_watershed(first["objects"], first["surface"], 26, device)
    got, n, _ = device_watershed(second["objects"], second["surface"], 6, device)
    want, n_want, _ = R.case_basins("tile+1-serpentine-solid", 6)
    assert n == n_want and np.array_equal(got, want)


def test_nan_neither_hangs_nor_leaves_a_voxel_unwritten(device):
    rng = np.random.default_rng(5)
    shape = C.SHAPES["tile+1"]
    surface = rng.standard_normal(shape).astype(np.float32)
    surface[rng.random(shape) < 0.3] = np.nan
    surface[rng.random(shape) < 0.1] = -np.nan
    objects = np.ones(shape, dtype=np.int32)
    got, n, guard = device_watershed(objects, surface, 26, device)
    twin, n_twin, _ = H.twin_watershed(objects, surface, 26)
    assert np.all(guard == FILL) and n == n_twin and np.array_equal(got, twin)


@pytest.mark.parametrize("name,connectivity", C.GRAPH_PARAMS, ids=C.GRAPH_IDS)
def test_saddles_equal_the_restatement(name, connectivity, device):
    case = C.case(name)
    basins, n, _ = R.case_basins(name, connectivity)
    want = R.case_saddles(name, connectivity)
    capacity = 1 << int(2 * len(want) + 16).bit_length()
    rows, counts, guards = device_saddles(case["objects"], basins, case["surface"], connectivity, capacity, device)
    assert np.all(guards == FILL), "the kernel wrote outside the table"
    assert counts == [len(want), 0]
    assert H.records_as_set(rows) == want
    got = W.basin_saddles(_d(case["objects"], device), _d(basins, device), n, _d(case["surface"], device), connectivity)
    H.check_saddle_arrays(got, R.saddle_arrays(want))


def test_a_table_that_is_too_small_says_so_and_the_python_layer_retries(device):
    case = C.case(C.TIE_HEAVY)
    basins, n, _ = R.case_basins(C.TIE_HEAVY, 26)
    want = R.case_saddles(C.TIE_HEAVY, 26)
    rows, counts, guards = device_saddles(case["objects"], basins, case["surface"], 26, 2, device)      # (status OK: it returned)
    assert counts[0] == 2 and counts[1] > 0 and np.all(guards == FILL), "a write outside the table"
    assert set(H.records_as_set(rows)) <= set(want)
    got = W.basin_saddles(_d(case["objects"], device), _d(basins, device), n, _d(case["surface"], device), 26, _capacity=2)
    H.check_saddle_arrays(got, R.saddle_arrays(want))


@pytest.mark.parametrize("name,connectivity", H.SPLIT_PARAMS, ids=[f"{n}-{k}" for n, k in H.SPLIT_PARAMS])
def test_split_labels_equal_the_restatement(name, connectivity, device):
    H.check_split(C.case(name), connectivity, device)


@pytest.mark.parametrize("min_depth,labels", [(1.0, 2), (8.0, 1)])
def test_touching_balls(min_depth, labels, device):
    from shrimpy_amd import distance
    from shrimpy_amd import dynatrack as D

    surface = D._gaussian_blur_3d(distance.distance_transform_labels(_d(C.touching_balls(), device), (1, 1, 1), invert=True), 1.0)
    H.check_balls(min_depth, labels, surface.cpu().numpy(), device)


def test_the_timing_entry_splits_like_the_plain_one(device):
    case = C.case("tiles-ties-bernoulli")
    ms7 = (ctypes.c_float * 7)(*([-1.0] * 7))
    got, n, guard = device_watershed(case["objects"], case["surface"], 18, device, entry="lsr_watershed_profile_f32", extra=(ms7,))
    want, n_want, _ = R.case_basins("tiles-ties-bernoulli", 18)
    assert np.all(guard == FILL) and n == n_want and np.array_equal(got, want)
    assert all(0.0 <= t < 1e4 for t in ms7), list(ms7)


def test_watershed_basins_returns_a_torch_tensor_on_the_device(device):
    case = C.case("tiles-random-diagonal")
    basins, n = W.watershed_basins(_d(case["objects"], device), _d(case["surface"], device), 26)
    assert basins.device.type == "cuda" and basins.dtype == torch.int32 and basins.is_contiguous()
    want, n_want, _ = R.case_basins("tiles-random-diagonal", 26)
    assert n == n_want and np.array_equal(basins.cpu().numpy(), want)


def test_segment_zyx_with_split_on_the_device(device):
    H.check_segment_with_split(device)
