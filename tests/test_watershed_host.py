"""The watershed on the host: the twins (``lsr_watershed_f32_cpu``, ``lsr_watershed_saddles_f32_cpu``) against the numpy
restatement of the rule (``tests/watershed_ref.py``: exact equality, saddle values bit for bit), the entry statuses of twin and
device entry alike, ``shrimpy_amd.watershed`` on CPU tensors, the settings, ``segment_zyx`` with ``split`` and the ``segment`` command.

Cases: ``tests/watershed_cases.py``, sized from the tile of the local launch.  PARITY UNPINNED: the restatement is the reference.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from shrimpy_amd import watershed as W
from shrimpy_amd.settings import SegmentSettings
from tests import label_ref as LR
from tests import watershed_cases as C
from tests import watershed_ref as R

GUARD = 64
FILL = -7
# one scratch buffer for every call of this module, never cleared between them (and poisoned to begin with)
SCRATCH = np.full(1 << 16, 0xA5, dtype=np.uint8)
INF = float("inf")
MIN_DEPTHS = (0.0, 0.5, INF)


def twin_watershed(objects, surface, connectivity):
    """The twin through the C ABI into a buffer pre-filled with -7 with 64 guard words behind it: (basins, B, guard)."""
    objects = np.ascontiguousarray(objects, dtype=np.int32)
    surface = np.ascontiguousarray(surface, dtype=np.float32)
    z, y, x = objects.shape
    assert 0 < _lib.call_value("lsr_watershed_scratch_bytes", z, y, x) <= SCRATCH.nbytes
    buf = np.full(objects.size + GUARD, FILL, dtype=np.int32)
    count = np.full(1, FILL, dtype=np.int32)
    _lib.call("lsr_watershed_f32_cpu", objects.ctypes.data, surface.ctypes.data, z, y, x, connectivity, buf.ctypes.data,
              count.ctypes.data, SCRATCH.ctypes.data, None)
    return buf[:objects.size].reshape(objects.shape), int(count[0]), buf[objects.size:]


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


def records_as_set(rows):
    """The claimed slots of a table as ``{(a, b): key}`` (and a check that no pair sits in two slots)."""
    rows = rows[rows["pair"] != 0]
    out = {(int(p >> np.uint64(32)), int(p & np.uint64(0xFFFFFFFF))): int(k) for p, k in zip(rows["pair"], rows["key"])}
    assert len(out) == len(rows), "a pair claimed two slots"
    assert not rows["unused"].any()
    return out


def check_saddle_arrays(got, want):
    assert np.array_equal(got["a"], want["a"]) and np.array_equal(got["b"], want["b"])
    assert got["saddle"].dtype == np.float32 and np.array_equal(got["saddle"].view(np.uint32), want["saddle"].view(np.uint32))


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))            # (a copy: the shared cases and references are read-only)


# ---- the basins -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_basins_equal_the_restatement(name, connectivity):
    case = C.case(name)
    want, n_want, summits = R.case_basins(name, connectivity)
    got, n, guard = twin_watershed(case["objects"], case["surface"], connectivity)
    assert np.all(guard == FILL), "the twin wrote behind its output"
    assert not np.any(got == FILL), "a voxel was not written"
    assert n == n_want == summits
    assert np.array_equal(got, want)
    again, n2, _ = twin_watershed(case["objects"], case["surface"], connectivity)
    assert n2 == n and got.tobytes() == again.tobytes()


def test_the_cases_aim_at_the_tile_faces_and_the_rule():
    tz, ty, tx = C.T
    assert min(C.T) >= 1
    assert C.SHAPES == {"one": (1, 1, 1), "row": (1, 1, 3 * tx + 5), "tile+1": (tz + 1, ty + 1, tx + 1),
                        "tiles": (2 * tz + 1, ty + 2, 2 * tx + 3)}
    assert len(C.CASES) == 4 * 6 * 4
    # by hand: a row of one object; of the plateau 2 2 the left voxel is the summit (the smaller index), the right climbs to it
    obj = np.ones((1, 1, 7), dtype=np.int32)
    srf = np.array([[[1, 2, 2, 0, 3, 0, 0]]], dtype=np.float32)
    got, n, _ = twin_watershed(obj, srf, 6)
    assert got.ravel().tolist() == [1, 1, 1, 2, 2, 2, 2] and n == 2
    want, n_want, summits = R.basins(obj, srf, 6)
    assert np.array_equal(got, want) and n_want == summits == 2
    # ... and -0.0 sorts below +0.0: the summits are the +0.0s, and the run of -0.0 leans on its smallest index
    srf = np.array([[[-0.0, 0.0, -0.0, -0.0, -0.0, 0.0, -0.0]]], dtype=np.float32)
    got, n, _ = twin_watershed(obj, srf, 6)
    assert got.ravel().tolist() == [1, 1, 1, 1, 2, 2, 2] and n == 2
    # two objects side by side never share a basin, whatever the surface says
    obj = np.array([[[4, 4, 9, 9]]], dtype=np.int32)
    got, n, _ = twin_watershed(obj, np.array([[[0, 1, 2, 3]]], dtype=np.float32), 26)
    assert got.ravel().tolist() == [1, 1, 2, 2] and n == 2
    # the serpentine is one basin of the solid block under 6: its chain of ascents is the whole path
    labels, n_serp, _ = R.case_basins("tiles-serpentine-solid", 6)
    path = C.serpentine_path(C.SHAPES["tiles"])
    assert len(path) > labels.size // 4 and len({int(labels[p]) for p in path}) == 1
    # NaN has a place in the order: nothing hangs, every voxel is written
    srf = np.array([[[np.nan, 1.0, -np.nan, 2.0, np.nan, 0.0, np.nan]]], dtype=np.float32)
    got, n, _ = twin_watershed(np.ones((1, 1, 7), dtype=np.int32), srf, 6)
    assert n >= 1 and got.min() >= 1 and got.max() == n


# ---- the saddles ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,connectivity", C.GRAPH_PARAMS, ids=C.GRAPH_IDS)
def test_twin_saddles_equal_the_restatement(name, connectivity):
    case = C.case(name)
    basins, n, _ = R.case_basins(name, connectivity)
    want = R.case_saddles(name, connectivity)
    capacity = 1 << int(2 * len(want) + 16).bit_length()
    rows, counts, guards = twin_saddles(case["objects"], basins, case["surface"], connectivity, capacity)
    assert np.all(guards == FILL), "the twin wrote outside the table"
    assert counts == [len(want), 0]
    assert records_as_set(rows) == want
    got = W.basin_saddles(_t(case["objects"]), _t(basins), n, _t(case["surface"]), connectivity)
    check_saddle_arrays(got, R.saddle_arrays(want))


def test_a_table_that_is_too_small_says_so_and_the_python_layer_retries():
    case = C.case(C.TIE_HEAVY)
    basins, n, _ = R.case_basins(C.TIE_HEAVY, 26)
    want = R.case_saddles(C.TIE_HEAVY, 26)
    assert len(want) > 100
    rows, counts, guards = twin_saddles(case["objects"], basins, case["surface"], 26, 2)          # (status OK: it returned)
    assert counts[0] == 2 and counts[1] > 0 and np.all(guards == FILL)
    assert set(records_as_set(rows)) <= set(want)
    got = W.basin_saddles(_t(case["objects"]), _t(basins), n, _t(case["surface"]), 26, _capacity=2)
    check_saddle_arrays(got, R.saddle_arrays(want))
    with pytest.raises(ValueError):
        W.basin_saddles(_t(case["objects"]), _t(basins), n, _t(case["surface"]), 26, _capacity=3)


# ---- the merge and the relabelling ------------------------------------------------------------------------------------------------

SPLIT_PARAMS = [(n, k) for n, k in C.GRAPH_PARAMS if C.case(n)["shape_name"] == "tiles"]


@pytest.mark.parametrize("name,connectivity", SPLIT_PARAMS, ids=[f"{n}-{k}" for n, k in SPLIT_PARAMS])
def test_split_labels_equal_the_restatement(name, connectivity):
    case = C.case(name)
    check_split(case, connectivity, torch.device("cpu"))


def check_split(case, connectivity, device):
    """Shared with tests/test_watershed_gpu.py."""
    objects = np.maximum(case["objects"], 0)
    for min_depth in MIN_DEPTHS:
        want, m_want = R.split(case["objects"], case["surface"], connectivity, min_depth)
        got, m = W.split_labels(_t(case["objects"]).to(device), _t(case["surface"]).to(device), connectivity, min_depth)
        assert got.dtype == torch.int32 and got.device.type == device.type
        got = got.cpu().numpy()
        assert m == m_want and np.array_equal(got, want), min_depth
        # a refinement of the input: the background stays, no output label spans two objects
        assert np.array_equal(got > 0, objects > 0)
        pairs = np.unique(np.stack([got[got > 0], objects[got > 0]]), axis=1)
        assert pairs.shape[1] == m
        if min_depth == INF:                                   # (the objects are connected under 6 and numbered in raster order)
            assert np.array_equal(got, objects)


def test_merge_map_by_hand():
    # three basins in a row: peaks 5, 3, 4; saddles (1, 2) at 2 and (2, 3) at 2.5
    peaks, a, b, s = [5.0, 3.0, 4.0], [1, 2], [2, 3], [2.0, 2.5]
    assert W.merge_map(peaks, a, b, s, 0.0).tolist() == [0, 1, 2, 3]
    assert W.merge_map(peaks, a, b, s, 0.5).tolist() == [0, 1, 2, 2]             # 2 into 3: depth 3 - 2.5
    assert W.merge_map(peaks, a, b, s, 1.9).tolist() == [0, 1, 2, 2]             # the cluster {2, 3} has peak 4: depth 4 - 2 = 2
    assert W.merge_map(peaks, a, b, s, 2.0).tolist() == [0, 1, 1, 1]
    assert W.merge_map(peaks, a, b, s, INF).tolist() == [0, 1, 1, 1]
    # a plateau the index rule split: the saddle equals the lower peak bit for bit, inf against inf included
    assert W.merge_map([INF, INF], [1], [2], [INF], 0.0).tolist() == [0, 1, 1]
    assert W.merge_map([1.0, 1.0, 7.0], [1], [2], [1.0], 0.0).tolist() == [0, 1, 1, 2]
    assert W.merge_map([], [], [], [], 0.0).tolist() == [0]
    for peaks_, a_, b_, s_, d in ((peaks, a, b, s, 0.7), ([INF, INF], [1], [2], [INF], 0.0)):
        table = {(p, q): int(R.key(np.float32([v]))[0]) for p, q, v in zip(a_, b_, s_)}
        assert W.merge_map(peaks_, a_, b_, s_, d).tolist() == R.merge(np.float32(peaks_), table, d).tolist()
    with pytest.raises(ValueError):
        W.merge_map(peaks, a, b, s, -1.0)


@pytest.fixture(scope="module")
def balls_surface():
    """The touching balls' depth map on the package's own EDT, blurred with sigma 1 (host twins: the device gives the same bits)."""
    from shrimpy_amd import distance
    from shrimpy_amd import dynatrack as D

    depth = D._gaussian_blur_3d(distance.distance_transform_labels(_t(C.touching_balls()), (1, 1, 1), invert=True), 1.0)
    return depth.numpy()


@pytest.mark.parametrize("min_depth,labels", [(1.0, 2), (8.0, 1)])
def test_touching_balls(min_depth, labels, balls_surface):
    check_balls(min_depth, labels, balls_surface, torch.device("cpu"))


def check_balls(min_depth, labels, surface, device):
    """Shared with tests/test_watershed_gpu.py: radius 10, centres 18 apart, sigma 1, connectivity 26."""
    objects = C.touching_balls()
    want, m_want = R.split(objects, surface, 26, min_depth)
    got, m = W.split_touching(_t(objects).to(device), (1, 1, 1), 1.0, min_depth, 26)
    assert m == m_want == labels
    assert np.array_equal(got.cpu().numpy(), want)
    if labels == 2:                                            # one label per ball: the centres differ
        assert want[12, 12, 12] != want[12, 12, 30] and min(want[12, 12, 12], want[12, 12, 30]) > 0


# ---- entry statuses ---------------------------------------------------------------------------------------------------------------


def test_entry_statuses():
    lib = _lib.load()
    zyx = (ctypes.c_int * 3)()
    assert lib.lsr_watershed_tile_shape(zyx) == 0 and tuple(zyx) == C.T and lib.lsr_watershed_tile_shape(None) == -1
    five = (ctypes.c_int64 * 5)()
    assert lib.lsr_watershed_launch_geometry(five) == 0 and tuple(five) == W.launch_geometry() and min(five) >= 1
    assert lib.lsr_watershed_launch_geometry(None) == -1 and b"NULL" in lib.lsr_last_error()
    assert lib.lsr_watershed_scratch_bytes(4, 5, 6) >= 4 * 5 * 6 + 4
    assert lib.lsr_watershed_scratch_bytes(0, 5, 6) == -2 and lib.lsr_watershed_scratch_bytes(2 ** 11, 2 ** 10, 2 ** 10) == -3
    big = lib.lsr_watershed_scratch_bytes(2 ** 11, 2 ** 10, 2 ** 10 - 1)       # a byte per voxel: past int32 territory
    assert 2 ** 31 - 2 ** 21 <= big <= 2 ** 31 + 2 ** 22
    obj = np.ones((2, 3, 4), dtype=np.int32)
    srf = np.ones((2, 3, 4), dtype=np.float32)
    out = np.full(24, FILL, dtype=np.int32)
    count = np.full(1, FILL, dtype=np.int32)
    g, f, o, c, s = obj.ctypes.data, srf.ctypes.data, out.ctypes.data, count.ctypes.data, SCRATCH.ctypes.data
    for name in ("lsr_watershed_f32_cpu", "lsr_watershed_f32"):          # (checked before anything is launched: safe without a GPU)
        fn = getattr(lib, name)
        assert fn(None, f, 2, 3, 4, 6, o, c, s, None) == -1
        assert fn(g, None, 2, 3, 4, 6, o, c, s, None) == -1
        assert fn(g, f, 2, 3, 4, 6, None, c, s, None) == -1
        assert fn(g, f, 2, 3, 4, 6, o, None, s, None) == -1
        assert fn(g, f, 2, 3, 4, 6, o, c, None, None) == -1 and b"scratch is NULL" in lib.lsr_last_error()
        assert fn(g, f, 0, 3, 4, 6, o, c, s, None) == -2
        assert fn(g, f, 2, -3, 4, 6, o, c, s, None) == -2
        assert fn(g, f, 2, 3, 0, 6, o, c, s, None) == -2
        for bad in (0, 4, 8, 7, 27, -6):
            assert fn(g, f, 2, 3, 4, bad, o, c, s, None) == -4 and b"6, 18 or 26" in lib.lsr_last_error()
        assert fn(g, f, 2 ** 11, 2 ** 10, 2 ** 10, 6, o, c, s, None) == -3           # 2^31 voxels: one too many
        assert fn(g, f, 2 ** 40, 2 ** 40, 2 ** 40, 6, o, c, s, None) == -3
        assert fn(g, f, 2, 3, 4, 6, g, c, s, None) == -4 and b"alias" in lib.lsr_last_error()
    ms7 = (ctypes.c_float * 7)(*([-1.0] * 7))
    fn = lib.lsr_watershed_profile_f32
    assert fn(None, f, 2, 3, 4, 6, o, c, s, ms7, None) == -1 and fn(g, f, 2, 3, 4, 6, o, c, None, ms7, None) == -1
    assert fn(g, f, 2, 0, 4, 6, o, c, s, ms7, None) == -2 and fn(g, f, 2, 3, 4, 8, o, c, s, ms7, None) == -4
    assert fn(g, f, 2 ** 11, 2 ** 10, 2 ** 10, 6, o, c, s, ms7, None) == -3
    assert fn(g, f, 2, 3, 4, 6, o, c, s, None, None) == -1 and b"ms7 is NULL" in lib.lsr_last_error()
    assert list(ms7) == [-1.0] * 7
    table = np.full(4 * 8, FILL, dtype=np.int32)
    two = np.full(2, FILL, dtype=np.int32)
    t, n2 = table.ctypes.data, two.ctypes.data
    for name in ("lsr_watershed_saddles_f32_cpu", "lsr_watershed_saddles_f32"):
        fn = getattr(lib, name)
        assert fn(None, o, f, 2, 3, 4, 6, 8, t, n2, None) == -1
        assert fn(g, None, f, 2, 3, 4, 6, 8, t, n2, None) == -1
        assert fn(g, o, None, 2, 3, 4, 6, 8, t, n2, None) == -1
        assert fn(g, o, f, 2, 3, 4, 6, 8, None, n2, None) == -1
        assert fn(g, o, f, 2, 3, 4, 6, 8, t, None, None) == -1
        assert fn(g, o, f, 2, 3, 0, 6, 8, t, n2, None) == -2
        assert fn(g, o, f, 2 ** 11, 2 ** 10, 2 ** 10, 6, 8, t, n2, None) == -3
        assert fn(g, o, f, 2, 3, 4, 5, 8, t, n2, None) == -4 and b"6, 18 or 26" in lib.lsr_last_error()
        for bad in (0, -8, 3, 6, 2 ** 31):
            assert fn(g, o, f, 2, 3, 4, 6, bad, t, n2, None) == -4 and b"power of two" in lib.lsr_last_error()
    assert np.all(out == FILL) and count[0] == FILL and np.all(table == FILL) and np.all(two == FILL), "a refused call wrote something"
    assert lib.lsr_watershed_f32_cpu(g, f, 2, 3, 4, 6, o, c, s, None) == 0 and np.all(out == 1) and count[0] == 1


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------


def test_the_python_layer_on_cpu_tensors():
    case = C.case("tiles-random-bernoulli")
    for k in C.CONNECTIVITIES:
        basins, n = W.watershed_basins(_t(case["objects"]), _t(case["surface"]), k)
        want, n_want, _ = R.case_basins("tiles-random-bernoulli", k)
        assert basins.dtype == torch.int32 and basins.device.type == "cpu" and basins.shape == want.shape
        assert n == n_want and np.array_equal(basins.numpy(), want)
    nothing, n0 = W.split_labels(_t(np.zeros((2, 3, 4), dtype=np.int32)), _t(np.ones((2, 3, 4), dtype=np.float32)))
    assert n0 == 0 and not nothing.any()
    obj, srf = _t(case["objects"]), _t(case["surface"])
    with pytest.raises(ValueError):
        W.watershed_basins(obj, srf, connectivity=8)
    with pytest.raises(TypeError):
        W.watershed_basins(obj.to(torch.int64), srf)
    with pytest.raises(TypeError):
        W.watershed_basins(obj, srf.to(torch.float64))
    with pytest.raises(ValueError):
        W.watershed_basins(obj, srf[:-1])
    with pytest.raises(ValueError):
        W.split_touching(obj, sigma=-1.0)


def test_settings():
    s = SegmentSettings(channel_name="GFP", threshold=1.0)
    assert s.split is False and s.split_sigma == 1.0 and s.split_min_depth == 0.0
    s = SegmentSettings(channel_name="GFP", threshold=1.0, split=True, split_sigma=0.0, split_min_depth=0.75)
    assert s.split and s.split_sigma == 0.0 and s.split_min_depth == 0.75
    assert "split_min_depth" in SegmentSettings.__doc__
    for bad in (dict(split_sigma=-1.0), dict(split_min_depth=-0.5), dict(split="maybe")):
        with pytest.raises(ValueError):
            SegmentSettings(**{"channel_name": "GFP", "threshold": 1.0, **bad})


# ---- segment_zyx ------------------------------------------------------------------------------------------------------------------

SETTINGS = dict(channel_name="GFP", threshold=500.0, min_volume=4, connectivity=26)
SPLIT = dict(split=True, split_sigma=1.0, split_min_depth=0.5)
SAMPLING = (0.5, 0.25, 0.25)


def nuclei_volume(seed=3):
    """Two overlapping balls (radius 7, centres 12 apart), a third apart from them, and one bright voxel of debris."""
    rng = np.random.default_rng(seed)
    z, y, x = np.indices((20, 24, 48))
    vol = rng.integers(0, 8, size=(20, 24, 48)).astype(np.float32)
    for cz, cy, cx, r in ((9, 11, 10, 7), (9, 11, 22, 7), (9, 11, 40, 5)):
        vol[(z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2 <= r * r] += 1000.0
    vol[1, 1, 1] = 3000.0
    return vol


def reference_split_segmentation(vol, sampling):
    """Labelling by scipy, the depth map and its blur by the package (pinned by their own tests), the split by the restatement,
    the filter by numpy: (labels, M, objects before the split)."""
    from shrimpy_amd import distance
    from shrimpy_amd import dynatrack as D

    before, n = LR.label(vol, SETTINGS["threshold"], SETTINGS["connectivity"])
    depth = D._gaussian_blur_3d(distance.distance_transform_labels(_t(before), sampling, invert=True), SPLIT["split_sigma"])
    parts, _ = R.split(before, depth.numpy(), SETTINGS["connectivity"], SPLIT["split_min_depth"])
    after, m = LR.filter_labels(parts, SETTINGS["min_volume"], False)
    return after, m, n


def check_segment_with_split(device):
    """Shared with tests/test_watershed_gpu.py."""
    vol = nuclei_volume()
    for sampling in ((1, 1, 1), SAMPLING):
        want, m, n_before = reference_split_segmentation(vol, sampling)
        labels, table, n = S.segment_zyx(_t(vol).to(device), SegmentSettings(**SETTINGS, **SPLIT), sampling=sampling)
        assert n_before == 3 and m == n == 3, "the clump counts as two, the debris is dropped after the split"
        assert np.array_equal(labels.cpu().numpy(), want)
        LR.check_table(table, LR.table(want, 3, vol))
        assert want[9, 11, 10] != want[9, 11, 22]
    # split: false is today's segmentation, to the byte
    plain = S.segment_zyx(_t(vol).to(device), SegmentSettings(**SETTINGS))
    off = S.segment_zyx(_t(vol).to(device), SegmentSettings(**SETTINGS, split=False, split_sigma=2.0, split_min_depth=3.0))
    assert plain[2] == off[2] == 2 and plain[0].cpu().numpy().tobytes() == off[0].cpu().numpy().tobytes()
    assert plain[1].keys() == off[1].keys()
    for key in ("label", "volume", "bbox", "sum_zyx", "intensity_min", "intensity_max"):
        assert plain[1][key].tobytes() == off[1][key].tobytes(), key
    # the radius and the expansion follow the split
    both = S.segment_zyx(_t(vol).to(device), SegmentSettings(**SETTINGS, **SPLIT, inscribed_radius=True, expand_distance=1.0),
                         sampling=SAMPLING)
    assert both[2] == 3 and len(both[1]["inscribed_radius"]) == 3 and np.all(both[1]["volume"] > LR.table(want, 3)["volume"])


def test_segment_zyx_with_split_on_the_host():
    check_segment_with_split(torch.device("cpu"))


def test_cli_segment_with_split(tmp_path, monkeypatch):
    """The command needs nothing beyond the YAML settings: its labels and rows are ``segment_zyx``'s at the position's scale."""
    import csv

    import yaml
    from click.testing import CliRunner

    import shrimpy_amd.cli as cli
    from shrimpy_amd.io.omezarr import open_ome_zarr

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    vols = [nuclei_volume(seed) for seed in (3, 4)]
    scale = (1.0, 1.0) + SAMPLING
    with open_ome_zarr(tmp_path / "in.zarr", layout="hcs", mode="w", channel_names=["GFP"], version="0.5", prefer_iohub=False) as plate:
        arr = plate.create_position("A", "1", "0").create_zeros("0", shape=(2, 1) + vols[0].shape, dtype=np.uint16, scale=scale)
        for t, vol in enumerate(vols):
            arr.write_volume(t, 0, vol.astype(np.uint16))
    settings = dict(SETTINGS, **SPLIT)
    cfg = tmp_path / "segment.yml"
    cfg.write_text(yaml.safe_dump(settings))
    out = tmp_path / "labels.zarr"
    r = CliRunner().invoke(cli.cli, ["segment", "-i", str(tmp_path / "in.zarr"), "-c", str(cfg), "-o", str(out)])
    assert r.exit_code == 0, r.output
    with open_ome_zarr(out, prefer_iohub=False) as plate:
        (key, pos), = dict(plate.positions()).items()
        with open(out / key / "objects.csv", newline="") as fh:
            rows = list(csv.DictReader(fh))
        for t, vol in enumerate(vols):
            want, table, n = S.segment_zyx(_t(vol), SegmentSettings(**settings), sampling=SAMPLING)
            assert n == 3 and S.segment_zyx(_t(vol), SegmentSettings(**SETTINGS), sampling=SAMPLING)[2] == 2
            assert np.array_equal(pos["0"].read_volume(t, 0), want.numpy())
            mine = [row for row in rows if int(row["t"]) == t]
            assert [int(row["volume_voxels"]) for row in mine] == table["volume"].tolist() and len(mine) == 3
    bad = tmp_path / "bad.yml"
    bad.write_text(yaml.safe_dump(dict(settings, split_min_depth=-1.0)))
    r = CliRunner().invoke(cli.cli, ["segment", "-i", str(tmp_path / "in.zarr"), "-c", str(bad), "-o", str(tmp_path / "x.zarr")])
    assert r.exit_code != 0 and "split_min_depth" in r.output and not (tmp_path / "x.zarr").exists()
