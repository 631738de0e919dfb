"""The labelling kernels (``csrc/label.hip``) on the device: ``scipy.ndimage.label`` element for element on every case of
``tests/label_cases.py`` (sized from the tile of the local launch), every voxel written and nothing behind the buffer, the
same bytes from two calls, one uncleared scratch buffer for every call; the object table against ``tests/label_ref.py``
(integers and the intensity range exactly, the float64 atomic sums within ``n_k * 2^-53 * sum|terms|``), the relabelling,
the Python layer and the ``segment`` command.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from shrimpy_amd.settings import SegmentSettings
from tests import label_cases as C
from tests import label_ref as R
from tests import test_label_host as H

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = -7
_SCRATCH = {}


def _scratch(device):
    """One poisoned scratch buffer for every call of this module, never cleared between them."""
    if device not in _SCRATCH:
        _SCRATCH[device] = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device=device)
    return _SCRATCH[device]


def device_label(vol, threshold, connectivity, device):
    """The kernels through the C ABI into a buffer pre-filled with -7 with 64 guard words behind it: (labels, n, guard)."""
    z, y, x = vol.shape
    scratch = _scratch(device)
    assert 0 < _lib.call_value("lsr_label_scratch_bytes", z, y, x) <= scratch.numel()
    d_vol = torch.from_numpy(np.array(vol, dtype=np.float32, order="C")).to(device)
    buf = torch.full((vol.size + GUARD,), FILL, dtype=torch.int32, device=device)
    count = torch.full((1,), FILL, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.call("lsr_label_f32", d_vol.data_ptr(), z, y, x, ctypes.c_float(threshold), connectivity, buf.data_ptr(),
                  count.data_ptr(), scratch.data_ptr(), _lib.stream_ptr(device))
    host = buf.cpu().numpy()
    return host[:vol.size].reshape(vol.shape), int(count.cpu().item()), host[vol.size:]


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_kernels_equal_scipy_label(name, connectivity, device):
    case = C.case(name)
    want, n_want = R.case_labels(name, connectivity)
    got, n, guard = device_label(case["vol"], case["threshold"], connectivity, device)
    assert np.all(guard == FILL), "the kernels wrote behind their output"
    assert not np.any(got == FILL), "a voxel was not written"
    assert n == n_want
    assert np.array_equal(got, want)
    again, n2, _ = device_label(case["vol"], case["threshold"], connectivity, device)
    assert n2 == n and got.tobytes() == again.tobytes()


def test_a_second_case_on_the_same_uncleared_scratch(device):
    first, second = C.case("noise_p0.5"), C.case("comb")               # many block counts, then few, in the same words
    device_label(first["vol"], first["threshold"], 26, device)
    got, n, _ = device_label(second["vol"], second["threshold"], 6, device)
    want, n_want = R.case_labels("comb", 6)
    assert n == n_want and np.array_equal(got, want)


def test_kernels_equal_the_twin(device):
    case = C.case("threshold_semantics")
    for k in C.CONNECTIVITIES:
        got, n, _ = device_label(case["vol"], case["threshold"], k, device)
        twin, n_twin, _ = H.twin_label(case["vol"], case["threshold"], k)
        assert n == n_twin and np.array_equal(got, twin)


@pytest.mark.parametrize("name,connectivity", H.TABLE_CASES, ids=[f"{n}-{k}" for n, k in H.TABLE_CASES])
def test_table_equals_the_restatement_and_the_twin(name, connectivity, device):
    labels, n = R.case_labels(name, connectivity)
    inten = C.intensities(name)
    want = R.table(labels, n, inten)
    d_labels, d_inten = torch.from_numpy(np.array(labels)).to(device), torch.from_numpy(inten).to(device)
    got = S.region_table(d_labels, n, d_inten)
    worst = R.check_table(got, want)
    print(f"{name}-{connectivity}: {n} objects, worst float64 sum error / bound = {worst:.3f}")
    twin = S.region_table(torch.from_numpy(np.array(labels)), n, torch.from_numpy(inten))
    for key in ("volume", "bbox", "sum_zyx"):
        assert np.array_equal(got[key], twin[key]), key
    for key in ("intensity_min", "intensity_max"):
        assert np.array_equal(got[key].view(np.uint32), twin[key].view(np.uint32)), key
    R.check_table(S.region_table(d_labels, n), R.table(labels, n))       # without intensities


def test_table_of_nothing_is_empty(device):
    labels = torch.zeros((2, 3, 4), dtype=torch.int32, device=device)
    got = S.region_table(labels, 0, torch.ones((2, 3, 4), dtype=torch.float32, device=device))
    assert all(len(v) == 0 for v in got.values())
    with torch.cuda.device(device):
        _lib.call("lsr_label_regions_f32", labels.data_ptr(), None, 2, 3, 4, 0, None, _lib.stream_ptr(device))


@pytest.mark.parametrize("min_volume,keep_largest", [(0, False), (2, False), (10 ** 9, False), (0, True), (2, True), (10 ** 9, True)])
def test_filter_matches_the_numpy_restatement(min_volume, keep_largest, device):
    labels, n = R.case_labels("noise_p0.2", 6)
    work = torch.from_numpy(np.array(labels)).to(device)
    got, table, m = S.filter_objects(work, S.region_table(work, n), min_volume, keep_largest)
    want, m_want = R.filter_labels(labels, min_volume, keep_largest)
    assert m == m_want and np.array_equal(got.cpu().numpy(), want)
    assert table["label"].tolist() == list(range(1, m + 1))


def test_keep_largest_with_a_tie_keeps_the_lowest_label(device):
    vol = np.zeros((1, 5, 9), dtype=np.float32)
    vol[0, 0, 0:2] = vol[0, 2, 0:3] = vol[0, 4, 5:8] = vol[0, 4, 0] = 1          # volumes 2, 3, 1, 3 in label order
    labels, n = S.label_volume(torch.from_numpy(vol).to(device), 0.5)
    table = S.region_table(labels, n)
    assert n == 4 and table["volume"].tolist() == [2, 3, 1, 3]
    got, kept, m = S.filter_objects(labels, table, keep_largest=True)
    want, _ = R.filter_labels(R.label(vol, 0.5, 6)[0], 0, True)
    assert m == 1 and np.array_equal(got.cpu().numpy(), want) and kept["volume"].tolist() == [3]


def test_the_timing_entry_labels_like_the_plain_one(device):
    case = C.case("noise_p0.3")
    vol = torch.from_numpy(np.array(case["vol"])).to(device)
    z, y, x = vol.shape
    labels = torch.full((vol.numel(),), FILL, dtype=torch.int32, device=device)
    count = torch.full((1,), FILL, dtype=torch.int32, device=device)
    ms7 = (ctypes.c_float * 7)(*([-1.0] * 7))
    with torch.cuda.device(device):
        _lib.call("lsr_label_profile_f32", vol.data_ptr(), z, y, x, ctypes.c_float(case["threshold"]), 6, labels.data_ptr(),
                  count.data_ptr(), _scratch(device).data_ptr(), ms7, _lib.stream_ptr(device))
    want, n_want = R.case_labels("noise_p0.3", 6)
    assert int(count.item()) == n_want and np.array_equal(labels.cpu().numpy().reshape(want.shape), want)
    assert all(0.0 <= t < 1e4 for t in ms7), list(ms7)


def test_label_volume_returns_a_torch_tensor_on_the_device(device):
    case = C.case("noise_p0.3")
    vol = torch.from_numpy(np.array(case["vol"])).to(device)
    before = torch.cuda.memory_allocated(device)
    labels, n = S.label_volume(vol, case["threshold"], 18)
    assert labels.device == vol.device and labels.dtype == torch.int32 and labels.is_contiguous()
    assert torch.cuda.memory_allocated(device) > before                  # torch's allocator owns it
    want, n_want = R.case_labels("noise_p0.3", 18)
    assert n == n_want and np.array_equal(labels.cpu().numpy(), want)


def test_segment_zyx_on_the_device(device):
    vol = H.blob_volume(5)
    want, m, n_before = H.reference_segmentation(vol, H.SETTINGS)
    labels, table, n = S.segment_zyx(torch.from_numpy(vol).to(device), SegmentSettings(**H.SETTINGS))
    assert m == 3 and n_before > 3 and n == 3 and np.array_equal(labels.cpu().numpy(), want)
    R.check_table(table, R.table(want, 3, vol))


def test_cli_segment_on_the_device(tmp_path, device):
    import shrimpy_amd.cli as cli

    H.check_segment_command(cli, tmp_path)
