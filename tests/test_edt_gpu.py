"""The distance-transform kernels (``csrc/edt.hip``) on the device, through the C ABI, on every case of ``tests/edt_cases.py``:
distances against ``scipy.ndimage.distance_transform_edt`` (bit for bit under the exact samplings, within one float32 ulp under
(0.4, 0.116, 0.116), no voxel excluded), ``nearest`` against the brute force, byte for byte against the twin; every voxel written
and nothing behind a buffer, the same bytes from two calls, one uncleared poisoned scratch buffer for every call; the label
expansion, the profile entry, the Python layer, ``segment_zyx`` and the ``segment`` command.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import distance as D
from tests import edt_cases as C
from tests import edt_ref as R
from tests import test_edt_host as H

pytestmark = pytest.mark.gpu

GUARD = H.GUARD
_SCRATCH = {}


def _scratch(device):
    """One poisoned scratch buffer for every call of this module, never cleared between them."""
    if device not in _SCRATCH:
        _SCRATCH[device] = torch.full((H.scratch_bytes_of_the_cases(),), 0xA5, dtype=torch.uint8, device=device)
    return _SCRATCH[device]


def device_edt(vol, threshold, invert, sampling, device, want_dist=True, want_nearest=True, labels=False, profile=False):
    """The kernels through the C ABI into poisoned buffers with 64 guard words behind each: (dist, nearest, guards)."""
    vol = np.array(vol, dtype=np.int32 if labels else np.float32, order="C")      # (a copy: the shared cases are read-only)
    z, y, x = vol.shape
    scratch = _scratch(device)
    assert 0 < _lib.call_value("lsr_edt_scratch_bytes", z, y, x) <= scratch.numel()
    d_vol = torch.from_numpy(vol).to(device)
    dist = torch.full((vol.size + GUARD,), float(H.FILL_F), dtype=torch.float32, device=device)
    nearest = torch.full((vol.size + GUARD,), H.FILL_I, dtype=torch.int32, device=device)
    head = () if labels else (ctypes.c_float(threshold),)
    tail = ()
    entry = "lsr_edt_labels_i32" if labels else "lsr_edt_f32"
    if profile:
        ms3 = (ctypes.c_float * 3)(*([-1.0] * 3))
        entry, tail = "lsr_edt_profile_f32", (ms3,)
    with torch.cuda.device(device):
        _lib.call(entry, d_vol.data_ptr(), z, y, x, *head, int(invert), H._c3(sampling), dist.data_ptr() if want_dist else None,
                  nearest.data_ptr() if want_nearest else None, scratch.data_ptr(), *tail, _lib.stream_ptr(device))
    if profile:
        assert all(0.0 <= t < 1e4 for t in ms3), list(ms3)
    h_dist, h_nearest = dist.cpu().numpy(), nearest.cpu().numpy()
    return (h_dist[:vol.size].reshape(vol.shape), h_nearest[:vol.size].reshape(vol.shape), (h_dist[vol.size:], h_nearest[vol.size:]))


@pytest.mark.parametrize("name,sampling,invert", C.PARAMS, ids=C.PARAM_IDS)
def test_kernels_equal_the_oracles_and_the_twin(name, sampling, invert, device):
    case = C.case(name)
    dist, nearest, guards = device_edt(case["vol"], case["threshold"], invert, sampling, device)
    H.check_buffers(dist, nearest, guards)
    R.check(name, sampling, invert, dist, nearest)
    twin = H.twin_edt(case["vol"], case["threshold"], invert, sampling)
    assert nearest.tobytes() == twin[1].tobytes(), "device and twin disagree on nearest"
    if sampling in C.EXACT:
        assert dist.tobytes() == twin[0].tobytes(), "device and twin disagree on dist"
    again = device_edt(case["vol"], case["threshold"], invert, sampling, device)
    assert dist.tobytes() == again[0].tobytes() and nearest.tobytes() == again[1].tobytes()


@pytest.mark.parametrize("name", ["noise_p0.9", "threshold_semantics"])
def test_the_label_entry_equals_the_float_entry(name, device):
    case, labels = C.case(name), C.label_volume(name)
    for invert in (False, True):
        for sampling in ((1.5, 0.5, 0.25), C.INEXACT):
            want = device_edt(case["vol"], case["threshold"], not invert, sampling, device)
            got = device_edt(labels, None, invert, sampling, device, labels=True)
            H.check_buffers(*got)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            R.check(name, sampling, not invert, got[0], got[1])


def test_a_null_output_leaves_the_other_unchanged(device):
    case = C.case("noise_p0.9")
    both = device_edt(case["vol"], case["threshold"], False, C.INEXACT, device)
    only_dist = device_edt(case["vol"], case["threshold"], False, C.INEXACT, device, want_nearest=False)
    only_nearest = device_edt(case["vol"], case["threshold"], False, C.INEXACT, device, want_dist=False)
    assert only_dist[0].tobytes() == both[0].tobytes() and np.all(only_dist[1] == H.FILL_I) and np.all(only_dist[2][0] == H.FILL_F)
    assert only_nearest[1].tobytes() == both[1].tobytes() and np.all(only_nearest[0] == H.FILL_F) and np.all(only_nearest[2][1] == H.FILL_I)


def test_the_timing_entry_transforms_like_the_plain_one(device):
    case = C.case("noise_p0.5")
    for sampling in ((2.0, 1.0, 1.0), C.INEXACT):
        plain = device_edt(case["vol"], case["threshold"], False, sampling, device)
        timed = device_edt(case["vol"], case["threshold"], False, sampling, device, profile=True)
        H.check_buffers(*timed)
        assert timed[0].tobytes() == plain[0].tobytes() and timed[1].tobytes() == plain[1].tobytes()


@pytest.mark.parametrize("name,labels,sampling,distance", H.EXPAND_CASES, ids=[c[0] for c in H.EXPAND_CASES])
def test_expansion_equals_the_restatement_and_the_twin(name, labels, sampling, distance, device):
    _, nearest, _ = device_edt(labels, None, False, sampling, device, want_dist=False, labels=True)
    _, twin_nearest, _ = H.twin_edt(labels, None, False, sampling, want_dist=False, labels=True)
    assert nearest.tobytes() == twin_nearest.tobytes()
    want = H.twin_expand(labels, twin_nearest, sampling, distance)             # (pinned to the restatement by the host tests)
    if sampling != C.INEXACT:
        assert np.array_equal(want, R.expand(labels, R.brute_nearest(labels != 0, sampling), sampling, distance))
    z, y, x = labels.shape
    d_labels, d_nearest = torch.from_numpy(labels).to(device), torch.from_numpy(np.array(nearest)).to(device)
    out = torch.full((labels.size + GUARD,), H.FILL_I, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.call("lsr_label_expand_i32", d_labels.data_ptr(), d_nearest.data_ptr(), z, y, x, H._c3(sampling), ctypes.c_double(distance),
                  out.data_ptr(), _lib.stream_ptr(device))
        rc = _lib.load().lsr_label_expand_i32(d_labels.data_ptr(), d_nearest.data_ptr(), z, y, x, H._c3(sampling),
                                              ctypes.c_double(distance), d_labels.data_ptr(), _lib.stream_ptr(device))
    assert rc == -4, "aliasing out with labels is refused"
    got = out.cpu().numpy()
    assert np.all(got[labels.size:] == H.FILL_I) and np.array_equal(got[:labels.size].reshape(labels.shape), want)
    assert np.array_equal(d_labels.cpu().numpy(), labels)
    grown = D.expand_labels(d_labels, distance, sampling)
    assert grown.device == d_labels.device and grown.dtype == torch.int32 and np.array_equal(grown.cpu().numpy(), want)


def test_distance_functions_return_torch_tensors_on_the_device(device):
    case = C.case("noise_p0.9")
    vol = torch.from_numpy(np.array(case["vol"])).to(device)
    before = torch.cuda.memory_allocated(device)
    dist, nearest = D.distance_transform(vol, case["threshold"], (1.5, 0.5, 0.25), return_indices=True)
    assert dist.device == vol.device and dist.dtype == torch.float32 and nearest.dtype == torch.int32 and dist.is_contiguous()
    assert torch.cuda.memory_allocated(device) > before                  # torch's allocator owns them
    R.check("noise_p0.9", (1.5, 0.5, 0.25), False, dist.cpu().numpy(), nearest.cpu().numpy())
    labels = torch.from_numpy(C.label_volume("noise_p0.9")).to(device)
    depth = D.distance_transform_labels(labels, (1.5, 0.5, 0.25), invert=True)
    assert depth.cpu().numpy().tobytes() == dist.cpu().numpy().tobytes()


def test_segment_zyx_distance_settings_on_the_device(device):
    H.check_segment_zyx(device)


def test_cli_segment_distance_settings_on_the_device(tmp_path, device):
    import shrimpy_amd.cli as cli

    H.check_segment_command(cli, tmp_path)
