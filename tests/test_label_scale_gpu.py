"""The labelling kernels (``csrc/label.hip``, ``label_uf.hpp``) AT SCALE on the device: ``scipy.ndimage.label`` element for element
on every case of ``tests/label_scale_cases.py`` -- each past one grid cap or scan edge that ``tests/label_cases.py`` stays below:
the scan's several counts per thread and its idle tail, the second trip of merge, flatten, final and local round their grids --
every voxel written, nothing behind the buffer, the same bytes from two calls, one uncleared scratch buffer for every call.  The
table, the relabelling and the expansion past the cap run on synthetic labels (52 objects on the ``voxel_wrap`` shape).

No case holds a long component (the cases module says why); every launch here asks ``safe_labels`` first.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from tests import label_ref as R
from tests import label_scale_cases as C
from tests import test_label_scale_host as H

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = -7
_SCRATCH = {}


def _scratch(device):
    """One poisoned scratch buffer for every call of this module, never cleared between them: what the largest case asks for."""
    if device not in _SCRATCH:
        need = max(_lib.call_value("lsr_label_scratch_bytes", *C.shape(name)) for name in C.NAMES)
        assert 0 < need <= 1 << 16, "64 KiB still suffice"
        _SCRATCH[device] = torch.full((need,), 0xA5, dtype=torch.uint8, device=device)
    return _SCRATCH[device]


def device_label(vol, threshold, connectivity, device, entry="lsr_label_f32", extra=()):
    """The kernels through the C ABI into a buffer pre-filled with -7 with 64 guard words behind it: (labels, n, guard)."""
    z, y, x = vol.shape
    scratch = _scratch(device)
    assert 0 < _lib.call_value("lsr_label_scratch_bytes", z, y, x) <= scratch.numel()
    d_vol = torch.from_numpy(np.array(vol, dtype=np.float32, order="C")).to(device)
    buf = torch.full((vol.size + GUARD,), FILL, dtype=torch.int32, device=device)
    count = torch.full((1,), FILL, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.call(entry, d_vol.data_ptr(), z, y, x, ctypes.c_float(threshold), connectivity, buf.data_ptr(), count.data_ptr(),
                  scratch.data_ptr(), *extra, _lib.stream_ptr(device))
    host = buf.cpu().numpy()
    return host[:vol.size].reshape(vol.shape), int(count.cpu().item()), host[vol.size:]


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_kernels_equal_scipy_label_at_scale(name, connectivity, device):
    case = C.case(name)
    want, n_want = C.safe_labels(name, connectivity)
    got, n, guard = device_label(case["vol"], case["thresholds"][connectivity], connectivity, device)
    assert np.all(guard == FILL), "the kernels wrote behind their output"
    assert not np.any(got == FILL), "a voxel was not written"
    assert n == n_want
    assert np.array_equal(got, want)
    again, n2, _ = device_label(case["vol"], case["thresholds"][connectivity], connectivity, device)
    assert n2 == n and got.tobytes() == again.tobytes()


def test_the_timing_entry_labels_like_the_plain_one_at_scale(device):
    case = C.case("merge_wrap")
    want, n_want = C.safe_labels("merge_wrap", 6)
    ms7 = (ctypes.c_float * 7)(*([-1.0] * 7))
    got, n, guard = device_label(case["vol"], case["thresholds"][6], 6, device, entry="lsr_label_profile_f32", extra=(ms7,))
    assert np.all(guard == FILL) and n == n_want and np.array_equal(got, want)
    assert all(0.0 <= t < 1e4 for t in ms7), list(ms7)


def test_table_of_the_synthetic_labels_past_the_cap(device):
    labels, n = C.synthetic_labels()
    want = C.synthetic_table()
    d_labels = torch.from_numpy(np.array(labels)).to(device)
    d_inten = torch.from_numpy(np.array(C.synthetic_intensity())).to(device)
    got = S.region_table(d_labels, n, d_inten)
    worst = R.check_table(got, want)
    print(f"synthetic: {n} objects, worst float64 sum error / bound = {worst:.3f}")
    R.check_table(S.region_table(d_labels, n), {k: want[k] for k in C.PLAIN_KEYS})       # without intensities


def test_filter_of_the_synthetic_labels_past_the_cap(device):
    labels, n = C.synthetic_labels()
    volumes = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    d_labels = torch.from_numpy(np.array(labels)).to(device)
    table = S.region_table(d_labels, n)
    assert np.array_equal(table["volume"], volumes)
    for min_volume, keep_largest in H.filter_params(volumes):
        work = d_labels.clone()
        got, kept, m = S.filter_objects(work, table, min_volume, keep_largest)
        want, m_want = R.filter_labels(labels, min_volume, keep_largest)
        assert m == m_want and 0 < m < n and np.array_equal(got.cpu().numpy(), want)
        assert kept["label"].tolist() == list(range(1, m + 1))


def test_expansion_past_the_cap(device):
    labels, _ = C.synthetic_labels()
    nearest = C.expand_nearest()
    want = C.expand_restatement(labels, nearest, C.EXPAND_SAMPLING, C.EXPAND_DISTANCE)
    z, y, x = labels.shape
    d_labels, d_nearest = torch.from_numpy(np.array(labels)).to(device), torch.from_numpy(np.array(nearest)).to(device)
    out = torch.full((labels.size + GUARD,), FILL, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.call("lsr_label_expand_i32", d_labels.data_ptr(), d_nearest.data_ptr(), z, y, x, (ctypes.c_double * 3)(*C.EXPAND_SAMPLING),
                  ctypes.c_double(C.EXPAND_DISTANCE), out.data_ptr(), _lib.stream_ptr(device))
    got = out.cpu().numpy()
    assert np.all(got[labels.size:] == FILL), "the kernel wrote behind its output"
    assert not np.any(got[:labels.size] == FILL), "a voxel was not written"
    assert np.array_equal(got[:labels.size].reshape(labels.shape), want)
    assert np.array_equal(d_labels.cpu().numpy(), labels)
