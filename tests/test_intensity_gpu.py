"""The label-intensity kernel (``csrc/intensity.hip``) on the device, on every case of ``tests/intensity_cases.py`` (sized from
``lsr_label_intensity_geometry``) at every grid cap: uint16 values byte for byte equal to the host twin and the numpy restatement
(``tests/intensity_ref.py``); float32 values with the twin's count and extremes exactly and every sum within ``2 n_k 2^-53
sum|terms|`` of the RESTATEMENT's exact sum; guards around the table; the measurement entry's forms; the entry checks.  Every
test is a few launches on at most 21 630 voxels.  PARITY UNPINNED: the rule of ``csrc/intensity.hpp`` is the specification."""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from tests import intensity_cases as C
from tests import test_intensity_host as H

pytestmark = pytest.mark.gpu

GUARD, FILL, WORDS = H.GUARD, H.FILL, H.WORDS


def device_intensity(d_labels, d_values, n, device, max_blocks=0, lds_slots=None, lds_probes=8):
    """The kernel through the C ABI, by ``d_values``' type: ``n`` zeroed records between two guards of 64 words of -7: (records,
    guards).  With ``lds_slots`` the measurement entry (``lsr_label_intensity_variant``)."""
    z, y, x = d_labels.shape
    f32 = d_values.dtype == torch.float32
    buf = torch.full((2 * GUARD + WORDS * n,), FILL, dtype=torch.int64, device=device)
    buf[GUARD:GUARD + WORDS * n] = 0
    with torch.cuda.device(device):
        if lds_slots is None:
            _lib.call("lsr_label_intensity_f32" if f32 else "lsr_label_intensity_u16", d_labels.data_ptr(), d_values.data_ptr(),
                      z, y, x, n, buf[GUARD:].data_ptr(), max_blocks, _lib.stream_ptr(device))
        else:
            _lib.call("lsr_label_intensity_variant", d_labels.data_ptr(), d_values.data_ptr(), 0 if f32 else 1, z, y, x, n,
                      buf[GUARD:].data_ptr(), max_blocks, lds_slots, lds_probes, _lib.stream_ptr(device))
    return H.split(buf.cpu().numpy(), n, S.INTENSITY_DTYPE_F32 if f32 else S.INTENSITY_DTYPE_U16)


def upload(arr, device):
    return torch.from_numpy(np.array(arr)).to(device)


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_kernel_f32_has_the_twins_integers_and_the_restatements_sums(shape, content, device):
    labels, n = C.labels_of(shape, content, H.LDS_SLOTS)
    d_labels = upload(labels, device)
    for kind in C.VALUES_F32:
        values = C.values_f32(shape, content, H.LDS_SLOTS, kind)
        want = C.want_f32(shape, content, H.LDS_SLOTS, kind)
        twin, _ = H.twin_intensity(labels, values, n)
        d_values = upload(values, device)
        for cap in C.CAPS:
            rows, guards = device_intensity(d_labels, d_values, n, device, cap)
            assert np.all(guards == FILL), f"{kind}, cap {cap}: the kernel wrote outside the table"
            assert np.array_equal(rows["count"], twin["count"]), f"{kind}, cap {cap}: count"
            for f in ("v_min", "v_max"):
                assert rows[f].tobytes() == twin[f].tobytes(), f"{kind}, cap {cap}: {f}"
            C.check_f32(rows, want, f"{kind}, cap {cap}")
    table = S.intensity_table(d_labels, n, d_values, _max_blocks=2)
    assert np.array_equal(table["count"], want["count"])


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_kernel_u16_equals_the_twin_and_the_restatement(shape, content, device):
    labels, n = C.labels_of(shape, content, H.LDS_SLOTS)
    d_labels = upload(labels, device)
    for kind in C.VALUES_U16:
        values = C.values_u16(shape, content, kind)
        want = C.want_u16(shape, content, H.LDS_SLOTS, kind)
        twin, _ = H.twin_intensity(labels, values, n)
        assert twin.tobytes() == want.tobytes()
        d_values = upload(values, device)
        for cap in C.CAPS:
            rows, guards = device_intensity(d_labels, d_values, n, device, cap)
            assert np.all(guards == FILL), f"{kind}, cap {cap}: the kernel wrote outside the table"
            assert rows.tobytes() == want.tobytes(), f"{kind}, cap {cap}"
    table = S.intensity_table(d_labels, n, d_values, _max_blocks=2)
    assert np.array_equal(table["sum"], want["sum_v"]) and np.array_equal(table["max"], want["v_max"])


@pytest.mark.parametrize("lds_slots,lds_probes", [(0, 1), (64, 1), (64, 64), (512, 8)])
def test_the_measurement_forms_give_the_same_records(lds_slots, lds_probes, device):
    for shape, content in [C.MANY_LABELS[1], C.ROW_CROSSING[2]]:
        labels, n = C.labels_of(shape, content, H.LDS_SLOTS)
        d_labels = upload(labels, device)
        for kind in ("offset", "non-finite"):
            want = C.want_f32(shape, content, H.LDS_SLOTS, kind)
            d_values = upload(C.values_f32(shape, content, H.LDS_SLOTS, kind), device)
            for cap in (1, 0):
                rows, guards = device_intensity(d_labels, d_values, n, device, cap, lds_slots, lds_probes)
                assert np.all(guards == FILL)
                C.check_f32(rows, want, f"{kind}, cap {cap}, {lds_slots} slots, {lds_probes} probes")
        want = C.want_u16(shape, content, H.LDS_SLOTS, "random")
        d_values = upload(C.values_u16(shape, content, "random"), device)
        for cap in (1, 0):
            rows, guards = device_intensity(d_labels, d_values, n, device, cap, lds_slots, lds_probes)
            assert np.all(guards == FILL) and rows.tobytes() == want.tobytes()


def test_no_objects_launches_nothing(device):
    d_labels = torch.ones((2, 3, 4), dtype=torch.int32, device=device)
    for dtype in (np.float32, np.uint16):
        rows, guards = device_intensity(d_labels, upload(np.ones((2, 3, 4), dtype=dtype), device), 0, device)
        assert len(rows) == 0 and np.all(guards == FILL)


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_entry_checks(u16, device):
    """Only calls whose pointers are valid for the stated shape, or that are refused for the shape before anything is read."""
    labels = torch.ones((2, 3, 4), dtype=torch.int32, device=device)
    values = upload(np.ones((2, 3, 4), dtype=np.uint16 if u16 else np.float32), device)
    table = torch.zeros((8 * WORDS,), dtype=torch.int64, device=device)
    entry = "lsr_label_intensity_u16" if u16 else "lsr_label_intensity_f32"
    with torch.cuda.device(device):
        for what, status, args in H.entry_check_calls(labels.data_ptr(), values.data_ptr(), table.data_ptr(), u16):
            with pytest.raises(_lib.LsrError) as err:
                _lib.call(entry, *args, _lib.stream_ptr(device))
            assert err.value.code == status, what
        for slots, probes in ((48, 8), (1024, 8), (64, 0)):
            with pytest.raises(_lib.LsrError):
                _lib.call("lsr_label_intensity_variant", labels.data_ptr(), values.data_ptr(), int(u16), 2, 3, 4, 8,
                          table.data_ptr(), 0, slots, probes, _lib.stream_ptr(device))
    assert not table.cpu().numpy().any() and bool((labels == 1).all())
