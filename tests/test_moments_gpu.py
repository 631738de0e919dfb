"""The label-moment kernel (``csrc/moments.hip``) on the device: the ``np.add.at`` restatement (``tests/moments_ref.py``) and the
host twin, byte for byte, on every case of ``tests/moments_cases.py`` (sized from ``lsr_label_moments_geometry``) at every grid
cap; guards around the table; the measurement entry's forms; the entry checks.  Every test is a few launches on at most
21 630 voxels.  PARITY UNPINNED: the rule of ``csrc/moments.hpp`` is the specification."""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from tests import moments_cases as C
from tests import moments_ref as R
from tests import test_moments_host as H

pytestmark = pytest.mark.gpu

GUARD = H.GUARD
FILL = H.FILL


def device_moments(labels, n, device, max_blocks=0, lds_slots=None, lds_probes=8):
    """The kernel through the C ABI: ``n`` zeroed records between two guards of 64 words of -7: (records, guards).  With
    ``lds_slots`` the measurement entry (``lsr_label_moments_variant_i32``)."""
    z, y, x = labels.shape
    buf = torch.full((2 * GUARD + 10 * n,), FILL, dtype=torch.int64, device=device)
    buf[GUARD:GUARD + 10 * n] = 0
    d_labels = torch.from_numpy(np.array(labels)).to(device)
    with torch.cuda.device(device):
        if lds_slots is None:
            _lib.call("lsr_label_moments_i32", d_labels.data_ptr(), z, y, x, n, buf[GUARD:].data_ptr(), max_blocks,
                      _lib.stream_ptr(device))
        else:
            _lib.call("lsr_label_moments_variant_i32", d_labels.data_ptr(), z, y, x, n, buf[GUARD:].data_ptr(), max_blocks,
                      lds_slots, lds_probes, _lib.stream_ptr(device))
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + 10 * n].view(S.MOMENTS_DTYPE), np.concatenate([host[:GUARD], host[GUARD + 10 * n:]])


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_kernel_equals_the_restatement_and_the_twin(shape, content, device):
    labels, n = C.case(shape, content, H.LDS_SLOTS)
    want = R.moments(labels, n)
    twin, _ = H.twin_moments(labels, n)
    assert twin.tobytes() == want.tobytes()
    for cap in C.CAPS:
        rows, guards = device_moments(labels, n, device, cap)
        assert np.all(guards == FILL), f"cap {cap}: the kernel wrote outside the table"
        assert rows.tobytes() == want.tobytes(), f"cap {cap}"
    table = S.moment_table(torch.from_numpy(np.array(labels)).to(device), n, _max_blocks=2)
    for f in R.FIELDS:
        assert table[f].dtype == np.int64 and np.array_equal(table[f], want[f])


@pytest.mark.parametrize("lds_slots,lds_probes", [(0, 1), (64, 1), (64, 64), (512, 8)])
def test_the_measurement_forms_give_the_same_records(lds_slots, lds_probes, device):
    for shape, content in [C.MANY_LABELS[1], C.ROW_CROSSING[2]]:
        labels, n = C.case(shape, content, H.LDS_SLOTS)
        want = R.moments(labels, n)
        for cap in (1, 0):
            rows, guards = device_moments(labels, n, device, cap, lds_slots, lds_probes)
            assert np.all(guards == FILL) and rows.tobytes() == want.tobytes()


def test_no_objects_launches_nothing(device):
    rows, guards = device_moments(np.ones((2, 3, 4), dtype=np.int32), 0, device)
    assert len(rows) == 0 and np.all(guards == FILL)


def test_entry_checks(device):
    """Only calls whose pointers are valid for the stated shape."""
    labels = torch.ones((2, 3, 4), dtype=torch.int32, device=device)
    table = torch.zeros((8 * 10,), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        for what, status, args in H.entry_check_calls(labels.data_ptr(), table.data_ptr()):
            if args[1] * args[2] * args[3] > 24:
                continue
            with pytest.raises(_lib.LsrError) as err:
                _lib.call("lsr_label_moments_i32", *args, _lib.stream_ptr(device))
            assert err.value.code == status, what
        with pytest.raises(_lib.LsrError):
            _lib.call("lsr_label_moments_variant_i32", labels.data_ptr(), 2, 3, 4, 8, table.data_ptr(), 0, 48, 8, _lib.stream_ptr(device))
    assert not table.cpu().numpy().any() and bool((labels == 1).all())
