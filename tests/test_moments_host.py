"""The label moments on the CPU: the host twin (``lsr_label_moments_i32_cpu``) against the ``np.add.at`` restatement
(``tests/moments_ref.py``), byte for byte, on every case of ``tests/moments_cases.py``; a census of what the cases claim to be;
the entry checks.  PARITY UNPINNED: the rule of ``csrc/moments.hpp`` is the specification."""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from tests import moments_cases as C
from tests import moments_ref as R

GUARD = 64
FILL = -7
E_ARG, E_UNSUPPORTED = -4, -3         # include/lsrecon.h
LDS_SLOTS, DEFAULT_BLOCKS = S.moments_geometry()


def twin_moments(labels, n, max_blocks=0):
    """The twin through the C ABI: ``n`` zeroed records between two guards of 64 words of -7: (records, guards)."""
    z, y, x = labels.shape
    buf = np.full((2 * GUARD + 10 * n,), FILL, dtype=np.int64)
    buf[GUARD:GUARD + 10 * n] = 0
    labels = np.ascontiguousarray(labels)
    _lib.call("lsr_label_moments_i32_cpu", labels.ctypes.data, z, y, x, n, buf[GUARD:].ctypes.data, max_blocks, None)
    return buf[GUARD:GUARD + 10 * n].view(S.MOMENTS_DTYPE), np.concatenate([buf[:GUARD], buf[GUARD + 10 * n:]])


def entry_check_calls(labels_ptr, table_ptr):
    """``(what, status, arguments)`` of every call the entry must refuse, for a (2, 3, 4) volume and a table of 8 records.  Every
    pointer is valid for the stated shape, except where the shape itself is what is refused before anything is read."""
    ok = dict(labels=labels_ptr, Z=2, Y=3, X=4, n=8, table=table_ptr, max_blocks=0)
    bad = [("labels is NULL", E_ARG, dict(labels=None)), ("table is NULL", E_ARG, dict(table=None)),
           ("an empty shape", E_ARG, dict(Z=0)), ("a negative extent", E_ARG, dict(X=-1)), ("n -1", E_ARG, dict(n=-1)),
           ("max_blocks -1", E_ARG, dict(max_blocks=-1)), ("table is labels", E_ARG, dict(table=labels_ptr)),
           ("table inside labels", E_ARG, dict(table=labels_ptr + 16)),
           ("2^31 voxels", E_UNSUPPORTED, dict(Z=1 << 11, Y=1 << 10, X=1 << 10)),
           ("sums past 2^63", E_UNSUPPORTED, dict(Z=1, Y=1, X=2 ** 31 - 1))]
    for what, status, change in bad:
        k = dict(ok, **change)
        yield what, status, (k["labels"], k["Z"], k["Y"], k["X"], k["n"], k["table"], k["max_blocks"])


def check_entry_refusals(entry, labels_ptr, table_ptr, read_table, *tail):
    for what, status, args in entry_check_calls(labels_ptr, table_ptr):
        with pytest.raises(_lib.LsrError) as err:
            _lib.call(entry, *args, *tail)
        assert err.value.code == status, what
        assert not read_table().any(), f"{what}: something was written"


# ---------------------------------------------------------------- the ABI


def test_the_record_is_eighty_bytes_and_the_geometry_is_sane():
    assert S.MOMENTS_DTYPE.itemsize == 80 and S.MOMENTS_DTYPE.names == R.FIELDS == S.MOMENT_FIELDS
    assert LDS_SLOTS >= 64 and LDS_SLOTS & (LDS_SLOTS - 1) == 0 and DEFAULT_BLOCKS >= 1


def test_census_of_the_cases():
    """The more-labels-than-slots cases and the row-crossing cases are what they claim to be, at every grid cap."""
    for shape, content in C.MANY_LABELS:
        labels, n = C.case(shape, content, LDS_SLOTS)
        assert n == 4 * LDS_SLOTS
        for cap in C.CAPS:
            flat = labels.ravel()
            distinct = [len(np.unique(flat[a:b][flat[a:b] > 0])) for a, b in C.spans(flat.size, cap, DEFAULT_BLOCKS)]
            assert max(distinct) > LDS_SLOTS, f"{shape} cap {cap}: no span holds more labels than the LDS table has slots"
    for shape, content in C.ROW_CROSSING:
        labels, _ = C.case(shape, content, LDS_SLOTS)
        rows = labels.reshape(-1, shape[2])
        carried = (rows[1:, 0] == rows[:-1, -1]) & (rows[1:, 0] != 0)
        assert carried.any(), f"{shape}: no label continues over a row end"
        x = shape[2]
        flat = labels.ravel()
        starts = np.flatnonzero(np.r_[True, flat[1:] != flat[:-1]])
        lengths = np.diff(np.r_[starts, flat.size])
        assert ((starts % x) + lengths > x).any(), "no run lies over a row end"
        if flat.size > 65 * 66 // 2:          # (the runs of lengths 1 .. 65 fit)
            assert lengths.max() > 64, "no run is longer than a wave step"
    assert max(int(np.prod(shape)) for shape, _ in C.ROW_CROSSING) > 65 * 66 // 2


# ---------------------------------------------------------------- the table


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_equals_the_restatement(shape, content):
    labels, n = C.case(shape, content, LDS_SLOTS)
    want = R.moments(labels, n)
    rows, guards = twin_moments(labels, n)
    assert np.all(guards == FILL), "the twin wrote outside the table"
    assert rows.tobytes() == want.tobytes()
    # ... and through the package, as a dict of int64 columns
    table = S.moment_table(torch.from_numpy(np.array(labels)), n)
    assert list(table) == list(R.FIELDS)
    for f in R.FIELDS:
        assert table[f].dtype == np.int64 and np.array_equal(table[f], want[f])


def test_zero_records_are_kept_and_the_volume_is_the_bincount():
    labels, n = C.case((5, 9, 130), "n-above", LDS_SLOTS)
    rows, _ = twin_moments(labels, n)
    assert np.array_equal(rows["volume"], np.bincount(labels.ravel(), minlength=n + 1)[1:n + 1])
    assert not rows[5:].view(np.int64).any() and rows["volume"][:5].all()


def test_no_objects():
    labels = np.ones((2, 3, 4), dtype=np.int32)
    rows, guards = twin_moments(labels, 0)
    assert len(rows) == 0 and np.all(guards == FILL)
    assert all(len(v) == 0 for v in S.moment_table(torch.from_numpy(labels), 0).values())


# ---------------------------------------------------------------- the entry checks


def test_entry_checks():
    labels = np.ones((2, 3, 4), dtype=np.int32)
    table = np.zeros((8 * 10,), dtype=np.int64)
    check_entry_refusals("lsr_label_moments_i32_cpu", labels.ctypes.data, table.ctypes.data, lambda: table, None)
    assert np.array_equal(labels, np.ones((2, 3, 4), dtype=np.int32))


def test_the_range_refusal_reads_nothing():
    """(1, 1, 2^31 - 1) passes the voxel bound and violates voxels * extent^2 < 2^63: refused with a buffer of 4 labels, which the
    entry therefore cannot have walked."""
    labels = np.ones((4,), dtype=np.int32)
    table = np.zeros((10,), dtype=np.int64)
    with pytest.raises(_lib.LsrUnsupported) as err:
        _lib.call("lsr_label_moments_i32_cpu", labels.ctypes.data, 1, 1, 2 ** 31 - 1, 1, table.ctypes.data, 0, None)
    assert err.value.code == E_UNSUPPORTED and "2^63" in str(err.value) and not table.any()
    # the config-2 deskewed shape is inside the bound by eleven bits
    z, y, x = 171, 2048, 2270
    assert z * y * x * max(z, y, x) ** 2 < 2 ** 63 // 2 ** 11 and z * y * x * max(z, y, x) ** 2 >= 2 ** 63 // 2 ** 12


def test_python_argument_checks():
    labels = torch.ones((2, 3, 4), dtype=torch.int32)
    with pytest.raises(TypeError):
        S.moment_table(labels.to(torch.int64), 1)
    with pytest.raises(ValueError):
        S.moment_table(labels, -1)
    with pytest.raises(ValueError):
        S.moment_table(labels[:, :, ::2], 1)
    with pytest.raises(ValueError):
        S.shape_table(labels, 1, sampling=(1, 0, 1))
    with pytest.raises(ValueError):
        S.contact_table(labels, sampling=(1, 1))
