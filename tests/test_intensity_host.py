"""The label intensities on the CPU: the host twins (``lsr_label_intensity_f32_cpu`` / ``_u16_cpu``) against the numpy
restatement (``tests/intensity_ref.py``) on every case of ``tests/intensity_cases.py`` at every grid cap -- uint16 byte for byte,
float32 exactly in the count and the extremes and within ``2 n_k 2^-53 sum|terms|`` in the sums; guards, the pad, the entry
checks; ``intensity_table`` against ``region_table``; ``shell_labels`` against scipy's distance transform.  PARITY UNPINNED: the
rule of ``csrc/intensity.hpp`` is the specification."""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from tests import intensity_cases as C
from tests import intensity_ref as R

GUARD = 64
FILL = -7
WORDS = 8                             # a record in 64-bit words
E_ARG, E_UNSUPPORTED = -4, -3         # include/lsrecon.h
LDS_SLOTS, DEFAULT_BLOCKS = S.intensity_geometry()


def guarded(n):
    """``n`` zeroed records between two guards of 64 words of -7."""
    buf = np.full((2 * GUARD + WORDS * n,), FILL, dtype=np.int64)
    buf[GUARD:GUARD + WORDS * n] = 0
    return buf


def split(buf, n, dtype):
    return buf[GUARD:GUARD + WORDS * n].view(dtype), np.concatenate([buf[:GUARD], buf[GUARD + WORDS * n:]])


def twin_intensity(labels, values, n, max_blocks=0):
    """The twin through the C ABI, by ``values``' type: (records, guards)."""
    z, y, x = labels.shape
    f32 = values.dtype == np.float32
    buf = guarded(n)
    labels, values = np.ascontiguousarray(labels), np.ascontiguousarray(values)
    _lib.call("lsr_label_intensity_f32_cpu" if f32 else "lsr_label_intensity_u16_cpu", labels.ctypes.data, values.ctypes.data,
              z, y, x, n, buf[GUARD:].ctypes.data, max_blocks, None)
    return split(buf, n, S.INTENSITY_DTYPE_F32 if f32 else S.INTENSITY_DTYPE_U16)


def u16_first_refused_x():
    """The least X at which (1, 1, X) is refused for uint16 values: 65535 * X * X >= 2^64, by arithmetic."""
    x = int((2 ** 64 / 65535) ** 0.5)
    while 65535 * x * x >= 2 ** 64:
        x -= 1
    while 65535 * x * x < 2 ** 64:
        x += 1
    assert 65535 * x * x >= 2 ** 64 > 65535 * (x - 1) * (x - 1) and x <= 2 ** 31 - 1
    return x


def entry_check_calls(labels_ptr, values_ptr, table_ptr, u16):
    """``(what, status, arguments)`` of every call the entry must refuse, for a (2, 3, 4) volume and a table of 8 records.  Every
    pointer is valid for the stated shape, except where the shape itself is what is refused before anything is read."""
    ok = dict(labels=labels_ptr, values=values_ptr, Z=2, Y=3, X=4, n=8, table=table_ptr, max_blocks=0)
    bad = [("labels is NULL", E_ARG, dict(labels=None)), ("values is NULL", E_ARG, dict(values=None)),
           ("table is NULL", E_ARG, dict(table=None)), ("an empty shape", E_ARG, dict(Z=0)),
           ("a negative extent", E_ARG, dict(X=-1)), ("n -1", E_ARG, dict(n=-1)), ("max_blocks -1", E_ARG, dict(max_blocks=-1)),
           ("table is labels", E_ARG, dict(table=labels_ptr)), ("table inside labels", E_ARG, dict(table=labels_ptr + 16)),
           ("table is values", E_ARG, dict(table=values_ptr)), ("table inside values", E_ARG, dict(table=values_ptr + 8)),
           ("2^31 voxels", E_UNSUPPORTED, dict(Z=1 << 11, Y=1 << 10, X=1 << 10))]
    if u16:
        bad.append(("uint16 sums past 2^64", E_UNSUPPORTED, dict(Z=1, Y=1, X=u16_first_refused_x())))
    for what, status, change in bad:
        k = dict(ok, **change)
        yield what, status, (k["labels"], k["values"], k["Z"], k["Y"], k["X"], k["n"], k["table"], k["max_blocks"])


def check_entry_refusals(entry, labels_ptr, values_ptr, table_ptr, u16, read_table, *tail):
    for what, status, args in entry_check_calls(labels_ptr, values_ptr, table_ptr, u16):
        with pytest.raises(_lib.LsrError) as err:
            _lib.call(entry, *args, *tail)
        assert err.value.code == status, what
        assert not read_table().any(), f"{what}: something was written"


# ---------------------------------------------------------------- the ABI


def test_the_records_are_sixty_four_bytes_and_the_geometry_is_sane():
    assert S.INTENSITY_DTYPE_F32.itemsize == 64 and S.INTENSITY_DTYPE_U16.itemsize == 64
    assert S.INTENSITY_DTYPE_F32 == R.DTYPE_F32 and S.INTENSITY_DTYPE_U16 == R.DTYPE_U16
    assert S.INTENSITY_DTYPE_F32.names == ("count",) + R.SUMS + ("v_min", "v_max", "pad")
    assert LDS_SLOTS >= 64 and LDS_SLOTS & (LDS_SLOTS - 1) == 0 and DEFAULT_BLOCKS >= 1
    for name in ("INTENSITY_DTYPE_F32", "INTENSITY_DTYPE_U16", "intensity_geometry", "intensity_table", "shell_labels"):
        assert name in S.__all__


def test_census_of_the_cases():
    """The label side is what ``tests/moments_cases.py`` claims at THIS kernel's slots, and the value side is what it claims."""
    for shape, content in C.MANY_LABELS:
        labels, n = C.labels_of(shape, content, LDS_SLOTS)
        assert n == 4 * LDS_SLOTS
        for cap in C.CAPS:
            flat = labels.ravel()
            distinct = [len(np.unique(flat[a:b][flat[a:b] > 0])) for a, b in C.M.spans(flat.size, cap, DEFAULT_BLOCKS)]
            assert max(distinct) > LDS_SLOTS, f"{shape} cap {cap}: no span holds more labels than the LDS table has slots"
    shape, content = C.ROW_CROSSING[2]
    v = C.values_f32(shape, content, LDS_SLOTS, "non-finite")
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    assert np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2 and len(np.unique(labels[~np.isfinite(v)])) == 1
    v = C.values_f32(shape, content, LDS_SLOTS, "signed-zeros")
    assert not v.any() and np.signbit(v).any() and not np.signbit(v).all()
    v = C.values_f32(shape, content, LDS_SLOTS, "cancelling").astype(np.float64)
    assert abs(v.sum()) <= 1e-6 * np.abs(v).sum() and (v > 0).any() and (v < 0).any()


# ---------------------------------------------------------------- the table


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_f32_is_within_the_bound_of_the_restatement(shape, content):
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    for kind in C.VALUES_F32:
        values = C.values_f32(shape, content, LDS_SLOTS, kind)
        want = C.want_f32(shape, content, LDS_SLOTS, kind)
        for cap in C.CAPS:
            rows, guards = twin_intensity(labels, values, n, cap)
            assert np.all(guards == FILL), f"{kind}, cap {cap}: the twin wrote outside the table"
            C.check_f32(rows, want, f"{kind}, cap {cap}")


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_u16_equals_the_restatement(shape, content):
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    for kind in C.VALUES_U16:
        values = C.values_u16(shape, content, kind)
        want = C.want_u16(shape, content, LDS_SLOTS, kind)
        for cap in C.CAPS:
            rows, guards = twin_intensity(labels, values, n, cap)
            assert np.all(guards == FILL), f"{kind}, cap {cap}: the twin wrote outside the table"
            assert rows.tobytes() == want.tobytes(), f"{kind}, cap {cap}"
            assert not rows["pad"].any()


def test_the_package_table():
    """``intensity_table``'s columns from the raw records, for both value types; zero rows keep zeros and NaN means."""
    shape, content = (5, 9, 130), "n-above"
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    t_labels = torch.from_numpy(np.array(labels))
    values = C.values_f32(shape, content, LDS_SLOTS, "offset")
    table = S.intensity_table(t_labels, n, torch.from_numpy(np.array(values)))
    assert list(table) == ["label", "count", "sum", "sum_sq", "mean", "std", "min", "max", "sum_zyx", "weighted_centroid"]
    assert np.array_equal(table["label"], np.arange(1, n + 1)) and table["count"].dtype == np.int64
    assert table["min"].dtype == np.float32 and table["sum"].dtype == np.float64 and table["sum_zyx"].shape == (n, 3)
    for k in range(n):
        inside = values[labels == k + 1].astype(np.float64)
        if len(inside) == 0:
            assert table["count"][k] == 0 and table["sum"][k] == 0 and table["min"][k] == 0 and table["max"][k] == 0
            assert np.isnan(table["mean"][k]) and np.isnan(table["std"][k]) and np.isnan(table["weighted_centroid"][k]).all()
            continue
        assert table["count"][k] == len(inside) and table["min"][k] == inside.min() and table["max"][k] == inside.max()
        assert table["mean"][k] == pytest.approx(inside.mean(), rel=1e-12)
        # (sum_sq / n - mean^2 cancels eight digits at 1e4 + N(0, 1))
        assert table["std"][k] == pytest.approx(inside.std(), rel=1e-6)
        zyx = np.argwhere(labels == k + 1).astype(np.float64)
        assert table["weighted_centroid"][k] == pytest.approx((zyx * inside[:, None]).sum(0) / inside.sum(), rel=1e-12)
    u16 = C.values_u16(shape, content, "random")
    table = S.intensity_table(t_labels, n, torch.from_numpy(np.array(u16)))
    want = C.want_u16(shape, content, LDS_SLOTS, "random")
    assert table["sum"].dtype == np.uint64 and table["min"].dtype == np.uint16
    assert np.array_equal(table["sum"], want["sum_v"]) and np.array_equal(table["sum_sq"], want["sum_vv"])
    assert np.array_equal(table["min"], want["v_min"]) and np.array_equal(table["max"], want["v_max"])
    assert np.array_equal(table["sum_zyx"], np.stack([want["sum_vz"], want["sum_vy"], want["sum_vx"]], axis=1))
    zeros = S.intensity_table(t_labels, n, torch.zeros(shape, dtype=torch.float32))
    assert np.isnan(zeros["weighted_centroid"]).all() and not zeros["sum"].any() and (zeros["std"][:5] == 0).all()


@pytest.mark.parametrize("shape,content", [C.MANY_LABELS[0], C.ROW_CROSSING[2], ((5, 9, 130), "n-above")],
                         ids=["many-labels", "runs", "n-above"])
def test_intensity_table_equals_region_table(shape, content):
    """Exactly in ``count``, ``min`` and ``max``; the sums within the two bounds added: ``region_table``'s ``n_k 2^-53
    sum|terms|`` (``segment.py``'s docstring) and this table's ``2 n_k 2^-53 sum|terms|``."""
    labels, n = C.labels_of(shape, content, LDS_SLOTS)
    t_labels = torch.from_numpy(np.array(labels))
    for kind in ("normal", "offset", "signed-zeros"):
        values = torch.from_numpy(np.array(C.values_f32(shape, content, LDS_SLOTS, kind)))
        ours, theirs = S.intensity_table(t_labels, n, values), S.region_table(t_labels, n, values)
        want = C.want_f32(shape, content, LDS_SLOTS, kind)
        assert np.array_equal(ours["count"], theirs["volume"])
        for a, b in (("min", "intensity_min"), ("max", "intensity_max")):
            assert np.array_equal(ours[a].view(np.uint32), theirs[b].view(np.uint32)), f"{kind}: {a}"
        both = 1.5 * want["bound"]
        assert np.all(np.abs(ours["sum"] - theirs["intensity_sum"]) <= both[:, 0]), kind
        assert np.all(np.abs(ours["sum_zyx"] - theirs["intensity_sum_zyx"]) <= both[:, 2:]), kind


def test_no_objects():
    labels = np.ones((2, 3, 4), dtype=np.int32)
    for values in (np.ones((2, 3, 4), np.float32), np.ones((2, 3, 4), np.uint16)):
        rows, guards = twin_intensity(labels, values, 0)
        assert len(rows) == 0 and np.all(guards == FILL)
        assert all(len(v) == 0 for v in S.intensity_table(torch.from_numpy(labels), 0, torch.from_numpy(values)).values())


# ---------------------------------------------------------------- the entry checks


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_entry_checks(u16):
    labels = np.ones((2, 3, 4), dtype=np.int32)
    values = np.ones((2, 3, 4), dtype=np.uint16 if u16 else np.float32)
    table = np.zeros((8 * WORDS,), dtype=np.int64)
    check_entry_refusals("lsr_label_intensity_u16_cpu" if u16 else "lsr_label_intensity_f32_cpu", labels.ctypes.data,
                         values.ctypes.data, table.ctypes.data, u16, lambda: table, None)
    assert (labels == 1).all() and (values == 1).all()


def test_the_u16_overflow_refusal_only_just_crosses_and_reads_nothing():
    """(1, 1, X) at the least X with 65535 * X * X >= 2^64 is refused with buffers of 4 voxels, which the entry therefore cannot
    have walked; float32 values have no such bound (their sums are float64), and neither has the shape one voxel shorter, which
    is shown by arithmetic alone."""
    x = u16_first_refused_x()
    assert 65535 * x * x >= 2 ** 64 and 65535 * (x - 1) * (x - 1) < 2 ** 64 and x < 2 ** 31
    labels, values = np.ones((4,), dtype=np.int32), np.ones((4,), dtype=np.uint16)
    table = np.zeros((WORDS,), dtype=np.int64)
    with pytest.raises(_lib.LsrUnsupported) as err:
        _lib.call("lsr_label_intensity_u16_cpu", labels.ctypes.data, values.ctypes.data, 1, 1, x, 1, table.ctypes.data, 0, None)
    assert err.value.code == E_UNSUPPORTED and "2^64" in str(err.value) and not table.any()
    # the same extent split over two axes is far inside the bound: 65535 * X * max extent
    assert 65535 * x * (x // 4096) < 2 ** 64
    # the config-2 deskewed shape is inside it by seven bits
    z, y, xx = 171, 2048, 2270
    assert 65535 * z * y * xx * max(z, y, xx) < 2 ** 64 // 2 ** 7


def test_python_argument_checks():
    labels = torch.ones((2, 3, 4), dtype=torch.int32)
    values = torch.ones((2, 3, 4), dtype=torch.float32)
    with pytest.raises(TypeError):
        S.intensity_table(labels.to(torch.int64), 1, values)
    with pytest.raises(TypeError):
        S.intensity_table(labels, 1, values.to(torch.float64))
    with pytest.raises(TypeError):
        S.intensity_table(labels, 1, values.numpy())
    with pytest.raises(ValueError):
        S.intensity_table(labels, -1, values)
    with pytest.raises(ValueError):
        S.intensity_table(labels, 1, values[:, :2])
    with pytest.raises(ValueError):
        S.intensity_table(labels[:, :, ::2], 1, values[:, :, ::2])
    with pytest.raises(ValueError):
        S.shell_labels(labels, -1.0)
    with pytest.raises(ValueError):
        S.shell_labels(labels, 1.0, gap=float("nan"))


# ---------------------------------------------------------------- the ring of local background


def test_shell_labels_equals_scipy_nearest_labels_in_the_ring():
    """Two balls in a (12, 24, 40) volume under sampling (2, 1, 1): a voxel whose distance to the nearest object lies in
    ``(gap, gap + distance]`` carries that object's label, every other voxel 0.  Squared distances are integers here and the two
    squared thresholds are not, so no voxel lies on a threshold; a voxel at the same distance from both balls may carry either."""
    from scipy import ndimage

    sampling, gap, distance = (2.0, 1.0, 1.0), 1.5, 2.2
    z, y, x = np.indices((12, 24, 40)).astype(np.float64)
    labels = np.zeros((12, 24, 40), np.int32)
    labels[(2 * (z - 5)) ** 2 + (y - 11) ** 2 + (x - 12) ** 2 <= 16.0] = 1
    labels[(2 * (z - 6)) ** 2 + (y - 13) ** 2 + (x - 25) ** 2 <= 25.0] = 2
    d = [ndimage.distance_transform_edt(labels != k, sampling=sampling) for k in (1, 2)]
    nearest, dist = np.where(d[0] <= d[1], 1, 2), np.minimum(d[0], d[1])
    want = np.where((dist > gap) & (dist <= gap + distance), nearest, 0)
    got = S.shell_labels(torch.from_numpy(labels), distance, gap, sampling)
    assert got.dtype == torch.int32 and tuple(got.shape) == labels.shape
    got = got.numpy()
    tied = d[0] == d[1]
    assert np.array_equal(got[~tied], want[~tied])
    assert np.all((got[tied] == 0) == (want[tied] == 0)) and set(np.unique(got)) == {0, 1, 2}
    assert not got[labels != 0].any() and (want != 0).sum() > 500
    # gap = 0: the ring starts at the objects
    close = S.shell_labels(torch.from_numpy(labels), distance, 0.0, sampling).numpy()
    assert np.array_equal(close != 0, (dist > 0) & (dist <= distance))
