"""The colocalization kernel (``csrc/coloc.hip``) on the device, on every case of ``tests/coloc_cases.py`` (sized from
``lsr_label_coloc_geometry``) at every threshold and grid cap: uint16 values byte for byte equal to the host twin and the numpy
restatement (``tests/coloc_ref.py``); float32 values with the twin's counts exactly and every sum within ``m 2^-53 sum|terms|`` of
the RESTATEMENT's exact sum; guards around the table; the measurement entry's forms; the form without labels against a volume of
ones; the entry checks; ``pair_table`` and ``costes_thresholds`` on device tensors.  Every test is a few launches on at most
21 630 voxels.  PARITY UNPINNED: the rule of ``csrc/coloc.hpp`` is the specification."""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import colocalize as K
from tests import coloc_cases as C
from tests import test_coloc_host as H

pytestmark = pytest.mark.gpu

GUARD, FILL, WORDS = H.GUARD, H.FILL, H.WORDS


def device_coloc(d_labels, d_a, d_b, n, device, thresholds=(0.0, 0.0), max_blocks=0, lds_slots=None, lds_probes=8):
    """The kernel through the C ABI, by the channels' type: ``n`` zeroed records between two guards of 64 words of -7: (records,
    guards).  ``d_labels`` may be None.  With ``lds_slots`` the measurement entry (``lsr_label_coloc_variant``)."""
    z, y, x = d_a.shape
    f32 = d_a.dtype == torch.float32
    buf = torch.full((2 * GUARD + WORDS * n,), FILL, dtype=torch.int64, device=device)
    buf[GUARD:GUARD + WORDS * n] = 0
    labels_ptr = None if d_labels is None else d_labels.data_ptr()
    ta, tb = (float(v) for v in thresholds)
    with torch.cuda.device(device):
        if lds_slots is None:
            _lib.call("lsr_label_coloc_f32" if f32 else "lsr_label_coloc_u16", labels_ptr, d_a.data_ptr(), d_b.data_ptr(), z, y, x, n,
                      ta, tb, buf[GUARD:].data_ptr(), max_blocks, _lib.stream_ptr(device))
        else:
            _lib.call("lsr_label_coloc_variant", labels_ptr, d_a.data_ptr(), d_b.data_ptr(), 0 if f32 else 1, z, y, x, n, ta, tb,
                      buf[GUARD:].data_ptr(), max_blocks, lds_slots, lds_probes, _lib.stream_ptr(device))
    return H.split(buf.cpu().numpy(), n, K.COLOC_DTYPE_F32 if f32 else K.COLOC_DTYPE_U16)


def upload(arr, device):
    return None if arr is None else torch.from_numpy(np.array(arr)).to(device)


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_kernel_f32_has_the_twins_counts_and_the_restatements_sums(shape, content, device):
    labels, n = C.labels_of(shape, content, H.LDS_SLOTS)
    d_labels = upload(labels, device)
    worst = 0.0
    for kind in C.PAIRS_F32:
        a, b = C.pair_f32(shape, content, H.LDS_SLOTS, kind)
        d_a, d_b = upload(a, device), upload(b, device)
        for name in C.THRESHOLDS_F32:
            thresholds = C.thresholds_of(a, b, name)
            want = C.want_f32(shape, content, H.LDS_SLOTS, kind, name)
            twin, _ = H.twin_coloc(labels, a, b, n, thresholds)
            for cap in C.CAPS:
                rows, guards = device_coloc(d_labels, d_a, d_b, n, device, thresholds, cap)
                what = f"{kind}, {name}, cap {cap}"
                assert np.all(guards == FILL), f"{what}: the kernel wrote outside the table"
                for f in K.COLOC_COUNTS:
                    assert np.array_equal(rows[f], twin[f]), f"{what}: {f}"
                worst = max(worst, C.check_f32(rows, want, what))
    print(f"worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_kernel_u16_equals_the_twin_and_the_restatement(shape, content, device):
    labels, n = C.labels_of(shape, content, H.LDS_SLOTS)
    d_labels = upload(labels, device)
    for kind in C.PAIRS_U16:
        a, b = C.pair_u16(shape, content, kind)
        d_a, d_b = upload(a, device), upload(b, device)
        for name in C.THRESHOLDS_U16:
            thresholds = C.thresholds_of(a, b, name)
            want = C.want_u16(shape, content, H.LDS_SLOTS, kind, name)
            twin, _ = H.twin_coloc(labels, a, b, n, thresholds)
            assert twin.tobytes() == want.tobytes()
            for cap in C.CAPS:
                rows, guards = device_coloc(d_labels, d_a, d_b, n, device, thresholds, cap)
                assert np.all(guards == FILL), f"{kind}, {name}, cap {cap}: the kernel wrote outside the table"
                assert rows.tobytes() == want.tobytes(), f"{kind}, {name}, cap {cap}"


@pytest.mark.parametrize("lds_slots,lds_probes", [(0, 1), (64, 1), (64, 64), (H.LDS_SLOTS, 8)])
def test_the_measurement_forms_give_the_same_records(lds_slots, lds_probes, device):
    worst = 0.0
    for shape, content in [C.MANY_LABELS[1], C.ROW_CROSSING[2], ((3, 7, 1030), C.NO_LABELS)]:
        labels, n = C.labels_of(shape, content, H.LDS_SLOTS)
        d_labels = upload(labels, device)
        for kind in ("offset", "non-finite"):
            a, b = C.pair_f32(shape, content, H.LDS_SLOTS, kind)
            want = C.want_f32(shape, content, H.LDS_SLOTS, kind, "at-value")
            d_a, d_b = upload(a, device), upload(b, device)
            for cap in (1, 0):
                rows, guards = device_coloc(d_labels, d_a, d_b, n, device, C.thresholds_of(a, b, "at-value"), cap, lds_slots, lds_probes)
                assert np.all(guards == FILL)
                worst = max(worst, C.check_f32(rows, want, f"{kind}, cap {cap}, {lds_slots} slots, {lds_probes} probes"))
        a, b = C.pair_u16(shape, content, "random")
        want = C.want_u16(shape, content, H.LDS_SLOTS, "random", "half")
        d_a, d_b = upload(a, device), upload(b, device)
        for cap in (1, 0):
            rows, guards = device_coloc(d_labels, d_a, d_b, n, device, C.thresholds_of(a, b, "half"), cap, lds_slots, lds_probes)
            assert np.all(guards == FILL) and rows.tobytes() == want.tobytes()
    print(f"worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("shape", C.SHAPES, ids=["x".join(map(str, s)) for s in C.SHAPES])
def test_no_labels_equals_a_volume_of_ones(shape, device):
    ones = torch.ones(shape, dtype=torch.int32, device=device)
    a, b = C.pair_u16(shape, C.NO_LABELS, "random")
    d_a, d_b = upload(a, device), upload(b, device)
    for name in C.THRESHOLDS_U16:
        thresholds = C.thresholds_of(a, b, name)
        for cap in C.CAPS:
            without, guards = device_coloc(None, d_a, d_b, 1, device, thresholds, cap)
            with_ones, _ = device_coloc(ones, d_a, d_b, 1, device, thresholds, cap)
            assert np.all(guards == FILL) and without.tobytes() == with_ones.tobytes(), f"{name}, cap {cap}"
    a, b = C.pair_f32(shape, C.NO_LABELS, H.LDS_SLOTS, "linear")
    want = C.want_f32(shape, C.NO_LABELS, H.LDS_SLOTS, "linear", "zero")
    d_a, d_b = upload(a, device), upload(b, device)
    for d_labels in (None, ones):
        rows, _ = device_coloc(d_labels, d_a, d_b, 1, device)
        C.check_f32(rows, want, "linear")


def test_no_objects_launches_nothing(device):
    d_labels = torch.ones((2, 3, 4), dtype=torch.int32, device=device)
    for dtype in (np.float32, np.uint16):
        d_a = upload(np.ones((2, 3, 4), dtype=dtype), device)
        rows, guards = device_coloc(d_labels, d_a, d_a.clone(), 0, device)
        assert len(rows) == 0 and np.all(guards == FILL)


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_entry_checks(u16, device):
    """Only calls whose pointers are valid for the stated shape, or that are refused for the shape before anything is read."""
    labels = torch.ones((2, 3, 4), dtype=torch.int32, device=device)
    a = upload(np.ones((2, 3, 4), dtype=np.uint16 if u16 else np.float32), device)
    b = a.clone()
    table = torch.zeros((8 * WORDS,), dtype=torch.int64, device=device)
    entry = "lsr_label_coloc_u16" if u16 else "lsr_label_coloc_f32"
    with torch.cuda.device(device):
        for what, status, args in H.entry_check_calls(labels.data_ptr(), a.data_ptr(), b.data_ptr(), table.data_ptr()):
            with pytest.raises(_lib.LsrError) as err:
                _lib.call(entry, *args, _lib.stream_ptr(device))
            assert err.value.code == status, what
        for slots, probes in ((48, 8), (2 * H.LDS_SLOTS * 4, 8), (64, 0)):
            with pytest.raises(_lib.LsrError):
                _lib.call("lsr_label_coloc_variant", labels.data_ptr(), a.data_ptr(), b.data_ptr(), int(u16), 2, 3, 4, 8, 0.0, 0.0,
                          table.data_ptr(), 0, slots, probes, _lib.stream_ptr(device))
    assert not table.cpu().numpy().any() and bool((labels == 1).all()) and bool((a == 1).all()) and bool((b == 1).all())


def test_the_package_on_device_tensors_equals_the_host(device):
    """``pair_table`` and ``costes_thresholds`` for uint16 data: the device's answers are the host's."""
    shape, content = (5, 9, 130), "n-above"
    labels, n = C.labels_of(shape, content, H.LDS_SLOTS)
    a, b = C.pair_u16(shape, content, "random")
    t_labels, t_a, t_b = (torch.from_numpy(np.array(v)) for v in (labels, a, b))
    for thresholds in ((0.0, 0.0), (1000.0, 32767.5)):
        host = K.pair_table(t_labels, n, t_a, t_b, thresholds)
        dev = K.pair_table(t_labels.to(device), n, t_a.to(device), t_b.to(device), thresholds, _max_blocks=2)
        assert dev.dtype == K.COLOC_DTYPE_U16 and dev.tobytes() == host.tobytes()
        whole = K.pair_table(None, 1, t_a.to(device), t_b.to(device), thresholds)
        assert whole.tobytes() == K.pair_table(None, 1, t_a, t_b, thresholds).tobytes()
    a, b, structure = C.costes_scene("uint16")
    t_a, t_b, t_labels = (torch.from_numpy(np.array(v)) for v in (a, b, structure.astype(np.int32)))
    for region in ("volume", "labelled"):
        host = K.costes_thresholds(t_labels, 1, t_a, t_b, region=region)
        dev = K.costes_thresholds(t_labels.to(device), 1, t_a.to(device), t_b.to(device), region=region)
        assert dev == host and dev["status"] == "ok" and dev["launches"] <= 34
        want = C.costes_want("uint16", region)
        assert (dev["ta"], dev["tb"]) == (want["ta"], want["tb"])
    # float32 on the device: the conditions of the scene, whatever the order of the adds
    a, b, structure = C.costes_scene("float32")
    got = K.costes_thresholds(None, 1, torch.from_numpy(np.array(a)).to(device), torch.from_numpy(np.array(b)).to(device))
    above = (a > np.float32(got["ta"])) & (b > np.float32(got["tb"]))
    print(f"float32 on the device: ta = {got['ta']!r}, tb = {got['tb']!r}; above: structure {above[structure].mean():.4f}, "
          f"background {above[~structure].mean():.4f}")
    assert got["status"] == "ok" and above[structure].all() and above[~structure].mean() <= 0.01
