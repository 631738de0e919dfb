"""The label-overlap kernel (``csrc/overlap.hip``) on the device: the ``np.unique`` restatement (``tests/track_ref.py``) and the
host twin as sets of ``(a, b, count)``, exactly, on every case of ``tests/track_cases.py`` (sized from
``lsr_label_overlap_geometry``); every shift; the grid cap; guards around the table and behind ``counts``; a table that is
too small; the entry checks; ``track_frames`` and the ``track`` command on the device.  Every test is a few launches on at
most a few ten thousand voxels.  PINNED (numpy) for the table, PARITY UNPINNED for the linking rule."""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import track as T
from tests import test_track_host as H
from tests import track_cases as C
from tests import track_ref as R

pytestmark = pytest.mark.gpu

GUARD = H.GUARD
FILL = H.FILL


def device_overlap(a, b, shift, capacity, device, max_blocks=0):
    """The kernel through the C ABI: the table (``capacity`` zeroed records between two guards of 64 words of -7) and ``counts``
    with a guard behind it: (records, counts, guards)."""
    z, y, x = a.shape
    buf = torch.full((2 * GUARD + 4 * capacity,), FILL, dtype=torch.int32, device=device)
    buf[GUARD:GUARD + 4 * capacity] = 0
    counts = torch.full((2 + GUARD,), FILL, dtype=torch.int32, device=device)
    d_a, d_b = H.tensor(a, device), H.tensor(b, device)
    with torch.cuda.device(device):
        _lib.call("lsr_label_overlap_i32", d_a.data_ptr(), d_b.data_ptr(), z, y, x, H.shift3(shift), capacity,
                  buf[GUARD:].data_ptr(), counts.data_ptr(), max_blocks, _lib.stream_ptr(device))
    host, c = buf.cpu().numpy(), counts.cpu().numpy()
    return host[GUARD:GUARD + 4 * capacity].view(T.OVERLAP_DTYPE), c[:2].tolist(), np.concatenate(
        [host[:GUARD], host[GUARD + 4 * capacity:], c[2:]])


def check(a, b, shift, device, max_blocks=0, capacity=None):
    want = R.overlap_table(a, b, shift)
    capacity = capacity or H.capacity_for(want)
    rows, counts, guards = device_overlap(a, b, shift, capacity, device, max_blocks)
    assert np.all(guards == FILL), "the kernel wrote outside the table or behind counts"
    assert counts == [len(want), 0]
    got = H.records_as_set(rows)
    assert got == want
    return got, capacity


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_kernel_equals_the_restatement_and_the_twin(shape, content, device):
    a, b = C.pair(shape, content)
    got, capacity = check(a, b, (0, 0, 0), device)
    again, _, _ = device_overlap(a, b, (0, 0, 0), capacity, device)
    assert H.records_as_set(again) == got, "two calls give the same set"
    twin, twin_counts, _ = H.twin_overlap(a, b, (0, 0, 0), capacity)
    assert H.records_as_set(twin) == got and twin_counts == [len(got), 0]
    assert H.dict_as_set(T.label_overlaps(H.tensor(a, device), H.tensor(b, device))) == got


def test_runs_of_every_length(device):
    a, b, _ = C.runs_flat(int(np.prod(C.RUNS_SHAPE)))
    for max_blocks in (0, 1):
        check(a.reshape(C.RUNS_SHAPE), b.reshape(C.RUNS_SHAPE), (0, 0, 0), device, max_blocks)


def test_every_voxel_a_pair_of_its_own_overflows_the_lds_table(device):
    a, b = C.distinct_pairs(H.LDS_SLOTS)
    assert a.size > 2 * H.LDS_SLOTS
    check(a, b, (0, 0, 0), device)
    check(a, b, (0, 0, 0), device, max_blocks=1)          # one workgroup: more than half of the pairs go straight to global memory
    check(a, b, (0, 1, -3), device, max_blocks=1)


def test_every_shift_of_a_small_volume(device):
    a, b = C.pair((3, 5, 7), "random-0..3")
    for shift in H.SHIFTS:
        check(a, b, shift, device, capacity=64)


def test_shifts_on_a_volume_of_several_workgroups(device):
    a, b = C.pair((5, 9, 130), "random-0..3")
    for shift in [(1, 0, 0), (-4, 8, -129), (0, -1, 2), (2, 2, 2), (0, 0, -1)]:
        check(a, b, shift, device)
        check(a, b, shift, device, max_blocks=1)


def test_a_shift_at_or_beyond_the_shape_gives_an_empty_table(device):
    a, b = C.pair((3, 5, 7), "one-pair")
    for shift in H.BEYOND:
        rows, counts, guards = device_overlap(a, b, shift, 8, device)
        assert counts == [0, 0] and not rows["pair"].any() and not rows["count"].any() and np.all(guards == FILL), shift


def test_max_blocks_does_not_change_the_table(device):
    a, b = C.pair(*C.MANY_PAIRS)
    default, _ = check(a, b, (0, 0, 0), device)
    for max_blocks in (1, 2):                              # one workgroup carries its LDS table across several strides
        got, _ = check(a, b, (0, 0, 0), device, max_blocks)
        assert got == default
    a, b = C.pair((5, 9, 130), "one-pair")
    assert check(a, b, (0, 0, 0), device, max_blocks=1)[0] == {(1, 1, 5 * 9 * 130)}


def test_a_table_that_is_too_small_says_so_and_the_python_layer_retries(device):
    a, b = C.pair(*C.MANY_PAIRS)
    want = R.overlap_table(a, b)
    H.check_partial_table(*device_overlap(a, b, (0, 0, 0), 2, device), want)          # (status OK: it returned)
    assert H.dict_as_set(T.label_overlaps(H.tensor(a, device), H.tensor(b, device), _capacity=2)) == want


def test_entry_checks_refuse_with_a_message_and_write_nothing(device):
    a = torch.ones((2, 3, 4), dtype=torch.int32, device=device)
    b = torch.ones((2, 3, 4), dtype=torch.int32, device=device)
    table = torch.full((8 * 4,), FILL, dtype=torch.int32, device=device)
    counts = torch.full((2,), FILL, dtype=torch.int32, device=device)
    lib = _lib.load()
    with torch.cuda.device(device):
        for what, args in H.entry_check_calls(a.data_ptr(), b.data_ptr(), table.data_ptr(), counts.data_ptr()):
            rc = lib.lsr_label_overlap_i32(*args, _lib.stream_ptr(device))
            assert rc == H.E_ARG, what
            assert lib.lsr_last_error().decode(), what
    torch.cuda.synchronize(device)
    assert bool((table == FILL).all()) and bool((counts == FILL).all()) and bool((a == 1).all()) and bool((b == 1).all())


@pytest.mark.parametrize("divisions", [True, False])
def test_scene_tracks_on_the_device(divisions, device):
    tracks, _ = H.check_tracks(C.scene(), device, divisions=divisions)
    assert tracks == (C.SCENE_TRACKS_DIVISIONS if divisions else C.SCENE_TRACKS_NO_DIVISIONS)
    H.check_tracks(C.scene(), device, shifts=[(0, 0, 2)] * 4, divisions=divisions)


def test_cli_track_on_the_device(tmp_path, device):
    import shrimpy_amd.cli as cli

    H.check_track_command(cli, tmp_path)
