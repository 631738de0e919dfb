"""Tracking on the CPU: the overlap table of the host twin (``lsr_label_overlap_i32_cpu``) against the ``np.unique``
restatement (``tests/track_ref.py``) as sets of ``(a, b, count)``, exactly, on every case of ``tests/track_cases.py``; the
entry checks; the linking and track rules against the plain-loop restatement and the figures of a numpy prototype; the
``track`` command on a temporary store.  PINNED (numpy) for the table, PARITY UNPINNED for the linking rule."""

import csv
import ctypes
import hashlib
import itertools

import numpy as np
import pytest
import torch
import yaml

from shrimpy_amd import _lib
from shrimpy_amd import track as T
from shrimpy_amd.settings import TrackSettings
from tests import track_cases as C
from tests import track_ref as R

GUARD = 64
FILL = -7
E_ARG = -4          # include/lsrecon.h LSR_E_ARG
LDS_SLOTS, DEFAULT_BLOCKS = T.overlap_geometry()


def tensor(a, device="cpu"):
    return torch.from_numpy(np.array(a, order="C")).to(device)          # (a copy: the cases are read-only)


def shift3(shift):
    return (ctypes.c_int32 * 3)(*[int(v) for v in shift])


def records_as_set(rows) -> set:
    rows = rows[rows["pair"] != 0]
    return {(int(p >> np.uint64(32)), int(p & np.uint64(0xFFFFFFFF)), int(c)) for p, c in zip(rows["pair"], rows["count"])}


def dict_as_set(table) -> set:
    assert table["a"].dtype == table["b"].dtype == table["count"].dtype == np.int64
    order = np.lexsort((table["b"], table["a"]))
    assert np.array_equal(order, np.arange(len(order))), "sorted by (a, b)"
    return {(int(a), int(b), int(c)) for a, b, c in zip(table["a"], table["b"], table["count"])}


def twin_overlap(a, b, shift, capacity, max_blocks=0):
    """The twin through the C ABI: the table (``capacity`` zeroed records between two guards of 64 words of -7) and ``counts``
    with a guard behind it: (records, counts, guards)."""
    z, y, x = a.shape
    buf = np.full((2 * GUARD + 4 * capacity,), FILL, dtype=np.int32)
    buf[GUARD:GUARD + 4 * capacity] = 0
    counts = np.full((2 + GUARD,), FILL, dtype=np.int32)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    _lib.call("lsr_label_overlap_i32_cpu", a.ctypes.data, b.ctypes.data, z, y, x, shift3(shift), capacity,
              buf[GUARD:].ctypes.data, counts.ctypes.data, max_blocks, None)
    return buf[GUARD:GUARD + 4 * capacity].view(T.OVERLAP_DTYPE), counts[:2].tolist(), np.concatenate(
        [buf[:GUARD], buf[GUARD + 4 * capacity:], counts[2:]])


def capacity_for(want) -> int:
    return 1 << int(2 * len(want) + 16).bit_length()


def check_partial_table(rows, counts, guards, want):
    """A table of two slots on a many-pair case: what is there is true, and nothing is lost without being counted."""
    assert np.all(guards == FILL), "a write outside the table"
    assert counts[0] <= 2 and counts[1] > 0
    true = {(a, b): c for a, b, c in want}
    got = records_as_set(rows)
    assert len(got) == counts[0]
    for a, b, c in got:
        assert (a, b) in true and 0 < c <= true[a, b]
    assert counts[1] + sum(c for _, _, c in got) == sum(true.values())


def entry_check_calls(a_ptr, b_ptr, table_ptr, counts_ptr):
    """``(what, arguments)`` of every call the entry must refuse, for a (2, 3, 4) volume and a table of 8 records."""
    ok = dict(a=a_ptr, b=b_ptr, Z=2, Y=3, X=4, shift=shift3((0, 0, 0)), capacity=8, table=table_ptr, counts=counts_ptr,
              max_blocks=0)
    bad = [("a is NULL", dict(a=None)), ("b is NULL", dict(b=None)), ("shift is NULL", dict(shift=None)),
           ("table is NULL", dict(table=None)), ("counts is NULL", dict(counts=None)),
           ("an empty shape", dict(Z=0)), ("a negative extent", dict(X=-1)),
           ("2^31 voxels", dict(Z=1 << 11, Y=1 << 10, X=1 << 10)),
           ("capacity 0", dict(capacity=0)), ("capacity 12", dict(capacity=12)), ("capacity 2^31", dict(capacity=1 << 31)),
           ("max_blocks -1", dict(max_blocks=-1)), ("table is a", dict(table=a_ptr)), ("table is b", dict(table=b_ptr)),
           ("table inside a", dict(table=a_ptr + 16))]
    for what, change in bad:
        k = dict(ok, **change)
        yield what, (k["a"], k["b"], k["Z"], k["Y"], k["X"], k["shift"], k["capacity"], k["table"], k["counts"], k["max_blocks"])


# ---------------------------------------------------------------- the ABI


def test_the_record_is_sixteen_bytes_and_the_geometry_is_sane():
    assert T.OVERLAP_DTYPE.itemsize == 16 and T.OVERLAP_DTYPE.names == ("pair", "count")
    assert LDS_SLOTS >= 64 and LDS_SLOTS & (LDS_SLOTS - 1) == 0 and DEFAULT_BLOCKS >= 1


# ---------------------------------------------------------------- the table


@pytest.mark.parametrize("shape,content", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_equals_the_restatement(shape, content):
    a, b = C.pair(shape, content)
    want = R.overlap_table(a, b)
    rows, counts, guards = twin_overlap(a, b, (0, 0, 0), capacity_for(want))
    assert np.all(guards == FILL), "the twin wrote outside the table"
    assert counts == [len(want), 0]
    assert records_as_set(rows) == want
    assert dict_as_set(T.label_overlaps(tensor(a), tensor(b))) == want


def test_one_pair_everywhere_counts_the_voxels():
    a, b = C.pair((5, 9, 130), "one-pair")
    assert R.overlap_table(a, b) == {(1, 1, 5 * 9 * 130)}


def test_the_run_cases_hold_what_they_promise():
    _, _, edges = C.runs_flat(int(np.prod(C.RUNS_SHAPE)))
    lengths = np.diff(edges)
    assert set(range(1, 131)) <= set(lengths.tolist())
    _, _, edges = C.runs_flat(5 * 9 * 130)
    inner = [(s, e) for s, e in zip(edges[:-1], edges[1:]) if e - s > 1]
    assert any(s // 64 != (e - 1) // 64 for s, e in inner), "a run crosses a wave boundary"
    assert any(s // 130 != (e - 1) // 130 for s, e in inner), "a run ends a row and continues on the next"


def test_runs_of_every_length():
    a, b, _ = C.runs_flat(int(np.prod(C.RUNS_SHAPE)))
    a, b = a.reshape(C.RUNS_SHAPE), b.reshape(C.RUNS_SHAPE)
    want = R.overlap_table(a, b)
    rows, counts, _ = twin_overlap(a, b, (0, 0, 0), capacity_for(want))
    assert counts == [len(want), 0] and records_as_set(rows) == want


def test_background_is_every_label_that_is_not_positive():
    a, b = C.pair((5, 9, 130), "background-values")
    want = R.overlap_table(a, b)
    assert {p[0] for p in want} == {p[1] for p in want} == {1, 2, 3}
    a, b = C.pair((5, 9, 130), "int32-max")
    assert (C.INT32_MAX, C.INT32_MAX) in {p[:2] for p in R.overlap_table(a, b)}, "the packing is unsigned"


def test_every_voxel_a_pair_of_its_own():
    a, b = C.distinct_pairs(LDS_SLOTS)
    want = R.overlap_table(a, b)
    assert len(want) == a.size > 2 * LDS_SLOTS
    for max_blocks in (0, 1):
        rows, counts, guards = twin_overlap(a, b, (0, 0, 0), capacity_for(want), max_blocks)
        assert np.all(guards == FILL) and counts == [len(want), 0] and records_as_set(rows) == want


SHIFTS = list(itertools.product((-1, 0, 2), repeat=3))
BEYOND = [(3, 0, 0), (-3, 0, 0), (0, 5, 0), (0, -5, 0), (0, 0, 7), (0, 0, -7), (4, 0, 0), (0, -6, 1), (1, 1, 100), (0, 0, -2 ** 31),
          (2 ** 31 - 1, 0, 0)]


def test_every_shift_of_a_small_volume():
    a, b = C.pair((3, 5, 7), "random-0..3")
    for shift in SHIFTS:
        want = R.overlap_table(a, b, shift)
        rows, counts, guards = twin_overlap(a, b, shift, 64)
        assert np.all(guards == FILL) and counts == [len(want), 0] and records_as_set(rows) == want, shift
    assert R.overlap_table(a, b, (2, 2, 2)) != R.overlap_table(a, b, (0, 0, 0))


def test_a_shift_at_or_beyond_the_shape_gives_an_empty_table():
    a, b = C.pair((3, 5, 7), "one-pair")
    for shift in BEYOND:
        assert R.overlap_table(a, b, shift) == set()
        rows, counts, guards = twin_overlap(a, b, shift, 8)
        assert counts == [0, 0] and not rows["pair"].any() and not rows["count"].any() and np.all(guards == FILL), shift
        table = T.label_overlaps(tensor(a), tensor(b), shift)
        assert len(table["a"]) == len(table["b"]) == len(table["count"]) == 0


def test_max_blocks_does_not_change_the_table():
    a, b = C.pair(*C.MANY_PAIRS)
    want = R.overlap_table(a, b)
    for max_blocks in (0, 1, 2):
        rows, counts, _ = twin_overlap(a, b, (0, 0, 0), capacity_for(want), max_blocks)
        assert counts == [len(want), 0] and records_as_set(rows) == want


def test_a_table_that_is_too_small_says_so_and_the_python_layer_retries():
    a, b = C.pair(*C.MANY_PAIRS)
    want = R.overlap_table(a, b)
    assert len(want) > 1000
    check_partial_table(*twin_overlap(a, b, (0, 0, 0), 2), want)
    assert dict_as_set(T.label_overlaps(tensor(a), tensor(b), _capacity=2)) == want


def test_entry_checks_refuse_with_a_message_and_write_nothing():
    a = np.ones((2, 3, 4), dtype=np.int32)
    b = np.ones((2, 3, 4), dtype=np.int32)
    table = np.full((8 * 4,), FILL, dtype=np.int32)
    counts = np.full((2,), FILL, dtype=np.int32)
    lib = _lib.load()
    seen = 0
    for what, args in entry_check_calls(a.ctypes.data, b.ctypes.data, table.ctypes.data, counts.ctypes.data):
        rc = lib.lsr_label_overlap_i32_cpu(*args, None)
        assert rc == E_ARG, what
        assert lib.lsr_last_error().decode(), what
        assert np.all(table == FILL) and np.all(counts == FILL) and np.all(a == 1) and np.all(b == 1), what
        seen += 1
    assert seen == 15
    with pytest.raises(_lib.LsrError, match="capacity"):
        _lib.call("lsr_label_overlap_i32_cpu", a.ctypes.data, b.ctypes.data, 2, 3, 4, shift3((0, 0, 0)), 3, table.ctypes.data,
                  counts.ctypes.data, 0, None)


def test_label_overlaps_checks_its_arguments():
    a = torch.ones((2, 3, 4), dtype=torch.int32)
    with pytest.raises(TypeError):
        T.label_overlaps(a.float(), a)
    with pytest.raises(ValueError):
        T.label_overlaps(a, torch.ones((2, 3, 5), dtype=torch.int32))
    with pytest.raises(ValueError):
        T.label_overlaps(a, a.transpose(1, 2))
    with pytest.raises(ValueError):
        T.label_overlaps(a, a, shift=(0, 0))
    with pytest.raises(ValueError):
        T.label_overlaps(a, a, _capacity=3)


# ---------------------------------------------------------------- linking and tracks


def settings(**kw):
    return TrackSettings(channel_name="GFP_labels", **kw)


def volumes_array(labels):
    return T.label_volumes(tensor(labels))


def check_tracks(frames, device=torch.device("cpu"), shifts=None, **kw):
    """``track_frames`` on ``device`` equals the restatement: tracks, per-object rows, and every voxel's track id."""
    s = settings(**kw)
    want_of, want_tracks, want_objects = R.tracks(frames, s.min_overlap_voxels, s.min_iou, s.divisions, shifts)
    tensors = [tensor(f, device) for f in frames]
    track_of, tracks = T.track_frames(iter(tensors), s, shifts)
    got = list(zip(*(tracks[c].tolist() for c in ("track_id", "t_begin", "t_end", "parent_track_id"))))
    assert got == want_tracks
    objects = tracks["objects"]
    rows = list(zip(*(objects[c].tolist() for c in ("t", "label", "track_id", "parent_label", "overlap_voxels", "iou"))))
    assert rows == want_objects                                   # (iou: the same float64 quotient)
    for t, frame in enumerate(frames):
        assert {k: int(v) for k, v in enumerate(track_of[t]) if v} == want_of[t]
        volume = T.relabel_by_track(tensors[t], track_of[t])
        assert volume.device == tensors[t].device and volume.dtype == torch.int32
        assert np.array_equal(volume.cpu().numpy(), R.track_volume(frame, want_of[t]))
        assert np.array_equal(tensors[t].cpu().numpy(), frame), "the labels are not changed"
    return want_tracks, want_objects


def test_the_scene_is_the_prototypes():
    frames = C.scene()
    assert [volumes_array(f)[1:].tolist() for f in frames] == C.SCENE_VOLUMES
    assert [list(R.volumes(f).values()) for f in frames] == C.SCENE_VOLUMES
    for t, want in enumerate(C.SCENE_TABLES):
        assert R.overlap_table(frames[t], frames[t + 1]) == want
        assert dict_as_set(T.label_overlaps(tensor(frames[t]), tensor(frames[t + 1]))) == want
    assert R.overlap_table(frames[0], frames[1], (0, 0, 2)) == C.SCENE_TABLE_SHIFTED
    assert dict_as_set(T.label_overlaps(tensor(frames[0]), tensor(frames[1]), (0, 0, 2))) == C.SCENE_TABLE_SHIFTED


def test_scene_tracks_with_divisions():
    tracks, objects = check_tracks(C.scene(), divisions=True)
    assert tracks == C.SCENE_TRACKS_DIVISIONS
    assert len(objects) == sum(len(v) for v in C.SCENE_VOLUMES)


def test_scene_tracks_without_divisions():
    tracks, _ = check_tracks(C.scene(), divisions=False)
    assert tracks == C.SCENE_TRACKS_NO_DIVISIONS              # B goes on in the daughter with the smaller label: 24 / 24


def test_scene_tracks_with_known_shifts():
    check_tracks(C.scene(), shifts=[(0, 0, 2)] * 4)


def test_link_frames_against_the_loops():
    frames = C.scene()
    for t in range(C.SCENE_T - 1):
        for kw in (dict(), dict(min_overlap_voxels=21), dict(min_iou=0.2), dict(min_overlap_voxels=25, min_iou=0.05)):
            table = T.label_overlaps(tensor(frames[t]), tensor(frames[t + 1]))
            va, vb = volumes_array(frames[t]), volumes_array(frames[t + 1])
            parent, overlap, iou = T.link_frames(table, va, vb, **kw)
            want = R.link(R.overlap_table(frames[t], frames[t + 1]), R.volumes(frames[t]), R.volumes(frames[t + 1]), **kw)
            assert parent[0] == overlap[0] == iou[0] == 0
            assert {b: (int(parent[b]), int(overlap[b]), float(iou[b])) for b in want} == want


SHAPE = (4, 8, 24)


def test_a_merge_goes_to_the_greater_count_and_ties_to_the_smaller_label():
    first = C.boxes(SHAPE, (1, 0, 4, 0, 4, 0, 6), (2, 0, 4, 0, 4, 8, 16))
    second = C.boxes(SHAPE, (1, 0, 4, 0, 4, 2, 12))                         # 64 voxels of 1, 64 of 2: a tie
    third = C.boxes(SHAPE, (1, 0, 4, 0, 4, 4, 12))                          # 32 of 1, 64 of 2
    for divisions in (True, False):
        tracks, objects = check_tracks([first, second], divisions=divisions)
        assert tracks == [(1, 0, 1, 0), (2, 0, 0, 0)] and objects[-1] == (1, 1, 1, 1, 64, 64 / (96 + 160 - 64))
        tracks, objects = check_tracks([first, third], divisions=divisions)
        assert tracks == [(1, 0, 0, 0), (2, 0, 1, 0)] and objects[-1][2:5] == (2, 2, 64)


def test_each_threshold_cuts_a_link():
    first = C.boxes(SHAPE, (1, 0, 4, 0, 4, 0, 8))                           # 128 voxels
    second = C.boxes(SHAPE, (1, 0, 4, 0, 4, 6, 14))                         # 128 voxels, 32 shared: IoU 32 / 224
    assert check_tracks([first, second])[0] == [(1, 0, 1, 0)]
    assert check_tracks([first, second], min_overlap_voxels=32)[0] == [(1, 0, 1, 0)]
    assert check_tracks([first, second], min_overlap_voxels=33)[0] == [(1, 0, 0, 0), (2, 1, 1, 0)]
    assert check_tracks([first, second], min_iou=32 / 224)[0] == [(1, 0, 1, 0)]
    assert check_tracks([first, second], min_iou=0.15)[0] == [(1, 0, 0, 0), (2, 1, 1, 0)]


def test_an_empty_frame_ends_every_track():
    first = C.boxes(SHAPE, (1, 0, 4, 0, 4, 0, 8), (2, 0, 4, 4, 8, 12, 20))
    empty = np.zeros(SHAPE, dtype=np.int32)
    tracks, _ = check_tracks([first, first, empty, first, first])
    assert tracks == [(1, 0, 1, 0), (2, 0, 1, 0), (3, 3, 4, 0), (4, 3, 4, 0)]


def test_no_objects_at_the_first_timepoint():
    first = C.boxes(SHAPE, (1, 0, 4, 0, 4, 0, 8))
    empty = np.zeros(SHAPE, dtype=np.int32)
    assert check_tracks([empty, first, first])[0] == [(1, 1, 2, 0)]
    assert check_tracks([empty, empty])[0] == []


def test_track_settings():
    s = settings()
    assert (s.min_overlap_voxels, s.min_iou, s.divisions) == (1, 0.0, True)
    for bad in (dict(min_overlap_voxels=0), dict(min_iou=-0.1), dict(min_iou=1.5), dict(gap=1)):
        with pytest.raises(ValueError):
            settings(**bad)


# ---------------------------------------------------------------- the command

SCALE = (1.0, 1.0, 0.5, 0.25, 0.25)
TRANSLATION = {"A/1/0": [0.0, 0.0, 1.5, -2.0, 3.25], "B/2/1": [0.0] * 5}
SEGMENT = {"channel_name": "GFP", "threshold": 50.0}
TRACK = {"channel_name": "GFP_labels", "divisions": True}


@pytest.fixture
def cpu_cli(monkeypatch):
    import shrimpy_amd.cli as cli

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    return cli


def make_store(path):
    """Two positions of the scene (the second runs backwards in time: merges), channels BF and GFP."""
    from shrimpy_amd.io.omezarr import open_ome_zarr

    with open_ome_zarr(path, layout="hcs", mode="w", channel_names=["BF", "GFP"], version="0.5", prefer_iohub=False) as plate:
        for p, key in enumerate(TRANSLATION):
            tr = TRANSLATION[key]
            arr = plate.create_position(*key.split("/")).create_zeros("0", shape=(C.SCENE_T, 2) + C.SCENE_SHAPE, dtype=np.uint16,
                                                                      scale=SCALE, translation=tr if any(tr) else None)
            for t in range(C.SCENE_T):
                arr.write_volume(t, 0, np.full(C.SCENE_SHAPE, 7, dtype=np.uint16))
                arr.write_volume(t, 1, (C.scene_mask(t if p == 0 else C.SCENE_T - 1 - t) * 100).astype(np.uint16))


def tree_digest(path):
    h = hashlib.sha256()
    for f in sorted(p for p in path.rglob("*") if p.is_file()):
        h.update(str(f.relative_to(path)).encode())
        h.update(f.read_bytes())
    return h.hexdigest()


def check_track_command(cli, tmp_path):
    """Shared with tests/test_track_gpu.py: ``segment`` then ``track`` on a temporary store, checked against the restatement."""
    from click.testing import CliRunner

    from shrimpy_amd.cli import TRACK_COLUMNS, TRACK_OBJECT_COLUMNS
    from shrimpy_amd.io.omezarr import open_ome_zarr, position_scale

    make_store(tmp_path / "in.zarr")
    seg, trk = tmp_path / "segment.yml", tmp_path / "track.yml"
    seg.write_text(yaml.safe_dump(SEGMENT))
    trk.write_text(yaml.safe_dump(TRACK))
    labels, out = tmp_path / "labels.zarr", tmp_path / "tracks.zarr"
    r = CliRunner().invoke(cli.cli, ["segment", "-i", str(tmp_path / "in.zarr"), "-c", str(seg), "-o", str(labels)])
    assert r.exit_code == 0, r.output
    before = tree_digest(labels)
    r = CliRunner().invoke(cli.cli, ["track", "-i", str(labels), "-c", str(trk), "-o", str(out), "--compression", "zstd"])
    assert r.exit_code == 0, r.output
    assert tree_digest(labels) == before, "the input store is untouched"
    with open_ome_zarr(labels, prefer_iohub=False) as src, open_ome_zarr(out, prefer_iohub=False) as plate:
        sources, positions = dict(src.positions()), dict(plate.positions())
        assert sorted(positions) == sorted(TRANSLATION)
        for key, pos in positions.items():
            assert list(pos.channel_names) == ["GFP_labels_tracks"] and pos.levels == ["0"]
            assert pos["0"].shape == (C.SCENE_T, 1) + C.SCENE_SHAPE and pos["0"].dtype == np.int32
            assert list(position_scale(pos)) == list(SCALE)
            assert list(cli._position_translation(pos)) == TRANSLATION[key]
            frames = [sources[key]["0"].read_volume(t, 0) for t in range(C.SCENE_T)]
            want_of, want_tracks, want_objects = R.tracks(frames)
            if key == "A/1/0":
                assert want_tracks == C.SCENE_TRACKS_DIVISIONS
            else:
                assert (3, 0, 2, 0) in want_tracks and all(row[3] == 0 for row in want_tracks)       # backwards: a merge, no division
            with open(out / key / "tracks.csv", newline="") as fh:
                rows = list(csv.reader(fh))
            assert tuple(rows[0]) == TRACK_COLUMNS
            assert [tuple(int(v) for v in row) for row in rows[1:]] == want_tracks
            with open(out / key / "track_objects.csv", newline="") as fh:
                rows = list(csv.reader(fh))
            assert tuple(rows[0]) == TRACK_OBJECT_COLUMNS
            assert [tuple(int(v) for v in row[:5]) + (float(row[5]),) for row in rows[1:]] == want_objects
            assert all(row[5] == repr(float(row[5])) for row in rows[1:]), "floats are written with repr"
            with open(labels / key / "objects.csv", newline="") as fh:
                objects = list(csv.DictReader(fh))
            assert [(row[0], row[1]) for row in rows[1:]] == [(o["t"], o["label"]) for o in objects]
            for t in range(C.SCENE_T):
                assert np.array_equal(pos["0"].read_volume(t, 0), R.track_volume(frames[t], want_of[t]))
    # clean errors: an output that exists, a channel that is not there, a store that holds no labels
    r = CliRunner().invoke(cli.cli, ["track", "-i", str(labels), "-c", str(trk), "-o", str(out)])
    assert r.exit_code != 0 and "exists" in r.output
    bad = tmp_path / "bad.yml"
    bad.write_text(yaml.safe_dump(dict(TRACK, channel_name="RFP_labels")))
    r = CliRunner().invoke(cli.cli, ["track", "-i", str(labels), "-c", str(bad), "-o", str(tmp_path / "x.zarr")])
    assert r.exit_code != 0 and "RFP_labels" in r.output and "Traceback" not in r.output and not (tmp_path / "x.zarr").exists()
    bad.write_text(yaml.safe_dump(dict(TRACK, min_iou=2.0)))
    r = CliRunner().invoke(cli.cli, ["track", "-i", str(labels), "-c", str(bad), "-o", str(tmp_path / "x.zarr")])
    assert r.exit_code != 0 and "min_iou" in r.output and not (tmp_path / "x.zarr").exists()
    # one position on request
    r = CliRunner().invoke(cli.cli, ["track", "-i", str(labels), "-c", str(trk), "-o", str(tmp_path / "one.zarr"), "-p", "B/2/1"])
    assert r.exit_code == 0, r.output
    assert (tmp_path / "one.zarr" / "B/2/1" / "tracks.csv").exists() and not (tmp_path / "one.zarr" / "A").exists()


def test_cli_track(tmp_path, cpu_cli):
    check_track_command(cpu_cli, tmp_path)


def test_cli_track_refuses_data_that_is_not_integer(tmp_path, cpu_cli):
    from click.testing import CliRunner

    from shrimpy_amd.io.omezarr import open_ome_zarr

    with open_ome_zarr(tmp_path / "f.zarr", layout="hcs", mode="w", channel_names=["GFP_labels"], version="0.5",
                       prefer_iohub=False) as plate:
        plate.create_position("A", "1", "0").create_zeros("0", shape=(2, 1, 2, 4, 4), dtype=np.float32, scale=SCALE)
    cfg = tmp_path / "track.yml"
    cfg.write_text(yaml.safe_dump(TRACK))
    r = CliRunner().invoke(cpu_cli.cli, ["track", "-i", str(tmp_path / "f.zarr"), "-c", str(cfg), "-o", str(tmp_path / "x.zarr")])
    assert r.exit_code != 0 and "integer" in r.output and not (tmp_path / "x.zarr").exists()
