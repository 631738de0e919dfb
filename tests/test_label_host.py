"""Labelling on the host: the twins (``lsr_label_f32_cpu``, ``lsr_label_regions_f32_cpu``, ``lsr_label_remap_i32_cpu``) against
``scipy.ndimage.label`` (``tests/label_ref.py``: exact equality), the entry statuses of twin and device entry alike, the
settings, ``shrimpy_amd.segment`` on CPU tensors and the ``segment`` command.

Cases: ``tests/label_cases.py``, sized from the tile of the local launch.
"""

import csv
import ctypes

import numpy as np
import pytest
import torch
import yaml

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from shrimpy_amd.settings import SegmentSettings
from tests import label_cases as C
from tests import label_ref as R

GUARD = 64
FILL = -7
# one scratch buffer for every call of this module, never cleared between them (and poisoned to begin with)
SCRATCH = np.full(1 << 16, 0xA5, dtype=np.uint8)


def twin_label(vol, threshold, connectivity):
    """The twin through the C ABI into a buffer pre-filled with -7 with 64 guard words behind it: (labels, n, guard)."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    z, y, x = vol.shape
    assert _lib.call_value("lsr_label_scratch_bytes", z, y, x) <= SCRATCH.nbytes
    buf = np.full(vol.size + GUARD, FILL, dtype=np.int32)
    count = np.full(1, FILL, dtype=np.int32)
    _lib.call("lsr_label_f32_cpu", vol.ctypes.data, z, y, x, ctypes.c_float(threshold), connectivity, buf.ctypes.data,
              count.ctypes.data, SCRATCH.ctypes.data, None)
    return buf[:vol.size].reshape(vol.shape), int(count[0]), buf[vol.size:]


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))            # (a copy: the shared cases and references are read-only)


# ---- the twin against scipy ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_equals_scipy_label(name, connectivity):
    case = C.case(name)
    want, n_want = R.case_labels(name, connectivity)
    got, n, guard = twin_label(case["vol"], case["threshold"], connectivity)
    assert np.all(guard == FILL), "the twin wrote behind its output"
    assert not np.any(got == FILL), "a voxel was not written"
    assert n == n_want
    assert np.array_equal(got, want)
    fixed = C.expected_count(name, connectivity)
    assert fixed is None or n == fixed, "the case is not what its construction says"
    again, n2, _ = twin_label(case["vol"], case["threshold"], connectivity)
    assert n2 == n and got.tobytes() == again.tobytes()


def test_the_cases_aim_at_the_tile_faces():
    tz, ty, tx = C.T
    assert min(C.T) >= 1 and C.case("all_fg")["vol"].shape == (2 * tz + 1, 2 * ty + 1, 2 * tx + 1)
    assert C.case("serpentine")["vol"].shape == (3, 2 * ty + 3, 2 * tx + 5)
    assert C.case("spiral")["vol"].shape[1] > 3 * ty and C.case("spiral")["vol"].shape[2] > 3 * tx
    assert C.case("noise_p0.3")["vol"].shape == (9, 70, 1030) and all(n % t for n, t in zip((9, 70, 1030), C.T))
    assert len([n for n in C.NAMES if n.startswith("pair_")]) == 13
    joined = {k: sum(C.expected_count(n, k) == 1 for n in C.NAMES if n.startswith("pair_")) for k in C.CONNECTIVITIES}
    assert joined == {6: 3, 18: 9, 26: 13}
    # the serpentine is one path: every voxel has at most two face neighbours, and under 6 it is one component
    path = C.case("serpentine")["vol"] > 0
    pad = np.pad(path, 1)
    nb = sum(np.roll(pad, s, axis=a) for a in range(3) for s in (-1, 1))[1:-1, 1:-1, 1:-1]
    assert nb[path].max() == 2 and (nb[path] == 1).sum() == 2 and path.sum() > path.size // 4


def test_threshold_semantics_by_hand():
    vol = np.array([[[0.0, np.nan, np.inf, -np.inf, -0.0, 1e-45, 1.0, 0.0, 2.0]]], dtype=np.float32)
    got, n, _ = twin_label(vol, 0.0, 6)
    assert got.ravel().tolist() == [0, 0, 1, 0, 0, 2, 2, 0, 3] and n == 3
    got, n, _ = twin_label(vol, float("nan"), 26)                      # nothing is greater than NaN
    assert n == 0 and not got.any()
    got, n, _ = twin_label(vol, float("-inf"), 6)                       # -inf itself is not greater than -inf
    assert got.ravel().tolist() == [1, 0, 2, 0, 3, 3, 3, 3, 3] and n == 3


# ---- the object table -----------------------------------------------------------------------------------------------------------

TABLE_CASES = [("all_fg", 6), ("checkerboard", 6), ("noise_p0.05", 26), ("noise_p0.3", 6), ("nested_us", 18), ("runs_x", 6),
               ("threshold_semantics", 18)]


@pytest.mark.parametrize("name,connectivity", TABLE_CASES, ids=[f"{n}-{k}" for n, k in TABLE_CASES])
def test_twin_table_equals_the_restatement(name, connectivity):
    labels, n = R.case_labels(name, connectivity)
    inten = C.intensities(name)
    want = R.table(labels, n, inten)
    got = S.region_table(_t(labels), n, _t(inten))
    worst = R.check_table(got, want)
    print(f"{name}-{connectivity}: {n} objects, worst float64 sum error / bound = {worst:.3f}")
    assert np.allclose(got["centroid"], want["centroid"], rtol=0, atol=0, equal_nan=True)
    plain = S.region_table(_t(labels), n)                               # without intensities: the integer columns alone
    assert "intensity_sum" not in plain
    R.check_table(plain, R.table(labels, n))


def test_table_of_nothing_is_empty_and_foreign_labels_are_ignored():
    labels = np.zeros((2, 3, 4), dtype=np.int32)
    got = S.region_table(_t(labels), 0, _t(np.ones((2, 3, 4), dtype=np.float32)))
    assert all(len(v) == 0 for v in got.values()) and "intensity_sum" in got
    lib = _lib.load()
    assert lib.lsr_label_regions_f32_cpu(labels.ctypes.data, None, 2, 3, 4, 0, None, None) == 0
    labels[0, 0, :] = [1, 5, -3, 2]                                      # 5 and -3 are outside 1 .. 2
    got = S.region_table(_t(labels), 2)
    assert got["volume"].tolist() == [1, 1] and got["bbox"].tolist() == [[0, 0, 0, 1, 1, 1], [0, 0, 3, 1, 1, 4]]


# ---- the filter -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("min_volume,keep_largest", [(0, False), (2, False), (10 ** 9, False), (0, True), (2, True), (10 ** 9, True)])
def test_filter_matches_the_numpy_restatement(min_volume, keep_largest):
    labels, n = R.case_labels("noise_p0.2", 6)
    work = _t(labels.copy())
    got, table, m = S.filter_objects(work, S.region_table(work, n), min_volume, keep_largest)
    want, m_want = R.filter_labels(labels, min_volume, keep_largest)
    assert got is work and m == m_want and np.array_equal(got.numpy(), want)
    assert table["label"].tolist() == list(range(1, m + 1))             # consecutive
    assert np.array_equal(table["volume"], np.bincount(want.ravel(), minlength=m + 1)[1:])
    assert (m == 0) == (min_volume == 10 ** 9) and (not keep_largest or m <= 1)


def test_keep_largest_with_a_tie_keeps_the_lowest_label():
    vol = np.zeros((1, 5, 9), dtype=np.float32)
    vol[0, 0, 0:2] = vol[0, 2, 0:3] = vol[0, 4, 5:8] = vol[0, 4, 0] = 1          # volumes 2, 3, 1, 3 in label order
    labels, n = S.label_volume(_t(vol), 0.5)
    assert n == 4
    table = S.region_table(labels, n)
    assert table["volume"].tolist() == [2, 3, 1, 3]
    assert S.filter_map(table["volume"], 0, True).tolist() == [0, 0, 1, 0, 0]
    got, kept, m = S.filter_objects(labels, table, keep_largest=True)
    want, _ = R.filter_labels(R.label(vol, 0.5, 6)[0], 0, True)
    assert m == 1 and np.array_equal(got.numpy(), want) and got.numpy()[0, 2, 1] == 1 and kept["volume"].tolist() == [3]


# ---- entry statuses ---------------------------------------------------------------------------------------------------------------


def test_entry_statuses():
    lib = _lib.load()
    zyx = (ctypes.c_int * 3)()
    assert lib.lsr_label_tile_shape(zyx) == 0 and tuple(zyx) == C.T and lib.lsr_label_tile_shape(None) == -1
    five = (ctypes.c_int64 * 5)()
    assert lib.lsr_label_launch_geometry(five) == 0 and tuple(five) == S.launch_geometry() and min(five) >= 1
    assert lib.lsr_label_launch_geometry(None) == -1 and b"NULL" in lib.lsr_last_error()
    assert lib.lsr_label_scratch_bytes(4, 5, 6) > 0
    assert lib.lsr_label_scratch_bytes(0, 5, 6) == -2 and lib.lsr_label_scratch_bytes(2 ** 11, 2 ** 10, 2 ** 10) == -3
    big = lib.lsr_label_scratch_bytes(1500, 1024, 518)               # 7.96e8 voxels: the config-2 deskewed grid fits
    assert 0 < big <= 1 << 21
    vol = np.ones((2, 3, 4), dtype=np.float32)
    out = np.full(24, FILL, dtype=np.int32)
    count = np.full(1, FILL, dtype=np.int32)
    v, o, c, s = vol.ctypes.data, out.ctypes.data, count.ctypes.data, SCRATCH.ctypes.data
    thr = ctypes.c_float(0.5)
    for name in ("lsr_label_f32_cpu", "lsr_label_f32"):                # (checked before anything is launched: safe without a GPU)
        fn = getattr(lib, name)
        assert fn(None, 2, 3, 4, thr, 6, o, c, s, None) == -1
        assert fn(v, 2, 3, 4, thr, 6, None, c, s, None) == -1
        assert fn(v, 2, 3, 4, thr, 6, o, None, s, None) == -1
        assert fn(v, 2, 3, 4, thr, 6, o, c, None, None) == -1 and b"scratch is NULL" in lib.lsr_last_error()
        assert fn(v, 0, 3, 4, thr, 6, o, c, s, None) == -2
        assert fn(v, 2, -3, 4, thr, 6, o, c, s, None) == -2
        assert fn(v, 2, 3, 0, thr, 6, o, c, s, None) == -2
        for bad in (0, 4, 8, 7, 27, -6):
            assert fn(v, 2, 3, 4, thr, bad, o, c, s, None) == -4 and b"6, 18 or 26" in lib.lsr_last_error()
        assert fn(v, 2 ** 11, 2 ** 10, 2 ** 10, thr, 6, o, c, s, None) == -3           # 2^31 voxels: one too many
        assert fn(v, 2 ** 40, 2 ** 40, 2 ** 40, thr, 6, o, c, s, None) == -3
    # the timing entry of tools/bench_kernels.py --label: lsr_label_f32's checks, then its own pointer
    ms7 = (ctypes.c_float * 7)(*([-1.0] * 7))
    fn = lib.lsr_label_profile_f32
    assert fn(None, 2, 3, 4, thr, 6, o, c, s, ms7, None) == -1 and fn(v, 2, 3, 4, thr, 6, o, c, None, ms7, None) == -1
    assert fn(v, 2, 0, 4, thr, 6, o, c, s, ms7, None) == -2 and fn(v, 2, 3, 4, thr, 8, o, c, s, ms7, None) == -4
    assert fn(v, 2 ** 11, 2 ** 10, 2 ** 10, thr, 6, o, c, s, ms7, None) == -3
    assert fn(v, 2, 3, 4, thr, 6, o, c, s, None, None) == -1 and b"ms7 is NULL" in lib.lsr_last_error()
    assert list(ms7) == [-1.0] * 7
    for name in ("lsr_label_regions_f32_cpu", "lsr_label_regions_f32"):
        fn = getattr(lib, name)
        assert fn(None, None, 2, 3, 4, 1, s, None) == -1
        assert fn(o, None, 2, 3, 4, 1, None, None) == -1
        assert fn(o, None, 2, 0, 4, 1, s, None) == -2
        assert fn(o, None, 2, 3, 4, -1, s, None) == -4
    for name in ("lsr_label_remap_i32_cpu", "lsr_label_remap_i32"):
        fn = getattr(lib, name)
        assert fn(None, 24, s, 2, None) == -1 and fn(o, 24, None, 2, None) == -1
        assert fn(o, 0, s, 2, None) == -2 and fn(o, 2 ** 31, s, 2, None) == -3 and fn(o, 24, s, 0, None) == -4
    assert np.all(out == FILL) and count[0] == FILL, "a refused call wrote something"
    assert lib.lsr_label_f32_cpu(v, 2, 3, 4, thr, 6, o, c, s, None) == 0 and np.all(out == 1) and count[0] == 1


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------


def test_label_volume_on_cpu_tensors():
    case = C.case("noise_p0.3")
    for k in C.CONNECTIVITIES:
        labels, n = S.label_volume(_t(case["vol"]), case["threshold"], k)
        want, n_want = R.case_labels("noise_p0.3", k)
        assert labels.dtype == torch.int32 and labels.device.type == "cpu" and labels.shape == want.shape
        assert n == n_want and np.array_equal(labels.numpy(), want)
    with pytest.raises(ValueError):
        S.label_volume(_t(case["vol"]), 0.5, connectivity=8)
    with pytest.raises(TypeError):
        S.label_volume(_t(case["vol"].astype(np.float64)), 0.5)
    with pytest.raises(ValueError):
        S.label_volume(_t(case["vol"][0]), 0.5)


def test_settings():
    s = SegmentSettings(channel_name="GFP", threshold="otsu", sigma=1.0, min_volume=4)
    assert s.connectivity == 6 and s.otsu_component == 0 and not s.keep_largest
    assert "scipy" in SegmentSettings.__doc__ and "skimage" in SegmentSettings.__doc__
    assert SegmentSettings(channel_name="GFP", threshold=3).threshold == 3.0
    for bad in (dict(connectivity=8), dict(threshold="li"), dict(sigma=-1.0), dict(min_volume=-1), dict(unknown=1),
                dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            SegmentSettings(**{"channel_name": "GFP", "threshold": 1.0, **bad})


def blob_volume(seed, shape=(12, 40, 48)):
    """Three separated blobs on a dark background plus bright single-voxel debris (uint16-valued float32)."""
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, 8, size=shape).astype(np.float32)
    vol[2:7, 4:12, 5:14] += 1000.0
    vol[4:10, 20:30, 8:16] += 1200.0
    vol[3:8, 10:18, 30:42] += 900.0
    for z, y, x in ((1, 34, 40), (10, 3, 25), (6, 35, 4)):
        vol[z, y, x] = DEBRIS
    return vol


DEBRIS = 2800.0        # blurred with sigma 1 its peak is 0.0635 of this (178) and its face neighbours 0.0385 (108), Otsu's cut
#                        between dark and blobs about 148: one voxel passes, two where the volume's face mirrors it
SETTINGS = dict(channel_name="GFP", threshold="otsu", sigma=1.0, min_volume=4)


def reference_segmentation(vol, settings):
    """The blur and the threshold are the package's (``dynatrack``, pinned by its own tests); labelling and filtering scipy's
    and numpy's.  Returns (labels, M, objects before the filter)."""
    from shrimpy_amd import dynatrack as D

    work = D._gaussian_blur_3d(_t(vol), settings["sigma"])
    thr = D._multiotsu_threshold(work, 0)
    before, n = R.label(work.numpy(), thr, settings.get("connectivity", 6))
    after, m = R.filter_labels(before, settings["min_volume"], False)
    return after, m, n


def test_segment_zyx_on_the_host():
    vol = blob_volume(5)
    want, m, n_before = reference_segmentation(vol, SETTINGS)
    assert m == 3 and n_before > 3, "the debris must pass the threshold for the filter to have work"
    labels, table, n = S.segment_zyx(_t(vol), SegmentSettings(**SETTINGS))
    assert n == 3 and np.array_equal(labels.numpy(), want)
    R.check_table(table, R.table(want, 3, vol))
    one, table1, n1 = S.segment_zyx(_t(vol), SegmentSettings(**dict(SETTINGS, keep_largest=True)))
    assert n1 == 1 and np.array_equal(one.numpy(), R.filter_labels(want, 0, True)[0]) and len(table1["volume"]) == 1
    flat, _, n0 = S.segment_zyx(_t(np.full((3, 4, 5), 7.0, dtype=np.float32)), SegmentSettings(**SETTINGS))
    assert n0 == 0 and not flat.any()                                    # a constant volume has no objects


# ---- the command ------------------------------------------------------------------------------------------------------------------

SCALE = (1.0, 1.0, 0.5, 0.25, 0.25)
TRANSLATION = {"A/1/0": [0.0, 0.0, 1.5, -2.0, 3.25], "B/2/1": [0.0] * 5}


@pytest.fixture
def cpu_cli(monkeypatch):
    import shrimpy_amd.cli as cli

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    return cli


def make_store(path):
    """Two positions, two timepoints, channels GFP (the blobs) and BF; returns {(key, t): the GFP volume}."""
    from shrimpy_amd.io.omezarr import open_ome_zarr

    vols = {}
    with open_ome_zarr(path, layout="hcs", mode="w", channel_names=["BF", "GFP"], version="0.5", prefer_iohub=False) as plate:
        for p, key in enumerate(TRANSLATION):
            tr = TRANSLATION[key]
            arr = plate.create_position(*key.split("/")).create_zeros("0", shape=(2, 2, 12, 40, 48), dtype=np.uint16, scale=SCALE,
                                                                      translation=tr if any(tr) else None)
            for t in range(2):
                vols[key, t] = blob_volume(10 * p + t)
                arr.write_volume(t, 0, np.full((12, 40, 48), 7, dtype=np.uint16))
                arr.write_volume(t, 1, vols[key, t].astype(np.uint16))
    return vols


def check_segment_command(cli, tmp_path):
    """Shared with tests/test_label_gpu.py: the command on a temporary store, checked against the restatement."""
    from click.testing import CliRunner

    from shrimpy_amd.cli import OBJECT_COLUMNS
    from shrimpy_amd.io.omezarr import open_ome_zarr, position_scale

    vols = make_store(tmp_path / "in.zarr")
    cfg = tmp_path / "segment.yml"
    cfg.write_text(yaml.safe_dump(SETTINGS))
    out = tmp_path / "labels.zarr"
    r = CliRunner().invoke(cli.cli, ["segment", "-i", str(tmp_path / "in.zarr"), "-c", str(cfg), "-o", str(out), "--compression",
                                     "zstd"])
    assert r.exit_code == 0, r.output
    with open_ome_zarr(out, prefer_iohub=False) as plate:
        positions = dict(plate.positions())
        assert sorted(positions) == sorted(TRANSLATION)
        for key, pos in positions.items():
            assert list(pos.channel_names) == ["GFP_labels"] and pos.levels == ["0"]
            assert pos["0"].shape == (2, 1, 12, 40, 48) and pos["0"].dtype == np.int32
            assert list(position_scale(pos)) == list(SCALE)                          # the scale is copied
            assert list(cli._position_translation(pos)) == TRANSLATION[key]          # ... and the translation
            with open(out / key / "objects.csv", newline="") as fh:
                rows = list(csv.DictReader(fh))
            assert tuple(rows[0]) == OBJECT_COLUMNS and len(rows) == 6               # three objects at each of two timepoints
            for t in range(2):
                got = pos["0"].read_volume(t, 0)
                want, m, n_before = reference_segmentation(vols[key, t], SETTINGS)
                assert m == 3 and n_before > 3 and got.max() == 3 and np.array_equal(got, want)
                ref = R.table(want, 3, vols[key, t])
                mine = [row for row in rows if int(row["t"]) == t]
                assert [int(row["label"]) for row in mine] == [1, 2, 3]
                sz, sy, sx = SCALE[2:]
                for k, row in enumerate(mine):
                    assert int(row["volume_voxels"]) == ref["volume"][k]
                    assert float(row["volume_um3"]) == ref["volume"][k] * sz * sy * sx
                    assert [int(row[c]) for c in OBJECT_COLUMNS[4:10]] == ref["bbox"][k].tolist()
                    assert [float(row[f"centroid_{a}"]) for a in "zyx"] == ref["centroid"][k].tolist()
                    um = [o + c * s_ for o, c, s_ in zip(TRANSLATION[key][2:], ref["centroid"][k], SCALE[2:])]
                    assert [float(row[f"centroid_{a}_um"]) for a in "zyx"] == um
                    assert abs(float(row["intensity_sum"]) - ref["intensity_sum"][k]) <= ref["bound_sum"][k]
                    assert float(row["intensity_mean"]) == pytest.approx(ref["intensity_mean"][k], rel=1e-12)
                    assert np.float32(row["intensity_min"]) == ref["intensity_min"][k]
                    assert np.float32(row["intensity_max"]) == ref["intensity_max"][k]
                    assert [float(row[f"weighted_centroid_{a}"]) for a in "zyx"] == pytest.approx(
                        ref["weighted_centroid"][k].tolist(), rel=1e-12)
    # clean errors: an unknown channel, a connectivity that is none of the three, an output that exists
    bad = tmp_path / "bad.yml"
    bad.write_text(yaml.safe_dump(dict(SETTINGS, channel_name="RFP")))
    r = CliRunner().invoke(cli.cli, ["segment", "-i", str(tmp_path / "in.zarr"), "-c", str(bad), "-o", str(tmp_path / "x.zarr")])
    assert r.exit_code != 0 and "RFP" in r.output and "Traceback" not in r.output and not (tmp_path / "x.zarr").exists()
    bad.write_text(yaml.safe_dump(dict(SETTINGS, connectivity=8)))
    r = CliRunner().invoke(cli.cli, ["segment", "-i", str(tmp_path / "in.zarr"), "-c", str(bad), "-o", str(tmp_path / "x.zarr")])
    assert r.exit_code != 0 and "connectivity" in r.output and r.exception.__class__ is SystemExit
    assert not (tmp_path / "x.zarr").exists()
    r = CliRunner().invoke(cli.cli, ["segment", "-i", str(tmp_path / "in.zarr"), "-c", str(cfg), "-o", str(out)])
    assert r.exit_code != 0 and "exists" in r.output
    r = CliRunner().invoke(cli.cli, ["segment", "--help"])
    assert "--levels" not in r.output.replace("no --levels", "") and "pyramid of labels is meaningless" in " ".join(r.output.split())


def test_cli_segment(tmp_path, cpu_cli):
    check_segment_command(cpu_cli, tmp_path)
