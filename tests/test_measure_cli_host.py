"""The ``measure`` command on the CPU, end to end through the host twins: a plate of two positions, three timepoints and two
channels of (6, 12, 20) as a uint16 store and as a float32 store of other content, labelled by ``run_segment`` and tracked by
``run_track``.  ``measure`` on the ``segment`` output reproduces ``objects.csv``'s intensity columns for the segmented channel
and numpy's values for the other channel and the other store; on the ``track`` output it gives one row per track id and
timepoint; a ball of 100 on a pedestal of 40 is 60 above its ring; every refusal comes before the output directory exists."""

import csv

import numpy as np
import pytest
import torch
import yaml
from click.testing import CliRunner

SCALE = (1.0, 1.0, 0.5, 0.25, 0.25)
TRANSLATION = (0.0, 0.0, 3.0, -2.0, 10.0)
KEYS = ("A/1/0", "B/2/0")
SHAPE, T = (6, 12, 20), 3
# objects.csv's bound and this table's added, relative to a sum of positive terms: (1 + 2) n_k 2^-53 with n_k = 60 voxels a box
BOUND = 3 * 60 * 2.0 ** -53


def scene(position: int, t: int):
    """Two boxes that drift by one voxel per timepoint: channel A (bright boxes on a dim noise floor) and channel B (noise)."""
    rng = np.random.default_rng(100 * position + t)
    a = rng.integers(0, 20, SHAPE)
    for z0, y0, x0 in ((1, 1 + t, 2 + position), (2, 6, 11 + t)):
        a[z0:z0 + 3, y0:y0 + 4, x0:x0 + 5] = 200 + rng.integers(0, 50, (3, 4, 5))
    return a.astype(np.uint16), rng.integers(0, 1000, SHAPE).astype(np.uint16)


def as_float(u16: np.ndarray) -> np.ndarray:
    """The float32 store's content: another function of the scene, with a fraction and both signs."""
    return (u16.astype(np.float32) * np.float32(0.37) - np.float32(25.5)).astype(np.float32)


def write_store(path, dtype, volumes, channels=("A", "B"), keys=KEYS, scale=SCALE, timepoints=T, shape=SHAPE):
    from shrimpy_amd.io.omezarr import open_ome_zarr

    with open_ome_zarr(path, layout="hcs", mode="w", channel_names=list(channels), version="0.5", prefer_iohub=False) as plate:
        for p, key in enumerate(keys):
            arr = plate.create_position(*key.split("/")).create_zeros("0", shape=(timepoints, len(channels)) + tuple(shape),
                                                                     dtype=dtype, scale=scale, translation=TRANSLATION)
            for t in range(timepoints):
                for c in range(len(channels)):
                    arr.write_volume(t, c, volumes(p, t, c).astype(dtype))


def read_volume(cli, path, key, t, c=0):
    from shrimpy_amd.io.omezarr import as_volume_array

    store, positions = cli._open_source(path, "native")
    try:
        return np.array(as_volume_array(positions[key]["0"]).read_volume(t, c))
    finally:
        close = getattr(store, "close", None)
        if close:
            close()


def read_csv(path):
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


def config(directory, name, **settings):
    path = directory / f"{name}.yml"
    path.write_text(yaml.safe_dump(settings))
    return path


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    """``(cli, directory)``: u16.zarr, f32.zarr, seg.zarr (``run_segment`` of channel A) and trk.zarr (``run_track`` of that)."""
    import shrimpy_amd.cli as cli

    patch = pytest.MonkeyPatch()
    patch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    d = tmp_path_factory.mktemp("measure")
    write_store(d / "u16.zarr", np.uint16, lambda p, t, c: scene(p, t)[c])
    write_store(d / "f32.zarr", np.float32, lambda p, t, c: as_float(scene(p, t)[1 - c]))
    cli.run_segment(d / "u16.zarr", config(d, "segment", channel_name="A", threshold=100.0), d / "seg.zarr")
    cli.run_track(d / "seg.zarr", config(d, "track", channel_name="A_labels"), d / "trk.zarr")
    yield cli, d
    patch.undo()


def measure(cli, d, labels, inputs, out, extra=(), **settings):
    cfg = config(d, f"measure_{out}", **settings)
    r = CliRunner().invoke(cli.cli, ["measure", "-l", str(d / labels), "-i", str(d / inputs), "-c", str(cfg), "-o", str(d / out), *extra])
    return r, d / out


def numpy_rows(labels, values, t, names):
    """What measurements.csv must hold for one timepoint: per label with voxels the values of every channel, from numpy."""
    sz, sy, sx = SCALE[2:]
    rows = []
    for k in range(1, int(labels.max()) + 1):
        inside = labels == k
        if not inside.any():
            continue
        row = {"t": t, "label": k, "volume_voxels": int(inside.sum()), "volume_um3": float(inside.sum()) * sz * sy * sx}
        zyx = np.argwhere(inside).astype(np.float64)
        for name, volume in zip(names, values):
            v = volume[inside].astype(np.float64)
            centroid = (zyx * v[:, None]).sum(0) / v.sum()
            row.update({f"{name}_sum": v.sum(), f"{name}_mean": v.mean(), f"{name}_std": v.std(), f"{name}_min": v.min(),
                        f"{name}_max": v.max(),
                        **{f"{name}_weighted_centroid_{axis}_um": TRANSLATION[2 + i] + centroid[i] * SCALE[2 + i]
                           for i, axis in enumerate("zyx")}})
        rows.append(row)
    return rows


def assert_rows(got, want, rel):
    assert len(got) == len(want) and len(want) > 0
    for g, w in zip(got, want):
        assert list(g)[:4] == ["t", "label", "volume_voxels", "volume_um3"] and set(g) == set(w)
        for name, value in w.items():
            if name in ("t", "label", "volume_voxels"):
                assert int(g[name]) == value, name
            else:
                assert float(g[name]) == pytest.approx(value, rel=rel, abs=1e-9), (name, g["t"], g["label"])


def test_measure_on_the_segment_output_reproduces_objects_csv_and_numpy(plate):
    cli, d = plate
    r, out = measure(cli, d, "seg.zarr", "u16.zarr", "m_u16", label_channel_name="A_labels", channels=["A", "B"])
    assert r.exit_code == 0, r.output
    for p, key in enumerate(KEYS):
        rows = read_csv(out / key / "measurements.csv")
        objects = read_csv(d / "seg.zarr" / key / "objects.csv")
        assert [(o["t"], o["label"]) for o in objects] == [(m["t"], m["label"]) for m in rows] and len(rows) >= 2 * T
        for o, m in zip(objects, rows):
            assert m["volume_voxels"] == o["volume_voxels"] and float(m["volume_um3"]) == float(o["volume_um3"])
            # uint16 sums are exact integers, and so are objects.csv's float64 sums of them: far inside the bound
            for theirs, ours in (("intensity_sum", "A_sum"), ("intensity_mean", "A_mean"), ("intensity_min", "A_min"),
                                 ("intensity_max", "A_max")):
                assert abs(float(m[ours]) - float(o[theirs])) <= BOUND * abs(float(o[theirs])), ours
            assert "." not in m["A_sum"] and "." not in m["A_min"], "uint16 sums and extremes are written as integers"
            for i, axis in enumerate("zyx"):
                um = TRANSLATION[2 + i] + float(o[f"weighted_centroid_{axis}"]) * SCALE[2 + i]
                assert float(m[f"A_weighted_centroid_{axis}_um"]) == pytest.approx(um, rel=1e-12, abs=1e-12)
        want = []
        for t in range(T):
            want += numpy_rows(read_volume(cli, d / "seg.zarr", key, t), scene(p, t), t, ("A", "B"))
        assert_rows(rows, want, rel=1e-12)


def test_measure_the_float32_store_and_all_channels_in_store_order(plate):
    cli, d = plate
    r, out = measure(cli, d, "seg.zarr", "f32.zarr", "m_f32", label_channel_name="A_labels", channels=None)
    assert r.exit_code == 0, r.output
    for p, key in enumerate(KEYS):
        rows = read_csv(out / key / "measurements.csv")
        header = list(rows[0])
        assert header[4] == "A_sum" and header[12] == "B_sum" and len(header) == 4 + 2 * 8
        want = []
        for t in range(T):
            a, b = scene(p, t)
            want += numpy_rows(read_volume(cli, d / "seg.zarr", key, t), (as_float(b), as_float(a)), t, ("A", "B"))
        # (sum_sq / n - mean^2 in float64 against numpy's two-pass std: eight digits are left at these values)
        assert_rows(rows, want, rel=1e-7)
        assert any("." in m["A_min"] for m in rows), "float32 extremes are written as floats"
    # one named channel, the second: its columns alone
    r, out = measure(cli, d, "seg.zarr", "f32.zarr", "m_b", extra=("-p", KEYS[1]), label_channel_name="A_labels", channels=["B"])
    assert r.exit_code == 0, r.output
    assert not (out / KEYS[0]).exists()
    assert list(read_csv(out / KEYS[1] / "measurements.csv")[0])[4:] == [
        "B_sum", "B_mean", "B_std", "B_min", "B_max", "B_weighted_centroid_z_um", "B_weighted_centroid_y_um", "B_weighted_centroid_x_um"]


def test_measure_on_the_track_output_gives_one_row_per_track_and_timepoint(plate):
    cli, d = plate
    r, out = measure(cli, d, "trk.zarr", "u16.zarr", "m_trk", label_channel_name="A_labels_tracks", channels=["B"])
    assert r.exit_code == 0, r.output
    for key in KEYS:
        rows = read_csv(out / key / "measurements.csv")
        linked = read_csv(d / "trk.zarr" / key / "track_objects.csv")
        assert sorted((int(o["t"]), int(o["track_id"])) for o in linked) == [(int(m["t"]), int(m["label"])) for m in rows]
        tracks = read_csv(d / "trk.zarr" / key / "tracks.csv")
        assert any(int(k["t_end"]) > int(k["t_begin"]) for k in tracks), "no track spans two timepoints"
        for k in tracks:
            curve = [m for m in rows if m["label"] == k["track_id"]]
            assert [int(m["t"]) for m in curve] == list(range(int(k["t_begin"]), int(k["t_end"]) + 1))


def test_a_ball_on_a_pedestal_is_sixty_above_its_ring(plate):
    """A ball of radius 4 voxels at the centre of (20, 24, 24) at 0.5 um per voxel: 100 in the ball, 40 around it.  The ring from
    0.6 um to 1.6 um (squared distances of 2 .. 10 voxels, none on a threshold) ends 7.2 voxels from the centre, inside the volume."""
    cli, d = plate
    shape = (20, 24, 24)
    z, y, x = np.indices(shape)
    ball = (z - 10) ** 2 + (y - 12) ** 2 + (x - 12) ** 2 <= 16
    write_store(d / "ball.zarr", np.uint16, lambda p, t, c: np.where(ball, 100, 40), channels=("GFP",), keys=KEYS[:1],
                scale=(1.0, 1.0, 0.5, 0.5, 0.5), timepoints=1, shape=shape)
    write_store(d / "ball_labels.zarr", np.int32, lambda p, t, c: ball.astype(np.int32) * 3, channels=("mask",), keys=KEYS[:1],
                scale=(1.0, 1.0, 0.5, 0.5, 0.5), timepoints=1, shape=shape)
    r, out = measure(cli, d, "ball_labels.zarr", "ball.zarr", "m_ball", label_channel_name="mask", background_distance=1.0,
                     background_gap=0.6)
    assert r.exit_code == 0, r.output
    rows = read_csv(out / KEYS[0] / "measurements.csv")
    assert len(rows) == 1 and rows[0]["label"] == "3" and int(rows[0]["volume_voxels"]) == int(ball.sum())
    assert list(rows[0])[-3:] == ["GFP_background_voxels", "GFP_background_mean", "GFP_mean_minus_background"]
    from scipy import ndimage

    dist = ndimage.distance_transform_edt(~ball, sampling=(0.5, 0.5, 0.5))
    assert int(rows[0]["GFP_background_voxels"]) == int(((dist > 0.6) & (dist <= 1.6)).sum()) > 0
    assert float(rows[0]["GFP_background_mean"]) == 40.0 and float(rows[0]["GFP_mean"]) == 100.0
    assert float(rows[0]["GFP_mean_minus_background"]) == 60.0


def refused(r, out, *words):
    assert r.exit_code != 0 and r.exception.__class__ is SystemExit and "Traceback" not in r.output, r.output
    assert all(w in r.output for w in words), r.output
    assert not out.exists(), "the output directory was created"


def test_refusals_come_before_the_output_directory(plate):
    cli, d = plate
    ok = dict(label_channel_name="A_labels", channels=["A"])
    r, out = measure(cli, d, "seg.zarr", "u16.zarr", "r_position", extra=("-p", "Z/9/9"), **ok)
    refused(r, out, "positions ['Z/9/9'] not found")
    r, out = measure(cli, d, "seg.zarr", "u16.zarr", "r_label_channel", label_channel_name="nuclei")
    refused(r, out, "label_channel_name 'nuclei' not in position A/1/0")
    r, out = measure(cli, d, "seg.zarr", "u16.zarr", "r_channel", label_channel_name="A_labels", channels=["A", "RFP"])
    refused(r, out, "channels ['RFP'] not in position A/1/0")
    r, out = measure(cli, d, "f32.zarr", "u16.zarr", "r_float_labels", label_channel_name="A")
    refused(r, out, "position A/1/0: label data type float32")
    r, out = measure(cli, d, "u16.zarr", "seg.zarr", "r_int_values", label_channel_name="A")
    refused(r, out, "position A/1/0: intensity data type int32")
    r, out = measure(cli, d, "seg.zarr", "u16.zarr", "r_settings", label_channel_name="A_labels", background_radius=1.0)
    refused(r, out, "background_radius")
    # a label store that lacks the second position
    write_store(d / "one.zarr", np.int32, lambda p, t, c: np.ones(SHAPE), channels=("A_labels",), keys=KEYS[:1])
    r, out = measure(cli, d, "one.zarr", "u16.zarr", "r_missing", **ok)
    refused(r, out, "position B/2/0 not found in")
    # ... whose timepoints, shape or scale differ
    write_store(d / "short.zarr", np.int32, lambda p, t, c: np.ones(SHAPE), channels=("A_labels",), timepoints=2)
    r, out = measure(cli, d, "short.zarr", "u16.zarr", "r_t", **ok)
    refused(r, out, "position A/1/0: the labels are (T, Z, Y, X) = (2, 6, 12, 20), the intensities (3, 6, 12, 20)")
    write_store(d / "wide.zarr", np.int32, lambda p, t, c: np.ones((6, 12, 21)), channels=("A_labels",), shape=(6, 12, 21))
    r, out = measure(cli, d, "wide.zarr", "u16.zarr", "r_shape", **ok)
    refused(r, out, "position A/1/0: the labels are (T, Z, Y, X) = (3, 6, 12, 21)")
    write_store(d / "coarse.zarr", np.int32, lambda p, t, c: np.ones(SHAPE), channels=("A_labels",), scale=(1.0, 1.0, 0.5, 0.25, 0.5))
    r, out = measure(cli, d, "coarse.zarr", "u16.zarr", "r_scale", **ok)
    refused(r, out, "position A/1/0: the labels' (z, y, x) scale is")
    # ... one of whose labels does not fit int32
    write_store(d / "big.zarr", np.int64, lambda p, t, c: np.full(SHAPE, 2 ** 31 if (p, t) == (1, 2) else 7), channels=("A_labels",))
    r, out = measure(cli, d, "big.zarr", "u16.zarr", "r_int32", **ok)
    refused(r, out, "position B/2/0, t = 2: a label does not fit int32")
    # an output directory that exists, even an empty one
    (d / "taken").mkdir()
    r, out = measure(cli, d, "seg.zarr", "u16.zarr", "taken", **ok)
    assert r.exit_code != 0 and "exists (never overwritten)" in r.output and not any((d / "taken").iterdir())


def test_labels_of_a_wider_type_that_fit_are_measured(plate):
    cli, d = plate
    write_store(d / "int64.zarr", np.int64, lambda p, t, c: np.where(scene(p, t)[0] > 100, 5, np.where(scene(p, t)[1] > 990, -1, 0)),
                channels=("mask",))
    r, out = measure(cli, d, "int64.zarr", "u16.zarr", "m_int64", label_channel_name="mask", channels=["A"])
    assert r.exit_code == 0, r.output
    rows = read_csv(out / KEYS[0] / "measurements.csv")
    assert [(m["t"], m["label"]) for m in rows] == [(str(t), "5") for t in range(T)]      # (negative labels are ignored)
    assert all(int(m["A_min"]) >= 200 for m in rows)
