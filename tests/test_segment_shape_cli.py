"""``run_segment`` with ``shape`` and ``contacts`` on a tiny store on the CPU: the header order of ``objects.csv``, the presence
and the rows of ``contacts.csv``, and with the defaults today's header and no ``contacts.csv``."""

import csv

import numpy as np
import torch
import yaml

from shrimpy_amd import segment as S
from tests import moments_cases as C
from tests import moments_ref as R
from tests.test_label_host import cpu_cli  # noqa: F401 -- the fixture
from tests.test_shape_host import SPLIT_SETTINGS

SCALE = (1.0, 1.0, 2.0, 0.5, 0.5)
KEY = "A/1/0"


def make_store(path):
    """One position, two timepoints of channel GFP: the two touching balls, then nothing."""
    from shrimpy_amd.io.omezarr import open_ome_zarr

    balls = C.two_balls()
    with open_ome_zarr(path, layout="hcs", mode="w", channel_names=["GFP"], version="0.5", prefer_iohub=False) as plate:
        arr = plate.create_position(*KEY.split("/")).create_zeros("0", shape=(2, 1) + balls.shape, dtype=np.uint16, scale=SCALE)
        arr.write_volume(0, 0, balls.astype(np.uint16))
        arr.write_volume(1, 0, np.zeros(balls.shape, dtype=np.uint16))


def run(cli, tmp_path, name, settings):
    cfg = tmp_path / f"{name}.yml"
    cfg.write_text(yaml.safe_dump(settings))
    out = tmp_path / f"{name}.zarr"
    result = cli.run_segment(str(tmp_path / "in.zarr"), cfg, out, compression="zstd")
    return out / KEY, result


def read(path):
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    return tuple(rows[0]), [dict(zip(rows[0], row)) for row in rows[1:]]


def test_run_segment_shape_and_contacts(tmp_path, cpu_cli):  # noqa: F811
    cli = cpu_cli
    make_store(tmp_path / "in.zarr")
    # the defaults: today's header, no contacts.csv; spelled out, the same bytes
    plain, _ = run(cli, tmp_path, "plain", SPLIT_SETTINGS)
    spelled, _ = run(cli, tmp_path, "spelled", dict(SPLIT_SETTINGS, shape=False, contacts=False))
    assert read(plain / "objects.csv")[0] == cli.OBJECT_COLUMNS
    assert (plain / "objects.csv").read_bytes() == (spelled / "objects.csv").read_bytes()
    assert not (plain / "contacts.csv").exists() and not (spelled / "contacts.csv").exists()

    both, _ = run(cli, tmp_path, "both", dict(SPLIT_SETTINGS, shape=True, contacts=True, inscribed_radius=True))
    header, rows = read(both / "objects.csv")
    assert header == cli.OBJECT_COLUMNS + ("inscribed_radius_um",) + cli.SHAPE_OBJECT_COLUMNS
    assert cli.SHAPE_OBJECT_COLUMNS == ("axis_length_major_um", "axis_length_mid_um", "axis_length_minor_um", "major_axis_z",
                                        "major_axis_y", "major_axis_x", "surface_area_um2", "contact_area_um2", "n_neighbours",
                                        "touches_border")
    assert [(int(r["t"]), int(r["label"])) for r in rows] == [(0, 1), (0, 2)]
    # the columns it had keep their values
    _, before = read(plain / "objects.csv")
    assert [[r[c] for c in cli.OBJECT_COLUMNS] for r in rows] == [[r[c] for c in cli.OBJECT_COLUMNS] for r in before]
    # ... and the new ones are shape_table's of the written labels, in micrometres
    from shrimpy_amd.io.omezarr import open_ome_zarr

    with open_ome_zarr(tmp_path / "both.zarr", prefer_iohub=False) as plate:
        labels = dict(plate.positions())[KEY]["0"].read_volume(0, 0)
    want = S.shape_table(torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)), 2, SCALE[2:])
    for k, r in enumerate(rows):
        assert [float(r[c]) for c in cli.SHAPE_OBJECT_COLUMNS[:3]] == want["axis_lengths"][k].tolist()
        assert [float(r[c]) for c in cli.SHAPE_OBJECT_COLUMNS[3:6]] == want["major_axis"][k].tolist()
        assert float(r["surface_area_um2"]) == want["surface_area"][k] and float(r["contact_area_um2"]) == want["contact_area"][k]
        assert int(r["n_neighbours"]) == 1 and r["touches_border"] in ("0", "1")
    header, touching = read(both / "contacts.csv")
    assert header == cli.CONTACT_COLUMNS == ("t", "label_a", "label_b", "faces_z", "faces_y", "faces_x", "area_um2")
    _, contacts = R.faces_and_contacts(labels, 2)
    fz, fy, fx = contacts[1, 2]
    assert len(touching) == 1 and [int(touching[0][c]) for c in header[:6]] == [0, 1, 2, fz, fy, fx]
    assert float(touching[0]["area_um2"]) == fz * 0.25 + fy * 1.0 + fx * 1.0

    # contacts alone: objects.csv is today's, contacts.csv is there; where nothing touches, the header alone
    alone, _ = run(cli, tmp_path, "alone", dict(SPLIT_SETTINGS, contacts=True))
    assert (alone / "objects.csv").read_bytes() == (plain / "objects.csv").read_bytes()
    assert (alone / "contacts.csv").read_bytes() == (both / "contacts.csv").read_bytes()
    apart, _ = run(cli, tmp_path, "apart", dict(channel_name="GFP", threshold=0.5, contacts=True))
    assert (apart / "contacts.csv").read_text().splitlines() == [",".join(cli.CONTACT_COLUMNS)]


def test_the_help_text_names_both_settings():
    import shrimpy_amd.cli as cli

    text = cli.segment.help
    assert "shape: true" in text and "contacts: true" in text and "contacts.csv" in text
