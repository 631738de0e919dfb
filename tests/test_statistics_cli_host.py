"""The ``statistics`` command on the CPU, end to end through the host twins: a plate of two positions, three timepoints and two
channels of (6, 12, 20) as a uint16 store and as a float32 copy of other content.  ``statistics.csv`` and ``statistics.json``
equal numpy's figures at the levels volume, position and dataset; ``--write-metadata`` changes two keys of the position
groups and nothing else; every refusal comes before the output directory exists."""

import json

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from tests.test_measure_cli_host import KEYS, T, as_float, config, read_csv, scene, write_store

QUANTILES = [0.001, 0.01, 0.25, 0.5, 0.75, 0.99, 0.999]


def volume_of(store: str, p: int, t: int, c: int) -> np.ndarray:
    return scene(p, t)[c] if store == "u16" else as_float(scene(p, t)[1 - c])


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    import shrimpy_amd.cli as cli

    patch = pytest.MonkeyPatch()
    patch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    d = tmp_path_factory.mktemp("statistics")
    write_store(d / "u16.zarr", np.uint16, lambda p, t, c: volume_of("u16", p, t, c))
    write_store(d / "f32.zarr", np.float32, lambda p, t, c: volume_of("f32", p, t, c))
    yield cli, d
    patch.undo()


def run(cli, d, store, out, extra=(), **settings):
    args = ["statistics", "-i", str(d / f"{store}.zarr"), "-o", str(d / out), *extra]
    if settings:
        args += ["-c", str(config(d, f"statistics_{out}", **settings))]
    return CliRunner().invoke(cli.cli, args), d / out


def check(figures: dict, x: np.ndarray, what: str):
    """One entry of the CSV (strings) or of the JSON against numpy on the float64 copy of the voxels."""
    x = x.astype(np.float64).ravel()
    number = {k: float(v) for k, v in figures.items() if k != "channel"}
    assert number["count"] == x.size and number["nan_count"] == 0, what
    assert number["min"] == x.min() and number["max"] == x.max(), what
    assert abs(number["mean"] - x.mean()) <= 1e-12 * max(abs(x.mean()), 1.0), what
    assert abs(number["std"] - x.std()) <= 1e-9 * max(x.std(), 1.0), what
    for q in QUANTILES:
        want = np.quantile(x, q)
        assert abs(number[f"q_{q!r}"] - want) <= 8 * 2.0 ** -53 * np.abs(x).max(), f"{what}: quantile {q}"
    assert number["median"] == number["q_0.5"] and number["iqr"] == number["q_0.75"] - number["q_0.25"], what


@pytest.mark.parametrize("store", ["u16", "f32"])
def test_csv_and_json_equal_numpy_at_every_level(plate, store):
    cli, d = plate
    r, out = run(cli, d, store, f"all_{store}", levels=["volume", "position", "dataset"])
    assert r.exit_code == 0, r.output
    document = json.loads((out / "statistics.json").read_text())
    assert document["quantiles"] == QUANTILES and document["settings"]["levels"] == ["volume", "position", "dataset"]
    for p, key in enumerate(KEYS):
        rows = read_csv(out / key / "statistics.csv")
        assert [(int(r_["t"]), r_["channel"]) for r_ in rows] == [(t, c) for t in range(T) for c in ("A", "B")]
        for row in rows:
            check(row, volume_of(store, p, int(row["t"]), "AB".index(row["channel"])), f"{key} t {row['t']} {row['channel']}")
        for c, name in enumerate("AB"):
            entry = document["positions"][key][name]
            check({**{k: v for k, v in entry.items() if k != "quantiles"}, **entry["quantiles"]},
                  np.stack([volume_of(store, p, t, c) for t in range(T)]), f"{key} {name} pooled over t")
    for c, name in enumerate("AB"):
        entry = document["dataset"][name]
        check({**{k: v for k, v in entry.items() if k != "quantiles"}, **entry["quantiles"]},
              np.stack([volume_of(store, p, t, c) for p in range(len(KEYS)) for t in range(T)]), f"dataset {name}")


def test_defaults_one_position_and_named_channels(plate):
    cli, d = plate
    r, out = run(cli, d, "u16", "defaults", extra=["-p", KEYS[1]])
    assert r.exit_code == 0, r.output
    assert not (out / KEYS[0]).exists() and len(read_csv(out / KEYS[1] / "statistics.csv")) == 2 * T
    document = json.loads((out / "statistics.json").read_text())
    assert "positions" not in document and "dataset" not in document
    r, out = run(cli, d, "u16", "named", channel_names=["B"], quantiles=[0.9], levels=["position"])
    assert r.exit_code == 0, r.output
    document = json.loads((out / "statistics.json").read_text())
    assert list(document["positions"][KEYS[0]]) == ["B"] and document["quantiles"] == [0.25, 0.5, 0.75, 0.9]
    assert not (out / KEYS[0]).exists()          # (no volume level: no CSV)


def test_write_metadata_changes_two_keys_only(plate):
    cli, d = plate
    write_store(d / "meta.zarr", np.uint16, lambda p, t, c: volume_of("u16", p, t, c))
    before = {f: f.read_bytes() for f in sorted((d / "meta.zarr").rglob("*")) if f.is_file()}
    r, out = run(cli, d, "meta", "meta_out", extra=["--write-metadata"], levels=["position", "dataset"])
    assert r.exit_code == 0, r.output
    document = json.loads((out / "statistics.json").read_text())
    after = {f: f.read_bytes() for f in sorted((d / "meta.zarr").rglob("*")) if f.is_file()}
    assert sorted(before) == sorted(after)
    changed = [f for f in before if before[f] != after[f]]
    assert sorted(changed) == sorted(d / "meta.zarr" / key / "zarr.json" for key in KEYS)
    for key in KEYS:
        old, new = (json.loads(blob[d / "meta.zarr" / key / "zarr.json"])["attributes"]["ome"] for blob in (before, after))
        normalization, omero = new.pop("normalization"), new.pop("omero")
        old_omero = old.pop("omero", None)
        assert old == new, "another key of the group's attributes changed"
        for name in "AB":
            fov, whole = document["positions"][key][name], document["dataset"][name]
            assert normalization[name] == {"fov_statistics": {f: fov[f] for f in ("mean", "std", "median", "iqr")},
                                           "dataset_statistics": {f: whole[f] for f in ("mean", "std", "median", "iqr")}}
            channel = omero["channels"]["AB".index(name)]
            assert channel["window"] == {"min": fov["min"], "max": fov["max"], "start": fov["quantiles"]["q_0.001"],
                                         "end": fov["quantiles"]["q_0.999"]}
            if old_omero is not None:
                was = dict(old_omero["channels"]["AB".index(name)])
                now = dict(channel)
                was.pop("window", None), now.pop("window")
                assert was == now
    # the store still opens and reads as it did
    from tests.test_measure_cli_host import read_volume

    assert np.array_equal(read_volume(cli, d / "meta.zarr", KEYS[1], 2, 1), volume_of("u16", 1, 2, 1))


def test_refusals_come_before_the_output_exists(plate):
    cli, d = plate
    for name, extra, settings in [
        ("unknown_channel", [], dict(channel_names=["C"])),
        ("bad_quantile", [], dict(quantiles=[1.5])),
        ("bad_level", [], dict(levels=["plate"])),
        ("metadata_without_levels", ["--write-metadata"], dict(levels=["volume", "position"])),
        ("metadata_without_window", ["--write-metadata"], dict(levels=["position", "dataset"], quantiles=[0.5])),
        ("unknown_position", ["-p", "C/3/0"], {}),
    ]:
        r, out = run(cli, d, "u16", f"refused_{name}", extra=extra, **settings)
        assert r.exit_code != 0 and not out.exists(), f"{name}: {r.output}"
    (d / "exists").mkdir()
    r, _ = run(cli, d, "u16", "exists")
    assert r.exit_code != 0 and not any((d / "exists").iterdir())
