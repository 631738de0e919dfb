"""The refusals that ``segment`` and ``track`` share (``cli._run_object_store``), each on both commands: an unknown position, a
channel that is not there, data that is not 5-D, a volume of more than 2^31 - 1 voxels and an output directory that is not
empty all end with a message, without a traceback, before anything is written."""

import numpy as np
import pytest
import torch
import yaml
from click.testing import CliRunner

SCALE = (1.0, 1.0, 0.5, 0.25, 0.25)
# per command: the store's dtype, its channels, the settings
COMMANDS = {"segment": (np.uint16, ["BF", "GFP"], {"channel_name": "GFP", "threshold": 50.0}),
            "track": (np.int32, ["GFP_labels"], {"channel_name": "GFP_labels"})}


@pytest.fixture
def cpu_cli(monkeypatch):
    import shrimpy_amd.cli as cli

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    return cli


class ShapeOnly:
    """Stands for a position's array in the checks that read nothing but its shape and dtype."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, np.dtype(dtype)


def invoke(cli, tmp_path, command, settings=None, extra=(), out=None):
    dtype, channels, default = COMMANDS[command]
    from shrimpy_amd.io.omezarr import open_ome_zarr

    if not (tmp_path / "in.zarr").exists():
        with open_ome_zarr(tmp_path / "in.zarr", layout="hcs", mode="w", channel_names=channels, version="0.5",
                           prefer_iohub=False) as plate:
            plate.create_position("A", "1", "0").create_zeros("0", shape=(1, len(channels), 2, 4, 4), dtype=dtype, scale=SCALE)
    cfg = tmp_path / "settings.yml"
    cfg.write_text(yaml.safe_dump(default if settings is None else settings))
    out = tmp_path / "out.zarr" if out is None else out
    r = CliRunner().invoke(cli.cli, [command, "-i", str(tmp_path / "in.zarr"), "-c", str(cfg), "-o", str(out), *extra])
    return r, out


def refused(r, out, *words):
    assert r.exit_code != 0 and r.exception.__class__ is SystemExit and "Traceback" not in r.output, r.output
    assert all(w in r.output for w in words), r.output
    assert not out.exists(), "nothing is written"


@pytest.mark.parametrize("command", sorted(COMMANDS))
def test_an_unknown_position_is_refused(tmp_path, cpu_cli, command):
    r, out = invoke(cpu_cli, tmp_path, command, extra=("-p", "Z/9/9"))
    refused(r, out, "positions ['Z/9/9'] not found; available: ['A/1/0']")


@pytest.mark.parametrize("command", sorted(COMMANDS))
def test_a_missing_channel_is_refused(tmp_path, cpu_cli, command):
    r, out = invoke(cpu_cli, tmp_path, command, settings=dict(COMMANDS[command][2], channel_name="RFP"))
    refused(r, out, "channel_name 'RFP' not in position A/1/0 (it has ", str(COMMANDS[command][1]))


@pytest.mark.parametrize("command", sorted(COMMANDS))
@pytest.mark.parametrize("shape, words", [
    ((2, 4, 4, 4), "position A/1/0: expected 5-D TCZYX data, got shape (2, 4, 4, 4)"),
    # 2^31 voxels, one more than fits (the shape is all the check reads: nothing of that size is allocated)
    ((1, 1, 2048, 1024, 1024), "position A/1/0: a volume of (2048, 1024, 1024) has more than 2^31 - 1 voxels"),
], ids=["not_5d", "too_many_voxels"])
def test_a_shape_that_cannot_be_labelled_is_refused(tmp_path, cpu_cli, monkeypatch, command, shape, words):
    import shrimpy_amd.io.omezarr as omezarr

    monkeypatch.setattr(omezarr, "as_volume_array", lambda array: ShapeOnly(shape, COMMANDS[command][0]))
    r, out = invoke(cpu_cli, tmp_path, command)
    refused(r, out, words)


@pytest.mark.parametrize("command", sorted(COMMANDS))
def test_an_output_directory_that_is_not_empty_is_refused(tmp_path, cpu_cli, command):
    out = tmp_path / "taken"
    out.mkdir()
    (out / "note.txt").write_text("mine")
    r, _ = invoke(cpu_cli, tmp_path, command, out=out)
    assert r.exit_code != 0 and r.exception.__class__ is SystemExit and "Traceback" not in r.output, r.output
    assert "exists (never overwritten)" in r.output
    assert sorted(p.name for p in out.iterdir()) == ["note.txt"] and (out / "note.txt").read_text() == "mine"
