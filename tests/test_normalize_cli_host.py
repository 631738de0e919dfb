"""The ``normalize`` command on the CPU, end to end through the host twins, and ``segment``'s percentile threshold: on a plate
of two positions, three timepoints and two channels, ``level: dataset`` reproduces ``(v - sub) / div`` with
``statistics.json``'s figures bit for bit and copies the other channel; ``level: volume`` on a series that decays by 0.9 per
timepoint gives equal medians; a constant volume is reported as degenerate; ``--resume`` works; the refusals come before the
output store exists; ``threshold: {percentile: 99}`` labels what ``scipy.ndimage.label(vol > np.percentile(vol, 99))`` labels."""

import json

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from tests.test_measure_cli_host import KEYS, SHAPE, T, config, read_volume, scene, write_store


def decaying(p: int, t: int, c: int) -> np.ndarray:
    """Channel A: one scene per position times 0.9^t; channel B: constant 7 (degenerate under every method)."""
    if c == 1:
        return np.full(SHAPE, 7, np.float32)
    return (scene(p, 0)[1].astype(np.float32) + np.float32(50)) * np.float32(0.9 ** t)


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    import shrimpy_amd.cli as cli

    patch = pytest.MonkeyPatch()
    patch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    d = tmp_path_factory.mktemp("normalize")
    write_store(d / "u16.zarr", np.uint16, lambda p, t, c: scene(p, t)[c])
    write_store(d / "decay.zarr", np.float32, decaying)
    cfg = config(d, "statistics", levels=["position", "dataset"], quantiles=[0.01, 0.999])
    r = CliRunner().invoke(cli.cli, ["statistics", "-i", str(d / "u16.zarr"), "-c", str(cfg), "-o", str(d / "stats")])
    assert r.exit_code == 0, r.output
    yield cli, d
    patch.undo()


def normalize(cli, d, store, out, extra=(), **settings):
    cfg = config(d, f"normalize_{out}", **settings)
    r = CliRunner().invoke(cli.cli, ["normalize", "-i", str(d / store), "-c", str(cfg), "-o", str(d / out), "--compression", "none", *extra])
    return r, d / out


def rescaled(v, sub, div, clip=None):
    o = (v.astype(np.float32) - np.float32(sub)) / np.float32(div)
    return o if clip is None else np.clip(o, np.float32(clip[0]), np.float32(clip[1]))


@pytest.mark.parametrize("level,method,clip", [("dataset", "percentile", True), ("position", "zscore", False), ("dataset", "robust", False)])
def test_store_levels_reproduce_the_json_figures(plate, level, method, clip):
    cli, d = plate
    r, out = normalize(cli, d, "u16.zarr", f"{level}_{method}.zarr", channel_names=["A"], method=method, level=level, clip=clip,
                       lower_percentile=1, upper_percentile=99.9, statistics_dirpath=str(d / "stats"))
    assert r.exit_code == 0, r.output
    document = json.loads((d / "stats" / "statistics.json").read_text())
    for p, key in enumerate(KEYS):
        e = document["dataset"]["A"] if level == "dataset" else document["positions"][key]["A"]
        sub, div = {"percentile": (e["quantiles"]["q_0.01"], e["quantiles"]["q_0.999"] - e["quantiles"]["q_0.01"]),
                    "zscore": (e["mean"], e["std"]), "robust": (e["median"], e["iqr"])}[method]
        for t in range(T):
            got = read_volume(cli, out, key, t, 0)
            assert got.dtype == np.float32
            assert got.tobytes() == rescaled(scene(p, t)[0], sub, div, (0.0, 1.0) if clip else None).tobytes(), f"{key} t {t}"
            assert np.array_equal(read_volume(cli, out, key, t, 1), scene(p, t)[1].astype(np.float32)), "channel B is copied"


def test_volume_level_undoes_a_decay_and_reports_a_constant_channel(plate):
    cli, d = plate
    cfg = config(d, "normalize_decay", channel_names=["A", "B"], method="percentile", level="volume")
    result = cli.run_normalize(d / "decay.zarr", cfg, d / "decay_out.zarr", compression=None)
    medians = {key: [float(np.median(read_volume(cli, d / "decay_out.zarr", key, t, 0).astype(np.float64))) for t in range(T)]
               for key in KEYS}
    for key, m in medians.items():
        before = [float(np.median(decaying(KEYS.index(key), t, 0))) for t in range(T)]
        assert before[2] < 0.82 * before[0]
        assert np.allclose(m, m[0], rtol=0, atol=1e-5), f"{key}: medians {m} after the normalization"
    assert sorted((u["position"], u["t"], u["c"]) for u in result["degenerate"]) == [(k, t, 1) for k in KEYS for t in range(T)]
    assert not read_volume(cli, d / "decay_out.zarr", KEYS[0], 1, 1).any()          # (7 - 7) / 1


def test_resume_completes_a_finished_store_without_rewriting(plate):
    cli, d = plate
    settings = dict(channel_names=["A"], method="robust", level="volume")
    r, out = normalize(cli, d, "u16.zarr", "resume.zarr", **settings)
    assert r.exit_code == 0, r.output
    first = read_volume(cli, out, KEYS[1], 2, 0)
    r, _ = normalize(cli, d, "u16.zarr", "resume.zarr", **settings)
    assert r.exit_code != 0, "an existing store is refused without --resume"
    r, _ = normalize(cli, d, "u16.zarr", "resume.zarr", extra=["--resume"], **settings)
    assert r.exit_code == 0, r.output
    assert np.array_equal(read_volume(cli, out, KEYS[1], 2, 0), first)
    r, _ = normalize(cli, d, "u16.zarr", "resume.zarr", extra=["--resume"], **dict(settings, method="zscore"))
    assert r.exit_code != 0, "other settings are another fingerprint"


def test_refusals_come_before_the_output_exists(plate):
    cli, d = plate
    stats = str(d / "stats")
    for name, settings in [
        ("unknown_channel", dict(channel_names=["C"])),
        ("no_channel", dict(channel_names=[])),
        ("clip_without_percentile", dict(channel_names=["A"], method="zscore", clip=True)),
        ("percentiles_reversed", dict(channel_names=["A"], lower_percentile=99, upper_percentile=1)),
        ("level_without_directory", dict(channel_names=["A"], level="dataset")),
        ("no_json", dict(channel_names=["A"], level="dataset", statistics_dirpath=str(d))),
        ("quantile_not_in_json", dict(channel_names=["A"], level="dataset", statistics_dirpath=stats, lower_percentile=5)),
    ]:
        r, out = normalize(cli, d, "u16.zarr", f"refused_{name}.zarr", **settings)
        assert r.exit_code != 0 and not out.exists(), f"{name}: {r.output}"
    # a statistics.json without the position asked for
    cfg = config(d, "statistics_one", levels=["position"])
    r = CliRunner().invoke(cli.cli, ["statistics", "-i", str(d / "u16.zarr"), "-c", str(cfg), "-o", str(d / "stats_one"), "-p", KEYS[0]])
    assert r.exit_code == 0, r.output
    for level in ("position", "dataset"):
        r, out = normalize(cli, d, "u16.zarr", f"refused_lacks_{level}.zarr", channel_names=["A"], method="zscore", level=level,
                           statistics_dirpath=str(d / "stats_one"))
        assert r.exit_code != 0 and not out.exists() and "statistics.json lacks" in r.output, r.output


def test_segment_percentile_threshold_labels_what_scipy_labels(plate):
    ndi = pytest.importorskip("scipy.ndimage")
    cli, d = plate
    cfg = config(d, "segment_percentile", channel_name="A", threshold={"percentile": 99})
    cli.run_segment(d / "u16.zarr", cfg, d / "seg.zarr")
    for p, key in enumerate(KEYS):
        for t in range(T):
            vol = scene(p, t)[0]
            want, n = ndi.label(vol > np.percentile(vol, 99))
            got = read_volume(cli, d / "seg.zarr", key, t, 0)
            assert n > 0 and int(got.max()) == n and np.array_equal(got != 0, want != 0)
            # (the numbering is raster order of the first voxel on both sides)
            assert np.array_equal(got.astype(np.int64), want.astype(np.int64))
    for bad in ({"percentile": 101}, {"percentile": 50, "other": 1}, {"quantile": 0.5}):
        with pytest.raises(Exception):
            cli.run_segment(d / "u16.zarr", config(d, "segment_bad", channel_name="A", threshold=bad), d / "seg_bad.zarr")
        assert not (d / "seg_bad.zarr").exists()
