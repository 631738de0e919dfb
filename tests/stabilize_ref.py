"""Synthetic drifting series and stores shared by ``test_stabilize_host.py`` and ``test_stabilize_gpu.py``."""

from __future__ import annotations

import numpy as np
import yaml

from tests import focus_ref as R

BASE_SHAPE, BASE_FOCUS = (12, 40, 48), 6
# known integer drifts (dz, dy, dx) per timepoint, |d| <= 3, timepoint 0 at rest
DRIFTS = {"0/0/000": [(0, 0, 0), (1, -2, 3), (-3, 1, -1), (2, 3, 0)],
          "0/1/000": [(0, 0, 0), (-1, 0, 2), (-2, -3, 1), (3, 2, -2)]}
CHANNELS = ["BF", "GFP"]
PIXEL = R.OPTICS["pixel_size"]
FOCUS_SETTINGS = dict(NA_det=R.OPTICS["NA_det"], lambda_ill=R.OPTICS["lambda_ill"], midband_fractions=list(R.FRACTIONS))


def base_volume(seed=None):
    return R.stack(*BASE_SHAPE, BASE_FOCUS, seed=seed)


def series(drifts, seed=None):
    base = base_volume(seed)
    return [np.roll(base, d, axis=(0, 1, 2)) for d in drifts]


def settings_dict(method, kind, t_reference="first"):
    return dict(stabilization_estimation_channel="BF", stabilization_channels=["BF"], stabilization_type=kind,
                stabilization_method=method, focus_finding_settings=dict(FOCUS_SETTINGS),
                phase_cross_corr_settings=dict(t_reference=t_reference))


def shifted_back(volume, shift):
    """``out[i] = volume[i + shift]`` where that lies inside the volume, zero elsewhere (numpy slicing)."""
    out = np.zeros(volume.shape, dtype=np.float32)
    dst, src = [], []
    for n, s in zip(volume.shape, (int(v) for v in shift)):
        dst.append(slice(max(0, -s), min(n, n - s)))
        src.append(slice(max(0, s), min(n, n + s)))
    out[tuple(dst)] = volume[tuple(src)]
    return out


def make_store(path):
    """Two positions, T = 4, channels BF (the drifting stack) and GFP (another one); returns {key: (T, C, Z, Y, X) uint16}."""
    from shrimpy_amd.io.omezarr import open_ome_zarr

    data = {}
    with open_ome_zarr(path, layout="hcs", mode="w", channel_names=CHANNELS, version="0.5", prefer_iohub=False) as plate:
        for p, (key, drifts) in enumerate(DRIFTS.items()):
            bf = series(drifts, seed=100 + p)
            gfp = series(drifts, seed=200 + p)
            d = np.stack([np.stack([a, b]) for a, b in zip(bf, gfp)]).astype(np.uint16)
            pos = plate.create_position(*key.split("/"))
            arr = pos.create_zeros("0", shape=d.shape, dtype=np.uint16, scale=(1, 1, 1.0, PIXEL, PIXEL))
            for t in range(d.shape[0]):
                for c in range(d.shape[1]):
                    arr.write_volume(t, c, d[t, c])
            data[key] = d
    return data


def run_cli_round_trip(tmp_path, method="phase-cross-corr", kind="xyz"):
    """estimate-stabilization then stabilize on a fresh store: (input data, {key: matrices}, {key: output array})."""
    from click.testing import CliRunner

    import shrimpy_amd.cli as cli

    from shrimpy_amd.io.omezarr import open_ome_zarr
    from shrimpy_amd.settings import StabilizationSettings

    data = make_store(tmp_path / "series.zarr")
    cfg = tmp_path / "estimate.yml"
    cfg.write_text(yaml.safe_dump(settings_dict(method, kind)))
    runner = CliRunner()
    res = runner.invoke(cli.cli, ["estimate-stabilization", "-i", str(tmp_path / "series.zarr"), "-c", str(cfg), "-o",
                                  str(tmp_path / "stab")], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    matrices = {}
    for key in DRIFTS:
        f = tmp_path / "stab" / (key.replace("/", "_") + ".yml")
        matrices[key] = np.asarray(StabilizationSettings.from_yaml(f).affine_transform_zyx_list)
    res = runner.invoke(cli.cli, ["stabilize", "-i", str(tmp_path / "series.zarr"), "-c", str(tmp_path / "stab"), "-o",
                                  str(tmp_path / "out.zarr"), "--compression", "none"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    out = {}
    with open_ome_zarr(tmp_path / "out.zarr", layout="auto", mode="r", prefer_iohub=False) as plate:
        for key, pos in plate.positions():
            assert list(pos.channel_names) == CHANNELS
            out[key] = np.asarray(pos["0"][:])
    return data, matrices, out


def check_round_trip(data, matrices, out):
    for key, drifts in DRIFTS.items():
        assert out[key].dtype == np.float32 and out[key].shape == data[key].shape
        for t, d in enumerate(drifts):
            assert matrices[key][t][:3, 3].tolist() == [float(v) for v in d], (key, t)
            assert np.array_equal(matrices[key][t][:3, :3], np.eye(3))
            bf = data[key][t, 0].astype(np.float32)
            assert np.array_equal(out[key][t, 0], shifted_back(bf, d)), (key, t)
            assert np.array_equal(out[key][t, 1], data[key][t, 1].astype(np.float32)), (key, t)    # GFP: copied
