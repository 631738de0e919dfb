"""Time-lapse stabilization on the host (CPU tensors through the twins): drift estimation on synthetic series with known
integer drifts, the settings models, and the ``estimate-stabilization`` / ``stabilize`` commands end to end."""

import numpy as np
import pytest
import torch
import yaml

from shrimpy_amd.settings import EstimateStabilizationSettings, StabilizationSettings
from shrimpy_amd.stabilize import apply_stabilization, estimate_stabilization, fill_missing
from tests import focus_ref as R
from tests import stabilize_ref as S

DRIFT = S.DRIFTS["0/0/000"]


@pytest.fixture(scope="module")
def volumes():
    return S.series(DRIFT)


def _shifts(matrices):
    for m in matrices:
        assert m.shape == (4, 4) and np.array_equal(m[:3, :3], np.eye(3)) and m[3].tolist() == [0, 0, 0, 1]
    return [tuple(int(v) for v in m[:3, 3]) for m in matrices]


def test_base_volume_focus(volumes):
    assert R.focus_index(R.power(volumes[0], **R.OPTICS)) == S.BASE_FOCUS


def test_focus_finding_z(volumes):
    got = _shifts(estimate_stabilization((torch.from_numpy(v) for v in volumes), S.settings_dict("focus-finding", "z"), S.PIXEL))
    assert got == [(d[0], 0, 0) for d in DRIFT]
    assert got == _shifts(R.drift_series(volumes, "focus-finding", "z"))


@pytest.mark.parametrize("t_reference", ["first", "previous"])
def test_phase_cross_corr_xyz(volumes, t_reference):
    s = S.settings_dict("phase-cross-corr", "xyz", t_reference)
    got = _shifts(estimate_stabilization((torch.from_numpy(v) for v in volumes), s, S.PIXEL))
    assert got == [tuple(d) for d in DRIFT]
    assert got == _shifts(R.drift_series(volumes, "phase-cross-corr", "xyz", t_reference))


def test_phase_cross_corr_xy(volumes):
    got = _shifts(estimate_stabilization(volumes, S.settings_dict("phase-cross-corr", "xy"), S.PIXEL))
    assert got == [(0, d[1], d[2]) for d in DRIFT]


def test_focus_finding_xyz(volumes, monkeypatch):
    # z from the focus measure, y and x from the correlation: a correlation that lies about z must not matter
    import shrimpy_amd.dynatrack as dt

    real = dt._phase_cross_corr
    monkeypatch.setattr(dt, "_phase_cross_corr", lambda *a, **k: (99,) + tuple(real(*a, **k))[1:])
    got = _shifts(estimate_stabilization((torch.from_numpy(v) for v in volumes), S.settings_dict("focus-finding", "xyz"), S.PIXEL))
    assert got == [tuple(d) for d in DRIFT]


def test_streamed_no_more_than_two_resident(volumes):
    import gc
    import weakref

    alive = []

    def stream():
        for v in volumes:
            t = torch.from_numpy(v.copy())
            alive.append(weakref.ref(t))
            yield t
            del t
            gc.collect()
            assert sum(r() is not None for r in alive) <= 2

    estimate_stabilization(stream(), S.settings_dict("phase-cross-corr", "xyz", "previous"), S.PIXEL)


@pytest.mark.parametrize("method,kind", [("focus-finding", "xy"), ("phase-cross-corr", "z")])
def test_invalid_pairs_are_refused(method, kind):
    with pytest.raises(ValueError):
        EstimateStabilizationSettings(**S.settings_dict(method, kind))


def test_missing_focus_takes_the_previous_index(volumes, monkeypatch):
    import shrimpy_amd.focus as F

    assert fill_missing([None, 5, None, 7, None]) == [5, 5, 5, 7, 7]
    assert fill_missing([None, 5, None, 7, None]) == R.fill_forward([None, 5, None, 7, None])
    with pytest.raises(ValueError):
        fill_missing([None, None])
    answers = iter([6, None, 3, None])
    monkeypatch.setattr(F, "focus_from_transverse_band", lambda *a, **k: next(answers))
    got = _shifts(estimate_stabilization(volumes, S.settings_dict("focus-finding", "z"), S.PIXEL))
    assert got == [(0, 0, 0), (0, 0, 0), (-3, 0, 0), (-3, 0, 0)]
    monkeypatch.setattr(F, "focus_from_transverse_band", lambda *a, **k: None)
    with pytest.raises(ValueError):
        estimate_stabilization(volumes, S.settings_dict("focus-finding", "z"), S.PIXEL)


def test_apply_is_an_exact_shift(volumes):
    m = np.eye(4)
    m[:3, 3] = DRIFT[1]
    out = apply_stabilization(torch.from_numpy(volumes[1]), m)
    assert np.array_equal(out.numpy(), S.shifted_back(volumes[1], DRIFT[1]))


def test_yaml_round_trips(tmp_path):
    est = EstimateStabilizationSettings(**S.settings_dict("focus-finding", "xyz", "previous"))
    est.to_yaml(tmp_path / "e.yml")
    assert EstimateStabilizationSettings.from_yaml(tmp_path / "e.yml") == est
    assert set(yaml.safe_load((tmp_path / "e.yml").read_text())) == {
        "stabilization_estimation_channel", "stabilization_channels", "stabilization_type", "stabilization_method",
        "focus_finding_settings", "phase_cross_corr_settings"}
    mats = [np.eye(4).tolist() for _ in range(3)]
    mats[1][0][3] = 2.0
    doc = dict(stabilization_estimation_channel="BF", stabilization_type="z", stabilization_channels=["BF"],
               affine_transform_zyx_list=mats)
    stab = StabilizationSettings(**doc)
    assert stab.time_indices == "all"
    stab.to_yaml(tmp_path / "s.yml")
    assert StabilizationSettings.from_yaml(tmp_path / "s.yml") == stab
    bad = [np.eye(4).tolist()]
    bad[0][3] = [0, 0, 1, 1]
    with pytest.raises(ValueError, match="last row"):
        StabilizationSettings(**dict(doc, affine_transform_zyx_list=bad))
    with pytest.raises(ValueError, match="4x4"):
        StabilizationSettings(**dict(doc, affine_transform_zyx_list=[np.eye(3).tolist()]))
    with pytest.raises(ValueError):
        StabilizationSettings(**dict(doc, unknown_field=1))


def test_cli_round_trip(tmp_path):
    S.check_round_trip(*S.run_cli_round_trip(tmp_path))


def test_cli_focus_finding_and_single_file(tmp_path):
    from click.testing import CliRunner

    import shrimpy_amd.cli as cli

    from shrimpy_amd.io.omezarr import open_ome_zarr

    data = S.make_store(tmp_path / "series.zarr")
    cfg = tmp_path / "estimate.yml"
    cfg.write_text(yaml.safe_dump(S.settings_dict("focus-finding", "z")))
    runner = CliRunner()
    res = runner.invoke(cli.cli, ["estimate-stabilization", "-i", str(tmp_path / "series.zarr"), "-c", str(cfg), "-o",
                                  str(tmp_path / "stab"), "-p", "0/1/000"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert [f.name for f in (tmp_path / "stab").iterdir()] == ["0_1_000.yml"]
    # one file applies to every position
    res = runner.invoke(cli.cli, ["stabilize", "-i", str(tmp_path / "series.zarr"), "-c", str(tmp_path / "stab" / "0_1_000.yml"),
                                  "-o", str(tmp_path / "out.zarr"), "--compression", "none"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    dz = [d[0] for d in S.DRIFTS["0/1/000"]]
    with open_ome_zarr(tmp_path / "out.zarr", layout="auto", mode="r", prefer_iohub=False) as plate:
        for key, pos in plate.positions():
            for t in range(4):
                want = S.shifted_back(data[key][t, 0].astype(np.float32), (dz[t], 0, 0))
                assert np.array_equal(np.asarray(pos["0"].read_volume(t, 0)), want)


def test_cli_wrong_length_fails_before_any_output(tmp_path):
    from click.testing import CliRunner

    import shrimpy_amd.cli as cli

    S.make_store(tmp_path / "series.zarr")
    doc = dict(stabilization_estimation_channel="BF", stabilization_type="z", stabilization_channels=["BF"],
               affine_transform_zyx_list=[np.eye(4).tolist()] * 3)
    (tmp_path / "short.yml").write_text(yaml.safe_dump(doc))
    res = CliRunner().invoke(cli.cli, ["stabilize", "-i", str(tmp_path / "series.zarr"), "-c", str(tmp_path / "short.yml"),
                                       "-o", str(tmp_path / "out.zarr")])
    assert res.exit_code != 0 and "T = 4" in res.output
    assert not (tmp_path / "out.zarr").exists()
    # a directory without the position's file
    (tmp_path / "empty").mkdir()
    res = CliRunner().invoke(cli.cli, ["stabilize", "-i", str(tmp_path / "series.zarr"), "-c", str(tmp_path / "empty"),
                                       "-o", str(tmp_path / "out.zarr")])
    assert res.exit_code != 0 and not (tmp_path / "out.zarr").exists()


def test_run_store_asks_a_step_for_its_unit_callable(tmp_path):
    """``for_unit`` is additive: a step without it is called as before (tests/test_io_cli.py covers the commands)."""
    from shrimpy_amd.cli import run_store
    from shrimpy_amd.io.omezarr import open_ome_zarr
    from shrimpy_amd.settings import ReconstructSettings

    data = S.make_store(tmp_path / "series.zarr")
    seen = []

    class PerUnit:
        def __init__(self, raw_shape, _settings, device):
            self.output_shape = tuple(raw_shape)

        def for_unit(self, unit):
            seen.append((unit.position, unit.t, unit.c))
            return lambda raw: torch.as_tensor(raw).to(torch.float32) + unit.t

    class Plain:
        def __init__(self, raw_shape, _settings, device):
            self.output_shape = tuple(raw_shape)

        def __call__(self, raw):
            return torch.as_tensor(raw).to(torch.float32) + 0.5

    for name, factory, add in (("a", PerUnit, None), ("b", Plain, 0.5)):
        run_store(tmp_path / "series.zarr", tmp_path / f"{name}.zarr", ReconstructSettings(), reconstructor_factory=factory,
                  compression="none")
        with open_ome_zarr(tmp_path / f"{name}.zarr", layout="auto", mode="r", prefer_iohub=False) as plate:
            for key, pos in plate.positions():
                for t in range(4):
                    want = data[key][t, 1].astype(np.float32) + (t if add is None else add)
                    assert np.array_equal(np.asarray(pos["0"].read_volume(t, 1)), want)
    assert len(seen) == 2 * 4 * 2
