"""The ``colocalize`` command on the CPU, end to end through the host twins: a plate of two positions, two timepoints and three
channels of (6, 12, 20) as a uint16 store and as a float32 store, labelled by ``run_segment``.  The per-object table equals
``coefficients`` of numpy-built records, the summary's whole-volume Pearson equals scipy's, with a label store and without,
with fixed thresholds and with Costes'; every refusal comes before the output directory exists."""

import math

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from shrimpy_amd import colocalize as K
from tests import coloc_ref as R
from tests import test_measure_cli_host as M

KEYS, SHAPE, T = M.KEYS, M.SHAPE, 2
CHANNELS = ("A", "B", "C")


def scene(position: int, t: int):
    """Channel A: two bright boxes on a dim noise floor (``test_measure_cli_host.scene``); channel B: 0.6 A and noise, so that it
    follows A; channel C: noise alone."""
    a, noise = M.scene(position, t)
    rng = np.random.default_rng(7 + 10 * position + t)
    b = np.rint(0.6 * a + rng.normal(30.0, 3.0, SHAPE)).astype(np.uint16)
    return a, b, noise


def as_float(u16):
    return (u16.astype(np.float32) * np.float32(0.37) + np.float32(1.25)).astype(np.float32)


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    """``(cli, directory)``: u16.zarr, f32.zarr and seg.zarr (``run_segment`` of channel A)."""
    import shrimpy_amd.cli as cli

    patch = pytest.MonkeyPatch()
    patch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    d = tmp_path_factory.mktemp("colocalize")
    M.write_store(d / "u16.zarr", np.uint16, lambda p, t, c: scene(p, t)[c], channels=CHANNELS, timepoints=T)
    M.write_store(d / "f32.zarr", np.float32, lambda p, t, c: as_float(scene(p, t)[c]), channels=CHANNELS, timepoints=T)
    cli.run_segment(d / "u16.zarr", M.config(d, "segment", channel_name="A", threshold=100.0), d / "seg.zarr")
    yield cli, d
    patch.undo()


def colocalize(cli, d, inputs, out, labels=None, extra=(), **settings):
    cfg = M.config(d, f"colocalize_{out}", **settings)
    args = ["colocalize", "-i", str(d / inputs), "-c", str(cfg), "-o", str(d / out), *extra]
    if labels is not None:
        args += ["-l", str(d / labels)]
    return CliRunner().invoke(cli.cli, args), d / out


def numpy_record(a, b, inside, thresholds):
    """One record of the table over the voxels ``inside``, from numpy (``coloc_ref``'s restatement on a mask)."""
    labels = inside.astype(np.int32)
    if a.dtype == np.uint16:
        return R.pair_u16(labels, a, b, 1, *thresholds)
    ref = R.pair_f32(labels, a, b, 1, *thresholds)
    out = np.zeros((1,), K.COLOC_DTYPE_F32)
    for j, f in enumerate(R.COUNTS):
        out[f] = ref["counts"][0, j]
    for j, f in enumerate(R.SUMS):
        out[f] = ref["sums"][0, j]
    return out


def assert_values(row, prefix, record, rel, cli):
    want = K.coefficients(record)
    for c in K.COEFFICIENTS:
        got = float(row[prefix + c])
        if math.isnan(want[c][0]):
            assert math.isnan(got), prefix + c
        else:
            assert got == pytest.approx(float(want[c][0]), rel=rel, abs=1e-15), prefix + c
    for c in cli.COLOCALIZE_COUNT_COLUMNS:
        assert int(row[prefix + c]) == int(record[c][0]), prefix + c


@pytest.mark.parametrize("store,convert,rel", [("u16.zarr", lambda v: v, 0.0), ("f32.zarr", as_float, 1e-9)], ids=["u16", "f32"])
def test_the_tables_equal_the_coefficients_of_numpy_records(plate, store, convert, rel):
    """With a label store: one row per (t, label) with voxels, every column of every pair from a numpy-built record -- exactly
    for uint16 data (integer sums), within 1e-9 for float32 data (sums of a few hundred terms, far inside); the summary has the
    whole volume and the labelled region, and its whole-volume Pearson is scipy's."""
    from scipy import stats

    cli, d = plate
    thresholds = [40.0, 50.0]
    r, out = colocalize(cli, d, store, "c_" + store[:3], labels="seg.zarr", pairs=[["A", "B"], ["C", "A"]],
                        label_channel_name="A_labels", thresholds=thresholds)
    assert r.exit_code == 0, r.output
    for p, key in enumerate(KEYS):
        rows = M.read_csv(out / key / "colocalization.csv")
        summary = M.read_csv(out / key / "colocalization_summary.csv")
        header = list(rows[0])
        assert header[:3] == ["t", "label", "volume_voxels"]
        assert header[3:] == [f"{pair}_{c}" for pair in ("A__B", "C__A") for c in cli.COLOCALIZE_PAIR_COLUMNS]
        assert list(summary[0]) == list(cli.COLOCALIZE_SUMMARY_COLUMNS) and len(summary) == T * 2 * 2
        at = 0
        for t in range(T):
            labels = M.read_volume(cli, d / "seg.zarr", key, t)
            volumes = dict(zip(CHANNELS, (convert(v) for v in scene(p, t))))
            present = [k for k in range(1, int(labels.max()) + 1) if (labels == k).any()]
            assert len(present) >= 2
            for k in present:
                row = rows[at]
                at += 1
                assert (int(row["t"]), int(row["label"]), int(row["volume_voxels"])) == (t, k, int((labels == k).sum()))
                for ca, cb in (("A", "B"), ("C", "A")):
                    assert_values(row, f"{ca}__{cb}_", numpy_record(volumes[ca], volumes[cb], labels == k, thresholds), rel, cli)
            for ca, cb in (("A", "B"), ("C", "A")):
                for region, inside in (("volume", np.ones(SHAPE, bool)), ("labelled", labels >= 1)):
                    line = [s for s in summary if (s["t"], s["channel_a"], s["channel_b"], s["region"]) == (str(t), ca, cb, region)]
                    assert len(line) == 1
                    line = line[0]
                    assert int(line["voxels"]) == int(inside.sum()) and line["thresholds_from"] == "settings"
                    assert (float(line["threshold_a"]), float(line["threshold_b"])) == tuple(thresholds)
                    assert_values(line, "", numpy_record(volumes[ca], volumes[cb], inside, thresholds), rel, cli)
                    if region == "volume":
                        theirs = stats.pearsonr(volumes[ca].ravel().astype(np.float64), volumes[cb].ravel().astype(np.float64))[0]
                        assert float(line["pearson"]) == pytest.approx(theirs, rel=1e-12 if rel == 0.0 else 1e-7)
        assert at == len(rows)
    # B follows A, C does not
    first = M.read_csv(out / KEYS[0] / "colocalization_summary.csv")[0]
    assert float(first["pearson"]) > 0.9 and first["channel_b"] == "B"


def test_without_labels_only_the_summary_is_written_and_one_position(plate):
    cli, d = plate
    r, out = colocalize(cli, d, "u16.zarr", "c_whole", extra=("-p", KEYS[1]), pairs=[["A", "B"]])
    assert r.exit_code == 0, r.output
    assert not (out / KEYS[0]).exists() and not (out / KEYS[1] / "colocalization.csv").exists()
    summary = M.read_csv(out / KEYS[1] / "colocalization_summary.csv")
    assert [(s["t"], s["region"]) for s in summary] == [("0", "volume"), ("1", "volume")]
    for t, line in enumerate(summary):
        a, b, _ = scene(1, t)
        assert (float(line["threshold_a"]), float(line["threshold_b"])) == (0.0, 0.0)
        assert_values(line, "", numpy_record(a, b, np.ones(SHAPE, bool), (0.0, 0.0)), 0.0, cli)


@pytest.mark.parametrize("region", ["volume", "labelled"])
def test_costes_thresholds_in_the_command(plate, region):
    """``thresholds: costes``: per (t, pair) the thresholds of the restatement (uint16: exactly), used for both regions; a pair
    whose covariance is not positive is marked and its threshold columns are NaN."""
    cli, d = plate
    r, out = colocalize(cli, d, "u16.zarr", "c_costes_" + region, labels="seg.zarr", pairs=[["A", "B"], ["A", "C"]],
                        label_channel_name="A_labels", thresholds="costes", costes_region=region)
    assert r.exit_code == 0, r.output
    seen = set()
    for p, key in enumerate(KEYS):
        summary = M.read_csv(out / key / "colocalization_summary.csv")
        rows = M.read_csv(out / key / "colocalization.csv")
        for line in summary:
            t = int(line["t"])
            labels = M.read_volume(cli, d / "seg.zarr", key, t)
            volumes = dict(zip(CHANNELS, scene(p, t)))
            a, b = volumes[line["channel_a"]], volumes[line["channel_b"]]
            want = R.costes(np.minimum(labels, 1), a, b, 1, region)
            inside = np.ones(SHAPE, bool) if line["region"] == "volume" else labels >= 1
            seen.add(want["status"])
            if want["status"] == "ok":
                assert line["thresholds_from"] == "costes"
                assert (float(line["threshold_a"]), float(line["threshold_b"])) == (want["ta"], want["tb"])
                assert_values(line, "", numpy_record(a, b, inside, (want["ta"], want["tb"])), 0.0, cli)
            else:
                assert line["thresholds_from"] == "costes:uncorrelated" and math.isnan(float(line["threshold_a"]))
                assert all(math.isnan(float(line[c])) for c in cli.COLOCALIZE_THRESHOLD_COLUMNS)
                assert all(int(line[c]) == 0 for c in cli.COLOCALIZE_COUNT_COLUMNS)
                record = numpy_record(a, b, inside, (0.0, 0.0))
                assert float(line["pearson"]) == pytest.approx(float(K.coefficients(record)["pearson"][0]), rel=1e-15)
        assert len(rows) >= 2 * T and all(float(row["A__B_pearson"]) > 0.5 for row in rows)
    assert "ok" in seen


def test_refusals_come_before_the_output_directory(plate):
    cli, d = plate
    ok = dict(pairs=[["A", "B"]], label_channel_name="A_labels")
    r, out = colocalize(cli, d, "u16.zarr", "r_position", labels="seg.zarr", extra=("-p", "Z/9/9"), **ok)
    M.refused(r, out, "positions ['Z/9/9'] not found")
    r, out = colocalize(cli, d, "u16.zarr", "r_channel", pairs=[["A", "RFP"]])
    M.refused(r, out, "channels ['RFP'] not in position A/1/0")
    r, out = colocalize(cli, d, "u16.zarr", "r_label_channel", labels="seg.zarr", pairs=[["A", "B"]], label_channel_name="nuclei")
    M.refused(r, out, "label_channel_name 'nuclei' not in position A/1/0")
    r, out = colocalize(cli, d, "u16.zarr", "r_no_label_channel", labels="seg.zarr", pairs=[["A", "B"]])
    M.refused(r, out, "label_channel_name is needed")
    r, out = colocalize(cli, d, "u16.zarr", "r_region", pairs=[["A", "B"]], thresholds="costes", costes_region="labelled")
    M.refused(r, out, "costes_region 'labelled' needs a label store")
    r, out = colocalize(cli, d, "u16.zarr", "r_float_labels", labels="f32.zarr", pairs=[["A", "B"]], label_channel_name="A")
    M.refused(r, out, "position A/1/0: label data type float32")
    r, out = colocalize(cli, d, "seg.zarr", "r_int_values", pairs=[["A_labels", "A_labels2"]])
    M.refused(r, out, "not in position A/1/0")
    for bad, word in ((dict(pairs=[]), "at least one pair"), (dict(pairs=[["A", "A"]]), "two different channel names"),
                      (dict(pairs=[["A", "B"], ["A", "B"]]), "named once"), (dict(pairs=[["A", "B"]], thresholds=[1.0]), "thresholds"),
                      (dict(pairs=[["A", "B"]], thresholds="otsu"), "thresholds"),
                      (dict(pairs=[["A", "B"]], costes_region="object"), "costes_region"),
                      (dict(pairs=[["A", "B"]], radius=1.0), "radius")):
        r, out = colocalize(cli, d, "u16.zarr", "r_settings", **bad)
        M.refused(r, out, word)
    # integer data of another type than uint16
    M.write_store(d / "i32.zarr", np.int32, lambda p, t, c: np.ones(SHAPE), channels=("A", "B"), timepoints=T)
    r, out = colocalize(cli, d, "i32.zarr", "r_int32", pairs=[["A", "B"]])
    M.refused(r, out, "position A/1/0: data type int32")
    # a label store that lacks the second position, or whose timepoints or scale differ
    M.write_store(d / "one.zarr", np.int32, lambda p, t, c: np.ones(SHAPE), channels=("A_labels",), keys=KEYS[:1], timepoints=T)
    r, out = colocalize(cli, d, "u16.zarr", "r_missing", labels="one.zarr", **ok)
    M.refused(r, out, "position B/2/0 not found in")
    M.write_store(d / "long.zarr", np.int32, lambda p, t, c: np.ones(SHAPE), channels=("A_labels",), timepoints=3)
    r, out = colocalize(cli, d, "u16.zarr", "r_t", labels="long.zarr", **ok)
    M.refused(r, out, "position A/1/0: the labels are (T, Z, Y, X) = (3, 6, 12, 20), the channels (2, 6, 12, 20)")
    M.write_store(d / "coarse.zarr", np.int32, lambda p, t, c: np.ones(SHAPE), channels=("A_labels",), timepoints=T,
                  scale=(1.0, 1.0, 0.5, 0.25, 0.5))
    r, out = colocalize(cli, d, "u16.zarr", "r_scale", labels="coarse.zarr", **ok)
    M.refused(r, out, "position A/1/0: the labels' (z, y, x) scale is")
    M.write_store(d / "big.zarr", np.int64, lambda p, t, c: np.full(SHAPE, 2 ** 31 if (p, t) == (1, 1) else 7), channels=("A_labels",),
                  timepoints=T)
    r, out = colocalize(cli, d, "u16.zarr", "r_int32_labels", labels="big.zarr", **ok)
    M.refused(r, out, "position B/2/0, t = 1: a label does not fit int32")
    # an output directory that exists, even an empty one
    (d / "taken").mkdir()
    r, out = colocalize(cli, d, "u16.zarr", "taken", pairs=[["A", "B"]])
    assert r.exit_code != 0 and "exists (never overwritten)" in r.output and not any((d / "taken").iterdir())
