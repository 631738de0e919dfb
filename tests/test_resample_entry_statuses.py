"""The affine resampler's entry points (csrc/affine.hip and the twin in csrc/host_twins.hip) answer every recorded call
as they did when tests/golden/resample_entry_statuses.json was recorded (oracle/record_resample_entry_statuses.py): the
same negative code where validation rejects the call, "ok" where it passes, and for the pure host functions -- the three
path queries, the box shape, the twin -- the same value and output bytes.  The rows are rebuilt from the recorder's
tables, the fixture holds the answers only."""

import json

import pytest
import torch

from oracle import record_resample_entry_statuses as rec
from oracle import record_stencil_entry_statuses as base

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="with a device a call that passes validation would launch on host pointers")


@pytest.fixture(scope="module")
def measured():
    return rec.measure(rec.Caller())


@pytest.fixture(scope="module")
def golden():
    data = json.loads(rec.FIXTURE.read_text())
    assert (data["seed"], data["draws"]) == (base.SEED, base.DRAWS)
    return data["entries"]


def test_every_entry_is_recorded(golden):
    assert sorted(golden) == sorted(rec.ENTRIES)
    for name, entry in golden.items():
        assert len(entry["rows"]) == 1 + len(rec.BREAKS[name])
        assert len(entry["draws"]) == base.DRAWS


def test_the_twin_resamples_at_most_6_x_10_x_12(golden):
    spec = rec.ENTRIES["lsr_affine_f32_cpu"]
    at = [i for i, (_, kind, _) in enumerate(spec) if kind == "s"]
    assert [spec[i][0] for i in at] == ["Zi", "Yi", "Xi", "Zo", "Yo", "Xo"]
    for (row, _), got in zip(base.rows_of("lsr_affine_f32_cpu", rec.TABLES), golden["lsr_affine_f32_cpu"]["rows"]):
        if (got[0] if isinstance(got, list) else got) == 0:    # the rows that resample
            assert all(row[i] <= most for i, most in zip(at, (6, 10, 12) * 2)), row


@pytest.mark.parametrize("name", sorted(rec.ENTRIES))
def test_statuses_match_the_record(name, measured, golden):
    rows = [(i, got, want) for i, (got, want) in enumerate(zip(measured[name]["rows"], golden[name]["rows"])) if got != want]
    assert not rows, f"{name}: (row, status, recorded) {rows}"
    draws = [(i, got, want) for i, (got, want) in enumerate(zip(measured[name]["draws"], golden[name]["draws"])) if got != want]
    assert not draws, f"{name}: (draw, status, recorded) {draws[:10]}"
