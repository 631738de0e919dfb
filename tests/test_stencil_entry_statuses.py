"""The stencil entry points of csrc/correlate.hip answer every recorded call as they did when
tests/golden/stencil_entry_statuses.json was recorded (oracle/record_stencil_entry_statuses.py): the same negative code
where validation rejects the call, "ok" (any status >= 0: the HIP runtime's, there is no device) where it passes, and for
the pure host functions the same value and output bytes.  The rows -- a baseline per entry, one broken condition each,
seeded draws from the fuzzer's pools -- are rebuilt from the recorder's tables, the fixture holds the answers only."""

import json

import pytest
import torch

from oracle import record_stencil_entry_statuses as rec

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="with a device a call that passes validation would launch on host pointers")


@pytest.fixture(scope="module")
def measured():
    return rec.measure(rec.Caller())


@pytest.fixture(scope="module")
def golden():
    data = json.loads(rec.FIXTURE.read_text())
    assert (data["seed"], data["draws"]) == (rec.SEED, rec.DRAWS)
    return data["entries"]


def test_every_entry_is_recorded(golden):
    assert sorted(golden) == sorted(rec.ENTRIES)
    for name, entry in golden.items():
        assert len(entry["rows"]) == 1 + len(rec.BREAKS[name])
        assert len(entry["draws"]) == (rec.DRAWS if rec.ENTRIES[name] else 0)


@pytest.mark.parametrize("name", sorted(rec.ENTRIES))
def test_statuses_match_the_record(name, measured, golden):
    rows = [(i, got, want) for i, (got, want) in enumerate(zip(measured[name]["rows"], golden[name]["rows"])) if got != want]
    assert not rows, f"{name}: (row, status, recorded) {rows}"
    draws = [(i, got, want) for i, (got, want) in enumerate(zip(measured[name]["draws"], golden[name]["draws"])) if got != want]
    assert not draws, f"{name}: (draw, status, recorded) {draws[:10]}"
