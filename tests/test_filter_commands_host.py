"""``stabilize``, ``subtract-background``, ``despeckle`` and ``enhance`` hand ``run_store`` what they always did: the plan and
the ``fingerprint_extra`` document the ``--resume`` fingerprint is hashed from, the position selection and the command line's
keywords, and their ``-h`` texts -- recorded by ``oracle/record_filter_command_calls.py`` (which names the invocations) on
the commit whose calls are kept, replayed here.  The step factory handed over filters when it is built with the plan and
copies when it is built with ``registration=None``: the named step is the library call at the recorded parameters, bit for
bit, the other returns the input's values as float32.
"""

import json

import numpy as np
import pytest
import torch

from oracle import record_filter_command_calls as rec
from shrimpy_amd import hessian, morphology, rank
from shrimpy_amd.pipeline import Unit
from shrimpy_amd.stabilize import apply_stabilization
from tests import test_label_host as LH

SHAPE = (12, 40, 48)
WANT = json.loads(rec.FIXTURE.read_text())


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    import shrimpy_amd.cli as cli

    return rec.record(cli, tmp_path_factory.mktemp("filter_commands"))


def test_the_fixture_holds_every_run_with_and_without_a_position():
    assert sorted(WANT["help"]) == sorted(rec.COMMANDS)
    assert sorted(WANT["calls"]) == sorted(f"{name}{p}" for name in ("stabilize", *rec.SETTINGS) for p in ("", " -p"))
    for name, call in WANT["calls"].items():
        assert call["positions"] == ([rec.POSITION] if name.endswith(" -p") else [])


@pytest.mark.parametrize("name", sorted(WANT["calls"]))
def test_run_store_is_called_as_recorded(replay, name):
    assert replay[0]["calls"][name] == WANT["calls"][name]


@pytest.mark.parametrize("command", rec.COMMANDS)
def test_help_is_as_recorded(replay, command):
    assert replay[0]["help"][command] == WANT["help"][command]


def _library_call(name, extra, key, t):
    """The direct call of the run ``name`` for position ``key`` and timepoint ``t``, at the recorded parameters."""
    if name == "stabilize":
        matrix = np.asarray(extra["stabilize"][key]["affine_transform_zyx_list"][t], dtype=np.float64)
        return lambda v: apply_stabilization(v, matrix)
    if name == "subtract-background":
        return lambda v: morphology.white_tophat(v, tuple(extra["subtract_background"]["half_widths"][key]))
    if name == "despeckle half_widths":
        return lambda v: rank.remove_outliers(v, tuple(extra["despeckle"]["half_widths"][key]), 50.0, "bright")
    if name == "despeckle percentile":
        return lambda v: rank.percentile_filter(v, 25.0, tuple(extra["despeckle"]["half_widths"][key]))
    sigmas, sampling = extra["enhance"]["scales"][key]
    return lambda v: hessian.enhance(v, "blob", sigmas, tuple(sampling), False)


@pytest.mark.parametrize("name", ["stabilize", *rec.SETTINGS])
def test_the_factory_filters_the_named_channels_and_copies_the_others(replay, name):
    factory, plan = replay[1][name]
    extra = WANT["calls"][name]["fingerprint_extra"]
    cpu = torch.device("cpu")
    named, other = factory(SHAPE, plan, cpu), factory(SHAPE, plan.model_copy(update={"registration": None}), cpu)
    assert tuple(named.output_shape) == SHAPE and tuple(other.output_shape) == SHAPE
    raw = torch.from_numpy(LH.blob_volume(7, SHAPE).astype(np.int16))
    vol = raw.to(torch.float32)
    results = []
    for key in LH.TRANSLATION:
        for t in range(2):
            unit = Unit(key, t, 1)
            got, want = named.for_unit(unit)(raw), _library_call(name, extra, key, t)(vol)
            assert got.dtype == torch.float32 and got.shape == vol.shape and torch.equal(got, want), (key, t)
            copied = other.for_unit(unit)(raw)
            assert copied.dtype == torch.float32 and copied.is_contiguous() and torch.equal(copied, vol)
            results.append(got)
    assert not torch.equal(results[1], vol), "the filter does something"
    if name == "stabilize":
        assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[3]), "one matrix per (position, t)"
