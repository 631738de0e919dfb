"""The native calls of a Richardson-Lucy run, against the sequences recorded in ``tests/golden/rl_launch_sequences.json``
by ``oracle/record_rl_launch_sequences.py`` (which states the format and how pointers are told from sizes): entry by
entry and argument by argument, with every pointer named by the first appearance of its allocation in the run.  That pins
which buffer an iteration reads and writes, the rotation order of the volumes, the row of the scalars each launch gets,
the launch that writes the dense output, and that a plain run is one call on the kinds that take a count -- for the eight
plan kinds and the two host routes; plain, ``stats``, ``tol``, RL-TV and accelerated runs, the last two with and without
``tol``; from y (dense and padded), from ``x0`` and from an ``x0`` that is also ``out``.

Not covered: ``torch`` copies between volumes do not pass through ``_lib.call``.  Their effect is pinned bit for bit by
the "equals chaining plain iterations" tests of ``tests/test_rl_tv_gpu.py`` and ``tests/test_rl_accel_gpu.py``.
"""
import pytest

from oracle import record_rl_launch_sequences as rec

GOLDEN = rec.load()


def _replay(runs, recorded):
    seen = set()
    for name, run in runs:
        want, got = GOLDEN[name], rec.record(run)
        first = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
        assert got == want, (f"{name}: {len(got)} calls against {len(want)} recorded; the first difference is call {first}: "
                             f"{got[first:first + 1]} against {want[first:first + 1]}")
        seen.add(name)
    assert seen == recorded


def test_the_host_routes_issue_the_recorded_calls():
    _replay(rec.host_runs(), {k for k in GOLDEN if k.startswith("host ")})


@pytest.mark.gpu
def test_every_plan_kind_issues_the_recorded_calls(device):
    _replay(rec.device_runs(device), {k for k in GOLDEN if not k.startswith("host ")})
