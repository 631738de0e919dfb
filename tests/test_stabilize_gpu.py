"""Time-lapse stabilization on the device: the series and the command-line round trip of ``test_stabilize_host.py`` with
the volumes on ``cuda:0``; matrices and stabilized volumes must equal the host run's (an integer translation is exact on
both)."""

import numpy as np
import pytest
import torch

from shrimpy_amd.stabilize import apply_stabilization, estimate_stabilization
from tests import stabilize_ref as S

pytestmark = pytest.mark.gpu

DRIFT = S.DRIFTS["0/0/000"]
COMBOS = [("focus-finding", "z", "first"), ("focus-finding", "xyz", "first"), ("phase-cross-corr", "xyz", "first"),
          ("phase-cross-corr", "xyz", "previous"), ("phase-cross-corr", "xy", "first")]


@pytest.fixture(scope="module")
def volumes():
    return S.series(DRIFT)


@pytest.mark.parametrize("method,kind,t_reference", COMBOS)
def test_series_matches_the_host_run(volumes, method, kind, t_reference):
    s = S.settings_dict(method, kind, t_reference)
    host = estimate_stabilization((torch.from_numpy(v) for v in volumes), s, S.PIXEL)
    dev = estimate_stabilization((torch.as_tensor(v, device="cuda:0") for v in volumes), s, S.PIXEL)
    assert all(np.array_equal(a, b) for a, b in zip(host, dev))
    want = [(d[0] if "z" in kind else 0, d[1] if "xy" in kind else 0, d[2] if "xy" in kind else 0) for d in DRIFT]
    assert [tuple(int(v) for v in m[:3, 3]) for m in dev] == want
    for v, m in zip(volumes, dev):
        a = apply_stabilization(torch.from_numpy(v), m).numpy()
        b = apply_stabilization(torch.as_tensor(v, device="cuda:0"), m)
        assert b.device.type == "cuda" and np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
        assert np.array_equal(a, S.shifted_back(v, m[:3, 3]))


def test_cli_round_trip_on_the_device(tmp_path):
    S.check_round_trip(*S.run_cli_round_trip(tmp_path))
