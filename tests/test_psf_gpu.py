"""Bead detection and PSF averaging on the MI355X: the kernels of ``csrc/peaks.hip`` against the NumPy / float64
restatement ``tests/psf_ref.py`` and against their host twins (the same peak lists, the same bits of the PSF), the
recovery of a known PSF and the ``characterize-psf`` command on the device.  The cases are those of
``tests/test_psf_host.py`` plus two 64 x 512 x 600 volumes (more than one workgroup per CU, every block boundary of the
marching passes).  PARITY UNPINNED, as there.

The smoothing (``lsr_box_smooth_f32``: float64 sums, one rounding) is held to 2 units of 2^-24 relative of scipy in float64
here as on the host, and to the twin's bits; the 64 x 512 x 600 volume is where three chained float32 blur passes, the
first implementation, measured 3.18 units.
"""
import numpy as np
import pytest
import torch

from shrimpy_amd import _lib, psf
from tests import psf_ref as r
from tests import test_psf_host as h

pytestmark = pytest.mark.gpu


def test_kernel_detection_equals_the_restatement_exactly(device):
    counts = h.hold_detection(device, big=True)
    assert counts["64 x 512 x 600"] > 20 and counts["64 x 512 x 600, ties"] > 100


def test_kernel_and_twin_find_the_same_peaks(device):
    for label, v, b, md, thr, *_ in h.detection_cases():
        s = psf.smooth(h._t(v), b)
        on_host = psf.local_maxima(s, md, thr)
        on_device = psf.local_maxima(s.to(device), md, thr)
        ka, kb = np.argsort(on_host[0]), np.argsort(on_device[0])
        assert np.array_equal(on_host[0][ka], on_device[0][kb]), label
        assert np.array_equal(on_host[1][ka], on_device[1][kb]), label
        assert np.array_equal(psf.smooth(h._t(v, device), b).cpu().numpy(), s.numpy(), equal_nan=True), label


def test_kernel_smoothing_against_scipy_in_float64(device):
    assert h.hold_smoothing(device, big=True) <= 1.0 + 1e-9


def test_candidate_overflow_is_a_value_error_and_writes_nothing_past_the_buffer(device):
    vol = h._t(h.noisy((16, 30, 44), 6), device)
    n = len(psf.detect_peaks(vol, min_distance=1, threshold_abs=0.0)[0])
    with pytest.raises(ValueError, match="threshold_abs"):
        psf.detect_peaks(vol, min_distance=1, threshold_abs=0.0, capacity=8)
    # the raw entry: the buffers sit inside guarded allocations, the counter runs past the capacity, the guards survive
    s = psf.smooth(vol, 3)
    index = torch.full((8 + 64,), -7, dtype=torch.int64, device=device)
    value = torch.full((8 + 64,), -7.0, dtype=torch.float32, device=device)
    count = torch.zeros(1, dtype=torch.int64, device=device)
    scratch = torch.empty(2 * s.numel(), dtype=torch.float32, device=device)
    import ctypes

    _lib.call("lsr_local_max_candidates_f32", s.data_ptr(), *s.shape, 1, 1, 1, ctypes.c_float(0.0), index.data_ptr(),
              value.data_ptr(), 8, count.data_ptr(), scratch.data_ptr(), _lib.stream_ptr(device))
    assert int(count.item()) == n > 8
    assert bool((index[8:] == -7).all()) and bool((value[8:] == -7.0).all())
    assert bool((index[:8] >= 0).all())


def test_kernel_average_has_the_twins_bits_and_holds_the_float64_bound(device):
    _lib.call("lsr_set_host_threads", 4)
    on_host, on_device = h.hold_average(h.CPU), h.hold_average(device)
    for label in on_host:
        assert np.array_equal(on_host[label][0], on_device[label][0]), label      # the PSF: the same bits
        assert np.array_equal(on_host[label][1], on_device[label][1]), label      # B and S per bead: the same bits


def test_a_bead_without_flux_is_skipped_on_the_device(device):
    v = np.full((20, 20, 20), 100.0, dtype=np.float32)
    v[10, 10, 10] = 500.0
    v[5, 5, 5] = 20.0
    got, skipped, stats = psf.average_psf(h._t(v, device), [[10, 10, 10], [5, 5, 5], [14, 6, 6]], (5, 5, 5), return_stats=True)
    assert list(skipped) == [1, 2] and np.array_equal(stats, [[100.0, 400.0], [100.0, -80.0], [100.0, 0.0]])
    assert float(got[2, 2, 2]) == 1.0 and float(got.abs().sum()) == 1.0


def test_a_known_psf_is_recovered_by_the_kernels(device):
    res = h.hold_recovery(device)
    twin = h.hold_recovery(h.CPU)
    for a, b in zip(res, twin):
        assert np.array_equal(a.peaks, b.peaks) and np.array_equal(a.isolated, b.isolated)
        assert np.array_equal(a.psf.cpu().numpy(), b.psf.numpy())
        assert np.array_equal(a.fwhm_vox_zyx, b.fwhm_vox_zyx, equal_nan=True)


def test_cli_round_trip_on_the_device(tmp_path, device):
    import shrimpy_amd.cli as cli

    h.round_trip(tmp_path, cli, device)
