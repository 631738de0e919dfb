"""Per-bead Gaussian fits and the Fourier-shifted PSF average on the MI355X: the kernels of ``csrc/psf_fit.hip`` through the
checks of ``tests/test_psf_fit_host.py`` -- the fit against the NumPy / float64 restatement ``tests/psf_fit_ref.py`` within
the bound measured from the restatement alone, the shifted average within its float64 bound and equal to the host twin's
bit for bit, what sub-voxel alignment buys, and the ``characterize-psf`` command on the device.  PARITY UNPINNED, as there.
"""
import numpy as np
import pytest

from shrimpy_amd import _lib
from tests import test_psf_fit_host as h

pytestmark = pytest.mark.gpu


def test_kernel_fit_against_the_restatement(device):
    on_device = h.hold_fit(device)
    again = h.hold_fit(device)
    for label in on_device:                                 # fixed butterflies, no atomics: the same bits every run
        assert np.array_equal(on_device[label][0], again[label][0], equal_nan=True), label


def test_kernel_outputs_stay_inside_their_buffers(device):
    h.hold_guards(device)


def test_kernel_shifted_average_has_the_twins_bits_and_holds_the_float64_bound(device):
    _lib.call("lsr_set_host_threads", 4)
    on_host, on_device = h.hold_shifted(h.CPU), h.hold_shifted(device)
    for label in on_host:
        assert np.array_equal(on_host[label][0], on_device[label][0]), label                       # the PSF: the same bits
        assert np.array_equal(on_host[label][1], on_device[label][1], equal_nan=True), label       # B and S per bead


def test_zero_offsets_give_the_bits_of_average_psf_on_the_device(device):
    h.hold_zero_offsets(device)


def test_subvoxel_alignment_recovers_the_true_widths_on_the_device(device):
    voxel, sub = h.hold_point(device)
    twin_voxel, twin_sub = h.hold_point(h.CPU)
    assert np.array_equal(voxel.psf.cpu().numpy(), twin_voxel.psf.numpy())
    # the shifted average takes the fitted offsets, which agree to the fit's bound only: an offset moved by 1e-9 voxel moves
    # a shifted sample by less than 1e-7 of the peak (|dD_N/dt| <= pi, three axes, 37 taps), then one float32 rounding
    assert np.allclose(sub.fit.offset_zyx, twin_sub.fit.offset_zyx, rtol=0, atol=1e-9, equal_nan=True)
    peak = float(twin_sub.psf.max())
    assert np.allclose(sub.psf.cpu().numpy(), twin_sub.psf.numpy(), rtol=0, atol=(1e-7 + 2.0 ** -23) * peak)


def test_cli_round_trip_on_the_device(tmp_path, device):
    import shrimpy_amd.cli as cli

    h.round_trip(tmp_path, cli, device)
