"""Per-bead Gaussian fits and the Fourier-shifted PSF average on the CPU: the host twins (``lsr_bead_fit_f32_cpu``,
``lsr_psf_accumulate_shifted_f32_cpu``) against the NumPy / float64 restatement ``tests/psf_fit_ref.py``, the restatement
against the truth of a synthetic scene, what sub-voxel alignment buys (the point of the feature), the unchanged defaults
and the ``characterize-psf`` command.  ``tests/test_psf_fit_gpu.py`` runs the same ``hold_*`` checks on the device.
PARITY UNPINNED: biahub's ``_characterize_psf`` is not vendored; the rule is this package's own.

Bounds.  The fit: statuses equal the restatement's; every parameter of a status-0 bead within ``fit_tolerance`` -- 16 times
what reversing the order of the restatement's own sums moves a parameter, at least 1e-9 (``tests/psf_fit_ref.py`` has the
measured values).  The shifted average: ``3 (pz + py + px) 2^-53 sum|c w|`` per element of the float64 restatement plus one
float32 rounding; with every offset zero the bits of ``average_psf``.
"""
import csv
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib, psf
from shrimpy_amd.io.omezarr import open_ome_zarr
from shrimpy_amd.settings import CharacterizeSettings
from tests import psf_fit_ref as r

CPU = torch.device("cpu")
PARENT_REPORT_KEYS = ["n_peaks", "n_isolated", "n_skipped", "n_averaged", "patch_shape_zyx", "zyx_scale", "fwhm_mean_vox_zyx",
                      "fwhm_median_vox_zyx", "fwhm_mean_zyx", "fwhm_median_zyx", "psf_fwhm_vox_zyx", "psf_fwhm_zyx"]
PARENT_CSV_HEADER = ["z", "y", "x", "value", "isolated", "fwhm_z", "fwhm_y", "fwhm_x"]
FIT_CSV_HEADER = ["fit_status", "mu_z", "mu_y", "mu_x", "fit_fwhm_z", "fit_fwhm_y", "fit_fwhm_x", "fit_fwhm_p0", "fit_fwhm_p1",
                  "fit_fwhm_p2"]


def _t(a, device=CPU):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def theta_of(f):
    """A ``BeadFits`` as the kernel's (N, 12) rows."""
    w = f.precision
    return np.column_stack([f.background, f.amplitude, f.offset_zyx, w[:, 0, 0], w[:, 1, 1], w[:, 2, 2], w[:, 0, 1], w[:, 0, 2],
                            w[:, 1, 2], f.cost])


# ------------------------------------------------------------------ the cases, each with the restatement's answer (once)


@functools.lru_cache(maxsize=None)
def fit_cases():
    """``label -> (volume, peaks, patch, theta, status, evaluations, tolerance)``: scenes A and B with the restatement's fit
    and the bound measured from its forward and reversed runs."""
    a_vol, a_peaks, _, _, a_patch = r.scene_a()
    s_vol, s_peaks, s_patch = r.scene_b_small()
    l_vol, l_flat, l_nan, l_peaks, _, l_patch = r.scene_b_large()
    outside = np.array([[16, 20, 10], [2, 20, 10], [50, 20, 10]])          # fits, does not fit, not in the volume
    cases = {}
    for label, vol, peaks, patch in (("A: 10 beads, 11 x 13 x 13", a_vol, a_peaks, a_patch),
                                     ("B: 3 x 5 x 7 and a patch that does not fit", s_vol, s_peaks, s_patch),
                                     ("B: 31 x 37 x 19, the second bead 1.3 voxels off", l_vol, l_peaks, l_patch),
                                     ("B: flat", l_flat, l_peaks, l_patch),
                                     ("B: a NaN in the first patch", l_nan, l_peaks, l_patch),
                                     ("B: centres outside", l_vol, outside, l_patch)):
        theta, status, evals = r.fit(vol, peaks, patch)
        back, back_status, _ = r.fit(vol, peaks, patch, reverse=True)
        assert np.array_equal(status, back_status), label
        cases[label] = (vol, peaks, patch, theta, status, evals, r.fit_tolerance(theta, back))
    return cases


def hold_fit(device):
    """Check 2 on ``device``: statuses equal the restatement's, status-0 parameters within the measured bound; non-zero
    statuses leave NaN.  Returns ``label -> (theta, status)``."""
    out = {}
    for label, (vol, peaks, patch, theta, status, evals, tol) in fit_cases().items():
        got = psf.fit_beads(_t(vol, device), peaks, patch)
        mine = theta_of(got)
        worst = r.scaled_difference(mine, theta)
        print(f"{label}: statuses {status.tolist()}, restatement iterations {evals.tolist()}, bound {tol:.3g}, worst {worst:.3g}")
        assert np.array_equal(got.status, status), label
        assert np.isnan(mine[status != 0]).all() and np.isfinite(mine[status == 0]).all(), label
        assert worst <= tol, label
        out[label] = (mine, got.status)
    return out


def shift_cases():
    """``label, volume, peaks, offsets (a NaN row: left out), patch``"""
    a_vol, a_peaks, a_centres, _, a_patch = r.scene_a()
    yield "A: 10 beads, their true offsets", a_vol, a_peaks, a_centres - a_peaks, a_patch
    l_vol, _, _, l_peaks, _, l_patch = r.scene_b_large()
    yield "B: 31 x 37 x 19, two beads", l_vol, l_peaks, np.array([[0.3, -0.4, 0.2], [-0.999, 0.3, 0.0]]), l_patch
    s_vol, _, s_patch = r.scene_b_small()
    rng = np.random.default_rng(7)
    n = 65                                                                 # one more than a batch of the kernel
    peaks = np.stack([rng.integers(1, 8, n), rng.integers(2, 9, n), rng.integers(3, 10, n)], axis=1)
    mu = rng.uniform(-0.5, 0.5, (n, 3))
    mu[3] = np.nan                                                         # an unfit bead: NaN weights
    peaks[:3] = [[4, 5, 6], [4, 5, 6], [3, 5, 7]]
    peaks[64] = [4, 5, 5]                                                  # the bead of the second batch carries flux
    yield "B: 3 x 5 x 7, 65 beads (a batch and one), some without flux, one with NaN weights", s_vol, peaks, mu, s_patch


def hold_shifted(device):
    """Check 3 on ``device``: the bound against the float64 restatement with the same weights.  Returns ``label -> (psf,
    stats)`` for the comparison of device and twin bit for bit."""
    out = {}
    for label, vol, peaks, mu, patch in shift_cases():
        got, stats, used = psf._average_shifted(_t(vol, device), peaks, mu, patch)
        got = got.cpu().numpy()
        weights = np.concatenate([psf.shift_weights(mu[:, a], n) for a, n in enumerate(patch)], axis=1)
        want, bound, n_used = r.shifted_average(vol, peaks, patch, weights, stats[:, 0], stats[:, 1])
        assert got.dtype == np.float32 and got.shape == tuple(patch)
        assert int(used.sum()) == n_used > 0, label
        excess = np.abs(got.astype(np.float64) - want) - (bound + 2.0 ** -24 * np.abs(want))
        print(f"{label}: {n_used} of {len(peaks)} beads used, worst error {np.abs(got - want).max():.3g}, bound exceeded by "
              f"{excess.max():.3g} (<= 0 holds)")
        assert excess.max() <= 0.0, label
        out[label] = (got, stats)
    return out


def hold_zero_offsets(device):
    """Check 3, last item: with every offset zero the weights are exactly a delta and the result is ``average_psf``'s."""
    for n in (1, 3, 19, 129):
        assert np.array_equal(psf.shift_weights(np.zeros(2), n), np.tile(np.eye(n)[0], (2, 1)))
        assert not np.signbit(psf.shift_weights(np.zeros(1), n)).any()
    vol, peaks, _, _, patch = r.scene_a()
    v = _t(vol, device)
    plain, skipped = psf.average_psf(v, peaks, patch)
    moved, skipped_too = psf.average_psf_aligned(v, peaks, peaks.astype(np.float64), patch)
    assert np.array_equal(plain.cpu().numpy(), moved.cpu().numpy()) and np.array_equal(skipped, skipped_too)


def scene_a_settings(**kw):
    return CharacterizeSettings(**dict(dict(blur_kernel_size=1, min_distance=4, threshold_abs=500.0, patch_size=(11, 13, 13),
                                            exclude_border=(0, 0, 0), max_num_peaks=None), **kw))


def sigma_errors(res):
    """Relative error of the fitted principal sigmas of the average against the truth, widest first."""
    assert int(res.psf_fit.status[0]) == 0
    return np.abs(res.psf_fit.fwhm_principal[0] / r.FWHM_PER_SIGMA / np.array(r.TRUE_SIGMA) - 1.0)


def hold_point(device):
    """Check 4 on ``device``, through ``characterize_psf``."""
    vol = _t(r.scene_a()[0], device)
    voxel = psf.characterize_psf(vol, scene_a_settings(gaussian_fit=True))
    sub = psf.characterize_psf(vol, scene_a_settings(alignment="subvoxel"))
    assert voxel.alignment == "voxel" and sub.alignment == "subvoxel" and voxel.unfit is None and len(sub.unfit) == 0
    assert int(sub.isolated.sum()) == 10 == sub.n_averaged == voxel.n_averaged
    e_voxel, e_sub = sigma_errors(voxel), sigma_errors(sub)
    print(f"principal sigma errors of the average: voxel-aligned {e_voxel}, sub-voxel {e_sub}")
    assert np.all(e_sub <= 0.005)
    assert np.all(e_sub <= e_voxel / 5.0)
    assert np.all(e_voxel[1:] > 0.02)
    # the tilt comes back: the widest principal axis of the average is the true one
    assert abs(float(sub.psf_fit.principal_axes[0, 0] @ r.true_axes()[0])) > 0.9999
    return voxel, sub


# ------------------------------------------------------------------ 1. the restatement against the truth


def test_the_restatement_recovers_scene_a_and_every_case_converges_within_30_iterations():
    vol, peaks, centres, amplitudes, patch = r.scene_a()
    theta, status, evals = fit_cases()["A: 10 beads, 11 x 13 x 13"][3:6]
    assert np.all(status == 0)
    centre_error = float(np.abs(theta[:, 2:5] - (centres - peaks)).max())
    sigma = np.array([r.principal_sigmas(r.precision(t))[0] for t in theta])
    sigma_error = float(np.abs(sigma / np.array(r.TRUE_SIGMA) - 1.0).max())
    print(f"scene A: centres off by {centre_error:.3g} voxel, principal sigmas by {sigma_error:.3g} relative")
    assert centre_error <= 1e-5 and sigma_error <= 1e-5
    assert np.allclose(theta[:, 1], amplitudes, rtol=1e-6) and np.allclose(theta[:, 0], 100.0, rtol=1e-6)
    for label, case in fit_cases().items():
        assert case[5].max() <= 30, label
    assert r.HALF_MAX_MOMENT == pytest.approx(0.1888664644521538, rel=1e-12)


def test_the_cases_have_the_statuses_the_scenes_were_built_for():
    s = {label: case[4].tolist() for label, case in fit_cases().items()}
    assert s["B: 3 x 5 x 7 and a patch that does not fit"] == [0, 5]
    assert s["B: 31 x 37 x 19, the second bead 1.3 voxels off"] == [0, 3]
    assert s["B: flat"] == [4, 4]
    assert s["B: a NaN in the first patch"] == [5, 3]
    assert s["B: centres outside"] == [0, 5, 5]


# ------------------------------------------------------------------ 2. the twin's fit


def test_twin_fit_against_the_restatement():
    _lib.call("lsr_set_host_threads", 4)
    four = hold_fit(CPU)
    _lib.call("lsr_set_host_threads", 1)
    one = hold_fit(CPU)
    for label in four:                                                     # beads are fitted one by one: no thread count shows
        assert np.array_equal(four[label][0], one[label][0], equal_nan=True), label


def guarded_fit(device, vol, peaks, patch, max_iter=100):
    """The raw entry with ``fit`` and ``status`` inside guarded allocations: ``(fit, status, guards intact)``."""
    n, g = len(peaks), 32
    v = _t(vol, device)
    fit = torch.full((g + 12 * n + g,), -7.0, dtype=torch.float64, device=device)
    status = torch.full((g + n + g,), -7, dtype=torch.int32, device=device)
    centres = _t(psf._centres(np.asarray(peaks, dtype=np.int64), vol.shape), device)
    psf._call(v, "lsr_bead_fit_f32", v.data_ptr(), *vol.shape, centres.data_ptr(), n, *patch, max_iter, fit.data_ptr() + 8 * g,
              status.data_ptr() + 4 * g)
    fit, status = fit.cpu().numpy(), status.cpu().numpy()
    intact = bool((fit[:g] == -7).all() and (fit[-g:] == -7).all() and (status[:g] == -7).all() and (status[-g:] == -7).all())
    return fit[g:-g].reshape(n, 12), status[g:-g], intact


def hold_guards(device):
    vol, _, nan, peaks, _, patch = r.scene_b_large()
    for v, want in ((nan, [5, 3]), (vol, [0, 3])):
        fit, status, intact = guarded_fit(device, v, peaks, patch)
        assert intact and status.tolist() == want
        assert np.isnan(fit[status != 0]).all() and np.isfinite(fit[status == 0]).all()
    fit, status, intact = guarded_fit(device, vol, peaks, patch, max_iter=3)       # the limit: status 1, NaN
    assert intact and status.tolist() == [1, 1] and np.isnan(fit).all()
    # the shifted average: psf inside a guarded allocation, beads that contribute nothing
    t = _t(nan, device)
    mu = np.array([[0.25, -0.25, 0.5], [np.nan, 0.0, 0.0]])
    n = int(np.prod(patch))
    out = torch.full((64 + n + 64,), -7.0, dtype=torch.float32, device=device)
    stats = torch.full((4 + 4 + 4,), -7.0, dtype=torch.float64, device=device)
    weights = _t(np.concatenate([psf.shift_weights(mu[:, a], m) for a, m in enumerate(patch)], axis=1), device)
    centres = _t(psf._centres(peaks, nan.shape), device)
    scratch = None
    if device.type != "cpu":
        nbytes = ctypes.c_int64(0)
        _lib.call("lsr_psf_shift_scratch_bytes", 2, *patch, ctypes.byref(nbytes))
        scratch = torch.empty(nbytes.value // 8, dtype=torch.float64, device=device)
    psf._call(t, "lsr_psf_accumulate_shifted_f32", t.data_ptr(), *nan.shape, centres.data_ptr(), 2, *patch, stats.data_ptr() + 32,
              weights.data_ptr(), None if scratch is None else scratch.data_ptr(), out.data_ptr() + 4 * 64)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    assert (out[:64] == -7).all() and (out[-64:] == -7).all() and (stats[:4] == -7).all() and (stats[-4:] == -7).all()
    # the first bead's S is NaN (not > 0), the second has NaN weights: nothing contributes, the PSF is zeros
    assert np.isnan(stats[5]) and stats[7] > 0 and (out[64:-64] == 0).all()


def test_twin_outputs_stay_inside_their_buffers():
    hold_guards(CPU)


# ------------------------------------------------------------------ 3. the shifted average


def test_twin_shifted_average_against_float64():
    _lib.call("lsr_set_host_threads", 4)
    four = hold_shifted(CPU)
    _lib.call("lsr_set_host_threads", 1)
    one = hold_shifted(CPU)
    for label in four:
        assert np.array_equal(four[label][0], one[label][0]) and np.array_equal(four[label][1], one[label][1], equal_nan=True), label


def test_zero_offsets_give_the_bits_of_average_psf():
    hold_zero_offsets(CPU)


def test_shift_weights_are_the_dirichlet_kernel():
    for n in (1, 3, 11, 37, 129):
        for mu in (0.3, -0.45, 0.5, -0.75):        # (near |mu| = 1 the definition itself cancels: the identity below covers it)
            assert np.allclose(psf.shift_weights([mu], n)[0], r.dirichlet(mu, n), rtol=0, atol=1e-12), (n, mu)
            assert psf.shift_weights([mu], n).sum() == pytest.approx(1.0, abs=1e-12)        # a shift keeps the mean
    # moving a sampled band-limited line by mu and back by -mu is the identity
    k = np.arange(11)
    x = np.cos(2 * np.pi * k / 11) + 0.5 * np.sin(4 * np.pi * k / 11)
    for mu in (0.37, -0.999):
        there, _ = r._circulant(x, psf.shift_weights([mu], 11)[0], 0)
        back, _ = r._circulant(there, psf.shift_weights([-mu], 11)[0], 0)
        assert np.allclose(back, x, atol=1e-13)
        assert np.allclose(there, np.cos(2 * np.pi * (k + mu) / 11) + 0.5 * np.sin(4 * np.pi * (k + mu) / 11), atol=1e-13)


# ------------------------------------------------------------------ 4. the point of the feature


def test_subvoxel_alignment_recovers_the_true_widths_where_voxel_alignment_broadens_them():
    hold_point(CPU)


# ------------------------------------------------------------------ 5. defaults, arguments


def test_the_defaults_produce_what_they_produced():
    d = CharacterizeSettings()
    assert (d.gaussian_fit, d.alignment, d.fit_max_iter) == (False, "voxel", 100)
    with pytest.raises(ValueError):
        CharacterizeSettings(alignment="cubic")
    with pytest.raises(ValueError):
        CharacterizeSettings(fit_max_iter=0)
    vol = _t(r.scene_a()[0])
    res = psf.characterize_psf(vol, scene_a_settings())
    assert res.fit is None and res.psf_fit is None and res.unfit is None and res.alignment == "voxel"
    assert list(res.report()) == PARENT_REPORT_KEYS
    # the PSF recomputed through the detection and the plain average
    coords, _ = psf.detect_peaks(vol, min_distance=4, threshold_abs=500.0, blur_kernel_size=1)
    assert np.array_equal(coords.numpy(), res.peaks)
    iso = psf.isolated_mask(res.peaks, vol.shape, (11, 13, 13))
    plain, skipped = psf.average_psf(vol, res.peaks[iso], (11, 13, 13))
    assert np.array_equal(plain.numpy(), res.psf.numpy()) and len(skipped) == 0 and res.n_averaged == 10
    # with the fit on, the voxel-aligned PSF and the old entries of the report are the same
    fitted = psf.characterize_psf(vol, scene_a_settings(gaussian_fit=True))
    assert np.array_equal(fitted.psf.numpy(), res.psf.numpy())
    assert {k: fitted.report()[k] for k in PARENT_REPORT_KEYS} == res.report()
    assert set(fitted.report()) - set(PARENT_REPORT_KEYS) >= {
        "fit_fwhm_axis_median_vox_zyx", "fit_fwhm_principal_median_vox", "fit_fwhm_axis_median_zyx", "fit_fwhm_principal_median",
        "psf_fit_fwhm_axis_vox_zyx", "psf_fit_fwhm_principal_vox", "psf_fit_principal_axes", "n_unfit", "alignment"}
    assert np.array_equal(fitted.fit.status == 0, fitted.isolated) and np.all(fitted.fit.status[~fitted.isolated] == -1)


def test_arguments_are_checked():
    vol, peaks, centres, _, patch = r.scene_a()
    v = _t(vol)
    with pytest.raises(ValueError, match="within one voxel"):
        psf.average_psf_aligned(v, peaks[:2], peaks[:2] + np.array([[0.0, 1.0, 0.0], [0, 0, 0]]), patch)
    with pytest.raises(ValueError, match="within one voxel"):
        psf.average_psf_aligned(v, peaks[:2], peaks[:2] + np.array([[0.0, np.nan, 0.0], [0, 0, 0]]), patch)
    with pytest.raises(ValueError, match="does not fit"):
        psf.average_psf_aligned(v, [[2, 30, 30]], [[2.0, 30.0, 30.0]], patch)
    with pytest.raises(ValueError, match="shape of peaks"):
        psf.average_psf_aligned(v, peaks, centres[:3], patch)
    with pytest.raises(ValueError, match="odd"):
        psf.fit_beads(v, peaks, (10, 13, 13))
    with pytest.raises(ValueError, match="max_iter"):
        psf.fit_beads(v, peaks, patch, max_iter=0)
    with pytest.raises(TypeError):
        psf.fit_beads(v.double(), peaks, patch)
    # a physical scale: widths along the principal axes of W in physical units
    w = np.linalg.inv(r.true_covariance())[None]
    fwhm, axes = psf.principal_widths(w, (2.0, 1.0, 0.5))
    cov = np.diag([2.0, 1.0, 0.5]) @ r.true_covariance() @ np.diag([2.0, 1.0, 0.5])
    assert np.allclose(np.sort(fwhm[0]), r.FWHM_PER_SIGMA * np.sqrt(np.linalg.eigvalsh(cov)))
    assert np.allclose(psf.principal_widths(w)[0][0], r.FWHM_PER_SIGMA * np.array(r.TRUE_SIGMA))


def test_c_abi_error_codes_before_any_launch():
    """Check 7: every new entry refuses a null pointer, an even patch, a patch over 129, a patch over the volume, n <= 0
    and (the device entry of the shifted average) a misaligned scratch -- before anything is launched: the device entries are
    called here, without a device."""
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    null, ok = -1, 0
    e_shape, e_unsupported, e_arg = -2, _lib.E_UNSUPPORTED, -4
    for fit in (lib.lsr_bead_fit_f32, lib.lsr_bead_fit_f32_cpu):
        assert fit(None, 20, 20, 20, p, 1, 3, 3, 3, 10, p, p, None) == null
        assert fit(p, 20, 20, 20, None, 1, 3, 3, 3, 10, p, p, None) == null
        assert fit(p, 20, 20, 20, p, 1, 3, 3, 3, 10, None, p, None) == null
        assert fit(p, 20, 20, 20, p, 1, 3, 3, 3, 10, p, None, None) == null
        assert fit(p, 20, 20, 20, p, 1, 3, 4, 3, 10, p, p, None) == e_arg
        assert fit(p, 200, 200, 200, p, 1, 3, 131, 3, 10, p, p, None) == e_unsupported
        assert fit(p, 20, 20, 20, p, 1, 21, 3, 3, 10, p, p, None) == e_shape
        assert fit(p, 20, 20, 20, p, 0, 3, 3, 3, 10, p, p, None) == e_arg
        assert fit(p, 20, 20, 20, p, -1, 3, 3, 3, 10, p, p, None) == e_arg
        assert fit(p, 20, 20, 20, p, 1, 3, 3, 3, 0, p, p, None) == e_arg
        assert fit(p, 0, 20, 20, p, 1, 3, 3, 3, 10, p, p, None) == e_shape
    for shifted in (lib.lsr_psf_accumulate_shifted_f32, lib.lsr_psf_accumulate_shifted_f32_cpu):
        for k in (0, 4, 9, 10, 12):                         # vol, centres, stats, weights, psf
            args = [p, 20, 20, 20, p, 1, 3, 3, 3, p, p, p, p, None]
            args[k] = None
            assert shifted(*args) == null, k
        assert shifted(p, 20, 20, 20, p, 1, 3, 3, 2, p, p, p, p, None) == e_arg
        assert shifted(p, 200, 200, 200, p, 1, 131, 3, 3, p, p, p, p, None) == e_unsupported
        assert shifted(p, 20, 20, 20, p, 1, 3, 3, 21, p, p, p, p, None) == e_shape
        assert shifted(p, 20, 20, 20, p, 0, 3, 3, 3, p, p, p, p, None) == e_arg
    assert lib.lsr_psf_accumulate_shifted_f32(p, 20, 20, 20, p, 1, 3, 3, 3, p, p, None, p, None) == null
    assert lib.lsr_psf_accumulate_shifted_f32(p, 20, 20, 20, p, 1, 3, 3, 3, p, p, p + 4, p, None) == e_arg
    assert b"8-byte aligned" in lib.lsr_last_error()
    nbytes = ctypes.c_int64(-1)
    assert lib.lsr_psf_shift_scratch_bytes(1, 3, 3, 3, None) == null
    assert lib.lsr_psf_shift_scratch_bytes(1, 3, 2, 3, ctypes.byref(nbytes)) == e_arg
    assert lib.lsr_psf_shift_scratch_bytes(1, 3, 3, 131, ctypes.byref(nbytes)) == e_unsupported
    assert lib.lsr_psf_shift_scratch_bytes(0, 3, 3, 3, ctypes.byref(nbytes)) == e_arg
    assert lib.lsr_psf_shift_scratch_bytes(3, 3, 5, 7, ctypes.byref(nbytes)) == ok
    assert nbytes.value == 8 * (105 + 1 + 64 + 2 * 3 * 105)               # accumulator, count, flags, two patches per bead
    assert lib.lsr_psf_shift_scratch_bytes(1000, 3, 5, 7, ctypes.byref(nbytes)) == ok
    assert nbytes.value == 8 * (105 + 1 + 64 + 2 * 64 * 105)              # ... of a batch of 64


# ------------------------------------------------------------------ 6. the command


@pytest.fixture
def cpu_cli(monkeypatch):
    import shrimpy_amd.cli as cli

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return cli


def _write_scene(tmp_path, scale):
    vol = r.scene_a()[0]
    src = tmp_path / "beads.zarr"
    with open_ome_zarr(src, layout="hcs", mode="w", channel_names=["GFP"], version="0.5", prefer_iohub=False) as plate:
        arr = plate.create_position("0", "0", "0").create_zeros("0", shape=(1, 1) + vol.shape, dtype="float32", scale=(1, 1) + scale)
        arr.write_volume(0, 0, vol)
    return vol, src


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def round_trip(tmp_path, cli, device):
    """Check 6 (``--alignment subvoxel`` over a YAML that does not ask for it) and the command's half of check 5."""
    from click.testing import CliRunner

    scale = (0.25, 0.116, 0.116)
    vol, src = _write_scene(tmp_path, scale)
    settings = scene_a_settings(patch_size=(11 * scale[0], 13 * scale[1], 13 * scale[2]))
    settings.to_yaml(tmp_path / "psf.yml")
    base = ["characterize-psf", "-i", str(src), "-c", str(tmp_path / "psf.yml")]
    # defaults: the parent's peaks.csv to the byte, the parent's report keys
    plain = tmp_path / "plain.zarr"
    res = CliRunner().invoke(cli.cli, base + ["-o", str(plain)])
    assert res.exit_code == 0, (res.output, res.exception)
    api = psf.characterize_psf(_t(vol, device), settings, scale)
    lines = [",".join(PARENT_CSV_HEADER)]
    for (z, y, x), v, iso, fw in zip(api.peaks, api.values, api.isolated, api.fwhm_vox_zyx):
        lines.append(",".join([str(int(z)), str(int(y)), str(int(x)), repr(float(v)), str(int(iso))] + [repr(float(q)) for q in fw]))
    assert (plain / "peaks.csv").read_bytes() == ("\r\n".join(lines) + "\r\n").encode()
    report = json.loads((plain / "report.json").read_text())
    assert [k for k in report if k in api.report()] == PARENT_REPORT_KEYS and "unfit" not in report
    assert not any(k.startswith(("fit_", "psf_fit_")) or k in ("n_unfit", "alignment") for k in report)
    # --alignment subvoxel
    out = tmp_path / "aligned.zarr"
    res = CliRunner().invoke(cli.cli, base + ["-o", str(out), "--alignment", "subvoxel"])
    assert res.exit_code == 0, (res.output, res.exception)
    api = psf.characterize_psf(_t(vol, device), scene_a_settings(patch_size=settings.patch_size, alignment="subvoxel"), scale)
    with open_ome_zarr(out, prefer_iohub=False) as store:
        key, pos = next(iter(store.positions()))
        assert key == "0/0/0" and tuple(pos["0"].shape) == (1, 1, 11, 13, 13)
        assert np.array_equal(pos["0"].read_volume(0, 0), api.psf.cpu().numpy())
    rows = _rows(out / "peaks.csv")
    assert list(rows[0]) == PARENT_CSV_HEADER + FIT_CSV_HEADER
    assert np.array_equal(np.array([[int(q[k]) for k in "zyx"] for q in rows]), api.peaks)
    assert np.array_equal(np.array([int(q["fit_status"]) for q in rows]), api.fit.status)
    for cols, want in ((["mu_z", "mu_y", "mu_x"], api.fit.offset_zyx), (["fit_fwhm_z", "fit_fwhm_y", "fit_fwhm_x"], api.fit.fwhm_axis_zyx),
                       (["fit_fwhm_p0", "fit_fwhm_p1", "fit_fwhm_p2"], api.fit.fwhm_principal),
                       (["fwhm_z", "fwhm_y", "fwhm_x"], api.fwhm_vox_zyx)):
        got = np.array([[float(q[k]) for k in cols] for q in rows])
        if device.type == "cpu" or cols[0] == "fwhm_z":
            assert np.array_equal(got, want, equal_nan=True), cols
        else:               # two runs of the kernel agree to the bit; said here only as far as the fit's bound
            assert np.allclose(got, want, rtol=1e-9, atol=1e-9, equal_nan=True), cols
    report = json.loads((out / "report.json").read_text())
    for k, v in api.report().items():
        assert report[k] == json.loads(json.dumps(v)), k
    assert report["alignment"] == "subvoxel" and report["n_unfit"] == 0 and report["unfit"] == []
    assert report["settings"]["alignment"] == "subvoxel" and report["n_averaged"] == 10
    assert report["psf_fit_fwhm_principal_vox"] == pytest.approx(list(r.FWHM_PER_SIGMA * np.array(r.TRUE_SIGMA)), rel=0.005)
    # --gaussian-fit alone: the voxel-aligned PSF of the defaults, the extended table
    fitted = tmp_path / "fitted.zarr"
    res = CliRunner().invoke(cli.cli, base + ["-o", str(fitted), "--gaussian-fit"])
    assert res.exit_code == 0, (res.output, res.exception)
    assert list(_rows(fitted / "peaks.csv")[0]) == PARENT_CSV_HEADER + FIT_CSV_HEADER
    with open_ome_zarr(fitted, prefer_iohub=False) as a, open_ome_zarr(plain, prefer_iohub=False) as b:
        assert np.array_equal(next(iter(a.positions()))[1]["0"].read_volume(0, 0), next(iter(b.positions()))[1]["0"].read_volume(0, 0))
    assert json.loads((fitted / "report.json").read_text())["alignment"] == "voxel"


def test_cli_round_trip_on_the_cpu(tmp_path, cpu_cli):
    round_trip(tmp_path, cpu_cli, CPU)


def test_unfit_beads_are_listed_and_left_out():
    """A bead whose fit fails (a NaN inside its patch) is isolated, unfit, and not in the sub-voxel average."""
    vol = r.scene_a()[0].copy()
    vol[10 + 4, 12 - 5, 14 + 5] = np.nan                     # a corner region of the first bead's patch
    res = psf.characterize_psf(_t(vol), scene_a_settings(alignment="subvoxel"))
    first = int(np.flatnonzero((res.peaks == [10, 12, 14]).all(axis=1))[0]) if (res.peaks == [10, 12, 14]).all(axis=1).any() else None
    assert len(res.unfit) == 1 and res.fit.status[res.unfit[0]] == 5 and res.n_averaged == int(res.isolated.sum()) - 1
    assert first is None or res.unfit[0] == first
    assert np.isfinite(res.psf.numpy()).all() and res.report()["n_unfit"] == 1
    assert np.all(sigma_errors(res) <= 0.005)
