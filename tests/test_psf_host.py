"""Bead detection and PSF averaging on CPU tensors: the host twins (``lsr_local_max_candidates_f32_cpu``,
``lsr_psf_accumulate_f32_cpu``) against the NumPy / float64 restatement ``tests/psf_ref.py``, the recovery of a known PSF,
the settings and the ``characterize-psf`` command through to ``deconvolve --psf-dirpath``.  PARITY UNPINNED: there is no
reference arithmetic for this stage (biahub's ``_characterize_psf`` is not vendored); the restatement is the pin.

Detection is an integer result and is held exactly: coordinates and order equal ``psf_ref.detect`` on the smoothed volume
the implementation itself produced.

The smoothing is held separately against ``scipy.ndimage.correlate1d(mode="mirror")`` in float64 (the same float32(1 / b)
taps, no intermediate rounding) at 2 units of 2^-24 relative, per voxel.  ``lsr_box_smooth_f32`` sums in float64, keeps
float64 between its three passes and rounds once: a-priori within one unit (half an ulp of a float32 is at most 2^-24 of
its value); measured worst case 1.00 on the twin (the kernel runs the same operations in the same order).  Three chained float32
passes of ``lsr_blur_reflect_f32`` -- the first implementation -- have an a-priori ceiling of 4.5 units and measured 2.88
on this file's cases and 3.18 on a 64 x 512 x 600 volume: beyond the bound, which is why the smoothing has its own kernel.

The patch average is float64 accumulation rounded to float32 once: ``4 * 2^-24 * max|psf|`` absolute per voxel.  Measured
worst case on this file's scenes: 0.76 units, twin and kernel alike -- the rounding of the final float32 store alone is
up to one unit, so nothing can be materially lower and the bound as set (four units) stands.
"""
import csv
import json

import numpy as np
import pytest
import torch
import yaml

from oracle import cpu_ref as o
from shrimpy_amd import _lib, morphology, psf
from shrimpy_amd.io.omezarr import open_ome_zarr
from shrimpy_amd.settings import CharacterizeSettings, DeconvolveSettings
from tests import psf_ref as r

CPU = torch.device("cpu")
U = 2.0 ** -24
SMOOTH_BOUND_U = 2.0
PSF_BOUND_U = 4.0
TRUE_SIGMA = (2.0, 1.2, 1.2)

# the three dicts of scripts/measure_psf.py:20-50 (values copied as data; `device` is whatever the script resolved)
REFERENCE_DICTS = {
    "epi": {"block_size": (8, 8, 8), "blur_kernel_size": 3, "min_distance": 20, "threshold_abs": 200.0, "max_num_peaks": 500,
            "exclude_border": (5, 5, 5), "device": "cuda"},
    "ls": {"block_size": (64, 64, 32), "blur_kernel_size": 3, "nms_distance": 32, "min_distance": 50, "threshold_abs": 200.0,
           "max_num_peaks": 2000, "exclude_border": (5, 10, 5), "device": "cpu"},
    "deskew": {"block_size": (64, 32, 16), "blur_kernel_size": 3, "nms_distance": 10, "min_distance": 50,
               "threshold_abs": 200.0, "max_num_peaks": 500, "exclude_border": (5, 5, 5), "device": "cuda"},
}


def _t(a, device=CPU):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def tied(shape, seed, levels=6):
    """Small integers: ties and plateaus everywhere, across every tile boundary of the kernels."""
    return np.random.default_rng(seed).integers(0, levels, shape).astype(np.float32)


def noisy(shape, seed):
    rng = np.random.default_rng(seed)
    v = rng.gamma(2.0, 50.0, shape).astype(np.float32)
    k = max(4, int(np.prod(shape)) // 4000)
    v.reshape(-1)[rng.integers(0, v.size, k)] += rng.uniform(500, 4000, k).astype(np.float32)
    return v


def engineered(shape=(12, 14, 16)):
    """A tie pair in reach of each other, a plateau, and a chain: the second 3 of ``5 3 3`` sees no larger value in its own
    window, but ties with a voxel of smaller index that is itself NOT a maximum -- the tie rule must see that voxel."""
    v = tied(shape, 3, levels=3)
    v[3, 4, 5] = v[3, 4, 7] = 9.0
    v[8:10, 8:10, 8:11] = 7.0
    v[6, 1, :6] = [0, 0, 0, 0, 0, 0]
    v[5:8, 0:3, 9:16] = 0.0
    v[6, 1, 10:13] = [5.0, 3.0, 3.0]
    return v


def boundary_ties(r3=(3, 3, 3)):
    """Equal pairs that straddle the tile boundaries of the FORMER kernels (bead detection had a sliding maximum of its own
    until it moved onto the morphology passes): the x pass staged rows in two segments of 552 columns at X = 1100, the y and z
    passes worked in blocks of w = 2 r + 1 positions, threads in groups of 256 columns.  ``walk_ties`` is the same
    construction at the edges of the passes that run now."""
    w = 2 * r3[1] + 1
    v = np.zeros((2 * w + 2, 2 * w + 3, 1100), dtype=np.float32)
    v[2, 3, 551] = v[2, 3, 552] = 8.0            # x segment boundary
    v[4, w - 1, 255] = v[4, w, 256] = 6.0        # y block boundary and a thread-group boundary
    v[w - 1, 12, 700] = v[w, 12, 700] = 5.0      # z block boundary
    v[w, 1, 30] = v[w - 1, 2, 29] = 4.0          # the smaller index is on the previous plane
    return v


def row_segments():
    """(X, segment): a row just over one staged segment of the x pass, and the equal segments it is cut into -- from the
    exported tiling (``lsr_grey_morph_tiling``), as ``tests/morphology_cases.py`` sizes its shapes."""
    _, columns, segment, _ = morphology.tiling()
    x = segment + 52
    parts = -(-x // segment)
    return x, -(-(-(-x // parts)) // columns) * columns


def walk_ties(r3=(3, 3, 3)):
    """``boundary_ties`` at the edges of the morphology passes: the x pass stages a row of X = 2100 in two segments of 1088
    (at a segment of 2048), the y and z walks cut a line into blocks of w = 2 r + 1 positions, a wavefront owns 64 columns."""
    _, columns, _, _ = morphology.tiling()
    x, seg = row_segments()
    w = 2 * r3[1] + 1
    v = np.zeros((2 * w + 2, 2 * w + 3, x), dtype=np.float32)
    v[2, 3, seg - 1] = v[2, 3, seg] = 8.0                      # x segment boundary
    v[4, w - 1, columns - 1] = v[4, w, columns] = 6.0          # y block boundary and a column-group boundary
    v[w - 1, 12, 700] = v[w, 12, 700] = 5.0                    # z block boundary
    v[w, 1, 30] = v[w - 1, 2, 29] = 4.0                        # the smaller index is on the previous plane
    return v


# Half-widths at which the composition of the passes changes: an axis without a window gets no pass (A is s, B is A) and the z
# walk still runs at w = 1 -- every axis in turn, and all; a window wider than every axis; one inside every axis.
COMPOSITION_TRIPLES = [(0, 0, 0), (0, 2, 3), (2, 0, 3), (2, 3, 0), (0, 0, 2), (1, 0, 0), (6, 8, 12), (1, 2, 3)]
ZERO_TRIPLES = COMPOSITION_TRIPLES[:6]


def composition_cases():
    """(label, volume, min_distance, threshold) on one (5, 7, 11) volume of small integers and three value classes of it:
    signed zeros (the passes may hand back +0.0 for -0.0: equal), +inf (a tied pair in reach of each other, and a lone
    one) and a NaN.  No -inf: the restatement pads with it."""
    base = tied((5, 7, 11), 1, levels=3)
    zeros = base.copy()
    at = zeros == 0.0
    zeros[at] = np.where(np.random.default_rng(21).integers(0, 2, int(at.sum())) == 1, -0.0, 0.0).astype(np.float32)
    assert np.signbit(zeros).any() and (at & ~np.signbit(zeros)).any()
    inf = base.copy()
    inf[1, 2, 3] = inf[1, 2, 5] = inf[3, 3, 3] = np.inf
    nan = base.copy()
    nan[2, 3, 4] = np.nan
    for md in COMPOSITION_TRIPLES:
        kind = "zero half-width" if md in ZERO_TRIPLES else "half-widths"
        yield f"{kind} {md}", base, md, 1.0
        yield f"signed zeros {md}", zeros, md, -1.0
        yield f"+inf {md}", inf, md, 1.0
        yield f"a NaN in reach {md}", nan, md, 0.0


# (label, volume, blur, min_distance, threshold, exclude_border, max_num_peaks)
def detection_cases(big=False):
    yield "engineered", engineered(), 1, 2, 1.0, (0, 0, 0), None
    yield "X not a multiple of 4", noisy((9, 21, 37), 0), 3, 2, 150.0, (0, 0, 0), None
    yield "smaller than the window", noisy((5, 6, 7), 1), 3, 8, 0.0, (0, 0, 0), None
    yield "non-cubic r", noisy((12, 40, 70), 2), 3, (2, 9, 17), 120.0, (0, 0, 0), None
    yield "non-cubic r, ties", tied((12, 40, 70), 2), 1, (2, 9, 17), 1.0, (0, 0, 0), None
    yield "r = 64", noisy((70, 80, 150), 4), 3, 64, 100.0, (0, 0, 0), None
    yield "r = 64, ties", tied((70, 80, 150), 5, levels=40), 1, 64, 1.0, (0, 0, 0), None
    yield "exclude_border", noisy((16, 30, 44), 6), 3, 3, 150.0, (2, 3, 4), None
    yield "max_num_peaks", noisy((16, 30, 44), 7), 3, 3, 150.0, (1, 1, 1), 5
    yield "ties across tile boundaries", boundary_ties(), 1, 3, 1.0, (0, 0, 0), None
    yield "ties everywhere, two row segments", tied((9, 17, 1100), 8), 1, (1, 3, 5), 2.0, (0, 0, 0), None
    nan = noisy((10, 24, 36), 9)
    nan[4, 10, 17] = np.nan
    yield "a NaN", nan, 1, 3, 100.0, (0, 0, 0), None
    yield "a NaN, smoothed", nan, 3, 3, 100.0, (0, 0, 0), None
    for label, v, md, thr in composition_cases():
        yield label, v, 1, md, thr, (0, 0, 0), None
    two_segments = tied((9, 17, row_segments()[0]), 8)
    yield "morphology tiling: ties everywhere, two row segments", two_segments, 1, (1, 3, 5), 2.0, (0, 0, 0), None
    yield "morphology tiling: ties across tile boundaries", walk_ties(), 1, 3, 1.0, (0, 0, 0), None
    if big:
        yield "64 x 512 x 600", noisy((64, 512, 600), 10), 3, (5, 20, 50), 300.0, (5, 5, 5), 500
        yield "64 x 512 x 600, ties", tied((64, 512, 600), 11, levels=1000), 1, (3, 10, 24), 990.0, (0, 0, 0), None


def hold_detection(device, big=False):
    counts = {}
    for label, v, b, md, thr, border, cap in detection_cases(big):
        vol = _t(v, device)
        s = psf.smooth(vol, b)
        s_host = s.cpu().numpy()
        want_c, want_v, _ = r.detect(s_host, md, thr, border, cap)
        got_c, got_v = psf.detect_peaks(vol, min_distance=md, threshold_abs=thr, blur_kernel_size=b, exclude_border=border,
                                        max_num_peaks=cap)
        print(f"{label}: {len(want_c)} peaks")
        counts[label] = len(want_c)
        assert got_c.dtype == torch.int64 and got_v.dtype == torch.float32
        assert np.array_equal(got_c.numpy(), want_c), label
        assert np.array_equal(got_v.numpy(), want_v), label
    assert counts["engineered"] > 0 and counts["a NaN"] > 0 and counts["r = 64"] > 0
    for label, n in counts.items():
        if label.startswith(("zero half-width", "+inf", "morphology tiling")):
            assert n > 0, label
    return counts


def hold_smoothing(device, big=False):
    """Every figure is printed before anything is asserted; returns the worst case over the cases."""
    worst_of = {}
    for label, v, b, *_ in detection_cases(big):
        if b == 1:
            continue
        s_host = psf.smooth(_t(v, device), b).cpu().numpy()
        want = r.smooth(v, b)
        assert np.array_equal(np.isnan(s_host), np.isnan(want)), label       # a NaN spreads to the same voxels
        ok = ~np.isnan(want)
        err = np.abs(s_host.astype(np.float64)[ok] - want[ok]) / np.abs(want[ok])
        worst_of[label] = float(err.max() / U)
        print(f"{label}: smoothing off by {worst_of[label]:.3f} units of 2^-24 relative")
    worst = max(worst_of.values())
    assert worst <= SMOOTH_BOUND_U, worst_of
    return worst


# ------------------------------------------------------------------ 1. the restatement itself


def test_the_restatement_agrees_with_the_literal_triple_loop():
    v = engineered()
    assert v.shape == (12, 14, 16)
    for rr in (1, 2, (1, 2, 3), (3, 1, 2)):
        fast, slow = r.peak_mask(v, rr, 1.0), r.peak_mask_literal(v, rr, 1.0)
        assert np.array_equal(fast, slow), rr
    m = r.peak_mask(v, 2, 1.0)
    assert m[3, 4, 5] and not m[3, 4, 7], "of a tied pair in reach of each other the first in C order wins"
    assert m[8, 8, 8] and m[8:10, 8:10, 8:11].sum() == 1, "a plateau has one peak: its first voxel"
    assert m[6, 1, 10] and not m[6, 1, 11] and not m[6, 1, 12], "5 3 3: the second 3 ties with a non-maximum before it"
    nan = v.copy()
    nan[5, 5, 5] = np.nan
    for rr in (1, (1, 2, 3)):
        assert np.array_equal(r.peak_mask(nan, rr, 1.0), r.peak_mask_literal(nan, rr, 1.0)), rr
    assert not r.peak_mask(nan, 2, 1.0)[3:8, 3:8, 3:8].any(), "no peak within reach of a NaN"


# ------------------------------------------------------------------ 2. detection is exact


def test_twin_detection_equals_the_restatement_exactly():
    _lib.call("lsr_set_host_threads", 4)
    hold_detection(CPU)


def test_twin_smoothing_against_scipy_in_float64():
    _lib.call("lsr_set_host_threads", 4)
    assert hold_smoothing(CPU) <= 1.0 + 1e-9, "one rounding of a float64 sum: at most one unit"


def test_twin_detection_does_not_depend_on_the_thread_count():
    v = _t(tied((9, 17, 300), 12))
    for md in ((1, 3, 5), (0, 3, 5)):
        lists = []
        for n in (1, 3, 7):
            torch.set_num_threads(n)
            lists.append(psf.local_maxima(v, md, 2.0))
        torch.set_num_threads(1)
        assert len(lists[0][0]) > 0
        for idx, val in lists[1:]:
            assert np.array_equal(np.sort(idx), np.sort(lists[0][0])), md


def test_candidate_overflow_is_a_value_error_naming_the_threshold():
    vol = _t(noisy((16, 30, 44), 6))
    n = len(psf.detect_peaks(vol, min_distance=1, threshold_abs=0.0)[0])
    assert n > 8
    with pytest.raises(ValueError, match="threshold_abs"):
        psf.detect_peaks(vol, min_distance=1, threshold_abs=0.0, capacity=8)
    assert len(psf.detect_peaks(vol, min_distance=1, threshold_abs=0.0, capacity=n)[0]) == n     # exactly full is fine


def test_arguments_are_checked():
    vol = _t(noisy((8, 9, 10), 0))
    with pytest.raises(ValueError, match="64"):
        psf.detect_peaks(vol, min_distance=65, threshold_abs=0.0)
    with pytest.raises(ValueError, match="odd"):
        psf.detect_peaks(vol, min_distance=2, threshold_abs=0.0, blur_kernel_size=4)
    with pytest.raises(TypeError):
        psf.detect_peaks(vol.double(), min_distance=2, threshold_abs=0.0)
    with pytest.raises(ValueError, match="larger than the volume"):
        psf.average_psf(vol, [[4, 4, 5]], (9, 9, 11))
    with pytest.raises(ValueError, match="does not fit"):
        psf.average_psf(vol, [[1, 4, 5]], (5, 5, 5))
    lib = _lib.load()
    p = vol.data_ptr()
    with pytest.raises(ValueError, match="above"):
        psf.smooth(vol, 17)                                  # mirrored borders: 8 < every extent
    assert lib.lsr_box_smooth_f32_cpu(p, p, 8, 9, 10, 3, 0.3, None, None) == -4          # out aliases in
    rc = lib.lsr_local_max_candidates_f32_cpu(p, 8, 9, 10, 65, 1, 1, 0.0, p, p, 4, p, None, None)
    assert rc == _lib.E_UNSUPPORTED
    rc = lib.lsr_local_max_candidates_f32(p, 8, 9, 10, 1, 1, 65, 0.0, p, p, 4, p, p, None)       # refused before any launch
    assert rc == _lib.E_UNSUPPORTED


# ------------------------------------------------------------------ 3. the patch average


def average_cases():
    true = o.gaussian_psf((9, 7, 7), TRUE_SIGMA)[0]
    for shape, seed, density in (((64, 96, 112), 11, 3e-5), ((48, 160, 160), 12, 2e-5)):
        scene = o.bead_scene(shape, seed, psf=true, density=density)
        coords, _, iso = r.detect(r.smooth(scene, 3).astype(np.float32), 6, 400.0, patch_half=(6, 5, 5))
        yield f"scene {shape}", scene, coords[iso], (13, 11, 11)
    rng = np.random.default_rng(5)
    v = rng.normal(100.0, 30.0, (20, 22, 24)).astype(np.float32)
    yield "noise, flat patches", v, np.array([[5, 6, 7], [10, 11, 12], [14, 15, 16], [3, 18, 4]]), (5, 7, 3)


def hold_average(device):
    out = {}
    for label, v, coords, patch in average_cases():
        got, skipped, stats = psf.average_psf(_t(v, device), coords, patch, return_stats=True)
        want, bg, total, want_skipped = r.average(v, coords, patch)
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == patch
        assert np.array_equal(skipped, want_skipped), label
        assert np.allclose(stats[:, 0], bg, rtol=1e-13, atol=0) and np.allclose(stats[:, 1], total, rtol=1e-9, atol=1e-7), label
        worst = float(np.abs(got.astype(np.float64) - want).max() / (U * np.abs(want).max()))
        print(f"{label}: {len(coords)} beads, {len(skipped)} skipped, worst {worst:.3f} units of 2^-24 max|psf|")
        assert worst <= PSF_BOUND_U, label
        out[label] = (got, stats)
    return out


def test_twin_average_against_float64():
    hold_average(CPU)


def test_a_bead_without_flux_is_skipped_and_listed():
    v = np.full((20, 20, 20), 100.0, dtype=np.float32)
    v[10, 10, 10] = 500.0                       # a bead: S = 400 > 0
    v[5, 5, 5] = 20.0                           # a hole: S = -80
    coords = np.array([[10, 10, 10], [5, 5, 5], [14, 6, 6]])       # the third is flat: S = 0
    got, skipped, stats = psf.average_psf(_t(v), coords, (5, 5, 5), return_stats=True)
    assert list(skipped) == [1, 2]
    assert np.array_equal(stats, [[100.0, 400.0], [100.0, -80.0], [100.0, 0.0]])
    want = np.zeros((5, 5, 5), dtype=np.float32)
    want[2, 2, 2] = 1.0
    assert np.array_equal(got.numpy(), want)
    with pytest.raises(ValueError, match="nothing to average"):
        psf.average_psf(_t(v), coords[1:], (5, 5, 5))


# ------------------------------------------------------------------ 4. a known PSF comes back


def settings_of_check_4(**kw):
    return CharacterizeSettings(**dict(dict(blur_kernel_size=3, min_distance=6, threshold_abs=400.0, patch_size=(13, 11, 11),
                                            exclude_border=(0, 0, 0), max_num_peaks=None), **kw))


def hold_recovery(device):
    true = o.gaussian_psf((9, 7, 7), TRUE_SIGMA)[0]
    results = []
    for shape, seed, density in (((64, 96, 112), 11, 3e-5), ((48, 160, 160), 12, 2e-5)):
        # the planted voxels: bead_scene's own first draws
        rng = np.random.default_rng(seed)
        n = int(np.prod(shape))
        planted = set(int(i) for i in rng.integers(0, n, size=max(1, int(round(density * n)))))
        scene = o.bead_scene(shape, seed, psf=true, density=density)
        res = psf.characterize_psf(_t(scene, device), settings_of_check_4())
        assert res.patch_shape_zyx == (13, 11, 11)
        iso = res.peaks[res.isolated]
        lin = np.ravel_multi_index(tuple(iso.T), shape)
        print(f"{shape}: {len(planted)} planted, {len(res.peaks)} detected, {len(iso)} isolated, {len(res.skipped)} skipped")
        assert all(int(i) in planted for i in lin), "an isolated peak is not a planted voxel"
        assert len(iso) >= 8
        cut = res.psf.cpu().numpy()[2:-2, 2:-2, 2:-2].clip(0, None).astype(np.float64)
        cut /= cut.sum()
        err = float(np.abs(cut - true).max() / true.max())
        print(f"{shape}: cut PSF off by {err:.4f} of the peak; FWHM of the average {res.psf_fwhm_vox_zyx}")
        assert err <= 0.03
        want = 2.3548 * np.asarray(TRUE_SIGMA)
        assert np.all(np.abs(res.psf_fwhm_vox_zyx - want) <= 0.10 * want)
        # per-bead widths exist exactly for the isolated beads
        assert np.array_equal(np.isfinite(res.fwhm_vox_zyx).any(axis=1) | ~res.isolated, np.ones(len(res.peaks), dtype=bool))
        assert np.isnan(res.fwhm_vox_zyx[~res.isolated]).all()
        results.append(res)
    return results


def test_a_known_psf_is_recovered_by_the_twins():
    res = hold_recovery(CPU)
    assert (len(res[0].peaks), int(res[0].isolated.sum())) == (19, 11)
    assert int(res[1].isolated.sum()) == 13


def test_fwhm_of_sampled_profiles():
    x = np.arange(-10, 11, dtype=np.float64)
    tri = np.zeros((21, 21, 21))
    tri[:, 10, 10] = np.clip(8.0 - np.abs(x), 0, None)              # triangle: half maximum 4 at |x| = 4
    tri[10, :, 10] = np.clip(8.0 - 2 * np.abs(x), 0, None)          # ... at |x| = 2
    tri[10, 10, :] = 8.0                                            # never comes down inside the patch
    assert np.allclose(psf.fwhm_vox(tri, 0.0)[:2], [8.0, 4.0]) and np.isnan(psf.fwhm_vox(tri, 0.0)[2])
    assert np.isnan(psf.fwhm_vox(-tri, 0.0)).all()


# ------------------------------------------------------------------ 5. settings and the command


def test_the_reference_dicts_validate_and_the_settings_are_strict():
    for name, d in REFERENCE_DICTS.items():
        s = CharacterizeSettings(**d, axis_labels=("SCAN", "TILT", "COVERSLIP"), patch_size=(0.2 * 30, 0.116 * 36, 0.116 * 18))
        assert s.patch_shape_zyx((0.2, 0.116, 0.116)) == (31, 37, 19), name
        assert CharacterizeSettings(**d).patch_shape_zyx((0.3, 0.1, 0.1)) == (15, 19, 19), name     # the script's 15 x 18 x 18
    assert CharacterizeSettings(patch_size=(1.0, 1.0, 1.05)).patch_shape_zyx((0.5, 0.25, 0.1)) == (3, 5, 11)
    with pytest.raises(ValueError, match="block_sise"):
        CharacterizeSettings(block_sise=(8, 8, 8))
    with pytest.raises(ValueError, match="odd"):
        CharacterizeSettings(blur_kernel_size=4)
    with pytest.raises(ValueError, match="64"):
        CharacterizeSettings(min_distance=65)
    with pytest.raises(ValueError, match="64"):
        CharacterizeSettings(min_distance=(3, 3, 100))
    with pytest.raises(ValueError):
        CharacterizeSettings(threshold_abs=float("nan"))
    vol = _t(noisy((10, 12, 14), 0))
    with pytest.raises(ValueError, match="larger than the volume"):
        psf.characterize_psf(vol, CharacterizeSettings(min_distance=2, patch_size=(11, 11, 11), exclude_border=(0, 0, 0)))


@pytest.fixture
def cpu_cli(monkeypatch):
    import shrimpy_amd.cli as cli

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return cli


def round_trip(tmp_path, cli, device):
    """characterize-psf on a store the package's writer wrote -> load_psf -> deconvolve --psf-dirpath."""
    from click.testing import CliRunner

    true = o.gaussian_psf((9, 7, 7), TRUE_SIGMA)[0]
    shape, scale = (64, 96, 112), (0.25, 0.116, 0.116)
    scene = o.bead_scene(shape, 11, psf=true, density=3e-5)
    src = tmp_path / "beads.zarr"
    with open_ome_zarr(src, layout="hcs", mode="w", channel_names=["GFP"], version="0.5", prefer_iohub=False) as plate:
        arr = plate.create_position("0", "0", "0").create_zeros("0", shape=(1, 1) + shape, dtype="float32", scale=(1, 1) + scale)
        arr.write_volume(0, 0, scene)
    settings = settings_of_check_4(patch_size=(13 * scale[0], 11 * scale[1], 11 * scale[2]))
    settings.to_yaml(tmp_path / "psf.yml")
    out = tmp_path / "psf.zarr"
    res = CliRunner().invoke(cli.cli, ["characterize-psf", "-i", str(src), "-c", str(tmp_path / "psf.yml"), "-o", str(out)])
    assert res.exit_code == 0, (res.output, res.exception)
    api = psf.characterize_psf(_t(scene, device), settings, scale)
    assert api.patch_shape_zyx == (13, 11, 11)
    # the store: the layout load_psf reads, the input's scale, the API's array
    with open_ome_zarr(out, prefer_iohub=False) as store:
        key, pos = next(iter(store.positions()))
        assert key == "0/0/0" and tuple(pos["0"].shape) == (1, 1, 13, 11, 11)
        assert pos.scale[2:] == pytest.approx(scale)
        assert np.array_equal(pos["0"].read_volume(0, 0), api.psf.cpu().numpy())
    loaded = DeconvolveSettings(psf_path=str(out), psf_shape_zyx=(9, 7, 7)).load_psf()
    cut = api.psf.cpu().numpy()[2:-2, 2:-2, 2:-2].clip(0, None)
    assert np.array_equal(loaded, (cut / float(cut.sum(dtype=np.float64))).astype(np.float32))
    assert np.abs(loaded - true).max() <= 0.03 * true.max()
    # peaks.csv and report.json agree with the API result
    with open(out / "peaks.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["z", "y", "x", "value", "isolated", "fwhm_z", "fwhm_y", "fwhm_x"]
    assert np.array_equal(np.array([[int(q[k]) for k in "zyx"] for q in rows]), api.peaks)
    assert np.array_equal(np.array([float(q["value"]) for q in rows], dtype=np.float32), api.values)
    assert np.array_equal(np.array([int(q["isolated"]) for q in rows], dtype=bool), api.isolated)
    assert np.array_equal(np.array([[float(q["fwhm_" + k]) for k in "zyx"] for q in rows]), api.fwhm_vox_zyx, equal_nan=True)
    report = json.loads((out / "report.json").read_text())
    for k, v in api.report().items():
        assert report[k] == json.loads(json.dumps(v)), k
    assert (report["n_peaks"], report["n_isolated"], report["n_averaged"]) == (19, 11, 11)
    assert report["settings"]["min_distance"] == 6 and report["zyx_scale"] == pytest.approx(scale)
    assert report["psf_fwhm_zyx"] == pytest.approx([w * s for w, s in zip(report["psf_fwhm_vox_zyx"], scale)])
    assert "'n_isolated': 11" in res.output
    # ... and deconvolve runs with it
    data = tmp_path / "data.zarr"
    with open_ome_zarr(data, layout="hcs", mode="w", channel_names=["LS"], version="0.5", prefer_iohub=False) as plate:
        arr = plate.create_position("A", "1", "0").create_zeros("0", shape=(1, 1, 12, 30, 44), dtype="float32", scale=(1, 1) + scale)
        vol = o.bead_scene((12, 30, 44), 3, psf=None, density=4e-3)
        arr.write_volume(0, 0, vol)
    (tmp_path / "deconvolve.yml").write_text(yaml.safe_dump(dict(iterations=2, psf_shape_zyx=[9, 7, 7])))
    res = CliRunner().invoke(cli.cli, ["deconvolve", "-i", str(data), "-c", str(tmp_path / "deconvolve.yml"), "-o",
                                       str(tmp_path / "x.zarr"), "--psf-dirpath", str(out)])
    assert res.exit_code == 0, (res.output, res.exception)
    with open_ome_zarr(tmp_path / "x.zarr", prefer_iohub=False) as store:
        got = next(iter(store.positions()))[1]["0"].read_volume(0, 0).astype(np.float64)
    ref = o.richardson_lucy(vol, loaded, 2).astype(np.float64)
    assert np.all(np.abs(got - ref) <= 2e-4 * np.abs(ref) + 1e-4 * np.abs(ref).max())
    # an output that exists is never overwritten
    res = CliRunner().invoke(cli.cli, ["characterize-psf", "-i", str(src), "-c", str(tmp_path / "psf.yml"), "-o", str(out)])
    assert res.exit_code != 0 and "not empty" in res.output


def test_cli_round_trip_on_the_cpu(tmp_path, cpu_cli):
    round_trip(tmp_path, cpu_cli, CPU)


def test_cli_reports_a_patch_larger_than_the_volume(tmp_path, cpu_cli):
    from click.testing import CliRunner

    src = tmp_path / "tiny.zarr"
    with open_ome_zarr(src, layout="hcs", mode="w", channel_names=["GFP"], prefer_iohub=False) as plate:
        plate.create_position("0", "0", "0").create_zeros("0", shape=(1, 1, 8, 9, 10), dtype="float32")
    CharacterizeSettings(min_distance=2).to_yaml(tmp_path / "psf.yml")
    res = CliRunner().invoke(cpu_cli.cli, ["characterize-psf", "-i", str(src), "-c", str(tmp_path / "psf.yml"), "-o",
                                           str(tmp_path / "psf.zarr")])
    assert res.exit_code != 0 and "larger than the volume" in res.output
