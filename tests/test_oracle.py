"""CPU tests of the oracle itself: frozen golden vectors, known answers, reference-captured fixtures.

Nothing here touches the GPU or the HIP library.  The oracle (``oracle/cpu_ref.py``) is test
infrastructure; these tests are what it is pinned by (parity with the reference's own arithmetic
is UNPINNED: the reference holds no golden vector for this path, see the oracle header).
"""

import numpy as np
import pytest

from oracle import cpu_ref as o

DESKEW_CASES = ["deskew_nooverhang_avg3", "deskew_overhang_avg1", "deskew_nooverhang_avg5_r0p4"]


@pytest.mark.parametrize("name", DESKEW_CASES)
def test_deskew_matches_frozen_golden(golden_dir, name):
    g = np.load(golden_dir / f"{name}.npz")
    out = o.deskew(g["raw"], float(g["ls_angle_deg"]), float(g["px_to_scan_ratio"]),
                   bool(g["keep_overhang"]), int(g["average_n_slices"]))
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out, g["out"])


def test_affine_matches_frozen_golden(golden_dir):
    g = np.load(golden_dir / "affine_rot2deg.npz")
    np.testing.assert_array_equal(o.affine_apply_4x4(g["vol"], g["matrix"], g["vol"].shape), g["out_constant"])
    out_g = o.affine_apply_4x4(g["vol"], g["matrix"], tuple(g["grid_shape"]), cval=float(g["grid_cval"]),
                               mode="grid-constant")
    np.testing.assert_array_equal(out_g, g["out_grid"])


def test_rl_matches_frozen_golden(golden_dir):
    g = np.load(golden_dir / "rl_5iter.npz")
    np.testing.assert_array_equal(o.richardson_lucy(g["y"], g["psf_sep"], 5), g["x_sep_5"])
    np.testing.assert_array_equal(o.richardson_lucy(g["y"], g["psf_rot"], 5), g["x_rot_5"])


def test_flatfield_matches_reference_capture(golden_dir):
    """The neighbour step: oracle == what the reference's own ``_flat_field_BF`` produced
    (captured by ``oracle/make_golden.py`` importing ``/root/reference/shrimpy/preprocessing.py``)."""
    g = np.load(golden_dir / "ref_preprocessing.npz")
    np.testing.assert_allclose(o.flat_field_bf(g["flatfield_in"]), g["flatfield_out"], rtol=2e-6)
    np.testing.assert_allclose(o.flat_field_bf(g["flatfield_in_odd"]), g["flatfield_out_odd"], rtol=2e-6)


# ---------------------------------------------------------------- known answers


def test_deskew_shape_rule_known_values():
    # config-2 mapping (2048, 512, 2048), 30 deg, r=0.755, avg 3
    shape, voxel = o.deskewed_shape((2048, 512, 2048), 30.0, 0.755, False, 3, 0.1133)
    assert shape == (171, 2048, 2270)
    assert voxel == pytest.approx((3 * 0.5 * 0.1133, 0.1133, 0.1133))
    shape_k, _ = o.deskewed_shape((2048, 512, 2048), 30.0, 0.755, True, 1)
    assert shape_k == (512, 2048, int(np.ceil(2048 / 0.755 + 512 * np.cos(np.pi / 6))))


def test_deskew_reproduces_a_linear_field_exactly_inside():
    """Order-1 interpolation is exact on a field linear in z: the deskew of raw[z,y,x] = z is the
    z-coordinate map itself wherever the sample is in range."""
    Z, Y, X = 40, 10, 6
    raw = np.broadcast_to(np.arange(Z, dtype=np.float32)[:, None, None], (Z, Y, X)).copy()
    m, off, shape = o.deskew_geometry(raw.shape, 30.0, 0.755, True)
    out = o.affine_apply(raw, m, off, shape)
    zp, _, xp = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    z_in = m[0, 0] * zp + m[0, 2] * xp + off[0]
    inside = (z_in >= 0) & (z_in <= Z - 1)
    np.testing.assert_allclose(out[inside], z_in[inside], rtol=0, atol=1e-4)
    assert np.all(out[~inside] == 0)


def test_deskew_chunks_along_raw_x_concatenate_reversed():
    """``scripts/measure_psf.py:221,249``: deskew is independent along raw X and chunks are
    concatenated in REVERSE order on output axis -2."""
    rng = np.random.default_rng(5)
    raw = rng.random((40, 12, 16)).astype(np.float32)
    whole = o.deskew(raw, 30.0, 0.755, True, 3)
    chunks = [o.deskew(c, 30.0, 0.755, True, 3) for c in np.split(raw, 4, axis=-1)]
    np.testing.assert_array_equal(np.concatenate(chunks[::-1], axis=-2), whole)


def test_a_deskewed_plane_is_one_tilt_row_across_the_scan_stack():
    """The reference's viewer builds a deskewed plane from "a single tilt row across the whole scan stack"
    (``shrimpy/viewer/ring_buffer.py:98-105``, ``shrimpy/viewer/_napari_process.py:202-217``): before the slice
    averaging, output plane Z' depends on tilt row Y - 1 - Z' of the raw stack and on nothing else -- in the oracle
    and, on a CPU tensor, in the product's host twin."""
    import torch

    from shrimpy_amd.deskew import fast_deskew_zyx

    rng = np.random.default_rng(17)
    raw = rng.poisson(300, (90, 7, 20)).astype(np.float32)
    kw = dict(ls_angle_deg=30.0, px_to_scan_ratio=0.755, keep_overhang=True, average_n_slices=1)
    base = o.deskew(raw, 30.0, 0.755, True, 1)
    assert base.shape[0] == raw.shape[1]
    for row in (0, 3, 6):
        bumped = raw.copy()
        bumped[:, row, :] += 1000.0
        out = o.deskew(bumped, 30.0, 0.755, True, 1)
        changed = [z for z in range(base.shape[0]) if not np.array_equal(out[z], base[z])]
        assert changed == [raw.shape[1] - 1 - row]
        np.testing.assert_array_equal(fast_deskew_zyx(raw_data=torch.as_tensor(bumped), **kw).numpy(), out)


def test_average_slices_edge_padding():
    d = np.arange(5 * 2 * 2, dtype=np.float32).reshape(5, 2, 2)
    a = o.average_slices(d, 3)
    assert a.shape == (2, 2, 2)
    np.testing.assert_array_equal(a[0], (d[0] + d[1] + d[2]) / np.float32(3))
    np.testing.assert_array_equal(a[1], (d[3] + d[4] + d[4]) / np.float32(3))  # edge pad


def test_affine_identity_and_integer_shift():
    rng = np.random.default_rng(7)
    v = rng.random((6, 7, 8)).astype(np.float32)
    np.testing.assert_array_equal(o.affine_apply(v, np.eye(3), np.zeros(3), v.shape), v)
    sh = o.affine_apply(v, np.eye(3), np.array([1.0, 0.0, -2.0]), v.shape)
    np.testing.assert_array_equal(sh[:-1, :, 2:], v[1:, :, :-2])
    assert np.all(sh[-1] == 0) and np.all(sh[:, :, :2] == 0)


def test_constant_mode_has_no_border_blending():
    """with mode="constant" a coordinate at -1e-9 is OUT, n-1 exactly is IN."""
    v = np.ones((4, 4, 4), dtype=np.float32)
    out = o.affine_apply(v, np.eye(3), np.array([-1e-9, 0.0, 0.0]), v.shape)
    assert np.all(out[0] == 0) and np.all(out[1:] == 1)
    out = o.affine_apply(v, np.eye(3), np.array([0.0, 0.0, 0.0]), (4, 4, 4))
    assert np.all(out == 1)  # index n-1 exactly is inside


def test_rl_delta_psf_is_identity():
    rng = np.random.default_rng(9)
    y = (rng.random((6, 8, 10)) * 100 + 1).astype(np.float32)
    psf = np.zeros((3, 3, 3), np.float32)
    psf[1, 1, 1] = 1
    x = o.richardson_lucy(y, psf, 3)
    np.testing.assert_allclose(x, y, rtol=1e-5)


def test_rl_direct_and_fft_agree():
    psf, _ = o.gaussian_psf((5, 5, 5), (1.2, 1.0, 1.0))
    y = o.bead_scene((12, 24, 24), seed=11, psf=psf, density=2e-3)
    a = o.richardson_lucy(y, psf, 5)
    b = o.richardson_lucy(y, psf, 5, use_fft=True)
    np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-2)


def test_rl_tolerates_all_zero_volume():
    """Autofocus-failed stacks are written as all-zero volumes
    (``shrimpy/tests/test_mantis_integration.py:285-341``)."""
    psf, _ = o.gaussian_psf((3, 3, 3), (1, 1, 1))
    x = o.richardson_lucy(np.zeros((4, 6, 6), np.float32), psf, 4)
    assert np.all(x == 0) and np.all(np.isfinite(x))


def test_rl_increases_bead_contrast_and_stays_nonnegative():
    psf, _ = o.gaussian_psf((9, 7, 7), (2.0, 1.2, 1.2))
    y = o.bead_scene((20, 32, 32), seed=13, psf=psf, density=1e-3)
    x = o.richardson_lucy(y, psf, 20)
    assert x.min() >= 0
    assert x.max() > 1.5 * y.max()
    assert np.all(np.isfinite(x))


def test_even_psf_axis_padding_is_equivalent():
    from scipy import ndimage

    rng = np.random.default_rng(15)
    v = rng.random((6, 9, 9)).astype(np.float32)
    w = rng.random((2, 4, 3)).astype(np.float32)
    np.testing.assert_allclose(
        ndimage.correlate(v, o._as_odd_psf(w), mode="constant"),
        ndimage.correlate(v, w, mode="constant"), rtol=1e-6)


def test_gaussian_psf_is_separable_and_normalised():
    psf, (kz, ky, kx) = o.gaussian_psf()
    assert psf.shape == (9, 7, 7)
    assert abs(psf.sum(dtype=np.float64) - 1) < 1e-6
    np.testing.assert_allclose(psf, kz[:, None, None] * ky[None, :, None] * kx[None, None, :], rtol=1e-6)


def test_separable_rl_matches_dense_rl_for_asymmetric_factors():
    """The CPU-baseline formulation (three correlate1d passes, flipped taps for H) is the same
    algorithm as the dense loop, also when the factors are not symmetric."""
    rng = np.random.default_rng(17)
    ks = [rng.random(n).astype(np.float32) + 0.1 for n in (5, 3, 7)]
    ks = [k / k.sum() for k in ks]
    psf = (ks[0][:, None, None] * ks[1][None, :, None] * ks[2][None, None, :]).astype(np.float32)
    y = (rng.random((9, 12, 15)) * 50 + 1).astype(np.float32)
    np.testing.assert_allclose(o.richardson_lucy_separable(y, ks, 4), o.richardson_lucy(y, psf, 4),
                               rtol=2e-5)


def test_dynatrack_oracle_matches_reference_capture(golden_dir):
    """The f-3 row's oracle against what the reference's own estimator functions produced."""
    g = np.load(golden_dir / "ref_dynatrack.npz")
    a, b, thin = g["a"], g["b"], g["thin"]
    for p, want in zip(g["percentile_p"], g["percentile_a"]):
        assert o.dt_percentile(a, float(p)) == pytest.approx(float(want), rel=1e-6)
    np.testing.assert_allclose(o.dt_intensity_center_of_mass(a), g["icom_a_bg0"], atol=2e-4)
    np.testing.assert_allclose(o.dt_intensity_center_of_mass(a, 300.0), g["icom_a_bg300"], atol=2e-4)
    np.testing.assert_allclose(o.dt_intensity_center_of_mass(np.zeros((4, 5, 6))), g["icom_blank"])
    np.testing.assert_allclose(o.dt_gaussian_blur_3d(a, 1.0), g["blur_a_s1"], rtol=2e-6, atol=1e-4)
    np.testing.assert_allclose(o.dt_gaussian_blur_3d(a, 2.5), g["blur_a_s2p5"], rtol=2e-6, atol=1e-4)
    np.testing.assert_allclose(o.dt_gaussian_blur_3d(thin, 2.0), g["blur_thin_s2"], rtol=2e-6, atol=1e-4)
    blur = o.dt_gaussian_blur_3d((a - a.min()) / (a.max() - a.min()), 2.0)
    assert [o.dt_multiotsu_threshold(blur, c) for c in (0, 1)] == pytest.approx(g["otsu_blur_a"].tolist(), rel=1e-5)
    mask = o.dt_binary_mask(a, sigma=2.0)
    assert (mask != g["mask_a_s2"]).sum() <= 2            # voxels within 1e-7 of the threshold
    np.testing.assert_allclose(o.dt_center_of_mass(g["mask_a_s2"]), g["com_mask_a_s2"], atol=1e-4)
    np.testing.assert_allclose(o.dt_center_of_mass(np.zeros((3, 4, 5), bool)), g["com_empty"])
    np.testing.assert_allclose(o.dt_roi_shift(a), g["roi_shift_a"], atol=2e-4)
    np.testing.assert_allclose(o.dt_roi_shift(a, 50.0), g["roi_shift_a_p50"], atol=2e-4)
    np.testing.assert_allclose(o.dt_roi_shift(b, 90.0, 1.5), g["roi_shift_b_p90_blur"], atol=1e-3)
    np.testing.assert_allclose(o.dt_multiotsu_center_of_mass(a, b, 2.0, 0), g["motsu_shift_ab_s2"], atol=2e-2)
    np.testing.assert_allclose(o.dt_multiotsu_center_of_mass(a, b, 2.0, 1), g["motsu_shift_ab_s2_c1"], atol=2e-2)


def test_dynatrack_pcc_oracle_on_the_references_2d_known_answers():
    """``shrimpy/tests/test_dynatrack.py:85-100``: (32, 32) against itself -> (0, 0); (64, 64) rolled by
    (3, -5) -> (3, -5)."""
    img = np.random.default_rng(42).random((32, 32)).astype(np.float32)
    assert o.dt_phase_cross_corr(img, img.copy()) == (0, 0)
    ref = np.random.default_rng(42).random((64, 64)).astype(np.float32)
    assert o.dt_phase_cross_corr(ref, np.roll(ref, (3, -5), axis=(0, 1))) == (3, -5)


def test_dynatrack_pcc_oracle_matches_reference_capture(golden_dir):
    g = np.load(golden_dir / "ref_dynatrack.npz")
    assert o.dt_phase_cross_corr(g["pcc_ref"], g["pcc_mov"]) == tuple(g["pcc_shift"]) == (1, 2, -3)
    assert o.dt_phase_cross_corr(g["a"], g["b"]) == tuple(g["pcc_shift_ab"])
    assert o.dt_phase_cross_corr(g["pcc_odd"], g["pcc_odd_mov"]) == tuple(g["pcc_shift_odd"])
    assert o.dt_phase_cross_corr(g["pcc_odd"], g["pcc_odd_mov"], 0.5) == tuple(g["pcc_shift_odd_half"])
    np.testing.assert_array_equal(o.dt_match_shape(g["pcc_odd"], (8, 36, 50)), g["match_shape_odd_pad"])
    np.testing.assert_array_equal(o.dt_match_shape(g["pcc_odd"], (4, 36, 25)), g["match_shape_odd_mixed"])


def test_dynatrack_dispatcher_oracle_matches_reference_capture(golden_dir):
    """``dt_compute_shift`` / ``dt_limit_shifts_zyx`` against the reference's own
    ``DynaTrackUpdater._compute_shift`` and ``_limit_shifts_zyx`` outputs (captured fixture)."""
    g = np.load(golden_dir / "ref_dynatrack.npz")
    limits = {"z": (0.5, 2.0), "y": (0.1, 100.0), "x": (0.2, 0.9)}
    for vin, vout in zip(g["limit_shifts_in"], g["limit_shifts_out"]):
        np.testing.assert_array_equal(o.dt_limit_shifts_zyx(vin, limits), vout)
    methods = ("pcc", "intensity_center_of_mass", "roi_center_pcc", "multiotsu_center_of_mass", "multiotsu_pcc")
    kw = dict(scale_z=0.17, scale_yx=0.1133, otsu_sigma=2.0, blob_sigma=4.0, background_percentile=50.0, blur_sigma=1.5)
    for variant, extra in (("plain", {}), ("limited", dict(limits=limits, dampening=(0.5, 1.0, 0.8)))):
        for method, want in zip(methods, g[f"compute_shift_{variant}_xyz_um"]):
            if method in ("roi_center_pcc", "multiotsu_pcc"):
                continue  # (their estimators are covered by the PCC and mask fixtures)
            np.testing.assert_allclose(o.dt_compute_shift(g["a"], g["b"], method, **kw, **extra), want,
                                       rtol=0, atol=2e-4)


# ---------------------------------------------------------------- float64 restatements of the LDS FFT kernels


def _dft(n, sign=-1):
    """The explicit O(n^2) DFT matrix, exp(sign 2 pi i j k / n)."""
    j = np.arange(n)
    return np.exp(sign * 2j * np.pi * np.outer(j, j) / n)


@pytest.mark.parametrize("src_shape,grid", [((2, 3, 8), (2, 3, 8)), ((3, 5, 7), (4, 4, 12)), ((2, 6, 21), (3, 5, 20)),
                                            ((1, 2, 9), (2, 3, 16))])
def test_row_leg_restatements_against_the_dft_matrix(src_shape, grid):
    rng = np.random.default_rng(11)
    src = rng.standard_normal(src_shape).astype(np.float32)
    x = grid[2]
    dft = _dft(x)[: x // 2 + 1]                                           # rows k <= X / 2
    for zero in (False, True):
        if zero and any(s > g for s, g in zip(src_shape, grid)):
            continue
        if zero:
            v = np.zeros(grid)
            v[: src_shape[0], : src_shape[1], : src_shape[2]] = src
        else:
            v = o.dt_match_shape(src, grid).astype(np.float64)
        want = np.einsum("kn,zyn->zky", dft, v)
        got = o.rows_rfft_t(src, grid, zero=zero)
        assert got.shape == (grid[0], x // 2 + 1, grid[1])
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())
        # the inverse leg: X times the real inverse, i.e. the full Hermitian spectrum through exp(+2 pi i k n / X)
        full = np.concatenate([want, np.conj(want[:, 1 : x // 2][:, ::-1])], axis=1)     # [Z][X][Y]
        back = np.einsum("nk,zky->zyn", _dft(x, +1), full).real
        np.testing.assert_allclose(o.rows_irfft_t(want, x), back, rtol=0, atol=1e-12 * np.abs(back).max())
        np.testing.assert_allclose(back, x * v, rtol=0, atol=1e-10 * np.abs(v).max() * x)


@pytest.mark.parametrize("n", [2, 3, 5, 6, 8])
def test_z_leg_restatement_against_the_dft_matrix(n):
    rng = np.random.default_rng(n)
    xc, y = 2, 3
    f1 = rng.standard_normal((xc, y, n)) + 1j * rng.standard_normal((xc, y, n))
    g = rng.standard_normal((n, xc, y)) + 1j * rng.standard_normal((n, xc, y))
    fwd, inv = _dft(n), _dft(n, +1)                                       # n IFFT = the unscaled +i transform
    F = f1.transpose(2, 0, 1)
    for z_valid, z_keep in ((n, n), (max(1, n - 1), max(1, n // 2)), (1, n)):
        gv = g.copy()
        gv[z_valid:] = np.nan                                             # never read
        G = np.einsum("kz,zab->kab", fwd, np.where(np.isnan(gv), 0, gv))
        for mode, prod in ((0, F * np.conj(G)), (1, F * G), (2, np.conj(F) * G)):
            want = np.einsum("zk,kab->zab", inv, prod)[:z_keep]
            got = o.z_leg(f1, gv, mode, z_valid, z_keep)
            assert got.shape == (z_keep, xc, y)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("shape,psf_shape", [((4, 5, 6), (3, 3, 5)), ((2, 3, 9), (5, 1, 7)), ((3, 4, 2), (1, 3, 9))])
def test_rl_norm_direct_sums_the_taps_inside(shape, psf_shape):
    rng = np.random.default_rng(3)
    w = rng.random(psf_shape)
    got = o.rl_norm_direct(shape, w)
    c = [s // 2 for s in psf_shape]
    want = np.zeros(shape)
    for z, yy, x in np.ndindex(*shape):
        for a, b, e in np.ndindex(*psf_shape):
            p = (z + a - c[0], yy + b - c[1], x + e - c[2])
            if all(0 <= q < n for q, n in zip(p, shape)):
                want[z, yy, x] += w[a, b, e]
    np.testing.assert_allclose(got, want, rtol=1e-14)
    np.testing.assert_allclose(got, o.rl_norm(shape, w), rtol=1e-6)


@pytest.mark.parametrize("ref_shape,roll", [((8, 12, 16), (1, 2, -3)), ((9, 15, 20), (-2, 4, 5)), ((5, 7, 26), (2, -3, 6))])
def test_restated_legs_compose_to_the_trackers_phase_cross_correlation(ref_shape, roll):
    """x leg (rows_rfft_t), y transform, z leg (mode 0), y inverse, x inverse (rows_irfft_t): the peak of the
    fftshift-ed modulus is the shift ``dt_phase_cross_corr`` returns, on odd and even grids."""
    rng = np.random.default_rng(5)
    ref = rng.random(ref_shape).astype(np.float32)
    mov = np.roll(ref, roll, axis=(0, 1, 2)) + 0.05 * rng.random(ref_shape).astype(np.float32)
    grid = tuple(o.dt_next_fast_len(s) for s in ref_shape)
    f1 = np.fft.fft(np.fft.fft(o.rows_rfft_t(ref, grid), axis=2), axis=0).transpose(1, 2, 0)   # [XC][Y][Z]
    g = np.fft.fft(o.rows_rfft_t(mov, grid), axis=2)                                           # [Z][XC][Y]
    c = grid[1] * np.fft.ifft(o.z_leg(f1, g, 0), axis=2)
    corr = o.rows_irfft_t(c, grid[2])
    n = float(np.prod(grid))
    a, b = (o.dt_match_shape(v, grid).astype(np.float64) for v in (ref, mov))
    want = np.fft.irfftn(np.fft.rfftn(a) * np.conj(np.fft.rfftn(b)), s=grid, axes=(0, 1, 2))
    np.testing.assert_allclose(corr, n * want, rtol=0, atol=1e-9 * n * np.abs(want).max())
    peak = np.unravel_index(int(np.argmax(np.fft.fftshift(np.abs(corr)))), grid)
    assert tuple(s // 2 - int(p) for s, p in zip(grid, peak)) == o.dt_phase_cross_corr(ref, mov)


# ---------------------------------------------------------------- the float64 RL iteration (rl_iteration_f64)


def _rl_loops(x, y, w, eps, total_rows=None, first=0):
    """The iteration as literal loops over the taps of an odd PSF ``w`` (float64), voxel by voxel."""
    z, yy, xx = x.shape
    pz, py, px = w.shape
    cz, cy, cx = pz // 2, py // 2, px // 2
    total_rows = yy if total_rows is None else total_rows

    def at(v, a, b, c):
        return v[a, b, c] if 0 <= a < z and 0 <= b < yy and 0 <= c < xx else 0.0

    blur, corr, norm = np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape)
    for i, j, k in np.ndindex(x.shape):
        for a, b, c in np.ndindex(w.shape):
            blur[i, j, k] += w[a, b, c] * at(x, i - (a - cz), j - (b - cy), k - (c - cx))       # convolution
    ratio = y / (blur + np.float64(np.float32(eps)))
    for i, j, k in np.ndindex(x.shape):
        for a, b, c in np.ndindex(w.shape):
            corr[i, j, k] += w[a, b, c] * at(ratio, i + a - cz, j + b - cy, k + c - cx)         # correlation
            if 0 <= i + a - cz < z and 0 <= first + j + b - cy < total_rows and 0 <= k + c - cx < xx:
                norm[i, j, k] += w[a, b, c]
    return blur, ratio, x * corr / norm


def _rl_case(shape, psf_shape, seed):
    rng = np.random.default_rng(seed)
    ks = [rng.uniform(0.2, 1.0, n).astype(np.float32) for n in psf_shape]           # asymmetric: a flipped stage shows
    x = rng.uniform(0.5, 50.0, shape).astype(np.float32)
    y = rng.uniform(0.5, 50.0, shape).astype(np.float32)
    w = np.einsum("a,b,c->abc", *(k.astype(np.float64) for k in ks))
    return x, y, ks, w


@pytest.mark.parametrize("shape,psf_shape", [((4, 5, 6), (3, 5, 3)), ((3, 4, 7), (5, 3, 7)), ((2, 3, 2), (5, 7, 9)),
                                             ((1, 1, 5), (1, 1, 3)), ((5, 4, 3), (3, 1, 5))])
def test_rl_iteration_f64_equals_literal_loops_over_the_taps(shape, psf_shape):
    """Dense, separable and ky (x) kzx formulations against a triple loop over the taps, to 1e-13 relative: asymmetric
    taps (so convolution and correlation differ), PSFs larger than the volume on every axis among them."""
    x, y, ks, w = _rl_case(shape, psf_shape, sum(shape) + sum(psf_shape))
    want = _rl_loops(x.astype(np.float64), y.astype(np.float64), w, 1e-3)
    kzx = np.einsum("a,c->ac", ks[0].astype(np.float64), ks[2].astype(np.float64))
    for kw in (dict(psf=w), dict(factors=ks), dict(factors=(ks[1], kzx))):
        got = o.rl_iteration_f64(x, y, eps=1e-3, **kw)
        for g, r, name in zip(got, want, ("blur", "ratio", "x_new")):
            assert g.dtype == np.float64
            np.testing.assert_allclose(g, r, rtol=1e-13, atol=0, err_msg=f"{name} {sorted(kw)}")
    # a flipped stage is a different result on these taps
    flipped = o.rl_iteration_f64(x, y, psf=w[::-1, ::-1, ::-1], eps=1e-3)
    if max(psf_shape) > 1 and min(shape) > 1:
        assert np.abs(flipped[0] - want[0]).max() > 1e-3 * np.abs(want[0]).max()


def test_rl_iteration_f64_takes_the_y_norm_of_the_taller_volume():
    x, y, ks, w = _rl_case((3, 4, 5), (3, 5, 3), 77)
    for first, total in ((0, 9), (3, 9), (5, 9), (0, 4)):
        want = _rl_loops(x.astype(np.float64), y.astype(np.float64), w, 1e-6, total, first)
        for kw in (dict(psf=w), dict(factors=ks)):
            got = o.rl_iteration_f64(x, y, y_window=(first, total), **kw)
            np.testing.assert_allclose(got[2], want[2], rtol=1e-13, atol=0)
    # an interior slab has the full y sum everywhere; the first slab keeps the top border only
    mid = o.rl_iteration_f64(x, y, factors=ks, y_window=(3, 10))[2]
    assert not np.allclose(mid, o.rl_iteration_f64(x, y, factors=ks)[2], rtol=1e-6)


def test_rl_iteration_f64_takes_eps_as_the_float32_the_entries_receive():
    x, y, ks, w = _rl_case((3, 4, 5), (3, 3, 3), 5)
    x[:] = 0                                                       # ratio = y / eps exactly
    _, ratio, x_new = o.rl_iteration_f64(x, y, factors=ks, eps=1e-6)
    np.testing.assert_array_equal(ratio, y.astype(np.float64) / np.float64(np.float32(1e-6)))
    assert not x_new.any()


def test_rl_iteration_f64_against_the_float32_oracle_loop():
    """``richardson_lucy(..., iterations=1)`` rounds blur, ratio, correlation and norm to float32: it stays within a
    few float32 roundings of the float64 iteration on positive data (and an even PSF axis is padded the same way)."""
    rng = np.random.default_rng(9)
    psf = rng.uniform(0.2, 1.0, (5, 4, 3)).astype(np.float32)
    psf /= psf.sum()
    x = rng.uniform(1.0, 100.0, (9, 12, 17)).astype(np.float32)
    y = rng.uniform(1.0, 100.0, (9, 12, 17)).astype(np.float32)
    want = o.rl_iteration_f64(x, y, psf=psf)[2]
    got = o.richardson_lucy(y, psf, iterations=1, x0=x).astype(np.float64)
    assert np.abs(got - want).max() > 0                                # (it does round)
    assert (np.abs(got - want) <= 8 * 2.0 ** -24 * want).all()
