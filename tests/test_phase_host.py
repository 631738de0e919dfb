"""Label-free phase reconstruction without a GPU: settings, transfer function, extension rule, the float64 model's round
trip, the host (``torch.fft``) route against ``tests/phase_ref.py``, the adapter and the command line.

waveorder is not installed: PARITY IS UNPINNED and ``phase_ref`` (float64 NumPy, nothing of the package) is the oracle.

``HOST_TOL``: the host route is ``torch.fft`` in complex64 with a complex64 filter; its error, ``max|got - ref| / max|ref|``
over the cases of ``phase_ref.CASES``, was measured at 3.6e-7 (worst: (24, 40, 72), z_padding 5; the others 1.5e-7 ..
2.5e-7) and is pinned at four times that.

The per-length sweep of the row kernels (``tests/test_phase_lengths_gpu.py``) rests on ``phase_ref.extend`` and on float64
``rfft`` / ``irfft``: the first is held here to the mirror rule index by index, the second recomputed in single precision
under the sweep's own bounds.
"""
import numpy as np
import pytest
import torch
import yaml

from shrimpy_amd import phase as P
from shrimpy_amd.settings import PhaseSettings
from tests import phase_ref as R
from tests import transform_cases as T

HOST_TOL = 1.45e-6     # 4 x 3.6e-7 (measured, see above)

YAML_BLOCK = {       # config/mda/mantis/dynatrack_demo.yaml:171-181 with the two injected pixel sizes
    "transfer_function": dict(wavelength_illumination=0.450, z_padding=5, index_of_refraction_media=1.4,
                              numerical_aperture_detection=1.35, numerical_aperture_illumination=0.52,
                              invert_phase_contrast=False, yx_pixel_size=0.1133, z_pixel_size=0.17),
    "apply_inverse": dict(reconstruction_algorithm="Tikhonov", regularization_strength=0.01),
}


def _block(**tf):
    return dict(YAML_BLOCK, transfer_function=dict(YAML_BLOCK["transfer_function"], **tf))


# ---------------------------------------------------------------- settings


def test_settings_validate_the_reference_block(tmp_path):
    s = PhaseSettings(**YAML_BLOCK)
    assert s.transfer_function.z_padding == 5 and s.apply_inverse.regularization_strength == 0.01
    assert PhaseSettings(transfer_function=YAML_BLOCK["transfer_function"]).apply_inverse.regularization_strength == 1e-3
    path = tmp_path / "phase.yml"
    s.to_yaml(path)
    assert PhaseSettings.from_yaml(path) == s


@pytest.mark.parametrize("block, message", [
    (dict(YAML_BLOCK, apply_inverse=dict(reconstruction_algorithm="TV")), "not built"),
    (_block(numerical_aperture_detection=1.4), "numerical_aperture_detection < index_of_refraction_media"),
    (_block(numerical_aperture_illumination=1.36), "numerical_aperture_illumination <= numerical_aperture_detection"),
    (_block(yx_pixel_size=0.13), "aliases"),
    (_block(absorption_ratio=0.1), "Extra inputs"),
    (_block(z_padding=-1), "z_padding"),
])
def test_settings_reject(block, message):
    with pytest.raises(ValueError, match=message) as err:
        PhaseSettings(**block)
    if message == "aliases":       # one line
        assert "\n" not in str(err.value.errors()[0]["msg"])


# ---------------------------------------------------------------- extension rule


@pytest.mark.parametrize("n, g, table", [
    (5, 9, [0, 1, 2, 3, 4, 4, 3, 1, 0]),
    (7, 8, [0, 1, 2, 3, 4, 5, 6, 6]),
    (3, 16, [0, 1, 2, 2, 1, 0, 0, 0, 0, 0, 2, 2, 2, 2, 1, 0]),
    (8, 8, [0, 1, 2, 3, 4, 5, 6, 7]),
])
def test_mirror_extension_tables(n, g, table):
    assert P.mirror_indices(n, g).tolist() == table == R.mirror_table(n, g)


def test_extend_is_the_mirror_rule_index_by_index():
    """``phase_ref.extend`` is the only witness of the kernel's ``mirror_index`` in the per-length sweep
    (``tests/test_phase_lengths_gpu.py``): here it is held, on every geometry of that sweep, against the rule as the header of
    ``csrc/phase.hip`` words it, index by index, and against the same extension built from ``np.pad``."""
    seen = set()
    for i, x in enumerate(T.ROW_X):
        shape, grid = T.phase_geometry(i, x)
        assert all(0 < n <= g for n, g in zip(shape, grid))
        vol = np.arange(1, 1 + int(np.prod(shape)), dtype=np.float64).reshape(shape)        # every voxel its own value
        ext = R.extend(vol, grid)
        assert ext.shape == grid
        iz, iy, ix = ([T.mirror_literal(j, n, g) for j in range(g)] for n, g in zip(shape, grid))
        assert np.array_equal(ext, vol[np.ix_(iz, iy, ix)]), (shape, grid)
        for (n, g), literal in zip(zip(shape, grid), (iz, iy, ix)):
            assert P.mirror_indices(n, g).tolist() == literal == T.mirror_by_padding(np.arange(n), g).tolist(), (n, g)
            seen.add((n == g, g - n > n, g - n > 2 * n, (g - n) % 2))
    # no padding, padding longer than the volume, the clamp on both sides, odd and even padding: all were met
    assert {s[0] for s in seen} == {True, False} and any(s[1] for s in seen) and any(s[2] for s in seen)
    assert {s[3] for s in seen if not s[0]} == {0, 1}


@pytest.mark.parametrize("part", T.slices(list(enumerate(T.ROW_X))), ids=lambda p: f"{p[0][1]}..{p[-1][1]}")
def test_row_references_hold_in_single_precision(part):
    """No bound of the per-length sweep can hide a failure of its float64 reference: pocketfft in single precision on the
    same rows (forward: the mirror-extended volumes; inverse: the complex64 spectra) sits inside the same bounds at every
    length.  Worst ratios over all lengths: forward l2 0.387, max 6.72; inverse l2 0.492, max 8.79 (of 2.5 and 32)."""
    import scipy.fft as sf

    for i, x in part:
        with T.at(f"X = {x}"):
            vols, shape, grid = T.phase_volumes(i, x)
            for vol in vols:
                single = sf.rfft(R.extend(vol, grid).astype(np.float32), axis=2)
                assert single.dtype == np.complex64
                T.check_rows("single forward", single, T.forward_reference(vol, grid), x)
            rows, specs, shape, grid = T.phase_grid_rows(i, x)
            for spec in specs:
                single = sf.irfft(np.ascontiguousarray(spec.transpose(0, 2, 1)), n=x, axis=2) / np.float32(grid[0] * grid[1] * 2.5)
                assert single.dtype == np.float32
                T.check_rows("single inverse", single, T.inverse_reference(spec, grid, 2.5), x)


def test_grid_rule():
    assert P.phase_grid((171, 2048, 2270), 5) == (192, 2048, 2304) == R.grid((171, 2048, 2270), 5)
    for shape, pad in R.CASES + [((1, 1, 1), 0), ((8, 12, 16), 0), ((250, 7, 4093), 3)]:
        assert P.phase_grid(shape, pad) == R.grid(shape, pad)
    assert P.phase_grid((8, 12, 16), 0) == (8, 12, 16)
    from shrimpy_amd._lib import E_UNSUPPORTED, LsrError

    for shape, pad in (((250, 8, 8), 4), ((8, 8, 4097), 0)):
        with pytest.raises(LsrError) as err:
            P.PhasePlan(shape, _block(z_padding=pad), "cpu")
        assert err.value.code == E_UNSUPPORTED


# ---------------------------------------------------------------- transfer function and filter

TF_GRID = (12, 20, 24)


def _optics(**kw):
    o = dict(YAML_BLOCK["transfer_function"], **kw)
    o.pop("z_padding")
    return o


@pytest.fixture(scope="module")
def tf():
    half = P._half_transfer_function(TF_GRID, **_optics())
    return P.expand_half_spectrum(half, TF_GRID[2]), half


def test_transfer_function_is_the_reference_models(tf):
    want, _ = R.transfer_function(TF_GRID, **_optics())
    assert np.abs(tf[0] - want).max() <= 1e-12 * np.abs(want).max()
    real_tf, imag_tf = P.calculate_transfer_function((12, 20, 24), z_padding=0, **_optics())
    assert imag_tf is None and real_tf.dtype == torch.complex128 and np.array_equal(real_tf.numpy(), tf[1])


def test_transfer_function_has_no_dc_response_and_a_bounded_support(tf):
    h = tf[0]
    peak = np.abs(h).max()
    assert peak > 0
    assert abs(h[0, 0, 0]) <= 1e-12 * peak
    o = YAML_BLOCK["transfer_function"]
    _, nu_r = R.transfer_function(TF_GRID, **_optics())
    step = 1.0 / (min(TF_GRID[1:]) * o["yx_pixel_size"])
    outside = nu_r > (o["numerical_aperture_illumination"] + o["numerical_aperture_detection"]) / o["wavelength_illumination"] + step
    assert outside.sum() >= 8      # the grid's corners lie beyond the support
    assert np.abs(h[:, outside]).max() <= 1e-12 * peak


def test_filter_is_hermitian(tf):
    w = R.inverse_filter(tf[0], 0.01)
    assert np.abs(w - np.conj(R.negated(w))).max() <= 1e-12 * np.abs(w).max()
    # the package's: complex64 (XC, gy, gz); the two columns that are their own partners' are Hermitian exactly, and the
    # whole of it is the model's filter to complex64 rounding
    got = P.inverse_filter(tf[1], 0.01, TF_GRID[2])
    assert got.dtype == np.complex64 and got.shape == (TF_GRID[2] // 2 + 1, TF_GRID[1], TF_GRID[0])
    for kx in (0, TF_GRID[2] // 2):
        col = got[kx].T                                     # (gz, gy)
        assert np.array_equal(col, np.conj(R.negated(col)))
    full = P.expand_half_spectrum(got.transpose(2, 1, 0), TF_GRID[2])
    assert np.abs(full - w).max() <= 2.0 ** -23 * np.abs(w).max()
    assert np.abs(full - np.conj(R.negated(full))).max() == 0.0


def test_invert_phase_contrast_flips_the_sign():
    vol, settings, ref = R.case(0)
    _, settings_inv, ref_inv = R.case(0, invert=True)
    assert np.abs(ref).max() > 0.1
    assert np.abs(ref + ref_inv).max() <= 1e-9 * np.abs(ref).max()
    got = P.PhasePlan(vol.shape, settings_inv, "cpu")(torch.from_numpy(vol.copy())).numpy()
    assert R.rel_err(got, -ref) <= HOST_TOL


# ---------------------------------------------------------------- round trip, host route


def test_round_trip_without_padding():
    """On a volume that is its own grid, ``y = 1 + Re ifftn(H fftn(phi))`` reconstructs to ``ifftn(|H|^2 / (|H|^2 + reg)
    fftn(phi))``: the filter's own regularised identity."""
    shape, reg = (8, 12, 16), 0.01
    assert R.grid(shape, 0) == shape
    h, _ = R.transfer_function(shape, **_optics())
    rng = np.random.default_rng(7)
    kz, ky, kx = np.meshgrid(*(np.fft.fftfreq(n) for n in shape), indexing="ij")
    band = np.sqrt(kz ** 2 + ky ** 2 + kx ** 2) < 0.35
    phi = np.fft.ifftn(np.fft.fftn(rng.standard_normal(shape)) * band).real
    # (the contrast of the cases HOST_TOL was measured on, uniform(80, 600): float32 rounding follows the size of y / mean,
    # about 1 whatever phi is, so a faint phi would be held to a bound relative to a result far below its input's scale)
    phi *= 0.44 / np.fft.ifftn(h * np.fft.fftn(phi)).real.std()
    y = 1.0 + np.fft.ifftn(h * np.fft.fftn(phi)).real
    want = np.fft.ifftn(np.abs(h) ** 2 / (np.abs(h) ** 2 + reg) * np.fft.fftn(phi)).real
    assert np.abs(want).max() > 1e-3
    got = R.reconstruct(y, 0, reg, **_optics())
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # the package's host route on the same (float32) data against the model on that data, and so against the identity
    y32 = y.astype(np.float32)
    host = P.PhasePlan(shape, dict(YAML_BLOCK, transfer_function=dict(_optics(), z_padding=0)), "cpu")(torch.from_numpy(y32))
    assert R.rel_err(host.numpy(), R.reconstruct(y32, 0, reg, **_optics())) <= HOST_TOL


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_host_route_against_the_model(index):
    vol, settings, ref = R.case(index)
    plan = P.PhasePlan(vol.shape, settings, "cpu")
    got = plan(torch.from_numpy(vol.copy()))
    assert got.dtype == torch.float32 and tuple(got.shape) == vol.shape
    err = R.rel_err(got.numpy(), ref)
    print(f"host route {vol.shape} z_padding {R.CASES[index][1]}: {err:.3g}")
    assert err <= HOST_TOL
    assert plan.last_mean == pytest.approx(vol.astype(np.float64).mean(), rel=1e-12)
    out = torch.empty_like(got)
    assert plan(torch.from_numpy(vol.copy()), out=out) is out and torch.equal(out, got)


def test_module_functions_have_the_references_call_shapes():
    vol, settings, ref = R.case(0)
    tf_kw = dict(settings["transfer_function"], zyx_shape=vol.shape)
    real_tf, imag_tf = P.calculate_transfer_function(**tf_kw)
    data = torch.from_numpy(vol.copy())
    got = P.apply_inverse_transfer_function(data, real_tf, imag_tf, z_padding=tf_kw["z_padding"], **settings["apply_inverse"])
    assert torch.equal(got, P.PhasePlan(vol.shape, settings, "cpu")(data))
    with pytest.raises(NotImplementedError, match="TV"):
        P.apply_inverse_transfer_function(data, real_tf, None, z_padding=2, reconstruction_algorithm="TV")


def test_a_mean_that_cannot_be_divided_by_is_an_error():
    vol, settings, _ = R.case(0)
    plan = P.PhasePlan(vol.shape, settings, "cpu")
    for bad in (np.zeros_like(vol), vol - vol.mean() - 1.0, np.full_like(vol, np.nan)):
        with pytest.raises(ValueError, match="mean"):
            plan(torch.from_numpy(np.ascontiguousarray(bad, dtype=np.float32)))


# ---------------------------------------------------------------- adapter and command line

DESKEW = dict(ls_angle_deg=30.0, pixel_size_um=0.1133, scan_step_um=0.15, keep_overhang=False, average_n_slices=3)


def test_adapter_runs_phase_behind_deskew(monkeypatch):
    from shrimpy_amd.preprocessing import build_preprocessor

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    shape = (96, 16, 24)
    pre = build_preprocessor(shape, ["deskew", "phase"], deskew=DESKEW, phase=YAML_BLOCK, output_channel="BF")
    raw = np.random.default_rng(5).integers(80, 600, shape).astype(np.uint16)
    out = pre(raw, return_intermediates=True)
    assert set(out) == {"BF", "deskew", "phase"} and out["phase"] is out["BF"]
    deskewed = out["deskew"]
    assert tuple(out["BF"].shape) == tuple(deskewed.shape) == pre._zyx_shape and out["BF"].dtype == torch.float32
    want = P.PhasePlan(tuple(deskewed.shape), YAML_BLOCK, "cpu")(deskewed)
    assert torch.equal(out["BF"], want) and float(want.abs().max()) > 0
    assert set(pre(raw)) == {"BF"}


def test_steps_without_their_settings_still_fail_loudly():
    from shrimpy_amd.preprocessing import build_preprocessor

    with pytest.raises(NotImplementedError, match="phase"):
        build_preprocessor((16, 64, 64), ["deskew", "phase"], deskew=DESKEW)
    with pytest.raises(NotImplementedError):
        build_preprocessor((16, 64, 64), ["vs"], phase=YAML_BLOCK)
    with pytest.raises(NotImplementedError):
        build_preprocessor((16, 64, 64), ["deskew", "phase", "vs"], deskew=DESKEW, phase=YAML_BLOCK)


def test_cli_writes_a_readable_phase_store(tmp_path, monkeypatch):
    from click.testing import CliRunner

    import shrimpy_amd.cli as cli

    from shrimpy_amd.io.omezarr import open_ome_zarr

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    shape, scale = (6, 10, 13), (1.0, 1.0, 0.17, 0.1133, 0.1133)
    rng = np.random.default_rng(11)
    vols = {key: rng.uniform(80, 600, (2,) + shape).astype(np.float32) for key in ("A/1/0", "B/2/0")}
    src = tmp_path / "deskewed.zarr"
    with open_ome_zarr(src, layout="hcs", mode="w", channel_names=["BF"], version="0.5", prefer_iohub=False) as plate:
        for key, v in vols.items():
            arr = plate.create_position(*key.split("/")).create_zeros("0", shape=(2, 1) + shape, dtype="float32", scale=scale)
            for t in range(2):
                arr.write_volume(t, 0, v[t])
    block = _block(z_padding=2)
    cfg = tmp_path / "phase.yml"
    cfg.write_text(yaml.safe_dump(block))
    out = tmp_path / "phase.zarr"
    run = CliRunner().invoke(cli.cli, ["phase", "-i", str(src), "-c", str(cfg), "-o", str(out), "--compression", "none"])
    assert run.exit_code == 0, run.output
    plan = P.PhasePlan(shape, block, "cpu")
    with open_ome_zarr(out, prefer_iohub=False) as plate:
        positions = dict(plate.positions())
        assert list(positions) == list(vols)
        for key, v in vols.items():
            arr = positions[key]["0"]
            assert arr.shape == (2, 1) + shape and arr.dtype == np.float32
            assert positions[key].channel_names == ["Phase3D"]
            assert tuple(positions[key].scale) == pytest.approx(scale)
            for t in range(2):
                np.testing.assert_array_equal(arr.read_volume(t, 0), plan(torch.from_numpy(v[t])).numpy())
    # the settings are part of the run's identity: --resume with another regularisation is refused
    cfg.write_text(yaml.safe_dump(dict(block, apply_inverse=dict(regularization_strength=0.1))))
    again = CliRunner().invoke(cli.cli, ["phase", "-i", str(src), "-c", str(cfg), "-o", str(out), "--resume"])
    assert again.exit_code != 0 and "different settings" in again.output
