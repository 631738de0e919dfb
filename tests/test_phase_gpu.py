"""Label-free phase reconstruction on the device (``csrc/phase.hip``, ``shrimpy_amd/phase.py``) against the float64 model
of ``tests/phase_ref.py`` (PARITY UNPINNED: waveorder is not installed; the model is the oracle).

``DEVICE_TOL``: ``max|got - ref| / max|ref|`` over ``phase_ref.CASES`` (inputs ``uniform(80, 600)`` float32) measured on an
MI355X: 1.6e-7, 2.5e-7, 1.1e-7, 2.4e-7, 3.8e-7 in the order of the cases (worst: (24, 40, 72), z_padding 5); ``torch.fft`` in
complex64 on the same device, extension and filter, the yardstick: 1.5e-7, 2.4e-7, 1.9e-7, 2.6e-7, 3.1e-7.  Pinned at four
times the device's worst.

The two row kernels are also held alone to a float64 DFT of the extended rows, with the bounds the same LDS transforms
carry in ``tests/test_fft_kernels_fp64_gpu.py`` (per row, ``u = 2^-24``): ``||err||_2 <= 2.5 u log2(X) ||ref||_2`` and
``max|err| <= 32 u log2(X) rms(ref)``.
"""
import math

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib, fft3
from shrimpy_amd import phase as P
from tests import phase_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24
C_L2_ROWS, C_MAX_ROWS = 2.5, 32.0        # tests/test_fft_kernels_fp64_gpu.py: the x leg's transforms
DEVICE_TOL = 1.52e-6                     # 4 x 3.8e-7 (measured, see above)


def _check_rows(got, want, n):
    got = np.asarray(got).astype(np.complex128).reshape(-1, got.shape[-1])
    want = np.asarray(want).astype(np.complex128).reshape(-1, want.shape[-1])
    assert np.isfinite(got).all(), "non-finite output (an unwritten element?)"
    norm = np.linalg.norm(want, axis=1)
    assert (norm > 0).all()
    err = np.abs(got - want)
    unit = U * math.log2(n) * norm
    l2 = (np.linalg.norm(err, axis=1) / unit).max()
    mx = (err.max(axis=1) / (unit / math.sqrt(want.shape[1]))).max()
    print(f"rows: l2 {l2:.3g}, max {mx:.3g} (u log2 n)")
    assert l2 <= C_L2_ROWS and mx <= C_MAX_ROWS


ROW_CASES = [((5, 11, 13), (9, 12, 16)),        # a ragged second y tile, padding on every axis
             ((3, 4, 8), (15, 5, 8)),            # padding longer than the volume along z: the clamp; x = the grid's
             ((6, 17, 70), (8, 18, 72))]         # three y tiles, a row longer than one pass of the 64 lanes


@pytest.mark.parametrize("shape, grid", ROW_CASES)
def test_forward_rows_alone(shape, grid):
    """``lsr_phase_rows_forward_c64``: every row of the grid is the float64 DFT of the mirror-extended row; the mean and
    the sum are the float64 ones."""
    rng = np.random.default_rng(sum(shape))
    vol = rng.uniform(80, 600, shape).astype(np.float32)
    gz, gy, gx = grid
    xc = gx // 2 + 1
    half, full = fft3._row_twiddles(gx, DEV)
    src = torch.as_tensor(vol.copy(), device=DEV)
    spec = torch.full((gz, xc, gy), float("nan"), dtype=torch.complex64, device=DEV)
    partial = torch.full((_lib.call_value("lsr_phase_rows_scratch_bytes", gz, gy) // 8,), float("nan"), dtype=torch.float64,
                         device=DEV)
    mean = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.call("lsr_phase_rows_forward_c64", src.data_ptr(), *shape, spec.data_ptr(), gz, gy, gx, half.data_ptr(),
              full.data_ptr(), partial.data_ptr(), mean.data_ptr(), _lib.stream_ptr(DEV))
    want = np.fft.rfft(R.extend(vol, grid), axis=2)                     # (gz, gy, xc)
    _check_rows(spec.cpu().numpy().transpose(0, 2, 1), want, gx)
    exact = vol.astype(np.float64)
    got_mean, got_sum = mean.cpu().numpy()
    assert abs(got_mean - exact.mean()) <= 1e-12 * exact.mean() and abs(got_sum - exact.sum()) <= 1e-12 * exact.sum()
    assert partial.cpu().numpy().shape == (gz * -(-gy // 8),) and np.isfinite(partial.cpu().numpy()).all()


@pytest.mark.parametrize("shape, grid", ROW_CASES)
def test_inverse_rows_alone(shape, grid):
    """``lsr_phase_rows_inverse_f32`` fed the float64 x-leg spectrum of known rows: the rows come back cropped, divided by
    ``gz gy mean``; nothing outside the volume is written."""
    rng = np.random.default_rng(1 + sum(shape))
    gz, gy, gx = grid
    z, y, x = shape
    rows = rng.uniform(80, 600, grid)
    spec = np.fft.rfft(rows, axis=2).astype(np.complex64)
    spec_d = torch.as_tensor(np.ascontiguousarray(spec.transpose(0, 2, 1)), device=DEV)
    half, full = fft3._row_twiddles(gx, DEV)
    m = 2.5
    mean = torch.tensor([m, 0.0], dtype=torch.float64, device=DEV)
    out = torch.full((z * y * x + 16,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("lsr_phase_rows_inverse_f32", spec_d.data_ptr(), gz, gy, gx, half.data_ptr(), full.data_ptr(), mean.data_ptr(),
              out.data_ptr(), z, y, x, _lib.stream_ptr(DEV))
    got = out.cpu().numpy()
    assert np.isnan(got[z * y * x:]).all(), "written past the volume"
    want = np.fft.irfft(spec.astype(np.complex128), n=gx, axis=2) / (gz * gy * m)
    # (the bound is on whole rows of the grid; the cropped part of a row carries no more than the whole)
    full_rows = np.zeros((z, y, gx))
    full_rows[:, :, :x] = got[:z * y * x].reshape(shape)
    full_rows[:, :, x:] = want[:z, :y, x:]
    _check_rows(full_rows, want[:z, :y], gx)


def _device_errors(index):
    vol, settings, ref = R.case(index)
    plan = P.PhasePlan(vol.shape, settings, DEV)
    v = torch.as_tensor(vol.copy(), device=DEV)
    got = plan(v)
    # the yardstick: torch.fft in complex64 on the device, the same extension and filter
    iz, iy, ix = (t.to(DEV) for t in plan._index)
    ext = v[iz][:, iy][:, :, ix]
    yard = torch.fft.irfftn(torch.fft.rfftn(ext) * plan._filter.permute(2, 1, 0), s=plan.grid)
    yard = yard[:vol.shape[0], :vol.shape[1], :vol.shape[2]] / plan.last_mean
    return plan, v, got, R.rel_err(got.cpu().numpy(), ref), R.rel_err(yard.cpu().numpy(), ref)


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_plan_against_the_model(index):
    vol, settings, ref = R.case(index)
    plan, v, got, err, yard = _device_errors(index)
    print(f"device {vol.shape} z_padding {R.CASES[index][1]} grid {plan.grid}: {err:.3g} (torch.fft complex64: {yard:.3g})")
    assert got.dtype == torch.float32 and got.device == v.device and tuple(got.shape) == vol.shape
    assert err <= DEVICE_TOL
    assert plan.last_mean == pytest.approx(vol.astype(np.float64).mean(), rel=1e-12)
    # the same bits on a second call, and into a tensor of the caller's
    assert torch.equal(plan(v), got)
    out = torch.full_like(got, float("nan"))
    assert plan(v, out=out) is out and torch.equal(out, got)
    plan.release()
    assert torch.equal(plan(v), got)


def test_inverted_contrast_and_the_host_route_agree_with_the_device():
    vol, settings, ref = R.case(0, invert=True)
    got = P.PhasePlan(vol.shape, settings, DEV)(torch.as_tensor(vol.copy(), device=DEV)).cpu().numpy()
    assert R.rel_err(got, ref) <= DEVICE_TOL
    assert R.rel_err(got, -R.case(0)[2]) <= DEVICE_TOL


def test_a_zero_mean_volume_is_an_error():
    vol, settings, _ = R.case(0)
    plan = P.PhasePlan(vol.shape, settings, DEV)
    centred = (vol - vol.mean(dtype=np.float64)).astype(np.float32)
    centred[0, 0, 0] -= np.float32(centred.astype(np.float64).sum() + 1.0)      # the sum is now below zero for certain
    for bad in (np.zeros_like(vol), centred):
        with pytest.raises(ValueError, match="mean"):
            plan(torch.as_tensor(bad, device=DEV))
    with pytest.raises(ValueError, match="must be"):
        plan(torch.zeros((2, 2, 2), device=DEV))


def test_adapter_on_the_device():
    from shrimpy_amd.preprocessing import build_preprocessor
    from tests.test_phase_host import DESKEW, YAML_BLOCK

    shape = (96, 16, 24)
    pre = build_preprocessor(shape, ["deskew", "phase"], deskew=DESKEW, phase=YAML_BLOCK, output_channel="BF", require_gpu=True)
    raw = np.random.default_rng(5).integers(80, 600, shape).astype(np.uint16)
    out = pre(raw, return_intermediates=True)
    assert set(out) == {"BF", "deskew", "phase"} and out["BF"].device.type == "cuda"
    ref = R.reconstruct(out["deskew"].cpu().numpy(), 5, 0.01, **{k: v for k, v in YAML_BLOCK["transfer_function"].items()
                                                                  if k != "z_padding"})
    assert R.rel_err(out["BF"].cpu().numpy(), ref) <= DEVICE_TOL
