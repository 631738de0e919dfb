"""The row kernels of the phase reconstruction (``csrc/phase.hip``) against a float64 DFT at EVERY row length they accept.

``phase.hip`` restates the tile helpers of ``csrc/rfft_rows.hip`` (``carve``, the half-table twiddle lookup, the XCD tile
order, the real-to-complex post step, the complex-to-real pre step, the dynamic-LDS opt-in) around its own gather
(``mirror_index``) and epilogues.  ``tests/test_fft_kernels_fp64_gpu.py`` pins the originals at all 86 lengths; this file
does the same for the copies, through the C entries directly, with that file's inputs (impulses at 0, 1 and width - 1,
tones at bins 0, 1, M / 2, M - 1, M, Hermitian-spectrum rows, zero-mean normal rows), row check and constants
(``tests/transform_cases.py``):

    ||got - ref||_2 <= 2.5 u log2(X) ||ref||_2        max|got - ref| <= 32 u log2(X) rms(ref)        u = 2^-24, per row

The geometry rotates with the length (``transform_cases.phase_geometry``): no padding, an odd width, padding shorter and
longer than the volume (the clamp), one sample; ragged second and third y tiles; z padding.  Lengths from X = 2048 launch
with more than 64 KB of LDS: the opt-in of both kernels runs here.  ``phase_ref.extend``, the witness of the mirror rule,
is itself held to the rule's wording in ``tests/test_phase_host.py``, where the float64 references are also recomputed in
single precision under the same bounds.

Worst ratios observed on an MI355X over all lengths (``WORST``): forward l2 0.538, max 10.1; inverse l2 0.536, max 5.08
(of 2.5 and 32; the originals: 0.655 and 8.30).
"""
import math

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib, fft3
from shrimpy_amd import phase as P
from tests import phase_ref as R
from tests import transform_cases as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 16
INDEXED = list(enumerate(T.ROW_X))
PARTS = T.slices(INDEXED)
PART_IDS = [f"{p[0][1]}..{p[-1][1]}" for p in PARTS]

# the worst ratio seen per family in this process (the FFT sweep's dict: read back when the constants are re-measured)
WORST = T.WORST


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device=DEV)


def _forward(vol_d, shape, grid, half, full):
    """One call with NaN-filled buffers: ``(spec with its guard, partial, mean)``."""
    gz, gy, gx = grid
    xc = gx // 2 + 1
    spec = _nan(gz * xc * gy + GUARD, torch.complex64)
    partial = _nan(_lib.call_value("lsr_phase_rows_scratch_bytes", gz, gy) // 8, torch.float64)
    mean = _nan(2, torch.float64)
    _lib.call("lsr_phase_rows_forward_c64", vol_d.data_ptr(), *shape, spec.data_ptr(), gz, gy, gx, half.data_ptr(),
              full.data_ptr(), partial.data_ptr(), mean.data_ptr(), _lib.stream_ptr(DEV))
    return spec, partial, mean


def test_the_sweep_covers_every_length_the_kernels_accept():
    assert len(T.ROW_X) == 86
    assert [x for x in range(0, 4101) if _lib.call_value("lsr_rfft_rows_supported", x)] == T.ROW_X
    # both sides of the 64 KB above which a launch needs the dynamic-LDS opt-in are swept
    lds = [(8 * (x // 2 + 1) + x // 4) * 8 for x in T.ROW_X]
    assert min(lds) < 65536 < max(lds) and sum(b > 65536 for b in lds) >= 10


@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
def test_forward_rows_every_length(part):
    """``lsr_phase_rows_forward_c64``: every row of the grid is the float64 DFT of the mirror-extended row; nothing is left
    unwritten and nothing is written past the spectrum; the sum and the mean are the float64 ones; the same bits twice."""
    for i, x in part:
        with T.at(f"X = {x}"):
            vols, shape, grid = T.phase_volumes(i, x)
            gz, gy, gx = grid
            xc = gx // 2 + 1
            count = int(np.prod(shape))
            half, full = fft3._row_twiddles(gx, DEV)
            for vol in vols:
                vol_d = torch.as_tensor(np.ascontiguousarray(vol), device=DEV)
                spec, partial, mean = _forward(vol_d, shape, grid, half, full)
                again = _forward(vol_d, shape, grid, half, full)
                spec_h, partial_h, (got_mean, got_sum) = spec.cpu().numpy(), partial.cpu().numpy(), mean.cpu().numpy()
                assert np.isnan(spec_h[-GUARD:]).all(), "written past the spectrum"
                body = spec_h[:-GUARD].reshape(gz, xc, gy)
                assert np.isfinite(body).all() and np.isfinite(partial_h).all(), "an element was not written"
                assert partial_h.shape == (gz * -(-gy // 8),)
                T.check_rows("phase forward", body.transpose(0, 2, 1), T.forward_reference(vol, grid), gx)
                exact = math.fsum(vol.astype(np.float64).ravel().tolist())
                budget = count * 2.0 ** -53 * float(np.abs(vol.astype(np.float64)).sum())
                assert abs(got_sum - exact) <= budget, f"sum {got_sum}, float64 {exact} (budget {budget:.3g})"
                assert got_mean == got_sum / float(count)
                for a, b in zip((spec, partial, mean), again):
                    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "a second call returns other bits"


@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
def test_inverse_rows_every_length(part):
    """``lsr_phase_rows_inverse_f32`` fed the complex64-rounded float64 spectrum of known rows of the grid and a mean of 2.5:
    the volume's rows come back cropped and divided by ``Z Y X mean``; nothing is written past the volume."""
    mean_value = 2.5
    mean = torch.tensor([mean_value, float("nan")], dtype=torch.float64, device=DEV)
    for i, x in part:
        with T.at(f"X = {x}"):
            _, specs, shape, grid = T.phase_grid_rows(i, x)
            gz, gy, gx = grid
            count = int(np.prod(shape))
            half, full = fft3._row_twiddles(gx, DEV)
            for spec in specs:
                spec_d = torch.as_tensor(spec, device=DEV)
                out = _nan(count + GUARD, torch.float32)
                _lib.call("lsr_phase_rows_inverse_f32", spec_d.data_ptr(), gz, gy, gx, half.data_ptr(), full.data_ptr(),
                          mean.data_ptr(), out.data_ptr(), *shape, _lib.stream_ptr(DEV))
                got = out.cpu().numpy()
                assert np.isnan(got[count:]).all(), "written past the volume"
                assert np.isfinite(got[:count]).all(), "a voxel was not written"
                want = T.inverse_reference(spec, grid, mean_value)
                T.check_rows("phase inverse", T.whole_rows(got[:count], want, shape), want[:shape[0], :shape[1]], gx)


# ---------------------------------------------------------------- the plan at a row length above the LDS opt-in

PLAN_SHAPE, PLAN_Z_PADDING = (4, 24, 2300), 2       # grid (8, 24, 2304): M = 1152, a 77 KB tile
PLAN_TOL = 1.33e-6                                  # 4 x 3.34e-7, the yardstick (measured, see the test)


def test_plan_above_the_lds_opt_in():
    """``PhasePlan`` on (4, 24, 2300) with ``z_padding`` 2 -- the production row length 2304, whose tile needs the dynamic-LDS
    opt-in -- against ``phase_ref.reconstruct``.  ``max|got - ref| / max|ref|`` measured on an MI355X: 4.40e-7;
    ``torch.fft`` in complex64 on the same device, extension and filter, the yardstick: 3.34e-7.  The convention of
    ``tests/test_phase_gpu.py`` is four times the device's value, 1.76e-6; that is above four times the yardstick, 1.34e-6,
    so the yardstick's multiple is the pin."""
    rng = np.random.default_rng(2304)
    vol = rng.uniform(80, 600, PLAN_SHAPE).astype(np.float32)
    optics = dict(R.YAML_OPTICS, invert_phase_contrast=False)
    settings = dict(transfer_function=dict(optics, z_padding=PLAN_Z_PADDING),
                    apply_inverse=dict(reconstruction_algorithm="Tikhonov", regularization_strength=R.YAML_REGULARIZATION))
    ref = R.reconstruct(vol, PLAN_Z_PADDING, R.YAML_REGULARIZATION, **optics)
    plan = P.PhasePlan(PLAN_SHAPE, settings, DEV)
    assert plan.grid == (8, 24, 2304) == R.grid(PLAN_SHAPE, PLAN_Z_PADDING)
    v = torch.as_tensor(vol, device=DEV)
    got = plan(v)
    iz, iy, ix = (t.to(DEV) for t in plan._index)
    ext = v[iz][:, iy][:, :, ix]
    yard = torch.fft.irfftn(torch.fft.rfftn(ext) * plan._filter.permute(2, 1, 0), s=plan.grid)
    yard = yard[:PLAN_SHAPE[0], :PLAN_SHAPE[1], :PLAN_SHAPE[2]] / plan.last_mean
    err, yard_err = R.rel_err(got.cpu().numpy(), ref), R.rel_err(yard.cpu().numpy(), ref)
    print(f"device {PLAN_SHAPE} z_padding {PLAN_Z_PADDING} grid {plan.grid}: {err:.3g} (torch.fft complex64: {yard_err:.3g})")
    T._record("phase plan 2304", err)
    T._record("phase plan 2304 yardstick", yard_err)
    assert got.dtype == torch.float32 and tuple(got.shape) == PLAN_SHAPE
    assert err <= PLAN_TOL
    assert plan.last_mean == pytest.approx(vol.astype(np.float64).mean(), rel=1e-12)
    assert torch.equal(plan(v), got)
