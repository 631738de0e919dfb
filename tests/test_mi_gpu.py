"""Mutual-information metric of the registration estimate on the device: the joint-histogram kernel against its host
twin bit for bit (integer sums), the sizes at which a 32-bit LDS counter would wrap, the gradient kernel against its twin,
the recovery of a known transform under a non-monotone intensity map, and ``estimate-registration --metric mi`` followed
by ``register`` store to store.  The twins are pinned to ``tests/mi_ref.py`` by ``test_mi_host.py``; the kernels meet
``mi_ref`` directly, at every dispatch edge, in ``test_mi_fp64_gpu.py``."""

import numpy as np
import pytest

from oracle import cpu_ref as o
from tests import mi_cases as cases
from tests import mi_ref as ref
from tests.test_estimate import _scene, _tilted

pytestmark = pytest.mark.gpu


def _both(device, mov, tgt, m, stride, bins, ranges):
    """(kernel, kernel again, twin) histograms of one case."""
    import torch

    from shrimpy_amd.estimate import joint_histogram

    dm, dt = torch.as_tensor(mov, device=device), torch.as_tensor(tgt, device=device)
    first = joint_histogram(dm, dt, m, stride, bins, ranges)
    again = joint_histogram(dm, dt, m, stride, bins, ranges)
    twin = joint_histogram(torch.as_tensor(mov), torch.as_tensor(tgt), m, stride, bins, ranges)
    return first, again, twin


@pytest.mark.parametrize("bins", cases.BINS)
def test_histogram_kernel_equals_the_twin_bit_for_bit(device, bins):
    """Every histogram case of the host file (moving and target shapes differ in all of them)."""
    mov, tgt = cases.exact_pair()
    gmov, gtgt, gm, granges = cases.general_pair()
    for stride in cases.STRIDES:
        for args in ((mov, tgt, cases.EIGHTHS, stride, bins, cases.exact_ranges(bins)), (gmov, gtgt, gm, stride, bins, granges)):
            first, again, twin = _both(device, *args)
            assert first[1] == twin[1] and first[1] > 500
            assert np.array_equal(first[0], twin[0]), (bins, stride)
            assert again[1] == first[1] and np.array_equal(again[0], first[0])
            assert int(first[0].sum()) == 65536 * first[1]


def test_histogram_kernel_edge_cases_equal_the_twin(device):
    rng = np.random.default_rng(1)
    tgt = rng.uniform(-50, 300, (6, 7, 8)).astype(np.float32)
    tgt[0, 0, 0], tgt[1, 1, 1], tgt[2, 2, 2] = 200.0, -1e6, 1e6
    mov = rng.uniform(-50, 300, (6, 7, 8)).astype(np.float32)
    ranges = ((0.0, 200.0), (10.0, 180.0))
    far = np.eye(4)
    far[:3, 3] = 1000.0
    for m in (np.eye(4), far):
        first, _, twin = _both(device, mov, tgt, m, 1, 8, ranges)
        assert first[1] == twin[1] and np.array_equal(first[0], twin[0])
    assert first[1] == 0 and not first[0].any()


@pytest.mark.parametrize("shape,bins", [((260, 256, 256), 4), ((513, 512, 512), 4)])
def test_histogram_counters_do_not_wrap(device, shape, bins):
    """A constant pair at stride 1: every sample puts its full weight into ONE cell.  (260, 256, 256): tens of thousands
    of samples per workgroup in that cell.  (513, 512, 512): more than 1000 iterations per wave, the interval at which a
    wave flushes its 32-bit LDS table -- 1026 iterations x 64 lanes x 65536 exceeds 2^32 without the flush."""
    import torch

    from shrimpy_amd.estimate import joint_histogram

    mov = torch.full(shape, 1.0, dtype=torch.float32, device=device)
    tgt = torch.full(shape, 1.0, dtype=torch.float32, device=device)
    hist, n = joint_histogram(mov, tgt, np.eye(4), 1, bins, ((0.0, 2.0), (0.0, 3.0)))   # a = 2; u = 1: b0 = 1, f = 0
    assert n == (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
    want = np.zeros((bins, bins), np.uint64)
    want[2, 1] = 65536 * n
    assert np.array_equal(hist, want)
    del mov, tgt
    torch.cuda.empty_cache()


@pytest.mark.parametrize("bins,stride", [(8, 1), (32, 2), (64, (1, 2, 3))])
def test_gradient_kernel_matches_the_twin(device, bins, stride):
    import torch

    from shrimpy_amd.estimate import mi_gradient

    mov, tgt, m, ranges = cases.general_pair()
    hist, _ = ref.joint_histogram(mov, tgt, m, stride, bins, ranges)
    want = mi_gradient(torch.as_tensor(mov), torch.as_tensor(tgt), m, stride, bins, ranges, hist, cases.CENTRE, cases.SCALE)
    dm, dt = torch.as_tensor(mov, device=device), torch.as_tensor(tgt, device=device)
    got = mi_gradient(dm, dt, m, stride, bins, ranges, hist, cases.CENTRE, cases.SCALE)
    again = mi_gradient(dm, dt, m, stride, bins, ranges, hist, cases.CENTRE, cases.SCALE)
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    assert np.array_equal(got, again)                      # fixed summation order
    # ... and with the histogram taken on the device by the function itself
    np.testing.assert_allclose(mi_gradient(dm, dt, m, stride, bins, ranges, None, cases.CENTRE, cases.SCALE), want,
                               rtol=1e-9, atol=1e-9 * np.abs(want).max())


def test_estimate_recovers_a_transform_under_a_non_monotone_intensity_map(device):
    """The recovery case of the host file at (32, 64, 72) on the device, under the same conditions: worst corner error
    below 0.25 voxel, the restatement's MI at the estimate no lower than at the truth minus 1e-3 nats.  What
    ``metric="ssd"`` does on the same pair is printed, not asserted (DESIGN.md 4.8 records it).  Measured on an MI355X:
    corner error 0.014 voxel, MI 1.0995 against 1.0987 at the truth; SSD: 0.71 voxel, gain 1.32, residual RMS 21.6."""
    import torch

    from shrimpy_amd.estimate import estimate_affine_zyx

    shape = (32, 64, 72)
    mov, tgt, true = cases.recovery_pair(shape)
    dm, dt = torch.as_tensor(mov, device=device), torch.as_tensor(tgt, device=device)
    est = estimate_affine_zyx(dm, dt, metric="mi")
    assert est.metric == "mi" and np.isnan(est.rms) and est.n_samples > 0.5 * np.prod(shape)
    ranges = ((float(tgt.min()), float(tgt.max())), (float(mov.min()), float(mov.max())))

    def mi(m):
        return ref.mutual_information(ref.joint_histogram(mov, tgt, m, 1, 32, ranges)[0])

    err = cases.corner_error(est.affine_transform_zyx, true, shape)
    at_est, at_true = mi(est.affine_transform_zyx), mi(true)
    print(f"mi: corner error {err:.4f} voxel, MI at the estimate {at_est:.5f}, at the truth {at_true:.5f}, "
          f"{est.iterations} iterations")
    try:
        ssd = estimate_affine_zyx(dm, dt)
        print(f"ssd on the same pair: corner error {cases.corner_error(ssd.affine_transform_zyx, true, shape):.3f} voxel, "
              f"gain {ssd.gain:.3f}, rms {ssd.rms:.3f}")
    except Exception as exc:     # (recorded, not asserted)
        print(f"ssd on the same pair: {type(exc).__name__}: {exc}")
    assert err < 0.25
    assert at_est >= at_true - 1e-3


def test_cpu_tensor_beside_a_device_tensor_is_refused(device):
    import torch

    from shrimpy_amd._lib import LsrError
    from shrimpy_amd.estimate import estimate_affine_zyx, joint_histogram, mi_gradient

    a = torch.rand((8, 8, 8), device=device)
    with pytest.raises(LsrError):
        joint_histogram(a.cpu(), a, np.eye(4), 1, 8, ((0, 1), (0, 1)))
    with pytest.raises(LsrError):
        mi_gradient(a, a.cpu(), np.eye(4), 1, 8, ((0, 1), (0, 1)))
    with pytest.raises(LsrError):
        estimate_affine_zyx(a.cpu(), a, metric="mi")
    with pytest.raises(LsrError):
        joint_histogram(a, a, np.eye(4), 1, 3, ((0, 1), (0, 1)))
    far = np.eye(4)
    far[:3, 3] = 100
    with pytest.raises(LsrError, match="samples"):
        estimate_affine_zyx(a, a, initial=far, metric="mi")


def test_cli_estimate_with_mutual_information_then_register_store_to_store(tmp_path, device):
    """``estimate-registration --metric mi`` writes the YAML, ``register`` applies it to the source channel; the
    registered channel pushed through the non-monotone map then matches the target inside the valid region.  Bound: RMS
    below 0.05 of the target's standard deviation -- 2.5 times the 0.02 of the SSD store-to-store test: the estimate is
    allowed 0.25 voxel and the map doubles local slopes.  Measured on an MI355X: 0.0050 of the standard deviation."""
    from click.testing import CliRunner

    from shrimpy_amd.cli import cli
    from shrimpy_amd.io.omezarr import open_ome_zarr

    shape = (32, 64, 72)
    true = _tilted(shape, tilt=2.0, shift=(1.0, -3.0, 4.0))
    mov = _scene(11, shape, n=60)
    tgt = cases.non_monotone(o.affine_apply_4x4(mov, true, shape)).astype(np.float32)
    with open_ome_zarr(tmp_path / "pair.zarr", layout="hcs", mode="w", channel_names=["LF", "LS"],
                       prefer_iohub=False) as plate:
        arr = plate.create_position("A", "1", "0").create_zeros("0", shape=(1, 2) + shape, dtype="float32")
        arr.write_volume(0, 0, tgt)
        arr.write_volume(0, 1, mov)
    run = CliRunner()
    r = run.invoke(cli, ["estimate-registration", "-s", str(tmp_path / "pair.zarr"), "-t", str(tmp_path / "pair.zarr"),
                         "-o", str(tmp_path / "register.yml"), "--source-channel", "LS", "--target-channel", "LF",
                         "--metric", "mi"])
    assert r.exit_code == 0, (r.output, r.exception)
    assert "'metric': 'mi'" in r.output and "'mi':" in r.output
    r = run.invoke(cli, ["register", "-i", str(tmp_path / "pair.zarr"), "-c", str(tmp_path / "register.yml"),
                         "-o", str(tmp_path / "registered.zarr")])
    assert r.exit_code == 0, (r.output, r.exception)
    with open_ome_zarr(tmp_path / "registered.zarr", prefer_iohub=False) as plate:
        out = plate["A/1/0"]["0"]
        np.testing.assert_array_equal(out.read_volume(0, 0), tgt)                 # the target channel: untouched
        reg = out.read_volume(0, 1)
    inside = o.affine_apply_4x4(np.ones(shape, np.float32), true, shape) > 0.999
    rms = float(np.sqrt(np.mean((cases.non_monotone(reg) - tgt)[inside] ** 2)))
    print(f"registered channel through the map against the target: RMS {rms:.4f} = {rms / tgt.std():.4f} of the target's std")
    assert rms < 0.05 * tgt.std()
