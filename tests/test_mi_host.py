"""Mutual-information metric of the registration estimate on the host: the native twins of the two kernels
(``lsr_affine_joint_histogram_f32_cpu``, ``lsr_affine_mi_gradient_f32_cpu``) against ``tests/mi_ref.py``, the float64
restatement of the rule; the restatement's gradient against finite differences of its own MI; the entry checks; the
recovery of a known transform between two volumes related by a non-monotone intensity map, end to end on CPU tensors;
and the CLI plumbing.  No upstream implementation exists: parity unpinned, these are the contract."""

import ctypes

import numpy as np
import pytest

from tests import mi_cases as cases
from tests import mi_ref as ref


def _t(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))


def _twin(mov, tgt, m, stride, bins, ranges):
    from shrimpy_amd.estimate import joint_histogram

    return joint_histogram(_t(mov), _t(tgt), m, stride, bins, ranges)


def _abs_diff(a, b):
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())


@pytest.mark.parametrize("bins", cases.BINS)
def test_twin_histogram_equals_the_restatement_where_rounding_cannot_matter(bins):
    mov, tgt = cases.exact_pair()
    for stride in cases.STRIDES:
        want, n_want = ref.joint_histogram(mov, tgt, cases.EIGHTHS, stride, bins, cases.exact_ranges(bins))
        got, n = _twin(mov, tgt, cases.EIGHTHS, stride, bins, cases.exact_ranges(bins))
        assert got.dtype == np.uint64 and got.shape == (bins, bins)
        assert n == n_want and n > 500
        assert np.array_equal(got, want), (bins, stride)
        assert int(got.sum()) == 65536 * n


@pytest.mark.parametrize("bins", cases.BINS)
def test_twin_histogram_on_general_volumes(bins):
    """The Parzen weights are continuous across bin edges: a last-bit difference in the moving value moves each of a
    sample's two weights by at most one unit -- 2 n units in all."""
    mov, tgt, m, ranges = cases.general_pair()
    for stride in cases.STRIDES:
        want, n_want = ref.joint_histogram(mov, tgt, m, stride, bins, ranges)
        got, n = _twin(mov, tgt, m, stride, bins, ranges)
        assert n == n_want and n > 500
        assert _abs_diff(got, want) <= 2 * n, (bins, stride)
        assert int(got.sum()) == 65536 * n


def test_twin_histogram_edge_cases():
    from shrimpy_amd.estimate import mutual_information

    rng = np.random.default_rng(1)
    eye = np.eye(4)
    # a target value exactly at t_hi, values outside both ranges: clamped into the edge bins
    tgt = rng.uniform(-50, 300, (6, 7, 8)).astype(np.float32)
    tgt[0, 0, 0], tgt[1, 1, 1], tgt[2, 2, 2] = 200.0, -1e6, 1e6
    mov = rng.uniform(-50, 300, (6, 7, 8)).astype(np.float32)
    ranges = ((0.0, 200.0), (10.0, 180.0))
    got, n = _twin(mov, tgt, eye, 1, 8, ranges)
    want, n_want = ref.joint_histogram(mov, tgt, eye, 1, 8, ranges)
    assert n == n_want == 5 * 6 * 7 and _abs_diff(got, want) <= 2 * n and int(got.sum()) == 65536 * n
    only = np.zeros((6, 7, 8), np.float32) + 100.0
    only[0, 0, 0] = 200.0                           # exactly t_hi -> the last bin, not one past it
    got, n = _twin(np.full((6, 7, 8), 10.0, np.float32), only, eye, 1, 8, ranges)
    assert got[7, 0] == 65536 and got[4, 0] == 65536 * (n - 1) and int(got.sum()) == 65536 * n
    # a constant moving volume: all weight in one column (u = 64 * 4 / 128 = 2 exactly)
    got, n = _twin(np.full((6, 7, 8), 64.0, np.float32), tgt, eye, 1, 5, ((0.0, 200.0), (0.0, 128.0)))
    assert int(got[:, 2].sum()) == 65536 * n and int(got.sum()) == 65536 * n
    assert mutual_information(got) == pytest.approx(0.0, abs=1e-12)
    # moving coordinates exactly 0 are counted, exactly n - 1 are not
    got, n = _twin(mov, tgt, eye, 1, 8, ranges)
    assert n == 5 * 6 * 7
    back = np.eye(4)
    back[:3, 3] = -1.0                               # coordinate = index - 1: index 0 is outside, n - 1 maps to n - 2
    assert _twin(mov, tgt, back, 1, 8, ranges)[1] == 5 * 6 * 7
    # every sample outside: n == 0, a zero histogram, no error
    far = np.eye(4)
    far[:3, 3] = 1000.0
    got, n = _twin(mov, tgt, far, 1, 8, ranges)
    assert n == 0 and not got.any()


def test_twin_histogram_does_not_depend_on_the_thread_count():
    import torch

    mov, tgt, m, ranges = cases.general_pair()
    before = torch.get_num_threads()
    try:
        torch.set_num_threads(1)
        one = _twin(mov, tgt, m, 1, 32, ranges)
        torch.set_num_threads(5)
        five = _twin(mov, tgt, m, 1, 32, ranges)
    finally:
        torch.set_num_threads(before)
    assert one[1] == five[1] and np.array_equal(one[0], five[0])


def test_mutual_information_matches_the_restatement():
    from shrimpy_amd.estimate import mutual_information

    mov, tgt, m, ranges = cases.general_pair()
    hist, _ = ref.joint_histogram(mov, tgt, m, 1, 32, ranges)
    assert mutual_information(hist) == pytest.approx(ref.mutual_information(hist), rel=1e-12)
    assert mutual_information(np.zeros((8, 8), np.uint64)) == 0.0
    # identical volumes: the MI is the entropy of the binned target, far above that of an unrelated pair
    same, _ = ref.joint_histogram(tgt, tgt, np.eye(4), 1, 32, (ranges[0], ranges[0]))
    assert ref.mutual_information(same) > 5 * ref.mutual_information(hist)


@pytest.mark.parametrize("bins,stride", [(8, 1), (32, 2), (64, (1, 2, 3))])
def test_twin_gradient_matches_the_restatement(bins, stride):
    """fp64 sums in a different order: the tolerance of the normal-equations kernel against its oracle."""
    from shrimpy_amd.estimate import mi_gradient

    mov, tgt, m, ranges = cases.general_pair()
    want = ref.gradient(mov, tgt, m, stride, bins, ranges, cases.CENTRE, cases.SCALE)
    got = mi_gradient(_t(mov), _t(tgt), m, stride, bins, ranges, None, cases.CENTRE, cases.SCALE)
    assert got.shape == (12,) and np.abs(want).max() > 0
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


def test_restatement_gradient_is_the_derivative_of_its_mutual_information():
    """Central differences (step 1e-4) of the restatement's MI with the window's weights unquantised, in the
    parameterisation the kernel uses.  The interpolant and the window are piecewise linear: a central difference is
    exact up to cell crossings.  Measured worst relative difference over the six parameters: 8.4e-5 (parameter 3), well
    inside the rel = 2e-3 of the SSD finite-difference test, which therefore stands."""
    mov, tgt, m, ranges = cases.general_pair()
    c, s = cases.CENTRE, cases.SCALE
    q0 = ref.normalised(m, c, s)

    def mi(q):
        hist, _ = ref.joint_histogram(mov, tgt, ref.from_normalised(q, c, s), 2, 32, ranges, quantised=False)
        return ref.mutual_information(hist)

    grad = ref.gradient(mov, tgt, m, 2, 32, ranges, c, s, quantised=False)
    for k in (0, 3, 5, 7, 10, 11):
        e = np.zeros(12)
        e[k] = 1e-4
        num = (mi(q0 + e) - mi(q0 - e)) / 2e-4
        print(f"parameter {k}: finite difference {num:.9e}, analytic {grad[k]:.9e}, rel {abs(num - grad[k]) / abs(grad[k]):.2e}")
        assert num == pytest.approx(grad[k], rel=2e-3)


def test_entry_checks_return_their_statuses_and_write_nothing():
    from shrimpy_amd import _lib

    lib = _lib.load()
    mov, tgt = cases.exact_pair()
    mov, tgt = np.ascontiguousarray(mov), np.ascontiguousarray(tgt)
    hist = np.full(64 * 64 + 1, 7, np.uint64)
    part = np.full((lib.lsr_affine_mi_gradient_blocks(), lib.lsr_affine_mi_gradient_size()), 7.0)
    assert part.shape[1] == 12 and part.shape[0] >= 1
    dl = np.zeros(64 * 63)
    m12 = _lib.matrix12(cases.EIGHTHS)
    c3 = (ctypes.c_double * 3)(*cases.CENTRE)
    d = ctypes.c_double

    def call(name, moving=mov.ctypes.data, target=tgt.ctypes.data, matrix=m12, stride=(1, 1, 1), bins=32, t=(0.0, 256.0),
             mr=(0.0, 256.0), out=True, count=True, centre=c3, scale=22.5, dlp=dl.ctypes.data):
        st = (ctypes.c_int * 3)(*stride) if stride is not None else None
        head = (moving, *cases.MOVING_SHAPE, target, *cases.TARGET_SHAPE, matrix, st)
        tail = () if name.endswith("_cpu") else (None,)
        if "histogram" in name:
            return getattr(lib, name)(*head, bins, d(t[0]), d(t[1]), d(mr[0]), d(mr[1]), hist.ctypes.data if out else None,
                                      hist.ctypes.data + 8 * 64 * 64 if count else None, *tail)
        return getattr(lib, name)(*head, centre, d(scale), bins, d(t[0]), d(t[1]), d(mr[0]), d(mr[1]), dlp,
                                  part.ctypes.data if out else None, *tail)

    # (the device entries check before they touch the device: safe without a GPU)
    for name in ("lsr_affine_joint_histogram_f32_cpu", "lsr_affine_mi_gradient_f32_cpu", "lsr_affine_joint_histogram_f32",
                 "lsr_affine_mi_gradient_f32"):
        assert call(name, bins=3) == -4 and b"bins" in lib.lsr_last_error()
        assert call(name, bins=65) == -4
        assert call(name, t=(5.0, 5.0)) == -4 and b"target range" in lib.lsr_last_error()
        assert call(name, mr=(9.0, 1.0)) == -4 and b"moving range" in lib.lsr_last_error()
        assert call(name, mr=(0.0, float("nan"))) == -4
        assert call(name, stride=(1, 0, 1)) == -4 and b"strides" in lib.lsr_last_error()
        assert call(name, moving=None) == -1
        assert call(name, target=None) == -1
        assert call(name, matrix=None) == -1
        assert call(name, stride=None) == -1
        assert call(name, out=False) == -1
        bad = _lib.matrix12(np.where(np.arange(12).reshape(3, 4) == 5, np.inf, cases.EIGHTHS))
        assert call(name, matrix=bad) == -4
        if "histogram" in name:
            assert call(name, count=False) == -1
        else:
            assert call(name, centre=None) == -1
            assert call(name, dlp=None) == -1
            assert call(name, scale=0.0) == -4
    assert np.all(hist == 7) and np.all(part == 7.0), "a refused call wrote something"
    # a moving volume needs two samples per axis
    st = (ctypes.c_int * 3)(1, 1, 1)
    assert lib.lsr_affine_joint_histogram_f32_cpu(mov.ctypes.data, 1, 37, 51, tgt.ctypes.data, *cases.TARGET_SHAPE, m12, st, 32,
                                                  d(0), d(1), d(0), d(1), hist.ctypes.data, hist.ctypes.data, ) == -2


def test_python_entry_refuses_what_it_cannot_run():
    import torch

    from shrimpy_amd.estimate import estimate_affine_zyx, joint_histogram, mi_gradient

    a = torch.zeros((8, 8, 8))
    with pytest.raises(ValueError, match="metric"):
        estimate_affine_zyx(a, a, metric="nmi")
    with pytest.raises(TypeError):
        joint_histogram(a.double(), a, np.eye(4), 1, 8, ((0, 1), (0, 1)))
    with pytest.raises(ValueError):
        joint_histogram(a[0], a, np.eye(4), 1, 8, ((0, 1), (0, 1)))
    with pytest.raises(ValueError, match="hist"):
        mi_gradient(a, a, np.eye(4), 1, 8, ((0, 1), (0, 1)), hist=np.ones((4, 4)))


def test_estimate_recovers_a_transform_under_a_non_monotone_intensity_map_on_the_cpu():
    """The probe's scene: beads at 24 x 40 x 48, a 3 degree tilt with 0.97 / 1.03 scales and a (0.8, -1.5, 2.2) shift,
    the target 150 sin^2(pi warp / 160) + 5.  From the identity, on CPU tensors end to end.  Conditions: worst corner
    error below 0.25 voxel (a quarter of the sampling pitch) and the restatement's MI at the estimate no lower than at
    the truth minus 1e-3 nats.  Measured: corner error 0.074 voxel, MI 1.2257 against 1.2114 at the truth.
    (``metric="ssd"`` needs a device and is recorded by the GPU test.)"""
    import torch

    from shrimpy_amd.estimate import estimate_affine_zyx

    shape = (24, 40, 48)
    mov, tgt, true = cases.recovery_pair(shape)
    est = estimate_affine_zyx(torch.as_tensor(mov), torch.as_tensor(tgt), metric="mi")
    assert est.metric == "mi" and np.isnan(est.rms) and (est.gain, est.offset) == (1.0, 0.0)
    assert est.n_samples > 0.5 * np.prod(shape) and est.converged
    ranges = ((float(tgt.min()), float(tgt.max())), (float(mov.min()), float(mov.max())))

    def mi(m):
        return ref.mutual_information(ref.joint_histogram(mov, tgt, m, 1, 32, ranges)[0])

    err = cases.corner_error(est.affine_transform_zyx, true, shape)
    at_est, at_true = mi(est.affine_transform_zyx), mi(true)
    print(f"corner error {err:.4f} voxel, MI at the estimate {at_est:.5f}, at the truth {at_true:.5f}, reported {est.mi:.5f}")
    assert err < 0.25
    assert at_est >= at_true - 1e-3
    assert est.mi == pytest.approx(at_est, abs=1e-9)     # the finest level is unblurred, stride 1, min / max ranges


def test_cli_passes_metric_and_bins_only_when_they_differ_from_the_defaults(tmp_path, monkeypatch):
    import torch

    import shrimpy_amd.cli as cli
    from click.testing import CliRunner
    from shrimpy_amd.estimate import RegistrationEstimate
    from shrimpy_amd.io.omezarr import open_ome_zarr

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    rng = np.random.default_rng(0)
    with open_ome_zarr(tmp_path / "a.zarr", layout="hcs", mode="w", channel_names=["BF", "LS"], prefer_iohub=False) as p:
        arr = p.create_position("A", "1", "0").create_zeros("0", shape=(1, 2, 6, 5, 4), dtype="uint16")
        for c in range(2):
            arr.write_volume(0, c, rng.integers(0, 900, (6, 5, 4)).astype(np.uint16))
    seen = []

    def fake(moving, target, **kwargs):
        seen.append(kwargs)
        metric = kwargs.get("metric", "ssd")
        return RegistrationEstimate(np.eye(4), 1.0, 0.0, float("nan") if metric == "mi" else 0.5, 100, 7, True,
                                    metric=metric, mi=1.25 if metric == "mi" else float("nan"))

    res = cli.run_estimate(tmp_path / "a.zarr", tmp_path / "a.zarr", tmp_path / "r0.yml", "LS", "BF", estimator=fake)
    assert seen[-1] == {"model": "affine", "intensity": True} and res["metric"] == "ssd" and "mi" not in res
    res = cli.run_estimate(tmp_path / "a.zarr", tmp_path / "a.zarr", tmp_path / "r1.yml", "LS", "BF", estimator=fake,
                           metric="mi", bins=16)
    assert seen[-1] == {"model": "affine", "intensity": True, "metric": "mi", "bins": 16}
    assert res["metric"] == "mi" and res["mi"] == 1.25 and (tmp_path / "r1.yml").exists()
    # the command line: the options reach run_estimate and the echo names the metric
    monkeypatch.setattr(cli, "run_estimate", lambda *a, **k: {"args": a[7:], **k})
    out = CliRunner().invoke(cli.cli, ["estimate-registration", "-s", str(tmp_path / "a.zarr"), "-t", str(tmp_path / "a.zarr"),
                                       "-o", str(tmp_path / "r2.yml"), "--metric", "mi", "--bins", "16"])
    assert out.exit_code == 0, (out.output, out.exception)
    assert "'metric': 'mi'" in out.output and "'bins': 16" in out.output
    out = CliRunner().invoke(cli.cli, ["estimate-registration", "-s", str(tmp_path / "a.zarr"), "-t", str(tmp_path / "a.zarr"),
                                       "-o", str(tmp_path / "r3.yml"), "--bins", "3"])
    assert out.exit_code != 0
