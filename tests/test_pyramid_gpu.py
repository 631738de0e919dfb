"""The downsampling kernel (``csrc/pyramid.hip``) on the device: bit-equal with its host twin, within the a-priori bound of
the float64 oracle (``tests/pyramid_ref.py``), nothing written outside its output -- and ``--levels`` end to end.

Shapes: ``pyramid_ref.GPU_SHAPES`` -- the host cases (single voxels, odd and even extents, rows shorter and longer than
one lane's eight inputs) plus (3, 5, 1030), whose rows of 129 pieces straddle workgroups, and (2, 3, 4099), whose odd X
puts the row starts on every 4-byte phase of a 16-byte line (uint16: every 2-byte phase), so each load width is taken.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import pyramid as P
from tests import pyramid_ref as R

pytestmark = pytest.mark.gpu

CASES = [(s, fz) for s in R.GPU_SHAPES for fz in R.FZ]
GUARD = 64


@functools.lru_cache(maxsize=None)
def _case(shape, fz, kind):
    """(input, host twin's output) of a case, computed once."""
    vol = (R.f32_volume if kind == "f32" else R.u16_volume)(shape, seed=sum(shape) + fz)
    twin = P.downsample2(torch.from_numpy(vol), fz).numpy()
    vol.setflags(write=False)
    twin.setflags(write=False)
    return vol, twin


def _device_call(vol: np.ndarray, fz: int, device, fill):
    """The kernel through the C ABI into a `fill`-ed buffer with GUARD more elements behind the output: (output, guard)."""
    name = {"float32": "lsr_downsample2_f32", "uint16": "lsr_downsample2_u16"}[vol.dtype.name]
    shape = R.out_shape(vol.shape, fz)
    n = int(np.prod(shape))
    d_in = torch.from_numpy(np.array(vol)).to(device)
    buf = torch.full((n + GUARD,), fill, dtype=d_in.dtype, device=device)
    with torch.cuda.device(device):
        _lib.call(name, d_in.data_ptr(), *vol.shape, buf.data_ptr(), fz, _lib.stream_ptr(device))
    host = buf.cpu().numpy()
    return host[:n].reshape(shape), host[n:]


@pytest.mark.parametrize("shape,fz", CASES)
def test_float32_kernel_equals_its_twin_and_meets_the_bound(shape, fz, device):
    vol, twin = _case(shape, fz, "f32")
    got, guard = _device_call(vol, fz, device, float("nan"))
    assert np.isnan(guard).all(), "the kernel wrote behind its output"
    assert not np.isnan(got).any(), "an output voxel was not written"
    assert np.array_equal(got.view(np.uint32), twin.view(np.uint32)), "device and host twin differ"
    err = np.abs(got.astype(np.float64) - R.downsample2_f64(vol, fz))
    bound = R.bound_f32(vol, fz)
    print(f"{shape} fz={fz}: worst |got - ref| / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("shape,fz", CASES)
def test_uint16_kernel_equals_its_twin_and_the_integer_formula(shape, fz, device):
    vol, twin = _case(shape, fz, "u16")
    got, guard = _device_call(vol, fz, device, 12345)
    assert np.all(guard == 12345), "the kernel wrote behind its output"
    assert np.array_equal(got, twin)
    assert np.array_equal(got, R.downsample2_u16(vol, fz))


@pytest.mark.parametrize("fz", R.FZ)
def test_zeros_stay_zeros_and_a_nan_stays_in_its_window(fz, device):
    shape = (3, 5, 1030)
    zeros = np.zeros(shape, dtype=np.float32)
    got, _ = _device_call(zeros, fz, device, float("nan"))
    assert np.array_equal(got.view(np.uint32), np.zeros(got.shape, dtype=np.uint32))
    vol = np.array(_case(shape, fz, "f32")[0])
    for at in ((1, 2, 515), (2, 4, 1029)):              # a full window in the second workgroup's part; the far corner
        vol[at] = np.nan
    got, _ = _device_call(vol, fz, device, 0.0)
    want = np.zeros(got.shape, dtype=bool)
    for at in ((1, 2, 515), (2, 4, 1029)):
        want[at[0] // fz, at[1] // 2, at[2] // 2] = True
    assert np.array_equal(np.isnan(got), want)


def test_avg_pool3d_agrees(device):
    """An independent second opinion: torch's partial-window mean (ceil_mode, count_include_pad=False)."""
    vol = torch.from_numpy(np.array(_case((7, 33, 67), 2, "f32")[0])).to(device)
    for fz in R.FZ:
        got = P.downsample2(vol, fz)
        ref = torch.nn.functional.avg_pool3d(vol[None, None], (fz, 2, 2), ceil_mode=True, count_include_pad=False)[0, 0]
        assert got.shape == ref.shape
        worst = float((got - ref).abs().max())
        print(f"fz={fz}: max |kernel - avg_pool3d| = {worst:.3e}")
        assert worst <= 4 * R.U * float(vol.abs().max())


def test_build_levels_returns_torch_tensors_on_the_device(device):
    vol = torch.from_numpy(np.array(_case((7, 33, 67), 2, "f32")[0])).to(device)
    before = torch.cuda.memory_allocated(device)
    levels = P.build_levels(vol, 3)
    assert [tuple(lv.shape) for lv in levels] == [(4, 17, 34), (2, 9, 17)]
    assert all(lv.device == vol.device and lv.dtype == torch.float32 and lv.is_contiguous() for lv in levels)
    assert torch.cuda.memory_allocated(device) > before            # torch's allocator owns them
    assert torch.equal(levels[1], P.downsample2(P.downsample2(vol)))
    host = P.build_levels(vol.cpu(), 3)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(levels, host))
    u = torch.from_numpy(np.array(_case((7, 33, 67), 2, "u16")[0])).to(device)
    lv = P.build_levels(u, 2, 1)[0]
    assert lv.dtype == torch.uint16 and tuple(lv.shape) == (7, 17, 34)


@pytest.mark.parametrize("compression", ["blosc-zstd", "none"])
def test_deskew_with_three_levels_end_to_end(tmp_path, compression):
    """Four units on one device: the staged route (``len(todo) > world``), level 0 in device-written frames where the output
    is blosc-zstd; every level read back is the twin's 2x mean of the level above it."""
    from shrimpy_amd import cli
    from shrimpy_amd.settings import DeskewSettings, ReconstructSettings
    from tests.test_pyramid_host import KEYS, check_cascade, make_raw_plate, read_levels

    src = make_raw_plate(tmp_path / "raw.zarr")
    settings = ReconstructSettings(deskew=DeskewSettings(pixel_size_um=0.1133, scan_step_um=0.15, ls_angle_deg=30.0,
                                                         keep_overhang=True, average_n_slices=3))
    res = cli.run_store(src, tmp_path / "out.zarr", settings, zarr_version="0.5", compression=compression, levels=3)
    assert res["units"] == res["units_total"] == 4 and not res["failed"]
    assert res["device_codec"]["encode"] == (compression == "blosc-zstd")
    data, attrs = read_levels(tmp_path / "out.zarr")
    check_cascade(data, attrs, 3, 2)
    assert np.abs(data[KEYS[1]][2][1]).max() > 0
    # level 0 is what the run without a pyramid writes
    plain = cli.run_store(src, tmp_path / "plain.zarr", settings, zarr_version="0.5", compression=compression)
    assert plain["units"] == 4
    ref, _ = read_levels(tmp_path / "plain.zarr")
    for key in KEYS:
        for a, b in zip(data[key][0], ref[key][0]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
