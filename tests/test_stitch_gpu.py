"""The stitching kernel (``csrc/stitch.hip``) on the device: bit-equal with its host twin, within the a-priori bound of the
float64 rule (``tests/stitch_ref.py``), every voxel of its box written and nothing behind it.

Cases: ``stitch_ref.GPU_CASES`` -- the smallest shapes at which the kernel can go wrong: a single voxel, rows that span
workgroups (1030 > 1024 voxels per run), (2, 3, 4099) tiles at x translations 0 .. 3 and 2.5 (every 4-byte phase of a 16-byte
line, so every load and store width, with four and with five floats per read), negative translations, translations fractional on x, y, z and all three, five tiles on one
voxel, a tile inside another, a tile outside the box, a strict sub-box, p in {0, 1, 4}.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import stitch as S
from tests import stitch_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64


def _device_call(tiles, tr, p, cval, box, device, fill=float("nan")):
    """The kernel through the C ABI into a ``fill``-ed buffer with GUARD more elements behind the box: (box, guard)."""
    shapes = [t.shape for t in tiles]
    if box is None:
        shape, origin = S.canvas_geometry(shapes, tr)
    else:
        origin, shape = box
    n = int(np.prod(shape))
    d_tiles = [torch.from_numpy(np.array(t)).to(device) for t in tiles]
    table = torch.from_numpy(S._host_table(d_tiles, tr)).to(device)
    buf = torch.full((n + GUARD,), fill, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.call("lsr_stitch_f32", table.data_ptr(), len(tiles), buf.data_ptr(), (ctypes.c_int64 * 3)(*origin),
                  (ctypes.c_int64 * 3)(*shape), int(p), float(cval), _lib.stream_ptr(device))
    host = buf.cpu().numpy()
    return host[:n].reshape(shape), host[n:]


@pytest.mark.parametrize("index", range(len(R.GPU_CASES)), ids=[c["name"] for c in R.GPU_CASES])
def test_kernel_equals_its_twin_and_meets_the_bound(index, device):
    case = R.GPU_CASES[index]
    tiles, tr, twin = R.twin_case(index)
    got, guard = _device_call(tiles, tr, case["p"], case["cval"], case["box"], device)
    assert np.isnan(guard).all(), "the kernel wrote behind its output"
    assert not np.isnan(got).any(), "an output voxel was not written"
    assert np.array_equal(got.view(np.uint32), twin.view(np.uint32)), "device and host twin differ"
    ref, bound, n_cover = R.stitch_f64(tiles, tr, case["p"], case["cval"], case["box"])
    assert np.all(got[n_cover == 0] == np.float32(case["cval"])), "an uncovered voxel is not cval"
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))
    print(f"{case['name']}: worst |got - ref| / bound = {ratio:.3f}")
    assert np.all(err <= bound)


def test_zeros_stay_zeros_and_a_nan_stays_under_its_tile(device):
    shapes, tr = [(2, 6, 1030), (2, 6, 1030)], [(0, 0, 0), (0, 2.5, 500)]
    zeros = [np.zeros(s, dtype=np.float32) for s in shapes]
    got, _ = _device_call(zeros, tr, 1, 3.0, None, device)
    n_cover = R.stitch_f64(zeros, tr, 1, 3.0)[2]
    assert np.array_equal(got[n_cover > 0].view(np.uint32), np.zeros(int((n_cover > 0).sum()), dtype=np.uint32))
    assert np.all(got[n_cover == 0] == np.float32(3.0))
    tiles = [R.f32_tile(s, 9 + k) for k, s in enumerate(shapes)]
    tiles[1][1, 3, 600] = np.nan
    got, _ = _device_call(tiles, tr, 1, 0.0, None, device, fill=0.0)
    want = np.zeros(got.shape, dtype=bool)
    want[1, 5:7, 1100] = True                  # the taps j - 1 and j along y
    assert np.array_equal(np.isnan(got), want)


def test_banded_equals_one_launch_and_the_result_is_a_torch_tensor_on_the_device(device):
    index = [c["name"] for c in R.GPU_CASES].index("frac_zyx")
    case = R.GPU_CASES[index]
    tiles, tr, twin = R.twin_case(index)
    d_tiles = [torch.from_numpy(np.array(t)).to(device) for t in tiles]
    before = torch.cuda.memory_allocated(device)
    whole = S.stitch_tiles(d_tiles, tr, case["p"], case["cval"])
    assert whole.device == d_tiles[0].device and whole.dtype == torch.float32 and whole.is_contiguous()
    assert torch.cuda.memory_allocated(device) > before            # torch's allocator owns it
    assert np.array_equal(whole.cpu().numpy().view(np.uint32), twin.view(np.uint32))
    for rows in (1, 3):
        got = S.stitch_banded(lambda k: d_tiles[k], [t.shape for t in tiles], tr, case["p"], case["cval"], band_rows=rows)
        assert torch.equal(got.view(torch.int32), whole.view(torch.int32)), f"bands of {rows} rows"


def test_estimate_translations_on_the_device_gives_the_host_integers(device):
    names, tiles, nominal, true = R.grid(2, 2)
    got = S.estimate_translations({n: torch.from_numpy(tiles[n]).to(device) for n in names}, {n: tiles[n].shape for n in names},
                                  nominal, R.ESTIMATE)
    for n in names:
        rel = tuple(a - b for a, b in zip(got[n], got[names[0]]))
        assert rel == tuple(float(a - b) for a, b in zip(true[n], true[names[0]])), n
