"""The band-power kernels (``csrc/focus.hip``) against the float64 model ``tests/focus_ref.py`` on the device.

Bound, per plane, from the constants the LDS transforms carry in ``tests/test_fft_kernels_fp64_gpu.py`` -- per coefficient
``max|err| <= 32 u log2(n) rms(ref)`` per leg, ``rms(F) = sqrt(Yc Xc) rms(v)`` by Parseval --

    |P_got - P_ref| <= 32 u (log2 Xc + log2 Yc) W sqrt(Yc Xc) rms(v),     u = 2^-24,

``W`` the weighted number of band bins, ``rms(v)`` of the windowed plane: of the order of 1e-4 of ``P``, thousands of times
below the 0.36 gap that decides the argmax, while a wrong twiddle, pairing, weight or interval exceeds it.

Worst observed |P_got - P_ref| / bound on an MI355X: 8.2e-4 (the band that reaches column Xc / 2; the others 8.6e-5 .. 5.9e-4) (the constant is not tightened to it).
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import focus as F
from tests import focus_ref as R

pytestmark = pytest.mark.gpu

ALL = [(f"case{i}", c, {}) for i, c in enumerate(R.CASES)] + [(n, a, kw) for n, (a, kw) in R.extra_cases().items()]
IDS = [a[0] for a in ALL]


@pytest.fixture(scope="module")
def data():
    out = {}
    for name, args, kw in ALL:
        vol = R.stack(*args)
        out[name] = (vol, kw, R.power(vol, **R.OPTICS, **kw), R.bound(vol, **R.OPTICS, **kw))
    return out


def _raw_call(vol, kw, dev):
    """lsr_band_power_f32 with NaN-filled output and scratch buffers: (power, spec, partial)."""
    z, y, x = vol.shape
    yc, xc, y0, x0 = F.focus_grid(vol.shape, kw.get("center_crop_xy", (800, 800)))
    lo, hi = F.band_limits(R.OPTICS["NA_det"], R.OPTICS["lambda_ill"], kw.get("midband_fractions", R.FRACTIONS))
    table, k_hi, _ = F.band_table(yc, xc, R.OPTICS["pixel_size"], lo, hi)
    sb, pb = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.call("lsr_band_power_scratch_bytes", z, yc, k_hi, ctypes.byref(sb), ctypes.byref(pb))
    spec = torch.full((sb.value // 4,), float("nan"), dtype=torch.float32, device=dev)
    partial = torch.full((pb.value // 8,), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full((z,), float("nan"), dtype=torch.float64, device=dev)
    half, full = F._row_twiddles(xc, dev)
    tw_y = F._column_twiddles(yc, dev)
    tab = torch.as_tensor(np.ascontiguousarray(table[:k_hi + 1]), device=dev)
    v = torch.as_tensor(vol, device=dev)
    _lib.call("lsr_band_power_f32", v.data_ptr(), z, y, x, y0, x0, yc, xc, half.data_ptr(), full.data_ptr(), tw_y.data_ptr(),
              tab.data_ptr(), k_hi, spec.data_ptr(), partial.data_ptr(), out.data_ptr(), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy(), spec, partial


@pytest.mark.parametrize("name", IDS)
def test_kernel_against_the_model(name, data):
    vol, kw, ref, bound = data[name]
    # the index comparison below is only worth something if the bound is far below what decides the argmax
    top = np.sort(ref)[::-1]
    assert top[0] - top[1] >= 100 * bound.max()
    got, spec, partial = _raw_call(vol, kw, torch.device("cuda:0"))
    assert not torch.isnan(partial).any() and not torch.isnan(spec).any()
    ratio = np.abs(got - ref) / bound
    print(f"{name}: worst |P - P_ref| / bound = {ratio.max():.3g}")
    assert np.all(np.isfinite(got)) and np.all(ratio <= 1.0)
    again, _, _ = _raw_call(vol, kw, torch.device("cuda:0"))
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))          # the same bits on every call
    public = F.midband_power(torch.as_tensor(vol, device="cuda:0"), **R.OPTICS, **kw)
    assert public.device.type == "cuda" and np.array_equal(public.cpu().numpy().view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("name", IDS)
def test_kernel_and_twin_agree_on_the_index(name, data):
    vol, kw, ref, _ = data[name]
    dev = F.focus_from_transverse_band(torch.as_tensor(vol, device="cuda:0"), **R.OPTICS, **kw)
    host = F.focus_from_transverse_band(torch.from_numpy(vol), **R.OPTICS, **kw)
    assert dev == host == int(np.argmax(ref))


def _rule(yc, xc):
    def smooth(n):
        for f in (2, 3, 5):
            while n % f == 0:
                n //= f
        return n == 1
    return int(2 <= yc <= 2048 and smooth(yc) and xc >= 8 and xc % 4 == 0 and xc // 2 <= 2048 and smooth(xc // 2))


def test_supported_follows_the_documented_rule():
    for yc in list(range(0, 70)) + [800, 1024, 2000, 2048, 2049, 2160, 2187, 2250, 4096]:
        for xc in list(range(0, 70)) + [800, 2270, 2304, 4096, 4100, 4104, 8192]:
            assert _lib.call_value("lsr_band_power_supported", yc, xc) == _rule(yc, xc), (yc, xc)


def test_unsupported_length_is_refused_before_any_launch():
    dev = torch.device("cuda:0")
    vol = torch.zeros((2, 14, 16), dtype=torch.float32, device=dev)           # Yc = 14 = 2 * 7
    out = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    buf = torch.zeros((4096,), dtype=torch.float64, device=dev)
    tab = torch.zeros((9, 2), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.LsrUnsupported) as err:
        _lib.call("lsr_band_power_f32", vol.data_ptr(), 2, 14, 16, 0, 0, 14, 16, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                  tab.data_ptr(), 3, buf.data_ptr(), buf.data_ptr(), out.data_ptr(), _lib.stream_ptr(dev))
    assert err.value.code == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
