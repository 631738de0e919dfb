"""The DynaTrack estimator kernels (``csrc/estimators.hip``) on the device, entry by entry through the C ABI, against the
float64 / exact restatements and case tables of ``tests/estimators_ref.py`` -- the assertions ``test_estimators_host.py``
makes of the host twins -- and, for every entry documented as such (all but the centroid sums), bit for bit against its
twin.  Every output sits in front of guard elements pre-filled with NaN that must stay NaN, in a buffer pre-filled with
NaN whose every element must have been written.
"""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from tests import estimators_ref as R
from tests.estimators_backends import Twin, _f, form_of

pytestmark = pytest.mark.gpu

GUARD = 64


class Device:
    """The kernels as an ``estimators_ref`` backend; each call also runs the twin and compares where they must agree."""

    def __init__(self, device):
        self.device = device
        self.twin = Twin()
        self.scratch = torch.empty((_lib.call_value("lsr_reduce_scratch_bytes"),), dtype=torch.uint8, device=device)

    def _up(self, x, offset=0):
        """``x`` on the device, ``offset`` elements behind a 16-byte aligned address."""
        t = torch.from_numpy(np.array(x).reshape(-1))        # (a copy: the cached case arrays are read-only)
        buf = torch.empty((t.numel() + offset,), dtype=t.dtype, device=self.device)
        view = buf[offset:]
        view.copy_(t)
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (offset * t.element_size()) % 16
        return view

    def _out(self, n, dtype=torch.float32, offset=0):
        """NaN everywhere: ``offset`` elements, the n the kernel is to write, the guard."""
        buf = torch.full((offset + n + GUARD,), float("nan"), dtype=dtype, device=self.device)
        assert buf.data_ptr() % 16 == 0
        return buf

    def _call(self, entry, *args):
        with torch.cuda.device(self.device):
            _lib.call(entry, *args, _lib.stream_ptr(self.device))

    @staticmethod
    def _take(buf, n, what, offset=0):
        """The n elements of an output buffer behind ``offset`` after the guard and written-everywhere checks."""
        host = buf.cpu().numpy()
        raw = host.view(np.uint32).reshape(host.size, -1)
        nan_bits = np.full(1, np.nan, host.dtype).view(np.uint32)      # what the buffer held before the call
        assert (raw[:offset] == nan_bits).all() and (raw[offset + n:] == nan_bits).all(), f"{what}: the kernel wrote outside its output"
        assert not (raw[offset:offset + n] == nan_bits).all(axis=1).any(), f"{what}: an output element was not written"
        return host[offset:offset + n]

    def minmax_f32(self, x, offset):
        src, out = self._up(x, offset), self._out(2)
        self._call("lsr_minmax_f32", src.data_ptr(), src.numel(), out.data_ptr(), self.scratch.data_ptr())
        got = self._take(out, 2, "lsr_minmax_f32").copy()
        assert np.array_equal(got.view(np.uint32), self.twin.minmax_f32(x, offset).view(np.uint32)), "device and twin differ"
        return got

    def minmax_u16(self, x, offset):
        src, out = self._up(x.view(np.int16), offset), self._out(2)
        self._call("lsr_minmax_u16", src.data_ptr(), src.numel(), out.data_ptr(), self.scratch.data_ptr())
        return self._take(out, 2, "lsr_minmax_u16").copy()

    def histogram(self, x, offset, vmin, vmax, nbins):
        src, out = self._up(x, offset), self._out(nbins)
        self._call("lsr_histogram_f32", src.data_ptr(), src.numel(), _f(vmin), _f(vmax), int(nbins), out.data_ptr())
        got = self._take(out, nbins, "lsr_histogram_f32").view(np.uint32).copy()
        assert np.array_equal(got, self.twin.histogram(x, offset, vmin, vmax, nbins)), "device and twin differ"
        return got

    def centroid(self, kind, vol, param):
        src, out = self._up(vol), self._out(4, torch.float64)
        self._call(f"lsr_{kind}_centroid_f32", src.data_ptr(), *vol.shape, _f(param), out.data_ptr(), self.scratch.data_ptr())
        return self._take(out, 4, f"lsr_{kind}_centroid_f32").copy()

    def blur(self, vol, axis, taps, r, sub, div, offset, out_offset=0):
        src, t = self._up(vol, offset), self._up(np.asarray(taps, np.float32))
        out = self._out(vol.size, offset=out_offset)
        self._call("lsr_blur_reflect_f32", src.data_ptr(), out[out_offset:].data_ptr(), *vol.shape, int(axis), t.data_ptr(), int(r),
                   _f(sub), _f(div))
        got = self._take(out, vol.size, "lsr_blur_reflect_f32", out_offset).reshape(vol.shape).copy()
        twin = self.twin.blur(vol, axis, taps, r, sub, div, offset, out_offset)
        assert np.array_equal(got.view(np.uint32), twin.view(np.uint32)), "device and twin differ"
        return got

    def match(self, vol, shape):
        n = int(np.prod(shape))
        src, out = self._up(vol), self._out(n)
        self._call("lsr_match_shape_f32", src.data_ptr(), *vol.shape, out.data_ptr(), *shape)
        got = self._take(out, n, "lsr_match_shape_f32").reshape(shape).copy()
        assert np.array_equal(got.view(np.uint32), self.twin.match(vol, shape).view(np.uint32)), "device and twin differ"
        return got

    def cross(self, a, b, into_b):
        n = a.size
        bufs = [self._out(2 * n), self._out(2 * n)]
        for buf, v in zip(bufs, (a, b)):
            buf[:2 * n].copy_(torch.from_numpy(np.ascontiguousarray(v).view(np.float32)))
        self._call("lsr_cross_power_into_c64" if into_b else "lsr_cross_power_c64", bufs[0].data_ptr(), bufs[1].data_ptr(), n)
        got = [self._take(buf, 2 * n, "cross power").copy().view(np.complex64) for buf in bufs]
        for g, t in zip(got, self.twin.cross(a, b, into_b)):
            assert np.array_equal(g.view(np.uint32), t.view(np.uint32)), "device and twin differ"
        return got

    def peak(self, vol, offset):
        src, out = self._up(vol, offset), self._out(1, torch.float64)
        self._call("lsr_peak_abs_shifted_f32", src.data_ptr(), *vol.shape, out.data_ptr(), self.scratch.data_ptr())
        got = int(self._take(out, 1, "lsr_peak_abs_shifted_f32").view(np.int64)[0])
        assert got == self.twin.peak(vol, offset), "device and twin differ"
        return got


@pytest.fixture(scope="module")
def dev(device):
    return Device(device)


@pytest.mark.parametrize("n", R.FLAT_N)
def test_minmax_f32(dev, n):
    for offset in R.FLAT_OFFSETS:
        R.check_minmax_f32(dev, n, offset)


@pytest.mark.parametrize("n", R.U16_N)
def test_minmax_u16(dev, n):
    for offset in R.U16_OFFSETS:
        R.check_minmax_u16(dev, n, offset)


@pytest.mark.parametrize("n", R.FLAT_N)
def test_histogram(dev, n):
    for nbins in R.HIST_BINS:
        for offset in R.FLAT_OFFSETS:
            R.check_histogram(dev, n, offset, nbins)


def test_histogram_rules(dev):
    R.check_histogram_rules(dev)


@pytest.mark.parametrize("kind", R.CENTROID_KINDS)
@pytest.mark.parametrize("shape", R.CENTROID_SHAPES, ids=str)
def test_centroid_sums(dev, shape, kind):
    print(f"{kind} {shape}: worst |got - fsum| / (N 2^-53 fsum) = {R.check_centroid(dev, shape, kind):.3g}")


@pytest.mark.parametrize("form", R.FORMS)
def test_blur(dev, form):
    cases = [c for c in R.BLUR_CASES if c["form"] == form]
    assert cases and all(R.FORMS[form_of(c)] == form for c in cases)
    worst = max(R.check_blur(dev, c) for c in cases)
    print(f"{form}: {len(cases)} cases, worst |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("si,so", R.MATCH_CASES, ids=str)
def test_match_shape(dev, si, so):
    R.check_match(dev, si, so)


@pytest.mark.parametrize("into_b", (False, True))
@pytest.mark.parametrize("n", R.CROSS_N)
def test_cross_power(dev, n, into_b):
    print(f"n={n} into_b={into_b}: worst error / bound = {R.check_cross(dev, n, into_b):.3f}")


@pytest.mark.parametrize("shape", R.PEAK_SHAPES, ids=str)
def test_peak(dev, shape):
    R.check_peak(dev, shape)


def test_a_volume_without_a_finite_sample(dev):
    """All NaN: kernel and twin both answer index ~0 (-1) and the range (+inf, -inf); what ``shrimpy_amd.dynatrack`` makes
    of them is pinned on CPU tensors in ``test_estimators_host.py``."""
    nan = np.full((3, 4, 8), np.nan, np.float32)
    for offset in (0, 1):                      # the vector and the scalar form of the peak search
        assert dev.peak(nan, offset) == -1
        got = dev.minmax_f32(nan, offset)
        assert got[0] == np.inf and got[1] == -np.inf
