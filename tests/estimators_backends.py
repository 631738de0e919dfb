"""What the host suite (``test_estimators_host.py``) and the device suite (``test_estimators_fp64_gpu.py``) share besides
``tests/estimators_ref.py``: the host twins (``lsr_*_cpu``) as an ``estimators_ref`` backend, and the blur dispatch query
for a case of the table.
"""

import ctypes

import numpy as np

from shrimpy_amd import _lib


def _f(v):
    return ctypes.c_float(float(v))


def _view(x, offset):
    """A copy of ``x`` that starts ``offset`` elements behind a 16-byte aligned address."""
    x = np.ascontiguousarray(x)
    pad = 16 // x.dtype.itemsize
    buf = np.empty(x.size + offset + pad, x.dtype)
    start = (-buf.ctypes.data // x.dtype.itemsize) % pad + offset
    out = buf[start:start + x.size].reshape(x.shape)
    out[...] = x
    assert out.ctypes.data % 16 == (offset * x.dtype.itemsize) % 16
    return out


class Twin:
    """The ``lsr_*_cpu`` entries as an ``estimators_ref`` backend."""

    def minmax_f32(self, x, offset):
        x, out = _view(x, offset), np.full(2, np.nan, np.float32)
        _lib.call("lsr_minmax_f32_cpu", x.ctypes.data, x.size, out.ctypes.data, None, None)
        return out

    minmax_u16 = None

    def histogram(self, x, offset, vmin, vmax, nbins):
        x, out = _view(x, offset), np.full(nbins, 0xFFFFFFFF, np.uint32)
        _lib.call("lsr_histogram_f32_cpu", x.ctypes.data, x.size, _f(vmin), _f(vmax), int(nbins), out.ctypes.data, None)
        return out

    def centroid(self, kind, vol, param):
        vol, out = np.ascontiguousarray(vol), np.full(4, np.nan)
        _lib.call(f"lsr_{kind}_centroid_f32_cpu", vol.ctypes.data, *vol.shape, _f(param), out.ctypes.data, None, None)
        return out

    def blur(self, vol, axis, taps, r, sub, div, offset, out_offset=0):
        src, out = _view(vol, offset), _view(np.full(vol.shape, np.nan, np.float32), out_offset)
        taps = np.ascontiguousarray(taps, np.float32)
        _lib.call("lsr_blur_reflect_f32_cpu", src.ctypes.data, out.ctypes.data, *vol.shape, int(axis), taps.ctypes.data, int(r),
                  _f(sub), _f(div), None)
        return out

    def match(self, vol, shape):
        vol, out = np.ascontiguousarray(vol), np.full(shape, np.nan, np.float32)
        _lib.call("lsr_match_shape_f32_cpu", vol.ctypes.data, *vol.shape, out.ctypes.data, *shape, None)
        return out

    def cross(self, a, b, into_b):
        a, b = a.copy(), b.copy()
        _lib.call("lsr_cross_power_into_c64_cpu" if into_b else "lsr_cross_power_c64_cpu", a.ctypes.data, b.ctypes.data, a.size,
                  None)
        return a, b

    def peak(self, vol, offset):
        src, out = _view(vol, offset), np.full(1, -7, np.int64)
        _lib.call("lsr_peak_abs_shifted_f32_cpu", src.ctypes.data, *vol.shape, out.ctypes.data, None, None)
        return int(out[0])


def form_of(case) -> int:
    """``lsr_blur_reflect_form`` for a case: input and output ``offset`` / ``out_offset`` floats off a 16-byte boundary."""
    return _lib.call_value("lsr_blur_reflect_form", *case["shape"], case["axis"], case["r"], (4 * case["offset"]) % 16,
                           (4 * case["out_offset"]) % 16)
