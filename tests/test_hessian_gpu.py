"""The Hessian-eigenvalue kernel (``csrc/hessian.hip``) on the device, through the C ABI, on every case of
``tests/hessian_cases.py``: the twin byte for byte under every measure, ``dark``, ``accumulate`` and sampling, the eigenvalue
bound asserted on the device's own outputs, every output word written and nothing behind the buffer, the input untouched;
refused arguments, a stream of its own, the Python layer, the structure scene and ``segment_zyx``.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import hessian as K
from tests import hessian_cases as C
from tests import hessian_ref as R
from tests import test_hessian_host as H

pytestmark = pytest.mark.gpu

GUARD = H.GUARD


def device_response(d_vol, sampling, scale, measure, dark, device, stored=None, stream=None):
    """The kernel through the C ABI into a poisoned buffer (or ``stored``, accumulating) with 64 guard words behind it:
    (out, guard) on the host."""
    z, y, x = d_vol.shape
    out = torch.full((d_vol.numel() + GUARD,), float(H.FILL), dtype=torch.float32, device=device)
    if stored is not None:
        out[:d_vol.numel()] = stored.reshape(-1)
    with torch.cuda.device(device):
        _lib.call("lsr_hessian_response_f32", d_vol.data_ptr(), out.data_ptr(), z, y, x, *(ctypes.c_double(s) for s in sampling),
                  ctypes.c_double(scale), int(measure), int(dark), int(stored is not None),
                  _lib.stream_ptr(device) if stream is None else stream)
    host = out.cpu().numpy()
    return host[:d_vol.numel()].reshape(z, y, x), host[d_vol.numel():]


def stored_volume(shape):
    """What the accumulating calls find in ``out``: noise with NaNs and zeros of both signs (read-only)."""
    rng = np.random.default_rng(17)
    stored = rng.normal(size=shape).astype(np.float32)
    stored[rng.random(size=shape) < 0.05] = np.nan
    stored[rng.random(size=shape) < 0.2] = -0.0
    stored[rng.random(size=shape) < 0.2] = 0.0
    return stored


@pytest.mark.parametrize("shape,sampling", C.PARAMS, ids=C.PARAM_IDS)
def test_kernel_equals_the_twin_and_keeps_the_bound(shape, sampling, device):
    stored = stored_volume(shape)
    d_stored = torch.from_numpy(stored).to(device)
    for content in C.CONTENTS:
        vol = C.case_volume(shape, content, sampling)
        d_vol = torch.from_numpy(np.array(vol)).to(device)
        for dark in (False, True):
            e = []
            for measure in range(8):
                out, guard = device_response(d_vol, sampling, C.SCALE, measure, dark, device)
                H.check_buffer(out, guard)
                twin = H.case_twin(shape, content, sampling, measure, dark)
                assert out.tobytes() == twin.tobytes(), f"{content} {R.MEASURES[measure]} dark {dark}: device and twin disagree"
                e.append(out)
                acc, guard = device_response(d_vol, sampling, C.SCALE, measure, dark, device, stored=d_stored)
                H.check_buffer(acc, guard)
                assert acc.tobytes() == R.accumulate(stored, twin).tobytes(), f"{content} {R.MEASURES[measure]} dark {dark}: accumulate"
            H.check_eigenvalues(shape, content, sampling, dark, e[:3])
        assert d_vol.cpu().numpy().tobytes() == vol.tobytes(), "the input was written"


def test_refused_arguments_leave_out_untouched(device):
    vol = torch.arange(24, dtype=torch.float32, device=device).reshape(2, 3, 4)
    out = torch.full((24,), float(H.FILL), dtype=torch.float32, device=device)
    lib = _lib.load()
    d = ctypes.c_double
    v, o, st = vol.data_ptr(), out.data_ptr(), _lib.stream_ptr(device)
    one = (d(1.0), d(1.0), d(1.0))
    with torch.cuda.device(device):
        fn = lib.lsr_hessian_response_f32
        assert fn(None, o, 2, 3, 4, *one, d(1.0), 0, 0, 0, st) == -1 and fn(v, None, 2, 3, 4, *one, d(1.0), 0, 0, 0, st) == -1
        assert fn(v, v, 2, 3, 4, *one, d(1.0), 0, 0, 0, st) == -4
        assert fn(v, o, 2, 0, 4, *one, d(1.0), 0, 0, 0, st) == -2
        assert fn(v, o, 2048, 1024, 1024, *one, d(1.0), 0, 0, 0, st) == -3
        assert fn(v, o, 2, 3, 4, d(0.0), d(1.0), d(1.0), d(1.0), 0, 0, 0, st) == -4
        assert fn(v, o, 2, 3, 4, *one, d(float("nan")), 0, 0, 0, st) == -4
        assert fn(v, o, 2, 3, 4, *one, d(1.0), 8, 0, 0, st) == -4 and fn(v, o, 2, 3, 4, *one, d(1.0), 0, 2, 0, st) == -4
        assert fn(v, o, 2, 3, 4, *one, d(1.0), 0, 0, 2, st) == -4
    torch.cuda.synchronize(device)
    assert torch.all(out == float(H.FILL)) and torch.equal(vol.cpu().reshape(-1), torch.arange(24, dtype=torch.float32))


def test_a_stream_of_its_own(device):
    shape, sampling = (C.TZ + 1, C.TY + 1, C.TX + 1), C.SAMPLINGS[2]
    d_vol = torch.from_numpy(np.array(C.volume(shape, "noise"))).to(device)
    torch.cuda.synchronize(device)
    stream = torch.cuda.Stream(device)
    with torch.cuda.stream(stream):
        out, guard = device_response(d_vol, sampling, C.SCALE, 4, False, device, stream=stream.cuda_stream)
    H.check_buffer(out, guard)
    assert out.tobytes() == H.case_twin(shape, "noise", sampling, 4, False).tobytes()


def test_python_layer_on_the_device(device):
    before = torch.cuda.memory_allocated(device)
    H.check_python_layer(device)
    assert torch.cuda.memory_allocated(device) >= before
    got = K.enhance(torch.from_numpy(np.array(C.volume(C.LARGEST, "beads"))).to(device), "tube", (1.0, 1.5), (2.0, 0.5, 0.5))
    assert got.device.type == "cuda" and got.dtype == torch.float32 and float(got.max()) > 0


def test_structures_on_the_device(device):
    H.check_structures(device)


def test_segment_zyx_enhance_on_the_device(device):
    H.check_segment_zyx(device)
