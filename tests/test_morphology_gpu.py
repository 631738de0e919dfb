"""The grey-morphology kernels (``csrc/morphology.hip``) on the device, through the C ABI, on every case of
``tests/morphology_cases.py`` and every op: ``scipy.ndimage`` element for element on the NaN-free cases, the restated rule and the
twin byte for byte (NaNs as a mask); every output word written and nothing behind the buffer, the input untouched, the same bytes
from two calls, one uncleared poisoned scratch buffer for every call; the Python layer, ``fill_holes``, ``segment_zyx`` on the ramp
scene and both commands.
"""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import morphology as M
from tests import morphology_cases as C
from tests import morphology_ref as R
from tests import test_morphology_host as H

pytestmark = pytest.mark.gpu

GUARD = H.GUARD
_SCRATCH = {}


def _scratch(device):
    """One poisoned scratch buffer for every call of this module, never cleared between them."""
    if device not in _SCRATCH:
        _SCRATCH[device] = torch.full((H.scratch_bytes_of_the_cases(),), 0xA5, dtype=torch.uint8, device=device)
    return _SCRATCH[device]


def device_morph(d_vol, r, op, device):
    """The kernels through the C ABI into a poisoned buffer with 64 guard words behind it: (out, guard) on the host."""
    z, y, x = d_vol.shape
    scratch = _scratch(device)
    assert 0 < _lib.call_value("lsr_grey_morph_scratch_bytes", z, y, x) <= scratch.numel()
    out = torch.full((d_vol.numel() + GUARD,), float(H.FILL), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.call("lsr_grey_morph_f32", d_vol.data_ptr(), out.data_ptr(), z, y, x, *r, C.OPS.index(op), scratch.data_ptr(),
                  _lib.stream_ptr(device))
    host = out.cpu().numpy()
    return host[:d_vol.numel()].reshape(z, y, x), host[d_vol.numel():]


@pytest.mark.parametrize("shape,r", C.PARAMS, ids=C.PARAM_IDS)
def test_kernels_equal_scipy_the_restatement_and_the_twin(shape, r, device):
    for content in C.CONTENTS:
        vol = C.volume(shape, content)
        d_vol = torch.from_numpy(np.array(vol)).to(device)
        for op in C.OPS:
            out, guard = device_morph(d_vol, r, op, device)
            H.check_buffer(out, guard)
            R.check(shape, content, r, op, out)
            assert R.same_bytes(out, H.twin_morph(vol, r, op)[0]), f"{content} {op}: device and twin disagree"
            again, _ = device_morph(d_vol, r, op, device)
            assert out.tobytes() == again.tobytes(), f"{content} {op}: two calls, two answers"
        assert d_vol.cpu().numpy().tobytes() == vol.tobytes(), "the input was written"


def test_morphology_functions_return_torch_tensors_on_the_device(device):
    shape, r = (5, 9, 13), (2, 2, 2)
    vol = torch.from_numpy(np.array(C.volume(shape, "noise"))).to(device)
    before = torch.cuda.memory_allocated(device)
    got = {op: getattr(M, op)(vol, r) for op in C.OPS}
    assert torch.cuda.memory_allocated(device) > before                  # torch's allocator owns them
    for op, t in got.items():
        assert t.device == vol.device and t.dtype == torch.float32 and t.is_contiguous() and t.shape == vol.shape
        R.check(shape, "noise", r, op, t.cpu().numpy())
    top = M.subtract_background(vol, 1.0, (0.5, 0.5, 0.5))
    assert top.cpu().numpy().tobytes() == got["white_tophat"].cpu().numpy().tobytes()


def test_fill_holes_on_the_device(device):
    H.check_fill_holes(device)


def test_segment_zyx_background_and_holes_on_the_device(device):
    H.check_segment_zyx(device)


def test_cli_segment_and_subtract_background_on_the_device(tmp_path, device):
    import shrimpy_amd.cli as cli

    H.check_commands(cli, tmp_path)
