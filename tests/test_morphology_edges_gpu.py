"""The sliding-window kernels at their dispatch edges, on the device and through the C ABI: every case of
``tests/morphology_edge_cases.py``.  ``lsr_grey_morph_f32`` against ``scipy.ndimage`` element for element, the restated rule and
the twin byte for byte (NaNs as a mask); every output word written and nothing behind the buffer, the input untouched, the same
bytes from two calls, one uncleared poisoned scratch buffer for every call.  ``lsr_local_max_candidates_f32`` against an oracle
that does not share the row kernel's doubling spans, into guarded buffers that are exactly full and one slot too small.
``lsr_box_smooth_f32`` against scipy in float64 at 2 units of 2^-24 relative, and the twin's bits.

What the twins cannot tell (``walk_host`` has no read-ahead, no row kernel, no late mask) is told here: the three instantiations of
the strided walk at their first and last half-width and at line lengths around their read-ahead depth, the row kernel at every
width, at one to three segments and on a workgroup's second and third row, the peak sink with every late bit set.
"""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from tests import morphology_cases as C
from tests import morphology_edge_cases as E
from tests import morphology_ref as R
from tests import test_morphology_edges_host as HE
from tests import test_morphology_host as H
from tests import test_psf_host as PH

pytestmark = pytest.mark.gpu

GUARD = H.GUARD
_SCRATCH = {}


def _scratch(device):
    """One poisoned scratch buffer for every morphology call of this module, never cleared between them."""
    if device not in _SCRATCH:
        _SCRATCH[device] = torch.full((E.scratch_bytes_of_the_cases(),), 0xA5, dtype=torch.uint8, device=device)
    return _SCRATCH[device]


def device_morph(d_vol, r, op, device):
    """``test_morphology_gpu.device_morph`` with this module's scratch (sized for the large case): (out, guard) on the host."""
    z, y, x = d_vol.shape
    scratch = _scratch(device)
    assert 0 < _lib.call_value("lsr_grey_morph_scratch_bytes", z, y, x) <= scratch.numel()
    out = torch.full((d_vol.numel() + GUARD,), float(H.FILL), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.call("lsr_grey_morph_f32", d_vol.data_ptr(), out.data_ptr(), z, y, x, *r, C.OPS.index(op), scratch.data_ptr(),
                  _lib.stream_ptr(device))
    host = out.cpu().numpy()
    return host[:d_vol.numel()].reshape(z, y, x), host[d_vol.numel():]


@pytest.mark.parametrize("batch", list(E.BATCHES))
def test_kernels_equal_scipy_the_restatement_and_the_twin_at_the_edges(batch, device):
    uploaded = {}                                                        # each volume goes to the device once
    for case in E.BATCHES[batch]:
        for content in case.contents:
            vol = E.volume(case.shape, content)
            if (case.shape, content) not in uploaded:
                uploaded[case.shape, content] = torch.from_numpy(np.array(vol)).to(device)
            d_vol = uploaded[case.shape, content]
            for op in case.ops:
                what = f"{case.shape} {content} r={case.r} {op}"
                out, guard = device_morph(d_vol, case.r, op, device)
                H.check_buffer(out, guard)
                E.check(case, content, op, out)
                assert R.same_bytes(out, HE.twin_morph(vol, case.r, op)[0]), f"{what}: device and twin disagree"
                again, _ = device_morph(d_vol, case.r, op, device)
                assert out.tobytes() == again.tobytes(), f"{what}: two calls, two answers"
    for (shape, content), d_vol in uploaded.items():
        assert d_vol.cpu().numpy().tobytes() == E.volume(shape, content).tobytes(), "the input was written"


@pytest.mark.parametrize("batch", list(E.PEAK_BATCHES))
def test_kernel_peaks_equal_an_independent_oracle(batch, device):
    uploaded = {}
    cases = E.PEAK_BATCHES[batch]
    voxels = max(int(np.prod(c.shape)) for c in cases)
    scratch = torch.full((2 * voxels,), float("nan"), dtype=torch.float32, device=device)     # A and B; never cleared

    def device_peaks(s, r, threshold, capacity):
        if id(s) not in uploaded:
            uploaded[id(s)] = (s, torch.from_numpy(np.array(s)).to(device))
        d_s = uploaded[id(s)][1]
        index = torch.full((capacity + GUARD,), HE.POISON, dtype=torch.int64, device=device)
        value = torch.full((capacity + GUARD,), float(HE.POISON), dtype=torch.float32, device=device)
        count = torch.full((1,), 12345, dtype=torch.int64, device=device)
        with torch.cuda.device(device):
            _lib.call("lsr_local_max_candidates_f32", d_s.data_ptr(), *s.shape, *r, threshold, index.data_ptr(),
                      value.data_ptr(), capacity, count.data_ptr(), scratch.data_ptr(), _lib.stream_ptr(device))
        return int(count.item()), index.cpu().numpy(), value.cpu().numpy()

    for case in cases:
        n = HE.hold_peaks(device_peaks, case)
        count, index, _ = device_peaks(E.peak_volume(case.shape, case.content), case.r, case.threshold, max(n, 1))
        assert count == n and np.array_equal(np.sort(index[:n]), E.expected_peaks(case)), f"{case}: two calls, two answers"
    for s, d_s in uploaded.values():
        assert d_s.cpu().numpy().tobytes() == s.tobytes(), "the input was written"


def test_kernel_box_smoothing_at_the_mirrors_limit(device):
    _lib.call("lsr_set_host_threads", 4)
    on_device, on_host = HE.hold_box_smoothing(device), HE.hold_box_smoothing(PH.CPU)
    for b in E.BOX_TAPS:
        assert on_device[b].tobytes() == on_host[b].tobytes(), f"{b} taps: the device and the twin differ"
