"""The fused deskew kernel on the MI355X (``csrc/deskew.hip``) against the restated rule (``tests/deskew_ref.py``) and the host twin,
bit for bit and with no voxel left out, on every case of ``tests/deskew_cases.py``: every tile width at its threshold, every staging
pass and slab position, both signs of ``b``, ``sy`` and ``sx``, rows and columns outside the stack, both borders, every fill value,
the six C entries, uint16 stacks, flat-field patterns, padded rows and planes, non-finite stacks (a NaN by position), and the
workgroup order with and without the XCD swizzle.  There is no tolerance anywhere.

``tests/test_deskew_host.py`` asserts that the cases reach what they aim at, and that the rows a workgroup stages fit its slab.
"""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import deskew as D
from tests import deskew_cases as C
from tests import deskew_ref as R
from tests import test_deskew_host as H

pytestmark = pytest.mark.gpu


def _d(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)


def run_kernel(name, device, u16=False):
    """The whole output buffer (uint32 words, ``C.output_buffer``'s layout) after the case's C entry ran on it."""
    c = C.case(name)
    raw = _d(C.raw_u16(name) if u16 else C.raw(name), device)
    buf = _d(C.output_buffer(c).view(np.int32), device)
    flat = C.flat(name)
    pattern = None if flat is None else _d(flat[0], device)
    mean = None if flat is None else torch.tensor([float(flat[1])], dtype=torch.float32, device=device)
    cval = None
    with torch.cuda.device(device):
        stream = _lib.stream_ptr(device)
        if c.cval == "min":                                                   # the stack's minimum, reduced on the device
            cval = torch.empty(2, dtype=torch.float32, device=device)
            scratch = torch.empty(_lib.call_value("lsr_reduce_scratch_bytes"), dtype=torch.uint8, device=device)
            _lib.call("lsr_minmax_u16" if u16 else "lsr_minmax_f32", raw.data_ptr(), raw.numel(), cval.data_ptr(), scratch.data_ptr(),
                      stream)
        elif c.cval is not None:
            cval = torch.tensor([float(C.fill(name))], dtype=torch.float32, device=device)
        entry, args = C.entry_args(c, u16, raw.data_ptr(), buf.data_ptr(), None if pattern is None else pattern.data_ptr(),
                                   None if mean is None else mean.data_ptr(), None if cval is None else cval.data_ptr(), stream)
        _lib.call(entry, *args)
    torch.cuda.synchronize(device)
    return buf.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("g", C.GROUPS)
def test_kernel_equals_the_restatement_and_the_twin_bit_for_bit(device, g):
    for name in C.group(g):
        c = C.case(name)
        first = None
        for u16 in ((False, True) if c.has_u16 else (False,)):
            buf = run_kernel(name, device, u16)
            out = C.window(c, buf)
            H.check(out, name, f"{C.entry_name(c, u16)}{' (uint16)' if u16 else ''}")
            kept, written = C.padding_intact(c, buf)
            assert kept, f"{name}: a word outside the output window was written"
            assert written, f"{name}: a word of the output window was left unwritten"
            if H.twin_answers(name):
                assert R.same_bits(out, H.case_twin(name)), f"{name}: kernel and twin differ: {R.describe_difference(out, H.case_twin(name))}"
            if first is None:
                first = buf
            else:
                assert R.same_bits(out, C.window(c, first)), f"{name}: the uint16 result differs from the float32 one"


def test_kernel_without_the_xcd_swizzle_gives_the_same_bits(device, monkeypatch):
    for name in C.SWIZZLE_CASES:
        c = C.case(name)
        on = run_kernel(name, device)
        assert c.plan[7] == 8 * ((c.plan[6] + 7) // 8)
        with monkeypatch.context() as mp:
            mp.setenv("LSR_DESKEW_SWIZZLE", "0")
            assert c.plan[7] == c.plan[6], "the switch reaches the launcher"
            off = run_kernel(name, device)
        H.check(C.window(c, off), name, "the kernel without the swizzle")
        assert R.same_bits(C.window(c, off), C.window(c, on)) and C.padding_intact(c, off) == (True, True), name


def test_kernel_average_equals_the_restatement_and_the_twin(device):
    for zd, avg, plane in C.AVERAGE_CASES:
        pre = C.average_input(zd, avg, plane)
        got = D.average_n_slices(_d(pre, device), avg).cpu().numpy()
        assert R.same_bits(got, R.average(pre, avg)), (zd, avg, plane)
        assert got.tobytes() == D.average_n_slices(torch.from_numpy(np.array(pre)), avg).numpy().tobytes(), (zd, avg, plane)


def test_kernel_general_matrix_falls_back_to_resample_then_average(device):
    got = D.deskew_with_matrix(_d(C.general_raw(), device), C.GENERAL_MATRIX, C.GENERAL_PRE, C.GENERAL_AVG).cpu().numpy()
    assert R.same_bits(got, H.general_expected())


def test_average_of_17_slices_on_the_device(device):
    raw, want = H.avg17_case()
    got = D.fast_deskew_zyx(_d(raw, device), **H.AVG17).cpu().numpy()
    assert R.same_bits(got, want)
    assert got.tobytes() == D.fast_deskew_zyx(torch.from_numpy(np.array(raw)), **H.AVG17).numpy().tobytes()
