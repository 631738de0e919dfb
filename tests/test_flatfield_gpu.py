"""The flat-field kernels on the MI355X (``csrc/flatfield.hip``, the fused staging of ``csrc/deskew.hip``) against the restated rule
(``tests/flatfield_ref.py``) and the host twins, bit for bit, on every case of ``tests/flatfield_cases.py``: every pass and state of
the radix select, the count mode and its fallbacks, the counter limit, NaNs, infinities, zeros of both signs and denormals; the mean
inside its a-priori bound and reproducible; the division in and out of place; the fused deskew against apply-then-deskew; and the
kernel against ``torch.quantile`` on the device.

``tests/test_flatfield_host.py`` asserts that the cases reach what they aim at.
"""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import flatfield as F
from tests import flatfield_cases as C
from tests import flatfield_ref as R
from tests import test_flatfield_host as H

pytestmark = pytest.mark.gpu


def _d(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)


def kernel(vol, device):
    """``(pattern, mean)`` of the device entry as numpy arrays."""
    ff = F.flat_field_pattern(_d(vol, device))
    return ff.pattern.cpu().numpy(), ff.mean.cpu().numpy()


def same_as_twin(got, name):
    """Byte for byte, a NaN the arithmetic itself made (``inf - inf``, no NaN in the column) by position."""
    twin, _ = H.case_twin(name)
    made = np.isnan(C.expected(name)) & ~np.isnan(C.volume(name)).any(axis=0)
    return np.array_equal(H.bits(got)[~made], H.bits(twin)[~made]) and np.isnan(got[made]).all() and np.isnan(twin[made]).all()


@pytest.mark.parametrize("prefix", C.GROUPS)
def test_kernel_pattern_equals_the_restatement_and_the_twin_bit_for_bit(device, prefix):
    worst = 0.0
    for name in C.group(prefix):
        pattern, mean = kernel(C.volume(name), device)
        H.check_pattern(pattern, name, "kernel")
        assert same_as_twin(pattern, name), f"{name}: kernel and twin differ"
        worst = max(worst, H.check_mean(mean[0], pattern, f"kernel on {name!r}"))
        again, mean2 = kernel(C.volume(name), device)
        assert again.tobytes() == pattern.tobytes() and mean2.tobytes() == mean.tobytes(), f"{name}: a second call differs"
        if C.is_u16_case(name):
            p16, m16 = kernel(C.volume_u16(name), device)
            assert p16.tobytes() == pattern.tobytes() and m16.tobytes() == mean.tobytes(), f"{name}: uint16 and float32 differ"
    print(f"{prefix}: worst mean error {worst:.4f} of the bound")


@pytest.mark.parametrize("content", C.MEAN_CONTENTS)
def test_kernel_mean_is_within_the_bound_of_an_fsum_and_reproducible(device, content):
    """Planes of 1, 255, 256, 257, 259 and 65537 pixels: fewer blocks than the reduction holds, exactly as many, and empty ones."""
    for plane in C.MEAN_PLANES:
        vol = C.mean_plane(plane, content)
        pattern, mean = kernel(vol, device)
        assert pattern.tobytes() == vol.tobytes(), "Z = 1: the pattern is the stack"
        frac = H.check_mean(mean[0], vol, f"kernel on {plane} {content}")
        assert kernel(vol, device)[1].tobytes() == mean.tobytes(), f"{plane} {content}: the mean of a second call differs"
        print(f"{plane} {content}: mean error {frac:.4f} of the bound")


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_kernel_apply_is_the_restatement_byte_for_byte(device, dtype):
    for shape in C.APPLY_SHAPES + [C.APPLY_BIG[dtype]]:
        vol, pat = C.apply_case(shape, dtype)
        want = torch.from_numpy(R.apply(vol, pat, C.APPLY_MEAN)).view(torch.int32)
        ff = F.FlatFieldPattern(_d(pat, device), torch.tensor([C.APPLY_MEAN], device=device))
        t = _d(vol, device)
        out = ff.apply(t)
        assert torch.equal(out.view(torch.int32).cpu(), want), (shape, dtype)
        assert torch.equal(t.cpu(), torch.from_numpy(np.array(vol))), "the input was written"
        if dtype == "float32":
            assert ff.apply(t, out=t) is t and torch.equal(t.view(torch.int32).cpu(), want), (shape, "in place")


@pytest.mark.parametrize("border", ["constant", "grid-constant"])
@pytest.mark.parametrize("shape,avg", [((100, 7, 37), 3), ((131, 11, 70), 2)])
def test_fused_deskew_equals_apply_then_deskew_bit_for_bit(device, shape, avg, border):
    """``lsr_deskew_flat_f32`` / ``_u16`` (and the fused staging under the grid-constant border) on rows that are neither a multiple
    of 4 nor of the deskew tile; the pattern holds a zero and a NaN pixel.  NaNs compare by position."""
    from shrimpy_amd.deskew import deskew_with_matrix
    from shrimpy_amd.geometry import deskew_geometry

    assert shape[2] % 4 and shape[2] % 64
    rng = np.random.default_rng(shape[2])
    raw16 = rng.integers(1, 600, shape).astype(np.uint16)
    pat = (100.0 + 500.0 * rng.random(shape[1:])).astype(np.float32)
    pat[1, 2], pat[shape[1] - 1, shape[2] - 1] = 0.0, np.nan
    ff = F.FlatFieldPattern(_d(pat, device), torch.tensor([C.APPLY_MEAN], device=device))
    geo = deskew_geometry(shape, 30.0, 0.755, False, avg)
    for raw in (_d(raw16, device), _d(raw16.astype(np.float32), device)):
        fused = deskew_with_matrix(raw, geo.matrix_3x4, geo.pre_average_shape, avg, flat_field=ff, border=border).cpu().numpy()
        two = deskew_with_matrix(ff.apply(raw), geo.matrix_3x4, geo.pre_average_shape, avg, border=border).cpu().numpy()
        nan = np.isnan(two)
        assert nan.any() and np.isinf(two).any() and np.isfinite(two).sum() > two.size // 2
        assert np.array_equal(np.isnan(fused), nan) and np.array_equal(H.bits(fused)[~nan], H.bits(two)[~nan]), str(raw.dtype)


@pytest.mark.parametrize("prefix", [g for g in C.GROUPS if g not in ("nan", "zeros")])
def test_kernel_equals_torch_quantile_on_the_device(device, prefix):
    """Every NaN-free case without zeros of both signs (an infinite median of an odd count is NaN in torch, as on the host).
    No stack is left out: on the MI355X ``torch.quantile`` (torch 2.10) gave the single-rounding answer on the three
    ``1e-38 N(0, 1)`` denormal stacks as well -- 0 of 259 pixels differ on each, so it neither flushes denormals nor rounds the lerp
    twice -- and where its bits differ from the kernel's at all (14, 31, 2 and 3 pixels of the infinity stacks) both hold a NaN
    that ``inf - inf`` made."""
    for name in C.group(prefix):
        if not C.torch_comparable(name):
            continue
        pattern, _ = kernel(C.volume(name), device)
        got = torch.quantile(_d(C.volume(name), device), 0.5, dim=0).cpu().numpy()
        mismatches = int((H.bits(got) != H.bits(pattern)).sum())
        print(f"{name}: device torch.quantile differs from the kernel on {mismatches} of {pattern.size} pixels")
        H.check_against_torch(got, name, "torch.quantile on the device")


def test_kernel_refuses_the_first_z_the_counters_cannot_hold(device):
    pattern = torch.full((3,), float("nan"), device=device)
    mean = torch.full((1,), float("nan"), device=device)
    scratch = torch.empty((_lib.call_value("lsr_flatfield_scratch_bytes"),), dtype=torch.uint8, device=device)
    for entry, vol in (("lsr_flatfield_pattern_f32", torch.ones((C.REFUSED_Z, 1, 3), device=device)),
                       ("lsr_flatfield_pattern_u16", torch.ones((C.REFUSED_Z, 1, 3), device=device).to(torch.uint16))):
        with pytest.raises(_lib.LsrUnsupported):
            _lib.call(entry, vol.data_ptr(), C.REFUSED_Z, 1, 3, pattern.data_ptr(), mean.data_ptr(), scratch.data_ptr(),
                      _lib.stream_ptr(device))
        torch.cuda.synchronize()
        assert torch.isnan(pattern).all() and torch.isnan(mean).all()
