"""The rank-filter kernels (``csrc/rank.hip``) on the device, through the C ABI, on every case of ``tests/rank_cases.py``:
``scipy.ndimage.rank_filter`` by value on the NaN-free cases, the restated rule and the twin byte for byte (NaNs as a mask), the
generic path (``variant = 1``) byte for byte what the dispatch gives; every output word written and nothing behind the buffer, the
input untouched, the same bytes from two calls; the Python layer, the spike scene, ``segment_zyx`` and the commands.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import rank as K
from tests import rank_cases as C
from tests import rank_ref as R
from tests import test_rank_host as H

pytestmark = pytest.mark.gpu

GUARD = H.GUARD


def device_rank(d_vol, r, rank, op, variant, device, threshold=C.THRESHOLD):
    """The kernel through the C ABI into a poisoned buffer with 64 guard words behind it: (out, guard) on the host."""
    z, y, x = d_vol.shape
    out = torch.full((d_vol.numel() + GUARD,), float(H.FILL), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.call("lsr_rank_filter_f32", d_vol.data_ptr(), out.data_ptr(), z, y, x, *r, rank, C.OPS.index(op),
                  ctypes.c_float(threshold), variant, _lib.stream_ptr(device))
    host = out.cpu().numpy()
    return host[:d_vol.numel()].reshape(z, y, x), host[d_vol.numel():]


@pytest.mark.parametrize("shape,r", C.PARAMS, ids=C.PARAM_IDS)
def test_kernels_equal_scipy_the_restatement_the_twin_and_each_other(shape, r, device):
    volumes = {content: torch.from_numpy(np.array(C.volume(shape, content))).to(device) for content in C.CONTENTS}
    for content, rank, op in C.calls_of(r):
        d_vol = volumes[content]
        out, guard = device_rank(d_vol, r, rank, op, 0, device)
        H.check_buffer(out, guard)
        R.check(shape, content, r, rank, op, out)
        assert out.tobytes() == H.case_twin(shape, content, r, rank, op).tobytes(), f"{content} rank {rank} {op}: device and twin disagree"
        generic, guard = device_rank(d_vol, r, rank, op, 1, device)
        H.check_buffer(generic, guard)
        assert out.tobytes() == generic.tobytes(), f"{content} rank {rank} {op}: the two paths disagree"
        again, _ = device_rank(d_vol, r, rank, op, 0, device)
        assert out.tobytes() == again.tobytes(), f"{content} rank {rank} {op}: two calls, two answers"
    for content, d_vol in volumes.items():
        assert d_vol.cpu().numpy().tobytes() == C.volume(shape, content).tobytes(), "the input was written"


def test_rank_functions_return_torch_tensors_on_the_device(device):
    shape, r = (5, 9, 65), (1, 1, 1)
    vol = torch.from_numpy(np.array(C.volume(shape, "noise"))).to(device)
    before = torch.cuda.memory_allocated(device)
    got = {"rank": K.rank_filter(vol, -2, r), "median": K.median_filter(vol, r), "percentile": K.percentile_filter(vol, 100, r),
           "outliers": K.remove_outliers(vol, r, C.THRESHOLD, "both"), "wide": K.median_filter(vol, (3, 0, 1))}
    assert torch.cuda.memory_allocated(device) > before                  # torch's allocator owns them
    for t in got.values():
        assert t.device == vol.device and t.dtype == torch.float32 and t.is_contiguous() and t.shape == vol.shape
    R.check(shape, "noise", r, 25, "value", got["rank"].cpu().numpy())
    R.check(shape, "noise", r, 13, "value", got["median"].cpu().numpy())
    R.check(shape, "noise", r, 26, "value", got["percentile"].cpu().numpy())
    R.check(shape, "noise", r, 13, "remove_both", got["outliers"].cpu().numpy())
    R.check(shape, "noise", (3, 0, 1), 10, "value", got["wide"].cpu().numpy())


def test_the_spike_scene_on_the_device(device):
    H.check_spike_scene(device)


def test_segment_zyx_median_radius_on_the_device(device):
    H.check_segment_zyx(device)


def test_cli_despeckle_and_segment_on_the_device(tmp_path, device):
    import shrimpy_amd.cli as cli

    H.check_commands(cli, tmp_path)
