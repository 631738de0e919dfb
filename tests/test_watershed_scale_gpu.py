"""The watershed kernels (``csrc/watershed.hip``) AT SCALE on the device: the code object's OWN copy of the numbering launches
(``label_uf.hpp``) past the scan's first edge (``merge_wrap``: two counts per scan thread) and, with
``watershed_saddles_kernel``, past the cap of the grid-stride launches (``voxel_wrap``: flatten, final and the saddles go round) --
what ``tests/watershed_cases.py`` with its few ten thousand voxels stays below.  Labels and count against the numpy restatement
(``tests/watershed_ref.py``), every voxel written, nothing behind the buffer, the same bytes from two calls and from the twin, a
scratch buffer of the module's own (poisoned, never cleared); the saddle table as a set of records, bit for bit.

References: the basins are the restatement's for every case.  The saddles of ``merge_wrap`` under 6 are the restatement's; under
26 and on ``voxel_wrap`` the restatement takes more than ten seconds, so there the kernel is held to the twin, and
``tests/test_watershed_scale_host.py`` holds the twin to the restatement on a sub-volume of the same arrays.

No basin is long (white noise: an ascent ends after a few steps; the cases module says why that matters); every launch here asks
``safe_basins`` first.

Not crossed: ``watershed_local_kernel``'s tile wrap needs a column of ``8 * 2^22`` voxels and ``watershed_merge_kernel``'s wrap
``n > 2^26`` -- tens of millions of voxels under a slow reference; their loops have the form of the labelling's, which
``tests/test_label_scale_gpu.py`` pins.  PARITY UNPINNED: the restatement is the reference.
"""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import watershed as W
from tests import test_watershed_scale_host as H
from tests import watershed_scale_cases as C

pytestmark = pytest.mark.gpu

GUARD = H.GUARD
FILL = H.FILL
_SCRATCH = {}


def _scratch(device):
    """One poisoned scratch buffer for every call of this module, never cleared between them: the host module's size."""
    if device not in _SCRATCH:
        _SCRATCH[device] = torch.full((H.scratch().nbytes,), 0xA5, dtype=torch.uint8, device=device)
    return _SCRATCH[device]


def _d(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)


def device_watershed(objects, surface, connectivity, device):
    """The kernels through the C ABI into a buffer pre-filled with -7 with 64 guard words behind it: (basins, B, guard)."""
    z, y, x = objects.shape
    scratch = _scratch(device)
    assert 0 < _lib.call_value("lsr_watershed_scratch_bytes", z, y, x) <= scratch.numel()
    d_objects, d_surface = _d(objects, device), _d(surface, device)
    buf = torch.full((objects.size + GUARD,), FILL, dtype=torch.int32, device=device)
    count = torch.full((1,), FILL, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.call("lsr_watershed_f32", d_objects.data_ptr(), d_surface.data_ptr(), z, y, x, connectivity, buf.data_ptr(),
                  count.data_ptr(), scratch.data_ptr(), _lib.stream_ptr(device))
    host = buf.cpu().numpy()
    return host[:objects.size].reshape(objects.shape), int(count.cpu().item()), host[objects.size:]


def device_saddles(objects, basins, surface, connectivity, capacity, device):
    """The kernel's table (``capacity`` zeroed slots between two guards of 64 words of -7): (records, counts, guards)."""
    z, y, x = objects.shape
    buf = torch.full((2 * GUARD + 4 * capacity,), FILL, dtype=torch.int32, device=device)
    buf[GUARD:GUARD + 4 * capacity] = 0
    counts = torch.full((2 + GUARD,), FILL, dtype=torch.int32, device=device)
    d_objects, d_basins, d_surface = _d(objects, device), _d(basins, device), _d(surface, device)
    with torch.cuda.device(device):
        _lib.call("lsr_watershed_saddles_f32", d_objects.data_ptr(), d_basins.data_ptr(), d_surface.data_ptr(), z, y, x,
                  connectivity, capacity, buf[GUARD:].data_ptr(), counts.data_ptr(), _lib.stream_ptr(device))
    host, c = buf.cpu().numpy(), counts.cpu().numpy()
    return host[GUARD:GUARD + 4 * capacity].view(W.SADDLE_DTYPE), c[:2].tolist(), np.concatenate(
        [host[:GUARD], host[GUARD + 4 * capacity:], c[2:]])


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_kernels_equal_the_restatement_and_the_twin_at_scale(name, connectivity, device):
    case = C.case(name)
    want, n_want, summits = C.safe_basins(name, connectivity)
    got, n, guard = device_watershed(case["objects"], case["surface"], connectivity, device)
    assert np.all(guard == FILL), "the kernels wrote behind their output"
    assert not np.any(got == FILL), "a voxel was not written"
    assert n == n_want == summits
    assert np.array_equal(got, want)
    again, n2, _ = device_watershed(case["objects"], case["surface"], connectivity, device)
    assert n2 == n and got.tobytes() == again.tobytes()
    twin, n_twin, _ = H.twin_watershed(case["objects"], case["surface"], connectivity)
    assert n_twin == n and got.tobytes() == twin.tobytes()


@pytest.mark.parametrize("name,connectivity", [p[:2] for p in H.SADDLE_PARAMS], ids=H.SADDLE_IDS)
def test_saddles_equal_their_reference_at_scale(name, connectivity, device):
    case = C.case(name)
    basins, pair, key, what = H.reference_saddles(name, connectivity)
    rows, counts, guards = device_saddles(case["objects"], basins, case["surface"], connectivity, H.saddle_capacity(len(pair)), device)
    assert np.all(guards == FILL), "the kernel wrote outside the table"
    assert counts == [len(pair), 0], what
    got = H.sorted_records(rows)
    assert np.array_equal(got[0], pair) and np.array_equal(got[1], key), what
