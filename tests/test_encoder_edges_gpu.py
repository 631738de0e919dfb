"""The device blosc-zstd encoder (``csrc/blosc_encode.hip``) at every lane-run and mode edge, byte for byte.

The cases are those of ``tests/encoder_cases.py``; ``tests/test_encoder_edges_host.py`` shows, without a GPU, that they reach
what they are named for and that the host twin's frames decode with libzstd and the Python walker.  Here, for each:

* the device frames equal the twin's frames, and
* the device frames, decoded by the system libzstd, equal the zero-padded input (which does not involve the twin).

Both are equalities of bytes; there is no tolerance in this file.  Every test is a loop of small encodes.
"""

import numpy as np
import pytest

from shrimpy_amd import _lib
from shrimpy_amd.io import codecs
from shrimpy_amd.io.device_codec import encode_frames_host, plan_frames
from tests import encoder_cases as ec

pytestmark = pytest.mark.gpu


def _compare(label, arr, frame_bytes, got, want):
    """Lines that say where ``got`` (device frames) departs from ``want`` (the twin's) or from the input."""
    bad = []
    if len(got) != len(want):
        return [f"{label}: {len(got)} frames, the twin has {len(want)}"]
    padded = ec.padded(arr, frame_bytes)
    for f, (g, w) in enumerate(zip(got, want)):
        if g != w:
            first = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            bad.append(f"{label}, frame {f}: differs from the twin at byte {first} (sizes {len(g)} / {len(w)})")
        try:
            ok = np.array_equal(codecs.blosc_decode(g, backend="lsrecon"), padded[f])
        except Exception as e:       # noqa: BLE001 -- whatever the decoder says about a frame it rejects is the finding
            bad.append(f"{label}, frame {f}: libzstd rejects the device frame ({e})")
        else:
            if not ok:
                bad.append(f"{label}, frame {f}: libzstd decodes the device frame to other bytes than the input")
    return bad


def _encode(device, arr, frame_bytes, blocksize):
    import torch

    from shrimpy_amd.io.device_codec import DeviceBloscEncoder

    enc = DeviceBloscEncoder(arr.nbytes, arr.dtype.itemsize, frame_bytes, device, blocksize)
    return enc.encode_to_host(torch.as_tensor(arr).to(device))


def _run(device, cases):
    bad = []
    for label, arr, frame_bytes, blocksize in cases:
        bad += _compare(label, arr, frame_bytes, _encode(device, arr, frame_bytes, blocksize),
                        encode_frames_host(arr, frame_bytes, blocksize))
    assert not bad, f"{len(bad)} findings:\n" + "\n".join(bad[:40])


# a. lane runs ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", ec.SWEEP_P)
@pytest.mark.parametrize("T", ec.SWEEP_T)
def test_lane_run_sweep(device, T, P):
    """Plane lengths P - 4 .. P + 33, one block per frame, three frames with the Huffman profiles dealt differently: every
    run length, every merged tail, 64 and fewer lanes, streams 0..2 and stream 3 with different run lengths, the aligned
    and the per-symbol staging, both sides of 2048 / 16384 / 32768."""
    _run(device, [ec.sweep_case(n, T) for n in ec.sweep_lengths(P)])


@pytest.mark.parametrize("T", ec.SWEEP_T)
def test_shortest_and_longest_planes(device, T):
    _run(device, [ec.sweep_case(n, T) for n in ec.END_LENGTHS])


# b. mode mixes at the sample threshold ---------------------------------------------------------------------------------

@pytest.mark.parametrize("T", (4, 2, 1))
def test_mode_mixes_at_the_sample_threshold(device, T):
    _run(device, [ec.mix_case(names, n) for names in ec.MIXES[T] for n in ec.MIX_N])


# c. the wave-uniform histogram shortcut --------------------------------------------------------------------------------

def test_wave_uniform_histogram_shortcut(device):
    _run(device, ec.uniform_wave_cases())


# d. source edges -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", (4, 2, 1))
def test_source_edges(device, T):
    _run(device, ec.source_edge_cases(T))


# e. more than 256 blocks per frame -------------------------------------------------------------------------------------

def test_more_than_256_blocks_per_frame(device):
    _run(device, ec.many_block_cases())


# f. buffers ------------------------------------------------------------------------------------------------------------

GUARD, FILL = 4096, 0xA5


def _guarded_cases():
    return [ec.sweep_case(2050, 4), ec.sweep_case(32771, 2), ec.sweep_case(4099, 1), ec.small_block_case(257),
            ec.mix_case(ec.EARLY_VERBATIM, ec.MAX_PLANE), ec.source_edge_case(4, frame=0, block=0, valid=4)]


def test_the_kernels_stay_inside_the_planned_buffers(device):
    """``lsr_blosc_encode_device`` with scratch and output of exactly the planned sizes, 4096 guard bytes behind each,
    all of it 0xA5 beforehand: the guards survive, and so do the bytes between a frame's end and the 16-byte-aligned
    start of the next."""
    import torch

    for label, arr, frame_bytes, blocksize in _guarded_cases():
        T = arr.dtype.itemsize
        n_frames, scratch_bytes, cap = plan_frames(arr.nbytes, T, frame_bytes, blocksize)
        src = torch.as_tensor(arr).to(device)
        scratch = torch.full((scratch_bytes + GUARD,), FILL, dtype=torch.uint8, device=device)
        out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device=device)
        table = torch.zeros((n_frames, 2), dtype=torch.int64, device=device)
        assert scratch.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        _lib.call("lsr_blosc_encode_device", src.data_ptr(), arr.nbytes, T, frame_bytes, blocksize, scratch.data_ptr(),
                  scratch_bytes, out.data_ptr(), cap, table.data_ptr(), _lib.stream_ptr(device))
        torch.cuda.synchronize(device)
        assert bool((scratch[scratch_bytes:] == FILL).all()), f"{label}: bytes behind the scratch buffer were written"
        assert bool((out[cap:] == FILL).all()), f"{label}: bytes behind the output buffer were written"
        host, tab = out[:cap].cpu().numpy(), table.cpu().numpy()
        want = encode_frames_host(arr, frame_bytes, blocksize)
        at = 0
        for f, (o, n) in enumerate(tab):
            assert o == at and o % 16 == 0, (label, f, tab)
            assert host[o:o + n].tobytes() == want[f], f"{label}, frame {f}: differs from the twin"
            at = (o + n + 15) // 16 * 16
            assert at <= cap and (host[o + n:at] == FILL).all(), f"{label}: the gap behind frame {f} was written"
        assert any(int(n) % 16 for _, n in tab), label        # (there were gaps to look at)


def test_one_encoder_on_four_different_volumes(device):
    """Verbatim blocks, then the early-then-verbatim case, then Huffman-coded planes, then RLE planes, all through the
    same scratch and output buffers: each call gives its own twin's bytes, whatever the call before left behind."""
    import torch

    from shrimpy_amd.io.device_codec import DeviceBloscEncoder

    volumes = ec.buffer_volumes()
    enc = DeviceBloscEncoder(volumes[0].nbytes, 4, volumes[0].nbytes, device, 0)
    bad = []
    for k, v in enumerate(volumes + volumes[::-1]):
        assert v.nbytes == volumes[0].nbytes
        got = enc.encode_to_host(torch.as_tensor(v).to(device))
        bad += _compare(f"call {k}", v, v.nbytes, got, encode_frames_host(v, v.nbytes, 0))
    assert not bad, "\n".join(bad)


# g. code construction --------------------------------------------------------------------------------------------------

def test_code_construction_edges(device):
    """Sort keys with the largest count, ties decided by the symbol, the deepest tree, and 128 / 129 weights (nibbles
    against the FSE stream) with the last present symbol at 128, 129 and 255."""
    _run(device, ec.code_cases())
