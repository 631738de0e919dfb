"""The device blosc-zstd decoder (``csrc/blosc_decode.hip`` + ``csrc/zstd_lane.hpp``) on what c-blosc writes at every
level: 32 KB - 1 MB blocks, zstd frames of several zstd blocks at zstd's higher strategies, leftover blocks, stored
frames, and the engine's own stack (4 frames of 512 planes, 65 536 lanes).

Frames: c-blosc 1.21's, recorded by ``oracle/make_blosc_levels.py``, and -- for inputs too large to commit -- the
test-side framer of ``tests/test_blosc_levels.py`` (c-blosc's layout over the system libzstd at c-blosc's levels).
Every comparison is bit for bit against the regenerated data.
"""

import numpy as np
import pytest

from tests.test_blosc_levels import (GROUPS, block_stream, byte_shuffle, cblosc_frame, framer_pool, group_data,
                                     level_frames, levels_meta, stored_frame, zstd_blocks)

pytestmark = pytest.mark.gpu


def _decoder(out_bytes, frame_nbytes, blocksize, typesize, device):
    from shrimpy_amd.io.device_codec import DeviceBloscDecoder

    return DeviceBloscDecoder(out_bytes, frame_nbytes, blocksize, typesize, device)


def _decode(dec, frames, device):
    import torch

    out = torch.empty(dec.out_bytes, dtype=torch.uint8, device=device)
    dec.decode_from_host(frames, out)
    assert int(dec.status.cpu().item()) == 0
    return out


@pytest.mark.parametrize("name", GROUPS)
def test_every_level_in_one_launch(device, name):
    """``[c-blosc frame, stored frame, absent, c-blosc frame]`` with the volume ending inside the last frame; then the
    same decoder on ``[absent, frame, stored, frame]``."""
    g = levels_meta()[0]["groups"][name]
    frame, data = level_frames()[name], group_data(name)
    raw, T, nb = data.view(np.uint8), data.itemsize, g["nbytes"]
    bs = int.from_bytes(frame[8:12], "little")
    other = raw[::-1].copy()
    stored = stored_frame(g["stored_header"], other)
    out_bytes = 3 * nb + (2 * nb // 3) // T * T
    zeros = np.zeros(nb, np.uint8)
    dec = _decoder(out_bytes, nb, bs, T, device)
    got = _decode(dec, [frame, stored, b"", frame], device).cpu().numpy()
    assert np.array_equal(got, np.concatenate([raw, other, zeros, raw])[:out_bytes])
    got = _decode(dec, [b"", frame, stored, frame], device).cpu().numpy()
    assert np.array_equal(got, np.concatenate([zeros, raw, other, raw])[:out_bytes])


def _damage_cases(name):
    """(label, frames, the block DecodeError must name, its code) for a two-frame launch [good, damaged]."""
    frame = level_frames()[name]
    nb = levels_meta()[0]["groups"][name]["nbytes"]
    bs = int.from_bytes(frame[8:12], "little")
    bpf = -(-nb // bs)
    k = 1 if bpf > 1 else 0                                  # a full block of the second frame
    at, cb = block_stream(frame, k)
    blocks = zstd_blocks(frame[at:at + cb])
    assert len(blocks) >= 2, "the block holds one zstd block: nothing after the first to damage"
    bad = bytearray(frame)
    bad[at + blocks[1][0]] |= 0x6                            # the second zstd block's type becomes 3 (reserved)
    cut = frame[:block_stream(frame, bpf - 1)[0] + 100]      # the last block's stream runs past the end
    wrong = bytearray(frame)
    wrong[8:12] = (bs // 2).to_bytes(4, "little")           # a blocksize that is not the launch's
    return [("flipped byte in zstd block 2", [frame, bytes(bad)], [bpf + k], 1),
            ("truncated frame", [frame, cut], [2 * bpf - 1], 1),
            ("header blocksize", [frame, bytes(wrong)], list(range(bpf, 2 * bpf)), 4)]


@pytest.mark.parametrize("name", ["u16_shuffle_c4", "f32_shuffle_c4", "u16_shuffle_c9", "f32_shuffle_c9"])
def test_damaged_frames_name_their_block(device, name):
    """The decoder's contract on corrupt input at 256 KB and 1 MB blocks: ``DecodeError`` naming the damaged block,
    and a correct decode on the same decoder afterwards."""
    from shrimpy_amd.io.device_codec import DecodeError

    frame, data = level_frames()[name], group_data(name)
    raw, nb = data.view(np.uint8), data.nbytes
    bs = int.from_bytes(frame[8:12], "little")
    dec = _decoder(2 * nb, nb, bs, data.itemsize, device)
    for label, frames, blocks, code in _damage_cases(name):
        with pytest.raises(DecodeError) as err:
            _decode(dec, frames, device)
        assert err.value.frame == 1 and err.value.block in blocks and err.value.code == code, (label, str(err.value))
        got = _decode(dec, [frame, frame], device).cpu().numpy()
        assert np.array_equal(got, np.concatenate([raw, raw])), label


def _stack(shape, seed):
    """A light-sheet-like uint16 stack, fast at any size: plane z = a window of a Poisson pool at a plane-dependent
    offset (no two planes, and no two blocks, alike)."""
    from oracle.make_blosc_levels import light_sheet

    plane = shape[1] * shape[2]
    pool = light_sheet(seed, (1 << 22) + plane, "uint16")
    out = np.empty(shape, np.uint16)
    flat = out.reshape(shape[0], plane)
    for z in range(shape[0]):
        o = (z * 40_503) % (1 << 22)
        flat[z] = pool[o:o + plane]
    return out


def _chunked(vol, zc):
    """Zarr's z-chunks of ``vol``: ``zc`` planes each, the last one padded with the fill value (zero)."""
    n = -(-vol.shape[0] // zc)
    for c in range(n):
        part = vol[c * zc:(c + 1) * zc]
        if part.shape[0] < zc:
            part = np.concatenate([part, np.zeros((zc - part.shape[0],) + vol.shape[1:], vol.dtype)])
        yield np.ascontiguousarray(part)


def _run_stack(device, vol, zc, clevel):
    import torch

    T = vol.dtype.itemsize
    with framer_pool() as pool:
        frames = [cblosc_frame(c, T, clevel, 1, pool=pool) for c in _chunked(vol, zc)]
    nb = zc * vol.shape[1] * vol.shape[2] * T
    bs = int.from_bytes(frames[0][8:12], "little")
    assert frames[0][2] == 0x91
    dec = _decoder(vol.nbytes, nb, bs, T, device)
    src = torch.from_numpy(vol.reshape(-1).view(np.int16)).to(device).view(torch.uint8)
    out = _decode(dec, frames, device)
    assert torch.equal(out, src)
    return dec


def test_the_engine_stack(device):
    """(2048, 256, 2048) uint16 as the engine stores it: 4 frames of 512 planes, 32 KB blocks (clevel 1) --
    2^31 bytes, 65 536 lanes; compared on the device."""
    dec = _run_stack(device, _stack((2048, 256, 2048), 7), 512, 1)
    assert dec.n_frames * dec.blocks_per_frame == 65536


def test_an_engine_stack_with_an_edge_chunk(device):
    """nz = 600 at reduced XY: the second 512-plane frame is a padded edge chunk."""
    _run_stack(device, _stack((600, 64, 256), 8), 512, 1)


def test_256_kb_blocks_over_two_chunks(device):
    """clevel 4 (256 KB blocks, zstd level 7) over two 512-plane chunks of (512, 256, 512)."""
    _run_stack(device, _stack((1024, 256, 512), 9), 512, 4)


@pytest.fixture(scope="module")
def megablocks():
    """Eight distinct 1 MB blocks per typesize and their zstd-max frames (compressed once for the module)."""
    from oracle.make_blosc_levels import light_sheet

    from shrimpy_amd.io import codecs

    cache, blocks = {}, {}

    def compress(src, level):
        if src not in cache:
            cache[src] = codecs.zstd_compress(src, level)
        return cache[src]

    for T, dtype in ((2, "uint16"), (4, "float32")):
        blocks[T] = [light_sheet(300 + 10 * T + j, (1 << 20) // T, dtype).view(np.uint8) for j in range(8)]
        with framer_pool() as pool:      # fills the cache: one zstd-22 compression per distinct block
            list(pool.map(lambda b: compress(byte_shuffle(b, T).tobytes(), 22), blocks[T]))
    return blocks, compress


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("lanes", [1, 63, 64, 65, 300])
def test_1_mb_blocks_at_scale(device, megablocks, T, lanes):
    """1 MB blocks at the clevel-9 mapping: one lane, around a wave (63 / 64 / 65), and past one 256-lane workgroup."""
    import torch

    blocks, compress = megablocks
    raw = np.concatenate([blocks[T][(5 * k + lanes) % 8] for k in range(lanes)])
    frame = cblosc_frame(raw, T, 9, 1, compress=compress)
    assert frame[2] == 0x91 and int.from_bytes(frame[8:12], "little") == 1 << 20 and len(frame) < 0.7 * raw.size
    dec = _decoder(raw.size, raw.size, 1 << 20, T, device)
    got = _decode(dec, [frame], device)
    assert torch.equal(got, torch.from_numpy(raw).to(device))
