"""The device decoder's inputs as c-blosc 1.21 writes them at every compression level (``oracle/make_blosc_levels.py``).

c-blosc with the zstd compressor picks its blocksize from the level (16 KB at clevel 0 up to 1 MB at clevel 9 on a
large chunk), never splits blocks (``DONTSPLIT``), and calls zstd at level ``2 clevel - 1`` (clevel 9: zstd's
maximum) -- so from clevel 2 on a block is a zstd frame of several zstd blocks at zstd's higher strategies.  This
module pins the host side on the recorded frames and holds the test-side framer that builds frames of c-blosc's
layout for inputs too large to commit; ``tests/test_device_decoder_levels_gpu.py`` feeds both to the device.

CPU tests: every recorded frame decodes bit for bit through the decoder twin, the native frame walker and the Python
walker; ``frame_layout`` and the framer agree with the recorded header table; libblosc (where it loads) reads the
framer's frames and this package's encoder twin's.
"""

import ctypes
import ctypes.util
import hashlib
import json
import os
import struct

from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from oracle.make_blosc_levels import light_sheet
from shrimpy_amd.io import codecs
from shrimpy_amd.io.device_codec import decode_frames_host, encode_frames_host, frame_layout

GOLDEN = Path(__file__).resolve().parent / "golden"


# ---------------------------------------------------------------------------------------------------------------------
# the recorded fixtures
# ---------------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def levels_meta() -> tuple[dict, np.ndarray]:
    z = np.load(GOLDEN / "blosc_levels_table.npz")
    return json.loads(str(z["meta"])), z["table"]


@lru_cache(maxsize=None)
def level_frames() -> dict:
    out = {}
    for p in sorted(GOLDEN.glob("blosc_levels_frames_*.npz")):
        z = np.load(p)
        out.update({k: z[k].tobytes() for k in z.files})
    return out


def group_data(name: str) -> np.ndarray:
    """A fixture group's data, rebuilt from its seeded recipe and checked against the recorded SHA-1."""
    g = levels_meta()[0]["groups"][name]
    r = g["recipe"]
    a = light_sheet(r["seed"], r["n"], r["dtype"])
    assert hashlib.sha1(a.tobytes()).hexdigest() == g["sha1"], f"{name} does not rebuild to the recorded bytes"
    return a


GROUPS = sorted(levels_meta()[0]["groups"])


# ---------------------------------------------------------------------------------------------------------------------
# the framer: c-blosc 1.21's layout with the zstd compressor, built here
# ---------------------------------------------------------------------------------------------------------------------

_F_SHUFFLE, _F_MEMCPYED, _F_DONTSPLIT, _ZSTD = 0x1, 0x2, 0x10, 4 << 5


def cblosc_blocksize(nbytes: int, clevel: int, typesize: int) -> int:
    """c-blosc 1.21's ``compute_blocksize`` for zstd (no forced blocksize, blocks never split): 64 KB scaled by the
    level on chunks of at least 32 KB, the whole chunk below; at most the chunk, a multiple of the typesize."""
    if nbytes < typesize:
        return 1
    bs = nbytes
    if nbytes >= 32 * 1024:
        bs = 64 * 1024 * {0: 0.25, 1: 0.5, 2: 1, 3: 2, 4: 4, 5: 4, 6: 8, 7: 8, 8: 8, 9: 16}[clevel]
    bs = min(int(bs), nbytes)
    return bs // typesize * typesize if bs > typesize else bs


def cblosc_flags(shuffle: int) -> int:
    return _ZSTD | _F_DONTSPLIT | (_F_SHUFFLE if shuffle else 0)


def zstd_level(clevel: int) -> int:
    """c-blosc's level rule (confirmed by the recipe against the libzstd libblosc links: ``zstd_level_rule``)."""
    return 2 * clevel - 1 if clevel < 9 else 22


def byte_shuffle(block: np.ndarray, typesize: int) -> np.ndarray:
    n = block.size // typesize
    return np.concatenate([block[:n * typesize].reshape(n, typesize).T.reshape(-1), block[n * typesize:]])


def cblosc_frame(raw, typesize: int, clevel: int, shuffle: int, blocksize: int | None = None, pool=None,
                 compress=None) -> bytes:
    """One frame of ``raw`` (uint8) in c-blosc's layout: the header c-blosc writes, one zstd frame per block through
    the system libzstd at c-blosc's level (``compress``: another ``(bytes, level) -> bytes``), the shuffled bytes
    verbatim where zstd does not shrink a block, and the stored form when the frame would not fit in ``nbytes + 16``
    (c-blosc's destination).  ``pool``: an executor for the blocks."""
    raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    nbytes = raw.size
    bs = cblosc_blocksize(nbytes, clevel, typesize) if blocksize is None else blocksize
    flags = cblosc_flags(shuffle)
    nblocks = -(-nbytes // bs)
    level = zstd_level(clevel)
    compress = compress or codecs.zstd_compress

    def one(k):
        blk = raw[k * bs:(k + 1) * bs]
        src = byte_shuffle(blk, typesize) if shuffle and typesize > 1 else blk
        src = src.tobytes()
        z = compress(src, level)
        return src if len(z) >= len(src) else z

    streams = list(pool.map(one, range(nblocks)) if pool is not None else map(one, range(nblocks)))
    pos, starts = 16 + 4 * nblocks, []
    for s in streams:
        starts.append(pos)
        pos += 4 + len(s)
    if pos > nbytes + 16:
        return stored_frame(struct.pack("<BBBBIII", 2, 1, flags | _F_MEMCPYED, typesize, nbytes, bs, nbytes + 16), raw)
    head = struct.pack("<BBBBIII", 2, 1, flags, typesize, nbytes, bs, pos)
    return b"".join([head, struct.pack(f"<{nblocks}i", *starts)] + [struct.pack("<i", len(s)) + s for s in streams])


def stored_frame(header, raw) -> bytes:
    """c-blosc's stored frame: the 16-byte header, then the plain bytes."""
    return bytes(header) + np.ascontiguousarray(raw).reshape(-1).view(np.uint8).tobytes()


def framer_pool():
    return ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))


def zstd_blocks(zframe: bytes) -> list[tuple[int, int, int]]:
    """(offset of the block header, type, size) of every block of one zstd frame."""
    fhd = zframe[4]
    at = 5 + (0 if (fhd >> 5) & 1 else 1)
    at += (0, 1, 2, 4)[fhd & 3]
    at += (((fhd >> 5) & 1), 2, 4, 8)[fhd >> 6]
    out = []
    while True:
        bh = int.from_bytes(zframe[at:at + 3], "little")
        typ, size = (bh >> 1) & 3, bh >> 3
        out.append((at, typ, size))
        at += 3 + (1 if typ == 1 else size)
        if bh & 1:
            return out


def block_stream(frame: bytes, k: int) -> tuple[int, int]:
    """(offset, size) of blosc block k's stream inside a frame (one stream per block: DONTSPLIT)."""
    at = int.from_bytes(frame[16 + 4 * k:20 + 4 * k], "little")
    return at + 4, int.from_bytes(frame[at:at + 4], "little")


def libblosc():
    """A real c-blosc through ctypes, or None (the build image has one at /opt/conda/lib)."""
    for cand in (os.environ.get("LSR_LIBBLOSC"), ctypes.util.find_library("blosc"), "/opt/conda/lib/libblosc.so.1"):
        if not cand:
            continue
        try:
            lib = ctypes.CDLL(cand)
        except OSError:
            continue
        lib.blosc_decompress_ctx.restype = ctypes.c_int
        lib.blosc_decompress_ctx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        return lib
    return None


def libblosc_decode(lib, frame: bytes, nbytes: int) -> np.ndarray:
    out = np.empty(max(nbytes, 1), np.uint8)
    got = lib.blosc_decompress_ctx(frame, out.ctypes.data, out.size, 1)
    assert got == nbytes, f"blosc_decompress_ctx returned {got}, expected {nbytes}"
    return out[:nbytes]


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------

def test_recipe_recorded_what_the_device_tests_assume():
    meta, table = levels_meta()
    assert meta["libblosc"].startswith("1.21")
    assert all(r["confirmed"] for r in meta["zstd_level_rule"].values()), meta["zstd_level_rule"]
    assert {int(c): r["zstd_level"] for c, r in meta["zstd_level_rule"].items()} == {c: zstd_level(c) for c in range(1, 10)}
    assert max(p.stat().st_size for p in GOLDEN.glob("blosc_levels_*.npz")) < 540_000
    assert sorted(set(table[:, 1].tolist())) == list(range(10)) and table.shape[1] == 7


@pytest.mark.parametrize("name", GROUPS)
def test_fixture_frames_decode_bit_for_bit_on_the_host(name):
    """Twin (``decode_frames_host``), ``lsr_blosc_decode_host`` and the Python walker on c-blosc's frame; then the
    twin on the GPU test's launch ``[frame, stored, absent, frame]`` with the volume ending inside the last frame."""
    g = levels_meta()[0]["groups"][name]
    frame, data = level_frames()[name], group_data(name)
    raw = data.view(np.uint8)
    lay = frame_layout(frame)
    assert lay == dict(nbytes=g["nbytes"], blocksize=cblosc_blocksize(g["nbytes"], g["clevel"], data.itemsize),
                       typesize=data.itemsize)
    got = decode_frames_host([frame], lay["nbytes"], lay["blocksize"], lay["typesize"], raw.size)
    assert np.array_equal(got, raw), "decoder twin"
    assert np.array_equal(codecs.blosc_decode(frame, backend="lsrecon"), raw), "lsr_blosc_decode_host"
    out = np.empty(raw.size, np.uint8)
    codecs._py_blosc_decode(frame, out)
    assert np.array_equal(out, raw), "Python walker"
    nb, T = raw.size, data.itemsize
    other = raw[::-1].copy()
    frames = [frame, stored_frame(g["stored_header"], other), b"", frame]
    out_bytes = 3 * nb + (2 * nb // 3) // T * T
    want = np.concatenate([raw, other, np.zeros(nb, np.uint8), raw])[:out_bytes]
    got = decode_frames_host(frames, nb, lay["blocksize"], T, out_bytes)
    assert np.array_equal(got, want)


def test_frame_layout_agrees_with_the_header_table():
    meta, table = levels_meta()
    for nbytes, clevel, T, shuffle, bs, flags, t_written in table.tolist():
        head = struct.pack("<BBBBIII", 2, 1, flags, t_written, nbytes, bs, 16)
        lay = frame_layout(head)
        if flags & _F_MEMCPYED:
            assert clevel == 0 and lay is None
        else:
            assert lay == dict(nbytes=nbytes, blocksize=bs, typesize=T), (nbytes, clevel, T, shuffle)
    for name, g in meta["groups"].items():
        assert frame_layout(bytes(g["stored_header"])) is None, name


def test_framer_headers_equal_c_blosc():
    """Per table row: c-blosc's blocksize rule, flags and typesize; per fixture group: the framer's frame of the same
    data has c-blosc's header (but for cbytes: the two libzstd builds differ), decodes through the twin and -- where
    libblosc loads -- through libblosc; the framer's stored frame of noise is c-blosc's, byte for byte."""
    meta, table = levels_meta()
    for nbytes, clevel, T, shuffle, bs, flags, t_written in table.tolist():
        assert cblosc_blocksize(nbytes, clevel, T) == bs, (nbytes, clevel, T)
        want_flags = cblosc_flags(shuffle) | (_F_MEMCPYED if clevel == 0 else 0)
        assert (flags, t_written) == (want_flags, T), (nbytes, clevel, T, shuffle)
    lib = libblosc()
    for name, g in meta["groups"].items():
        data = group_data(name)
        T = data.itemsize
        mine = cblosc_frame(data, T, g["clevel"], g["shuffle"])
        assert mine[:12] == level_frames()[name][:12], name
        got = decode_frames_host([mine], g["nbytes"], cblosc_blocksize(g["nbytes"], g["clevel"], T), T, data.nbytes)
        assert np.array_equal(got, data.view(np.uint8)), name
        noise = np.random.default_rng(g["recipe"]["seed"]).integers(0, 256, g["nbytes"], dtype=np.uint8)
        stored = cblosc_frame(noise, T, g["clevel"], g["shuffle"])
        assert stored[:16] == bytes(g["stored_header"]) and stored[16:] == noise.tobytes(), name
        if lib is not None:
            assert np.array_equal(libblosc_decode(lib, mine, g["nbytes"]), data.view(np.uint8)), name
            assert np.array_equal(libblosc_decode(lib, stored, g["nbytes"]), noise), name


def test_framer_edges():
    """A raw block where zstd does not shrink it; the whole frame stored where the frame would not fit."""
    rng = np.random.default_rng(4)
    noisy = rng.integers(0, 256, 70_000, dtype=np.uint8)
    flat = np.full(70_000, 7, np.uint8)
    raw = np.concatenate([flat, noisy])               # clevel 1: 32 KB blocks, the last ones incompressible
    frame = cblosc_frame(raw, 2, 1, 1)
    assert frame[2] == 0x91
    kinds = [block_stream(frame, k)[1] for k in range(-(-raw.size // 32768))]
    assert kinds[0] < 100 and kinds[-2] == 32768
    got = decode_frames_host([frame], raw.size, 32768, 2, raw.size)
    assert np.array_equal(got, raw)
    stored = cblosc_frame(noisy, 4, 5, 0)
    assert stored[2] == 0x92 and len(stored) == noisy.size + 16 and stored[16:] == noisy.tobytes()
    lib = libblosc()
    if lib is not None:
        assert np.array_equal(libblosc_decode(lib, frame, raw.size), raw)
        assert np.array_equal(libblosc_decode(lib, stored, noisy.size), noisy)


def test_libblosc_reads_the_encoder_twins_frames():
    """libblosc decodes ``encode_frames_host``'s frames for every case of ``tests/test_device_codec.py``."""
    from tests.test_device_codec import CASES, _want

    lib = libblosc()
    if lib is None:
        pytest.skip("no libblosc on this host")
    for label, arr, frame_bytes, blocksize in CASES:
        raw = arr.reshape(-1).view(np.uint8)
        for f, frame in enumerate(encode_frames_host(arr, frame_bytes, blocksize)):
            assert np.array_equal(libblosc_decode(lib, frame, frame_bytes), _want(raw, f, frame_bytes)), (label, f)
