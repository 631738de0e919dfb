"""Generate ``tests/golden/blosc_levels_*.npz``: what a REAL c-blosc (libblosc 1.21.0 from the build image, through
ctypes) writes with the zstd compressor at every compression level, for the device decoder's tests
(``tests/test_blosc_levels.py``, ``tests/test_device_decoder_levels_gpu.py``).  TEST INFRASTRUCTURE: run in the
build container, commit the output.

    python oracle/make_blosc_levels.py [/path/to/libblosc.so]

Written:

* ``blosc_levels_table.npz`` -- ``table``: one row ``(nbytes, clevel, typesize, shuffle, blocksize, flags, typesize
  written)`` per header c-blosc writes, for clevels 0-9, typesizes 2 and 4, shuffle 0 and 1, at the engine's chunk
  (512 x 256 x 2048 uint16), config 5's chunk (512 x 200 x 2048 uint16) and every fixture's ``nbytes``; ``meta``
  (JSON): the fixture groups, each with its data as a seeded recipe (``light_sheet``) and the SHA-1 of its bytes,
  and the 16-byte header c-blosc writes for a stored (incompressible) frame of the group's ``nbytes``; and what this
  run confirmed about c-blosc's zstd level rule.
* ``blosc_levels_frames_<k>.npz`` -- ``<group>``: the frame c-blosc wrote for that group, packed into files of at
  most 450 KB (a single frame above that gets a file of its own: the largest, 1 MB of uint16 at clevel 9 without
  shuffle, is 510 KB).

The headers of the two large chunks come from a compression that is refused for want of room (the destination
holds the header and the block table only): c-blosc writes the header first, and the recipe checks on every fixture
size that such a header equals the one of the finished frame.
"""

import ctypes
import hashlib
import json
import sys

from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden"
FILE_LIMIT = 450_000

ENGINE_CHUNK = 512 * 256 * 2048 * 2         # mantis_engine: z-chunk min(512, nz) of (nz, 256, 2048) uint16
CONFIG5_CHUNK = 512 * 200 * 2048 * 2


def light_sheet(seed: int, n: int, dtype: str) -> np.ndarray:
    """``n`` elements of a light-sheet-like plane stack, rows of 2048 pixels: a Poisson(100) background and a bright
    band (a Gaussian profile across rows, up to 1 500 counts above the background).  float32 = the counts / 8."""
    rng = np.random.default_rng(seed)
    row = np.arange(n) // 2048
    lam = 100.0 + 1500.0 * np.exp(-(((row % 512) - 180.0) / 24.0) ** 2)
    counts = rng.poisson(lam)
    if dtype == "uint16":
        return counts.astype(np.uint16)
    if dtype == "float32":
        return counts.astype(np.float32) * np.float32(0.125)
    raise ValueError(dtype)


def level_blocksize(clevel: int) -> int:
    return {0: 16, 1: 32, 2: 64, 3: 128, 4: 256, 5: 256, 6: 512, 7: 512, 8: 512, 9: 1024}[clevel] * 1024


def _groups():
    """(name, dtype, shuffle, clevel, nbytes): two full blocks and a ragged leftover (a quarter of a block plus 12
    bytes) at clevels 1-5; one full block at 6-9 (512 KB and 1 MB: the size of the fixtures)."""
    out = []

    def nbytes(cl):
        bs = level_blocksize(cl)
        return 2 * bs + bs // 4 + 12 if cl <= 5 else bs

    for cl in range(1, 10):
        out.append((f"u16_shuffle_c{cl}", "uint16", 1, cl, nbytes(cl)))
    for cl in (1, 4, 9):
        out.append((f"f32_shuffle_c{cl}", "float32", 1, cl, nbytes(cl)))
    for cl in (3, 9):
        out.append((f"u16_noshuffle_c{cl}", "uint16", 0, cl, nbytes(cl)))
    return out


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else "/opt/conda/lib/libblosc.so.1"
    b = ctypes.CDLL(lib)
    b.blosc_get_version_string.restype = ctypes.c_char_p
    b.blosc_compress_ctx.restype = ctypes.c_int
    b.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p,
                                     ctypes.c_size_t, ctypes.c_int]
    version = b.blosc_get_version_string().decode()
    print("libblosc", version)
    # the libzstd that libblosc itself calls (its dependency, found beside it): the level rule is checked against it
    z = ctypes.CDLL(str(Path(lib).resolve().parent / "libzstd.so.1"))
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    zmax = int(z.ZSTD_maxCLevel())

    def zstd(src: np.ndarray, level: int) -> bytes:
        cap = z.ZSTD_compressBound(src.size)
        buf = ctypes.create_string_buffer(cap)
        n = z.ZSTD_compress(buf, cap, src.ctypes.data, src.size, level)
        return buf.raw[:n]

    def compress(a: np.ndarray, clevel: int, shuffle: int, typesize: int, cap: int | None = None) -> bytes:
        cap = a.nbytes + 16 if cap is None else cap
        buf = ctypes.create_string_buffer(cap)
        n = b.blosc_compress_ctx(clevel, shuffle, typesize, a.nbytes, a.ctypes.data, buf, cap, b"zstd", 0, 1)
        return buf.raw[:n] if n > 0 else buf.raw[:16]

    def header_only(nbytes: int, clevel: int, shuffle: int, typesize: int) -> bytes:
        """The header c-blosc writes before it runs out of room (a destination of header + block table + 16)."""
        a = np.zeros(nbytes, np.uint8)                 # (pages never touched past the first block)
        nblocks = -(-nbytes // 1024)
        return compress(a, clevel, shuffle, typesize, cap=16 + 4 * nblocks + 16)[:16]

    groups = _groups()
    meta = {"libblosc": version, "groups": {}, "zstd_level_rule": {}}
    frames = {}
    for name, dtype, shuffle, cl, nbytes in groups:
        T = np.dtype(dtype).itemsize
        seed = 2000 + len(frames)
        data = light_sheet(seed, nbytes // T, dtype)
        frame = compress(data, cl, shuffle, T)
        assert len(frame) > 16 and not frame[2] & 0x2, f"{name}: c-blosc stored the frame"
        assert header_only(nbytes, cl, shuffle, T)[:12] == frame[:12], f"{name}: the refused compression's header differs"
        noise = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
        stored = compress(noise, cl, shuffle, T)
        assert stored[2] & 0x2 and len(stored) == nbytes + 16, f"{name}: noise was not stored"
        # c-blosc's zstd level: every block stream against the libzstd it links, at 2 clevel - 1 (clevel 9: the maximum)
        level = 2 * cl - 1 if cl < 9 else zmax
        bs = int.from_bytes(frame[8:12], "little")
        raw = data.view(np.uint8)
        same = True
        for k in range(-(-nbytes // bs)):
            blk = raw[k * bs:(k + 1) * bs]
            if shuffle:
                n = blk.size // T
                blk = np.concatenate([blk[:n * T].reshape(n, T).T.reshape(-1), blk[n * T:]])
            at = int.from_bytes(frame[16 + 4 * k:20 + 4 * k], "little")
            cb = int.from_bytes(frame[at:at + 4], "little")
            want = bytes(blk) if cb == blk.size else zstd(np.ascontiguousarray(blk), level)
            same &= frame[at + 4:at + 4 + cb] == want
        meta["zstd_level_rule"].setdefault(str(cl), {"zstd_level": level, "confirmed": True})
        meta["zstd_level_rule"][str(cl)]["confirmed"] &= bool(same)
        meta["groups"][name] = dict(dtype=dtype, shuffle=shuffle, clevel=cl, nbytes=nbytes,
                                    recipe=dict(fn="light_sheet", seed=seed, n=nbytes // T, dtype=dtype),
                                    sha1=hashlib.sha1(data.tobytes()).hexdigest(), stored_header=list(stored[:16]))
        frames[name] = np.frombuffer(frame, np.uint8)
        print(f"{name}: {nbytes} -> {len(frame)} bytes, blocksize {bs}, flags {frame[2]:#04x}, "
              f"stored flags {stored[2]:#04x}, zstd level {level} reproduced: {same}")
    sizes = sorted({ENGINE_CHUNK, CONFIG5_CHUNK} | {g[4] for g in groups})
    rows = []
    for nbytes in sizes:
        for cl in range(10):
            for T in (2, 4):
                for shuffle in (0, 1):
                    h = header_only(nbytes, cl, shuffle, T)
                    assert int.from_bytes(h[4:8], "little") == nbytes
                    rows.append((nbytes, cl, T, shuffle, int.from_bytes(h[8:12], "little"), h[2], h[3]))
    table = np.array(rows, dtype=np.int64)
    np.savez_compressed(OUT / "blosc_levels_table.npz", table=table, meta=np.array(json.dumps(meta, sort_keys=True)))
    print("level table (nbytes = engine chunk, typesize 2, shuffle 1):")
    for r in rows:
        if r[0] == ENGINE_CHUNK and r[2] == 2 and r[3] == 1:
            print(f"  clevel {r[1]}: blocksize {r[4]}, flags {r[5]:#04x}")
    # frames, greedily packed into files below the size limit (in the order above)
    part, size, k = {}, 0, 0
    for name, _, _, _, _ in groups:
        f = frames[name]
        if part and size + f.size > FILE_LIMIT:
            np.savez(OUT / f"blosc_levels_frames_{k}.npz", **part)
            part, size, k = {}, 0, k + 1
        part[name] = f
        size += f.size
    np.savez(OUT / f"blosc_levels_frames_{k}.npz", **part)
    for p in sorted(OUT.glob("blosc_levels_*.npz")):
        print(f"wrote {p.name}: {p.stat().st_size} bytes")


if __name__ == "__main__":
    main()
