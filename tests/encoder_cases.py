"""Inputs that steer the device blosc-zstd encoder (``csrc/blosc_encode.hip``) to every edge of its geometry, and a
census that says what a frame of the host twin holds.  NumPy only (the package's codecs are not used), fixed seeds; shared by
``tests/test_encoder_edges_host.py`` (no GPU) and ``tests/test_encoder_edges_gpu.py``.

The existing cases of ``tests/test_device_codec.py`` were picked for their byte statistics.  These are picked for the
kernel's shape: the lane runs of ``stream_runs`` (restated in :func:`runs`, used only to NAME the partition a plane
length reaches), the plane-length thresholds 2048 / 16384 / 32768, the wave-uniform histogram shortcut, the batches of
``load_ahead`` and the frame assembly.  A case is an ``(id, elements, frame_bytes, blocksize)`` tuple: ``elements`` is
cut into frames of ``frame_bytes`` (the last one zero-padded) of blocks of ``blocksize``.

The branch of ``huf_description_size`` that returns -1 -- more than 128 weights whose FSE stream does not stay below
128 bytes, so a plane that would pay falls to Raw -- is NOT reached by any case here.  A deterministic search
(:func:`search_long_fse_description` with the host twin as its encoder, well under a minute of one core; a short run of
it is a test in ``tests/test_encoder_edges_host.py``) drew 4000 complete length profiles over 256 present symbols, grown by
random leaf splits with five depth biases, the lengths dealt to the symbols at random, in planes of 16384 bytes with
counts ``8 * 2^(11 - length)`` so that the tree is the profile.  All 4000 planes got a tree description, each in the FSE
form; the largest took 91 bytes, and no plane fell to Raw.  Under the Kraft sum (at most ``2^l`` symbols of length ``l``)
the weights of 256 symbols cannot be spread evenly over the twelve values, which is what a stream of 3.9 bits per weight
would take.  The branch is recorded here as unreached, not as impossible.
"""

import functools

import numpy as np

MIN_HUF_PLANE = 2048          # kMinHufPlane
SAMPLE_EVERY = 16             # kSampleEvery
MAX_PLANE = 65536             # kMaxDevPlane

ELEMENT = {1: np.uint8, 2: np.int16, 4: np.int32}      # (dtypes torch takes as they are)


def interleave(planes):
    """Elements of typesize ``T = len(planes)`` whose byte shuffle gives back exactly ``planes``."""
    planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
    assert len(planes) in ELEMENT and all(p.shape == planes[0].shape and p.ndim == 1 for p in planes)
    return np.stack(planes, axis=1).reshape(-1).view(ELEMENT[len(planes)])


# ---------------------------------------------------------------------------------------------------------------------
# plane profiles: n bytes from (n, seed)
# ---------------------------------------------------------------------------------------------------------------------

def huf_deep(n, seed=0):
    """2^-k over 39 symbols: code lengths up to the 11-bit limit."""
    p = 0.5 ** np.arange(1, 40)
    return np.random.default_rng(seed).choice(39, n, p=p / p.sum()).astype(np.uint8)


def huf_3(n, seed=0):
    return np.random.default_rng(seed).integers(0, 3, n).astype(np.uint8)


def huf_fse(n, seed=0):
    """More than 128 weights: the tree description is an FSE stream."""
    return np.random.default_rng(seed).geometric(0.02, n).astype(np.uint8)


def huf_two_far(n, seed=0):
    """Symbols {0, 255} with counts (n - 1, 1): max_bits 1, 255 weights, the largest count of a sort key."""
    out = np.zeros(n, np.uint8)
    out[int(np.random.default_rng(seed).integers(0, n))] = 255
    return out


def huf_ties(n, seed=0):
    """All counts equal or off by one: the order of the leaves is decided by the symbol."""
    return ((np.arange(n) + seed) % 37).astype(np.uint8)


def noise(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)


def rle(n, seed=0):
    return np.full(n, 1 + seed % 255, np.uint8)


def near_230(n, seed=0):
    """Uniform over 230 symbols: not hopeless by the collision tests, yet no prefix code saves 1/64 of it."""
    return np.random.default_rng(seed).integers(0, 230, n).astype(np.uint8)


def mostly_const(n, seed=0, span=1024):
    """One non-zero value but for: every third span of ``span`` symbols (the symbols of this plane that one wave holds
    in one step of the histogram sweep) carries a few other values, spans 2 and 5 are uniform with ANOTHER value, and
    whatever follows the last whole span is a partial wave."""
    rng = np.random.default_rng(seed)
    value, other = 7 + seed % 100, 201 + seed % 50
    out = np.full(n, value, np.uint8)
    for k in range(n // span + 1):
        lo, hi = k * span, min((k + 1) * span, n)
        if hi <= lo:
            break
        if k in (2, 5) and hi - lo == span:
            out[lo:hi] = other
        elif k % 3 == 1:
            at = rng.integers(lo, hi, 3)
            out[at] = rng.integers(0, 256, 3)
            out[lo if k % 2 else hi - 1] = value ^ 0x80       # (the first / the last lane of the wave)
    return out


PROFILES = {f.__name__: f for f in (huf_deep, huf_3, huf_fse, huf_two_far, huf_ties, noise, rle, near_230, mostly_const)}
HUF_SWEEP = (huf_deep, huf_3, huf_fse, huf_ties)     # every one is Huffman-coded at every plane length >= 2048


def planes_of(names, n, seed=0):
    return [PROFILES[name](n, seed + 17 * p) for p, name in enumerate(names)]


# ---------------------------------------------------------------------------------------------------------------------
# restatement of stream_runs / huf_stream_len (to name partitions, never to produce bytes)
# ---------------------------------------------------------------------------------------------------------------------

def stream_len(n, j):
    q = (n + 3) // 4
    return q if j < 3 else n - 3 * q


def runs(m):
    """The lane runs of a stream of ``m`` symbols: run length ``c``, lanes in use, length of the last lane's run and
    whether a tail shorter than 8 was merged into it."""
    c = 1
    while c < (m + 63) // 64:
        c *= 2
    c = max(c, 8)
    lanes = (m + c - 1) // c
    last_len = m - (lanes - 1) * c
    merged = last_len < 8 and lanes > 1
    if merged:
        lanes -= 1
        last_len += c
    return dict(c=c, lanes=lanes, last_len=last_len, merged=merged)


# ---------------------------------------------------------------------------------------------------------------------
# census: what a frame holds, read from the format (c-blosc 1.x header, RFC 8878)
# ---------------------------------------------------------------------------------------------------------------------

def walk(frame):
    """Per blosc block of ``frame``: ``"verbatim"`` (cbytes == the block's size) or one dict per zstd block -- ``kind``
    ("raw" / "rle" / "compressed") and, for a compressed one, ``header`` (bytes of the literals header), ``form`` of the
    tree description ("nibble" / "fse"), ``at`` (where the description starts) and ``size`` (description, jump table
    and the four streams)."""
    b = bytes(frame)
    u32 = lambda at: int.from_bytes(b[at:at + 4], "little")
    assert b[0] == 2 and b[2] >> 5 == 4, "not a blosc 1.x frame of the zstd compressor"
    typesize, nbytes, blocksize, cbytes = b[3], u32(4), u32(8), u32(12)
    assert cbytes == len(b)
    nblocks = -(-nbytes // blocksize)
    out = []
    for k in range(nblocks):
        at = u32(16 + 4 * k)
        bsize = min(blocksize, nbytes - k * blocksize)
        csize = u32(at)
        end = at + 4 + csize
        assert end <= len(b)
        if csize == bsize:
            out.append("verbatim")
            continue
        at += 4
        assert b[at:at + 4] == b"\x28\xb5\x2f\xfd" and b[at + 4] == 0xA0 and u32(at + 5) == bsize
        at += 9
        planes, regenerated, last = [], 0, False
        while not last:
            head = int.from_bytes(b[at:at + 3], "little")
            last, kind, size = bool(head & 1), (head >> 1) & 3, head >> 3
            at += 3
            if kind == 0:
                planes.append(dict(kind="raw"))
                regenerated += size
                at += size
            elif kind == 1:
                planes.append(dict(kind="rle"))
                regenerated += size
                at += 1
            else:
                assert kind == 2
                lit = b[at]
                assert lit & 3 == 2, "literals are not Huffman-compressed"
                fmt = (lit >> 2) & 3
                assert fmt in (2, 3), "four streams with a 4- or 5-byte header"
                lh = 4 if fmt == 2 else 5
                word = int.from_bytes(b[at:at + lh], "little")
                regen = (word >> 4) & (0x3FFF if lh == 4 else 0x3FFFF)
                comp = (word >> (18 if lh == 4 else 22)) & (0x3FFF if lh == 4 else 0x3FFFF)
                assert size == lh + comp + 1 and b[at + size - 1] == 0, "literals, then an empty sequences section"
                planes.append(dict(kind="compressed", header=lh, form="fse" if b[at + lh] < 128 else "nibble",
                                   at=at + lh, size=comp))
                regenerated += regen
                at += size
        assert at == end and regenerated == bsize and len(planes) == typesize
        out.append(planes)
    return out


def census(frame):
    """:func:`walk` in short: per block ``"verbatim"`` or the list of ``"raw"``, ``"rle"`` or
    ``("compressed", literals-header bytes, "nibble" | "fse")``."""
    return [blk if blk == "verbatim" else [p["kind"] if p["kind"] != "compressed" else ("compressed", p["header"], p["form"])
                                           for p in blk] for blk in walk(frame)]


def description_bytes(frame, plane):
    """Bytes of the tree description of a compressed plane (an entry of :func:`walk`), its head byte included."""
    head = bytes(frame)[plane["at"]]
    return 1 + head if head < 128 else 1 + (head - 127 + 1) // 2


def nibble_code_lengths(frame, plane):
    """Code length of every symbol (0: absent) from a description in the nibble form: weights of the symbols but the
    last present one, whose weight completes ``sum 2^(w - 1)`` to a power of two; length = max_bits + 1 - weight."""
    b = bytes(frame)
    nw = b[plane["at"]] - 127
    assert plane["form"] == "nibble" and 1 <= nw <= 128
    body = b[plane["at"] + 1:plane["at"] + 1 + (nw + 1) // 2]
    w = [(body[k // 2] >> (0 if k % 2 else 4)) & 15 for k in range(nw)]
    total = sum(1 << (x - 1) for x in w if x)
    max_bits = total.bit_length()
    rest = (1 << max_bits) - total
    assert rest & (rest - 1) == 0 and rest > 0
    w.append(rest.bit_length())
    lengths = np.zeros(256, np.int64)
    lengths[:len(w)] = [max_bits + 1 - x if x else 0 for x in w]
    return lengths


def stream_sizes(frame, plane):
    """Bytes of the four Huffman streams of a compressed plane (the jump table holds the first three)."""
    b = bytes(frame)
    at = plane["at"] + description_bytes(frame, plane)
    three = [int.from_bytes(b[at + 2 * j:at + 2 * j + 2], "little") for j in range(3)]
    return three + [plane["size"] - description_bytes(frame, plane) - 6 - sum(three)]


def lane_phases(symbols, lengths, sizes):
    """For each stream of a coded plane: ``(runs, skip)`` with ``skip[l]`` = the bits in front of lane l's first byte
    boundary, which pass B hands to lane l + 1 (streams are written last symbol first, so the bits of the lanes above l
    lie in front of its run).  ``lengths`` are the twin's (read from its frame); that they are is checked against the
    stream sizes the frame states."""
    out, at = [], 0
    for j in range(4):
        m = stream_len(symbols.size, j)
        r = runs(m)
        bits = lengths[symbols[at:at + m]]
        at += m
        assert bits.min() >= 1 and (int(bits.sum()) + 1 + 7) // 8 == sizes[j]
        starts = np.arange(r["lanes"]) * r["c"]
        per_lane = np.add.reduceat(bits, starts)
        in_front = per_lane[::-1].cumsum()[::-1] - per_lane
        out.append((r, (8 - in_front % 8) % 8))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's two "hopeless" rules, in NumPy
# ---------------------------------------------------------------------------------------------------------------------

def sample_ratio(plane, typesize):
    """``235 * sum c (c - 1) / (n (n - 1))`` over the sampled symbols: one 16-byte vector of the block in 16.  The plane
    is hopeless on the sample (stored raw, never counted) when this is <= 1."""
    per = 16 // typesize
    idx = np.arange(plane.size)
    c = np.bincount(plane[(idx // per) % SAMPLE_EVERY == 0], minlength=256).astype(np.int64)
    n = int(c.sum())
    return 235 * int((c * (c - 1)).sum()) / (n * (n - 1))


def full_ratio(plane):
    """``235 * sum c^2 / n^2`` over the whole plane: hopeless when <= 1."""
    c = np.bincount(plane, minlength=256).astype(np.int64)
    return 235 * int((c * c).sum()) / int(plane.size) ** 2


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------

SWEEP_P = (2048, 4096, 8192, 16384, 32768)
SWEEP_T = (1, 2, 4)


def sweep_lengths(P):
    return list(range(P - 4, P + 34))


def sweep_volume(n, T):
    """Three one-block frames of plane length ``n``, the Huffman profiles dealt to the planes differently in each."""
    frames = [interleave([HUF_SWEEP[(p + k) % len(HUF_SWEEP)](n, 100 * k + p) for p in range(T)]) for k in range(3)]
    return np.concatenate(frames)


def sweep_case(n, T):
    return (f"sweep T={T} n={n}", sweep_volume(n, T), n * T, n * T)


END_LENGTHS = (2044, 2045, 2046, 2047, 2048, 65533, 65534, 65535, 65536)

MIX_N = (32767, 32768, 65536)
MIXES = {
    4: [("noise", "huf_deep", "rle", "huf_3"), ("huf_deep", "noise", "rle", "noise"), ("noise", "noise", "noise", "huf_fse"),
        ("noise",) * 4, ("noise", "noise", "near_230", "near_230"), ("rle",) * 4],
    2: [("noise", "huf_deep"), ("huf_deep", "noise")],
    1: [(name,) for name in ("huf_deep", "huf_3", "huf_fse", "huf_two_far", "huf_ties", "noise", "rle", "near_230", "mostly_const")],
}
MIX_TYPE = {"noise": "raw", "near_230": "raw", "rle": "rle"}      # every other profile: compressed
EARLY_VERBATIM = ("noise", "noise", "near_230", "near_230")
EARLY_SEED = 5


def mix_planes(names, n):
    if tuple(names) == EARLY_VERBATIM:        # (the seeds the early-then-verbatim conditions were established with)
        rng = np.random.default_rng(EARLY_SEED)
        return [rng.integers(0, 256 if name == "noise" else 230, n).astype(np.uint8) for name in names]
    return planes_of(names, n, seed=40)


def mix_case(names, n):
    return (f"mix {'/'.join(names)} n={n}", interleave(mix_planes(names, n)), n * len(names), n * len(names))


def mix_cases():
    return [mix_case(names, n) for T in (4, 2, 1) for names in MIXES[T] for n in MIX_N]


def expected_mix(names, n):
    """Per-plane types a mixed-mode block must have (a block none of whose planes compresses is verbatim)."""
    assert n >= MIN_HUF_PLANE
    kinds = [MIX_TYPE.get(name, "compressed") for name in names]
    return "verbatim" if all(k == "raw" for k in kinds) else kinds


UNIFORM_N = 16 * 1024 + 333        # whole wave spans and a partial one, for T = 1 (1024 symbols) and T = 4 (256)


def uniform_wave_cases():
    out = []
    n = UNIFORM_N
    deep = [huf_deep(n, 60 + p) for p in range(4)]
    volumes = [("T=1", [mostly_const(n, 3, span=1024)]),
               ("T=4", [deep[0], mostly_const(n, 3, span=256), deep[2], deep[3]]),
               ("T=4, two such planes", [mostly_const(n, 5, span=256), deep[1], deep[2], mostly_const(n, 4, span=256)])]
    for label, planes in volumes:
        T = len(planes)
        arr = interleave(planes)
        out.append((f"uniform waves {label}", arr, n * T, n * T))
        # the source ends inside the block, a few bytes into a wave span: uniform waves of zeros behind it
        cut = (9 * 1024 + 48) // T
        out.append((f"uniform waves {label}, source ends in the block", arr[:cut].copy(), n * T, n * T))
    return out


def source_edge_geometry(T):
    """(frame_bytes, blocksize) of the source-edge cases: two whole blocks and a tail block of 2052 elements."""
    blocksize = MAX_PLANE * T
    return 2 * blocksize + 2052 * T, blocksize


def source_edge_valid(T):
    """Bytes of the last touched block that come from the source: both sides of a 16-byte vector (``load_block16``'s
    whole-vector test), of the 32768-byte batches of ``load_ahead``, and of the block's end."""
    _, bsize = source_edge_geometry(T)
    want = {4, 12, 16, 20, T, 16 - T, 16 + T, 32768 - T, 32768, 32768 + T, 65536 - T, 65536, 65536 + T, bsize - T, bsize}
    return sorted(v for v in want if 0 < v <= bsize and v % T == 0)


@functools.lru_cache(maxsize=None)
def _source_edge_volume(T):
    """Two frames: Huffman-coded planes beside a noise plane, then noise beside Huffman-coded planes in the other order
    (T = 1: one of each), so the histogram, staging and raw sweeps over a block all meet the edge."""
    fe = source_edge_geometry(T)[0] // T
    names = ("huf_deep", "noise", "huf_3", "huf_fse")
    first = interleave(planes_of(names[:T], fe, seed=70))
    second = interleave(planes_of(names[:T][::-1] if T > 1 else ("noise",), fe, seed=71))
    return np.concatenate([first, second])


def source_edge_case(T, frame, block, valid):
    """The source ends ``valid`` bytes into ``block`` of ``frame``; the blocks behind it lie wholly beyond it (valid = 0)."""
    frame_bytes, blocksize = source_edge_geometry(T)
    elems = (frame * frame_bytes + block * blocksize + valid) // T
    where = "the tail block" if block == 2 else f"block {block}"
    return (f"source edge T={T} valid={valid} in {where} of frame {frame}", _source_edge_volume(T)[:elems].copy(),
            frame_bytes, blocksize)


def source_edge_cases(T):
    """The edge in block 0 of frame 0, in block 1 of frame 1, and in the tail block (plane length 2052: still coded)."""
    out = [source_edge_case(T, frame, block, valid) for valid in source_edge_valid(T) for frame, block in ((0, 0), (1, 1))]
    tail = sorted({4, 12, 16, 20, T, 16 - T, 16 + T, 2052 * T - T, 2052 * T})
    return out + [source_edge_case(T, 0, 2, valid) for valid in tail if valid % T == 0]


SMALL_BLOCKS_PER_FRAME = (256, 257, 513)


def small_block_case(bpf):
    """Two frames (the second one short of 3 blocks) of ``bpf`` blocks of 64 bytes, constant and noise blocks mixed."""
    rng = np.random.default_rng(bpf)
    blocks = [np.full(64, 1 + k % 200, np.uint8) if rng.random() < 0.5 else rng.integers(0, 256, 64).astype(np.uint8)
              for k in range(2 * bpf - 3)]
    return (f"{bpf} blocks of 64 bytes per frame", np.concatenate(blocks), 64 * bpf, 64)


def huffman_blocks_case():
    """257 blocks of four Huffman-coded planes of 2048 symbols: block sizes vary, so their places in the frame take every
    alignment."""
    n = 2048
    blocks = [interleave([HUF_SWEEP[(p + k) % 4](n, 900 + 4 * k + p) for p in range(4)]) for k in range(257)]
    return ("257 Huffman blocks per frame", np.concatenate(blocks), 257 * n * 4, n * 4)


def many_block_cases():
    return [small_block_case(bpf) for bpf in SMALL_BLOCKS_PER_FRAME] + [huffman_blocks_case()]


def _present(symbols, n, seed):
    """A plane of ``n`` bytes in which exactly ``symbols`` occur, with geometric-like counts (so that it pays)."""
    rng = np.random.default_rng(seed)
    symbols = np.asarray(symbols)
    p = 0.97 ** np.arange(symbols.size)
    out = symbols[rng.choice(symbols.size, n, p=p / p.sum())].astype(np.uint8)
    out[:symbols.size] = symbols
    rng.shuffle(out)
    return out


def fibonacci_bytes():
    """Exact Fibonacci counts: the deepest tree 46364 bytes can make (cut to the 11-bit limit)."""
    counts = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711]
    arr = np.concatenate([np.full(c, i, np.uint8) for i, c in enumerate(counts)])
    np.random.default_rng(0).shuffle(arr)
    return arr[:arr.size // 4 * 4].copy()


def code_cases():
    n = 4096
    cases = [
        ("two symbols far apart", huf_two_far(n, 1), n),
        ("counts tied", huf_ties(n, 0), n),
        ("Fibonacci counts", fibonacci_bytes(), 46364),
        ("128 present, last at 255", _present(np.r_[np.arange(0, 254, 2), 255], n, 11), n),
        ("129 present, last at 255", _present(np.r_[np.arange(0, 256, 2), 255], n, 12), n),
        ("128 present in 0..128, last at 128 (128 weights)", _present(np.r_[np.arange(0, 127), 128], n, 13), n),
        ("129 present in 0..129, last at 129 (129 weights)", _present(np.r_[np.arange(0, 128), 129], n, 14), n),
    ]
    return [(f"code: {label}", arr, fb, fb) for label, arr, fb in cases]


def buffer_volumes(n=MAX_PLANE):
    """Four volumes of one size whose frames differ in kind: what one leaves in the buffers the next must not keep."""
    return [interleave(planes_of(("noise",) * 4, n, seed=80)), interleave(mix_planes(EARLY_VERBATIM, n)),
            sweep_volume(n, 4)[:n].copy(), interleave(planes_of(("rle",) * 4, n, seed=81))]


def padded(arr, frame_bytes):
    """The bytes the frames of ``arr`` must decode to: ``(n_frames, frame_bytes)``, zero behind the source."""
    raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    n_frames = -(-raw.size // frame_bytes)
    out = np.zeros(n_frames * frame_bytes, np.uint8)
    out[:raw.size] = raw
    return out.reshape(n_frames, frame_bytes)


# ---------------------------------------------------------------------------------------------------------------------
# the search for an FSE description of 128 bytes or more (module docstring)
# ---------------------------------------------------------------------------------------------------------------------

def random_length_profile(rng, bias):
    """Code lengths (<= 11) of a complete prefix code over 256 symbols, grown by splitting random leaves; ``bias``
    weighs a leaf of depth d by ``bias^d`` (> 1: deep and skewed trees, < 1: flat ones)."""
    leaves = [0]
    while len(leaves) < 256:
        can = [i for i, d in enumerate(leaves) if d < 11]
        w = np.array([bias ** leaves[i] for i in can], np.float64)
        i = can[int(rng.choice(len(can), p=w / w.sum()))]
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    return rng.permutation(np.array(leaves))


SEARCH_SCALE = 8        # counts 8 * 2^(11 - length): planes of 16384 bytes, where a code of up to 7.8 bits per symbol pays


def plane_of_lengths(lengths, rng):
    """A plane whose Huffman tree has exactly these lengths: counts proportional to 2^(11 - length) (the Kraft sum is one)."""
    out = np.repeat(np.arange(256), SEARCH_SCALE * 2 ** (11 - lengths)).astype(np.uint8)
    assert out.size == SEARCH_SCALE * 2048
    rng.shuffle(out)
    return out


def search_long_fse_description(encode, trials=4000):
    """``encode(plane) -> frame`` (the host twin, T = 1, one block).  Returns ``described`` (trials whose plane got a tree
    description: the others are hopeless by the collision test, flat profiles mostly), ``largest`` (bytes of the largest
    FSE description among them) and ``found`` (the first plane stored Raw although it is not hopeless and its code would
    pay with a description of 128 bytes, or None)."""
    rng = np.random.default_rng(2024)
    described, largest, found = 0, 0, None
    for t in range(trials):
        lengths = random_length_profile(rng, (0.8, 1.0, 1.2, 1.4, 1.7)[t % 5])
        plane = plane_of_lengths(lengths, rng)
        frame = encode(plane)
        block = walk(frame)[0]
        if block != "verbatim" and block[0]["kind"] == "compressed":
            assert block[0]["form"] == "fse"
            described += 1
            largest = max(largest, description_bytes(frame, block[0]))
            continue
        payload = (SEARCH_SCALE * int((2 ** (11 - lengths) * lengths).sum()) + 7) // 8
        if full_ratio(plane) > 1 and 128 + 6 + payload + 10 < plane.size - plane.size // 64 and found is None:
            found = plane
    return dict(described=described, largest=largest, found=found)
