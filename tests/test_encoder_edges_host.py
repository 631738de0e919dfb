"""The host twin of the device blosc-zstd encoder on the cases of ``tests/encoder_cases.py`` (no GPU).

The twin is the specification of ``tests/test_encoder_edges_gpu.py`` (the kernels must write its bytes), so here its frames
are held to two decoders that share nothing with it -- the system libzstd behind ``lsr_blosc_decode_host`` and the
Python frame walker -- and a census asserts that the cases reach the lane-run partitions, plane modes, header sizes and
description forms they are named for.  A case that misses its census is changed until it holds; none is dropped.
"""

import functools

import numpy as np
import pytest

from shrimpy_amd.io import codecs
from shrimpy_amd.io.device_codec import encode_frames_host
from tests import encoder_cases as ec


@functools.lru_cache(maxsize=None)
def _sweep_frames(n, T):
    _, arr, frame_bytes, blocksize = ec.sweep_case(n, T)
    return arr, encode_frames_host(arr, frame_bytes, blocksize)


def _check_decodes(label, arr, frame_bytes, frames):
    want = ec.padded(arr, frame_bytes)
    assert len(frames) == len(want), label
    for f, frame in enumerate(frames):
        h = codecs.blosc_header(frame)
        assert (h["nbytes"], h["cbytes"], h["typesize"], h["compressor"]) == (frame_bytes, len(frame), arr.dtype.itemsize, "zstd"), label
        assert np.array_equal(codecs.blosc_decode(frame, backend="lsrecon"), want[f]), f"{label}, frame {f}: system libzstd disagrees"
        got = np.empty(frame_bytes, np.uint8)
        codecs._py_blosc_decode(frame, got)
        assert np.array_equal(got, want[f]), f"{label}, frame {f}: the Python walker disagrees"


def _check_case(case):
    label, arr, frame_bytes, blocksize = case
    _check_decodes(label, arr, frame_bytes, encode_frames_host(arr, frame_bytes, blocksize))


@pytest.mark.parametrize("P", ec.SWEEP_P)
@pytest.mark.parametrize("T", ec.SWEEP_T)
def test_twin_frames_of_the_lane_run_sweep_decode(T, P):
    for n in ec.sweep_lengths(P):
        arr, frames = _sweep_frames(n, T)
        _check_decodes(f"T={T} n={n}", arr, n * T, frames)


@pytest.mark.parametrize("T", ec.SWEEP_T)
def test_twin_frames_at_the_shortest_and_longest_planes_decode(T):
    for n in ec.END_LENGTHS:
        arr, frames = _sweep_frames(n, T)
        _check_decodes(f"T={T} n={n}", arr, n * T, frames)


def _groups():
    return ([("mode mixes", ec.mix_cases), ("uniform waves", ec.uniform_wave_cases)]
            + [(f"source edges T={T}", functools.partial(ec.source_edge_cases, T)) for T in (4, 2, 1)]
            + [("many blocks", ec.many_block_cases), ("code construction", ec.code_cases),
               ("buffer volumes", lambda: [(f"volume {k}", v, v.nbytes, 0) for k, v in enumerate(ec.buffer_volumes())])])


@pytest.mark.parametrize("name,build", _groups(), ids=[g[0] for g in _groups()])
def test_twin_frames_of_every_other_case_decode(name, build):
    cases = build()
    assert cases
    for case in cases:
        _check_case(case)


def test_sweep_lengths_reach_every_lane_run_partition():
    """``runs()`` over the plane lengths of the sweep that are Huffman-coded, for stream 0 (the run length of streams
    0..2, and of the LDS layout) and stream 3 (its own run length in that layout)."""
    lengths = sorted({n for P in ec.SWEEP_P for n in ec.sweep_lengths(P)} | set(ec.END_LENGTHS))
    lengths = [n for n in lengths if n >= ec.MIN_HUF_PLANE]
    for j in (0, 3):
        rs = [ec.runs(ec.stream_len(n, j)) for n in lengths]
        assert {r["c"] for r in rs} == {8, 16, 32, 64, 128, 256}, j
        merged = {(r["c"], r["last_len"] - r["c"]) for r in rs if r["merged"]}
        assert merged >= {(c, d) for c in (16, 32, 64, 128, 256) for d in range(1, 8)}, j
        assert any(not r["merged"] and r["last_len"] == 8 for r in rs), j
        assert {r["c"] for r in rs if r["last_len"] == r["c"]} == {8, 16, 32, 64, 128, 256}, j
        assert any(r["lanes"] == 64 for r in rs) and any(r["lanes"] < 64 for r in rs), j
        assert all(r["lanes"] <= 64 and r["last_len"] >= 8 and r["last_len"] <= r["c"] + 7 for r in rs), j
    # a stream of run length 8 has a merged tail only as stream 3 (stream 0 of a coded plane holds 512 symbols or more)
    tails8 = {r["last_len"] for r in (ec.runs(ec.stream_len(n, 3)) for n in lengths) if r["c"] == 8 and r["merged"]}
    assert tails8 == {14, 15}
    differ = [n for n in lengths if ec.runs(ec.stream_len(n, 0))["c"] != ec.runs(ec.stream_len(n, 3))["c"]]
    assert {2049, 2050} <= set(differ) and len(differ) >= 10
    # both sides of the literals header's 16384 and of the sample threshold
    assert {16383, 16384, 32767, 32768} <= set(lengths)


def test_sweep_planes_are_coded_from_2048_symbols_on_and_not_below():
    headers, forms = set(), set()
    for T in ec.SWEEP_T:
        for n in sorted({n for P in ec.SWEEP_P for n in ec.sweep_lengths(P)} | set(ec.END_LENGTHS)):
            for f, frame in enumerate(_sweep_frames(n, T)[1]):
                (block,) = ec.census(frame)
                if n < ec.MIN_HUF_PLANE:
                    assert block == "verbatim" or all(k in ("raw", "rle") for k in block), (T, n, f, block)
                    continue
                assert block != "verbatim" and len(block) == T and all(k[0] == "compressed" for k in block), (T, n, f, block)
                for _, lh, form in block:
                    assert lh == (4 if n < 16384 else 5), (T, n, f, block)      # (regenerated size below 16384 or not)
                    headers.add(lh)
                    forms.add(form)
    assert headers == {4, 5} and forms == {"nibble", "fse"}


def test_lane_boundaries_of_the_sweep_fall_on_every_bit_phase():
    """Pass B hands the ``skip`` = 0..7 bits in front of a lane's first byte boundary to the next lane.  With the twin's own
    code lengths (read from the nibble descriptions of its frames and checked against the stream sizes they state), summed
    per lane run: at every P and T the lane boundaries of the sweep take all eight phases, and so does the boundary in front
    of a merged last run, for streams 0..2 and for stream 3."""
    behind_merged = {(T, j == 3): set() for T in ec.SWEEP_T for j in (0, 3)}
    for T in ec.SWEEP_T:
        for P in ec.SWEEP_P:
            seen = set()
            for n in ec.sweep_lengths(P):
                if n < ec.MIN_HUF_PLANE:
                    continue
                arr, frames = _sweep_frames(n, T)
                for f, frame in enumerate(frames):
                    block = ec.padded(arr, n * T)[f]
                    for p, plane in enumerate(ec.walk(frame)[0]):
                        if plane["form"] != "nibble":
                            continue
                        lengths = ec.nibble_code_lengths(frame, plane)
                        for j, (r, skip) in enumerate(ec.lane_phases(block[p::T], lengths, ec.stream_sizes(frame, plane))):
                            seen |= {int(v) for v in skip[:-1]}
                            if r["merged"]:
                                behind_merged[T, j == 3].add(int(skip[-2]))
            assert seen == set(range(8)), (T, P, seen)
    assert all(v == set(range(8)) for v in behind_merged.values()), behind_merged


def test_the_search_for_a_long_fse_description_runs():
    """The search the module docstring of ``encoder_cases`` reports, at 1 / 100 of its length: planes get descriptions, all
    below 128 bytes, and none falls to Raw."""
    got = ec.search_long_fse_description(lambda plane: encode_frames_host(plane, plane.size, plane.size)[0], trials=40)
    assert got["described"] >= 20 and 0 < got["largest"] < 128 and got["found"] is None, got


def test_mixed_mode_cases_hold_the_plane_types_they_name():
    for T in (4, 2, 1):
        for names in ec.MIXES[T]:
            for n in ec.MIX_N:
                _, arr, frame_bytes, blocksize = ec.mix_case(names, n)
                (block,) = ec.census(encode_frames_host(arr, frame_bytes, blocksize)[0])
                got = block if block == "verbatim" else [k if isinstance(k, str) else k[0] for k in block]
                assert got == ec.expected_mix(names, n), (names, n, block)


def test_the_early_then_verbatim_case_is_one():
    """T = 4, n = 65536, planes (noise, noise, near_230, near_230): the sample rule sends planes 0 and 1 out raw during
    the histogram sweep (in the compressed layout), planes 2 and 3 pass both collision tests, are counted, get a code --
    and do not pay, so the block is written again, verbatim.  All of it evaluated here, from the rules."""
    n = ec.MAX_PLANE
    planes = ec.mix_planes(ec.EARLY_VERBATIM, n)
    sample = [ec.sample_ratio(p, 4) for p in planes]
    assert sample[0] <= 1 and sample[1] <= 1, sample            # hopeless on one vector in 16
    assert sample[2] > 1 and sample[3] > 1, sample              # not so
    assert ec.full_ratio(planes[2]) > 1 and ec.full_ratio(planes[3]) > 1
    arr = ec.interleave(planes)
    assert ec.census(encode_frames_host(arr, 4 * n, 4 * n)[0]) == ["verbatim"]
    # the same case in the buffer-reuse sequence, between a verbatim volume and a coded one
    kinds = [ec.census(encode_frames_host(v, v.nbytes, 0)[0])[0] for v in ec.buffer_volumes()]
    assert kinds[0] == "verbatim" and kinds[1] == "verbatim" and kinds[3] == ["rle"] * 4
    assert all(k[0] == "compressed" for k in kinds[2])


def test_uniform_wave_cases_have_waves_of_each_kind():
    """Per 1024-byte span of the block (what one wave holds in one step of the histogram sweep) and plane: uniform with the
    plane's value, uniform with another value, uniform zero padding, mixed, and a last partial span."""
    for label, arr, frame_bytes, _ in ec.uniform_wave_cases():
        T = arr.dtype.itemsize
        block = ec.padded(arr, frame_bytes)[0]
        seen = set()
        for p in range(T):
            plane = block[p::T]
            span = 1024 // T
            whole = plane[:plane.size // span * span].reshape(-1, span)
            uniform = (whole == whole[:, :1]).all(axis=1)
            seen |= {("uniform", int(v)) for v in whole[uniform, 0]} | ({"mixed"} if (~uniform).any() else set())
            assert plane.size % span, label
        values = {v for k in seen if k != "mixed" for v in [k[1]]}
        assert "mixed" in seen and len(values - {0}) >= 2, (label, seen)
        assert (0 in values) == ("source ends" in label), (label, seen)


def test_source_edge_cases_touch_what_they_name():
    for T in (4, 2, 1):
        frame_bytes, blocksize = ec.source_edge_geometry(T)
        assert frame_bytes == 2 * blocksize + 2052 * T and blocksize == 65536 * T
        valids = set()
        for _, arr, fb, bs in ec.source_edge_cases(T):
            assert (fb, bs) == (frame_bytes, blocksize)
            valids.add(arr.nbytes % frame_bytes % blocksize or blocksize)
        batch = 32768
        assert {16 - T, 16, 16 + T, batch - T, batch, batch + T, blocksize - T, blocksize} <= valids
        if T == 4:
            assert {4, 12, 16, 20, 32764, 32768, 32772, 65532, 65540, blocksize - 4, blocksize} <= valids


def test_many_block_and_code_cases_are_what_they_name():
    per_frame = [-(-fb // bs) for _, _, fb, bs in ec.many_block_cases()]
    assert per_frame == [256, 257, 513, 257]
    label, arr, fb, bs = ec.huffman_blocks_case()
    sizes = set()
    for frame in encode_frames_host(arr, fb, bs):
        starts = np.frombuffer(frame, "<u4", 257, 16)
        sizes |= {int(s) % 4 for s in starts}
        assert all(all(k[0] == "compressed" for k in block) for block in ec.census(frame))
    assert sizes == {0, 1, 2, 3}                     # every alignment of a block's place in the frame
    for label, arr, fb, bs in map(ec.small_block_case, ec.SMALL_BLOCKS_PER_FRAME):
        kinds = {str(b) for frame in encode_frames_host(arr, fb, bs) for b in ec.census(frame)}
        assert kinds == {"verbatim", "['rle']"}, (label, kinds)
    forms = {}
    for label, arr, fb, bs in ec.code_cases():
        (block,) = ec.census(encode_frames_host(arr, fb, bs)[0])
        assert block[0][0] == "compressed", label
        forms[label] = block[0][2]
        present = np.flatnonzero(np.bincount(arr, minlength=256))
        if "present" in label:
            assert present.size == int(label.split()[1]) and present[-1] == int(label.split("last at ")[1].split()[0]), label
    assert forms["code: two symbols far apart"] == "fse"
    assert forms["code: 128 present in 0..128, last at 128 (128 weights)"] == "nibble"      # the switch: 128 weights ...
    assert forms["code: 129 present in 0..129, last at 129 (129 weights)"] == "fse"         # ... and 129
    assert forms["code: 128 present, last at 255"] == "fse" and forms["code: 129 present, last at 255"] == "fse"
