"""What every stencil entry point of csrc/correlate.hip answers on a machine WITHOUT a GPU: a call that its validation
rejects ends with the library's negative code, one that passes ends in the HIP runtime with a status >= 0 (there is no
device to launch on) -- the property tools/fuzz_device_args.py rests on.  Recorded per call: the negative code exactly,
or "ok" for any status >= 0 (the positive value belongs to the HIP runtime).  For the pure host functions
(lsr_sep_padded_shape, the *_supported / *_taps_count, the three *_prepare_taps) the value and the output array are
recorded too, exactly (the output as the sha256 of its bytes).

    python -m oracle.record_stencil_entry_statuses      # rewrites tests/golden/stencil_entry_statuses.json

Run it on the commit whose statuses are to be kept; tests/test_stencil_entry_statuses.py replays the same rows against
the library under test.  Per entry: a hand-written baseline that passes validation; one row per requirement of the
entry, the baseline with exactly that condition broken (``BREAKS``); and ``DRAWS`` seeded draws from the value pools of
the fuzzer, stored as seed + count, never as argument lists.

Pointers are host buffers nobody dereferences, except the documented host-pointer arguments (taps, shape outputs),
which point at slots sized for the documented maxima.  NEVER run this where a device is visible: a row that passes
validation would launch on host pointers.
"""

from __future__ import annotations

import ctypes
import hashlib
import json

from pathlib import Path

import numpy as np

FIXTURE = Path(__file__).resolve().parent.parent / "tests" / "golden" / "stencil_entry_statuses.json"
SEED = 20261017
DRAWS = 300
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ARG = -1, -2, -3, -4

# the fuzzer's pools (tools/fuzz_device_args.py)
INTS = [-(1 << 40), -1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 15, 16, 17, 63, 64, 65, 100, 256, 1000, 2048, 4096, 65535, 65536,
        (1 << 30) - 1, 1 << 30, (1 << 31) - 1, 1 << 31, 1 << 32, 1 << 40, (1 << 62)]
SMALL = [-1, 0, 1, 2, 3, 4, 5, 7, 9, 15, 16, 17, 256, 257, (1 << 31) - 1]
FLOATS = [0.0, -0.0, 1.0, -1.0, 0.5, 1e-6, 1e30, float("inf"), float("nan")]
BAD_EXTENTS = [-(1 << 40), -1, 0, 1 << 30, 1 << 31, 1 << 40, 1 << 62]

SLOT = 1 << 16          # bytes between two pointer slots: 16384 floats, more than any tap block or PSF (15^3 floats)
Z, Y, X = 6, 20, 70     # the baseline volume; its padded shape for 3 x 3 x 3 taps (asserted when the rows are built)
ROWS, PITCH = 36, 192
PLANE = ROWS * PITCH

# Argument kinds: p<k> = pointer slot k, n = NULL stream, i = int, l = int64, f = float.  (name, kind, baseline value)
_VOL = [("Z", "l", Z), ("Y", "l", Y), ("X", "l", X)]
_STRIDED = [("in", "p", 0), ("in_pitch", "l", PITCH), ("in_plane", "l", PLANE), ("aux", "p", 1), ("aux_pitch", "l", PITCH),
            ("aux_plane", "l", PLANE), ("out", "p", 2), ("out_pitch", "l", PITCH), ("out_plane", "l", PLANE)] + _VOL
_RL_HEAD = [("y", "p", 0), ("y_pitch", "l", PITCH), ("y_plane", "l", PLANE), ("init_from_y", "i", 1)]
_TAPS = [("pz", "i", 3), ("py", "i", 3), ("px", "i", 3)]
_NORMS = [("nz", "p", 6), ("ny", "p", 7), ("nx", "p", 8)]
_TAIL = [("stats", "p", None), ("stream", "n", None)]
ENTRIES = {
    "lsr_correlate_sep_stats_f32": [("in", "p", 0), ("out", "p", 2), ("aux", "p", 1)] + _VOL + [
        ("wz", "p", 3), ("pz", "i", 3), ("wy", "p", 4), ("py", "i", 3), ("wx", "p", 5), ("px", "i", 3),
        ("epilogue", "i", 2), ("eps", "f", 1e-6)] + _NORMS + _TAIL,
    "lsr_correlate_dense_stats_f32": [("in", "p", 0), ("out", "p", 2), ("aux", "p", 1)] + _VOL + [("w", "p", 3)] + _TAPS + [
        ("epilogue", "i", 2), ("eps", "f", 1e-6), ("norm_table", "p", 9)] + _TAIL,
    "lsr_correlate_sep_strided_stats_f32": _STRIDED + [
        ("wz", "p", 3), ("pz", "i", 3), ("wy", "p", 4), ("py", "i", 3), ("wx", "p", 5), ("px", "i", 3),
        ("epilogue", "i", 2), ("eps", "f", 1e-6)] + _NORMS + _TAIL,
    "lsr_rl_sep_stats_f32": _RL_HEAD + [("x_pad", "p", 1), ("ratio_pad", "p", 2), ("x_out", "p", 10)] + _VOL + [
        ("kz", "p", 3), ("kz_flipped", "p", 3), ("pz", "i", 3), ("ky", "p", 4), ("ky_flipped", "p", 4), ("py", "i", 3),
        ("kx", "p", 5), ("kx_flipped", "p", 5), ("px", "i", 3)] + _NORMS + [("iters", "i", 2), ("eps", "f", 1e-6)] + _TAIL,
    "lsr_rl_sep_fused_stats_f32": _RL_HEAD + [("x_a", "p", 1), ("x_b", "p", 2), ("x_out", "p", 10)] + _VOL + [
        ("taps", "p", 3)] + _TAPS + _NORMS + [("iters", "i", 2), ("eps", "f", 1e-6)] + _TAIL,
    "lsr_rl_ysep_fused_stats_f32": _RL_HEAD + [("x_a", "p", 1), ("x_b", "p", 2), ("x_out", "p", 10)] + _VOL + [
        ("taps", "p", 3)] + _TAPS + [("norm_table", "p", 9), ("norm_full", "f", 1.0), ("iters", "i", 2),
                                     ("eps", "f", 1e-6)] + _TAIL,
    "lsr_rl_dense_stats_f32": [("y", "p", 0), ("x", "p", 1), ("ratio", "p", 2)] + _VOL + [
        ("psf", "p", 3), ("psf_flipped", "p", 4)] + _TAPS + [("norm_table", "p", 9), ("iters", "i", 2),
                                                            ("eps", "f", 1e-6)] + _TAIL,
    "lsr_correlate_dense_padded_stats_f32": _STRIDED + [("taps", "p", 3)] + _TAPS + [
        ("epilogue", "i", 2), ("eps", "f", 1e-6), ("norm_table", "p", 9), ("norm_full", "f", 1.0)] + _TAIL,
    "lsr_correlate_zxy_padded_stats_f32": _STRIDED + [("taps_zx", "p", 3), ("ky", "p", 4)] + _TAPS + [
        ("epilogue", "i", 2), ("eps", "f", 1e-6), ("norm_table", "p", 9), ("norm_full", "f", 1.0)] + _TAIL,
    "lsr_rl_dense_padded_stats_f32": _RL_HEAD + [("x_pad", "p", 1), ("ratio_pad", "p", 2), ("x_out", "p", 10)] + _VOL + [
        ("taps", "p", 3), ("taps_flipped", "p", 4)] + _TAPS + [("norm_table", "p", 9), ("norm_full", "f", 1.0),
                                                              ("iters", "i", 2), ("eps", "f", 1e-6)] + _TAIL,
    # ---- pure host functions: (value, sha256 of the output array) recorded as well
    "lsr_sep_padded_shape": [("Y", "l", Y), ("X", "l", X)] + _TAPS + [("shape", "p", 11)],
    "lsr_rl_sep_fused_supported": list(_TAPS),
    "lsr_rl_ysep_fused_supported": list(_TAPS),
    "lsr_rl_sep_fused_taps_count": [],
    "lsr_rl_ysep_fused_taps_count": [],
    "lsr_rl_sep_fused_prepare_taps": [("kz_host", "p", 3), ("pz", "i", 3), ("ky_host", "p", 4), ("py", "i", 3),
                                      ("kx_host", "p", 5), ("px", "i", 3), ("taps_host", "p", 11)],
    "lsr_rl_ysep_fused_prepare_taps": [("ky_host", "p", 4), ("py", "i", 3), ("kzx_host", "p", 3), ("pz", "i", 3),
                                       ("px", "i", 3), ("taps_host", "p", 11)],
    "lsr_dense_taps_count": list(_TAPS),
    "lsr_dense_prepare_taps": [("psf_host", "p", 3)] + _TAPS + [("flip", "i", 1), ("taps_host", "p", 11)],
}
OUTPUT = {"lsr_sep_padded_shape": 4 * 8, "lsr_rl_sep_fused_prepare_taps": 96 * 4, "lsr_rl_ysep_fused_prepare_taps": 320 * 4,
          "lsr_dense_prepare_taps": 2 * 11 * 9 * 9 * 4}     # bytes of the output slot that are hashed
HOST_ONLY = set(OUTPUT) | {n for n in ENTRIES if n.endswith("_supported") or n.endswith("_count")}

# ---- one row per requirement: the baseline with exactly that condition broken -> the code it must give ---------------
_SHAPE = [({"Z": 0}, E_SHAPE), ({"Y": -1}, E_SHAPE), ({"X": 1 << 30}, E_UNSUPPORTED), ({"Z": 1 << 20, "Y": 1 << 20, "X": 1 << 20}, E_UNSUPPORTED)]
_BAD_TAPS = [({"pz": 4}, E_UNSUPPORTED), ({"py": 0}, E_UNSUPPORTED), ({"px": 17}, E_UNSUPPORTED)]
_EPI = [({"epilogue": 3}, E_ARG), ({"epilogue": -1}, E_ARG), ({"aux": None}, E_NULL), ({"aux": None, "epilogue": 0}, "ok")]
_SEP_NORMS = [({"nz": None}, E_NULL), ({"ny": None}, E_NULL), ({"nx": None}, E_NULL), ({"nx": None, "epilogue": 1}, "ok")]
_PADDED_IN = [({"in_pitch": -4}, E_UNSUPPORTED), ({"in_plane": 1 << 32}, E_UNSUPPORTED), ({"in_pitch": PITCH - 32}, E_SHAPE),
              ({"in_plane": PLANE - 4}, E_SHAPE), ({"in_pitch": PITCH + 2, "in_plane": ROWS * (PITCH + 2)}, E_ARG),
              ({"in_plane": PLANE + 2}, E_ARG), ({"in_plane": 1 << 30}, E_UNSUPPORTED), ({"aux_plane": 1 << 30}, E_UNSUPPORTED),
              ({"out_plane": 1 << 30}, E_UNSUPPORTED), ({"out_pitch": X - 1}, E_SHAPE), ({"aux_pitch": X - 1}, E_SHAPE),
              ({"aux_pitch": X - 1, "epilogue": 0}, "ok")]
_PADDED_Y = [({"y_pitch": -4}, E_UNSUPPORTED), ({"y_plane": 1 << 32}, E_UNSUPPORTED), ({"y_pitch": PITCH - 32}, E_SHAPE),
             ({"y_plane": PLANE - 4}, E_SHAPE), ({"y_pitch": PITCH + 2, "y_plane": ROWS * (PITCH + 2)}, E_ARG),
             ({"y_plane": PLANE + 2}, E_ARG), ({"y_plane": 1 << 29}, E_UNSUPPORTED)]
_TWO_LAUNCH = [({"y": None}, E_NULL), ({"x_pad": None}, E_NULL), ({"ratio_pad": None}, E_NULL), ({"iters": 0}, E_ARG),
               ({"ratio_pad": 1}, E_ARG), ({"x_out": None}, "ok"), ({"init_from_y": 0}, "ok"), ({"Y": 0}, E_SHAPE),
               ({"y_pitch": PITCH - 32}, E_SHAPE), ({"y_plane": PLANE + 2}, E_ARG)] + _BAD_TAPS
_FUSED = [({"y": None}, E_NULL), ({"x_a": None}, E_NULL), ({"x_b": None}, E_NULL), ({"taps": None}, E_NULL),
          ({"iters": 0}, E_ARG), ({"x_b": 1}, E_ARG), ({"x_out": None}, "ok"), ({"init_from_y": 0}, "ok")] + _SHAPE + _BAD_TAPS + _PADDED_Y
BREAKS = {
    "lsr_correlate_sep_stats_f32": [({"in": None}, E_NULL), ({"out": None}, E_NULL), ({"out": 0}, E_ARG), ({"wz": None}, E_NULL),
                                    ({"wy": None}, E_NULL), ({"wx": None}, E_NULL)] + _SHAPE + _BAD_TAPS + _EPI + _SEP_NORMS,
    "lsr_correlate_dense_stats_f32": [({"in": None}, E_NULL), ({"out": None}, E_NULL), ({"out": 0}, E_ARG), ({"w": None}, E_NULL),
                                      ({"norm_table": None}, E_NULL), ({"norm_table": None, "epilogue": 1}, "ok")]
                                     + _SHAPE + _BAD_TAPS + _EPI,
    "lsr_correlate_sep_strided_stats_f32": [({"in": None}, E_NULL), ({"out": None}, E_NULL), ({"out": 0}, E_ARG),
                                            ({"wz": None}, E_NULL), ({"wy": None}, E_NULL), ({"wx": None}, E_NULL)]
                                           + _SHAPE + _BAD_TAPS + _EPI + _SEP_NORMS + _PADDED_IN,
    "lsr_rl_sep_stats_f32": _TWO_LAUNCH + [({"kz_flipped": None}, E_NULL), ({"ky_flipped": None}, E_NULL), ({"kx_flipped": None}, E_NULL)],
    "lsr_rl_sep_fused_stats_f32": _FUSED + [({"nz": None}, E_NULL), ({"ny": None}, E_NULL), ({"nx": None}, E_NULL),
                                            ({"pz": 15, "py": 11, "px": 11}, E_UNSUPPORTED)],
    "lsr_rl_ysep_fused_stats_f32": _FUSED + [({"norm_table": None}, E_NULL), ({"pz": 13}, E_UNSUPPORTED), ({"px": 11}, E_UNSUPPORTED)],
    "lsr_rl_dense_stats_f32": [({"y": None}, E_NULL), ({"x": None}, E_NULL), ({"ratio": None}, E_NULL), ({"iters": -1}, E_ARG),
                               ({"iters": 0}, "ok"), ({"ratio": 1}, E_ARG), ({"ratio": 0}, E_ARG), ({"x": 0}, E_ARG),
                               ({"psf_flipped": None}, E_NULL)] + _SHAPE + _BAD_TAPS,
    "lsr_correlate_dense_padded_stats_f32": [({"in": None}, E_NULL), ({"out": None}, E_NULL), ({"out": 0}, E_ARG),
                                             ({"taps": None}, E_NULL), ({"pz": 13}, E_UNSUPPORTED), ({"py": 11}, E_UNSUPPORTED),
                                             ({"epilogue": 4}, E_ARG), ({"epilogue": -1}, E_ARG), ({"aux": None}, E_NULL),
                                             ({"aux": None, "epilogue": 3}, "ok"), ({"norm_table": None}, E_NULL),
                                             ({"norm_table": None, "epilogue": 3}, E_NULL), ({"norm_table": None, "epilogue": 1}, "ok")]
                                            + _SHAPE + _BAD_TAPS + _PADDED_IN,
    "lsr_correlate_zxy_padded_stats_f32": [({"in": None}, E_NULL), ({"out": None}, E_NULL), ({"out": 0}, E_ARG),
                                           ({"taps_zx": None}, E_NULL), ({"ky": None}, E_NULL), ({"epilogue": 0}, E_ARG),
                                           ({"epilogue": 3}, E_ARG), ({"epilogue": 4}, E_ARG), ({"pz": 13}, E_UNSUPPORTED),
                                           ({"aux": None}, E_NULL), ({"norm_table": None}, E_NULL)] + _SHAPE + _BAD_TAPS + _PADDED_IN[:-1],
    "lsr_rl_dense_padded_stats_f32": _TWO_LAUNCH + [({"taps_flipped": None}, E_NULL), ({"pz": 13}, E_UNSUPPORTED)],
    "lsr_sep_padded_shape": [({"shape": None}, E_NULL), ({"Y": 0}, E_SHAPE), ({"X": -3}, E_SHAPE), ({"X": 1 << 30}, E_UNSUPPORTED),
                             ({"Y": 1 << 29, "X": 1 << 29}, E_UNSUPPORTED), ({"pz": 15, "py": 7, "px": 13}, 0),
                             ({"Y": 24, "X": 128, "py": 9}, 0), ({"Y": 1, "X": 1, "pz": 1, "py": 1, "px": 1}, 0)] + _BAD_TAPS,
    "lsr_rl_sep_fused_supported": [({"pz": 15, "py": 11}, 0), ({"pz": 15, "py": 9, "px": 9}, 1), ({"pz": 2}, 0), ({"px": 17}, 0),
                                   ({"py": 0}, 0), ({"pz": 1, "py": 1, "px": 1}, 1), ({"pz": 13, "py": 15, "px": 15}, 1)],
    "lsr_rl_ysep_fused_supported": [({"pz": 11, "py": 9, "px": 9}, 1), ({"pz": 13}, 0), ({"px": 11}, 0), ({"py": 4}, 0),
                                    ({"pz": -1}, 0), ({"pz": 1, "py": 1, "px": 1}, 1)],
    "lsr_rl_sep_fused_taps_count": [],
    "lsr_rl_ysep_fused_taps_count": [],
    "lsr_rl_sep_fused_prepare_taps": [({"kz_host": None}, E_NULL), ({"ky_host": None}, E_NULL), ({"kx_host": None}, E_NULL),
                                      ({"taps_host": None}, E_NULL), ({"pz": 15, "py": 11}, E_UNSUPPORTED),
                                      ({"pz": 5, "py": 1, "px": 13}, 0), ({"pz": 15, "py": 9, "px": 7}, 0)] + _BAD_TAPS,
    "lsr_rl_ysep_fused_prepare_taps": [({"ky_host": None}, E_NULL), ({"kzx_host": None}, E_NULL), ({"taps_host": None}, E_NULL),
                                       ({"pz": 13}, E_UNSUPPORTED), ({"px": 11}, E_UNSUPPORTED), ({"pz": 11, "py": 9, "px": 5}, 0),
                                       ({"pz": 1, "py": 7, "px": 1}, 0)] + _BAD_TAPS,
    "lsr_dense_taps_count": [({"pz": 13}, E_UNSUPPORTED), ({"px": 11}, E_UNSUPPORTED), ({"pz": 11, "py": 9, "px": 9}, 2 * 11 * 81),
                             ({"pz": 1, "py": 1, "px": 1}, 54)] + _BAD_TAPS,
    "lsr_dense_prepare_taps": [({"psf_host": None}, E_NULL), ({"taps_host": None}, E_NULL), ({"pz": 13}, E_UNSUPPORTED),
                               ({"flip": 0}, 0), ({"pz": 11, "py": 9, "px": 9}, 0), ({"pz": 5, "py": 1, "px": 7, "flip": 0}, 0)]
                              + _BAD_TAPS,
}
# every negative code the source of an entry can return (asserted covered when recording)
CODES = {n: ({E_NULL, E_SHAPE, E_UNSUPPORTED, E_ARG} if n.endswith("_stats_f32") else set()) for n in ENTRIES}
CODES["lsr_sep_padded_shape"] = {E_NULL, E_SHAPE, E_UNSUPPORTED}
for _n in ("lsr_rl_sep_fused_prepare_taps", "lsr_rl_ysep_fused_prepare_taps", "lsr_dense_prepare_taps"):
    CODES[_n] = {E_NULL, E_UNSUPPORTED}
CODES["lsr_dense_taps_count"] = {E_UNSUPPORTED}


class Tables:
    """One family of entries: what the caller and the row machinery below read.  ``output``: bytes of the output slot
    that are hashed, per entry that fills one; ``output_args``: the names an output array goes by; ``baseline``: what
    the baseline of a pure host function answers where that is not 0."""

    def __init__(self, fixture, entries, breaks, output, host_only, codes, output_args=("shape", "taps_host"), baseline=None):
        self.fixture, self.entries, self.breaks, self.output, self.host_only, self.codes = (
            fixture, entries, breaks, output, host_only, codes)
        self.output_args, self.baseline = output_args, baseline or {}

    def output_at(self, name):
        """Index of the argument that is the entry's output array."""
        return next(i for i, (a, _, _) in enumerate(self.entries[name]) if a in self.output_args)


STENCIL = Tables(FIXTURE, ENTRIES, BREAKS, OUTPUT, HOST_ONLY, CODES)


class Caller:
    """Calls entries of the loaded library with rows of plain values; pointer slot k -> buffer + k * SLOT."""

    def __init__(self):
        import torch

        if torch.cuda.is_available():
            raise RuntimeError("a device is visible: a row that passes validation would launch on host pointers")
        from shrimpy_amd import _lib

        self.lib, self.sigs = _lib.load(), _lib.SIGNATURES
        self.buf = np.ascontiguousarray(np.random.default_rng(SEED).random(16 * SLOT // 8))   # finite values everywhere
        need = (ctypes.c_int64 * 4)()
        assert self.lib.lsr_sep_padded_shape(Y, X, 3, 3, 3, need) == 0 and (need[0], need[1]) == (ROWS, PITCH), list(need)

    def pointer(self, slot):
        return None if slot is None else self.buf.ctypes.data + slot * SLOT

    def call(self, name, kinds, values, t=STENCIL):
        sig, args = self.sigs[name], []
        assert len(sig) == len(kinds), name
        for ctype, kind, v in zip(sig, kinds, values):
            if kind in "pn":
                p = self.pointer(v)
                args.append(p if ctype is ctypes.c_void_p or p is None else ctypes.cast(p, ctype))
            elif kind == "f":
                args.append(ctypes.c_float(v))
            else:
                args.append(int(v))
        if name in t.output:
            ctypes.memset(self.pointer(11), 0xA5, t.output[name])
        rc = int(getattr(self.lib, name)(*args))
        if name not in t.host_only:
            return rc if rc < 0 else "ok"
        if name in t.output and values[t.output_at(name)] is not None:
            return [rc, hashlib.sha256(ctypes.string_at(self.pointer(11), t.output[name])).hexdigest()[:16]]
        return rc


def rows_of(name, t=STENCIL):
    """The baseline, then its broken copies: (values, expected status or None)."""
    spec = t.entries[name]
    names = [a for a, _, _ in spec]
    base = [v for _, _, v in spec]
    # (None: a value, recorded as it is)
    out = [(base, "ok" if name not in t.host_only else t.baseline.get(name, 0) if name in t.output else None)]
    for change, want in t.breaks[name]:
        row = list(base)
        for k, v in change.items():
            row[names.index(k)] = v
        out.append((row, want))
    return out


def draws_of(name, index, t=STENCIL):
    """DRAWS argument lists from the fuzzer's pools (pointers: 5 % NULL, else a slot; the stream always NULL).  Kind
    "s": an extent of a volume that the entry really reads or writes -- 1 to 6, or (10 %) one that validation refuses."""
    rng = np.random.default_rng([SEED, index])
    for _ in range(DRAWS):
        row = []
        for _, kind, _ in t.entries[name]:
            if kind == "s":
                row.append(int(rng.choice(BAD_EXTENTS)) if rng.random() < 0.1 else int(rng.integers(1, 7)))
            elif kind == "l":
                row.append(int(rng.choice(INTS)) if rng.random() < 0.6 else int(rng.integers(1, 70)))
            elif kind == "i":
                row.append(int(rng.choice(SMALL)) if rng.random() < 0.6 else int(rng.integers(0, 12)))
            elif kind == "f":
                row.append(float(rng.choice(FLOATS)))
            elif kind == "p":
                row.append(None if rng.random() < 0.05 else int(rng.integers(0, 11)))
            else:
                row.append(None)
        if name in t.output and row[t.output_at(name)] is not None:
            row[t.output_at(name)] = 11    # an output array goes to the output slot
        yield row


def measure(caller, t=STENCIL):
    """{entry: {"rows": [status per row of rows_of], "draws": [status per draw]}}"""
    result = {}
    for index, name in enumerate(t.entries):
        kinds = ["l" if k == "s" else k for _, k, _ in t.entries[name]]
        result[name] = {"rows": [caller.call(name, kinds, row, t) for row, _ in rows_of(name, t)],
                        "draws": [caller.call(name, kinds, row, t) for row in draws_of(name, index, t)] if kinds else []}
    return result


def main(t=STENCIL, caller=None):
    got = measure(caller or Caller(), t)
    for name, rec in got.items():
        expect = [want for _, want in rows_of(name, t)]
        status = [r[0] if isinstance(r, list) else r for r in rec["rows"]]
        assert all(s == e for s, e in zip(status, expect) if e is not None), \
            (name, [(i, s, e) for i, (s, e) in enumerate(zip(status, expect)) if s != e])
        every = status + [r[0] if isinstance(r, list) else r for r in rec["draws"]]
        assert any(s == "ok" or (isinstance(s, int) and s >= 0) for s in every), name
        assert t.codes[name] <= {s for s in every if isinstance(s, int) and s < 0}, (name, t.codes[name])
        if name not in t.host_only or name in t.output:
            first_null = sum(1 for row in list(r for r, _ in rows_of(name, t)) + list(draws_of(name, list(t.entries).index(name), t))
                             if row[0] is None)
            assert 2 * first_null <= len(every), (name, first_null)
    t.fixture.write_text(json.dumps({"seed": SEED, "draws": DRAWS, "entries": got}, separators=(",", ":")) + "\n")
    print(f"{t.fixture}: {sum(len(r['rows']) + len(r['draws']) for r in got.values())} calls, {t.fixture.stat().st_size} bytes")


if __name__ == "__main__":
    main()
