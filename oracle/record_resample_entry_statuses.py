"""What the affine resampler's entry points (csrc/affine.hip, the twin in csrc/host_twins.hip) answer on a machine
WITHOUT a GPU, recorded as oracle/record_stencil_entry_statuses.py records the stencil entries -- its caller, rows and
draws are used as they are; this file holds the tables only.

    python -m oracle.record_resample_entry_statuses      # rewrites tests/golden/resample_entry_statuses.json

The device entries (lsr_affine_f32, lsr_affine_pitched_f32): the negative code, or "ok".  The pure host functions: the
value (lsr_affine_path, lsr_affine_path_pitched, lsr_affine_kernel_choice), the value and the six ints
(lsr_affine_box_shape), the status and the sixteen numbers (lsr_affine_plan), the status and the output bytes (lsr_affine_f32_cpu, which really resamples: its extents are
of kind "s", a volume of at most 6 x 10 x 12 in the rows and 6 x 6 x 6 in the draws).  NEVER run this where a device is
visible.
"""

from __future__ import annotations

import numpy as np

from oracle import record_stencil_entry_statuses as base
from oracle.record_stencil_entry_statuses import E_ARG, E_NULL, E_SHAPE, E_UNSUPPORTED

FIXTURE = base.FIXTURE.with_name("resample_entry_statuses.json")

# pointer slots: 0 the moving volume (float32), 2 the device entries' output, 11 the host functions' output, and
# the matrices (12 doubles at the start of a slot)
PLANAR, TILTED, STEEP, NAN, INF, SHRINK = 3, 4, 5, 6, 7, 8
_c, _s = np.cos(np.deg2rad(2.0)), np.sin(np.deg2rad(2.0))
MATRICES = {
    PLANAR: [1, 0, 0, 3.5, 0, 0.98 * _c, -1.02 * _s, -12.25, 0, 0.98 * _s, 1.02 * _c, 20.75],   # rotation in the plane
    TILTED: [0.999, 0.01, -0.05, 1.5, -0.01, 0.98, -0.03, -4.25, 0.05, 0.03, 1.02, 6.75],       # couples z with the plane
    STEEP: [0.1, 9.0, 40.0, 0, 30.0, 0.2, 50.0, 0, 70.0, 20.0, 0.3, 0],                         # no source box fits LDS
    NAN: [1, 0, 0, 0, 0, 1, 0, float("nan"), 0, 0, 1, 0],
    INF: [1, 0, 0, 0, 0, 1, float("inf"), 0, 0, 0, 1, 0],
    SHRINK: [0.8, 0.02, -0.03, 0.4, 0.05, 0.9, 0.1, -0.5, -0.04, 0.08, 0.85, 0.7],              # the twin's baseline map
}

Z, Y, X = 24, 96, 132
PITCH, OPITCH = 136, 140
_IN = [("in", "p", 0), ("Zi", "l", Z), ("Yi", "l", Y), ("Xi", "l", X)]
_OUT = [("out", "p", 2), ("Zo", "l", Z), ("Yo", "l", Y), ("Xo", "l", X)]
_CALL = [("M", "p", PLANAR), ("cval", "f", -3.0), ("mode", "i", 0), ("stream", "n", None)]
ENTRIES = {
    "lsr_affine_f32": _IN + _OUT + _CALL,
    "lsr_affine_pitched_f32": _IN + [("in_pitch", "l", PITCH), ("in_plane", "l", Y * PITCH)] + _OUT + [
        ("out_pitch", "l", OPITCH), ("out_plane", "l", Y * OPITCH)] + _CALL,
    "lsr_affine_f32_cpu": [("in", "p", 0), ("Zi", "s", 5), ("Yi", "s", 9), ("Xi", "s", 11), ("out", "p", 11), ("Zo", "s", 6),
                           ("Yo", "s", 10), ("Xo", "s", 12), ("M", "p", SHRINK), ("cval", "f", -3.0), ("mode", "i", 0),
                           ("stream", "n", None)],
    "lsr_affine_path": [("Zi", "l", Z), ("Yi", "l", Y), ("Xi", "l", X), ("M", "p", PLANAR), ("mode", "i", 0)],
    "lsr_affine_path_pitched": [("Zi", "l", Z), ("Yi", "l", Y), ("Xi", "l", X), ("in_pitch", "l", PITCH),
                                ("in_plane", "l", Y * PITCH), ("M", "p", PLANAR), ("mode", "i", 0)],
    "lsr_affine_kernel_choice": [("Yi", "l", Y), ("Xi", "l", X), ("M", "p", PLANAR), ("mode", "i", 0)],
    "lsr_affine_box_shape": [("Zi", "l", Z), ("Yi", "l", Y), ("Xi", "l", X), ("M", "p", TILTED), ("out6", "p", 11)],
    "lsr_affine_plan": [("Zi", "l", Z), ("Yi", "l", Y), ("Xi", "l", X), ("in_pitch", "l", PITCH), ("in_plane", "l", Y * PITCH),
                        ("Zo", "l", Z), ("Yo", "l", Y), ("Xo", "l", X), ("out_pitch", "l", OPITCH), ("M", "p", PLANAR),
                        ("mode", "i", 0), ("out16", "p", 11)],
}
OUTPUT = {"lsr_affine_f32_cpu": 6 * 10 * 12 * 4, "lsr_affine_box_shape": 6 * 4, "lsr_affine_plan": 16 * 8}
HOST_ONLY = set(ENTRIES) - {"lsr_affine_f32", "lsr_affine_pitched_f32"}

# ---- one row per check group: the baseline with exactly that condition broken ---------------------------------------
_MODES = [({"mode": 1}, "ok"), ({"mode": 256}, "ok"), ({"mode": 257}, "ok"), ({"mode": 2}, E_ARG), ({"mode": 258}, E_ARG),
          ({"mode": -1}, E_ARG)]
_MATRIX = [({"M": None}, E_NULL), ({"M": NAN}, E_ARG), ({"M": INF}, E_ARG), ({"M": TILTED}, "ok"), ({"M": STEEP}, "ok")]
_POINTERS = [({"in": None}, E_NULL), ({"out": None}, E_NULL), ({"out": 0}, "ok")]
_HUGE = [({"Xi": 1 << 30}, E_UNSUPPORTED), ({"Zo": 1 << 20, "Yo": 1 << 20, "Xo": 1 << 20}, E_UNSUPPORTED)]
_QUERY_MODES = [({"mode": 1}, None), ({"mode": 256}, None), ({"mode": 2}, 0), ({"mode": 258}, 0), ({"mode": -1}, 0)]
_QUERY_MAPS = [({"M": None}, 0), ({"M": TILTED}, None), ({"M": STEEP}, None), ({"M": NAN}, None)]
BREAKS = {
    # (a dense call states its shape checks first: a bad extent and a NULL pointer together give the shape's code)
    "lsr_affine_f32": _POINTERS + [({"Zi": 0}, E_SHAPE), ({"Yo": -1}, E_SHAPE), ({"Zi": 0, "in": None}, E_SHAPE)] + _HUGE
                      + _MODES + _MATRIX,
    # (a padded call has no "positive" check of its own: an extent <= 0 is outside the supported range)
    "lsr_affine_pitched_f32": _POINTERS + [({"Zi": 0}, E_UNSUPPORTED), ({"Yo": -1}, E_UNSUPPORTED)] + _HUGE + [
        ({"in_pitch": -4}, E_UNSUPPORTED), ({"in_plane": 1 << 32}, E_UNSUPPORTED), ({"out_pitch": 1 << 31}, E_UNSUPPORTED),
        ({"out_plane": -1}, E_UNSUPPORTED), ({"in_pitch": X - 1}, E_SHAPE), ({"in_plane": Y * PITCH - 1}, E_SHAPE),
        ({"out_pitch": X - 1}, E_SHAPE), ({"out_plane": Y * OPITCH - 1}, E_SHAPE),
        ({"in_pitch": 1 << 30, "in_plane": (1 << 32) - 1, "Yi": 3}, E_UNSUPPORTED), ({"in_pitch": X, "in_plane": Y * X}, "ok"),
        ({"in_plane": Y * PITCH + 2}, "ok"), ({"in_pitch": X - 1, "in": None}, E_SHAPE),
        # (the order of the later groups: pointers, the 2^30 row limit, the border mode, the matrix)
        ({"in_pitch": 1 << 30, "in_plane": (1 << 32) - 1, "Yi": 3, "in": None}, E_NULL),
        ({"in_pitch": 1 << 30, "in_plane": (1 << 32) - 1, "Yi": 3, "mode": 2}, E_UNSUPPORTED), ({"mode": 2, "M": None}, E_NULL),
        ({"mode": 2, "M": NAN}, E_ARG)] + _MODES + _MATRIX,
    # (the twin: pointers and the matrix first; no f32 interpolation on the host)
    "lsr_affine_f32_cpu": [({"in": None}, E_NULL), ({"out": None}, E_NULL), ({"M": None}, E_NULL), ({"M": NAN}, E_ARG),
                           ({"M": INF}, E_ARG), ({"M": NAN, "Zi": 0}, E_ARG), ({"Zi": 0}, E_SHAPE), ({"Yo": -1}, E_SHAPE),
                           ({"Xi": 1 << 30}, E_UNSUPPORTED), ({"Zo": 1 << 20, "Yo": 1 << 20, "Xo": 1 << 20}, E_UNSUPPORTED),
                           ({"mode": 1}, 0), ({"mode": 2}, E_ARG), ({"mode": 256}, E_ARG), ({"mode": 257}, E_ARG),
                           ({"mode": -1}, E_ARG), ({"M": PLANAR}, 0), ({"M": TILTED, "mode": 1}, 0),
                           ({"Zi": 1, "Yi": 1, "Xi": 1, "M": TILTED, "mode": 1}, 0), ({"Zo": 1, "Yo": 1, "Xo": 1}, 0),
                           ({"cval": 0.0, "mode": 1}, 0)],
    "lsr_affine_path": _QUERY_MODES + _QUERY_MAPS + [({"Zi": 0}, 0), ({"Xi": 1 << 30}, 0), ({"Zi": 1, "M": TILTED}, None),
                                                     ({"Xi": 7}, None), ({"Yi": 1}, None)],
    "lsr_affine_path_pitched": _QUERY_MODES + _QUERY_MAPS + [
        ({"Zi": 0}, 0), ({"Xi": 1 << 30}, 0), ({"in_pitch": -4}, 0), ({"in_plane": 1 << 32}, 0), ({"in_pitch": X + 1}, None),
        ({"in_plane": Y * PITCH + 2}, None), ({"in_plane": Y * PITCH + 2, "M": TILTED}, None), ({"in_pitch": X - 1}, None),
        ({"in_pitch": X, "in_plane": Y * X}, None)],
    "lsr_affine_kernel_choice": _QUERY_MODES + _QUERY_MAPS + [({"Yi": 0}, None), ({"Xi": 7}, None), ({"Yi": 1}, None),
                                                              ({"Xi": 1 << 30}, None)],
    "lsr_affine_box_shape": [({"M": None}, 0), ({"out6": None}, 0), ({"Zi": 0}, 0), ({"Xi": 1 << 30}, 0), ({"M": STEEP}, 0),
                             ({"M": PLANAR}, 1), ({"Zi": 1}, 0), ({"Xi": 7}, 0), ({"M": NAN}, None)],
    # (the pitched entry's statuses in its order, the buffers apart; the 16 numbers where the call passes)
    "lsr_affine_plan": [({"out16": None}, E_NULL), ({"M": None}, E_NULL), ({"Zi": 0}, E_UNSUPPORTED), ({"Yo": -1}, E_UNSUPPORTED),
                        ({"Xi": 1 << 30}, E_UNSUPPORTED), ({"in_pitch": -4}, E_UNSUPPORTED), ({"in_plane": 1 << 32}, E_UNSUPPORTED),
                        ({"out_pitch": 1 << 31}, E_UNSUPPORTED), ({"in_pitch": X - 1}, E_SHAPE), ({"in_plane": Y * PITCH - 1}, E_SHAPE),
                        ({"out_pitch": X - 1}, E_SHAPE), ({"in_pitch": X - 1, "M": None}, E_SHAPE), ({"mode": 2, "M": None}, E_NULL),
                        ({"mode": 2}, E_ARG), ({"mode": 2, "M": NAN}, E_ARG), ({"M": NAN}, E_ARG), ({"M": INF}, E_ARG),
                        ({"mode": 1}, 0), ({"mode": 256}, 0), ({"mode": 257}, 0), ({"M": TILTED}, 0), ({"M": STEEP}, 0),
                        ({"in_pitch": X + 1, "in_plane": Y * (X + 1)}, 0), ({"in_plane": Y * PITCH + 2}, 0),
                        ({"in_pitch": X, "in_plane": Y * X, "out_pitch": X}, 0), ({"Zi": 1, "M": TILTED}, 0)],
}
CODES = {n: set() for n in ENTRIES}
CODES["lsr_affine_f32"] = CODES["lsr_affine_pitched_f32"] = CODES["lsr_affine_f32_cpu"] = {E_NULL, E_SHAPE, E_UNSUPPORTED, E_ARG}
CODES["lsr_affine_plan"] = {E_NULL, E_SHAPE, E_UNSUPPORTED, E_ARG}

TABLES = base.Tables(FIXTURE, ENTRIES, BREAKS, OUTPUT, HOST_ONLY, CODES, output_args=("out", "out6", "out16"),
                     baseline={"lsr_affine_box_shape": 1})


class Caller(base.Caller):
    """The stencil caller with the moving volume and the matrices written into their slots."""

    def __init__(self):
        super().__init__()
        rng = np.random.default_rng([base.SEED, 1])
        floats = self.buf.view(np.float32)
        floats[: base.SLOT // 4] = (rng.random(base.SLOT // 4) * 1000 - 100).astype(np.float32)
        for slot, m in MATRICES.items():
            self.buf[slot * base.SLOT // 8: slot * base.SLOT // 8 + 12] = m


def measure(caller):
    return base.measure(caller, TABLES)


if __name__ == "__main__":
    base.main(TABLES, Caller())
