"""The cases of the affine tests (``tests/test_affine_host.py``, ``tests/test_affine_edges_gpu.py``): a designed list, sized from the
exported launch plan (``lsr_affine_plan``) -- no threshold is written down here, each is bisected over the doubles against the plan.

* ``planar_tile``: each of the four tiles of ``csrc/affine_planar.hip`` under 8 and under 4 waves, at the last double the plan
  still gives it, at the next double (the next smaller tile, or another kernel) and well inside; both signs of ``b, c, d, e``;
  output extents ``1, t - 1, t, t + 1, 2 t + 1``; the staging limit at equality; the ring of 4 at its own budget; in-plane extents
  one double below an integer, on it and above it, and at the doubles where ``box_y`` / ``box_x`` step;
* ``planar_z``: the z march -- ``a`` at the ring thresholds, 0, small, negative, fractional ``tz``, chunks entered and left inside
  the volume, every plane outside, ``Zo`` around the chunk edges, ``Zi`` of 1 and 2, full and ragged tiles in one launch;
* ``planar_map``: more than one patch along y and along x under the default patch and ``LSR_PLANAR_PATCH=1,64`` / ``64,1``;
* ``box_shape``: the block shapes and walks of ``csrc/affine_box.hip`` found by a search over tilts and scalings, the doubles at
  which a box extent steps on each axis, the last map the box kernel takes and the first it does not, more than four blocks per
  axis under ``LSR_BOX_LINEAR=0`` and ``1``;
* ``box_kind``: interior, border and blind blocks in one launch, a block's corner coordinate exactly on each value its kind is
  decided against and one double either side;
* ``grid_points``: whole-number maps whose coordinates land on ``-1, 0, n - 1, n``, and ``+-2^-30``, ``+-2^-52`` about them;
* ``strides``: padded rows and planes on both sides, the padding first zeros, then a large finite value;
* ``content``: negatives, ``+-3e38``, denormals, ``+-0.0``, a constant, and volumes with a NaN, ``+inf`` and ``-inf``.

Every case runs under both borders; ``cval`` cycles over ``CVALS``.  Every array is read-only and computed once.
"""

import contextlib
import ctypes
import dataclasses
import functools
import math
import os
import zlib

import numpy as np

from shrimpy_amd import _lib
from tests import affine_ref as R

PAYLOAD = 0x7FC5A5A5                       # the NaN the output buffers are filled with before a call
CVALS = (0.0, -3.0, 7.25, float(np.float32(132.8)))
MODE_CODE = {"constant": _lib.MODE_CONSTANT, "grid-constant": _lib.MODE_GRID_CONSTANT}
SWITCHES = ("LSR_PLANAR_WAVES", "LSR_PLANAR_PATCH", "LSR_BOX_LINEAR")
GROUPS = ["planar_tile", "planar_z", "planar_map", "box_shape", "box_kind", "grid_points", "strides", "content"]
PLANAR_TILES = ((4, 2), (4, 1), (2, 2), (2, 1))          # rows per wave, 64-column groups: 32x128, 32x64, 16x128, 16x64 at 8 waves
BOX_BLOCKS = ((8, 8, 64), (16, 8, 32), (8, 16, 32), (16, 4, 64), (8, 4, 128), (16, 2, 128))
MAX_VOXELS = 2_000_000


def next_up(v):
    return float(np.nextafter(np.float64(v), np.float64(np.inf)))


def next_down(v):
    return float(np.nextafter(np.float64(v), np.float64(-np.inf)))


def round_up4(n):
    return (int(n) + 3) & ~3


@contextlib.contextmanager
def switched(env):
    """The measurement switches of ``env`` (pairs) set, every other one unset, for the duration."""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in env:
            os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def raw_plan(shape, pitch, plane, out_shape, out_pitch, m, mode_code):
    """``lsr_affine_plan`` under the environment as it stands: the 16 numbers of include/lsrecon.h."""
    out = (ctypes.c_int64 * 16)()
    _lib.call("lsr_affine_plan", *(int(v) for v in shape), int(pitch), int(plane), *(int(v) for v in out_shape), int(out_pitch),
              _lib.matrix12(m), int(mode_code), out)
    return tuple(int(v) for v in out)


PROBE = (40, 64, 64)


def probe(m, env=(), f32=False):
    """The plan of a matrix on a small dense volume (no decision about the kernel or its tile depends on the extents)."""
    with switched(env):
        return raw_plan(PROBE, PROBE[2], PROBE[1] * PROBE[2], PROBE, PROBE[2], m, _lib.MODE_F32_INTERP if f32 else 0)


def bisect(pred, lo, hi):
    """The last double in ``[lo, hi)`` for which ``pred`` holds (``0 <= lo < hi``, ``pred(lo)``, ``not pred(hi)``, one change)."""
    assert 0.0 <= lo < hi and pred(lo) and not pred(hi), (lo, hi)
    a, b = int(np.float64(lo).view(np.int64)), int(np.float64(hi).view(np.int64))
    while b - a > 1:
        mid = (a + b) // 2
        if pred(float(np.int64(mid).view(np.float64))):
            a = mid
        else:
            b = mid
    return float(np.int64(a).view(np.float64))


def planar_tile_index(plan, waves=None):
    """0 .. 3 as ``PLANAR_TILES``; 4 when the planar kernel does not take the map, or takes it with another wave count than
    ``waves`` (a map none of whose four-wave tiles fits runs under eight waves whatever ``LSR_PLANAR_WAVES`` says)."""
    if plan[0] != 1 or (waves is not None and plan[1] != waves):
        return 4
    return PLANAR_TILES.index((plan[2] // plan[1], plan[3] // 64))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str
    shape: tuple                             # (Zi, Yi, Xi)
    out_shape: tuple
    m: tuple                                 # 12 doubles, row-major 3x4
    path: int                                # the kernel the case aims at: 0 gather, 1 planar, 2 box
    cval: float = 0.0
    content: str = "uniform"
    in_pad: int = 0                          # source pitch = Xi rounded up to 4, plus this
    in_rows: int = 0                         # spare rows behind every source plane
    in_pitch: int = 0                        # an explicit source pitch instead (one the LDS kernels cannot take)
    pad_value: float = 0.0                   # what the source's padding holds
    out_pad: int = 0
    out_rows: int = 0
    env: tuple = ()                          # measurement switches as (name, value) pairs
    f32: bool = True                         # also run under LSR_MODE_F32_INTERP
    aim: tuple = ()                          # what the census reads: free-form (key, value) pairs

    @property
    def pitch(self):
        return self.in_pitch if self.in_pitch else round_up4(self.shape[2]) + self.in_pad

    @property
    def plane(self):
        return (self.shape[1] + self.in_rows) * self.pitch

    @property
    def out_pitch(self):
        return self.out_shape[2] + self.out_pad

    @property
    def out_plane(self):
        return (self.out_shape[1] + self.out_rows) * self.out_pitch

    @property
    def dense(self):
        return (self.pitch == self.shape[2] and self.in_rows == 0 and self.out_pad == 0 and self.out_rows == 0)

    @property
    def gather_pitch(self):
        """A source pitch neither LDS kernel takes: the forced gather run of the same voxels."""
        return self.shape[2] + 1 + (self.shape[2] % 4 == 3)

    def plan(self, mode="constant", f32=False, pitch=None, plane=None):
        """The plan of the case's own call under its switches."""
        pitch = self.pitch if pitch is None else pitch
        plane = (self.shape[1] + self.in_rows) * pitch if plane is None else plane
        with switched(self.env):
            return raw_plan(self.shape, pitch, plane, self.out_shape, self.out_pitch, self.m,
                            MODE_CODE[mode] | (_lib.MODE_F32_INTERP if f32 else 0))

    def aimed(self, key, default=None):
        return dict(self.aim).get(key, default)


_CASES = {}


def _add(group, name, shape, out_shape, m, path, **kw):
    name = f"{group}: {name}"
    assert name not in _CASES, name
    shape, out_shape = tuple(int(v) for v in shape), tuple(int(v) for v in out_shape)
    assert int(np.prod(out_shape)) <= MAX_VOXELS and int(np.prod(shape)) <= MAX_VOXELS, name
    kw.setdefault("cval", CVALS[len(_CASES) % len(CVALS)])
    _CASES[name] = Case(name, group, shape, out_shape, tuple(float(v) for v in np.asarray(m, dtype=np.float64).reshape(12)),
                        int(path), **kw)
    return _CASES[name]


def matrix(rows3x3, shifts=(0.0, 0.0, 0.0)):
    m = np.zeros((3, 4))
    m[:, :3] = np.asarray(rows3x3, dtype=np.float64)
    m[:, 3] = shifts
    return m


def planar(a, b, c, d, e):
    return [[a, 0.0, 0.0], [0.0, b, c], [0.0, d, e]]


def rotation(s, degrees, sy=1.0, sx=1.0, a=1.0):
    """Rotation by ``degrees`` times the scale ``s`` in the plane; ``sy``, ``sx`` = -1 mirror the source rows / columns."""
    co, si = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    return planar(a, sy * s * co, -sy * s * si, sx * s * si, sx * s * co)


def fit(rows3x3, out_shape, keep=0.9, cap=(48, 288, 288), low=(2, 2, 8), frac=0.3125):
    """``(shape, matrix)``: a source volume that holds ``keep`` of the output's footprint per axis (so that the output's rim is
    outside it), capped, the output's centre on the source's centre plus a fraction."""
    rows = np.asarray(rows3x3, dtype=np.float64)
    half = np.array([(n - 1) / 2.0 for n in out_shape])
    span = np.abs(rows) @ np.array([n - 1 for n in out_shape], dtype=np.float64)
    shape = [int(min(max(int(keep * s) + 2, lo), hi)) for s, lo, hi in zip(span, low, cap)]
    shape[2] = round_up4(shape[2])
    shifts = [(n - 1) / 2.0 - float(r @ half) + frac for n, r in zip(shape, rows)]
    return tuple(shape), matrix(rows, shifts)


def extents(t):
    return [1, t - 1, t, t + 1, 2 * t + 1]


# ---- planar_tile ------------------------------------------------------------------------------------------------------------------

SIGNS = ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))


def _tile_family(t):
    """In-plane maps of one parameter ``s`` under which the plan walks down to the tile ``t`` as ``s`` grows."""
    if t == 2:      # 16 x 128 only beats 32 x 64 for maps that decimate along y alone
        return lambda s, k=0: planar(1.0, SIGNS[k % 4][0] * s, 0.05 * (-1) ** k, -0.03 * SIGNS[k % 4][1], SIGNS[k % 4][1] * 1.0)
    return lambda s, k=0: rotation(s, 17.0 * (-1) ** (k // 4), *SIGNS[k % 4])


@functools.lru_cache(maxsize=None)
def tile_threshold(t, waves, a=1.0):
    """``(below, last)``: the last ``s`` of the tile's family the plan gives a larger tile, and the last it gives the tile ``t``
    (``None`` where the family never reaches it)."""
    env = (("LSR_PLANAR_WAVES", str(waves)),)
    fam = _tile_family(t)

    def index(s):
        rows = np.array(fam(s))
        rows[0, 0] = a
        return planar_tile_index(probe(matrix(rows), env), waves)

    lo, hi = 2.0 ** -6, 64.0
    if index(lo) > t or index(hi) <= t:
        return None, None
    last = bisect(lambda s: index(s) <= t, lo, hi)
    below = bisect(lambda s: index(s) <= t - 1, lo, hi) if t > 0 and index(lo) <= t - 1 else lo
    return below, (last if index(last) == t else None)


def _build_planar_tile():
    k = 0
    for waves in (8, 4):
        env = (("LSR_PLANAR_WAVES", str(waves)),)
        for t, (nr, nc) in enumerate(PLANAR_TILES):
            below, last = tile_threshold(t, waves)
            if last is None:
                continue                    # (the census reports the tile as not reached)
            ty, tx = waves * nr, 64 * nc
            for label, s in (("last", last), ("next", next_up(last)), ("inside", 1.0 if t == 0 else 0.5 * (below + last))):
                for full in (True, False):
                    rows = _tile_family(t)(s, k)
                    yo, xo = (2 * ty + 1, 2 * tx + 1) if full else (extents(ty)[k % 5], extents(tx)[(k // 2 + 3) % 5])
                    out_shape = (2, yo, xo)
                    shape, m = fit(rows, out_shape)
                    path = probe(m, env)[0]
                    _add("planar_tile", f"{waves} waves tile {ty}x{tx} {label} {'full' if full else 'small'} k={k}", shape, out_shape, m,
                         path, env=env, aim=(("tile", t), ("waves", waves), ("at", label)))
                    k += 1
    # the ring of 4 at its own budget
    below, last = tile_threshold(0, 8, a=1.25)
    for label, s in (("last", last), ("next", next_up(last))):
        rows = np.array(_tile_family(0)(s, 1))
        rows[0, 0] = 1.25
        shape, m = fit(rows, (3, 65, 257))
        _add("planar_tile", f"ring of 4, tile 32x128 {label}", shape, (3, 65, 257), m, probe(m)[0], aim=(("ring4", label),))
    # the staging limit (16-byte chunks a workgroup stages per plane) at equality: four waves, the y extent growing under a fixed box_x
    env4 = (("LSR_PLANAR_WAVES", "4"),)
    stage = lambda s: planar(1.0, s, 0.0, 0.0, -1.95)                                 # noqa: E731
    last = bisect(lambda s: planar_tile_index(probe(matrix(stage(s)), env4), 4) == 0, 1.0, 8.0)
    for label, s in (("last", last), ("next", next_up(last))):
        shape, m = fit(stage(s), (2, 33, 257))
        _add("planar_tile", f"staging limit {label}", shape, (2, 33, 257), m, probe(m, env4)[0], env=env4, aim=(("staging", label),))
    # in-plane extents about an integer: |b| (32 - 1) = 62 and |e| (128 - 1) = 254 exactly, one double below, one above
    for axis, whole in (("y", 2.0), ("x", 2.0)):
        for label, v in (("below", next_down(whole)), ("on", whole), ("above", next_up(whole))):
            for sign in (1.0, -1.0):
                rows = planar(0.5, sign * v, 0.0, 0.0, 1.0) if axis == "y" else planar(0.5, 1.0, 0.0, 0.0, sign * v)
                shape, m = fit(rows, (2, 65, 257), frac=0.0 if label == "on" else 0.3125)
                _add("planar_tile", f"extent {axis} {label} the integer {'+' if sign > 0 else '-'}", shape, (2, 65, 257), m, probe(m)[0],
                     aim=(("whole", axis + label),))
    # ... and the doubles at which box_y and box_x step
    for axis, field, start in (("y", 4, 1.3), ("x", 5, 1.3)):
        fam = (lambda s: planar(1.0, -s, 0.0, 0.0, 1.0)) if axis == "y" else (lambda s: planar(1.0, 1.0, 0.0, 0.0, -s))
        base = probe(matrix(fam(start)))
        last = bisect(lambda s: probe(matrix(fam(s)))[field] == base[field] and probe(matrix(fam(s)))[0] == 1, start, 2.0 * start)
        for label, s in (("last", last), ("next", next_up(last))):
            shape, m = fit(fam(s), (2, 65, 257))
            _add("planar_tile", f"box_{axis} step {label}", shape, (2, 65, 257), m, probe(m)[0], aim=(("step", axis + label),))


# ---- planar_z ---------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def ring_thresholds():
    """``(the last a with a ring of 3, the last a the planar kernel takes)``."""
    z = lambda a: matrix(planar(a, 1.0, 0.0, 0.0, 1.0))                               # noqa: E731
    return (bisect(lambda a: probe(z(a))[6] == 3, 0.5, 4.0), bisect(lambda a: probe(z(a))[0] == 1, 0.5, 4.0))


def _build_planar_z():
    ring3, ring4 = ring_thresholds()
    inplane = rotation(1.0, 3.0)
    small, mixed = (20, 70), (40, 150)          # one ragged tile; a full tile beside ragged ones (counted and uncounted waits)

    def add(name, a, tz, zi, zo, plane=small, **kw):
        rows = np.array(inplane)
        rows[0, 0] = a
        shape, m = fit(rows, (zo,) + plane)
        m[0, 3] = tz
        shape = (zi,) + shape[1:]
        _add("planar_z", name, shape, (zo,) + plane, m, probe(m)[0], **kw)

    add("a = 1", 1.0, 0.0, 20, 17, mixed)
    add("a = 1, fractional tz", 1.0, 0.37, 20, 17)
    add("a = the last of the ring of 3", ring3, 0.25, 20, 17, aim=(("ring", "3 last"),))
    add("a = the first of the ring of 4", next_up(ring3), 0.25, 24, 17, mixed, aim=(("ring", "4 first"),))
    add("a = the last the kernel takes", ring4, 0.125, 30, 17, aim=(("ring", "4 last"),))
    add("a = minus the last the kernel takes", -ring4, 24.5, 30, 17, mixed)
    add("a = the first the kernel refuses", next_up(ring4), 0.125, 30, 17, aim=(("ring", "refused"),))
    add("a = minus the first the kernel refuses", -next_up(ring4), 24.5, 30, 17)
    add("a = 0", 0.0, 3.25, 8, 17, mixed)
    add("a = 0 on a plane", 0.0, 3.0, 8, 5)
    add("a small: every source plane many times", 0.0625, 0.03125, 4, 33)
    add("a = 0.37, tz fractional", 0.37, 0.61, 14, 33, mixed)
    add("a = -0.73", -0.73, 22.9, 24, 33)
    add("a = 1.37", 1.37, -3.3, 40, 33)
    add("entered and left inside a chunk", 1.0, -5.5, 12, 33, mixed)                   # planes 6 .. 16 inside: chunk 0 starts outside, 1 starts inside
    add("entered and left inside a chunk, a < 0", -1.0, 22.5, 12, 33)
    add("first planes inside, the rest outside", 1.0, 0.5, 9, 33)
    add("every plane outside", 1.0, -100.0, 12, 33, mixed)
    add("every plane above", 0.5, 100.0, 12, 17)
    for zo in (1, 15, 16, 17, 32, 33):
        add(f"Zo = {zo}", 0.9, 0.45, 31, zo, mixed if zo in (16, 33) else small)
    for zi in (1, 2):
        add(f"Zi = {zi}", 0.25, -0.5, zi, 17)
        add(f"Zi = {zi}, on the planes", 1.0, -1.0, zi, 5)


# ---- planar_map -------------------------------------------------------------------------------------------------------------------


def _build_planar_map():
    for out_shape in ((2, 270, 130), (2, 40, 1100)):
        for patch in (None, "1,64", "64,1"):
            env = () if patch is None else (("LSR_PLANAR_PATCH", patch),)
            rows = rotation(0.97, -2.0)
            shape, m = fit(rows, out_shape, cap=(3, 288, 1104))
            _add("planar_map", f"{out_shape} patch {patch or 'default'}", shape, out_shape, m, 1, env=env, aim=(("patch", patch or "8,8"),))
    # 8 x 8 patches: more than one along both axes at the smallest tile (8 x 64 under four waves: patches of 64 x 512)
    env = (("LSR_PLANAR_WAVES", "4"),)
    below, last = tile_threshold(3, 4)
    rows = _tile_family(3)(0.5 * (below + last), 2)
    shape, m = fit(rows, (1, 80, 600))
    _add("planar_map", "8x64 tiles, 2 x 2 patches", shape, (1, 80, 600), m, probe(m, env)[0], env=env, aim=(("patch", "8,8"),))


# ---- box_shape --------------------------------------------------------------------------------------------------------------------


def tilt(about, alpha, az=1.0, s=1.0):
    """A tilt of ``alpha`` about y, about x or both, the plane scaled by ``s`` and z by ``az``."""
    y, x = (about in ("y", "both")), (about in ("x", "both"))
    return [[az, alpha * x, alpha * y], [-alpha * x, s, 0.02 * (about == "both")], [-alpha * y, 0.0, s]]


def box_walk(m):
    """The compiled walk the launcher picks: which of z_in, y_in, x_in depend on zo (bit 0, 1, 2), as ``launch_shape`` has it."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    dz, dy, dx = m[0, 0] != 0.0, m[1, 0] != 0.0, m[2, 0] != 0.0
    return 5 if dz and not dy and dx else (3 if dz and dy and not dx else 7)


@functools.lru_cache(maxsize=None)
def box_search():
    """``{(block, walk): rows}``: the first map of a fixed search order for which the plan picks the block under the walk."""
    found = {}
    for about in ("y", "x", "both"):
        for alpha in (0.02, 0.05, 0.1, 0.2, 0.3, 0.45, 0.6, 0.8, 1.0, 1.3, 1.7, 2.2):
            for az in (1.0, 0.5, 2.0, 3.0):
                for s in (1.0, 0.7, 1.4, 2.0, 0.3):
                    for flip in (1.0, -1.0):
                        rows = np.array(tilt(about, alpha, az, s)) * flip
                        p = probe(matrix(rows))
                        if p[0] == 2:
                            found.setdefault((p[1:4], box_walk(matrix(rows))), rows)
    # z_in steep in yo under a small z step and a decimating y: the blocks that are short along y
    for steep in (0.5, 1.0, 2.0, 3.0):
        for az in (0.3, 0.5):
            for s in (2.0, 3.0, 4.0):
                for my, mx in ((-0.1, 0.0), (0.0, 0.05), (-0.1, 0.05)):
                    rows = np.array([[az, steep, 0.0], [my, s, 0.0], [mx, 0.0, 1.0]])
                    p = probe(matrix(rows))
                    if p[0] == 2:
                        found.setdefault((p[1:4], box_walk(matrix(rows))), rows)
    return found


def _build_box_shape():
    k = 0
    for (block, walk), rows in sorted(box_search().items(), key=lambda kv: (BOX_BLOCKS.index(kv[0][0]), kv[0][1])):
        out_shape = tuple(extents(t)[(k + j) % 5] if (k + j) % 5 else 2 * t + 1 for j, t in enumerate(block))
        if k % 4 == 3:
            out_shape = (extents(block[0])[k % 5], extents(block[1])[(k + 1) % 5], extents(block[2])[(k + 2) % 5])
        shape, m = fit(rows, out_shape)
        _add("box_shape", f"block {block} walk {walk}", shape, out_shape, m, 2, aim=(("block", block), ("walk", walk)))
        k += 1
    # the doubles at which the box steps by one plane, one row, one chunk of columns
    for axis, (r, c), base in (("z", (0, 2), np.array(tilt("both", 0.11))), ("y", (1, 1), np.array(tilt("both", 0.11))),
                               ("x", (2, 2), np.array(tilt("both", 0.03)))):
        def fam(v, r=r, c=c, base=base):
            rows = base.copy()
            rows[r, c] = v
            return rows
        start = float(base[r, c])
        p0 = probe(matrix(fam(start)))
        last = bisect(lambda v: probe(matrix(fam(v)))[:7] == p0[:7], start, start + 0.5)
        for label, v in (("last", last), ("next", next_up(last))):
            for sign in (1.0, -1.0):
                rows = fam(v)
                rows[r] *= sign
                shape, m = fit(rows, (17, 17, 129))
                _add("box_shape", f"box_{axis} step {label} {'+' if sign > 0 else '-'}", shape, (17, 17, 129), m, probe(m)[0],
                     aim=(("step", axis + label),))
    # the last map the box kernel takes and the first it leaves to the gather kernel
    fam = lambda s: np.array(tilt("both", 0.3, 1.0, 1.0)) * s                         # noqa: E731
    last = bisect(lambda s: probe(matrix(fam(s)))[0] == 2, 1.0, 64.0)
    for label, s in (("last", last), ("next", next_up(last))):
        shape, m = fit(fam(s), (17, 17, 129))
        _add("box_shape", f"largest box {label}", shape, (17, 17, 129), m, probe(m)[0], aim=(("limit", label),))
    # more than four blocks along each axis, both block orders
    for linear in ("0", "1"):
        shape, m = fit(tilt("both", 0.04), (40, 70, 150))
        _add("box_shape", f"(40, 70, 150) LSR_BOX_LINEAR={linear}", shape, (40, 70, 150), m, 2, env=(("LSR_BOX_LINEAR", linear),),
             aim=(("linear", int(linear)),))


# ---- box_kind ---------------------------------------------------------------------------------------------------------------------

KIND_ROWS = [[1.0, 2.0 ** -5, 2.0 ** -6], [-(2.0 ** -5), 1.0, 2.0 ** -7], [-(2.0 ** -4), 2.0 ** -6, 1.0]]   # dyadic: every coordinate is exact
KIND_OUT, KIND_IN = (32, 16, 96), (20, 13, 48)
KIND_SHIFTS = (2.0, 2.0, 3.0)
KIND_BLOCK = (0, 0, 0)                       # the block whose corner the cases move


def block_corners(m, plan, out_shape, blk):
    """``(cmin, cmax)`` per source axis of the block ``blk`` (indices per axis) as ``locate`` of the box kernel computes them."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    lo = [b * t for b, t in zip(blk, plan[1:4])]
    hi = [min(l + t, n) - 1 for l, t, n in zip(lo, plan[1:4], out_shape)]
    out = []
    for r in m:
        a = [float(hi[k] if r[k] < 0.0 else lo[k]) for k in range(3)]
        b = [float(lo[k] if r[k] < 0.0 else hi[k]) for k in range(3)]
        out.append((float(((a[0] * r[0] + a[1] * r[1]) + a[2] * r[2]) + r[3]), float(((b[0] * r[0] + b[1] * r[1]) + b[2] * r[2]) + r[3])))
    return out


def block_kinds(m, plan, out_shape, shape, grid):
    """The kind of every block of a box-kernel launch, restated from the kernel's predicates: a dict kind -> count."""
    counts = {"interior": 0, "border": 0, "blind": 0}
    last = [float(n - 1) for n in shape]
    for bz in range(plan[8]):
        for by in range(plan[9]):
            for bx in range(plan[10]):
                cs = block_corners(m, plan, out_shape, (bz, by, bx))
                if grid:
                    blind = any(not (hi > -1.0) or not (lo < l + 1.0) for (lo, hi), l in zip(cs, last))
                else:
                    blind = any(hi < 0.0 or lo > l for (lo, hi), l in zip(cs, last))
                interior = all(lo >= 0.0 and hi < l for (lo, hi), l in zip(cs, last))
                counts["interior" if interior else ("blind" if blind else "border")] += 1
    return counts


def _build_box_kind():
    base = matrix(KIND_ROWS, KIND_SHIFTS)
    plan = probe(base)
    for axis in range(3):
        n = KIND_IN[axis]
        # the corner the kind is decided on, and the value it is compared with: interior (min >= 0, max < n - 1), blind under
        # "constant" (max < 0, min > n - 1) and under "grid-constant" (max > -1, min < n)
        for which, value in (("min", 0.0), ("max", n - 1.0), ("max", 0.0), ("min", n - 1.0), ("max", -1.0), ("min", float(n))):
            def corner(shift, axis=axis, which=which):
                m = base.copy()
                m[axis, 3] = shift
                return block_corners(m, plan, KIND_OUT, KIND_BLOCK)[axis][0 if which == "min" else 1]
            exact = base[axis, 3] + (value - corner(base[axis, 3]))
            assert corner(exact) == value
            below = above = exact
            while corner(below) == value:        # (the shift's doubles are finer than the coordinate's where the corner is far from 0)
                below = next_down(below)
            while corner(above) == value:
                above = next_up(above)
            for label, shift in (("on", exact), ("the double below", below), ("the double above", above)):
                m = base.copy()
                m[axis, 3] = shift
                _add("box_kind", f"{'zyx'[axis]} {which} {label} {value:g}", KIND_IN, KIND_OUT, m, 2,
                     aim=(("axis", axis), ("which", which), ("value", value), ("at", label), ("corner", corner(shift))))


# ---- grid_points ------------------------------------------------------------------------------------------------------------------


def _build_grid_points():
    shape = (6, 12, 16)
    n = np.array(shape, dtype=np.float64)
    eye = np.eye(3)
    wide = tuple(v + 3 for v in shape)

    def add(name, rows, shifts, out_shape=wide, shape=shape):
        m = matrix(rows, shifts)
        _add("grid_points", name, shape, out_shape, m, probe(m)[0], aim=(("whole", float(np.all(m == np.floor(m)))),))

    add("identity", eye, (0, 0, 0), shape)
    add("identity from -1", eye, (-1, -1, -1))
    add("identity from -2", eye, (-2, -2, -2))
    add("identity from +1", eye, (1, 1, 1), shape)
    add("flips", -eye, n - 1, shape)
    add("flips from n", -eye, n)
    add("flip x from n + 1", np.diag([1.0, 1.0, -1.0]), (-1, -1, shape[2] + 1))
    add("2 x decimation", 2 * eye, (-2, -2, -2), (5, 8, 10))
    add("2 x decimation, odd start", 2 * eye, (-1, -1, -1), (5, 8, 10))
    add("2 x decimation in the plane", np.diag([1.0, 2.0, 2.0]), (-1, -2, -2), (9, 8, 10))
    add("2 x decimation in the plane, odd start", np.diag([1.0, 2.0, -2.0]), (-2, -1, 17), (9, 8, 10))
    add("0.5 x upsampling", 0.5 * eye, (-1, -1, -1), (16, 28, 36))
    add("0.5 x upsampling, flipped", -0.5 * eye, n, (16, 28, 36))
    for e in (30, 52):
        for sign in (1.0, -1.0):
            d = sign * 2.0 ** -e
            s = "+" if sign > 0 else "-"
            add(f"identity {s}2^-{e}", eye, (d, d, d), shape)
            add(f"identity from -1 {s}2^-{e}", eye, (-1 + d, -1 + d, -1 + d))
            add(f"flips from n {s}2^-{e}", -eye, n + d)
            add(f"flips from n - 1 {s}2^-{e}", -eye, n - 1 + d, shape)
    # the same through the box kernel: z_in = zo + yo, then x_in = xo + zo, whole numbers throughout
    tall = (24, 20, 16)
    couple = np.array([[1.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    add("coupled z and y", couple, (-1, -1, -1), (13, 23, 19), tall)
    add("coupled z and y, flipped", couple * np.array([[-1], [-1], [-1]]), (24, 20, 16), (13, 23, 19), tall)
    couple_x = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 1.0]])
    add("coupled x and z", couple_x, (-1, -1, -2), (26, 23, 11), tall)
    for e in (30, 52):
        add(f"coupled z and y +2^-{e}", couple, (-1 + 2.0 ** -e,) * 3, (13, 23, 19), tall)
        add(f"coupled z and y -2^-{e}", couple, (-1 - 2.0 ** -e,) * 3, (13, 23, 19), tall)
        add(f"coupled x and z -2^-{e}", couple_x, (-1 - 2.0 ** -e, -1 + 2.0 ** -e, -2 - 2.0 ** -e), (26, 23, 11), tall)


# ---- strides ----------------------------------------------------------------------------------------------------------------------

STRIDE_MAPS = {1: rotation(1.03, 4.0, a=0.8), 2: tilt("both", 0.06), 0: (np.array(tilt("both", 0.9, 2.0, 3.0)))}


def _build_strides():
    for path, rows in STRIDE_MAPS.items():
        for xi in (72, 70):
            for i, in_pad in enumerate((0, 4, 12)):
                for pad_value in (0.0, 3.0e30):
                    out_shape = (9, 21, 75)
                    shape, m = fit(rows, out_shape)
                    shape = (max(shape[0], 6), max(shape[1], 16), xi)
                    case = _add("strides", f"path {path} Xi={xi} pitch +{in_pad} padding {pad_value:g}", shape, out_shape, m, path,
                                in_pad=in_pad, in_rows=(0, 3, 1)[i], pad_value=pad_value, out_pad=(5, 1, 0)[i], out_rows=(2, 0, 3)[i])
                    assert case.plan()[0] == path, (case.name, case.plan())
        shape, m = fit(rows, (9, 21, 75))
        shape = (max(shape[0], 6), max(shape[1], 16), 72)
        _add("strides", f"path {path} on a pitch of Xi + 1", shape, (9, 21, 75), m, 0, in_pitch=73, pad_value=3.0e30, out_pad=3, out_rows=1)


# ---- content ----------------------------------------------------------------------------------------------------------------------

CONTENTS = ("negative", "huge", "denormal", "zeros", "constant", "nonfinite interior", "nonfinite face", "nonfinite last")
CONTENT_SHAPE, CONTENT_OUT = (20, 40, 136), (19, 43, 140)
CONTENT_MAPS = {1: matrix(rotation(0.98, 1.5, a=0.9), (0.3517, 0.6113, -1.2719)),
                2: matrix(tilt("both", 0.013, 0.97, 0.99), (0.3517, 0.6113, -1.2719))}
CONSTANT = float(np.float32(311.37))
NONFINITE = (np.nan, np.inf, -np.inf)


def _build_content():
    for content in CONTENTS:
        for path, m in CONTENT_MAPS.items():
            _add("content", f"{content} path {path}", CONTENT_SHAPE, CONTENT_OUT, m, path, content=content,
                 f32=content in ("negative", "constant"))
        _add("content", f"{content} gather", CONTENT_SHAPE, CONTENT_OUT, CONTENT_MAPS[2], 0, content=content, in_pitch=CONTENT_SHAPE[2] + 1,
             f32=content in ("negative", "constant"))


def nonfinite_at(c):
    """The three voxels of a non-finite volume that hold NaN, +inf, -inf."""
    z, y, x = c.shape
    if c.content == "nonfinite interior":
        return [(z // 2, y // 2, x // 2 + 3), (z // 2 - 3, y // 3, x // 3), (z // 2 + 3, y // 2 + 5, x // 4)]
    if c.content == "nonfinite face":       # on the faces between tiles (rows 32, columns 128) and blocks (planes 8, 16, rows 8k, columns 64)
        return [(8, 32, 128), (16, 8, 64), (7, 31, 63)]
    return [(z - 1, y // 2, x // 2), (z // 2, y - 1, x // 3), (z // 3, y // 3, x - 1)]


for _build in (_build_planar_tile, _build_planar_z, _build_planar_map, _build_box_shape, _build_box_kind, _build_grid_points,
               _build_strides, _build_content):
    _build()
CASES = list(_CASES)


def case(name):
    return _CASES[name]


def group(g):
    return [n for n in CASES if _CASES[n].group == g]


def is_finite(name):
    return not _CASES[name].content.startswith("nonfinite")


# ---- arrays -----------------------------------------------------------------------------------------------------------------------


def _rng(*parts):
    return np.random.default_rng([zlib.crc32(str(p).encode()) for p in parts])


@functools.lru_cache(maxsize=None)
def _content(content, shape):
    rng = _rng("affine", content, shape)
    if content == "uniform" or content.startswith("nonfinite"):
        v = rng.uniform(-50.0, 150.0, shape).astype(np.float32)
    elif content == "negative":
        v = rng.uniform(-65000.0, -1.0, shape).astype(np.float32)
    elif content == "huge":
        v = np.where(rng.random(shape) < 0.5, np.float32(-3e38), np.float32(3e38)).astype(np.float32)
        v[rng.random(shape) < 0.3] = np.float32(1.5)
    elif content == "denormal":
        v = (1e-40 * rng.standard_normal(shape)).astype(np.float32)
    elif content == "zeros":
        v = np.where(rng.random(shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        v[rng.random(shape) < 0.1] = np.float32(-2.5)
    elif content == "constant":
        v = np.full(shape, CONSTANT, dtype=np.float32)
    else:
        raise KeyError(content)
    return v


@functools.lru_cache(maxsize=None)
def source(name):
    """The float32 moving volume of a case (read-only)."""
    c = _CASES[name]
    v = _content(c.content, c.shape).copy()
    if c.content.startswith("nonfinite"):
        for at, value in zip(nonfinite_at(c), NONFINITE):
            v[at] = value
    v.setflags(write=False)
    return v


def source_buffer(c, pitch=None, pad_value=None):
    """The volume in its padded layout: ``Zi`` planes of ``plane`` floats, the padding holding ``pad_value``."""
    pitch = c.pitch if pitch is None else pitch
    rows = c.shape[1] + c.in_rows
    buf = np.full((c.shape[0], rows, pitch), c.pad_value if pad_value is None else pad_value, dtype=np.float32)
    buf[:, :c.shape[1], :c.shape[2]] = source(c.name)
    return buf


@dataclasses.dataclass(frozen=True)
class Expected:
    out: np.ndarray
    exact: np.ndarray
    inside: np.ndarray
    on_last: np.ndarray
    max_tap: np.ndarray        # max |tap| over the eight corners, cval counted where a tap is outside
    tap_nonfinite: np.ndarray  # some corner holds a NaN or an infinity


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """The restatement's result of a case under a border, computed once (read-only)."""
    c = _CASES[name]
    r = R.resample(source(name), c.m, c.out_shape, mode, c.cval)
    with np.errstate(all="ignore"):
        e = Expected(r.out, r.exact, r.inside, r.on_last, np.abs(r.taps).max(axis=0), ~np.isfinite(r.taps).all(axis=0))
    for f in dataclasses.fields(e):
        getattr(e, f.name).setflags(write=False)
    return e


def output_buffer(c):
    """A host buffer of ``Zo`` padded planes, every word the recognisable NaN."""
    return np.full(c.out_shape[0] * c.out_plane, PAYLOAD, dtype=np.uint32)


def window(c, buf):
    zo, yo, xo = c.out_shape
    return buf.view(np.float32).reshape(zo, yo + c.out_rows, c.out_pitch)[:, :yo, :xo]


def padding_intact(c, buf):
    """No word outside the window was written, and none inside it was left."""
    zo, yo, xo = c.out_shape
    words = buf.view(np.uint32).reshape(zo, yo + c.out_rows, c.out_pitch)
    inside = np.zeros(words.shape, dtype=bool)
    inside[:, :yo, :xo] = True
    return bool((words[~inside] == PAYLOAD).all()), bool((words[inside] != PAYLOAD).all())
