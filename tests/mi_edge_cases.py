"""Named cases that pin the two mutual-information kernels (``csrc/estimate_mi.hip``) and their host twins to
``tests/mi_ref.py`` at every dispatch edge.  Built once per process, read-only, shared by ``test_mi_edges_host.py`` (the
twins, the integer proofs and the per-case property checks) and ``test_mi_fp64_gpu.py`` (the kernels).

Sizes come from the library: ``T = lsr_affine_joint_histogram_blocks() * 256`` threads per launch, one grid sample per
thread and trip, 64 lanes per wave.

Exact cases.  Moving voxels are small integers (``4 B + r`` with a block value ``B`` in 0 .. 3 per 3 x 3 x 3 block and
``r`` in 0 .. 3, so whole neighbourhoods lie below, inside and above the moving range (4, 12), which is 8 wide and
strictly inside the span 0 .. 15), target voxels integers in -4 .. 67 against the range (0, 64), matrix entries
multiples of 1/8, the centre an integer, the scale 64 and ``dl`` the integer table ``((3 a + 5 b) % 7) - 3``, which
differs between neighbours along both axes.  A few samples per case get their eight taps planted -- ``p`` at x offset 0,
``p + 8`` at x offset 1 with ``p = v - 8 fx`` -- so that their value is exactly ``v`` = 4 (u == 0) or 12 (u == bins - 1)
while the interpolant's x gradient is 8: a rule that let such a sample contribute would change the sums.
"""

import functools

from dataclasses import dataclass, replace

import numpy as np

from tests import mi_cases
from tests import mi_ref as ref

WAVE = 64
THREADS = 256
EXACT_BITS = 15                    # every term of an exact case is a multiple of 2^-15 (mi_ref's docstring)
M_RANGE, T_RANGE = (4.0, 12.0), (0.0, 64.0)
RANGES = (T_RANGE, M_RANGE)
SCALE = 64.0
ALL_BINS = (4, 5, 8, 33, 63, 64)

# 3-D cases: every fraction varies, x and y of the moving volume advance a quarter voxel per target voxel
SOLID = ((2.5, 0.0, 0.0, 0.375),
         (0.125, 0.25, 0.0, 0.0),
         (0.0, 0.125, 0.25, 0.5))
# one target plane, two moving planes
PLANE = ((0.0, 0.0, 0.0, 0.5),
         (0.0, 0.75, 0.125, 0.5),
         (0.0, 0.125, 0.625, 0.375))
# one or a few long target rows: the moving volume grows along x alone
LINE = ((0.0, 0.0, 0.0, 0.5),
        (0.0, 0.25, 0.0, 0.25),
        (0.0, 0.0, 0.125, 0.5))
# a band of the target maps outside the moving volume on every side; (0, 0, 24) maps to (0, 0, 0) exactly
BAND = ((0.5, 0.125, 0.0, 0.0),
        (0.0, 0.75, 0.125, -3.0),
        (0.125, 0.0, 0.875, -21.0))
BAND_MOVING = (15, 81, 141)
# 64 consecutive x share one moving value (the coordinates do not depend on x) that varies along z and y
RAMP = ((0.5, 0.0, 0.0, 0.25),
        (0.0, 0.5, 0.0, 0.25),
        (0.0, 0.0, 0.0, 0.5))


@functools.lru_cache(maxsize=None)
def blocks():
    """Workgroups per launch, read from the library (both kernels must agree, or the cases need another look)."""
    from shrimpy_amd import _lib

    n = _lib.call_value("lsr_affine_joint_histogram_blocks")
    assert n >= 1 and n == _lib.call_value("lsr_affine_mi_gradient_blocks")
    return n


def launch_threads():
    return blocks() * THREADS


@dataclass(frozen=True)
class Case:
    name: str
    target: object                 # the target shape, or a function of T that returns it
    matrix: tuple
    bins: int
    stride: tuple = (1, 1, 1)
    moving: tuple | None = None    # None: the smallest moving volume that keeps every sample with coordinates >= 0
    seed: int = 0
    fill: str = "blocks"           # "blocks", "ramp" (one cell per wave, w1 != 0) or "lanes" (64 cells per wave)
    gradient: bool = True          # runs the gradient entry; then the five kinds of u must be present (``kinds``)
    kinds: bool = True
    trips: int | None = None       # the trips of the grid-stride loop that see a sample, where the case is about them

    @property
    def target_shape(self):
        return tuple(self.target(launch_threads())) if callable(self.target) else tuple(self.target)

    @property
    def moving_shape(self):
        if self.moving is not None:
            return tuple(self.moving)
        m = np.array(self.matrix)
        top = [sum(max(m[r, k], 0.0) * ((n - 1) // s * s) for k, (n, s) in enumerate(zip(self.target_shape, self.stride)))
               + m[r, 3] for r in range(3)]
        return tuple(max(int(np.floor(t)) + 2, 2) for t in top)

    @property
    def grid_samples(self):
        return int(np.prod([-(-n // s) for n, s in zip(self.target_shape, self.stride)]))

    @property
    def centre(self):
        return np.array([float(n // 2) for n in self.target_shape])

    @property
    def m(self):
        return np.array(self.matrix, dtype=np.float64)


# seeds at which a volume this small holds every kind of sample (test_mi_edges_host.py asserts that it does)
SMALL_SEEDS = (6, 0, 0, 0, 0, 0, 0)


def _counts():
    small = [("one-sample", (1, 1, 1), 5), ("wave-less-one", (1, 7, 9), 8), ("one-wave", (1, 8, 8), 4),
             ("wave-plus-one", (5, 1, 13), 33), ("workgroup-less-one", (3, 5, 17), 63), ("one-workgroup", (4, 8, 8), 64),
             ("workgroup-plus-one", (1, 1, 257), 5)]
    out = [Case(name, shape, PLANE if shape[0] == 1 and shape[1] > 1 else SOLID, bins, seed=seed, kinds=name != "one-sample")
           for seed, (name, shape, bins) in zip(SMALL_SEEDS, small)]
    out += [
        Case("every-thread-but-one", lambda t: (1, 1, t - 1), LINE, 8, seed=10, trips=1),
        Case("every-thread-once", lambda t: (1, 256, t // 256), PLANE, 33, seed=11, trips=1),
        Case("one-sample-on-the-second-trip", lambda t: (1, 3, (t + 1) // 3), LINE, 4, seed=12, trips=2),
        Case("second-trip-of-workgroup-0", lambda t: (1, 256, t // 256 + 1), PLANE, 63, seed=13, trips=2),
        Case("ragged-third-trip", lambda t: (3, 301, (2 * t + 7853) // 903), SOLID, 33, seed=14, trips=3),
    ]
    return out


BIG_TARGET, BIG_MOVING = (5, 257, 511), (12, 70, 140)      # more than five trips at 512 workgroups; the high x band is cut

COUNT_CASES = _counts()
BINS_CASES = [Case(f"five-trips-bins-{b}", BIG_TARGET, SOLID, b, moving=BIG_MOVING, seed=20) for b in ALL_BINS]
STRIDE_CASES = [
    Case("strides-2-3-5", BIG_TARGET, SOLID, 5, (2, 3, 5), seed=21),                    # none divides its axis
    Case("strides-7-1-2", BIG_TARGET, SOLID, 63, (7, 1, 2), seed=22),                   # 7 > 5: one sample along z
    Case("strides-1-300-1", BIG_TARGET, SOLID, 8, (1, 300, 1), moving=(12, 2, 140), seed=23),
]
GEOMETRY_CASES = [Case("band-outside", (3, 129, 257), BAND, 8, moving=BAND_MOVING, seed=30, trips=1)]
CONTENTION_CASES = [
    Case("wave-in-one-cell", (4, 6, 128), RAMP, 8, seed=40, fill="ramp", gradient=False, kinds=False),
    Case("wave-in-64-cells", (2, 9, 128), SOLID, 64, seed=41, fill="lanes"),
]
EXACT_CASES = COUNT_CASES + BINS_CASES + STRIDE_CASES + GEOMETRY_CASES + CONTENTION_CASES


def synthetic_dl(bins):
    a, b = np.meshgrid(np.arange(bins), np.arange(bins - 1), indexing="ij")
    return (((3 * a + 5 * b) % 7) - 3).astype(np.float64)


def _scene(case):
    """The part of a case that the volumes and the sample rows depend on (not the bin count)."""
    return replace(case, name="", bins=0, gradient=True, kinds=True, trips=None)


def _plant(mov, case):
    """Give a few kept samples a value of exactly 4 and exactly 12 with an x gradient of 8 (module docstring)."""
    index, _, _, cell, frac, _ = ref.geometry(mov.shape, case.target_shape, case.m, case.stride)
    n = len(index)
    if n < 16:
        return
    used = np.zeros(mov.shape, dtype=bool)
    for value, spots in ((M_RANGE[0], (0.07, 0.33, 0.61, 0.93)), (M_RANGE[1], (0.19, 0.47, 0.79))):
        for q in spots:
            for k in range(int(q * n), n):
                jz, jy, jx = cell[:, k]
                if not used[jz:jz + 2, jy:jy + 2, jx:jx + 2].any():
                    break
            else:
                continue
            used[jz:jz + 2, jy:jy + 2, jx:jx + 2] = True
            p = value - 8.0 * frac[2, k]
            mov[jz:jz + 2, jy:jy + 2, jx] = p
            mov[jz:jz + 2, jy:jy + 2, jx + 1] = p + 8.0


@functools.lru_cache(maxsize=None)
def _inputs(scene):
    rng = np.random.default_rng(7000 + scene.seed)
    ms, ts = scene.moving_shape, scene.target_shape
    if scene.fill == "ramp":
        # 5 + (z + y) % 6 in 5 .. 10: u = 7 (m - 4) / 8 has a fraction at every value, so w1 != 0; a constant target
        z, y, _ = np.meshgrid(*(np.arange(n) for n in ms), indexing="ij")
        mov = (5 + (z + y) % 6).astype(np.float32)
        tgt = np.full(ts, 21.0, dtype=np.float32)
    else:
        coarse = rng.integers(0, 4, tuple(-(-n // 3) for n in ms))
        big = np.repeat(np.repeat(np.repeat(coarse, 3, axis=0), 3, axis=1), 3, axis=2)[:ms[0], :ms[1], :ms[2]]
        mov = (4 * big + rng.integers(0, 4, ms)).astype(np.float32)
        if scene.fill == "lanes":
            tgt = np.broadcast_to((np.arange(ts[2]) % WAVE).astype(np.float32), ts).copy()      # bins = 64: a = x % 64
        else:
            tgt = rng.integers(-4, 68, ts).astype(np.float32)
        _plant(mov, scene)
    for a in (mov, tgt):
        a.setflags(write=False)
    return mov, tgt


def inputs(case):
    """``(moving, target)`` float32, read-only."""
    return _inputs(_scene(case))


@functools.lru_cache(maxsize=4)
def _rows(scene):
    mov, tgt = _inputs(scene)
    return ref.sample_rows(mov, tgt, scene.m, scene.stride)


def rows(case):
    return _rows(_scene(case))


def histogram_of(r, bins, ranges=RANGES):
    """``(hist uint64, n)`` of sample rows by the restatement's rule."""
    a, b0, _, f = ref.bin_rule(r.tv, r.mval, bins, ranges)
    w1 = np.floor(f * 65536.0 + 0.5).astype(np.int64)
    hist = np.zeros((bins, bins), dtype=np.int64)
    np.add.at(hist, (a, b0), ref.WEIGHT_ONE - w1)
    np.add.at(hist, (a, b0 + 1), w1)
    return hist.astype(np.uint64), int(r.tv.size)


@functools.lru_cache(maxsize=None)
def expected_histogram(case):
    hist, n = histogram_of(rows(case), case.bins)
    hist.setflags(write=False)
    return hist, n


@functools.lru_cache(maxsize=2)
def expected_terms(case):
    """``ref.Terms`` of an exact case at the synthetic ``dl``."""
    return ref.gradient_terms(rows(case), case.bins, RANGES, case.centre, SCALE, synthetic_dl(case.bins))


def raw_histogram(mov, tgt, matrix, stride, bins, ranges, hist_ptr, count_ptr):
    """The histogram entry as ``estimate.joint_histogram`` calls it (torch tensors: the kernel on the current stream,
    CPU tensors: the twin), into memory of the caller's."""
    import ctypes

    from shrimpy_amd import _lib
    from shrimpy_amd.estimate import _mi_call

    (t_lo, t_hi), (m_lo, m_hi) = ranges
    _mi_call("lsr_affine_joint_histogram_f32", mov, tgt, _lib.matrix12(np.asarray(matrix)[:3]),
             (ctypes.c_int * 3)(*ref.stride3(stride)), int(bins), ctypes.c_double(t_lo), ctypes.c_double(t_hi),
             ctypes.c_double(m_lo), ctypes.c_double(m_hi), hist_ptr, count_ptr)


def raw_gradient(mov, tgt, matrix, stride, centre, scale, bins, ranges, dl, partial):
    """The gradient entry as ``estimate.mi_gradient`` calls it, with the caller's ``dl`` and ``partial`` tensors (on the
    volumes' device): nothing is added up, nothing divided."""
    import ctypes

    from shrimpy_amd import _lib
    from shrimpy_amd.estimate import _f64p, _mi_call

    (t_lo, t_hi), (m_lo, m_hi) = ranges
    c = np.ascontiguousarray(centre, dtype=np.float64)
    assert dl.is_contiguous() and partial.is_contiguous() and dl.device == partial.device == tgt.device
    _mi_call("lsr_affine_mi_gradient_f32", mov, tgt, _lib.matrix12(np.asarray(matrix)[:3]),
             (ctypes.c_int * 3)(*ref.stride3(stride)), _f64p(c), ctypes.c_double(float(scale)), int(bins),
             ctypes.c_double(t_lo), ctypes.c_double(t_hi), ctypes.c_double(m_lo), ctypes.c_double(m_hi), dl.data_ptr(),
             partial.data_ptr())


# ------------------------------------------------------------------------------------------------------------ edge cases


@dataclass(frozen=True)
class EdgeCase:
    name: str
    bins: int = 8
    matrix: tuple = ((1.0, 0.0, 0.0, 0.5), (0.0, 1.0, 0.125, 0.25), (0.0, 0.0, 0.5, 0.0))    # fx = 0 at even x, 1/2 at odd
    moving_shape: tuple = (6, 8, 7)
    target_shape: tuple = (5, 6, 10)
    ranges: tuple = RANGES
    stride: tuple = (1, 1, 1)
    seed: int = 0
    moving_at: tuple = ()          # ((z, y, x), value) pairs written into the moving volume
    target_at: tuple = ()
    launch_only: bool = False      # the values of ``moving_at`` reach the launch, not the expectation: they must not matter
    n: int | None = None

    @property
    def m(self):
        return np.array(self.matrix, dtype=np.float64)

    @property
    def centre(self):
        return np.array([float(n // 2) for n in self.target_shape])

    @property
    def grid_samples(self):
        return int(np.prod([-(-n // s) for n, s in zip(self.target_shape, self.stride)]))


_NAN, _INF = float("nan"), float("inf")
_FAR = ((1.0, 0.0, 0.0, 100.0), (0.0, 1.0, 0.0, 100.0), (0.0, 0.0, 1.0, 100.0))
_IDENTITY = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0))

EDGE_CASES = [
    EdgeCase("target-nan-inf-zero-and-range-ends", bins=5, seed=1,
             target_at=(((0, 0, 0), _NAN), ((1, 2, 3), _INF), ((2, 3, 4), -_INF), ((3, 1, 2), -0.0), ((3, 4, 5), 0.0),
                        ((4, 2, 6), 64.0), ((0, 5, 7), _NAN), ((1, 1, 1), 63.96875))),
    EdgeCase("moving-nan-at-a-tap", seed=2, moving_at=(((2, 3, 2), _NAN),)),
    EdgeCase("moving-plus-inf-at-a-tap", seed=3, moving_at=(((2, 3, 2), _INF),)),
    EdgeCase("moving-minus-inf-at-a-tap", bins=4, seed=4, moving_at=(((3, 4, 1), -_INF),)),
    EdgeCase("moving-inf-beside-minus-inf", bins=33, seed=5, moving_at=(((2, 3, 2), _INF), ((2, 3, 3), -_INF), ((4, 1, 1), _NAN))),
    EdgeCase("negative-zero", bins=5, seed=6, ranges=((0.0, 64.0), (0.0, 8.0)),
             moving_at=tuple(((z, y, x), -0.0) for z in (1, 2) for y in (2, 3) for x in (1, 2, 3)),
             target_at=(((1, 2, 3), -0.0), ((1, 2, 4), -0.0))),
    EdgeCase("nothing-kept", matrix=_FAR, seed=7, n=0),
    EdgeCase("nan-outside-every-tap", matrix=_IDENTITY, moving_shape=(7, 8, 12), target_shape=(3, 4, 5), seed=8,
             moving_at=(((5, 2, 2), _NAN), ((1, 6, 3), _INF), ((2, 2, 9), -_INF)), launch_only=True, n=60),
]


@functools.lru_cache(maxsize=None)
def edge_inputs(case):
    """``(moving for the launch, target, moving for the expectation)``."""
    rng = np.random.default_rng(9000 + case.seed)
    mov = rng.integers(0, 16, case.moving_shape).astype(np.float32)
    tgt = rng.integers(-4, 68, case.target_shape).astype(np.float32)
    for where, value in case.target_at:
        tgt[where] = value
    launch = mov.copy()
    for where, value in case.moving_at:
        launch[where] = value
    expect = mov if case.launch_only else launch
    for a in (launch, tgt, expect):
        a.setflags(write=False)
    return launch, tgt, expect


@functools.lru_cache(maxsize=None)
def edge_rows(case):
    _, tgt, expect = edge_inputs(case)
    return ref.sample_rows(expect, tgt, case.m, case.stride)


@functools.lru_cache(maxsize=None)
def edge_expected(case):
    """``(hist, n, Terms at the synthetic dl)``."""
    r = edge_rows(case)
    hist, n = histogram_of(r, case.bins, case.ranges)
    return hist, n, ref.gradient_terms(r, case.bins, case.ranges, case.centre, SCALE, synthetic_dl(case.bins))


# ----------------------------------------------------------------------------------------------------------- bound cases


@dataclass(frozen=True)
class BoundCase:
    name: str
    bins: int
    stride: object
    large: bool = False


BOUND_CASES = [BoundCase("general-bins-8-stride-1", 8, 1), BoundCase("general-bins-32-stride-2", 32, 2),
               BoundCase("general-bins-64-strides-1-2-3", 64, (1, 2, 3)), BoundCase("two-trips-bins-32", 32, 1, large=True)]


@functools.lru_cache(maxsize=None)
def bound_inputs(case):
    """``(moving, target, matrix, ranges, centre, scale)``: the generic pair of ``mi_cases``, or a (32, 64, 72) bead
    scene under a 3 degree tilt -- 147 456 grid samples, more than one trip."""
    if not case.large:
        mov, tgt, m, ranges = mi_cases.general_pair()
        return mov, tgt, m, ranges, mi_cases.CENTRE, mi_cases.SCALE
    from tests.test_estimate import _scene as beads, _tilted

    shape = (32, 64, 72)
    mov, tgt = beads(7, shape, n=60), beads(8, shape, n=60)
    ranges = ((float(tgt.min()), float(tgt.max())), (float(mov.min()), float(mov.max())))
    return mov, tgt, _tilted(shape, tilt=3.0, shift=(0.8, -1.5, 2.2)), ranges, np.array([15.5, 31.5, 35.5]), 36.0


@functools.lru_cache(maxsize=None)
def bound_rows(case):
    mov, tgt, m, _, _, _ = bound_inputs(case)
    return ref.sample_rows(mov, tgt, m, case.stride)


def bound_expected(case, hist):
    """``(gradient, bound)`` of a bound case with ``dL`` from ``hist``: the restatement's normalised gradient and the
    a-priori bound on a float64 evaluation that formed its own ``dL`` from the same histogram."""
    _, _, _, ranges, centre, scale = bound_inputs(case)
    r = bound_rows(case)
    t = ref.gradient_terms(r, case.bins, ranges, centre, scale, ref.d_log(hist))
    n = int(r.tv.size)
    return t.sums / n, ref.gradient_bound(t, n, ref.d_log_slack(hist))
