"""A float64 restatement of the SSD normal-equations kernel (``csrc/estimate_affine.hip``), its a-priori error bound, and
the cases shared by ``test_estimate_host.py`` (the restatement pinned on the CPU) and ``test_estimate_fp64_gpu.py`` (the
kernel against the restatement).

The rule restated (the kernel's header comment), per grid sample ``(zo, yo, xo) = (iz sz, iy sy, ix sx)`` of the target:

* moving coordinate per axis ``((m0 zo + m1 yo) + m2 xo) + m3``, every operation rounded on its own (the library is built
  without contraction), NOT a matrix product;
* the sample is kept when ``c >= 0 and c < n - 1`` on every axis of the moving volume;
* cell index = truncation, fraction ``f = c - j`` (exact), lerp along x, then y, then z; the gradient expressions of the
  header comment; ``x~ = (index - centre) * (1 / scale)``; ``r = (gain * M + offset) - T``;
* ``H = sum J J^T``, ``b = sum J r``, ``sse = sum r r``, ``n`` = the samples kept.

The per-sample rows ``J`` and ``r`` are float64 numpy expressions in the kernel's written order: each is the same IEEE
operation on the same operands, so they carry the kernel's own bits.  Only the sums are free: the kernel adds with one
fused multiply-add per term in a lane / wave / workgroup / host order; here every product and sum is taken in extended
precision (64-bit mantissa) by pairwise halving, and rounded to float64 once at the end.

Exact cases
-----------
Voxels are integers in 0 .. 15, matrix entries multiples of 1/4, gain a multiple of 1/2, offset an integer, the scale a
power of two <= 64 and the centre an integer or a half: every fraction is a multiple of 1/4, ``M`` of 1/64, the gradients
of 1/16, ``x~`` of 1/128, so ``J 2^12`` and ``r 2^12`` are integers.  While ``sum |J_i J_j| 2^24 < 2^53`` every partial sum
in ANY order is an integer below 2^53 in units of 2^-24 and float64 holds it: the kernel must return the restatement's
bits.  ``exact_integer_sums`` re-proves that per case in int64.

The a-priori bound of the generic cases
---------------------------------------
Model ``fl(a op b) = (a op b)(1 + d)``, ``|d| <= u = 2^-53``.  Every quantity gets a magnitude companion (a hat): a tap
its absolute value, a difference the SUM of its operands' hats, a product the product; the fractions are data (``c - j`` is
exact).  By induction a computed ``q`` differs from its exact value by at most ``k u q^`` with ``k`` the roundings on the
longest path to it:

    d = v1 - v0 ............ 1      gz = b1 - b0 ........................ 7      x~ = (idx - centre) * inv_s ... 3
    a = v0 + fx d .......... 3      gy = (a01-a00) + fz((a11-a10)-(a01-a00))  7      (1 / scale counts as one)
    b = a0 + fy (a1 - a0) .. 6      gx = e0 + fz (e1 - e0), e = d + fy (d' - d)  7
    M = b0 + fz (b1 - b0) .. 9      gain g ............................. 8      J[0..11] = (gain g) x~ .. 12
    r = (gain M + offset) - T  12   J[12] = M ... 9                              J[13] = 1 ............... 0

A term ``J_i J_j``, ``J_i r`` or ``r r`` therefore carries at most ``12 + 12 + 1 = 25`` roundings (the last one is the
product; the kernel's fused multiply-add spares it).  Adding ``n`` terms in any order costs at most ``n - 1`` more on every
term.  Any float64 evaluation of the same expressions thus differs from the exact sums of the exact terms by at most
``(n - 1 + 25) u sum J^_i J^_j``.  The sums here carry the same 25 per term and, being extended, less than one more
(19 roundings of 2^-64 each for n < 2^18); one is left for the second-order terms.  A float64 evaluation -- the kernel, the
oracle -- and this restatement therefore differ by at most ``c u sum J^_i J^_j`` with ``c = n + 52`` (``K_ROUNDINGS``); two
float64 evaluations differ from each other by at most the sum of their two bounds.  The bound is absolute per entry: where
two columns nearly cancel in
``H`` it does not shrink with the entry.

Against the oracle (``oracle.cpu_ref.affine_normal_equations``) the fractions are NOT the same data: its coordinates come
from a matrix product, whose roundings (and fusing) differ.  A coordinate has at most 6 roundings either way, each at most
``u c^`` with ``c^ = |m0| zo + |m1| yo + |m2| xo + |m3|``: two evaluations differ by ``delta <= 12 u c^``.  While no kept
coordinate lies within ``delta`` of an integer (``apriori_bound`` asserts it) both sides use the same cell and the same keep
decision, inside a cell ``M, gz, gy, gx`` are multilinear in the fractions with tap coefficients in [-1, 1], so each moves by
at most ``3 delta V`` (``V`` = the sum of the eight |taps|).  ``coordinate_roundings=12`` adds that first-order term; it is
zero in every comparison of the kernel with this restatement, which share the written order.
"""

import functools

from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -53
K_ROUNDINGS = 52
N_PARAMS = 14
EXACT_SCALE_BITS = 12          # J 2^12 and r 2^12 are integers in an exact case
N_THREADS = 256 * 256          # the launch: 256 workgroups of 256 threads, one grid sample per thread and trip

Rows = namedtuple("Rows", "J r Jhat rhat lipschitz index keep coord touched")


def stride3(strides):
    return (int(strides),) * 3 if np.isscalar(strides) else tuple(int(v) for v in strides)


def grid_samples(target_shape, strides):
    """``nz ny nx``: the launch's grid samples (kept or not)."""
    return int(np.prod([-(-n // s) for n, s in zip(target_shape, stride3(strides))]))


def written_order_coordinates(matrix, zd, yd, xd):
    m = np.asarray(matrix, np.float64)[:3]
    return [((m[a, 0] * zd + m[a, 1] * yd) + m[a, 2] * xd) + m[a, 3] for a in range(3)]


def _sum_extended(terms):
    """Column sums of float64 / extended ``terms`` (samples along axis 0) by pairwise halving in extended precision:
    at most ceil(log2 n) roundings of 2^-64 on any term."""
    assert np.finfo(np.longdouble).nmant >= 63, "the restatement's sums need an extended-precision long double"
    a = np.asarray(terms, np.longdouble)
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:], np.longdouble)
    while a.shape[0] > 1:
        if a.shape[0] % 2:
            a = np.concatenate([a, np.zeros((1,) + a.shape[1:], np.longdouble)])
        half = a.shape[0] // 2
        a = a[:half] + a[half:]
    return a[0]


def packed_sums(J, r):
    """The kernel's 121-entry row ``[H upper triangle row by row, b, sse, n]`` from the per-sample rows."""
    row = np.zeros(121)
    jl, rl = J.astype(np.longdouble), r.astype(np.longdouble)
    k = 0
    for i in range(N_PARAMS):
        row[k:k + N_PARAMS - i] = _sum_extended(jl[:, i:i + 1] * jl[:, i:]).astype(np.float64)
        k += N_PARAMS - i
    row[105:119] = _sum_extended(jl * rl[:, None]).astype(np.float64)
    row[119] = float(_sum_extended(rl * rl))
    row[120] = float(len(r))
    return row


def unpack(row):
    """``(H, b, sse, n)`` of a packed row, written out here on its own (``estimate._unpack`` is tested against it)."""
    h = np.zeros((N_PARAMS, N_PARAMS))
    k = 0
    for i in range(N_PARAMS):
        for j in range(i, N_PARAMS):
            h[i, j] = h[j, i] = row[k]
            k += 1
    return h, np.array(row[105:119], dtype=np.float64), float(row[119]), int(row[120])


def normal_equations_f64(moving, target, matrix, gain, offset, strides, centre, scale, rows=False):
    """``(H, b, sse, n)`` of one launch, and with ``rows=True`` a fifth item: the per-sample ``Rows`` of the kept samples
    in grid order (``J``, ``r``, their magnitude companions, the Lipschitz rows of the coordinate term, the grid sample
    numbers ``index``, the ``keep`` mask and the coordinates of the whole grid, and the moving voxels ``touched``)."""
    mov, tgt = np.asarray(moving, np.float64), np.asarray(target, np.float64)
    assert mov.ndim == 3 and tgt.ndim == 3 and min(mov.shape) >= 2
    gain, offset = float(gain), float(offset)
    st = stride3(strides)
    axes = [np.arange(0, n, s, dtype=np.int64) for n, s in zip(tgt.shape, st)]
    zo, yo, xo = (g.ravel() for g in np.meshgrid(*axes, indexing="ij"))      # z slowest: the kernel's sample number
    zd, yd, xd = zo.astype(np.float64), yo.astype(np.float64), xo.astype(np.float64)
    coord = written_order_coordinates(matrix, zd, yd, xd)
    keep = np.ones(len(zo), bool)
    for c, n in zip(coord, mov.shape):
        keep &= (c >= 0.0) & (c < float(n - 1))
    index = np.flatnonzero(keep)
    cz, cy, cx = (c[keep] for c in coord)
    jz, jy, jx = (c.astype(np.int64) for c in (cz, cy, cx))                 # truncation
    fz, fy, fx = cz - jz, cy - jy, cx - jx

    def tap(a, b, c_):
        return mov[jz + a, jy + b, jx + c_]

    v000, v001, v010, v011 = tap(0, 0, 0), tap(0, 0, 1), tap(0, 1, 0), tap(0, 1, 1)
    v100, v101, v110, v111 = tap(1, 0, 0), tap(1, 0, 1), tap(1, 1, 0), tap(1, 1, 1)
    a00, a01 = v000 + fx * (v001 - v000), v010 + fx * (v011 - v010)
    a10, a11 = v100 + fx * (v101 - v100), v110 + fx * (v111 - v110)
    b0, b1 = a00 + fy * (a01 - a00), a10 + fy * (a11 - a10)
    mval = b0 + fz * (b1 - b0)
    gz = b1 - b0
    gy = (a01 - a00) + fz * ((a11 - a10) - (a01 - a00))
    d00, d01, d10, d11 = v001 - v000, v011 - v010, v101 - v100, v111 - v110
    e0, e1 = d00 + fy * (d01 - d00), d10 + fy * (d11 - d10)
    gx = e0 + fz * (e1 - e0)
    tv = tgt[zo[keep], yo[keep], xo[keep]]
    r = (gain * mval + offset) - tv
    c3 = np.asarray(centre, np.float64)
    inv_s = 1.0 / float(scale)
    ones = np.ones(len(index))
    xt = [(zd[keep] - c3[0]) * inv_s, (yd[keep] - c3[1]) * inv_s, (xd[keep] - c3[2]) * inv_s, ones]
    cols = [(gain * g) * x for g in (gz, gy, gx) for x in xt] + [mval, ones]
    J = np.stack(cols, axis=1)
    out = unpack(packed_sums(J, r))
    if not rows:
        return out

    # magnitude companions: |tap|, a difference -> the sum of the hats, the fractions as they are
    w = {k: np.abs(v) for k, v in dict(v000=v000, v001=v001, v010=v010, v011=v011, v100=v100, v101=v101, v110=v110,
                                       v111=v111).items()}
    h00, h01 = w["v001"] + w["v000"], w["v011"] + w["v010"]
    h10, h11 = w["v101"] + w["v100"], w["v111"] + w["v110"]
    A00, A01, A10, A11 = w["v000"] + fx * h00, w["v010"] + fx * h01, w["v100"] + fx * h10, w["v110"] + fx * h11
    B0, B1 = A00 + fy * (A01 + A00), A10 + fy * (A11 + A10)
    M = B0 + fz * (B1 + B0)
    GZ = B1 + B0
    GY = (A01 + A00) + fz * ((A11 + A10) + (A01 + A00))
    E0, E1 = h00 + fy * (h01 + h00), h10 + fy * (h11 + h10)
    GX = E0 + fz * (E1 + E0)
    xh = [(np.abs(v[keep]) + abs(ck)) * inv_s for v, ck in zip((zd, yd, xd), c3)] + [ones]
    Jhat = np.stack([(abs(gain) * g) * x for g in (GZ, GY, GX) for x in xh] + [M, ones], axis=1)
    rhat = abs(gain) * M + abs(offset) + np.abs(tv)
    # coordinate term: per unit of u, 3 V c^ on M and on each gradient (module docstring)
    m = np.abs(np.asarray(matrix, np.float64)[:3])
    chat = np.max([m[a, 0] * zd + m[a, 1] * yd + m[a, 2] * xd + m[a, 3] for a in range(3)], axis=0)   # the whole grid
    lip = 3.0 * sum(w.values()) * chat[keep]
    L = np.stack([(abs(gain) * lip) * x for _ in range(3) for x in xh] + [lip, 0.0 * ones], axis=1)
    touched = np.zeros(mov.shape, bool)
    for a in (0, 1):
        for b in (0, 1):
            for c_ in (0, 1):
                touched[jz + a, jy + b, jx + c_] = True
    return out + (Rows(J, r, Jhat, rhat, (L, abs(gain) * lip, chat), index, keep, coord, touched),)


def apriori_bound(rows, coordinate_roundings=0):
    """``(bound on H 14x14, on b 14, on sse)``: ``(n + K_ROUNDINGS) u sum J^_i J^_j`` and likewise with ``r^`` (module
    docstring).  ``coordinate_roundings`` > 0 (12 against the oracle's matrix-product coordinates) adds the first-order
    effect of coordinates that differ by that many roundings, and asserts that no cell or keep decision can change."""
    n = len(rows.r)
    c = (n + K_ROUNDINGS) * U
    jh, rh = rows.Jhat, rows.rhat
    bh, bb, bs = c * (jh.T @ jh), c * (jh.T @ rh), c * float(rh @ rh)
    if coordinate_roundings:
        L, lr, chat = rows.lipschitz
        e = coordinate_roundings * U
        for cc, size in zip(rows.coord, rows.touched.shape):
            assert np.all(np.abs(cc[rows.keep] - np.rint(cc[rows.keep])) > e * chat[rows.keep]), "a coordinate on a cell boundary"
            assert np.all(np.abs(cc) > e * chat) and np.all(np.abs(cc - (size - 1)) > e * chat), "a coordinate on a keep limit"
        bh = bh + e * (L.T @ jh + jh.T @ L + e * (L.T @ L))
        bb = bb + e * (L.T @ rh + jh.T @ lr + e * (L.T @ lr))
        bs = bs + e * float(2.0 * (rh @ lr) + e * (lr @ lr))
    return bh, bb, bs


def worst_fraction(got, want, bound):
    """Largest ``|got - want| / bound`` over the entries (an entry with a zero bound must be equal)."""
    got, want, bound = (np.atleast_1d(np.asarray(v, np.float64)) for v in (got, want, bound))
    err = np.abs(got - want)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0))


def exact_integer_sums(rows):
    """The exactness proof of one case in int64: ``J 2^12`` and ``r 2^12`` must be integers and the widest sum of
    magnitudes must stay below 2^53 (in units of 2^-24); returns the packed row computed in integers, as float64."""
    scale = float(1 << EXACT_SCALE_BITS)
    ji, ri = rows.J * scale, rows.r * scale
    assert np.array_equal(ji, np.rint(ji)) and np.array_equal(ri, np.rint(ri)), "a per-sample row is not a multiple of 2^-12"
    ji, ri = ji.astype(np.int64), ri.astype(np.int64)
    full = np.concatenate([ji, ri[:, None]], axis=1)
    peak = int(np.abs(full).max(initial=0))
    assert peak * peak * max(len(ri), 1) < 2 ** 62                    # the int64 products below cannot overflow
    mags = np.abs(full).T @ np.abs(full)
    widest = int(mags.max(initial=0))
    assert widest < 2 ** 53, f"the widest sum needs {widest.bit_length()} bits"
    sums = full.T @ full
    row = np.zeros(121)
    row[:105] = sums[:N_PARAMS, :N_PARAMS][np.triu_indices(N_PARAMS)] / scale ** 2
    row[105:119] = sums[:N_PARAMS, N_PARAMS] / scale ** 2
    row[119] = sums[N_PARAMS, N_PARAMS] / scale ** 2
    row[120] = len(ri)
    return row, widest.bit_length()


# ---------------------------------------------------------------------------------------------------------------- cases

QUARTERS = np.array([[1.0, 0.25, 0.0, 0.5],
                     [0.0, 1.0, -0.25, 1.25],
                     [0.5, 0.0, 0.75, -0.75]])
QUARTERS_IN = np.array([[1.0, 0.25, 0.0, 0.5],          # the same, the x row shifted so that index 0 is kept
                        [0.0, 1.0, -0.25, 1.25],
                        [0.5, 0.0, 0.75, 0.75]])
FLAT_Z = np.array([[0.0, 0.0, 0.0, 0.25],               # every grid sample in the first moving cell along z
                   [0.0, 1.0, -0.25, 1.25],
                   [0.0, 0.0, 0.75, 0.75]])


@dataclass(frozen=True)
class Case:
    name: str
    moving_shape: tuple
    target_shape: tuple
    matrix: tuple                    # 3x4 as nested tuples
    gain: float
    offset: float
    strides: tuple = (1, 1, 1)
    scale: float = 64.0
    seed: int = 0
    n: int | None = None             # the closed-form number of kept samples, where there is one
    late_kept: bool = False          # multi-trip: samples beyond the launch's 65 536 threads must be kept
    same_volume: bool = False        # the target IS the moving volume
    constant_axis: int | None = None   # the moving volume does not vary along this axis
    nan_at: tuple | None = None      # a moving voxel set to NaN in the launch (the expectation is taken without it)
    sse: float | None = None
    extra: dict = field(default_factory=dict, compare=False, hash=False)

    @property
    def centre(self):
        return np.array([(n - 1) / 2 for n in self.target_shape])          # an integer or a half

    @property
    def m(self):
        return np.array(self.matrix, dtype=np.float64)

    @property
    def grid_samples(self):
        return grid_samples(self.target_shape, self.strides)


def _t(m):
    return tuple(tuple(float(v) for v in row) for row in np.asarray(m)[:3])


def _shifted(axis, by):
    m = np.eye(4)[:3].copy()
    m[axis, 3] = by
    return _t(m)


EXACT_CASES = [
    Case("one-sample", (4, 4, 4), (1, 1, 1), _t(QUARTERS_IN), 0.5, 3.0, scale=8.0, seed=1, n=1),
    Case("less-than-a-wave", (5, 6, 7), (2, 3, 5), _t(QUARTERS_IN), -1.5, -2.0, scale=4.0, seed=2, n=30),
    Case("ragged-workgroup-gain-0", (8, 10, 12), (3, 7, 9), _t(QUARTERS_IN), 0.0, 2.0, scale=16.0, seed=3),
    Case("every-thread-once", (34, 66, 56), (16, 64, 64), _t(QUARTERS), 1.0, -2.0, seed=4),
    Case("second-trip-of-workgroup-0", (2, 260, 200), (1, 257, 256), _t(FLAT_Z), 0.5, 1.0, scale=32.0, seed=5,
         late_kept=True),
    Case("ragged-second-trip", (40, 70, 90), (17, 64, 96), _t(QUARTERS), -1.5, 4.0, seed=6, late_kept=True),
    Case("seven-trips", (60, 110, 130), (33, 97, 131), _t(QUARTERS), 0.5, -3.0, seed=7, n=352609, late_kept=True),
    Case("strides-4-2-1", (60, 110, 130), (33, 97, 131), _t(QUARTERS), 1.0, 0.0, (4, 2, 1), seed=7),
    Case("strides-1-3-7", (60, 110, 130), (33, 97, 131), _t(QUARTERS), -1.5, 1.0, (1, 3, 7), seed=7),
    Case("strides-64-1-1", (60, 110, 130), (33, 97, 131), _t(QUARTERS), 0.5, 5.0, (64, 1, 1), seed=7),
]

_EPS = 2.0 ** -40


def _edge_cases():
    out = [
        Case("identity-2-2-2", (2, 2, 2), (2, 2, 2), _shifted(0, 0.0), 1.0, 0.0, scale=1.0, seed=11, n=1, same_volume=True,
             sse=0.0),
        Case("identity-5-6-7", (5, 6, 7), (5, 6, 7), _shifted(0, 0.0), 1.0, 0.0, scale=4.0, seed=12, n=4 * 5 * 6,
             same_volume=True, sse=0.0),
        Case("nothing-kept", (8, 8, 8), (8, 8, 8), _t(np.concatenate([np.eye(3), np.full((3, 1), 100.0)], axis=1)), 0.5, 1.0,
             scale=4.0, seed=13, n=0, sse=0.0),
        Case("nan-outside-the-taps", (6, 6, 6), (3, 3, 3), _shifted(0, 0.0), -1.5, 2.0, scale=2.0, seed=14, n=27,
             nan_at=(5, 4, 2)),
    ]
    shape = (5, 6, 7)
    for axis in range(3):
        rest = int(np.prod([n - 1 for k, n in enumerate(shape) if k != axis]))
        n_a = shape[axis]
        # idx - 1: index 0 drops out (coordinate -1), index n - 1 lands on n - 2 and stays
        out.append(Case(f"shift-minus-1-axis-{axis}", shape, shape, _shifted(axis, -1.0), 0.5, 1.0, scale=4.0, seed=20 + axis,
                        n=(n_a - 1) * rest, extra=dict(dropped=[0], axis=axis)))
        # idx + 1: the last two indices land on n - 1 and n
        out.append(Case(f"shift-plus-1-axis-{axis}", shape, shape, _shifted(axis, 1.0), -1.5, 0.0, scale=4.0, seed=23 + axis,
                        n=(n_a - 2) * rest, extra=dict(dropped=[n_a - 2, n_a - 1], axis=axis)))
        # 0 - 2^-40 is dropped, (n - 1) - 2^-40 is kept
        out.append(Case(f"ulp-below-axis-{axis}", shape, shape, _shifted(axis, -_EPS), 1.0, -1.0, scale=4.0, seed=26 + axis,
                        n=(n_a - 1) * rest, constant_axis=axis, extra=dict(dropped=[0], axis=axis)))
        # 0 + 2^-40 is kept, n - 1 + 2^-40 and n - 1 itself (the identity cases) are dropped
        out.append(Case(f"ulp-above-axis-{axis}", shape, shape, _shifted(axis, _EPS), 0.5, 2.0, scale=4.0, seed=29 + axis,
                        n=(n_a - 1) * rest, constant_axis=axis, extra=dict(dropped=[n_a - 1], axis=axis)))
    return out


EDGE_CASES = _edge_cases()


@functools.lru_cache(maxsize=None)
def _volumes(case):
    rng = np.random.default_rng(1000 + case.seed)
    mov = rng.integers(0, 16, case.moving_shape).astype(np.float32)
    if case.constant_axis is not None:
        mov = np.ascontiguousarray(np.broadcast_to(np.take(mov, [0], axis=case.constant_axis), mov.shape))
    tgt = mov if case.same_volume else rng.integers(0, 16, case.target_shape).astype(np.float32)
    for a in (mov, tgt):
        a.setflags(write=False)
    return mov, tgt


def volumes(case):
    """``(moving for the launch, target, moving for the expectation)``; the first carries the case's NaN, if any."""
    mov, tgt = _volumes(case)
    launch = mov
    if case.nan_at is not None:
        launch = mov.copy()
        launch[case.nan_at] = np.nan
    return launch, tgt, mov


@functools.lru_cache(maxsize=None)
def expectation(case):
    """``(H, b, sse, n, Rows)`` of an exact or edge case, computed once per process and shared."""
    _, tgt, mov = volumes(case)
    out = normal_equations_f64(mov, tgt, case.m, case.gain, case.offset, case.strides, case.centre, case.scale, rows=True)
    for a in out[:2] + tuple(out[4][:4]):
        a.setflags(write=False)
    return out


@dataclass(frozen=True)
class BoundCase:
    name: str
    moving_shape: tuple
    target_shape: tuple
    strides: tuple
    centre: tuple
    scale: float
    tilt: float = 4.0
    shift: tuple = (1.5, -2.0, 3.0)
    seeds: tuple = (5, 6)
    blobs: int = 25
    gain: float = 1.3
    offset: float = -2.0


BOUND_CASES = [BoundCase(f"legacy-stride-{'-'.join(map(str, st))}", (20, 37, 51), (18, 40, 45), st, (8.5, 19.5, 22.0), 22.5)
               for st in ((1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3))] + \
              [BoundCase(f"multi-trip-stride-{'-'.join(map(str, st))}", (32, 64, 72), (32, 64, 72), st, (15.5, 31.5, 35.5), 36.0,
                         tilt=3.0, shift=(0.8, -1.5, 2.2), seeds=(7, 8), blobs=60) for st in ((1, 1, 1), (2, 4, 4))]


@functools.lru_cache(maxsize=None)
def _scene_pair(moving_shape, target_shape, seeds, blobs):
    from tests.test_estimate import _scene

    mov, tgt = _scene(seeds[0], moving_shape, n=blobs), _scene(seeds[1], target_shape, n=blobs)
    for a in (mov, tgt):
        a.setflags(write=False)
    return mov, tgt


@functools.lru_cache(maxsize=None)
def bound_inputs(case):
    """``(moving, target, 4x4 matrix)`` of a bound case: the bead scenes and tilted matrices of ``test_estimate.py``."""
    from tests.test_estimate import _tilted

    mov, tgt = _scene_pair(case.moving_shape, case.target_shape, case.seeds, case.blobs)
    return mov, tgt, _tilted(case.target_shape, tilt=case.tilt, shift=case.shift)


@functools.lru_cache(maxsize=None)
def bound_expectation(case):
    mov, tgt, m = bound_inputs(case)
    return normal_equations_f64(mov, tgt, m, case.gain, case.offset, case.strides, np.array(case.centre), case.scale, rows=True)
