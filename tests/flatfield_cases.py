"""The cases of the flat-field tests (``tests/test_flatfield_host.py``, ``tests/test_flatfield_gpu.py``), sized from the exported
tiling (``lsr_flatfield_tiling``): with ``c`` pixels per workgroup, ``g`` z phases per pixel and ``u`` loads in flight per thread,

* the plane is ``7 x 37 = 259`` pixels: two full workgroups and one of 3 real pixels and ``c - 3`` clamped duplicates;
* ``Z``: 1 .. 5 (phases without a sample), ``g u - 4 .. g u + 4`` (the full-batch condition on both sides, tails of 0 to 3 per
  phase), ``2 g u - 4, 2 g u - 3, 2 g u, 2 g u + 1``, and 300;
* engineered columns (``CLASSES``): every class of the per-pixel state machine -- no split, a split at each key byte, in the float
  and in the count mode, the lower middle element's bin even and odd -- with decoys around the two middle elements, and
  NEIGHBOURING PIXELS OF DIFFERENT CLASSES, so that shared, split and finished pixels sit side by side in a pass;
* run counting, fallbacks out of the count mode, NaNs, infinities, negative-only, denormal and mixed-zero stacks, the counter limit
  ``Z = 65535``, the uint16 forms of the count cases, and the planes and volumes of the mean and the division.

Every array is read-only: the tests share them.  ``CASES`` names every median case: ``volume(name)`` builds it.
"""

import functools
import zlib

import numpy as np

from shrimpy_amd import flatfield as F
from tests import flatfield_ref as R

COLS, PHASES, LOADS, REFUSED_Z = F.tiling()
PLANE = (7, 37)
NPIX = PLANE[0] * PLANE[1]
GU = PHASES * LOADS

Z_SMALL = [1, 2, 3, 4, 5]
Z_BATCH = [GU - 4, GU - 3, GU - 1, GU, GU + 1, GU + 3, GU + 4]
Z_TWO = [2 * GU - 4, 2 * GU - 3, 2 * GU, 2 * GU + 1]
Z_LIST = Z_SMALL + Z_BATCH + Z_TWO + [300]
Z_DECOYS = 60                               # from here on a column has room for every decoy


def _k(b0, b1, b2, b3):
    return (b0 << 24) | (b1 << 16) | (b2 << 8) | b3


def _fk(v):
    return int(R.key(np.float32(v)).ravel()[0])


# (name, count mode, key of a, key of b, the level of the split or None); in the count mode the key is the integer itself
CLASSES = [
    ("none", False, _k(0xBF, 0x85, 0x47, 0x23), _k(0xBF, 0x85, 0x47, 0x23), None),
    ("sign, even bin", False, _k(0x40, 0x7A, 0x47, 0x23), _k(0xBF, 0x85, 0x10, 0x11), 0),
    ("sign, odd bin", False, _k(0x41, 0x7A, 0x47, 0x23), _k(0xBE, 0x85, 0x10, 0x11), 0),
    ("exponent, even bin", False, _k(0xBE, 0x85, 0x47, 0x23), _k(0xBF, 0x85, 0x10, 0x11), 0),
    ("exponent, odd bin", False, _k(0xBF, 0x85, 0x47, 0x23), _k(0xC2, 0x85, 0x10, 0x11), 0),
    ("level 1, even bin", False, _k(0xBF, 0x84, 0x47, 0x23), _k(0xBF, 0x85, 0x10, 0x11), 1),
    ("level 1, odd bin", False, _k(0xBF, 0x85, 0x47, 0x23), _k(0xBF, 0x88, 0x10, 0x11), 1),
    ("level 1, negative", False, _k(0x40, 0x39, 0x47, 0x23), _k(0x40, 0x3C, 0x10, 0x11), 1),
    ("level 2, even bin", False, _k(0xBF, 0x85, 0x46, 0x23), _k(0xBF, 0x85, 0x47, 0x11), 2),
    ("level 2, odd bin", False, _k(0xBF, 0x85, 0x47, 0x23), _k(0xBF, 0x85, 0x4A, 0x11), 2),
    ("level 3, even bin", False, _k(0xBF, 0x85, 0x47, 0x22), _k(0xBF, 0x85, 0x47, 0x23), 3),
    ("level 3, odd bin", False, _k(0xBF, 0x85, 0x47, 0x23), _k(0xBF, 0x85, 0x47, 0x26), 3),
    ("-1, 1", False, _fk(-1.0), _fk(1.0), 0),
    ("1, 2", False, _fk(1.0), _fk(2.0), 0),
    ("1, 1.5", False, _fk(1.0), _fk(1.5), 1),
    ("-1.5, -1", False, _fk(-1.5), _fk(-1.0), 1),
    ("1, 1 + 2^-15", False, _fk(1.0), _fk(1.0 + 2.0 ** -15), 2),
    ("1, the next float", False, _fk(1.0), _fk(np.nextafter(np.float32(1.0), np.float32(2.0))), 3),
    ("count, none", True, 300, 300, None),
    ("count, 255, 256", True, 255, 256, 2),
    ("count, level 2, odd bin", True, 0x01F3, 0x0412, 2),
    ("count, 300, 301", True, 300, 301, 3),
    ("count, level 3, odd bin", True, 0x2A35, 0x2A38, 3),
]
FLOAT_CLASSES = [c for c in CLASSES if not c[1]]
COUNT_CLASSES = [c for c in CLASSES if c[1]]


def _values(keys, count):
    keys = np.array(keys, dtype=np.uint32)
    return keys.astype(np.float32) if count else R.value(keys)


def decoys(ka, kb, level, count):
    """``(below, above)``: keys below ``ka`` and above ``kb`` in the order of their use -- in a's bin below a and in b's bin above b,
    a sample equal to a in the byte of the split but not in the byte before, neighbours one and two bins away at every level (both
    parities, below a and above b), then values far away; ``ka`` and ``kb`` themselves close the lists (ties)."""
    levels = (2, 3) if count else (0, 1, 2, 3)
    cand = [ka - 1, kb + 1]
    if level is not None and level - 1 in levels:
        cand.append(ka ^ (1 << (32 - 8 * level)))
    for lv in reversed(levels):
        shift = 24 - 8 * lv
        cand += [ka - (1 << shift), ka - (2 << shift), kb + (1 << shift), kb + (2 << shift)]
    cand += [0, 7, 90, 1000, 40000, 65535] if count else [_fk(v) for v in (-3.5, -1e-3, 1e-3, 0.011, 5.0, 100.5, 1e10)]
    ok = [k for k in cand if (0 <= k <= 65535 if count else 0 <= k < 2 ** 32 and np.isfinite(R.value(np.uint32(k))))]
    below = list(dict.fromkeys(k for k in ok if k < ka)) + [ka]
    above = list(dict.fromkeys(k for k in ok if k > kb)) + [kb]
    return below, above


def column(z, cls, rng):
    """A column of ``z`` samples whose middle elements are the class's ``a`` (and ``b`` for an even ``z``), in a random order."""
    _, count, ka, kb, level = cls
    below, above = decoys(ka, kb, level, count)
    if z % 2:
        above = [kb] + above[:-1]
    nb = (z - 1) // 2
    keys = [below[j % len(below)] for j in range(nb)] + [ka] + ([kb] if z % 2 == 0 else [])
    keys += [above[j % len(above)] for j in range(z - len(keys))]
    return rng.permutation(_values(keys, count))


def class_of_pixel(i, count):
    classes = COUNT_CLASSES if count else FLOAT_CLASSES
    return classes[i % len(classes)]


# ---- the volumes of the median cases ------------------------------------------------------------------------------------------

NAN_BITS = (0x7FC00000, 0xFFC00001)         # one of each sign, the second with a payload
NON_COUNTS = [("0.5", 0x3F000000), ("-1", 0xBF800000), ("65536", 0x47800000), ("65535.5", 0x477FFF80), ("-0.0", 0x80000000),
              ("+inf", 0x7F800000), ("nan", 0x7FC00000), ("denormal", 0x00012345)]
FALLBACK_Z = [GU - 3, GU]
FALLBACK_AT = ["0", "1", "2", "3", "g", "Z-1"]
FALLBACK_WHERE = {"first": [5], "ragged": [NPIX - 1], "every": [5, COLS + 2, NPIX - 1]}
RUN_KINDS = ["every sample", "per phase", "break at u - 1", "break at u", "break at u + 1"]


def _rng(*parts):
    return np.random.default_rng([zlib.crc32(str(p).encode()) for p in parts])


def _counts(z, rng):
    v = rng.integers(0, 65536, (z,) + PLANE).astype(np.float32)
    v.reshape(z, -1)[0, [0, COLS, NPIX - 2]] = 0.0                    # 0 and 65535 stay counts
    v.reshape(z, -1)[z - 1, [1, COLS + 1, NPIX - 3]] = 65535.0
    return v


def _engineered(z, count):
    rng = _rng("engineered", z, count)
    v = np.empty((z, NPIX), dtype=np.float32)
    for i in range(NPIX):
        v[:, i] = column(z, class_of_pixel(i, count), rng)
    return v.reshape((z,) + PLANE)


def _runs(z, count):
    """The first pass counts runs of equal bins in registers: the bin of pixel ``i`` follows ``RUN_KINDS[i % 5]`` along the samples
    ``j = z // g`` of a phase."""
    rng = _rng("runs", z, count)
    zz = np.arange(z)
    j, phase = zz // PHASES, zz % PHASES
    v = np.empty((z, NPIX), dtype=np.float32)
    for i in range(NPIX):
        kind = i % len(RUN_KINDS)
        if kind == 0:
            b = (j + phase) % 2
        elif kind == 1:
            b = phase
        else:
            b = (j >= LOADS + kind - 3).astype(int) + 2 * (phase % 2)
        if count:
            v[:, i] = 256 * (b + 1 + i % 2) + rng.integers(0, 256, z)
        else:
            v[:, i] = 4.0 ** (b + i % 2) * (1.0 + rng.random(z))       # top key bytes 0xBF, 0xC0, 0xC1, ...
    return v.reshape((z,) + PLANE)


def _fallback(z, value, at, where):
    v = _counts(z, _rng("fallback", z))
    zi = {"0": 0, "1": 1, "2": 2, "3": 3, "g": PHASES, "Z-1": z - 1}[at]
    v.reshape(z, -1).view(np.uint32)[zi, FALLBACK_WHERE[where]] = dict(NON_COUNTS)[value]
    return v


def _nan(z, kind):
    v = _counts(z, _rng("nan", z)) if kind == "counts" else _engineered(z, False).copy()
    bits = v.reshape(z, -1).view(np.uint32)
    bits[z // 2, 7] = NAN_BITS[0]
    bits[z - 1, COLS + 12] = NAN_BITS[1]
    bits[0, NPIX - 2] = NAN_BITS[1]                                   # in the ragged workgroup
    bits[min(PHASES, z - 1), NPIX - 1] = NAN_BITS[0]
    return v


def _other(z, kind):
    rng = _rng("other", z, kind)
    shape = (z,) + PLANE
    if kind == "inf":
        v = (100.0 * rng.standard_normal(shape)).astype(np.float32)
        u = rng.random(shape)
        v[u < 0.2] = -np.inf
        v[u > 0.8] = np.inf
        flat = v.reshape(z, -1)
        flat[:, 3] = np.inf                                            # a == b == inf: inf - inf
        flat[:, 4] = -np.inf
        flat[:, 5] = np.where(np.arange(z) % 2 == 0, -np.inf, np.inf)  # a = -inf, b = +inf for an even z
    elif kind == "negative":
        v = -np.abs(100.0 * rng.standard_normal(shape)).astype(np.float32) - np.float32(0.25)
    elif kind == "denormal":
        v = (1e-38 * rng.standard_normal(shape)).astype(np.float32)
    elif kind == "zeros":
        v = np.where(rng.random(shape) < 0.5, -0.0, 0.0).astype(np.float32)
        flat = v.reshape(z, -1)
        flat[:, 3] = -0.0
        flat[:, 4] = 0.0
    elif kind == "zeros beside counts":
        v = _counts(z, rng)
        flat = v.reshape(z, -1)
        flat[:, 3] = -0.0                                              # workgroup 0: not a count, the float keys
        flat[:, 4] = np.where(rng.random(z) < 0.5, -0.0, 0.0)
        flat[:, COLS + 3] = 0.0                                        # workgroup 1: +0.0 is a count
        flat[:, NPIX - 2] = -0.0                                       # the ragged workgroup
    else:
        raise KeyError(kind)
    return v


LIMIT_Z = REFUSED_Z - 1


def _limit(count):
    """``Z = 65535`` on a (1, 3) plane: a constant column whose first-pass bin is even, one whose bin is odd, one alternating between
    the two along the samples of every phase."""
    even, odd = (512.0, 300.0) if count else (2.5, 1.5)               # count bins 2 and 1, float bins 0xC0 and 0xBF
    zz = np.arange(LIMIT_Z)
    v = np.empty((LIMIT_Z, 1, 3), dtype=np.float32)
    v[:, 0, 0] = even
    v[:, 0, 1] = odd
    v[:, 0, 2] = np.where((zz // PHASES + zz) % 2 == 0, even, odd)
    return v


def _build_cases():
    cases = {}
    for z in Z_LIST:
        cases[f"engineered float Z={z}"] = (_engineered, (z, False))
        cases[f"engineered count Z={z}"] = (_engineered, (z, True))
    for z in Z_BATCH + Z_TWO + [300]:
        cases[f"runs float Z={z}"] = (_runs, (z, False))
        cases[f"runs count Z={z}"] = (_runs, (z, True))
    for z in FALLBACK_Z:
        cases[f"counts Z={z}"] = (lambda z: _counts(z, _rng("fallback", z)), (z,))
        for value, _ in NON_COUNTS:
            for at in FALLBACK_AT:
                for where in FALLBACK_WHERE:
                    cases[f"fallback Z={z} {value} at {at} in {where}"] = (_fallback, (z, value, at, where))
    for z in (5, GU):
        cases[f"nan in counts Z={z}"] = (_nan, (z, "counts"))
        cases[f"nan in floats Z={z}"] = (_nan, (z, "floats"))
    for kind in ("inf", "negative", "zeros", "zeros beside counts"):
        for z in (4, 5, GU, GU + 1):
            cases[f"{kind} Z={z}"] = (_other, (z, kind))
    for z in (2, 4, GU):
        cases[f"denormal Z={z}"] = (_other, (z, "denormal"))
    cases["limit float"] = (_limit, (False,))
    cases["limit count"] = (_limit, (True,))
    return cases


_CASES = _build_cases()
CASES = list(_CASES)
SMALL_CASES = [n for n in CASES if not n.startswith("limit")]
FALLBACK_CASES = [n for n in CASES if n.startswith("fallback")]
GROUPS = ["engineered", "runs", "counts", "fallback", "nan", "inf", "negative", "zeros", "denormal", "limit"]


def group(prefix):
    return [n for n in CASES if n.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def volume(name):
    """The float32 volume of a median case (read-only)."""
    fn, args = _CASES[name]
    v = np.ascontiguousarray(fn(*args), dtype=np.float32)
    v.setflags(write=False)
    return v


def is_u16_case(name):
    """The count cases whose uint16 form is a case of its own."""
    return name.startswith(("engineered count", "runs count", "counts", "limit count"))


U16_CASES = [n for n in CASES if is_u16_case(n)]


@functools.lru_cache(maxsize=None)
def volume_u16(name):
    v = volume(name)
    out = v.astype(np.uint16)
    assert np.array_equal(out.astype(np.float32), v)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's pattern of a case, computed once (read-only)."""
    p = R.pattern(volume(name))
    p.setflags(write=False)
    return p


def has_nan(name):
    return bool(np.isnan(volume(name)).any())


def has_mixed_zeros(name):
    """Whether a column holds zeros of both signs among its two middle elements' ties (torch's answer is positional there)."""
    v = volume(name)
    zero = v == 0
    neg = np.signbit(v) & zero
    return bool(((neg.any(axis=0)) & ((zero & ~neg).any(axis=0))).any())


def torch_comparable(name):
    return not has_nan(name) and not has_mixed_zeros(name)


# ---- the mean -----------------------------------------------------------------------------------------------------------------

MEAN_PLANES = [(1, 1), (3, 85), (16, 16), (1, 257), PLANE, (1, 256 * 256 + 1)]
MEAN_CONTENTS = ["counts", "cancelling"]


@functools.lru_cache(maxsize=None)
def mean_plane(plane, content):
    """A ``Z = 1`` stack, so that the pattern is the stack: counts, or ``+-1e30`` in alternation (they cancel exactly) between terms
    of 1 .. 2 -- a float32 sum, or one that is not float64 from the first add, loses the small terms' sum among the large."""
    n = plane[0] * plane[1]
    rng = _rng("mean", n, content)
    if content == "counts":
        p = rng.integers(80, 600, n).astype(np.float32)
    else:
        p = (1.0 + rng.random(n)).astype(np.float32)
        m = n // 4
        p[0:4 * m:4] = 1e30
        p[2:4 * m:4] = -1e30
    p = p.reshape((1,) + plane)
    p.setflags(write=False)
    return p


# ---- the division -------------------------------------------------------------------------------------------------------------

APPLY_SHAPES = [(5, 3, 4), (3, 3, 7), (3, 2, 5), (5, 1, 3), (9,) + PLANE, (3, 16, 24)]     # plane % 4 = 0, 1, 2, 3, 3, 0
APPLY_BIG = {"float32": (65, 512, 512), "uint16": (17, 512, 512)}                       # past each kernel's grid cap
APPLY_MEAN = np.float32(311.37)


@functools.lru_cache(maxsize=None)
def apply_case(shape, dtype):
    """``(volume, pattern)``: the pattern holds a 0, a -0.0, a denormal and a NaN pixel where the plane has room."""
    rng = _rng("apply", shape, dtype)
    if dtype == "uint16":
        vol = rng.integers(0, 65536, shape).astype(np.uint16)
    else:
        vol = (300.0 * rng.standard_normal(shape)).astype(np.float32)
    pat = (100.0 + 500.0 * rng.random(shape[1:])).astype(np.float32)
    flat = pat.reshape(-1).view(np.uint32)
    for i, bits in zip(range(1, flat.size, 2), (0x00000000, 0x80000000, 0x00012345, 0x7FC00000)):
        flat[i] = bits
    vol.setflags(write=False)
    pat.setflags(write=False)
    return vol, pat
