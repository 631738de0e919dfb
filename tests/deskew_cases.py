"""The cases of the deskew tests (``tests/test_deskew_host.py``, ``tests/test_deskew_edges_gpu.py``): a designed list, sized from the
exported launch plan (``lsr_deskew_plan``) -- no threshold is written down here, each is bisected against the plan.

* ``tile``: every tile width the launcher can choose (64 halved down to 1), at the largest ``|b|`` the plan maps to it, at the next
  double above the wider tile's threshold, and inside the range, with both signs of ``b``; ``b = 0, 2^-40, 0.3, 0.755, 1``;
  ``a`` in ``{0, -b cos 30, 0.37}``; ``Xo`` in ``{1, w - 1, w, w + 1, 2 w + 1}``; the scan a little shorter than the coordinates'
  range, so that the first and the last tiles straddle its ends;
* ``slab``: per tile width and sign one tile wholly inside a long scan, ``c`` chosen from ``slab_offsets`` to stage the most rows;
* ``position``: tiles wholly below, straddling ``z < 0``, inside, straddling ``z > Z - 1`` and wholly above the scan in one launch;
  ``z_in`` exactly 0 and ``Z - 1`` (whole ``b``, ``c``), inside (-1, 0) and (Z - 1, Z); ``Z`` of 1, 2, 3;
* ``extent``: ``Yo`` in ``{1, 63, 64, 65, 129}``, the ``(Zd, avg)`` list, every residue of ``blocks % 8``, 1 and 7 blocks;
* ``sign``: the four ``(sy, sx)``, rows and columns outside the stack in every way an averaging group and a tile can meet them;
* ``fill``: both borders times the fill values; ``entry``: the six C entries, uint16 stacks, the flat-field patterns;
* ``content``: negatives, counts, ``+-3e38``, denormals, and the non-finite stacks that only the restatement describes.

Padded rows and planes are spread over the groups.  Every array is read-only and computed once: the tests share them.
"""

import ctypes
import dataclasses
import functools
import math
import zlib

import numpy as np

from shrimpy_amd import _lib
from tests import deskew_ref as R

WIDTHS = (64, 32, 16, 8, 4, 2, 1)
COS30 = math.cos(math.pi / 6.0)
PAYLOAD = 0x7FC5A5A5                       # the NaN the output buffers are filled with before a call
FRACTIONS = (0.0, 2.0 ** -30, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -10, 1.0 - 2.0 ** -30, 1.0 - 2.0 ** -52)
ZD_AVG = [(1, 1), (5, 1), (5, 2), (6, 3), (5, 5), (5, 7), (9, 4), (3, 17), (40, 17)]
YO_LIST = [1, 63, 64, 65, 129]
FILLS = [None, 7.25, -3.0, float(np.float32(132.8)), "min"]
FAMILIES = ("plain", "flat", "border", "cval")
ENTRIES = ("lsr_deskew_f32", "lsr_deskew_u16", "lsr_deskew_flat_f32", "lsr_deskew_flat_u16", "lsr_deskew_border", "lsr_deskew_cval")


def plan(zo, yo, xo, m):
    """``lsr_deskew_plan``: (tile_x, tile_y, slab rows, rows per staging pass, tiles_x, tiles_y, blocks, launched grid)."""
    out = (ctypes.c_int64 * 8)()
    _lib.call("lsr_deskew_plan", int(zo), int(yo), int(xo), _lib.matrix12(m), out)
    return tuple(int(v) for v in out)


def tile_width(b):
    return plan(1, 1, 1, R.shear(0.0, b, 0.0, -1, 0, -1, 0))[0]


TILE_Y, SLAB_ROWS, PASS_ROWS = plan(1, 1, 1, R.shear(0.0, 0.0, 0.0, -1, 0, -1, 0))[1:4]


def next_up(v):
    return float(np.nextafter(np.float64(v), np.float64(np.inf)))


def next_down(v):
    return float(np.nextafter(np.float64(v), np.float64(-np.inf)))


@functools.lru_cache(maxsize=None)
def threshold(w):
    """The largest ``b > 0`` the plan gives the tile width ``w`` (``w >= 2``; the width 1 takes every larger finite ``b``), found by
    bisecting over the doubles between 0 and 2^20: the width never grows with ``b``."""
    assert w in WIDTHS and w > 1
    lo, hi = np.float64(0.0).view(np.int64), np.float64(2.0 ** 20).view(np.int64)
    as_b = lambda i: float(np.int64(i).view(np.float64))                      # noqa: E731
    assert tile_width(as_b(lo)) >= w > tile_width(as_b(hi))
    while hi - lo > 1:
        mid = (int(lo) + int(hi)) // 2
        if tile_width(as_b(mid)) >= w:
            lo = mid
        else:
            hi = mid
    return as_b(lo)


def inside_b(w):
    """A ``b`` well inside the range of the width ``w``."""
    if w == 64:
        return 0.6
    if w == 1:
        return 300.0
    return math.sqrt(threshold(w) * threshold(2 * w))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str
    Z: int
    Y: int
    X: int
    Zd: int
    Yo: int
    Xo: int
    avg: int
    a: float
    b: float
    c: float
    sy: int
    oy: int
    sx: int
    ox: int
    mode: str = "constant"
    cval: object = None                     # None (absent), a number, or "min"
    family: str = "plain"                   # which C entry: plain / flat (lsr_deskew_f32|u16, _flat_f32|u16), border, cval
    flat: object = None                     # None, "generic", "zero", "nan"
    content: str = "uniform"
    pitch_pad: int = 0
    spare_rows: int = 0
    swizzle_off: bool = False               # repeated with LSR_DESKEW_SWIZZLE=0

    @property
    def matrix(self):
        return R.shear(self.a, self.b, self.c, self.sy, self.oy, self.sx, self.ox)

    @property
    def pre_shape(self):
        return (self.Zd, self.Yo, self.Xo)

    @property
    def Zo(self):
        return -(-self.Zd // self.avg)

    @property
    def pitch(self):
        return self.Xo + self.pitch_pad

    @property
    def plane(self):
        return (self.Yo + self.spare_rows) * self.pitch

    @property
    def has_u16(self):
        return self.content.startswith("counts")

    @property
    def plan(self):
        return plan(self.Zo, self.Yo, self.Xo, self.matrix)


def _rng(*parts):
    return np.random.default_rng([zlib.crc32(str(p).encode()) for p in parts])


_CASES = {}


def _add(group, name, Z, Y, X, Xo, a, b, c, Zd=None, Yo=None, avg=1, sy=-1, oy=None, sx=-1, ox=None, **kw):
    """The defaults are the product's geometry: planes walk the tilt rows backwards, Y' walks the raw X backwards."""
    Zd = Y if Zd is None else Zd
    Yo = X if Yo is None else Yo
    oy = (Y - 1 if sy < 0 else 0) if oy is None else oy
    ox = (X - 1 if sx < 0 else 0) if ox is None else ox
    name = f"{group}: {name}"
    assert name not in _CASES, name
    assert kw.get("family", "plain") in FAMILIES
    assert Z * Y * X <= 200_000 and Zd * Yo * Xo <= 400_000, name
    _CASES[name] = Case(name, group, int(Z), int(Y), int(X), int(Zd), int(Yo), int(Xo), int(avg), float(a), float(b), float(c),
                        int(sy), int(oy), int(sx), int(ox), **kw)


def _fit(a, b, zd_n, xo_n, lo=1.5, hi=1.5):
    """``(Z, c)`` such that the lowest coordinate is ``-lo`` and the highest ``Z - 1 + hi`` or a little more."""
    zs = [a * zd + b * xo for zd in (0, zd_n - 1) for xo in (0, xo_n - 1)]
    zmin, zmax = min(zs), max(zs)
    return max(int(math.ceil(zmax - zmin - lo - hi)) + 1, 1), -zmin - lo


def _xo_list(w):
    return sorted({1, w, w + 1, 2 * w + 1} | ({w - 1} if w > 1 else set()))


def _family_of(mode, i):
    return "border" if mode == "grid-constant" else ("plain", "cval", "border")[i % 3]


def _build_tile():
    for w in WIDTHS:
        values = []
        if w > 1:
            values.append(("largest b", threshold(w)))
        if w < 64:
            values.append(("next above the wider tile", next_up(threshold(2 * w))))
        values.append(("inside", inside_b(w)))
        if w == 64:
            values += [("b = 0", 0.0), ("b = 2^-40", 2.0 ** -40), ("b = 0.3", 0.3), ("b = 0.755", 0.755), ("b = 1", 1.0)]
        if w == 1:
            values.append(("b = 1000.25", 1000.25))
        xos = _xo_list(w)
        i = 0
        for label, v in values:
            for sign in ((1.0,) if v == 0.0 else (1.0, -1.0)):
                b = sign * v
                a = (0.0, -b * COS30, 0.37)[i % 3]
                xo = xos[i % len(xos)]
                mode = R.MODES[(i // 2) % 2]
                z, c = _fit(a, b, 3, xo)
                _add("tile", f"w={w} {label} {'+' if sign > 0 else '-'}", max(z, 3), 3, 5, xo, a, b, c, mode=mode,
                     family=_family_of(mode, i), pitch_pad=i % 4, spare_rows=(i // 4) % 3,
                     content="counts" if i % 3 == 1 else "uniform")
                i += 1


SLAB_BASES = (2.0, 1000.0)


def slab_offsets(w, b):
    """The ``c`` of the slab cases' search: a tile of ``w`` columns from 0 starts (``b > 0``) or ends (``b < 0``) at a base plus a
    fraction of ``FRACTIONS`` -- near 2, and near 1000 where the coordinates round more coarsely."""
    return [base + (0.0 if b > 0 else math.floor(abs(b) * (w - 1))) + f for base in SLAB_BASES for f in FRACTIONS]


def _build_slab():
    for w in WIDTHS:
        v = threshold(w) if w > 1 else 300.0
        for sign in (1.0, -1.0):
            b = sign * v
            cs = slab_offsets(w, b)
            rows = [R.tile_rows(R.shear(0.0, b, c, -1, 0, -1, 0), 2 ** 40, 0, 0, w)[0] for c in cs]
            c = cs[int(np.argmax(rows))]
            z = int(c + v * (w - 1)) + 8
            _add("slab", f"w={w} {'+' if sign > 0 else '-'}", z, 1, 3, w, 0.0, b, c, mode=R.MODES[w.bit_length() % 2],
                 family="border", swizzle_off=w in (64, 8, 1))


def _build_position():
    for sign in (1, -1):
        for mode in R.MODES:
            s = "+" if sign > 0 else "-"
            # tiles of 64 columns at z in [-60, -12.4], [-11.7, 35.9], [36.6, 84.2], [85, 132.5], [133, 180], 181.6 against Z = 110
            _add("position", f"five tiles {s} {mode}", 110, 2, 3, 321, 0.37, sign * 0.755, -60.0 if sign > 0 else 169.0,
                 mode=mode, family="border", swizzle_off=True, pitch_pad=3)
            for z in (1, 2, 3, 10):
                # whole coordinates -3 .. 11: 0 and Z - 1 themselves, -1 and Z
                _add("position", f"whole z_in {s} {mode} Z={z}", z, 2, 3, 14, -1.0, sign * 1.0, -2.0 if sign > 0 else 11.0,
                     mode=mode, family="cval" if z == 2 else "border", cval=7.25 if z == 2 else None)
            for z in (1, 2, 3, 5):
                # -1.25, -0.75, -0.25, 0.25, ...: inside (-1, 0) and (Z - 1, Z)
                _add("position", f"quarter z_in {s} {mode} Z={z}", z, 2, 3, 16, 0.0, sign * 0.5, -1.25 if sign > 0 else 6.25,
                     mode=mode, family="cval", cval=-3.0)


def _build_extent():
    tiles_x = [1, 1, 2, 2, 1, 7, 3, 2, 2]         # blocks = tiles_x * tiles_y * Zo: 1, 5, 6, 8, 3, 7, 9, 2, 12
    for i, ((zd, avg), tx) in enumerate(zip(ZD_AVG, tiles_x)):
        yo = YO_LIST[i % len(YO_LIST)]
        xo = 40 + i if tx == 1 else 64 * tx - (9 if i % 2 else 0)
        b = 0.4 if i % 2 == 0 else -0.4
        a = -b * COS30
        z, c = _fit(a, b, zd, xo)
        mode = R.MODES[i % 2]
        _add("extent", f"Zd={zd} avg={avg} Yo={yo} Xo={xo}", z, zd, yo, xo, a, b, c, avg=avg, mode=mode, family=("border", "cval")[i % 2],
             cval=(None, 7.25, "min")[i % 3] if i % 2 else None, swizzle_off=True, pitch_pad=(i + 1) % 4, spare_rows=i % 3)


ROW_KINDS = ["no row", "a whole group", "the first of a group", "the last of a group", "every row"]
COL_KINDS = ["no column", "the first of a tile", "the last of a tile", "a whole tile", "every column"]
SIGN_SHAPE = dict(Z=20, Y=6, X=140, Zd=6, Yo=130, Xo=40, avg=3)


def _build_sign():
    oy = {1: [0, -3, -1, 1, 100], -1: [5, 2, 6, 4, -1]}
    ox = {1: [0, -5, 15, -64, 1000], -1: [139, 144, 124, 203, -1]}
    for s, (sy, sx) in enumerate([(-1, -1), (-1, 1), (1, -1), (1, 1)]):
        for i in range(5):
            j = (i + s) % 5
            _add("sign", f"sy={sy:+d} sx={sx:+d} {ROW_KINDS[i]} and {COL_KINDS[j]} outside", a=0.1, b=0.3 if sy > 0 else -0.3,
                 c=-1.0 if sy > 0 else 12.5, sy=sy, oy=oy[sy][i], sx=sx, ox=ox[sx][j], mode=R.MODES[(i + s) % 2],
                 family="cval", cval=(7.25, None)[i % 2], spare_rows=i % 2, **SIGN_SHAPE)


def _build_fill():
    for mode in R.MODES:
        for k, cval in enumerate(FILLS):
            # two columns (yo = 9, 10) and the last row of the second group are outside, the scan ends before the coordinates do
            _add("fill", f"{mode} cval={cval!r}", 12, 4, 9, 30, -0.65, 0.755, -3.0, Yo=11, avg=2, oy=2, mode=mode, cval=cval,
                 family="cval" if cval is not None or k % 2 else "border", content="counts100", pitch_pad=1 + k % 3)


def _build_entry():
    shape = dict(Z=40, Y=5, X=37, Xo=45, a=0.2, b=-0.755, c=36.0, avg=2, sy=1, sx=1)
    _add("entry", "lsr_deskew_f32 / _u16", family="plain", content="counts", **shape)
    for pattern in ("generic", "zero", "nan"):
        _add("entry", f"lsr_deskew_flat_f32 / _u16, {pattern} pattern", family="flat", flat=pattern, content="counts", pitch_pad=2, **shape)
    for mode in R.MODES:
        _add("entry", f"lsr_deskew_border {mode}", family="border", mode=mode, content="counts", **shape)
        _add("entry", f"lsr_deskew_border {mode}, generic pattern", family="border", mode=mode, flat="generic", content="counts", **shape)
        _add("entry", f"lsr_deskew_cval {mode}, generic pattern", family="cval", mode=mode, flat="generic", cval=7.25,
             content="counts", spare_rows=2, **shape)
        _add("entry", f"lsr_deskew_cval {mode}, zero pattern", family="cval", mode=mode, flat="zero", cval="min", content="counts", **shape)


def _build_content():
    for content in ("uniform", "counts", "huge", "denormal", "nonfinite interior"):
        for mode in R.MODES:
            _add("content", f"{content} {mode}", 30, 7, 9, 50, -0.65, 0.755, -2.5, avg=3, mode=mode, family="border", content=content)
    for content in ("nonfinite interior", "nonfinite top"):
        for mode in R.MODES:
            _add("content", f"{content}, whole z_in {mode}", 10, 2, 3, 14, -1.0, 1.0, -2.0, mode=mode, family="border", content=content)


for _build in (_build_tile, _build_slab, _build_position, _build_extent, _build_sign, _build_fill, _build_entry, _build_content):
    _build()
CASES = list(_CASES)
GROUPS = ["tile", "slab", "position", "extent", "sign", "fill", "entry", "content"]
SWIZZLE_CASES = [n for n in CASES if _CASES[n].swizzle_off]


def case(name):
    return _CASES[name]


def group(g):
    return [n for n in CASES if _CASES[n].group == g]


# ---- contents -------------------------------------------------------------------------------------------------------------------

NONFINITE = (np.nan, np.inf, -np.inf)


def nonfinite_at(c):
    """The three voxels of a non-finite stack that hold NaN, +inf, -inf."""
    z = c.Z - 1 if c.content == "nonfinite top" else c.Z // 2
    return [(z, 0, 0), (z, c.Y - 1, c.X // 2), (max(z - (c.Z > 3), 0), c.Y // 2, c.X - 1)]


@functools.lru_cache(maxsize=None)
def raw(name):
    """The float32 stack of a case (read-only)."""
    c = _CASES[name]
    rng = _rng("raw", name)
    shape = (c.Z, c.Y, c.X)
    if c.content == "uniform" or c.content.startswith("nonfinite"):
        v = rng.uniform(-50.0, 150.0, shape).astype(np.float32)
        if c.content.startswith("nonfinite"):
            for at, value in zip(nonfinite_at(c), NONFINITE):
                v[at] = value
    elif c.content == "counts":
        v = rng.integers(0, 65536, shape).astype(np.float32)
        v.reshape(-1)[0] = 0.0
        v.reshape(-1)[-1] = 65535.0
        v[c.Z // 2, c.Y // 2, c.X // 2] = 65535.0
        v[c.Z // 2, c.Y // 2, c.X // 2 - 1] = 0.0
    elif c.content == "counts100":
        v = rng.integers(104, 600, shape).astype(np.float32)
    elif c.content == "huge":
        v = np.where(rng.random(shape) < 0.5, np.float32(-3e38), np.float32(3e38)).astype(np.float32)
        v[rng.random(shape) < 0.3] = np.float32(1.5)
    elif c.content == "denormal":
        v = (1e-40 * rng.standard_normal(shape)).astype(np.float32)
    else:
        raise KeyError(c.content)
    v = np.ascontiguousarray(v, dtype=np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def raw_u16(name):
    v = raw(name)
    out = v.astype(np.uint16)
    assert np.array_equal(out.astype(np.float32), v)
    out.setflags(write=False)
    return out


FLAT_MEAN = np.float32(311.37)


@functools.lru_cache(maxsize=None)
def flat(name):
    """``(pattern, mean)`` of a case with a flat-field, else ``None``."""
    c = _CASES[name]
    if c.flat is None:
        return None
    pat = (100.0 + 500.0 * _rng("flat", name).random((c.Y, c.X))).astype(np.float32)
    if c.flat == "zero":
        pat[c.Y // 2, c.X // 3] = 0.0
    elif c.flat == "nan":
        pat[c.Y // 2, c.X // 3] = np.nan
    pat.setflags(write=False)
    return pat, FLAT_MEAN


def fill(name):
    """The fill value as a float32, ``None`` when the case names none; ``"min"`` is the minimum of the uncorrected stack."""
    c = _CASES[name]
    if c.cval is None:
        return None
    return np.float32(raw(name).min()) if c.cval == "min" else np.float32(c.cval)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's result of a case, computed once (read-only)."""
    c = _CASES[name]
    cv = fill(name)
    out = R.deskew(raw(name), c.matrix, c.pre_shape, c.avg, c.mode, 0.0 if cv is None else cv, flat(name))
    out.setflags(write=False)
    return out


def is_finite(name):
    """Whether every sample the interpolation reads is finite (the cases scipy can be asked about)."""
    return bool(np.isfinite(R.corrected(raw(name), flat(name))).all())


# ---- calling an entry -------------------------------------------------------------------------------------------------------------


def entry_name(c, u16, cpu=False):
    if cpu:
        return ("lsr_deskew_u16_cpu" if u16 else "lsr_deskew_f32_cpu") if c.family == "plain" else "lsr_deskew_cval_cpu"
    return {"plain": "lsr_deskew_u16" if u16 else "lsr_deskew_f32", "flat": "lsr_deskew_flat_u16" if u16 else "lsr_deskew_flat_f32",
            "border": "lsr_deskew_border", "cval": "lsr_deskew_cval"}[c.family]


def entry_args(c, u16, in_ptr, out_ptr, pattern_ptr, mean_ptr, cval_ptr, stream, cpu=False):
    """``(entry, args)`` of the case's C entry (the device's, or with ``cpu`` the twin's) on these buffers."""
    assert (c.family in ("plain", "flat")) <= (c.mode == "constant" and c.cval is None), c.name
    assert (c.family == "plain") <= (c.flat is None) and (c.family == "flat") <= (c.flat is not None), c.name
    assert c.family == "cval" or c.cval is None, c.name
    head = [c.Z, c.Y, c.X, out_ptr, c.Zo, c.Yo, c.Xo, c.pitch, c.plane, c.Zd, _lib.matrix12(c.matrix), c.avg]
    mode = _lib.MODE_CONSTANT if c.mode == "constant" else _lib.MODE_GRID_CONSTANT
    name = entry_name(c, u16, cpu)
    if name.startswith(("lsr_deskew_f32", "lsr_deskew_u16")):
        return name, [in_ptr] + head + [stream]
    if name.startswith("lsr_deskew_flat"):
        return name, [in_ptr] + head + [pattern_ptr, mean_ptr, stream]
    if name == "lsr_deskew_border":
        return name, [in_ptr, int(u16)] + head + [mode, pattern_ptr, mean_ptr, stream]
    return name, [in_ptr, int(u16)] + head + [mode, pattern_ptr, mean_ptr, cval_ptr, stream]


def output_buffer(c):
    """A host buffer of ``Zo`` padded planes, every word the recognisable NaN."""
    return np.full(c.Zo * c.plane, PAYLOAD, dtype=np.uint32)


def window(c, buf):
    """The (Zo, Yo, Xo) result inside a buffer of ``output_buffer``'s layout, as float32."""
    return buf.view(np.float32).reshape(c.Zo, c.Yo + c.spare_rows, c.pitch)[:, :c.Yo, :c.Xo]


def padding_intact(c, buf):
    """No word outside the window was written, and none inside it was left."""
    words = buf.view(np.uint32).reshape(c.Zo, c.Yo + c.spare_rows, c.pitch)
    inside = np.zeros(words.shape, dtype=bool)
    inside[:, :c.Yo, :c.Xo] = True
    return bool((words[~inside] == PAYLOAD).all()), bool((words[inside] != PAYLOAD).all())


# ---- lsr_average_slices_f32 and the general-matrix fallback -------------------------------------------------------------------------

AVERAGE_CASES = [(zd, avg, (5, 70)) for zd, avg in ZD_AVG] + [(24, 8, (1, 1)), (3, 2, (1025, 1024))]
GENERAL_MATRIX = [[0.755, 0.02, -0.65, 1.5], [0.03, -1.0, 0.01, 8.25], [0.0, 0.015, -1.0, 10.5]]   # not a shear: y_in, x_in fractional
GENERAL_RAW, GENERAL_PRE, GENERAL_AVG = (14, 10, 12), (9, 11, 13), 2


@functools.lru_cache(maxsize=None)
def average_input(zd, avg, plane):
    v = _rng("average", zd, avg, plane).uniform(-50.0, 150.0, (zd,) + plane).astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def general_raw():
    v = _rng("general").uniform(-50.0, 150.0, GENERAL_RAW).astype(np.float32)
    v.setflags(write=False)
    return v
