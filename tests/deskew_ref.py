"""The fused deskew (``csrc/deskew.hip``, ``deskew_cpu`` of ``csrc/host_twins.hip``), restated in float64 numpy; nothing here calls
the library.  This text is the specification the kernel and the twin are held to, bit for bit.

The matrix is a shear: row 0 = ``(a, M[1] = 0, b, c)``, row 1 = ``(sy, 0, 0, oy)``, row 2 = ``(0, sx, 0, ox)`` with ``sy, sx = +-1`` and
whole ``oy, ox``.  For the pre-average voxel ``(zd, yo, xo)``:

* ``z_in = ((zd * a + 0 * M[1]) + xo * b) + c``, every product and sum a float64 operation of its own; ``y_in = sy * zd + oy`` and
  ``x_in = sx * yo + ox`` are integers;
* the sample is ``cval`` when ``y_in`` or ``x_in`` is outside the stack, or ``z_in < 0 or z_in > Z - 1`` (``"constant"``), or
  ``z_in <= -1 or z_in >= Z`` (``"grid-constant"``);
* otherwise ``f = z_in - floor(z_in)``, ``w0 = 1 - f``, ``w1 = 1 - w0``, the upper neighbour's index clamped to ``Z - 1``, under
  ``"grid-constant"`` a neighbour outside the scan holding ``cval``, and the value ``float32((0.0 + float64(v0) * w0) + float64(v1) * w1)``;
* an output plane is the float32 sum of its ``avg`` pre-average planes in plane order, starting from the first plane itself, plane
  indices clamped to ``Zd - 1``, divided once in float32 -- no division when ``avg == 1``;
* ``cval`` is a float32; uint16 counts convert exactly; with a flat-field every raw sample is first ``tests/flatfield_ref.apply``'s.

The rule is ``scipy.ndimage.affine_transform(order=1)`` (``oracle.cpu_ref.affine_apply``) followed by ``oracle.cpu_ref.average_slices``
bit for bit, the sign of a zero included, with two exceptions where the oracle is not the rule:

* ``average_slices`` is ``numpy.mean``, which sums pairwise instead of in plane order when the plane is a single voxel and
  ``avg >= 8`` (2 of 3 groups differ at ``avg = 8`` on a (1, 1) plane; none for ``avg`` up to 130 on planes of two voxels and more):
  ``oracle_comparable_plane`` says where the two may be compared;
* on non-finite content scipy also multiplies the six zero-weight y / x corners, and at ``z_in == Z - 1`` it mirrors the upper
  neighbour where this rule clamps it: a stack holding a NaN or an infinity is held to this restatement alone.

``same_bits`` compares by bits, a NaN by position.
"""

import numpy as np

from tests import flatfield_ref

MODES = ("constant", "grid-constant")


def shear(a, b, c, sy, oy, sx, ox):
    """The 12 matrix entries of a deskew shear."""
    return [float(a), 0.0, float(b), float(c), float(sy), 0.0, 0.0, float(oy), 0.0, float(sx), 0.0, float(ox)]


def z_coords(m, zd, xo):
    """``z_in`` of the pre-average planes ``zd`` and the columns ``xo`` (arrays), as a (len(zd), len(xo)) float64 array."""
    zd = np.asarray(zd, dtype=np.float64).reshape(-1, 1)
    xo = np.asarray(xo, dtype=np.float64).reshape(1, -1)
    with np.errstate(all="ignore"):
        return ((zd * np.float64(m[0]) + np.float64(0.0) * np.float64(m[1])) + xo * np.float64(m[2])) + np.float64(m[3])


def y_rows(m, zd_count, y_extent):
    """``y_in`` of every pre-average plane and whether it is a row of the stack."""
    y_in = int(m[4]) * np.arange(zd_count, dtype=np.int64) + int(m[7])
    return y_in, (y_in >= 0) & (y_in < y_extent)


def x_cols(m, yo_count, x_extent):
    x_in = int(m[9]) * np.arange(yo_count, dtype=np.int64) + int(m[11])
    return x_in, (x_in >= 0) & (x_in < x_extent)


def z_inside(z_in, z_extent, mode):
    """Whether the scan coordinate yields a sample rather than ``cval``."""
    if mode == "constant":
        return (z_in >= 0.0) & (z_in <= float(z_extent - 1))
    return (z_in > -1.0) & (z_in < float(z_extent))


def corrected(raw, flat=None):
    """The stack as the float32 samples the interpolation reads: uint16 exactly, the flat-field applied first."""
    raw = np.ascontiguousarray(raw)
    assert raw.dtype in (np.float32, np.uint16) and raw.ndim == 3
    if flat is not None:
        return flatfield_ref.apply(raw, flat[0], flat[1])
    return raw.astype(np.float32)


def pre_average(raw, m, pre_shape, mode="constant", cval=0.0, flat=None):
    """The (Zd, Yo, Xo) float32 volume before the averaging."""
    assert mode in MODES
    vol = corrected(raw, flat)
    z_ext, y_ext, x_ext = vol.shape
    zd_n, yo_n, xo_n = (int(v) for v in pre_shape)
    cv = np.float32(cval)
    z_in = z_coords(m, np.arange(zd_n), np.arange(xo_n))                       # (Zd, Xo)
    y_in, y_ok = y_rows(m, zd_n, y_ext)
    x_in, x_ok = x_cols(m, yo_n, x_ext)
    ok = z_inside(z_in, z_ext, mode)
    zi = np.where(ok, z_in, 0.0)
    fl = np.floor(zi)
    w0 = 1.0 - (zi - fl)
    w1 = 1.0 - w0
    i0 = fl.astype(np.int64)                                                   # -1 .. Z - 1
    i1 = i0 + 1
    yy = np.where(y_ok, y_in, 0)[:, None, None]
    xx = np.where(x_ok, x_in, 0)[None, :, None]
    v0 = vol[np.clip(i0, 0, z_ext - 1)[:, None, :], yy, xx].astype(np.float64)
    v1 = vol[np.minimum(i1, z_ext - 1)[:, None, :], yy, xx].astype(np.float64)
    if mode == "grid-constant":
        v0 = np.where((i0 < 0)[:, None, :], np.float64(cv), v0)
        v1 = np.where((i1 > z_ext - 1)[:, None, :], np.float64(cv), v1)
    with np.errstate(all="ignore"):
        t = (0.0 + v0 * w0[:, None, :]) + v1 * w1[:, None, :]
        val = t.astype(np.float32)
    inside = ok[:, None, :] & y_ok[:, None, None] & x_ok[None, :, None]
    return np.where(inside, val, cv).astype(np.float32)


def average(pre, avg):
    """Groups of ``avg`` planes, the last group edge-padded: a float32 sum in plane order, one float32 division."""
    pre = np.ascontiguousarray(pre, dtype=np.float32)
    avg = int(avg)
    zd_n = pre.shape[0]
    zo_n = -(-zd_n // avg)
    out = np.empty((zo_n,) + pre.shape[1:], dtype=np.float32)
    with np.errstate(all="ignore"):
        for zo in range(zo_n):
            acc = pre[min(zo * avg, zd_n - 1)].copy()
            for k in range(1, avg):
                acc = (acc + pre[min(zo * avg + k, zd_n - 1)]).astype(np.float32)
            out[zo] = (acc / np.float32(avg)).astype(np.float32) if avg > 1 else acc
    return out


def deskew(raw, m, pre_shape, avg=1, mode="constant", cval=0.0, flat=None):
    """The (ceil(Zd / avg), Yo, Xo) float32 result of the fused kernel."""
    return average(pre_average(raw, m, pre_shape, mode, cval, flat), avg)


def oracle_comparable_plane(yo_n, xo_n, avg):
    """Where ``numpy.mean`` adds in plane order, as the rule does."""
    return yo_n * xo_n >= 2 or avg < 8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """Bit for bit; a NaN compares by position."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def describe_difference(got, want):
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return f"shape {got.shape} instead of {want.shape}"
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (bits(got) != bits(want)))
    at = np.argwhere(bad)
    first = tuple(int(i) for i in at[0]) if len(at) else None
    return (f"{int(bad.sum())} of {want.size} voxels differ, the first at {first}: "
            f"{got[first]!r} instead of {want[first]!r}" if first is not None else "no difference")


# ---- what a workgroup stages: the kernel's own formula, for the census ---------------------------------------------------------


def tile_rows(m, z_extent, zd, xo0, n_xo):
    """``(rows, z_lo_d, z_hi_d)`` of the tile of ``n_xo`` columns from ``xo0`` in the pre-average plane ``zd``: the slab rows the
    kernel stages -- ``floor(max z) + 1 - floor(min z) + 1`` over the tile's two end columns, clamped to the scan, 0 when the range
    misses the scan -- and the unclamped range."""
    z = z_coords(m, [zd], [xo0, xo0 + n_xo - 1])[0]
    lo_d = float(np.floor(min(z[0], z[1])))
    hi_d = float(np.floor(max(z[0], z[1]))) + 1.0
    zmax = float(z_extent - 1)
    if not (hi_d >= 0.0 and lo_d <= zmax):
        return 0, lo_d, hi_d
    lo = int(min(max(lo_d, 0.0), zmax))
    hi = int(min(max(hi_d, 0.0), zmax))
    return hi - lo + 1, lo_d, hi_d
