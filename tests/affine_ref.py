"""The order-1 affine resample (``csrc/resample.hpp``: the rule of ``csrc/affine.hip``, ``affine_planar.hip``, ``affine_box.hip`` and
of ``lsr_affine_f32_cpu``), restated in float64 numpy in scipy's operation order; nothing here calls the library.  This text is the
specification the three kernels and the twin are held to, bit for bit.

For the output voxel ``(zo, yo, xo)`` and the row ``(m0, m1, m2, shift)`` of an input axis of extent ``n``:

* the coordinate is ``c = ((zo * m0 + yo * m1) + xo * m2) + shift``, every product and sum a float64 operation of its own;
* ``"constant"``: the sample is ``cval`` when ``c < 0`` or ``c > n - 1`` on any axis; otherwise the lower index is ``floor(c)`` and the
  upper one ``min(floor(c) + 1, n - 1)``;
* ``"grid-constant"``: the lower index is ``floor(c)`` clamped to ``[-2, n + 1]``, the upper one is one more, and a tap whose index on
  any axis is outside ``[0, n - 1]`` carries ``cval``;
* the weights are ``w0 = 1 - f``, ``w1 = 1 - w0`` with ``f = c - floor(c)``;
* the eight corners are summed z-major, ``t = t + ((v * wz) * wy) * wx`` from ``t = 0``, and ``t`` is rounded to float32 once.

On finite volumes this is ``scipy.ndimage.affine_transform(order=1, prefilter=False)`` bit for bit under both modes
(``tests/test_affine_host.py`` holds it to scipy on every finite case).  On a volume with a NaN or an infinity the rule above is the
specification: a tap of weight exactly 0 is still multiplied (``inf * 0`` is a NaN), and the upper tap of a coordinate exactly on
``n - 1`` is voxel ``n - 1`` itself.
"""

import dataclasses

import numpy as np

from tests.deskew_ref import bits, describe_difference, same_bits  # noqa: F401  (the comparison helpers, shared)

MODES = ("constant", "grid-constant")


def coords(m, out_shape):
    """The three float64 coordinate arrays (broadcastable to ``out_shape``) of a row-major 3x4 matrix."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    zo = np.arange(out_shape[0], dtype=np.float64).reshape(-1, 1, 1)
    yo = np.arange(out_shape[1], dtype=np.float64).reshape(1, -1, 1)
    xo = np.arange(out_shape[2], dtype=np.float64).reshape(1, 1, -1)
    return [np.broadcast_to(((zo * r[0] + yo * r[1]) + xo * r[2]) + r[3], out_shape) for r in m]


@dataclasses.dataclass(frozen=True)
class Result:
    out: np.ndarray          # (Zo, Yo, Xo) float32: the result
    exact: np.ndarray        # float64: the corner sum before its one rounding (cval where the sample is cval)
    inside: np.ndarray       # bool: the voxel is a sample, not cval ("grid-constant": every voxel)
    taps: np.ndarray         # (8, Zo, Yo, Xo) float32: the corner values z-major, cval where a tap is outside the volume
    on_last: np.ndarray      # bool: a sample some coordinate of which is exactly n - 1 on its axis


def resample(vol, m, out_shape, mode="constant", cval=0.0):
    assert mode in MODES
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    out_shape = tuple(int(v) for v in out_shape)
    cv = np.float32(cval)
    grid = mode == "grid-constant"
    inside = np.ones(out_shape, dtype=bool)
    on_last = np.zeros(out_shape, dtype=bool)
    idx, wts, outs = [], [], []
    for c, n in zip(coords(m, out_shape), vol.shape):
        fl = np.floor(c)
        w0 = 1.0 - (c - fl)
        w1 = 1.0 - w0
        if grid:
            start = np.clip(fl, -2.0, float(n) + 1.0).astype(np.int64)
            i0, i1 = start, start + 1
            outs.append(((i0 < 0) | (i0 >= n), (i1 < 0) | (i1 >= n)))
            i0, i1 = np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1)
        else:
            ok = (c >= 0.0) & (c <= float(n - 1))
            inside &= ok
            i0 = np.where(ok, fl, 0.0).astype(np.int64)
            i1 = np.minimum(i0 + 1, n - 1)
            outs.append((np.zeros(out_shape, dtype=bool),) * 2)
        on_last |= c == float(n - 1)
        idx.append((i0, i1))
        wts.append((w0, w1))
    taps = np.empty((8,) + out_shape, dtype=np.float32)
    t = np.zeros(out_shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    v = vol[idx[0][a], idx[1][b], idx[2][c]]
                    v = np.where(outs[0][a] | outs[1][b] | outs[2][c], cv, v)
                    taps[4 * a + 2 * b + c] = v
                    t = t + ((v.astype(np.float64) * wts[0][a]) * wts[1][b]) * wts[2][c]
        exact = np.where(inside, t, np.float64(cv))
        out = np.where(inside, t.astype(np.float32), cv).astype(np.float32)
    return Result(out, exact, inside, taps, on_last & inside)
