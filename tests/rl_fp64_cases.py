"""Seeded inputs and the per-voxel bound shared by the float64 pins of one Richardson-Lucy iteration
(``tests/test_rl_fp64_gpu.py`` for the kernels, ``tests/test_host_twins.py`` for the host twins).  Not a test module.

Inputs are float32 and non-negative, so nothing cancels in ``x * H^T(y / (H x + eps)) / H^T 1`` and every voxel is
held to a purely relative bound against ``oracle.cpu_ref.rl_iteration_f64``:

    ref == 0  ->  got == 0 exactly
    ref  > 0  ->  |got - ref| <= C * u * ref          u = 2^-24

with ``C <= 2 T + 16`` a priori, ``T`` the taps summed per correlation (one rounding per FMA in both correlations, the
``eps`` add, the refined reciprocal, three norm factors rounded to float32 and inverted, two products).
"""
import numpy as np

U = 2.0 ** -24
EPS = 1e-6


def ceiling(taps_per_correlation):
    """The a-priori bound on C for a path that sums ``taps_per_correlation`` taps per correlation."""
    return 2.0 * taps_per_correlation + 16.0


def taps_1d(n, rng, scale=1.0):
    """``n`` positive float32 taps, asymmetric, summing to ``scale`` (to float32 rounding)."""
    k = rng.uniform(0.2, 1.0, n)
    k[0] *= 1.5                                     # never palindromic, whatever the draw
    return (k * (scale / k.sum())).astype(np.float32)


def taps_nd(shape, rng, scale=1.0):
    k = rng.uniform(0.2, 1.0, shape)
    k[(0,) * len(shape)] *= 1.5
    return (k * (scale / k.sum())).astype(np.float32)


def _boxes(shape, psf_shape):
    """Two disjoint boxes ``(zero, tiny)``, each ``2 p + 1`` wide per axis where the axis has room and the whole axis
    where it has not; along the longest axis they are kept apart (a third of the axis each when it is short)."""
    split = int(np.argmax(shape))
    zero, tiny = [], []
    for axis, (n, p) in enumerate(zip(shape, psf_shape)):
        w = 2 * p + 1
        if axis == split:
            w = min(w, n // 3)
            zero.append(slice(min(1, n // 3 - w), min(1, n // 3 - w) + w) if n >= 2 * w + 3 else slice(0, w))
            tiny.append(slice(n - 1 - w, n - 1) if n >= 2 * w + 3 else slice(n - w, n))
        else:
            w = min(w, n)
            lo = min(n - w, 1)
            zero.append(slice(lo, lo + w))
            tiny.append(slice(n - w - lo, n - lo))
    return tuple(zero), tuple(tiny)


def make_inputs(shape, psf_shape, seed, tile=(32, 128)):
    """``(x, y)`` float32, no denormals: positive values of order 1 .. 100; a box of exact zeros in ``x`` wider than
    twice the PSF on every axis (clipped to the volume: there ``H x = 0``, ``ratio = y / eps`` and the result is 0); a
    box where ``x`` is of order ``eps`` (2^-24 .. 2^-17) under ordinary ``y`` (``H x + eps`` dominated by neither term);
    rows of ``y = 0``; isolated voxels of 1e4 on the corners of ``tile`` (rows, columns)."""
    rng = np.random.default_rng(seed)
    z, yy, xx = shape
    x = np.exp(rng.uniform(0.0, np.log(100.0), shape))
    y = np.exp(rng.uniform(0.0, np.log(100.0), shape))
    zero, tiny = _boxes(shape, psf_shape)               # (empty on a volume shorter than 3 along every axis)
    x[tiny] = 2.0 ** rng.uniform(-24.0, -17.0, x[tiny].shape)
    x[zero] = 0.0
    if z * yy >= 4:
        y[z // 2, yy // 3, :] = 0.0
        y[0, yy - 1, :] = 0.0
    ty, tx = tile
    for i, (zz, r, c) in enumerate([(0, ty - 1, tx - 1), (z - 1, ty, tx), (z // 2, ty - 1, tx), (z // 3, ty, tx - 1),
                                    (z - 1, 0, 0), (0, yy - 1, xx - 1), (z // 2, 2 * ty, 2 * tx - 1)]):
        if r < yy and c < xx:
            (x if i % 2 == 0 else y)[zz, r, c] = 1e4
    return x.astype(np.float32), y.astype(np.float32)


def worst_voxel(got, ref):
    """``(ratio, index, leak)``: the largest ``|got - ref| / (u ref)`` over the voxels with ``ref > 0`` and where it
    is; ``leak`` = index of a voxel that is not exactly 0 where ``ref == 0``, or ``None``.  Every ``got`` must be
    finite."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    if not np.isfinite(got).all():
        bad = np.unravel_index(int(np.argmin(np.isfinite(got))), got.shape)
        raise AssertionError(f"non-finite output at (z, y, x) = {tuple(int(v) for v in bad)}")
    assert (ref >= 0).all()
    live = ref > 0
    leak = None
    if not live.all():
        nz = (~live) & (got != 0)
        if nz.any():
            leak = tuple(int(v) for v in np.unravel_index(int(np.argmax(nz)), got.shape))
    err = np.zeros_like(ref)
    np.divide(np.abs(got - ref), U * ref, out=err, where=live)
    idx = tuple(int(v) for v in np.unravel_index(int(np.argmax(err)), err.shape))
    return float(err[idx]), idx, leak
