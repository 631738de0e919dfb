"""The Hessian-eigenvalue rule of ``csrc/hessian.hpp`` restated in numpy float64: ``np.gradient`` twice (what
``skimage.feature.hessian_matrix(use_gaussian_derivatives=False)`` does), ``np.linalg.eigvalsh`` (``hessian_matrix_eigvals``),
then the float32 response functions.  Nothing here calls the package."""

from __future__ import annotations

import numpy as np

MEASURES = ("e1", "e2", "e3", "ridge", "tube", "sheet", "blob", "log")
CANONICAL_NAN = np.uint32(0x7FC00000)
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # the order of the kernel's six entries


def gradient(f: np.ndarray, axis: int, s: float) -> np.ndarray:
    """``np.gradient(f, s, axis=axis)``; along an axis of length 1, where numpy raises, the derivative is 0."""
    if f.shape[axis] == 1:
        return np.zeros_like(f)
    return np.gradient(f, float(s), axis=axis)


def hessian(g: np.ndarray, sampling) -> np.ndarray:
    """``(Z, Y, X, 3, 3)`` float64: ``H_ab = D_b (D_a g)`` for ``a <= b``, symmetric."""
    g64 = np.asarray(g, dtype=np.float32).astype(np.float64)
    first = [gradient(g64, a, sampling[a]) for a in range(3)]
    H = np.empty(g64.shape + (3, 3), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for a, b in PAIRS:
            H[..., a, b] = H[..., b, a] = gradient(first[a], b, sampling[b])
    return H


def _reads(bad: np.ndarray, axis: int) -> np.ndarray:
    """Where the derivative along ``axis`` reads a voxel of ``bad``: ``i - 1`` and ``i + 1`` inside, ``0`` and ``1`` at
    ``i = 0``, ``n - 2`` and ``n - 1`` at ``i = n - 1``, nothing on an axis of length 1."""
    n = bad.shape[axis]
    out = np.zeros_like(bad)
    if n == 1:
        return out
    b = np.moveaxis(bad, axis, 0)
    o = np.moveaxis(out, axis, 0)
    o[1:-1] = b[2:] | b[:-2]
    o[0] = b[0] | b[1]
    o[-1] = b[-1] | b[-2]
    return out


def stencil_mask(g: np.ndarray) -> np.ndarray:
    """True where the stencil of a voxel -- the voxels its six entries read -- holds a non-finite value."""
    bad = ~np.isfinite(np.asarray(g))
    mask = np.zeros_like(bad)
    for a, b in PAIRS:
        mask |= _reads(_reads(bad, a), b)
    return mask


def eigenvalues(g: np.ndarray, sampling, dark: bool = False):
    """``(l, norm, mask)``: the ascending float64 eigenvalues ``(Z, Y, X, 3)`` of ``H`` (of ``-H`` under ``dark``) with zeros
    where ``mask`` -- the stencil holds a non-finite value -- is set, and ``||H||_F``."""
    H = hessian(g, sampling)
    mask = stencil_mask(g)
    assert np.array_equal(mask, ~np.isfinite(H).all(axis=(-1, -2))), "the stencil is where H is not finite"
    H[mask] = 0.0
    if dark:
        H = -H
    return np.linalg.eigvalsh(H), np.sqrt((H * H).sum(axis=(-1, -2))), mask


def response(e1: np.ndarray, e2: np.ndarray, e3: np.ndarray, measure: int) -> np.ndarray:
    """The float32 response of the three float32 eigenvalue outputs (NaNs pass through as the canonical one)."""
    e1, e2, e3 = (np.asarray(e, dtype=np.float32) for e in (e1, e2, e3))
    zero = np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        m1, m2, m3 = (np.where(-e > zero, -e, zero).astype(np.float32) for e in (e1, e2, e3))
        r = (e1, e2, e3, m1, np.sqrt(m1 * m2, dtype=np.float32), m1 - m2, m3, -((e1 + e2) + e3))[measure]
    r = np.array(r, dtype=np.float32)
    nan = np.isnan(e1) | np.isnan(e2) | np.isnan(e3) | np.isnan(r)
    r.view(np.uint32)[nan] = CANONICAL_NAN
    return r


def accumulate(old: np.ndarray, r: np.ndarray) -> np.ndarray:
    """``np.maximum(old, r)`` with a NaN made canonical.  Between ``-0.0`` and ``+0.0``, where numpy's answer depends on the
    loop it takes, the stored value stays (``old >= r ? old : r``): the bits are pinned to that, the values to numpy."""
    old, r = np.asarray(old, dtype=np.float32), np.asarray(r, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        out = np.where(old >= r, old, r).astype(np.float32)
        out[np.isnan(old) | np.isnan(r)] = np.nan
        assert np.array_equal(out, np.maximum(old, r), equal_nan=True)
    out.view(np.uint32)[np.isnan(old) | np.isnan(r)] = CANONICAL_NAN
    return out


def gaussian_blur(vol: np.ndarray, sigma, sampling=(1, 1, 1)) -> np.ndarray:
    """The package's blur restated in float64: per axis ``sigma / s`` voxels, radius ``min(int(4 sigma_a + 0.5), n - 1)``,
    normalised taps, the border mirrored about the edge voxel (numpy's ``reflect`` padding).  For the scenes only."""
    out = np.asarray(vol, dtype=np.float64)
    for axis in range(3):
        sa = float(sigma) / float(sampling[axis])
        r = min(int(4 * sa + 0.5), out.shape[axis] - 1)
        if r == 0:
            continue
        taps = np.exp(-0.5 * (np.arange(-r, r + 1) / sa) ** 2)
        taps /= taps.sum()
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        padded = np.pad(out, pad, mode="reflect")
        acc = np.zeros_like(out)
        for k in range(2 * r + 1):
            acc += taps[k] * np.take(padded, range(k, k + out.shape[axis]), axis=axis)
        out = acc
    return out
