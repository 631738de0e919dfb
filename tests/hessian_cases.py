"""The cases of the Hessian tests (``tests/test_hessian_host.py``, ``tests/test_hessian_gpu.py``), sized from the exported tiling
(``lsr_hessian_tiling``): with ``h`` the halo and ``(tz, ty, tx)`` the tile of outputs of a workgroup,

* shapes: per axis ``1 .. 5`` -- every composition of one-sided and central differences, and the length-1 rule -- and ``t - 1``,
  ``t``, ``t + 1``, ``2t + 1`` -- the halo crossing tile faces; ``(2tz + 1, 2ty + 1, 2tx + 1)``, the largest, is three tiles on
  every axis, the last with one live plane, row and lane;
* samplings: isotropic, dyadic anisotropic, and the config-2 voxel;
* contents: zeros, a constant, a ramp, five exact quadratics ``1/2 r^T A r`` (``r`` in the units of the sampling, from the centre
  voxel, so that under dyadic sampling every value is exact in float32 and the interior Hessian is ``A``), noise, noise on a
  pedestal of 1e4 (cancellation), a blurred bead scene, and noise with a NaN in the interior, ``+inf`` at a tile face and
  ``-inf`` at the volume's corner.

Every array is read-only: the tests share them.
"""

import functools

import numpy as np

from shrimpy_amd import hessian as K
from tests import hessian_ref as R

HALO, TZ, TY, TX = K.tiling()
TILE = (TZ, TY, TX)

SHAPES = [(1, 1, 1), (2, 3, 4), (3, 4, 5), (4, 5, 2), (5, 2, 3), (TZ - 1, TY - 1, TX - 1), (TZ, TY, TX), (TZ + 1, TY + 1, TX + 1),
          (2 * TZ + 1, 2 * TY + 1, 2 * TX + 1), (1, 2 * TY + 1, 2), (2, 1, 2 * TX + 1)]
LARGEST = SHAPES[8]
SAMPLINGS = [(1.0, 1.0, 1.0), (2.0, 0.5, 0.5), (0.4, 0.116, 0.116)]
DYADIC = SAMPLINGS[:2]
SCALE = 2.25                                   # sigma = 1.5

QUADRATICS = {
    "quadratic_ball": np.diag([2, 2, 2]),
    "quadratic_tube": np.diag([1, 1, 3]),
    "quadratic_saddle": np.diag([-3, -3, 1]),
    "quadratic_full": np.array([[1, 2, -1], [2, -2, 3], [-1, 3, 1]]),           # eigenvalues of both signs
    "quadratic_rank1": np.outer([1, 2, -1], [1, 2, -1]),
}
CONTENTS = ["zeros", "constant", "ramp", *QUADRATICS, "noise", "pedestal", "beads", "nonfinite"]
MEASURES = list(R.MEASURES)

PARAMS = [(shape, s) for shape in SHAPES for s in SAMPLINGS]
PARAM_IDS = ["x".join(map(str, shape)) + "-s" + "_".join(map(str, s)) for shape, s in PARAMS]


def nonfinite_sites(shape):
    """Where the non-finite content puts its NaN (interior), ``+inf`` (the first voxel of the second tile, or the last voxel
    of a shorter axis) and ``-inf`` (the corner): later ones win where a small shape makes them coincide."""
    interior = tuple(min(3, n // 2) for n in shape)
    face = tuple(min(t, n - 1) for t, n in zip(TILE, shape))
    return interior, face, (0, 0, 0)


@functools.lru_cache(maxsize=None)
def volume(shape, content, sampling=(1.0, 1.0, 1.0)):
    """The float32 volume of a case (read-only).  Only the quadratics depend on the sampling."""
    rng = np.random.default_rng([SHAPES.index(shape), CONTENTS.index(content)])
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    if content == "zeros":
        v = np.zeros(shape)
    elif content == "constant":
        v = np.full(shape, 1e4)
    elif content == "ramp":
        v = 0.25 * x - 0.5 * y + 3.0 * z - 3.0
    elif content in QUADRATICS:
        A = QUADRATICS[content]
        r = [(c - n // 2) * s for c, n, s in zip((z, y, x), shape, sampling)]
        v = sum(0.5 * A[a, b] * r[a] * r[b] for a in range(3) for b in range(3)) + np.zeros(shape)
    elif content == "noise":
        v = rng.normal(size=shape)
    elif content == "pedestal":
        v = 1e4 + rng.normal(size=shape)
    elif content == "beads":
        v = np.zeros(shape)
        v[rng.random(size=shape) < 0.02] = 1000.0
        v = R.gaussian_blur(v, 1.5)
    elif content == "nonfinite":
        v = rng.normal(size=shape)
        for site, value in zip(nonfinite_sites(shape), (np.nan, np.inf, -np.inf)):
            v[site] = value
    else:
        raise KeyError(content)
    v = np.ascontiguousarray(v, dtype=np.float32)
    v.setflags(write=False)
    return v


def case_volume(shape, content, sampling):
    return volume(shape, content, tuple(sampling) if content in QUADRATICS else SAMPLINGS[0])


@functools.lru_cache(maxsize=None)
def reference(shape, content, sampling, dark):
    """``(l, norm, mask)`` of ``tests/hessian_ref.py`` for a case, computed once (read-only)."""
    out = R.eigenvalues(case_volume(shape, content, sampling), sampling, dark)
    for a in out:
        a.setflags(write=False)
    return out


def face_classes(n, t):
    """Per index of an axis of length ``n`` under tiles of ``t``: ``(distance to the first voxel, to the last, to the tile's
    first voxel, to its last)``, each capped at the halo -- what decides the form of the differences and where the halo is
    read across a tile face."""
    i = np.arange(n)
    p = i % t
    last = np.minimum(t - 1, n - 1 - (i - p))           # the tile's last live voxel
    return np.stack([np.minimum(i, HALO), np.minimum(n - 1 - i, HALO), np.minimum(p, HALO), np.minimum(last - p, HALO)], axis=1)


# ---- the structure scene -----------------------------------------------------------------------------------------------------------

STRUCTURE_SHAPE = (40, 48, 56)
TUBE_CENTRE, PLATE_CENTRE, BALL_CENTRE, BACKGROUND = (10, 12, 28), (30, 34, 28), (10, 30, 28), (30, 10, 28)


@functools.lru_cache(maxsize=None)
def structures():
    """Zeros with a tube of radius 2 along x, a plate three voxels thick and a ball of radius 3, all at 100."""
    z, y, x = np.ogrid[:STRUCTURE_SHAPE[0], :STRUCTURE_SHAPE[1], :STRUCTURE_SHAPE[2]]
    vol = np.zeros(STRUCTURE_SHAPE, dtype=np.float32)
    span = (x > 6) & (x < 50)
    vol[((z - 10) ** 2 + (y - 12) ** 2 <= 4) & span] = 100.0
    vol[(np.abs(y - 34) <= 1) & (z > 22) & (z < 38) & span] = 100.0
    vol[(z - 10) ** 2 + (y - 30) ** 2 + (x - 28) ** 2 <= 9] = 100.0
    vol.setflags(write=False)
    return vol


# ---- the segmentation scene --------------------------------------------------------------------------------------------------------

TUBES_SHAPE = (16, 40, 96)


@functools.lru_cache(maxsize=None)
def tubes_on_a_ramp():
    """``4 x + N(0, 1)`` with two tubes of radius 2 raised by 60, one along x and one along y: ``(volume, mask of the tubes)``."""
    z, y, x = np.ogrid[:TUBES_SHAPE[0], :TUBES_SHAPE[1], :TUBES_SHAPE[2]]
    vol = 4.0 * x + np.random.default_rng(5).normal(size=TUBES_SHAPE)
    along_x = ((z - 8) ** 2 + (y - 10) ** 2 <= 4) & (x > 8) & (x < 88)
    along_y = ((z - 8) ** 2 + (x - 48) ** 2 <= 4) & (y > 18) & (y < 36)
    tubes = along_x | along_y
    vol[tubes] += 60.0
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    vol.setflags(write=False)
    tubes.setflags(write=False)
    return vol, tubes
