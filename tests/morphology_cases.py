"""The cases of the grey-morphology tests (``tests/test_morphology_host.py``, ``tests/test_morphology_gpu.py``), sized from the
exported tiling (``lsr_grey_morph_tiling``): with ``c`` the columns per workgroup of the strided passes, ``R`` the greatest
half-width and ``S`` the outputs per staged row segment of the x pass,

* shapes: the three smallest; a row and a column count of ``c + 6`` (a second workgroup with 6 live lanes); every axis at
  ``2R + 3`` (a window at the cap with one voxel that sees the whole of it, and a second block of the walk), the y one over
  ``c + 1`` columns; an axis of exactly ``w``, ``w + 1`` and ``2w - 1`` for ``w = 5``; a row of ``S + 7`` (the x pass carries
  its halo into a second segment);
* half-widths: none, mixed with a zero, a cube, three different ones, the cap ``R`` on the longest axis (on every axis in turn
  for the (5, 9, 13) shape), and one larger than every axis it acts on;
* contents: noise, small integers (many ties), a ramp up and down each axis, a constant, one spike, +-inf at 10 %, NaN at 10 %
  (two payloads), a mix of ``-0.0`` and ``+0.0``.

Every array is read-only: the tests share them.
"""

import functools

import numpy as np

from shrimpy_amd import morphology as M

R, COLUMNS, SEGMENT, _ = M.tiling()
W5 = 5

SHAPES = [(1, 1, 1), (2, 3, 5), (5, 9, 13),
          (3, 4, COLUMNS + 6),
          (3, COLUMNS + 6, 5),
          (2 * R + 3, 1, 3), (1, 2 * R + 3, COLUMNS + 1), (1, 1, 2 * R + 3),
          (W5, W5 + 1, 2 * W5 - 1),
          (2, 1, SEGMENT + 7)]
SMALLEST = SHAPES[:3]

CONTENTS = ["noise", "small_integers", "ramp_up_z", "ramp_down_z", "ramp_up_y", "ramp_down_y", "ramp_up_x", "ramp_down_x",
            "constant", "spike", "inf", "nan", "zeros"]
NAN_FREE = [c for c in CONTENTS if c != "nan"]

OPS = ["grey_erosion", "grey_dilation", "grey_opening", "grey_closing", "white_tophat", "black_tophat"]


def half_widths_of_shape(shape):
    """The half-width triples a shape is run at."""
    out = [(0, 0, 0), (1, 0, 2), (2, 2, 2), (7, 1, 3)]
    axes = (0, 1, 2) if shape == (5, 9, 13) else (int(np.argmax(shape)),)
    out += [tuple(R if a == axis else 0 for a in range(3)) for axis in axes]
    out.append(tuple(min(n, R) for n in shape))                # (n > n - 1: wider than the axis wherever n <= R)
    return out


PARAMS = [(shape, r) for shape in SHAPES for r in half_widths_of_shape(shape)]
PARAM_IDS = ["x".join(map(str, s)) + "-r" + "_".join(map(str, r)) for s, r in PARAMS]


@functools.lru_cache(maxsize=None)
def volume(shape, content):
    """The float32 volume of a case (read-only)."""
    return filled(shape, content, np.random.default_rng([SHAPES.index(shape), CONTENTS.index(content)]))


def filled(shape, content, rng):
    """``content`` at ``shape`` from ``rng`` (read-only): what ``volume`` caches, for case files with shapes of their own."""
    n = int(np.prod(shape))
    if content == "noise":
        v = rng.normal(size=shape)
    elif content == "small_integers":
        v = rng.integers(-2, 3, size=shape)
    elif content.startswith("ramp_"):
        axis = "zyx".index(content[-1])
        line = np.arange(shape[axis], dtype=np.float64) * 0.25 - 3.0
        if "_down_" in content:
            line = line[::-1]
        v = np.broadcast_to(line.reshape([-1 if a == axis else 1 for a in range(3)]), shape)
    elif content == "constant":
        v = np.full(shape, 2.5)
    elif content == "spike":
        v = np.zeros(shape)
        v.flat[n // 2] = 9.0
    elif content == "inf":
        v = rng.normal(size=shape)
        u = rng.random(size=shape)
        v[u < 0.05] = np.inf
        v[u > 0.95] = -np.inf
    elif content == "nan":
        v = rng.normal(size=shape).astype(np.float32)
        u = rng.random(size=shape)
        bits = v.view(np.uint32)
        bits[u < 0.05] = 0x7FC00000
        bits[u > 0.95] = 0xFFC00001                                # a negative NaN with a payload
        v = bits.view(np.float32)
    elif content == "zeros":
        v = np.where(rng.random(size=shape) < 0.5, -0.0, 0.0)
    else:
        raise KeyError(content)
    v = np.ascontiguousarray(v, dtype=np.float32)
    v.setflags(write=False)
    return v


# ---- the scenes of the segmentation tests ---------------------------------------------------------------------------------------

RAMP_SHAPE = (12, 40, 96)
RAMP_THRESHOLD = 30.0
BALL_CENTRES = [(6, y, x) for y in (10, 30) for x in (16, 48, 80)]


def ball(shape, centre, radius_sq):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius_sq


@functools.lru_cache(maxsize=None)
def ramp_scene():
    """Six balls of amplitude 60 and radius 3 (123 voxels each) on the ramp ``4 * x``: no global threshold separates them."""
    vol = np.broadcast_to(4.0 * np.arange(RAMP_SHAPE[2], dtype=np.float32), RAMP_SHAPE).copy()
    for centre in BALL_CENTRES:
        vol[ball(RAMP_SHAPE, centre, 9)] += 60.0
    vol.setflags(write=False)
    return vol


SHELL_SHAPE = (15, 16, 17)


@functools.lru_cache(maxsize=None)
def shell_mask():
    """A hollow shell, 15 < d^2 <= 36 around (7, 8, 8): 674 voxels, 925 once filled."""
    mask = ball(SHELL_SHAPE, (7, 8, 8), 36) & ~ball(SHELL_SHAPE, (7, 8, 8), 15)
    mask.setflags(write=False)
    return mask


@functools.lru_cache(maxsize=None)
def open_shell_mask():
    """The shell with a tunnel from its hollow to the face z = 0: the hole touches a face and stays open."""
    mask = shell_mask().copy()
    mask[:8, 8, 8] = False
    mask.setflags(write=False)
    return mask
