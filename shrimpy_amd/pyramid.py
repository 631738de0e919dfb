"""Multiscale pyramids: the lower levels of an NGFF ``multiscales`` list, computed where the result already is.

NGFF viewers open a large volume through the coarser arrays ``"1"``, ``"2"``, ... of its ``multiscales`` block.  Level
``k`` here is the 2x mean of level ``k - 1`` (never of level 0 directly), factors ``(fz, 2, 2)`` with ``fz`` 1 or 2.
iohub's ``initialize_pyramid`` / ``compute_pyramid`` is the counterpart; it is not vendored, so the convention at the
far faces is this package's own (**PARITY UNPINNED**; ``tests/pyramid_ref.py`` restates it in float64):

* the output has ``ceil(n / f)`` voxels per axis; output voxel ``(z, y, x)`` is the mean over the input voxels
  ``(fz z + a, 2 y + b, 2 x + c)`` that lie inside the volume -- nothing is padded and nothing dropped, so a window holds
  1, 2, 4 or 8 voxels, always a power of two;
* float32: ``s = ((v000 + v001) + (v010 + v011)) + ((v100 + v101) + (v110 + v111))`` in float32 (x pairs, then y, then
  z; a missing neighbour is left out), result ``s * 2^-k``: three roundings, ``|out - exact| <= 3 * 2^-24 * mean|v|`` of
  the window; device and host agree bit for bit (one definition, ``csrc/pyramid.hpp``);
* uint16: 32-bit sum, ``(sum + (count >> 1)) >> k``: round half up, exact.

A HIP tensor runs ``csrc/pyramid.hip`` on the current stream, a CPU tensor the host twin; results are torch tensors on
the volume's device.
"""

from __future__ import annotations

import ctypes

from . import _lib

__all__ = ["MAX_LEVELS", "downsample2", "level_shapes", "build_levels"]

MAX_LEVELS = 8


def _check_fz(fz) -> int:
    if fz not in (1, 2):
        raise ValueError(f"fz must be 1 or 2, got {fz!r}")
    return int(fz)


def level_shapes(shape_zyx, levels: int, fz: int = 2):
    """``(shapes, factors)`` of levels ``0 .. levels - 1``: ``shapes[k]`` is level ``k``'s ``(Z, Y, X)`` -- ``ceil`` of
    the level above over ``(fz, 2, 2)`` -- and ``factors[k] = (fz^k, 2^k, 2^k)`` what its voxel size is multiplied by."""
    fz = _check_fz(fz)
    levels = int(levels)
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be in 1 .. {MAX_LEVELS}, got {levels}")
    shape = tuple(int(n) for n in shape_zyx)
    if len(shape) != 3 or min(shape) <= 0:
        raise ValueError(f"expected a positive (Z, Y, X) shape, got {tuple(shape_zyx)}")
    shapes, factors = [shape], [(1, 1, 1)]
    for k in range(1, levels):
        z, y, x = shapes[-1]
        shapes.append((-(-z // fz), -(-y // 2), -(-x // 2)))
        factors.append((fz ** k, 2 ** k, 2 ** k))
    return shapes, factors


def downsample2(volume, fz: int = 2):
    """The next pyramid level of ``volume`` ((Z, Y, X), float32 or uint16, contiguous): a new tensor on its device."""
    import torch

    fz = _check_fz(fz)
    if not isinstance(volume, torch.Tensor):
        raise TypeError(f"volume must be a torch.Tensor, got {type(volume).__name__}")
    if volume.dtype == torch.float32:
        name = "lsr_downsample2_f32"
    elif volume.dtype == torch.uint16:
        name = "lsr_downsample2_u16"
    else:
        raise TypeError(f"volume must be float32 or uint16, got {volume.dtype}")
    if volume.dim() != 3:
        raise ValueError(f"volume must be (Z, Y, X), got shape {tuple(volume.shape)}")
    if not volume.is_contiguous():
        raise ValueError("volume must be contiguous")
    if volume.device.type not in ("cpu", "cuda"):
        raise ValueError(f"volume is on {volume.device}: a HIP device or the CPU")
    z, y, x = (int(n) for n in volume.shape)
    out3 = (ctypes.c_int64 * 3)()
    _lib.call("lsr_downsample2_shape", z, y, x, fz, out3)
    out = torch.empty(tuple(out3), dtype=volume.dtype, device=volume.device)
    if volume.device.type == "cpu":
        from .host import _threads

        _threads()
        _lib.call(name + "_cpu", volume.data_ptr(), z, y, x, out.data_ptr(), fz, None)
    else:
        with torch.cuda.device(volume.device):
            _lib.call(name, volume.data_ptr(), z, y, x, out.data_ptr(), fz, _lib.stream_ptr(volume.device))
    return out


def build_levels(volume, levels: int, fz: int = 2) -> list:
    """Levels ``1 .. levels - 1`` of ``volume`` (level 0), each from the one above it; ``[]`` for ``levels == 1``."""
    level_shapes(tuple(volume.shape), levels, fz)      # (validates levels and fz)
    out, cur = [], volume
    for _ in range(1, int(levels)):
        cur = downsample2(cur, fz)
        out.append(cur)
    return out
