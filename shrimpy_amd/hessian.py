"""Ridge, sheet and blob filters on the eigenvalues of the Gaussian-smoothed Hessian: Sato's tubeness (ImageJ's "Tubeness",
skimage's ``sato``), its sheet and blob counterparts and the scale-normalised Laplacian.

``csrc/hessian.hip`` runs on the device (one launch per scale: a workgroup stages its tile of the blurred volume and a halo of
2 in LDS, every voxel computes the Hessian in float64, its eigenvalues by cyclic Jacobi and the measure, and writes one float),
``csrc/host_twins.hip`` on the CPU over the same derivative, entries, sweeps and responses (``csrc/hessian.hpp``).  The rule,
PINNED to numpy (``np.gradient`` twice and ``np.linalg.eigvalsh``: what ``skimage.feature.hessian_matrix`` with
``use_gaussian_derivatives=False`` and ``hessian_matrix_eigvals`` compute; ``tests/hessian_ref.py``):

* ``g`` is ``vol`` blurred as ``segment``'s ``sigma`` blurs, with per-axis voxel sigma ``sigma / s_a`` and radius
  ``int(4 sigma_a + 0.5)`` (at most the blur's cap, :data:`MAX_BLUR_RADIUS`; a wider one is a ``ValueError``);
* ``H_ab = D_b (D_a g)`` with numpy's central differences inside and one-sided ones at the faces, 0 along an axis of length 1;
* ``e1 <= e2 <= e3`` are ``sigma^2`` times the eigenvalues of ``H`` (of ``-H`` with ``dark``), rounded to float32 once;
* with ``m_k = max(-e_k, 0)``: ``ridge`` ``m1``, ``tube`` ``sqrt(m1 m2)``, ``sheet`` ``m1 - m2``, ``blob`` ``m3``, ``log``
  ``-(e1 + e2 + e3)``, each a float32 function of the three;
* a voxel whose stencil holds a non-finite value is NaN; the maximum over several sigmas is NaN where one of them is.

Not built: Frangi's ratio form with its three parameters, eigenvectors and orientation, a blur pass fused into the kernel,
uint16 volumes, multi-GPU or slab filtering, non-maximum suppression of ridges.
"""

from __future__ import annotations

import ctypes
import math

from . import _lib
from .segment import _check_volume, _run, _same_volume, _shape3

__all__ = ["tiling", "MEASURES", "MAX_BLUR_RADIUS", "hessian_eigenvalues", "hessian_response", "enhance"]

MEASURES = {"e1": 0, "e2": 1, "e3": 2, "ridge": 3, "tube": 4, "sheet": 5, "blob": 6, "log": 7}
MAX_BLUR_RADIUS = 64          # lsr_blur_reflect_f32's cap on the radius


def tiling() -> tuple[int, int, int, int]:
    """``(halo, tile z, tile y, tile x)``: the outputs a workgroup takes and the halo it stages (``lsr_hessian_tiling``)."""
    out = (ctypes.c_int * 4)()
    _lib.call("lsr_hessian_tiling", out)
    return tuple(out)


def _measure(measure) -> int:
    if measure not in MEASURES:
        raise ValueError(f"measure must be one of {list(MEASURES)}, got {measure!r}")
    return MEASURES[measure]


def _sampling(sampling) -> tuple[float, float, float]:
    try:
        s = tuple(float(v) for v in sampling)
    except TypeError as exc:
        raise ValueError(f"sampling must be (sz, sy, sx), got {sampling!r}") from exc
    if len(s) != 3 or not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"sampling must be three positive finite numbers, got {sampling!r}")
    return s


def blur_radii(sigma, sampling=(1, 1, 1)) -> tuple[int, int, int]:
    """The blur's radius per axis for a ``sigma`` in the units of ``sampling``: ``int(4 sigma / s_a + 0.5)``; one above the
    blur's cap of :data:`MAX_BLUR_RADIUS` voxels, and a sigma that is not positive and finite, is a ``ValueError``."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be positive and finite, got {sigma!r}")
    radii = tuple(int(4 * (sigma / s) + 0.5) for s in _sampling(sampling))
    if max(radii) > MAX_BLUR_RADIUS:
        raise ValueError(f"sigma {sigma} at sampling {tuple(sampling)} needs blur radii {radii}: the blur's cap is "
                         f"{MAX_BLUR_RADIUS} voxels")
    return radii


def _blur(vol, sigma: float, sampling, buffers):
    """``vol`` blurred along z, y and x into ``buffers`` (two volumes like ``vol``, taken in turn): the pass of
    ``dynatrack._gaussian_blur_3d`` with the voxel sigma ``sigma / s_a`` of each axis.  Returns the buffer that holds the
    result (``vol`` itself if no axis has a window)."""
    import torch

    z, y, x = _shape3(vol, "vol")
    src, turn = vol, 0
    for axis, (n, radius, s) in enumerate(zip((z, y, x), blur_radii(sigma, sampling), _sampling(sampling))):
        r = min(radius, n - 1)   # (the reflect border needs radius < axis length)
        if r == 0:
            continue
        xs = torch.arange(-r, r + 1, device=vol.device, dtype=torch.float32)
        k1d = torch.exp(-0.5 * (xs / (sigma / s)) ** 2)
        k1d = (k1d / k1d.sum()).contiguous()
        dst = buffers[turn]
        _run(vol.device, "lsr_blur_reflect_f32", src.data_ptr(), dst.data_ptr(), z, y, x, axis, k1d.data_ptr(), r,
             ctypes.c_float(0.0), ctypes.c_float(0.0))
        src, turn = dst, 1 - turn
    return src


def _respond(g, out, sampling, scale: float, measure: int, dark: bool, accumulate: bool) -> None:
    z, y, x = _shape3(g, "vol")
    _run(g.device, "lsr_hessian_response_f32", g.data_ptr(), out.data_ptr(), z, y, x, *(ctypes.c_double(s) for s in sampling),
         ctypes.c_double(scale), measure, int(bool(dark)), int(bool(accumulate)))


def _buffers(vol):
    import torch

    return [torch.empty_like(vol), torch.empty_like(vol)]


def hessian_eigenvalues(vol, sigma, sampling=(1, 1, 1), dark=False):
    """``(e1, e2, e3)``, ``e1 <= e2 <= e3``: ``sigma^2`` times the eigenvalues of the Hessian of ``vol`` ((Z, Y, X) float32)
    blurred at ``sigma`` (in the units of ``sampling``), of its negative with ``dark``: three new float32 tensors on ``vol``'s
    device."""
    import torch

    vol = _check_volume(vol, "vol", torch.float32)
    sampling = _sampling(sampling)
    sigma = float(sigma)
    g = _blur(vol, sigma, sampling, _buffers(vol))
    outs = tuple(torch.empty_like(vol) for _ in range(3))
    for k, out in enumerate(outs):
        _respond(g, out, sampling, sigma * sigma, k, dark, False)
    return outs


def hessian_response(vol, sigma, measure, sampling=(1, 1, 1), dark=False, out=None, _scratch=None):
    """The ``measure`` (a name of :data:`MEASURES`) of ``vol`` at ``sigma``: a new float32 tensor, or with ``out`` (a float32
    volume like ``vol`` on its device) the voxelwise maximum of ``out`` and the response, stored in ``out`` and returned."""
    import torch

    vol = _check_volume(vol, "vol", torch.float32)
    code = _measure(measure)
    sampling = _sampling(sampling)
    sigma = float(sigma)
    blur_radii(sigma, sampling)
    if out is not None:
        out = _check_volume(out, "out", torch.float32)
        _same_volume(vol, out, "vol", "out")
        if out.data_ptr() == vol.data_ptr():
            raise ValueError("out must not be vol")
    g = _blur(vol, sigma, sampling, _scratch if _scratch is not None else _buffers(vol))
    result = torch.empty_like(vol) if out is None else out
    _respond(g, result, sampling, sigma * sigma, code, dark, out is not None)
    return result


def enhance(vol, measure, sigmas, sampling=(1, 1, 1), dark=False):
    """The maximum over ``sigmas`` of :func:`hessian_response` -- the multi-scale response as Sato and Frangi define it: a new
    float32 tensor.  Two blur buffers and the output are all it allocates, whatever the number of scales."""
    import torch

    vol = _check_volume(vol, "vol", torch.float32)
    _measure(measure)
    sigmas = [float(s) for s in sigmas]
    if not sigmas:
        raise ValueError("sigmas is empty")
    for sigma in sigmas:
        blur_radii(sigma, sampling)
    scratch = _buffers(vol)
    out = hessian_response(vol, sigmas[0], measure, sampling, dark, _scratch=scratch)
    for sigma in sigmas[1:]:
        hessian_response(vol, sigma, measure, sampling, dark, out=out, _scratch=scratch)
    return out
