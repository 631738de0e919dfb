"""The hot path on HOST tensors: what runs when no HIP device is visible.

The reference resolves its device as ``cuda`` if available, else ``cpu`` (``shrimpy/preprocessing.py:78-82``)
and its CI has no GPU (``shrimpy/tests/conftest.py:11-17``), so a drop-in has to accept CPU tensors too --
BASELINE config 1 ("deskew-only via the CPU path, plumbing, no GPU") is exactly that.  The public functions
(``deskew.fast_deskew_zyx``, ``register.apply_affine_transform_zyx``, ``deconvolve.richardson_lucy`` /
``correlate3d``) hand CPU tensors to the functions below, which call the native host twins of
``csrc/host_twins.hip`` (``lsr_*_cpu``: the device entry points' signatures, host pointers, the same
arithmetic in the same order -- results equal the kernels' bit for bit).  Nothing here imports, calls or
reads anything under ``oracle/``; the library must be built (``_lib.load`` raises otherwise).

Threads: ``lsr_set_host_threads`` is set from ``torch.get_num_threads()`` at each call -- the knob the
reference's CPU path is governed by -- and the twins use plain ``std::thread`` (no second OpenMP runtime).
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, rl_loop

__all__ = ["is_host", "deskew_with_matrix", "average_n_slices", "apply_affine", "correlate3d", "richardson_lucy"]

_MODES = {"constant": _lib.MODE_CONSTANT, "grid-constant": _lib.MODE_GRID_CONSTANT}


def is_host(t) -> bool:
    import torch

    return isinstance(t, torch.Tensor) and t.device.type == "cpu"


_warned = [False]


def _threads() -> None:
    """Worker count of the twins = torch's CPU thread count; and, once per process, a warning when a HIP device
    is visible: the kernels are the product's path there, and a CPU tensor reaching this module on such a box
    should be a decision, not an accident (nothing falls back silently)."""
    import torch

    if not _warned[0] and torch.cuda.is_available():
        import warnings

        _warned[0] = True
        warnings.warn("shrimpy_amd: a CPU tensor is being processed by the native host twins although a HIP device is "
                      "visible; move the tensor to the device to run the gfx950 kernels", RuntimeWarning, stacklevel=3)
    _lib.call("lsr_set_host_threads", max(1, min(1024, int(torch.get_num_threads()))))


def _f32(t, name: str):
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cpu":
        raise ValueError(f"{name} is on {t.device}; the host path takes CPU tensors")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def average_n_slices(data, avg: int):
    import torch

    data = _f32(data, "data")
    if avg == 1:
        return data
    zd, y, x = (int(v) for v in data.shape)
    out = torch.empty((-(-zd // avg), y, x), dtype=torch.float32)
    _threads()
    _lib.call("lsr_average_slices_f32_cpu", data.data_ptr(), zd, y, x, out.data_ptr(), int(out.shape[0]), avg, None)
    return out


def deskew_with_matrix(raw, m, pre_average_shape, avg: int, out=None, flat_field=None, border: str = "constant", cval=None):
    """``deskew.deskew_with_matrix`` for a CPU tensor (float32 or uint16 counts), dense ``out`` only.
    ``cval``: ``None`` (zero) or a one-element float32 CPU tensor (``deskew.fill_value``)."""
    import torch

    if flat_field is not None:     # (the fusion is a kernel matter; the values are those of correcting first)
        raw = flat_field.apply(raw)
    u16 = raw.dtype == torch.uint16
    if not u16:
        raw = _f32(raw, "raw_data")
    elif not raw.is_contiguous():
        raise ValueError("raw_data must be contiguous")
    zd, yo, xo = (int(v) for v in pre_average_shape)
    zo = -(-zd // avg)
    if out is None:
        out = torch.empty((zo, yo, xo), dtype=torch.float32)
    else:
        if hasattr(out, "logical_ptr"):
            raise ValueError("a padded device volume cannot receive a host deskew")
        _f32(out, "out")
        if tuple(out.shape) != (zo, yo, xo):
            raise ValueError(f"out must be {(zo, yo, xo)} on cpu")
    z, y, x = (int(v) for v in raw.shape)
    _threads()
    try:
        if border != "constant":
            raise _lib.LsrUnsupported("lsr_deskew_f32_cpu", _lib.E_UNSUPPORTED, "grid-constant border")
        if cval is not None:
            _lib.call("lsr_deskew_cval_cpu", raw.data_ptr(), 1 if u16 else 0, z, y, x, out.data_ptr(), zo, yo, xo, xo, yo * xo,
                      zd, _lib.matrix12(m), avg, _lib.MODE_CONSTANT, None, None, cval.data_ptr(), None)
        else:
            _lib.call("lsr_deskew_u16_cpu" if u16 else "lsr_deskew_f32_cpu", raw.data_ptr(), z, y, x, out.data_ptr(),
                      zo, yo, xo, xo, yo * xo, zd, _lib.matrix12(m), avg, None)
    except _lib.LsrUnsupported:
        # a general matrix, or the blending border rule: trilinear resample, then average
        src = raw.to(torch.float32) if u16 else raw
        pre = out if avg == 1 else torch.empty((zd, yo, xo), dtype=torch.float32)
        _lib.call("lsr_affine_f32_cpu", src.data_ptr(), z, y, x, pre.data_ptr(), zd, yo, xo, _lib.matrix12(m),
                  ctypes.c_float(0.0 if cval is None else float(cval.item())), _MODES[border], None)
        if avg > 1:
            _lib.call("lsr_average_slices_f32_cpu", pre.data_ptr(), zd, yo, xo, out.data_ptr(), zo, avg, None)
    _lib.mark_written(out)
    return out


def apply_affine(moving, m, shape, mode: str, cval: float, out=None):
    """``register.apply_affine_transform_zyx`` for a CPU tensor: scipy's fp64 arithmetic (``exact``)."""
    import torch

    moving = _f32(moving, "moving")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32)
    else:
        if hasattr(out, "logical_ptr"):
            raise ValueError("a padded device volume cannot receive a host resample")
        _f32(out, "out")
        if tuple(out.shape) != tuple(shape):
            raise ValueError(f"out must be {tuple(shape)} on cpu")
        if out.data_ptr() == moving.data_ptr():
            raise ValueError("out must not alias moving")
    zi, yi, xi = (int(v) for v in moving.shape)
    _threads()
    _lib.call("lsr_affine_f32_cpu", moving.data_ptr(), zi, yi, xi, out.data_ptr(), int(shape[0]), int(shape[1]),
              int(shape[2]), _lib.matrix12(m), ctypes.c_float(float(cval)), _MODES[mode], None)
    _lib.mark_written(out)
    return out


def _taps(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def correlate3d(volume, weights=None, weight_factors=None):
    """``scipy.ndimage.correlate(volume, weights, mode="constant", cval=0)`` on a CPU tensor."""
    import torch

    from .deconvolve import prepare_psf

    vol = _f32(volume, "volume")
    if vol.dim() != 3:
        raise ValueError("volume must be (Z, Y, X)")
    out = torch.empty_like(vol)
    z, y, x = (int(v) for v in vol.shape)
    _threads()
    if weight_factors is not None:
        wz, wy, wx = (_taps(np.asarray(k).ravel()) for k in weight_factors)
        _lib.call("lsr_correlate_sep_f32_cpu", vol.data_ptr(), out.data_ptr(), None, z, y, x, wz.ctypes.data, len(wz),
                  wy.ctypes.data, len(wy), wx.ctypes.data, len(wx), _lib.EPI_NONE, ctypes.c_float(0.0), None, None, None,
                  None)
    else:
        w = prepare_psf(weights)
        _lib.call("lsr_correlate_dense_f32_cpu", vol.data_ptr(), out.data_ptr(), None, z, y, x, w.ctypes.data, w.shape[0],
                  w.shape[1], w.shape[2], _lib.EPI_NONE, ctypes.c_float(0.0), None, None)
    return out


class _SeparableStepper:
    """The separable form, between rotating volumes: ``ratio = y / (H x + eps)`` (H = correlation with the flipped taps),
    then ``x * H^T ratio / H^T 1`` into the other volume."""

    rotates, dense_out = True, False

    def __init__(self, y, x, factors, eps: float):
        import torch

        from .deconvolve import _axis_norm

        self.y, self.eps, self.ratio, self._vols = y, ctypes.c_float(eps), torch.empty_like(y), (x, torch.empty_like(y))
        self.k, self.kf = [_taps(f) for f in factors], [_taps(f[::-1]) for f in factors]
        self.norm = [_axis_norm(f, n) for f, n in zip(factors, y.shape)]

    def volumes(self):
        return self._vols

    def third(self):
        import torch

        return torch.empty_like(self.y)

    def _correlate(self, src, dst, aux, taps, epilogue, sp=None) -> None:
        _lib.call("lsr_correlate_sep_stats_f32_cpu", src.data_ptr(), dst.data_ptr(), aux.data_ptr(), *self.y.shape,
                  taps[0].ctypes.data, len(taps[0]), taps[1].ctypes.data, len(taps[1]), taps[2].ctypes.data, len(taps[2]),
                  epilogue, self.eps, self.norm[0].ctypes.data, self.norm[1].ctypes.data, self.norm[2].ctypes.data, sp, None)

    def run(self, it0, n, x_out, rows, ab=None) -> None:
        rd, wr = ab or self._vols
        for it in range(it0, it0 + n):
            self._correlate(rd, self.ratio, self.y, self.kf, _lib.EPI_RATIO)
            self._correlate(self.ratio, wr, rd, self.k, _lib.EPI_UPDATE, rl_loop.row_ptr(rows, it))
            rd, wr = wr, rd


class _DenseStepper:
    """The dense form, in place in ``cur``: one native call for ``n`` iterations (the twin of ``lsr_rl_dense_f32``).
    What the launches behind an iteration need is cloned aside; an accelerated run lets ``cur`` and ``held`` trade
    places instead of copying p_{k+1} back."""

    rotates = dense_out = False

    def __init__(self, y, x, w, eps: float):
        import torch

        from .deconvolve import _prefix_table

        self.y, self.cur, self.eps, self.ratio, self._held = y, x, ctypes.c_float(eps), torch.empty_like(y), None
        self.w, self.k, self.kf = w, _taps(w), _taps(w[::-1, ::-1, ::-1])
        self.table = np.ascontiguousarray(_prefix_table(w).ravel(), dtype=np.float64)

    def run(self, it0, n, x_out, rows, ab=None) -> None:
        _lib.call("lsr_rl_dense_stats_f32_cpu", self.y.data_ptr(), self.cur.data_ptr(), self.ratio.data_ptr(),
                  *self.y.shape, self.k.ctypes.data, self.kf.ctypes.data, *self.w.shape, self.table.ctypes.data, n,
                  self.eps, rl_loop.row_ptr(rows, it0), None)

    def keep(self):
        return self.cur.clone()

    @property
    def held(self):
        import torch

        if self._held is None:
            self._held = torch.empty_like(self.cur)
        return self._held

    def turn(self):
        self.cur, self._held = self._held, self.cur
        return self.cur.clone()


def richardson_lucy(y, psf=None, iterations: int = 20, eps: float = 1e-6, x0=None, *, separable: str = "auto",
                    separable_rtol: float = 1e-6, psf_factors=None, tol: float | None = None,
                    return_stats: bool = False, tv_lambda: float = 0.0, tv_eps: float = 1e-6,
                    acceleration: str = "none"):
    """``deconvolve.richardson_lucy`` for a CPU tensor: ``x <- x * H^T(y / (H x + eps)) / H^T 1`` with the two
    correlations and their epilogues as the host twins of the device launches (rank-1 PSFs run the
    separable form, others the dense one).  ``tol`` / ``return_stats``: the iteration scalars of
    ``deconvolve.RLStats``, summed by the twins' UPDATE pass.  ``tol`` as the device plans read it
    (``shrimpy_amd.rl_loop.run``): the scalars of iteration i are looked at after iteration i + 1 has run, so the estimate
    returned is the one iteration PAST the first that met ``tol`` -- the same iterate, and the same
    ``RLStats.iterations``, whichever device the tensor lives on.  ``tv_lambda > 0``: every iteration is followed by the
    twin of the total-variation launch (``lsr_rl_tv_scale_f32_cpu``); ``change`` / ``total`` and ``tol`` are then those of
    the regularised iterate.  ``acceleration="biggs-andrews"``: every iteration but the last is followed by the twins of
    the two launches of ``csrc/rl_accel.hip`` and the next one starts from the extrapolated point (``RLStats.alphas``:
    the step lengths)."""
    import torch

    from .deconvolve import MAX_TAPS, MAX_Z_TAPS, factor_psf, prepare_psf

    y = _f32(y, "y")
    if separable not in ("auto", "force", "never"):
        raise ValueError("separable must be 'auto', 'force' or 'never'")
    req = rl_loop.check_run(y, iterations, eps, x0, None, return_stats, tol, tv_lambda, tv_eps, acceleration, _f32)
    factors = None
    if psf_factors is not None:
        factors = tuple(_taps(np.asarray(k).ravel()) for k in psf_factors)
        if (len(factors) != 3 or any(len(k) % 2 == 0 for k in factors) or len(factors[0]) > MAX_Z_TAPS
                or max(len(factors[1]), len(factors[2])) > MAX_TAPS):
            raise ValueError("psf_factors must be three odd-length 1-D kernels (<= 31 taps along z, <= 15 in plane)")
    else:
        # (up to the extents the device takes through the Fourier domain: the steppers take any count)
        from .deconvolve_fft import MAX_FFT_TAPS

        w = prepare_psf(psf, MAX_FFT_TAPS, MAX_FFT_TAPS)
        if separable != "never":
            factors = factor_psf(w, separable_rtol)
            if factors is None and separable == "force":
                raise ValueError("psf is not rank-1 within separable_rtol")

    def begin():
        _threads()
        x = req.init.clone()
        step = _SeparableStepper(y, x, factors, req.eps) if factors is not None else _DenseStepper(y, x, w, req.eps)
        return step, rl_loop.HostBackend(y.shape), None, lambda: torch.empty_like(y)

    res = rl_loop.run(req, begin)
    if res.stats is not None:
        res.stats.alphas = res.alphas
    return (res.x, res.stats) if return_stats else res.x
