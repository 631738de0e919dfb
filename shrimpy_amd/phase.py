"""Label-free 3-D phase reconstruction: a Tikhonov inverse filter applied in the Fourier domain.

The reference's label-free preprocessor runs ``flatfield -> deskew -> phase -> vs`` and hands the phase step to
waveorder (``shrimpy/preprocessing.py:254-282, 419-436``; parameters ``config/mda/mantis/dynatrack_demo.yaml:171-181``).
waveorder is not vendored and not installed: PARITY IS UNPINNED.  The model below is this package's own statement of the
step -- [RECALLED] where it follows waveorder's ``phase_thick_3d`` / ``optics`` from memory -- and ``tests/phase_ref.py``
restates it in float64 NumPy as the test oracle.

**Grid.**  A volume ``(Z, Y, X)`` is filtered on ``(gz, gy, gx)`` (:func:`phase_grid`): the smallest lengths the z-leg
kernel, hipFFT (5-smooth) and the row kernels take that hold ``Z + 2 z_padding``, ``Y`` and ``X``.

**Periodic mirror extension** (:func:`mirror_indices`), the same on every axis of ``n`` samples on ``g`` points: index
``i < n`` is sample ``i``; behind it, with ``a = i - n`` and ``b = g - 1 - i``, sample ``n - 1 - min(a, n - 1)`` if
``a <= b``, else sample ``min(b, n - 1)``.  The data sit at offset 0; on z with ``g - Z = 2 z_padding`` this is waveorder's
symmetric z padding seen through the grid's periodicity [RECALLED ``pad_zyx_along_z``].  The padded volume is never written.

**Transfer function** [RECALLED], float64 on the host, one z plane at a time (:func:`calculate_transfer_function`)::

    nu_r = hypot(fftfreq(gy, yx_pixel_size), fftfreq(gx, yx_pixel_size)),    lm = wavelength / n_media
    z_k  = ifftshift((arange(gz) - gz // 2) * z_pixel_size)                  (negated by invert_phase_contrast)
    S = [nu_r < NA_ill / wavelength],  P = [nu_r < NA_det / wavelength],  o = sqrt(max(1 - lm^2 nu_r^2, 0)) / lm on P
    A_k = fft2(S P exp(2 pi i z_k o)),   B_k = fft2(P (-i / 4 pi) exp(2 pi i z_k o) / (o + 1e-15))
    h_k = ifft2(conj(A_k) B_k) + ifft2(A_k conj(B_k))
    H   = fft_z(h * ifftshift(hanning(gz))) * z_pixel_size / sum(S |P|^2)

The Green's function ``B_k`` carries the SIGNED ``z_k``.  (With ``|z_k|`` there, the planes behind the focus add a
back-scattered term ``sin(4 pi |z| o) / (2 pi o)`` at ``nu = 0``: the transfer function then has a DC response of a third
of its peak and ``invert_phase_contrast`` no longer flips the sign of the result -- both of which the step's contract
requires, ``tests/test_phase_host.py``.)  ``conj(A) B + A conj(B)`` is real, so ``h_k`` and ``H`` are Hermitian and only
``kx <= gx / 2`` is ever computed or kept.  The imaginary-potential (absorption) function is not built.

**Filter.**  ``W = conj(H) / (|H|^2 + regularization_strength)``, made exactly Hermitian (``(W(k) + conj(W(-k))) / 2``), kept
on the device as complex64 in the ``[XC][Y][Z]`` layout ``lsr_spectrum_multiply_z_c64`` reads.

**Result.**  ``phase = crop(ifftn(fftn(ext(y)) W)) / mean(y)`` -- the filter of ``y / mean - 1``, since ``W(0) = 0`` and
the extension of a constant is constant.  A mean that is not positive and finite is a ``ValueError``.

One application on a HIP device is five launches (plus the one-workgroup reduction of the mean), none of which writes a
real-space volume but the result:

1. ``lsr_phase_rows_forward_c64``   mirror extension + real-to-complex x transform + transpose, the volume's float64 sum
2. hipFFT, batched, in place        y on all ``gz * XC`` rows (the padding is not zeros: no plane is skipped)
3. ``lsr_spectrum_multiply_z_c64``  z transform, product with ``W``, inverse z; only the volume's ``Z`` planes are stored
4. hipFFT                           y back on ``Z * XC`` rows
5. ``lsr_phase_rows_inverse_f32``   complex-to-real x transform, crop, ``1 / (gz gy gx mean)`` with the mean read on the device

CPU tensors take the same grid, extension and filter through ``torch.fft`` in complex64: a host route, never the oracle.
"""

from __future__ import annotations

import logging
import time

import numpy as np

from . import _lib
from .deconvolve_fft import _next_smooth

log = logging.getLogger(__name__)

__all__ = ["PhasePlan", "phase_grid", "mirror_indices", "calculate_transfer_function", "apply_inverse_transfer_function",
           "inverse_filter", "expand_half_spectrum"]

_MAX_GZ, _MAX_GX = 256, 4096      # csrc/zcorr.hip: kMaxN; csrc/phase.hip: 2 * kMaxM


def phase_grid(shape_zyx, z_padding: int = 0) -> tuple[int, int, int]:
    """The transform grid of a ``(Z, Y, X)`` volume: z 5-smooth and >= ``Z + 2 z_padding`` (at least 2), y 5-smooth, x a
    multiple of 4 whose half is 5-smooth (at least 8) -- the rules of ``deconvolve_fft.fft_grid``."""
    z, y, x = (int(v) for v in shape_zyx)
    if min(z, y, x) <= 0 or int(z_padding) < 0:
        raise ValueError(f"shape_zyx {tuple(shape_zyx)} must be positive and z_padding {z_padding} >= 0")
    return (_next_smooth(max(z + 2 * int(z_padding), 2)), _next_smooth(y), 4 * _next_smooth(max(-(-x // 4), 2)))


def _require_grid(shape, grid, device_type: str) -> None:
    gz, _, gx = grid
    ok = gz <= _MAX_GZ and gx <= _MAX_GX
    if ok and device_type == "cuda":
        from . import fft3

        ok = fft3.rows_supported(grid)
    if not ok:
        raise _lib.LsrUnsupported("PhasePlan", _lib.E_UNSUPPORTED,
                                  f"volume {tuple(shape)} needs the transform grid {tuple(grid)}: the kernels take at most "
                                  f"{_MAX_GZ} points along z and {_MAX_GX} along x (and hipFFT for the y leg)")


def mirror_indices(n: int, g: int) -> np.ndarray:
    """Source index of every point of a grid axis of ``g >= n`` points that holds ``n`` samples (module docstring)."""
    n, g = int(n), int(g)
    if not 0 < n <= g:
        raise ValueError(f"an axis of {n} samples does not fit a grid of {g}")
    i = np.arange(g)
    a, b = i - n, g - 1 - i
    return np.where(i < n, i, np.where(a <= b, n - 1 - np.minimum(a, n - 1), np.minimum(b, n - 1))).astype(np.int64)


# ---- transfer function and filter (host, float64) -----------------------------------------------------------------------


def _half_transfer_function(grid, yx_pixel_size, z_pixel_size, wavelength_illumination, index_of_refraction_media,
                            numerical_aperture_illumination, numerical_aperture_detection, invert_phase_contrast=False):
    """``H[kz, ky, kx]``, ``kx <= gx / 2``, complex128 (the module docstring's formulas; one z plane at a time, then the z
    transform a slab of rows at a time: beside the result itself nothing larger than a few planes is alive)."""
    gz, gy, gx = (int(v) for v in grid)
    xc = gx // 2 + 1
    lam, dz = float(wavelength_illumination), float(z_pixel_size)
    nu_r = np.hypot(np.fft.fftfreq(gy, float(yx_pixel_size))[:, None], np.fft.fftfreq(gx, float(yx_pixel_size))[None, :])
    lm = lam / float(index_of_refraction_media)
    source = nu_r < float(numerical_aperture_illumination) / lam
    pupil = nu_r < float(numerical_aperture_detection) / lam
    oblique = np.where(pupil, np.sqrt(np.maximum(1.0 - lm * lm * nu_r * nu_r, 0.0)) / lm, 0.0)
    z_k = np.fft.ifftshift((np.arange(gz) - gz // 2) * dz)
    if invert_phase_contrast:
        z_k = -z_k
    window = np.fft.ifftshift(np.hanning(gz))
    direct = float(np.sum(source & pupil))        # sum S |P|^2
    if not direct > 0:
        raise ValueError("the illumination aperture holds no point of the frequency grid: the volume is too small in y, x "
                         "for these optics")
    illum = (source & pupil).astype(np.float64)
    green = np.where(pupil, (-1j / (4.0 * np.pi)) / (oblique + 1e-15), 0.0)
    h = np.zeros((gz, gy, xc), dtype=np.complex128)
    told = time.monotonic()
    for k in range(gz):
        if window[k] == 0.0:
            continue
        if time.monotonic() - told > 30.0:     # a full-size grid takes minutes: about a second per plane
            told = time.monotonic()
            log.info("phase transfer function: plane %d of %d", k, gz)
        prop = np.exp(2j * np.pi * z_k[k] * oblique)
        a = np.fft.fft2(illum * prop)
        b = np.fft.fft2(green * prop)
        # ifft2(conj(A) B) + ifft2(A conj(B)) = ifft2 of a real array: Hermitian, its half is conj(rfft2) / (gy gx)
        real = 2.0 * (a.real * b.real + a.imag * b.imag)
        h[k] = np.conj(np.fft.rfft2(real)) * (window[k] * dz / (direct * gy * gx))
    rows = max(1, (1 << 22) // (gz * xc))
    for y0 in range(0, gy, rows):
        h[:, y0:y0 + rows] = np.fft.fft(h[:, y0:y0 + rows], axis=0)
    return h


def calculate_transfer_function(zyx_shape, yx_pixel_size, z_pixel_size, wavelength_illumination, z_padding,
                                index_of_refraction_media, numerical_aperture_illumination,
                                numerical_aperture_detection, invert_phase_contrast=False):
    """The reference's call shape (``shrimpy/preprocessing.py:264-270``): ``(real_potential_tf, None)``.

    ``real_potential_tf``: a complex128 CPU tensor ``(gz, gy, gx // 2 + 1)`` on :func:`phase_grid` of ``zyx_shape`` -- the
    half ``kx <= gx / 2`` of a Hermitian function (:func:`expand_half_spectrum` gives the rest).  The second entry, the
    imaginary-potential function, is not built."""
    import torch

    grid = phase_grid(zyx_shape, z_padding)
    _require_grid(zyx_shape, grid, "cpu")
    h = _half_transfer_function(grid, yx_pixel_size, z_pixel_size, wavelength_illumination, index_of_refraction_media,
                                numerical_aperture_illumination, numerical_aperture_detection, invert_phase_contrast)
    return torch.from_numpy(h), None


def expand_half_spectrum(half, gx: int) -> np.ndarray:
    """``(gz, gy, gx)`` from the ``kx <= gx / 2`` half of a Hermitian function: ``F(k) = conj(F(-k))``."""
    half = np.asarray(half)
    gz, gy, xc = half.shape
    if xc != int(gx) // 2 + 1:
        raise ValueError(f"a half spectrum of {xc} columns does not belong to gx = {gx}")
    full = np.empty((gz, gy, int(gx)), dtype=half.dtype)
    full[:, :, :xc] = half
    kz, ky = (-np.arange(gz)) % gz, (-np.arange(gy)) % gy
    for kx in range(xc, int(gx)):
        full[:, :, kx] = np.conj(half[kz][:, ky, int(gx) - kx])
    return full


def inverse_filter(half_tf, regularization_strength: float, gx: int) -> np.ndarray:
    """``W = conj(H) / (|H|^2 + regularization_strength)`` made Hermitian, from the half ``H`` :func:`calculate_transfer_function`
    returns: complex64 ``(XC, gy, gz)``, the layout of the z-leg kernel.  (Columns ``0 < kx < gx / 2`` have their partner
    in the half that is not kept; ``kx = 0`` and ``kx = gx / 2`` are their own partners' columns and are averaged here.)"""
    h = np.asarray(half_tf)
    gz, gy, xc = h.shape
    if xc != int(gx) // 2 + 1 or int(gx) % 2:
        raise ValueError(f"a half spectrum of {xc} columns does not belong to an even gx = {gx}")
    reg = float(regularization_strength)
    if not (reg > 0 and np.isfinite(reg)):
        raise ValueError("regularization_strength must be positive and finite")
    out = np.empty((xc, gy, gz), dtype=np.complex64)
    kz, ky = (-np.arange(gz)) % gz, (-np.arange(gy)) % gy
    cols = max(1, (1 << 22) // (gz * gy))
    for x0 in range(0, xc, cols):
        s = h[:, :, x0:x0 + cols]
        w = np.conj(s) / (s.real * s.real + s.imag * s.imag + reg)
        for kx in (0, xc - 1):
            if x0 <= kx < x0 + w.shape[2]:
                c = w[:, :, kx - x0]
                w[:, :, kx - x0] = 0.5 * (c + np.conj(c[kz][:, ky]))
        out[x0:x0 + cols] = w.transpose(2, 1, 0)
    return out


# ---- the plan -----------------------------------------------------------------------------------------------------------


class PhasePlan:
    """The filter and the scratch of one (volume shape, :class:`~shrimpy_amd.settings.PhaseSettings`, device).

    ``plan(volume, out=None)`` returns the phase volume: float32, the volume's shape, on its device.  The filter is computed
    at construction (``seconds`` holds the time): that is the warm-up.  ``release()`` drops the scratch, not the filter.
    ``last_mean``: the mean the last call divided by."""

    def __init__(self, shape_zyx, settings, device):
        from .settings import PhaseSettings

        if not isinstance(settings, PhaseSettings):
            settings = PhaseSettings(**settings)
        self.settings = settings
        self._setup(shape_zyx, settings.transfer_function.z_padding, settings.apply_inverse.regularization_strength, device)

    @classmethod
    def from_transfer_function(cls, shape_zyx, half_tf, z_padding, regularization_strength, device):
        """A plan around a transfer function that exists already (what :func:`calculate_transfer_function` returned for
        this shape and ``z_padding``)."""
        self = cls.__new__(cls)
        self.settings = None
        self._setup(shape_zyx, z_padding, regularization_strength, device, half_tf)
        return self

    def _setup(self, shape_zyx, z_padding, regularization_strength, device, half_tf=None) -> None:
        import torch

        self.device = torch.device(device)
        self.shape = tuple(int(v) for v in shape_zyx)
        if len(self.shape) != 3 or min(self.shape) <= 0:
            raise ValueError(f"shape_zyx must be three positive ints, got {self.shape}")
        self.grid = phase_grid(self.shape, z_padding)
        _require_grid(self.shape, self.grid, self.device.type)
        gz, gy, gx = self.grid
        self._xc = gx // 2 + 1
        started = time.monotonic()
        if half_tf is None:
            kw = self.settings.transfer_function.model_dump()
            kw.pop("z_padding")
            half_tf = _half_transfer_function(self.grid, **kw)
        elif tuple(half_tf.shape) != (gz, gy, self._xc):
            raise ValueError(f"the transfer function is {tuple(half_tf.shape)}; a {self.shape} volume with z_padding "
                             f"{z_padding} needs {(gz, gy, self._xc)}")
        w = inverse_filter(np.asarray(half_tf), regularization_strength, gx)
        del half_tf
        self._filter = torch.from_numpy(w).to(self.device)       # [XC][Y][Z] complex64
        self.seconds = time.monotonic() - started
        self._index = tuple(torch.from_numpy(mirror_indices(n, g)) for n, g in zip(self.shape, self.grid))
        if self.device.type == "cuda":
            from . import fft3

            self._half, self._full = fft3._row_twiddles(gx, self.device)
            self._tw_z = fft3._twiddle_table(gz, self.device)
        self._b = self._partial = self._mean = None
        self.last_mean = None

    def release(self) -> None:
        self._b = self._partial = None

    def __call__(self, volume, out=None):
        import torch

        if not isinstance(volume, torch.Tensor):
            raise TypeError(f"volume must be a torch.Tensor, got {type(volume).__name__}")
        if tuple(volume.shape) != self.shape or volume.device.type != self.device.type or (
                self.device.index is not None and volume.device != self.device):
            raise ValueError(f"volume must be {self.shape} on {self.device}, got {tuple(volume.shape)} on {volume.device}")
        volume = volume.to(torch.float32).contiguous()
        if out is None:
            out = torch.empty(self.shape, dtype=torch.float32, device=volume.device)
        elif (tuple(out.shape) != self.shape or out.dtype != torch.float32 or out.device != volume.device
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 {self.shape} tensor on {volume.device}")
        if out.data_ptr() == volume.data_ptr():
            raise ValueError("out must not alias the volume")
        mean = self._apply_device(volume, out) if self.device.type == "cuda" else self._apply_host(volume, out)
        self.last_mean = mean
        if not (mean > 0 and np.isfinite(mean)):
            raise ValueError(f"the volume's mean is {mean}: phase reconstruction divides by it, it must be positive and finite")
        _lib.mark_written(out)
        return out

    def _apply_device(self, volume, out) -> float:
        import torch

        from . import fft3

        gz, gy, gx = self.grid
        z, y, x = self.shape
        dev = volume.device
        with torch.cuda.device(dev):
            if self._b is None:
                self._b = torch.empty((gz, self._xc, gy), dtype=torch.complex64, device=dev)
                self._partial = torch.empty((_lib.call_value("lsr_phase_rows_scratch_bytes", gz, gy) // 8,),
                                            dtype=torch.float64, device=dev)
            if self._mean is None:
                self._mean = torch.zeros((2,), dtype=torch.float64, device=dev)
            b, stream = self._b, _lib.stream_ptr(dev)
            _lib.call("lsr_phase_rows_forward_c64", volume.data_ptr(), z, y, x, b.data_ptr(), gz, gy, gx,
                      self._half.data_ptr(), self._full.data_ptr(), self._partial.data_ptr(), self._mean.data_ptr(), stream)
            fft3._exec(dev, fft3._HIPFFT_C2C, gy, gz * self._xc, b.data_ptr(), b.data_ptr(), fft3._FORWARD)
            _lib.call("lsr_spectrum_multiply_z_c64", self._filter.data_ptr(), b.data_ptr(), self._tw_z.data_ptr(), gz, gy,
                      self._xc, 0, gz, z, stream)
            fft3._exec(dev, fft3._HIPFFT_C2C, gy, z * self._xc, b.data_ptr(), b.data_ptr(), fft3._BACKWARD)
            _lib.call("lsr_phase_rows_inverse_f32", b.data_ptr(), gz, gy, gx, self._half.data_ptr(), self._full.data_ptr(),
                      self._mean.data_ptr(), out.data_ptr(), z, y, x, stream)
            # the one wait of a call, behind all of its launches: a mean that cannot be divided by is an error
            return float(self._mean[0].item())

    def _apply_host(self, volume, out) -> float:
        """The host route: ``torch.fft`` in complex64 on the extended volume (which this route does write)."""
        import torch

        gz, gy, gx = self.grid
        z, y, x = self.shape
        mean = float(volume.to(torch.float64).mean().item())
        if not (mean > 0 and np.isfinite(mean)):
            return mean
        iz, iy, ix = self._index
        ext = volume[iz][:, iy][:, :, ix]
        spec = torch.fft.rfftn(ext) * self._filter.permute(2, 1, 0)
        out.copy_(torch.fft.irfftn(spec, s=(gz, gy, gx))[:z, :y, :x] / mean)
        return mean


_plans: dict = {}


def apply_inverse_transfer_function(zyx_data, real_potential_transfer_function, imaginary_potential_transfer_function=None,
                                    z_padding: int = 0, reconstruction_algorithm: str = "Tikhonov",
                                    regularization_strength: float = 1e-3):
    """The reference's call shape (``shrimpy/preprocessing.py:428-435``): the phase of ``zyx_data`` (a float32 tensor, on
    its device) from the transfer function :func:`calculate_transfer_function` returned for its shape and ``z_padding``.
    The filter made from a transfer function is kept for the next call with the same one."""
    if reconstruction_algorithm != "Tikhonov":
        raise NotImplementedError(f"reconstruction_algorithm {reconstruction_algorithm!r}: only 'Tikhonov' is built")
    if imaginary_potential_transfer_function is not None:
        raise NotImplementedError("the imaginary-potential (absorption) transfer function is not built")
    tf = real_potential_transfer_function
    key = (id(tf), tuple(zyx_data.shape), str(zyx_data.device), int(z_padding), float(regularization_strength))
    hit = _plans.get(key)
    if hit is None or hit[0] is not tf:
        half = tf.numpy() if hasattr(tf, "numpy") else np.asarray(tf)
        _plans.clear()
        hit = _plans[key] = (tf, PhasePlan.from_transfer_function(tuple(zyx_data.shape), half, int(z_padding),
                                                                  float(regularization_strength), zyx_data.device))
    return hit[1](zyx_data)
