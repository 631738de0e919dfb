"""Float64 NumPy restatement of the phase reconstruction (``shrimpy_amd/phase.py``): the test oracle.

waveorder is not installed and not vendored, so PARITY IS UNPINNED: this file states the model -- grid, periodic mirror
extension by explicit index arrays, transfer function on the FULL frequency grid exactly as the formulas read (both
``ifft2`` products, no symmetry used), the Tikhonov filter made Hermitian, ``fftn`` / ``ifftn``, crop -- and the package's
host and device routes are held against it.  Nothing here imports the package.
"""

from __future__ import annotations

import numpy as np

# the reference's ``phase:`` block (``config/mda/mantis/dynatrack_demo.yaml:171-181``) with the pixel sizes its caller injects
YAML_OPTICS = dict(wavelength_illumination=0.450, index_of_refraction_media=1.4, numerical_aperture_detection=1.35,
                   numerical_aperture_illumination=0.52, yx_pixel_size=0.1133, z_pixel_size=0.17)
YAML_REGULARIZATION = 0.01

# (shape, z_padding): the cases of tests/test_phase_gpu.py, shared with the host route's test
CASES = [((5, 6, 10), 2), ((7, 9, 13), 0), ((3, 4, 8), 5), ((6, 10, 16), 1), ((24, 40, 72), 5)]


def _smooth(n: int) -> int:
    while True:
        m = n
        for f in (2, 3, 5):
            while m % f == 0:
                m //= f
        if m == 1:
            return n
        n += 1


def grid(shape_zyx, z_padding: int):
    """z: 5-smooth >= Z + 2 z_padding (and >= 2); y: 5-smooth >= Y; x: a multiple of 4 >= max(X, 8) whose half is 5-smooth."""
    z, y, x = shape_zyx
    gx = max(x, 8)
    while gx % 4 or _smooth(gx // 2) != gx // 2:
        gx += 1
    return _smooth(max(z + 2 * z_padding, 2)), _smooth(y), gx


def mirror_table(n: int, g: int) -> list[int]:
    out = []
    for i in range(g):
        if i < n:
            out.append(i)
            continue
        a, b = i - n, g - 1 - i
        out.append(n - 1 - min(a, n - 1) if a <= b else min(b, n - 1))
    return out


def extend(volume, grid_zyx):
    v = np.asarray(volume, dtype=np.float64)
    iz, iy, ix = (np.array(mirror_table(n, g)) for n, g in zip(v.shape, grid_zyx))
    return v[iz][:, iy][:, :, ix]


def transfer_function(grid_zyx, wavelength_illumination, index_of_refraction_media, numerical_aperture_detection,
                      numerical_aperture_illumination, yx_pixel_size, z_pixel_size, invert_phase_contrast=False):
    """``(H, nu_r)``: the real-potential transfer function on the full grid, complex128, and the radial frequencies."""
    gz, gy, gx = grid_zyx
    lam = wavelength_illumination
    nu_r = np.hypot(np.fft.fftfreq(gy, yx_pixel_size)[:, None], np.fft.fftfreq(gx, yx_pixel_size)[None, :])
    lm = lam / index_of_refraction_media
    z_k = np.fft.ifftshift((np.arange(gz) - gz // 2) * z_pixel_size)
    if invert_phase_contrast:
        z_k = -z_k
    s = (nu_r < numerical_aperture_illumination / lam).astype(np.float64)
    p = (nu_r < numerical_aperture_detection / lam).astype(np.float64)
    o = np.sqrt(np.maximum(1.0 - lm ** 2 * nu_r ** 2, 0.0)) / lm * p
    h1 = np.zeros(grid_zyx, dtype=np.complex128)
    h2 = np.zeros(grid_zyx, dtype=np.complex128)
    for k in range(gz):
        a = np.fft.fft2(s * p * np.exp(2j * np.pi * z_k[k] * o))
        b = np.fft.fft2(p * (-1j / (4 * np.pi)) * np.exp(2j * np.pi * z_k[k] * o) / (o + 1e-15))     # signed z_k
        h1[k] = np.fft.ifft2(np.conj(a) * b)
        h2[k] = np.fft.ifft2(a * np.conj(b))
    w = np.fft.ifftshift(np.hanning(gz))[:, None, None]
    big_h1 = np.fft.fft(h1 * w, axis=0) * z_pixel_size
    big_h2 = np.fft.fft(h2 * w, axis=0) * z_pixel_size
    return (big_h1 + big_h2) / np.sum(s * p * p), nu_r


def negated(a):
    """``a(-k)`` on a periodic grid."""
    for axis in range(a.ndim):
        a = np.roll(np.flip(a, axis), 1, axis)
    return a


def inverse_filter(h, regularization_strength: float):
    w = np.conj(h) / (np.abs(h) ** 2 + regularization_strength)
    return 0.5 * (w + np.conj(negated(w)))


def reconstruct(volume, z_padding: int, regularization_strength: float = YAML_REGULARIZATION, **optics):
    """float64 ``(Z, Y, X)``: ``crop(ifftn(fftn(ext(y)) W)) / mean(y)``."""
    v = np.asarray(volume, dtype=np.float64)
    g = grid(v.shape, z_padding)
    h, _ = transfer_function(g, **optics)
    w = inverse_filter(h, regularization_strength)
    m = v.mean()
    if not (m > 0 and np.isfinite(m)):
        raise ValueError("mean")
    full = np.fft.ifftn(np.fft.fftn(extend(v, g)) * w)
    z, y, x = v.shape
    return full.real[:z, :y, :x] / m


_cache: dict = {}


def case(index: int, invert: bool = False):
    """``(volume float32, settings dict, reference float64)`` of ``CASES[index]``, computed once per session."""
    key = (index, invert)
    if key not in _cache:
        shape, pad = CASES[index]
        vol = np.random.default_rng(100 + index).uniform(80, 600, shape).astype(np.float32)
        optics = dict(YAML_OPTICS, invert_phase_contrast=invert)
        settings = dict(transfer_function=dict(optics, z_padding=pad),
                        apply_inverse=dict(reconstruction_algorithm="Tikhonov", regularization_strength=YAML_REGULARIZATION))
        ref = reconstruct(vol, pad, YAML_REGULARIZATION, **optics)
        ref.setflags(write=False)
        vol.setflags(write=False)
        _cache[key] = (vol, settings, ref)
    return _cache[key]


def rel_err(got, ref) -> float:
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / np.max(np.abs(ref)))
