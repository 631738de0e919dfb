"""float64 restatement of accelerated Richardson-Lucy (Biggs & Andrews 1997; ``csrc/rl_accel.hip``) over
``oracle.cpu_ref.rl_iteration_f64`` and the shared cases of its tests (``tests/test_rl_accel_host.py`` for the host twins,
``tests/test_rl_accel_gpu.py`` for the kernels).  Not a test module.

    p_0 = x_0
    for k = 0 .. K-1:
        x_{k+1} = RL(p_k);  stop after the last one
        g_k     = x_{k+1} - p_k
        a_{k+1} = 0 for k == 0, else clamp(<g_k, g_{k-1}> / <g_{k-1}, g_{k-1}>, 0, 1), 0 for a zero denominator
        p_{k+1} = max(x_{k+1} + a_{k+1} (x_{k+1} - x_k), 0)
    return x_K
"""
import numpy as np

from oracle import cpu_ref as o
from tests import rl_tv_ref

SHAPES = rl_tv_ref.SHAPES
framed = rl_tv_ref.framed
EPS = 1e-6


def accelerated_f64(y, iterations, psf=None, factors=None, x0=None, eps=EPS):
    """``(x_K, [a_1 .. a_{K-1}], number of voxels the ``max(., 0)`` changed over the run)`` in float64 from float32 ``y``
    (``x0 = y`` unless given)."""
    y = np.asarray(y, np.float32)
    x = p = np.asarray(y if x0 is None else x0, np.float64)
    g_prev, alphas, xs, clamped = None, [], [], 0
    for k in range(iterations):
        x1 = o.rl_iteration_f64(p, y, psf=psf, factors=factors, eps=eps)[2]
        xs.append(x1)
        if k + 1 == iterations:
            break
        g = x1 - p
        a = 0.0
        if g_prev is not None:
            den = float((g_prev * g_prev).sum())
            a = 0.0 if den == 0.0 else min(max(float((g * g_prev).sum()) / den, 0.0), 1.0)
        alphas.append(a)
        p = x1 + a * (x1 - x)
        clamped += int((p < 0).sum())
        p = np.maximum(p, 0.0)
        x, g_prev = x1, g
    return xs[-1] if xs else x, np.array(alphas), clamped


def plain_f64(y, iterations, psf=None, factors=None, eps=EPS):
    x = np.asarray(y, np.float64)
    for _ in range(iterations):
        x = o.rl_iteration_f64(x, np.asarray(y, np.float32), psf=psf, factors=factors, eps=eps)[2]
    return x


def log_likelihood(x, d, psf, eps=EPS):
    """Poisson log-likelihood ``sum d log(H x + eps) - (H x + eps)`` in float64 (``H`` = convolution, zeros outside)."""
    from scipy import ndimage

    hx = ndimage.convolve(np.asarray(x, np.float64), np.asarray(psf, np.float64), mode="constant", cval=0.0) + float(np.float32(eps))
    return float((np.asarray(d, np.float64) * np.log(hx) - hx).sum())


def gaussian_factors(shape=(9, 7, 7), sigma=(2.0, 1.2, 1.2)):
    ks = []
    for n, s in zip(shape, sigma):
        k = np.exp(-0.5 * ((np.arange(n) - n // 2) / s) ** 2)
        ks.append((k / k.sum()).astype(np.float32))
    return ks


def rotated_psf(shape=(9, 7, 7), sigma=(2.0, 1.2, 1.2), degrees=30.0):
    """The Gaussian above turned by ``degrees`` in the (z, x) plane (a tilted light sheet): ``ky (x) kzx``, sum 1."""
    zz, yy, xx = np.meshgrid(*[np.arange(n) - n // 2 for n in shape], indexing="ij")
    c, s = np.cos(np.deg2rad(degrees)), np.sin(np.deg2rad(degrees))
    zr, xr = c * zz + s * xx, -s * zz + c * xx
    w = np.exp(-0.5 * ((zr / sigma[0]) ** 2 + (yy / sigma[1]) ** 2 + (xr / sigma[2]) ** 2))
    return (w / w.sum()).astype(np.float32)


def outer(ks):
    return (ks[0][:, None, None].astype(np.float64) * ks[1][None, :, None] * ks[2][None, None, :]).astype(np.float32)


def scene(shape=(40, 48, 56), seed=2007, density=2e-4):
    """``{name: (d, psf, plan keywords)}``: the bead scene blurred by the separable Gaussian and by its rotated form."""
    ks = gaussian_factors()
    sep, rot = outer(ks), rotated_psf()
    return {"separable": (o.bead_scene(shape, seed, sep, density=density), sep, dict(psf_factors=ks)),
            "rotated": (o.bead_scene(shape, seed, rot, density=density), rot, dict(psf=rot))}


def _strided(t):
    z, y, x = (int(n) for n in t.shape)
    assert x == 1 or t.stride(2) == 1
    return [t.data_ptr(), t.stride(1), t.stride(0)]


def _run(name, device, args):
    from shrimpy_amd import _lib

    if device.type == "cpu":
        _lib.call(name + "_cpu", *args)
    else:
        import torch

        with torch.cuda.device(device):
            _lib.call(name, *args, _lib.stream_ptr(device))


def dots_call(x1, p, g, first, dots2):
    """``lsr_rl_accel_dots_f32`` (device tensors) or its twin (CPU tensors): ``x1``, ``p`` float32 tensors or views of
    (Z, Y, X) with unit x stride, ``g`` dense, ``dots2`` a float64 tensor of two elements on the same device."""
    import torch

    from shrimpy_amd import _lib

    z, y, x = (int(n) for n in x1.shape)
    assert g.is_contiguous() and tuple(g.shape) == (z, y, x) and tuple(p.shape) == (z, y, x)
    work = torch.empty(_lib.call_value("lsr_rl_accel_workspace_bytes", z, y, x) // 8, dtype=torch.float64, device=x1.device)
    _run("lsr_rl_accel_dots_f32", x1.device, _strided(x1) + _strided(p) + [g.data_ptr(), z, y, x, int(first), dots2.data_ptr(),
                                                                          work.data_ptr()])
    return g, dots2


def predict_call(x1, x0, num=None, den=None, alpha=None):
    """``lsr_rl_accel_predict_f32`` or its twin: p_{k+1} over ``x0`` in place; ``num`` / ``den`` / ``alpha`` one-element
    float64 tensors on the same device (``den=None``: the first step)."""
    z, y, x = (int(n) for n in x1.shape)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    _run("lsr_rl_accel_predict_f32", x1.device, _strided(x1) + _strided(x0) + [z, y, x, ptr(num), ptr(den), ptr(alpha)])
    return x0


def f32_ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)

