"""float64 restatement of the total-variation factor of an RL-TV iteration (``csrc/rl_tv.hip``) and the shared cases of
its tests (``tests/test_rl_tv_host.py`` for the host twin, ``tests/test_rl_tv_gpu.py`` for the kernel).  Not a test module.

    D_a u(r) = u(r + e_a) - u(r)            0 where r + e_a is outside the volume
    n        = sqrt(D_z^2 + D_y^2 + D_x^2 + tv_eps^2),   p_a = D_a u / n
    div(r)   = sum_a p_a(r) - p_a(r - e_a)  p_a(r - e_a) := 0 where r - e_a is outside
    out      = v / (1 - lambda * div)
"""
import numpy as np

LAMBDAS = (0.002, 0.02, 0.1, 0.16)
TILE = (16, 64)          # rows x columns of the kernel's tile (csrc/rl_tv.hip)
# (Z, Y, X): smaller than one tile; ragged in rows and columns; each degenerate axis alone; a few tiles each way
SHAPES = [(5, 7, 9), (6, 21, 71), (1, 19, 70), (9, 1, 70), (9, 19, 1), (19, 70, 150)]


def ceiling(lam):
    """The a-priori bound on C (units of 2^-24 * ref) at this lambda: see ``test_rl_tv_gpu.py``'s docstring."""
    return 4.0 + 80.0 * lam / (1.0 - 6.0 * lam)


def _forward(u, axis):
    d = np.zeros_like(u)
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[axis], hi[axis] = slice(0, -1), slice(1, None)
    d[tuple(lo)] = u[tuple(hi)] - u[tuple(lo)]
    return d


def divergence_of_normalised_gradient(u, tv_eps=1e-6):
    u = np.asarray(u, np.float64)
    d = [_forward(u, a) for a in range(3)]
    n = np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2 + float(tv_eps) ** 2)
    div = np.zeros_like(u)
    for a in range(3):
        p = d[a] / n
        div += p
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[a], lo[a] = slice(1, None), slice(0, -1)
        div[tuple(hi)] -= p[tuple(lo)]
    return div


def tv_scale(u, v, lam, tv_eps=1e-6):
    """``v / (1 - lam * div(grad u / |grad u|))`` in float64."""
    return np.asarray(v, np.float64) / (1.0 - float(lam) * divergence_of_normalised_gradient(u, tv_eps))


def total_variation(u):
    u = np.asarray(u, np.float64)
    return float(np.sqrt(sum(_forward(u, a) ** 2 for a in range(3))).sum())


def tv_call(u, v, out, lam, tv_eps=1e-6, stats=None):
    """``lsr_rl_tv_scale_f32`` (device tensors) or its host twin (CPU tensors) on float32 torch tensors or views of
    (Z, Y, X) with unit x stride; ``stats``: a float64 tensor of two elements the call adds to."""
    import ctypes

    from shrimpy_amd import _lib

    z, y, x = (int(n) for n in u.shape)
    args = []
    for t in (u, v, out):
        assert tuple(t.shape) == (z, y, x) and (x == 1 or t.stride(2) == 1)
        args += [t.data_ptr(), t.stride(1), t.stride(0)]
    args += [z, y, x, ctypes.c_float(lam), ctypes.c_float(tv_eps), None if stats is None else stats.data_ptr()]
    if u.device.type == "cpu":
        _lib.call("lsr_rl_tv_scale_f32_cpu", *args)
    else:
        import torch

        with torch.cuda.device(u.device):
            _lib.call("lsr_rl_tv_scale_f32", *args, _lib.stream_ptr(u.device))
    return out


def framed(a, device, fill=float("nan"), margin=(2, 3, 5)):
    """A copy of ``a`` as the interior view of a larger allocation filled with ``fill`` (rows and planes strided as
    those of a padded working volume; NaN around it shows any read outside the logical volume)."""
    import torch

    z, y, x = a.shape
    mz, my, mx = margin
    full = torch.full((z + mz, y + 2 * my, x + 2 * mx), fill, dtype=torch.float32, device=device)
    view = full[:z, my:my + y, mx:mx + x]
    view.copy_(torch.as_tensor(a))
    return full, view
