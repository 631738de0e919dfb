"""NumPy / float64 restatement of the per-bead Gaussian fit and of the Fourier-shifted PSF average (``shrimpy_amd/psf.py``:
``fit_beads``, ``average_psf_aligned``; ``csrc/psf_fit.hpp``, ``csrc/psf_fit.hip``), and the synthetic scenes of
``tests/test_psf_fit_host.py`` / ``tests/test_psf_fit_gpu.py``.  PARITY UNPINNED, as ``tests/psf_ref.py``.

The fit.  ``m(r) = B + A exp(-(r - mu)^T W (r - mu) / 2)`` on the patch, ``r`` the voxel offset from the centre voxel,
``theta = (B, A, mu_z, mu_y, mu_x, w_zz, w_yy, w_xx, w_zy, w_zx, w_yx)``, unweighted least squares by Levenberg-Marquardt:

    start     B0 = mean of the six faces, A0 = d(0) - B0 (A0 <= 0: status 4), g = max(d - B0 - A0 / 2, 0),
              mu0 = sum(g r) / sum(g), var_i = sum(g r_i^2) / sum(g) - mu0_i^2, W0 = diag(c / max(var_i, c / 4)),
              c = HALF_MAX_MOMENT (the second moment per axis of a unit Gaussian cut at its half maximum)
    sums      J^T J, J^T r, cost = sum(res^2) at theta, res = d - m
    solve     (D^-1 J^T J D^-1 + lambda I) y = D^-1 J^T r by Cholesky, D = sqrt(diag(J^T J)); trial = theta + D^-1 y
              (a diagonal entry or a pivot that is not positive: status 2)
    judge     trial cost <= cost: theta = trial, lambda / 10 (not below 1e-15); otherwise lambda * 10, solve again;
              converged when max |trial mu - mu| < 1e-9 and |cost - trial cost| <= 1e-12 cost, accepted or not;
              otherwise status 1 after ``max_iter`` trial costs
    finish    converged: W not positive definite -> 2, some |mu_i| >= 1 -> 3, A <= 0 -> 4; NaN unless the status is 0

``reverse=True`` takes every sum over the voxels in the opposite order: the difference between the two runs is the fit's
sensitivity to the order of the sums (and of that size: to the rounding of ``exp``) and gives the bound the kernel and
the twin are held to, ``fit_tolerance``: 16 times the largest ``|delta| / max(|theta|, 1)`` over the parameters of the
status-0 beads of the test scenes, at least 1e-9.  Measured on the scenes below: 1.6e-14 (scene A), 2.0e-16 (scene B) --
so the floor of 1e-9 is the bound in force on every case.  Against the truth of scene A the restatement is off by at most
1.8e-8 voxel in a centre and 1.0e-8 relative in a principal sigma (bound 1e-5: the float32 rounding of the samples is 6e-8
relative) and needs 17 to 27 iterations over all the cases (the limit set for it: 30).

The shifted average.  Per bead ``c = double(patch) - B``, then along x, y, z ``out[i] = sum_j c[j] w[(i - j) mod N]`` with
``j`` ascending as separate multiplications and additions; ``out / S`` is added over the beads in list order and divided
by their number.  ``B`` and ``S`` are inputs here (the kernel's own, ``bead_stats``), as the weights are.
"""

import math

import numpy as np

_A = math.sqrt(2.0 * math.log(2.0))
_G = math.sqrt(math.pi / 2.0) * math.erf(_A / math.sqrt(2.0))
HALF_MAX_MOMENT = (3.0 * (_G - _A / 2.0) - _A ** 3 / 2.0 - _A ** 5 / 10.0) / (_G - _A / 2.0 - _A ** 3 / 6.0) / 3.0
FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))
PAIRS = [(i, j) for i in range(11) for j in range(i + 1)]


def shell_mask(shape):
    m = np.ones(shape, dtype=bool)
    if min(shape) > 2:
        m[1:-1, 1:-1, 1:-1] = False
    return m


def _offsets(shape):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) - n // 2 for n in shape], indexing="ij")
    return [a.ravel() for a in g]


def _model(t, rz, ry, rx):
    dz, dy, dx = rz - t[2], ry - t[3], rx - t[4]
    uz = t[5] * dz + t[8] * dy + t[9] * dx
    uy = t[8] * dz + t[6] * dy + t[10] * dx
    ux = t[9] * dz + t[10] * dy + t[7] * dx
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-0.5 * (dz * uz + dy * uy + dx * ux))
    return e, (dz, dy, dx), (uz, uy, ux)


def fit_patch(patch, max_iter=100, reverse=False):
    """``(theta12, status, evaluations)`` of one patch (any float array, widened to float64)."""
    d = np.asarray(patch, dtype=np.float64)
    nan12 = np.full(12, np.nan)
    if not np.isfinite(d).all():
        return nan12, 5, 0
    step = -1 if reverse else 1

    def total(a):
        return a[::step].sum(axis=0)

    rz, ry, rx = _offsets(d.shape)
    bg = d[shell_mask(d.shape)].mean()
    amp = d[tuple(n // 2 for n in d.shape)] - bg
    v = d.ravel()
    g = np.clip(v - (bg + 0.5 * amp), 0.0, None)
    m0 = total(g)
    if not amp > 0 or not m0 > 0:
        return nan12, 4, 0
    t = np.zeros(11)
    t[0], t[1] = bg, amp
    for i, r in enumerate((rz, ry, rx)):
        mu = total(g * r) / m0
        var = total(g * r * r) / m0 - mu * mu
        t[2 + i], t[5 + i] = mu, HALF_MAX_MOMENT / max(var, 0.25 * HALF_MAX_MOMENT)

    def cost_of(q):
        e, _, _ = _model(q, rz, ry, rx)
        res = v - (q[0] + q[1] * e)
        return total(res * res)

    lam, evals, status, need_sums = 1e-3, 0, 0, True
    with np.errstate(all="ignore"):
        while True:
            if need_sums:
                e, (dz, dy, dx), (uz, uy, ux) = _model(t, rz, ry, rx)
                res = v - (t[0] + t[1] * e)
                ae = t[1] * e
                jac = np.stack([np.ones_like(e), e, ae * uz, ae * uy, ae * ux, -0.5 * ae * dz * dz, -0.5 * ae * dy * dy,
                                -0.5 * ae * dx * dx, -ae * dz * dy, -ae * dz * dx, -ae * dy * dx], axis=1)
                jtj = np.zeros((11, 11))
                for i, j in PAIRS:
                    jtj[i, j] = jtj[j, i] = total(jac[:, i] * jac[:, j])
                jtr = total(jac * res[:, None])
                cost = total(res * res)
            diag = np.diag(jtj)
            if not np.all((diag > 0) & (diag < 1e300)):
                status = 2
                break
            scale = np.sqrt(diag)
            try:
                low = np.linalg.cholesky(jtj / np.outer(scale, scale) + lam * np.eye(11))
            except np.linalg.LinAlgError:
                status = 2
                break
            y = np.linalg.solve(low.T, np.linalg.solve(low, jtr / scale))
            trial = t + y / scale
            trial_cost = cost_of(trial)
            evals += 1
            small = np.abs(trial[2:5] - t[2:5]).max() < 1e-9 and abs(cost - trial_cost) <= 1e-12 * cost
            need_sums = bool(trial_cost <= cost)
            if need_sums:
                t, cost, lam = trial, trial_cost, (lam / 10.0 if lam > 1e-14 else lam)
            else:
                lam *= 10.0
            if small:
                break
            if evals >= max_iter:
                status = 1
                break
    if status == 0:
        w = precision(t)
        if not np.isfinite(t).all() or not np.all(np.linalg.eigvalsh(w) > 0):
            status = 2
        elif not np.all(np.abs(t[2:5]) < 1.0):
            status = 3
        elif not t[1] > 0:
            status = 4
    return (np.append(t, cost) if status == 0 else nan12), status, evals


def precision(t):
    return np.array([[t[5], t[8], t[9]], [t[8], t[6], t[10]], [t[9], t[10], t[7]]])


def cut(volume, centre, patch_shape):
    """The patch around ``centre``, or None when it does not fit the volume."""
    lo = [int(c) - n // 2 for c, n in zip(centre, patch_shape)]
    if any(a < 0 or a + n > s for a, n, s in zip(lo, patch_shape, np.shape(volume))):
        return None
    return np.asarray(volume)[tuple(slice(a, a + n) for a, n in zip(lo, patch_shape))]


def fit(volume, coords, patch_shape, max_iter=100, reverse=False):
    """``(theta (N, 12), status (N,), evaluations (N,))`` over the beads at ``coords``; status 5 where the patch does not fit."""
    out = []
    for c in np.asarray(coords).reshape(-1, 3):
        p = cut(volume, c, patch_shape)
        out.append((np.full(12, np.nan), 5, 0) if p is None else fit_patch(p, max_iter, reverse))
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def scaled_difference(a, b):
    """Largest ``|a - b| / max(|b|, 1)`` over the parameters (and the cost) of the rows that are finite in both."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 12), np.asarray(b, dtype=np.float64).reshape(-1, 12)
    ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    if not ok.any():
        return 0.0
    return float((np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1.0)).max())


def fit_tolerance(forward, backward):
    """The bound of the module docstring from the restatement's two runs."""
    return max(16.0 * scaled_difference(forward, backward), 1e-9)


def principal_sigmas(w):
    """``(sigma (3,) widest first, axes as rows)`` of a precision matrix."""
    val, vec = np.linalg.eigh(np.asarray(w, dtype=np.float64))
    return 1.0 / np.sqrt(val), vec.T


def dirichlet(mu, n):
    """``w[k] = D_n(k + mu)`` straight from the definition (``mu`` not an integer, or n == 1)."""
    t = np.arange(n, dtype=np.float64) + mu
    return np.ones(1) if n == 1 else np.sin(np.pi * t) / (n * np.sin(np.pi * t / n))


def _circulant(c, w, axis):
    c = np.moveaxis(c, axis, -1)
    n = c.shape[-1]
    out = np.zeros_like(c)
    mag = np.zeros_like(c)
    i = np.arange(n)
    for j in range(n):
        term = c[..., j:j + 1] * w[(i - j) % n]
        out = out + term
        mag = mag + np.abs(term)
    return np.moveaxis(out, -1, axis), np.moveaxis(mag, -1, axis)


def shifted_average(volume, coords, patch_shape, weights, bg, total):
    """``(psf float64, bound float64, used)``: the shifted average with the caller's weights (N x (pz + py + px)), ``B`` and
    ``S``, summed as the kernel sums; ``bound`` is the per-element ``3 (pz + py + px) 2^-53 sum|c w|`` of the average -- the
    magnitudes carried through the three passes, over ``S``, averaged."""
    pz, py, px = patch_shape
    acc, mag_acc, used = np.zeros(patch_shape), np.zeros(patch_shape), 0
    for b, c in enumerate(np.asarray(coords).reshape(-1, 3)):
        p = cut(volume, c, patch_shape)
        w = np.asarray(weights[b], dtype=np.float64)
        if p is None or not total[b] > 0 or not np.isfinite(w).all():
            continue
        cur = p.astype(np.float64) - bg[b]
        mag = np.abs(cur)
        for axis, wa in ((2, w[pz + py:]), (1, w[pz:pz + py]), (0, w[:pz])):
            cur, _ = _circulant(cur, wa, axis)
            mag, _ = _circulant(mag, np.abs(wa), axis)
        acc = acc + cur / total[b]
        mag_acc = mag_acc + mag / abs(total[b])
        used += 1
    n = max(used, 1)
    return acc / n, 3.0 * (pz + py + px) * 2.0 ** -53 * mag_acc / n, used


# ------------------------------------------------------------------ the scenes

TRUE_SIGMA = (1.8, 1.0, 0.9)          # principal sigmas of every bead, voxels
TILT_DEG = 20.0                        # the widest axis is tilted from z towards x


def true_axes():
    """The principal axes as rows (unit ZYX vectors), in the order of ``TRUE_SIGMA``."""
    a = np.deg2rad(TILT_DEG)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def true_covariance():
    axes = true_axes()
    return (axes.T * np.array(TRUE_SIGMA) ** 2) @ axes


def render(shape, centres, amplitudes, cov, background=100.0):
    """Noise-free beads: ``background + sum_k A_k exp(-(r - c_k)^T cov^-1 (r - c_k) / 2)`` sampled at the voxel centres,
    float64 arithmetic, rounded to float32 once."""
    w = np.linalg.inv(cov)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    out = np.full(shape, float(background))
    for c, a in zip(np.asarray(centres, dtype=np.float64).reshape(-1, 3), amplitudes):
        d = grid - c
        out += a * np.exp(-0.5 * np.einsum("...i,ij,...j->...", d, w, d))
    return out.astype(np.float32)


def scene_a():
    """``(volume float32 40 x 72 x 80, integer peaks (10, 3), true centres (10, 3), amplitudes, patch (11, 13, 13))``: ten
    beads at least 19 voxels apart on an axis, offsets stratified over (-0.5, 0.5) on every axis (k-th of ten strata, the
    strata permuted differently per axis), amplitudes 1000 .. 3000 on a background of 100."""
    peaks = np.array([[10, 12, 14], [10, 12, 40], [10, 12, 66], [10, 36, 27], [10, 36, 53], [10, 60, 14], [10, 60, 40],
                      [10, 60, 66], [29, 24, 27], [29, 48, 53]])
    k = np.arange(10)
    strata = (np.stack([k, (3 * k + 1) % 10, (7 * k + 4) % 10], axis=1) + 0.5) / 10.0 - 0.5
    centres = peaks + strata
    amplitudes = 1000.0 + 2000.0 * k / 9.0
    return render((40, 72, 80), centres, amplitudes, true_covariance()), peaks, centres, amplitudes, (11, 13, 13)


def scene_b_small():
    """A 3 x 5 x 7 patch (105 voxels, fewer than one workgroup) in a 9 x 11 x 13 volume: one narrow bead; a second centre
    whose patch does not fit (status 5)."""
    cov = np.diag(np.array([0.55, 0.7, 0.9]) ** 2)
    centre = np.array([[4.2, 5.3, 6.1]])
    vol = render((9, 11, 13), centre, [1500.0], cov)
    return vol, np.array([[4, 5, 6], [0, 5, 6]]), (3, 5, 7)


def scene_b_large():
    """A 31 x 37 x 19 patch on a 48 x 64 x 40 volume: two beads (many strides per lane, intermediates beyond LDS) -- the
    second 1.3 voxels from the centre it is given (status 3) -- a flat patch (status 2 or 4: 4, A0 = 0), a patch with a
    NaN in it (status 5) and a centre outside the volume (status 5)."""
    cov = true_covariance()
    centres = np.array([[16.3, 19.6, 10.2], [31.0, 44.3, 29.0]])
    vol = render((48, 64, 40), centres, [2000.0, 1200.0], cov)
    flat = np.full((48, 64, 40), 100.0, dtype=np.float32)
    peaks = np.array([[16, 20, 10], [31, 43, 29]])
    nan = vol.copy()
    nan[16 + 9, 20 - 11, 10 + 3] = np.nan          # inside the first bead's patch, outside the second's
    return vol, flat, nan, peaks, centres, (31, 37, 19)
