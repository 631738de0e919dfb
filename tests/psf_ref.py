"""NumPy / float64 restatement of the bead-detection rule and of the PSF patch average (``shrimpy_amd/psf.py``,
``csrc/peaks.hip``).  PARITY UNPINNED: the reference hands this stage to biahub's ``_characterize_psf``, which is not
vendored (``scripts/measure_psf.py:17, 194-203``); the rule is the package's own and this file is what pins it.

Detection, on a float32 ``(Z, Y, X)`` volume ``s`` with window half-widths ``r = (rz, ry, rx)``: voxel ``p`` is a peak iff

    s(p) >= threshold_abs,
    s(p) >= s(q) for every in-volume q with |q - p| <= r per axis,
    s(p) >  s(q) for every such q whose linear index is below p's.

Comparisons with a NaN are false: a NaN is never a peak and no voxel with a NaN in its window is one.  Peaks closer than
``exclude_border`` to a face are dropped; the rest are ordered by value descending, then linear index ascending; a peak
is *isolated* for patch half-sizes ``h`` iff its patch fits the volume and no other peak lies within ``2 h`` of it on all
three axes (tested on the list before ``max_num_peaks`` keeps its first N).

``detect`` evaluates the rule with whole-array window maxima (inclusive for the full window, one-sided and exclusive for
the part of the window below ``p`` in C order); ``detect_literal`` is the triple loop of the definition, for small
volumes -- ``tests/test_psf_host.py`` holds the two against each other.
"""

import numpy as np


def smooth(v, b):
    """The box smoothing in float64: ``b`` equal taps per axis, mirrored borders (index -k -> k)."""
    from scipy import ndimage

    s = np.asarray(v, dtype=np.float64)
    if b == 1:
        return s
    taps = np.full(b, np.float64(np.float32(1.0 / b)))        # the taps the implementation uses: float32(1 / b)
    for axis in range(3):
        s = ndimage.correlate1d(s, taps, axis=axis, mode="mirror")
    return s


def _window_max(a, axis, lo, hi):
    """max of ``a`` over offsets ``[lo, hi]`` along ``axis``; out-of-volume = -inf; an empty range = -inf; NaNs spread."""
    if hi < lo:
        return np.full(a.shape, -np.inf, dtype=a.dtype)
    n, left, right = hi - lo + 1, max(-lo, 0), max(hi, 0)
    p = np.moveaxis(a, axis, -1)
    length = p.shape[-1]
    p = np.pad(p, [(0, 0)] * (a.ndim - 1) + [(left, right)], constant_values=-np.inf)
    span = 1                                  # p[j] = max over [j, j + span) of the padded line, spans doubled
    while span * 2 <= n:
        p = np.maximum(p[..., :-span], p[..., span:])
        span *= 2
    start = lo + left
    out = np.maximum(p[..., start:start + length], p[..., start + n - span:start + n - span + length])
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def _r3(r):
    return (int(r),) * 3 if np.isscalar(r) else tuple(int(v) for v in r)


def peak_mask(s, r, threshold_abs):
    s = np.asarray(s, dtype=np.float32)
    rz, ry, rx = _r3(r)
    a = _window_max(s, 2, -rx, rx)
    b = _window_max(a, 1, -ry, ry)
    m = _window_max(b, 0, -rz, rz)
    with np.errstate(invalid="ignore"):
        below = np.stack([_window_max(s, 2, -rx, -1), _window_max(a, 1, -ry, -1), _window_max(b, 0, -rz, -1)])
        # (`not >=` rather than `<`: a one-sided maximum of -inf must not veto, and a NaN there has made m a NaN already)
        return (s >= np.float32(threshold_abs)) & (s >= m) & ~(below >= s).any(axis=0)


def peak_mask_literal(s, r, threshold_abs):
    s = np.asarray(s, dtype=np.float32)
    rz, ry, rx = _r3(r)
    nz, ny, nx = s.shape
    out = np.zeros(s.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    v = s[z, y, x]
                    if not v >= np.float32(threshold_abs):
                        continue
                    z0, y0, x0 = max(z - rz, 0), max(y - ry, 0), max(x - rx, 0)
                    win = s[z0:z + rz + 1, y0:y + ry + 1, x0:x + rx + 1]
                    if not (v >= win).all():
                        continue
                    flat = win.ravel()
                    me = np.ravel_multi_index((z - z0, y - y0, x - x0), win.shape)   # C order in the window = C order in s
                    out[z, y, x] = bool((v > flat[:me]).all())
    return out


def isolated_mask(coords, shape, half):
    """Per peak: its patch of half-sizes ``half`` fits ``shape`` and no other peak is within ``2 * half`` on all axes."""
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    half = np.asarray(half, dtype=np.int64)
    fits = np.all((coords >= half) & (coords + half < np.asarray(shape)), axis=1)
    d = np.abs(coords[:, None, :] - coords[None, :, :])
    near = np.all(d <= 2 * half, axis=2)
    np.fill_diagonal(near, False)
    return fits & ~near.any(axis=1)


def finish(mask, s, exclude_border=(0, 0, 0), max_num_peaks=None, patch_half=None):
    """Border filter, ordering, isolation and cap on a peak mask: ``(coords (N, 3) int64, values float32, isolated)``."""
    s = np.asarray(s, dtype=np.float32)
    coords = np.argwhere(mask)
    e = np.asarray(_r3(exclude_border))
    keep = np.all((coords >= e) & (coords <= np.asarray(s.shape) - 1 - e), axis=1)
    coords = coords[keep]
    values = s[tuple(coords.T)]
    lin = np.ravel_multi_index(tuple(coords.T), s.shape)
    order = np.lexsort((lin, -values.astype(np.float64)))
    coords, values = coords[order], values[order]
    iso = isolated_mask(coords, s.shape, patch_half) if patch_half is not None else None
    if max_num_peaks is not None:
        coords, values = coords[:max_num_peaks], values[:max_num_peaks]
        iso = None if iso is None else iso[:max_num_peaks]
    return coords.astype(np.int64), values.astype(np.float32), iso


def detect(s, r, threshold_abs, exclude_border=(0, 0, 0), max_num_peaks=None, patch_half=None, literal=False):
    mask = (peak_mask_literal if literal else peak_mask)(s, r, threshold_abs)
    return finish(mask, s, exclude_border, max_num_peaks, patch_half)


def shell_mask(shape):
    m = np.ones(shape, dtype=bool)
    if min(shape) > 2:
        m[1:-1, 1:-1, 1:-1] = False
    return m


def average(volume, coords, patch_shape):
    """``(psf float64, B per bead, S per bead, skipped indices)``: the mean over the beads with ``S > 0`` of
    ``(patch - B) / S``, ``B`` = mean of the patch's six faces, ``S = sum(patch - B)``, everything float64."""
    vol = np.asarray(volume, dtype=np.float64)
    half = [n // 2 for n in patch_shape]
    shell = shell_mask(tuple(patch_shape))
    acc, bgs, totals, skipped = np.zeros(patch_shape), [], [], []
    for i, c in enumerate(np.asarray(coords).reshape(-1, 3)):
        patch = vol[tuple(slice(int(p) - h, int(p) + h + 1) for p, h in zip(c, half))]
        assert patch.shape == tuple(patch_shape), "the patch does not fit the volume"
        bg = patch[shell].mean()
        total = (patch - bg).sum()
        bgs.append(bg)
        totals.append(total)
        if total > 0:
            acc += (patch - bg) / total
        else:
            skipped.append(i)
    used = len(bgs) - len(skipped)
    return (acc / used if used else acc), np.array(bgs), np.array(totals), np.array(skipped, dtype=np.int64)

