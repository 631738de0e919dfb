"""Float64 numpy restatement of the mutual-information metric of the registration estimate (no reference code exists
for it): the per-sample rule of the joint histogram, the mutual information, and the analytic gradient.  Written from the
rule's statement, not from the native twin:

    a  = clamp(floor((t - t_lo) * bins / (t_hi - t_lo)), 0, bins - 1)           target bin, zero order
    u  = clamp((m - m_lo) * (bins - 1) / (m_hi - m_lo), 0, bins - 1)            m: trilinear, lerped x, then y, then z
    b0 = min(floor(u), bins - 2), f = u - b0
    w1 = floor(f * 65536 + 0.5), w0 = 65536 - w1                                (``quantised=False``: w1 = f * 65536)
    hist[a, b0] += w0, hist[a, b0 + 1] += w1

A sample counts when its moving coordinate lies in [0, n - 1) on every axis.  The gradient takes the samples whose
unclamped u lies strictly inside (0, bins - 1); a u of exactly 0 or bins - 1 counts as clamped.

Values that are not finite (the text of ``csrc/mi_sample.hpp``, not the twin's output)
--------------------------------------------------------------------------------------
The lerp is IEEE arithmetic as written, so a NaN tap makes m NaN and so does an infinite tap at any fraction
(``v0 + 0 * (inf - v0)`` is NaN).  The clamps are comparisons that a NaN fails: a NaN target value goes to target bin 0,
-inf to bin 0, +inf to the last bin; a NaN u is clamped to 0 -- b0 = 0, w1 = 0, the whole weight in column 0 -- and adds
nothing to the gradient; u = -inf goes to 0 and +inf to bins - 1 (b0 = bins - 2, w1 = 65536).  Such a sample is still
counted: the count depends on the coordinates alone.  ``bin_rule`` states this explicitly.

The raw gradient and who owns a sample
--------------------------------------
``gradient_terms`` takes the operands of ``lsr_affine_mi_gradient_f32`` -- a caller-supplied ``dl`` included -- and
returns the 12 unnormalised sums with the per-sample terms ``((dl[a, b0] * du) * g_i) * x~_j``, ``du = (bins - 1) /
(m_hi - m_lo)``, in the kernel's written order; ``owner`` names the workgroup that visits a grid sample, so a test can
add the terms per workgroup and compare the kernel's partial rows one by one.

Exact cases (``tests/mi_edge_cases.py``): small integer voxels, matrix entries multiples of 1/8, power-of-two range
widths and scale, an integer centre and an integer ``dl``.  Every coordinate, fraction, lerp, u and ``f * 65536 + 0.5`` is
then a float64 without rounding and every term a multiple of 2^-15 (``du`` of 2^-3 with a range 8 wide, ``g`` of 2^-6,
``x~`` of 2^-6 at scale 64); while ``sum |terms| 2^15 < 2^53`` every partial sum in ANY order is a float64 too, so the kernel must return the restatement's bits whatever its summation order.
``exact_integer_terms`` re-proves that per case in int64.

The a-priori bound of the generic cases
---------------------------------------
Model ``fl(a op b) = (a op b)(1 + d)``, ``|d| <= u = 2^-53``.  Kernel, twin and restatement form ``a``, ``b0``, ``u``,
``g`` and ``w g = (dl[a, b0] * du) * g_i`` with the same IEEE operations on the same operands in the same order (no
contraction on either side): the same bits, and the same samples contribute.  What differs, per component:

* ``x~``: the library multiplies by ``fl(1 / scale)`` (2 roundings), the rule divides (1): the two ``x~`` differ by at
  most 3 u |x~|; the last product of a term is rounded on both sides (2 more): two terms differ by at most 5 u |term|,
  6 with the second-order remainder of everything here;
* the library adds the N <= n contributing terms per thread, wave, workgroup and then row by row on the host.  Adding
  an exact zero costs nothing, and a summation tree over N terms has depth at most N - 1: at most (N - 1) u sum|terms|;
* the restatement's sums are extended (64-bit mantissa, pairwise) and rounded once: at most 1 u sum|terms|;
* both sides divide by n (an integer below 2^53, exact on both): 1 rounding each, 2 u sum|terms| / n.

Together ``|kernel - restatement| <= (n + 8) u sum|terms| / n`` (``K_ROUNDINGS = 8``), absolute per component.

``mi_gradient`` forms ``dL`` from a histogram on the host in its own float64 order (``log(h / h_m)`` with the exact
integer column sum ``h_m``: 1 rounding in the ratio), ``d_log`` here as ``log(p / p_m)`` with ``p = h / total`` (1
rounding), ``p_m`` a sum of ``bins`` non-negative values (at most ``bins`` u relative) and the quotient (1): the two
arguments of the logarithm differ by at most ``(bins + 3) u`` relative, which moves ``L`` by as much in absolute terms; a
logarithm within one unit in the last place adds ``2 u |L|`` on each side, and the difference ``L[a, b + 1] - L[a, b]``
one rounding on each side (``u |dL| <= u (|L[a, b]| + |L[a, b + 1]|)``).  Per entry the two ``dL`` differ by at most
``(2 (bins + 3) + 6 (|L[a, b]| + |L[a, b + 1]|)) u`` (``d_log_slack``); the gradient is linear in ``dL``, so this adds
``sum slack[a, b0] |du g_i x~_j| / n`` (``gradient_bound(..., dl_slack)``).  No figure of a device run enters either part.
"""

from collections import namedtuple

import numpy as np

WEIGHT_ONE = 65536
U = 2.0 ** -53
K_ROUNDINGS = 8


def stride3(stride):
    return (int(stride),) * 3 if np.isscalar(stride) else tuple(int(v) for v in stride)


Rows = namedtuple("Rows", "tv mval g idx index keep coord cell frac")
Terms = namedtuple("Terms", "sums terms index unit a b0 u_raw inside")


def geometry(moving_shape, target_shape, matrix, stride):
    """What the coordinates alone decide: ``(index, keep, coord, cell, frac, (zo, yo, xo))``.  ``keep`` and ``coord``
    cover the whole strided grid in the kernels' sample order (z slowest); ``index`` holds the grid sample numbers of
    the kept samples; ``cell`` (truncation) and ``frac = coord - cell`` (exact) are per kept sample."""
    m = np.asarray(matrix, dtype=np.float64)[:3]
    sz, sy, sx = stride3(stride)
    zo, yo, xo = np.meshgrid(np.arange(0, target_shape[0], sz), np.arange(0, target_shape[1], sy),
                             np.arange(0, target_shape[2], sx), indexing="ij")
    zo, yo, xo = zo.ravel(), yo.ravel(), xo.ravel()
    zd, yd, xd = zo.astype(np.float64), yo.astype(np.float64), xo.astype(np.float64)
    coord = [m[r, 0] * zd + m[r, 1] * yd + m[r, 2] * xd + m[r, 3] for r in range(3)]      # left to right, no fma
    keep = np.ones(zo.shape, dtype=bool)
    for cc, n in zip(coord, moving_shape):
        keep &= (cc >= 0.0) & (cc < n - 1)
    cell = np.stack([cc[keep].astype(np.int64) for cc in coord])
    frac = np.stack([cc[keep] for cc in coord]) - cell
    return np.flatnonzero(keep), keep, coord, cell, frac, (zo[keep], yo[keep], xo[keep])


def sample_rows(moving, target, matrix, stride):
    """Per counted sample, in grid order: target value, moving value, gradient of the interpolant (3, n), target index
    (3, n) as float64, and the ``geometry`` of the launch.  The lerp is IEEE arithmetic as written: a NaN tap makes the
    value NaN, and so does an infinite one, whatever its fraction (0 * inf, inf - inf)."""
    mov = np.asarray(moving, dtype=np.float64)
    tgt = np.asarray(target, dtype=np.float64)
    index, keep, coord, cell, frac, (zo, yo, xo) = geometry(mov.shape, tgt.shape, matrix, stride)
    (jz, jy, jx), (fz, fy, fx) = cell, frac
    with np.errstate(invalid="ignore", over="ignore"):
        v = {(a, b, c): mov[jz + a, jy + b, jx + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)}
        a00 = v[0, 0, 0] + fx * (v[0, 0, 1] - v[0, 0, 0])
        a01 = v[0, 1, 0] + fx * (v[0, 1, 1] - v[0, 1, 0])
        a10 = v[1, 0, 0] + fx * (v[1, 0, 1] - v[1, 0, 0])
        a11 = v[1, 1, 0] + fx * (v[1, 1, 1] - v[1, 1, 0])
        b0 = a00 + fy * (a01 - a00)
        b1 = a10 + fy * (a11 - a10)
        mval = b0 + fz * (b1 - b0)
        gz = b1 - b0
        gy = (a01 - a00) + fz * ((a11 - a10) - (a01 - a00))
        d00, d01 = v[0, 0, 1] - v[0, 0, 0], v[0, 1, 1] - v[0, 1, 0]
        d10, d11 = v[1, 0, 1] - v[1, 0, 0], v[1, 1, 1] - v[1, 1, 0]
        e0, e1 = d00 + fy * (d01 - d00), d10 + fy * (d11 - d10)
        gx = e0 + fz * (e1 - e0)
    tv = tgt[zo, yo, xo]
    idx = np.stack([zo, yo, xo]).astype(np.float64)
    return Rows(tv, mval, np.stack([gz, gy, gx]), idx, index, keep, coord, cell, frac)


def samples(moving, target, matrix, stride):
    """Per counted sample: target value, moving value, gradient of the interpolant (3, n), target index (3, n)."""
    r = sample_rows(moving, target, matrix, stride)
    return r.tv, r.mval, r.g, r.idx


def bin_rule(tv, mval, bins, ranges):
    """(a, b0, unclamped u, f) per sample.  Values that are not finite follow the text of ``mi_sample.hpp``: a NaN or
    -inf target value goes to bin 0, +inf to the last bin; a NaN u is clamped to 0 (b0 = 0, f = 0: the whole weight in
    column 0), -inf to 0, +inf to bins - 1 (b0 = bins - 2, f = 1).  The unclamped u is returned as it is -- NaN
    included, which fails both comparisons of the gradient's ``0 < u < bins - 1``."""
    (t_lo, t_hi), (m_lo, m_hi) = ranges
    tv, mval = np.asarray(tv, dtype=np.float64), np.asarray(mval, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a_raw = np.floor((tv - float(t_lo)) * bins / (float(t_hi) - float(t_lo)))
        u_raw = (mval - float(m_lo)) * (bins - 1) / (float(m_hi) - float(m_lo))
    a = np.where(np.isnan(a_raw), 0.0, np.clip(a_raw, 0.0, float(bins - 1))).astype(np.int64)
    u = np.where(np.isnan(u_raw), 0.0, np.clip(u_raw, 0.0, float(bins - 1)))
    b0 = np.minimum(np.floor(u).astype(np.int64), bins - 2)
    return a, b0, u_raw, u - b0


def joint_histogram(moving, target, matrix, stride, bins, ranges, quantised=True):
    """``(hist [bins, bins], n)``: uint64 in units of 2^-16 sample, or -- ``quantised=False`` -- float64 in the same
    units with the window's weights as they are."""
    tv, mval, _, _ = samples(moving, target, matrix, stride)
    a, b0, _, f = bin_rule(tv, mval, bins, ranges)
    if quantised:
        w1 = np.floor(f * 65536.0 + 0.5).astype(np.int64)
        hist = np.zeros((bins, bins), dtype=np.int64)
    else:
        w1 = f * 65536.0
        hist = np.zeros((bins, bins), dtype=np.float64)
    np.add.at(hist, (a, b0), WEIGHT_ONE - w1)
    np.add.at(hist, (a, b0 + 1), w1)
    return (hist.astype(np.uint64) if quantised else hist), int(tv.size)


def mutual_information(hist):
    """sum P log(P / (P_t P_m)) over the non-empty cells, nats."""
    h = np.asarray(hist, dtype=np.float64)
    total = h.sum()
    if total <= 0:
        return 0.0
    p = h / total
    pt, pm = p.sum(axis=1), p.sum(axis=0)
    value = 0.0
    for a in range(h.shape[0]):
        for b in range(h.shape[1]):
            if p[a, b] > 0:
                value += p[a, b] * np.log(p[a, b] / (pt[a] * pm[b]))
    return float(value)


def d_log(hist):
    """dL[a, b] = L[a, b + 1] - L[a, b], L = log(P / P_m), 0 in empty cells."""
    h = np.asarray(hist, dtype=np.float64)
    p = h / h.sum()
    pm = p.sum(axis=0)
    big_l = np.zeros_like(p)
    for a in range(h.shape[0]):
        for b in range(h.shape[1]):
            if p[a, b] > 0:
                big_l[a, b] = np.log(p[a, b] / pm[b])
    return big_l[:, 1:] - big_l[:, :-1]


def gradient(moving, target, matrix, stride, bins, ranges, centre, scale, hist=None, quantised=True):
    """Gradient of the MI with respect to the matrix rows in centred, scaled coordinates ((x - centre) / scale, 1):
    (1 / n) sum dL[a, b0] * (bins - 1) / (m_hi - m_lo) * grad m (x) x~ over the unclamped samples."""
    tv, mval, g, idx = samples(moving, target, matrix, stride)
    if hist is None:
        hist, _ = joint_histogram(moving, target, matrix, stride, bins, ranges, quantised)
    dl = d_log(hist)
    a, b0, u_raw, _ = bin_rule(tv, mval, bins, ranges)
    inside = (u_raw > 0.0) & (u_raw < bins - 1)
    (_, _), (m_lo, m_hi) = ranges
    w = np.where(inside, dl[a, b0], 0.0) * ((bins - 1) / (float(m_hi) - float(m_lo)))
    c = np.asarray(centre, dtype=np.float64)
    xt = np.concatenate([(idx - c[:, None]) / float(scale), np.ones((1, tv.size))])
    out = np.zeros(12)
    for i in range(3):
        for j in range(4):
            out[4 * i + j] = np.sum(w * g[i] * xt[j])
    return out / max(tv.size, 1)


def _sum_extended(terms):
    """Column sums (samples along axis 0) by pairwise halving in extended precision, rounded to float64 once."""
    assert np.finfo(np.longdouble).nmant >= 63, "the restatement's sums need an extended-precision long double"
    a = np.asarray(terms, np.longdouble)
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:])
    while a.shape[0] > 1:
        if a.shape[0] % 2:
            a = np.concatenate([a, np.zeros((1,) + a.shape[1:], np.longdouble)])
        half = a.shape[0] // 2
        a = a[:half] + a[half:]
    return a[0].astype(np.float64)


def gradient_terms(rows, bins, ranges, centre, scale, dl):
    """The operands of ``lsr_affine_mi_gradient_f32`` with a caller-supplied ``dl`` [bins, bins - 1], unnormalised:
    ``Terms`` with the 12 ``sums`` (extended-precision sums of the terms, rounded once), the per-sample ``terms``
    (n, 12) in grid order -- ``((dl[a, b0] * du) * g_i) * x~_j``, 0 for a sample that contributes nothing --, the grid
    sample numbers ``index``, and what the bound needs: ``unit = |du g_i x~_j|``, ``a``, ``b0``, ``u_raw``, ``inside``.
    ``rows`` = ``sample_rows(...)``."""
    a, b0, u_raw, _ = bin_rule(rows.tv, rows.mval, bins, ranges)
    inside = (u_raw > 0.0) & (u_raw < bins - 1)                      # a NaN fails both
    (_, _), (m_lo, m_hi) = ranges
    du = (bins - 1) / (float(m_hi) - float(m_lo))
    dl = np.asarray(dl, dtype=np.float64)
    assert dl.shape == (bins, bins - 1)
    w = dl[a, b0] * du
    c = np.asarray(centre, dtype=np.float64)
    xt = [(rows.idx[k] - c[k]) / float(scale) for k in range(3)] + [np.ones(rows.tv.size)]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.stack([(w * rows.g[i]) * xt[j] for i in range(3) for j in range(4)], axis=1)
        unit = np.abs(np.stack([(du * rows.g[i]) * xt[j] for i in range(3) for j in range(4)], axis=1))
    terms[~inside] = 0.0
    unit[~inside] = 0.0
    return Terms(_sum_extended(terms), terms, rows.index, unit, a, b0, u_raw, inside)


def owner(index, blocks):
    """The workgroup that visits grid sample ``s`` in a launch of ``blocks`` workgroups of 256 threads: thread
    ``s % (256 blocks)`` on trip ``s // (256 blocks)``, that is workgroup ``(s // 256) % blocks`` -- in both kernels."""
    return (np.asarray(index, dtype=np.int64) // 256) % int(blocks)


def sums_by_owner(terms, index, blocks):
    """(blocks, 12): the terms added per owning workgroup, in extended precision, rounded once."""
    own = owner(index, blocks)
    out = np.zeros((int(blocks), terms.shape[1]), dtype=np.longdouble)
    np.add.at(out, own, terms.astype(np.longdouble))
    return out.astype(np.float64)


def u_kinds(u_raw, bins):
    """How many samples have u < 0, == 0, inside (0, bins - 1), == bins - 1, > bins - 1, NaN."""
    top = bins - 1
    return dict(below=int((u_raw < 0).sum()), zero=int((u_raw == 0).sum()), inside=int(((u_raw > 0) & (u_raw < top)).sum()),
                top=int((u_raw == top).sum()), above=int((u_raw > top).sum()), nan=int(np.isnan(u_raw).sum()))


def exact_integer_terms(terms, bits):
    """The exactness proof of one case in int64: every term is a multiple of 2^-bits and the sum of the magnitudes, in
    that unit, stays below 2^53 in every column -- so every partial sum in ANY order is a float64.  Returns the 12 sums
    computed in integers, as float64, and the bits the widest column needs."""
    scaled = terms * float(1 << bits)
    assert np.array_equal(scaled, np.rint(scaled)), f"a term is not a multiple of 2^-{bits}"
    assert np.abs(scaled).max(initial=0.0) < 2.0 ** 62 / max(len(scaled), 1)
    i = scaled.astype(np.int64)
    widest = int(np.abs(i).sum(axis=0).max(initial=0))
    assert widest < 2 ** 53, f"the widest sum needs {widest.bit_length()} bits"
    return i.sum(axis=0) / float(1 << bits), widest.bit_length()


def d_log_slack(hist):
    """Bound on ``|dL - dL'|`` per entry between two float64 evaluations of ``d_log`` of one histogram (module
    docstring): ``(2 (bins + 3) + 6 (|L[a, b]| + |L[a, b + 1]|)) u``."""
    h = np.asarray(hist, dtype=np.float64)
    pm = h.sum(axis=0)
    big_l = np.zeros_like(h)
    nz = h > 0
    big_l[nz] = np.abs(np.log((h / np.where(pm > 0, pm, 1.0)[None, :])[nz]))
    return (2.0 * (h.shape[0] + 3) + 6.0 * (big_l[:, 1:] + big_l[:, :-1])) * U


def gradient_bound(t, n, dl_slack=None):
    """A-priori bound (12,) on the difference between a float64 evaluation of the normalised gradient and
    ``t.sums / n`` (module docstring): ``(n + K_ROUNDINGS) u sum|terms| / n``, and with ``dl_slack`` the first-order
    effect of a ``dL`` that differs by that much per entry."""
    b = (n + K_ROUNDINGS) * U * np.abs(t.terms).sum(axis=0)
    if dl_slack is not None:
        b = b + (dl_slack[t.a, t.b0][:, None] * t.unit).sum(axis=0) * (1.0 + 4 * U)
    return b / max(n, 1)


def worst_fraction(got, want, bound):
    """Largest ``|got - want| / bound`` over the entries (an entry with a zero bound must be equal)."""
    got, want, bound = (np.atleast_1d(np.asarray(v, np.float64)) for v in (got, want, bound))
    err = np.abs(got - want)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0))


def normalised(m, c, s):
    """3x4 in voxel units -> the 12 parameters acting on ((x - c) / s, 1)."""
    m = np.asarray(m, dtype=np.float64)[:3]
    q = np.empty((3, 4))
    q[:, :3] = m[:, :3] * s
    q[:, 3] = m[:, :3] @ c + m[:, 3]
    return q.ravel()


def from_normalised(params, c, s):
    q = np.asarray(params, dtype=np.float64).reshape(3, 4)
    m = np.empty((3, 4))
    m[:, :3] = q[:, :3] / s
    m[:, 3] = q[:, 3] - m[:, :3] @ c
    return m
