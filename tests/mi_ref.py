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
"""

import numpy as np

WEIGHT_ONE = 65536


def stride3(stride):
    return (int(stride),) * 3 if np.isscalar(stride) else tuple(int(v) for v in stride)


def samples(moving, target, matrix, stride):
    """Per counted sample: target value, moving value, gradient of the interpolant (3, n), target index (3, n)."""
    mov = np.asarray(moving, dtype=np.float64)
    tgt = np.asarray(target, dtype=np.float64)
    m = np.asarray(matrix, dtype=np.float64)[:3]
    sz, sy, sx = stride3(stride)
    zo, yo, xo = np.meshgrid(np.arange(0, tgt.shape[0], sz), np.arange(0, tgt.shape[1], sy), np.arange(0, tgt.shape[2], sx),
                             indexing="ij")
    zo, yo, xo = zo.ravel(), yo.ravel(), xo.ravel()
    zd, yd, xd = zo.astype(np.float64), yo.astype(np.float64), xo.astype(np.float64)
    coords = [m[r, 0] * zd + m[r, 1] * yd + m[r, 2] * xd + m[r, 3] for r in range(3)]
    ok = np.ones(zo.shape, dtype=bool)
    for cc, n in zip(coords, mov.shape):
        ok &= (cc >= 0.0) & (cc < n - 1)
    cz, cy, cx = (cc[ok] for cc in coords)
    jz, jy, jx = cz.astype(np.int64), cy.astype(np.int64), cx.astype(np.int64)
    fz, fy, fx = cz - jz, cy - jy, cx - jx
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
    tv = tgt[zo[ok], yo[ok], xo[ok]]
    return tv, mval, np.stack([gz, gy, gx]), np.stack([zd[ok], yd[ok], xd[ok]])


def bin_rule(tv, mval, bins, ranges):
    """(a, b0, unclamped u, f) per sample."""
    (t_lo, t_hi), (m_lo, m_hi) = ranges
    a = np.floor((tv - float(t_lo)) * bins / (float(t_hi) - float(t_lo)))
    a = np.clip(a, 0, bins - 1).astype(np.int64)
    u_raw = (mval - float(m_lo)) * (bins - 1) / (float(m_hi) - float(m_lo))
    u = np.clip(u_raw, 0.0, float(bins - 1))
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
