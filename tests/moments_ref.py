"""The restatement of the moment, shape and contact rules (``csrc/moments.hpp``, ``segment.shape_table``'s docstring) in plain
numpy on the raw voxel coordinates.  PARITY UNPINNED: no upstream is vendored; this file and the rule say the same thing in two
ways."""

import numpy as np

FIELDS = ("volume", "s_z", "s_y", "s_x", "m_zz", "m_yy", "m_xx", "m_zy", "m_zx", "m_yx")
DTYPE = np.dtype([(f, "<i8") for f in FIELDS])


def moments(labels: np.ndarray, n: int) -> np.ndarray:
    """``n`` records of ten int64: ``np.add.at`` of every voxel's gains, labels outside ``1 .. n`` ignored."""
    labels = np.asarray(labels)
    z, y, x = (c.ravel().astype(np.int64) for c in np.indices(labels.shape))
    flat = labels.ravel().astype(np.int64)
    keep = (flat >= 1) & (flat <= n)
    k, z, y, x = flat[keep] - 1, z[keep], y[keep], x[keep]
    out = np.zeros((n,), dtype=DTYPE)
    gains = dict(volume=np.ones_like(z), s_z=z, s_y=y, s_x=x, m_zz=z * z, m_yy=y * y, m_xx=x * x, m_zy=z * y, m_zx=z * x, m_yx=y * x)
    for f in FIELDS:
        column = np.zeros((n,), dtype=np.int64)
        np.add.at(column, k, gains[f])
        out[f] = column
    return out


def eigenvalues(labels: np.ndarray, k: int, sampling) -> np.ndarray:
    """``l0 >= l1 >= l2`` of label ``k``: ``np.cov(ddof=0)`` of its voxels' physical coordinates plus ``s^2 / 12`` on the
    diagonal, in float64."""
    s = np.asarray(sampling, dtype=np.float64)
    coords = np.argwhere(np.asarray(labels) == k).astype(np.float64) * s
    cov = np.cov(coords.T, ddof=0).reshape(3, 3) + np.diag(s * s / 12.0)
    return np.clip(np.linalg.eigvalsh(cov)[::-1], 0.0, None)


def faces_and_contacts(labels: np.ndarray, n: int):
    """Brute force: every voxel against its six neighbours in the volume padded with 0.  ``faces`` ((n, 3) int64): per label and
    axis the faces behind which another value lies (the background, another label, the padding).  ``contacts``: ``{(a, b):
    [faces_z, faces_y, faces_x]}`` for the labels ``a < b`` in ``1 .. n`` that share a face."""
    labels = np.asarray(labels).astype(np.int64)
    labels = np.where((labels >= 1) & (labels <= n), labels, 0)
    padded = np.pad(labels, 1)
    core = (slice(1, -1),) * 3
    faces = np.zeros((n, 3), dtype=np.int64)
    contacts = {}
    for c in range(3):
        for step in (-1, 1):
            other = np.roll(padded, step, axis=c)[core]
            differs = (labels > 0) & (other != labels)
            faces[:, c] += np.bincount(labels[differs] - 1, minlength=n)[:n] if n else 0
            if step == 1:       # (every touching pair of voxels once)
                touch = differs & (other > 0)
                for a, b in zip(labels[touch].tolist(), other[touch].tolist()):
                    contacts.setdefault((min(a, b), max(a, b)), [0, 0, 0])[c] += 1
    return faces, contacts
