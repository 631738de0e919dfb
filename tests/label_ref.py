"""The oracle of the labelling tests: ``scipy.ndimage.label`` for the labels, ``find_objects`` / ``bincount`` for the integer
columns of the object table, ``math.fsum`` for its float64 sums, numpy for the filter.

``scipy.ndimage.label`` numbers the components ``1 .. N`` in raster order of each component's first voxel, for every
structure of ``generate_binary_structure(3, 1 | 2 | 3)`` -- the numbering ``csrc/label.hip`` produces by construction (its
union-find is rooted at the smallest linear index), so the comparison is exact equality, element for element.

The float64 sums of the table are compared within the a-priori bound ``n_k * 2^-53 * sum|terms|`` per label (``n_k`` voxels;
any order of ``n_k - 1`` float64 additions of exactly representable terms stays inside it -- the products ``v * coordinate``
are exact in float64 at the sizes tested: 24 significant bits times fewer than 2^11.  That holds at scale too: the greatest
extent a table is measured over in ``tests/label_scale_cases.py`` is 2000 < 2^11, which ``tests/test_label_scale_host.py``
asserts; 35 bits of a product leave 18 to spare).
"""

import functools
import math

import numpy as np
from scipy import ndimage

from tests import label_cases as C

LEVEL = {6: 1, 18: 2, 26: 3}


def label(vol, threshold, connectivity):
    """``(labels int32, n)`` of ``vol > threshold`` (NaN compares false: background)."""
    with np.errstate(invalid="ignore"):
        mask = np.asarray(vol) > np.float32(threshold)
    labels, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, LEVEL[connectivity]))
    return labels.astype(np.int32), int(n)


@functools.lru_cache(maxsize=None)
def case_labels(name, connectivity):
    """The reference labels of a named case, computed once and shared (read-only)."""
    c = C.case(name)
    labels, n = label(c["vol"], c["threshold"], connectivity)
    labels.setflags(write=False)
    return labels, n


def table(labels, n, intensity=None):
    """The object table of ``labels`` (1 .. n): dict of arrays as ``segment.region_table`` returns them, the float sums by
    ``math.fsum``, plus ``bound_sum`` / ``bound_sum_zyx``: the a-priori bounds of the float64 sums."""
    labels = np.asarray(labels)
    flat = labels.ravel()
    volume = np.bincount(flat, minlength=n + 1)[1:n + 1].astype(np.int64)
    coords = np.indices(labels.shape).reshape(3, -1)
    sums = np.stack([np.bincount(flat, weights=coords[a], minlength=n + 1)[1:n + 1] for a in range(3)], axis=1)
    assert np.all(sums < 2.0 ** 53)
    bbox = np.zeros((n, 6), dtype=np.int32)
    for k, sl in enumerate(ndimage.find_objects(labels, max_label=n)):
        if sl is not None:
            bbox[k] = [s.start for s in sl] + [s.stop for s in sl]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"label": np.arange(1, n + 1, dtype=np.int32), "volume": volume, "bbox": bbox, "sum_zyx": sums.astype(np.int64),
               "centroid": sums / volume[:, None].astype(np.float64)}
        if intensity is None:
            return out
        v = np.asarray(intensity, dtype=np.float32).ravel()
        order = np.argsort(flat, kind="stable")
        starts = np.searchsorted(flat[order], np.arange(1, n + 2))
        s_v, s_vzyx = np.zeros(n), np.zeros((n, 3))
        b_v, b_vzyx = np.zeros(n), np.zeros((n, 3))
        vmin, vmax = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        u = 2.0 ** -53
        for k in range(n):
            idx = order[starts[k]:starts[k + 1]]
            if len(idx) == 0:
                continue
            vals = v[idx].astype(np.float64)
            s_v[k] = math.fsum(vals)
            b_v[k] = len(idx) * u * math.fsum(np.abs(vals))
            for a in range(3):
                terms = vals * coords[a][idx]
                s_vzyx[k, a] = math.fsum(terms)
                b_vzyx[k, a] = len(idx) * u * math.fsum(np.abs(terms))
            vmin[k], vmax[k] = v[idx].min(), v[idx].max()
        out.update({"intensity_sum": s_v, "intensity_mean": s_v / volume, "intensity_min": vmin, "intensity_max": vmax,
                    "intensity_sum_zyx": s_vzyx, "weighted_centroid": s_vzyx / s_v[:, None],
                    "bound_sum": b_v, "bound_sum_zyx": b_vzyx})
    return out


def check_table(got, want):
    """Integer columns and the intensity range exactly; the float64 sums within their bounds.  Returns the worst ratio of an
    error to its bound (0 where both are 0)."""
    for key in ("label", "volume", "bbox", "sum_zyx"):
        assert np.array_equal(got[key], want[key]), key
    if "intensity_sum" not in want:
        return 0.0
    for key in ("intensity_min", "intensity_max"):
        assert np.array_equal(np.asarray(got[key], dtype=np.float32).view(np.uint32), want[key].view(np.uint32)), key
    worst = 0.0
    for key, bound in (("intensity_sum", "bound_sum"), ("intensity_sum_zyx", "bound_sum_zyx")):
        err = np.abs(np.asarray(got[key], dtype=np.float64) - want[key])
        assert np.all(err <= want[bound]), (key, float(np.max(err - want[bound])))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(want[bound] > 0, err / want[bound], 0.0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    return worst


def filter_labels(labels, min_volume=0, keep_largest=False):
    """numpy restatement of ``segment.filter_objects``: ``(new labels, M)``; the kept labels keep their order."""
    labels = np.asarray(labels)
    n = int(labels.max()) if labels.size else 0
    volume = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    keep = [k for k in range(1, n + 1) if volume[k - 1] >= min_volume]
    if keep_largest and keep:
        best = max(volume[k - 1] for k in keep)
        keep = [min(k for k in keep if volume[k - 1] == best)]
    lut = np.zeros(n + 1, dtype=labels.dtype)
    lut[keep] = np.arange(1, len(keep) + 1)
    return lut[labels], len(keep)
