"""The specification of the watershed tests: the rule of ``shrimpy_amd/watershed.py`` restated in numpy.  No upstream is pinned
(``skimage`` is absent; ``scipy.ndimage.watershed_ift`` breaks ties by queue order), so this file IS the reference: ``up`` from
shifted arrays, the basins from ``scipy.sparse.csgraph.connected_components`` numbered by first index, the saddles from a
dictionary, the merge as the rule is written.  Everything here is exact: equality element for element, saddle values bit for
bit (a maximum of minima has no rounding).
"""

import functools
import itertools

import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

from tests import watershed_cases as C

LEVEL = {6: 1, 18: 2, 26: 3}
# every direction of the 3 x 3 x 3 block in raster order -- ascending linear index of the neighbour; (0, 0, 0) is v itself
BLOCK = list(itertools.product((-1, 0, 1), repeat=3))


def key(values):
    """The order-preserving integer image of float32 values (``lsr::label::float_key``), as int64."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.int64)


def _shifted(padded, d, shape):
    return padded[tuple(slice(1 + c, 1 + c + n) for c, n in zip(d, shape))]


def up(objects, surface, connectivity):
    """``up(v)`` as a linear index for every voxel (v itself on the background and at a summit)."""
    objects = np.where(np.asarray(objects) > 0, objects, 0).astype(np.int64)
    shape = objects.shape
    keys = key(surface).reshape(shape)
    pad_o, pad_k = np.pad(objects, 1), np.pad(keys, 1)
    index = np.arange(objects.size, dtype=np.int64).reshape(shape)
    pad_i = np.pad(index, 1)
    best = np.full(shape, -1, dtype=np.int64)
    target = index.copy()
    for d in BLOCK:                                   # ascending index: a later candidate wins only with a GREATER key
        nnz = sum(1 for c in d if c)
        if nnz > LEVEL[connectivity]:
            continue
        o, k, i = _shifted(pad_o, d, shape), _shifted(pad_k, d, shape), _shifted(pad_i, d, shape)
        take = ((o == objects) if nnz else np.ones(shape, dtype=bool)) & (objects > 0) & (k > best)
        best = np.where(take, k, best)
        target = np.where(take, i, target)
    return target


def number_by_first_index(component, foreground):
    """Component ids -> 1 .. N in raster order of each component's first voxel, 0 off the foreground: ``(labels int32, N)``."""
    flat, fg = np.asarray(component).ravel(), np.asarray(foreground).ravel()
    out = np.zeros(flat.shape, dtype=np.int32)
    if not fg.any():
        return out, 0
    ids, first = np.unique(flat[fg], return_index=True)
    rank = np.empty(len(ids), dtype=np.int32)
    rank[np.argsort(first, kind="stable")] = np.arange(1, len(ids) + 1, dtype=np.int32)
    out[fg] = rank[np.searchsorted(ids, flat[fg])]
    return out, len(ids)


def basins(objects, surface, connectivity):
    """``(basins int32, B, summits)``: the components of the edges {v, up(v)}; ``summits`` counts ``up(v) == v`` on the objects."""
    objects = np.asarray(objects)
    target = up(objects, surface, connectivity).ravel()
    fg = (objects > 0).ravel()
    n = objects.size
    v = np.flatnonzero(fg)
    graph = sparse.coo_matrix((np.ones(len(v), dtype=np.int8), (v, target[v])), shape=(n, n))
    _, component = csgraph.connected_components(graph, directed=False)
    labels, count = number_by_first_index(component, fg)
    return labels.reshape(objects.shape), count, int((target[v] == v).sum())


def saddles(objects, basin_labels, surface, connectivity):
    """``{(a, b): key of saddle(a, b)}`` over the neighbouring voxels of one object in different basins ``a < b``."""
    objects, basin_labels = np.asarray(objects), np.asarray(basin_labels)
    keys = key(surface).reshape(objects.shape)
    shape = objects.shape
    out = {}
    for d in BLOCK:
        nnz = sum(1 for c in d if c)
        if d <= (0, 0, 0) or nnz > LEVEL[connectivity]:          # every unordered pair once: the forward directions
            continue
        lo = tuple(slice(max(0, -c), n - max(0, c)) for c, n in zip(d, shape))
        hi = tuple(slice(max(0, c), n - max(0, -c)) for c, n in zip(d, shape))
        hit = (objects[lo] > 0) & (objects[lo] == objects[hi]) & (basin_labels[lo] != basin_labels[hi])
        a = np.minimum(basin_labels[lo][hit], basin_labels[hi][hit]).tolist()
        b = np.maximum(basin_labels[lo][hit], basin_labels[hi][hit]).tolist()
        p = np.minimum(keys[lo][hit], keys[hi][hit]).tolist()
        for pair, value in zip(zip(a, b), p):
            if value > out.get(pair, -1):
                out[pair] = value
    return out


def key_to_float(k):
    k = np.asarray(k, dtype=np.int64).astype(np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return bits.view(np.float32)


def saddle_arrays(table):
    """The dictionary of :func:`saddles` as ``basin_saddles`` returns it: sorted by (a, b)."""
    pairs = sorted(table)
    return {"a": np.array([p[0] for p in pairs], dtype=np.int32), "b": np.array([p[1] for p in pairs], dtype=np.int32),
            "saddle": key_to_float([table[p] for p in pairs]).reshape(len(pairs))}


def peaks(basin_labels, count, surface):
    """float32 (count,): the greatest surface value (by key) of each basin."""
    flat, keys = np.asarray(basin_labels).ravel(), key(surface).ravel()
    best = np.full(count + 1, -1, dtype=np.int64)
    np.maximum.at(best, flat, keys)
    return key_to_float(best[1:]).reshape(count)


def merge(peak, table, min_depth):
    """The merge as the rule is written: ``map`` (int32, B + 1 entries, map[0] = 0) from basin to cluster 1 .. M."""
    count = len(peak)
    peak = [None] + [np.float32(p) for p in peak]
    cluster = list(range(count + 1))                          # basin -> the smallest label of its cluster

    def root(k):
        while cluster[k] != k:
            k = cluster[k]
        return k

    def bits(f):
        return int(np.float32(f).view(np.uint32))

    edges = [(float(key_to_float([k])[0]), a, b) for (a, b), k in table.items()]
    edges.sort(key=lambda e: (-e[0], e[1], e[2]))
    for s, a, b in edges:
        ra, rb = root(a), root(b)
        if ra == rb:
            continue
        pa, pb = peak[ra], peak[rb]
        low, high = (pa, pb) if key([pa])[0] <= key([pb])[0] else (pb, pa)
        depth = 0.0 if bits(low) == bits(s) else float(low) - float(s)
        if depth <= min_depth:
            keep, gone = min(ra, rb), max(ra, rb)
            cluster[gone] = keep
            peak[keep] = high
    roots = sorted({root(k) for k in range(1, count + 1)})
    rank = {r: i + 1 for i, r in enumerate(roots)}
    return np.array([0] + [rank[root(k)] for k in range(1, count + 1)], dtype=np.int32)


def split(objects, surface, connectivity, min_depth):
    """``(labels int32, M)`` of the whole rule."""
    labels, count, _ = basins(objects, surface, connectivity)
    if count == 0:
        return labels, 0
    lut = merge(peaks(labels, count, surface), saddles(objects, labels, surface, connectivity), min_depth)
    return lut[labels], int(lut.max())


@functools.lru_cache(maxsize=None)
def case_basins(name, connectivity):
    """The reference basins of a named case, computed once and shared (read-only): ``(basins, B, summits)``."""
    c = C.case(name)
    labels, count, summits = basins(c["objects"], c["surface"], connectivity)
    labels.setflags(write=False)
    return labels, count, summits


@functools.lru_cache(maxsize=None)
def case_saddles(name, connectivity):
    c = C.case(name)
    return saddles(c["objects"], case_basins(name, connectivity)[0], c["surface"], connectivity)
