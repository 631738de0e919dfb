"""A replay of the EDGES the labelling kernels unite (``csrc/label.hip``), on the host, against ``scipy.ndimage.label``.

The host twin unites a voxel with every preceding neighbour.  The kernels do not: the local launch makes the x runs of a tile
row from a ballot, the merge launch handles the edges that cross a tile face, and both leave out an edge where two edges that
are made imply it (``dx == 0``: the left neighbours of both ends are foreground; ``dx != 0``: the voxel at ``(dz, dy, 0)`` is).
Which edges that leaves is decided by integer rules only, so it can be checked without a card: this module restates those
rules in numpy over the tile shape the library exports, takes the connected components of exactly the edges the two launches
would unite (``scipy.sparse.csgraph``), numbers them by their lowest linear index -- what rooting every set at its smallest
index and counting the roots amounts to -- and compares with ``scipy.ndimage.label`` element for element, on every case of
``tests/label_cases.py``.  What it cannot check is the concurrency of the union-find; ``tests/test_label_gpu.py`` runs that.
"""

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import label_cases as C
from tests import label_ref as R

OFFSETS = [(dz, dy, dx) for dz in (-1, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
           if dz < 0 or (dz == 0 and (dy < 0 or (dy == 0 and dx < 0)))]            # the 13 preceding neighbours
assert len(OFFSETS) == 13


def _at(mask, d):
    """``out[v] = mask[v + d]``, False outside the volume."""
    z, y, x = mask.shape
    p = np.pad(mask, 1)
    return p[1 + d[0]:1 + d[0] + z, 1 + d[1]:1 + d[1] + y, 1 + d[2]:1 + d[2] + x]


def kernel_edges(mask, level):
    """``(sources, targets, made, left_out)``: linear indices of the edges the local and merge launches unite, how many they
    are, and how many foreground edges of the neighbourhood they leave out."""
    tz, ty, tx = C.T
    Z, Y, X = mask.shape
    index = np.arange(mask.size).reshape(mask.shape)
    lz, ly, lx = (c % t for c, t in zip(np.indices(mask.shape), C.T))
    left = (0, 0, -1)
    src, dst, left_out = [], [], 0

    def add(sel, d):
        src.append(index[sel])
        dst.append(index[sel] + (d[0] * Y + d[1]) * X + d[2])

    # local: the x runs inside a tile row (one ballot) ...
    add(mask & _at(mask, left) & (lx > 0), left)
    merge_rows = (lz == 0) | (ly == 0) | (ly == ty - 1)
    merge_active = merge_rows | (lx == 0) | (lx == tx - 1)
    for d in OFFSETS:
        if sum(1 for c in d if c) > level:
            continue
        dz, dy, dx = d
        both = mask & _at(mask, d)
        inside = (lz + dz >= 0) & (ly + dy >= 0) & (ly + dy < ty) & (lx + dx >= 0) & (lx + dx < tx)       # target in the same tile
        if dx == 0:
            implied = _at(mask, left) & _at(mask, (dz, dy, -1))          # the left neighbours of both ends
            implied_local, implied_merge = implied & (lx > 0), implied          # (merge asks x > 0: _at is False outside)
        else:
            implied_local = implied_merge = _at(mask, (dz, dy, 0))
        # ... and the other 12 offsets inside the tile
        if d != left:
            add(both & inside & ~implied_local, d)
            left_out += int((both & inside & implied_local).sum())
        # merge: the edges that cross a tile face; an x edge is never left out
        crosses = both & ~inside & merge_active
        assert np.array_equal(crosses, both & ~inside), "a crossing edge starts at a voxel the merge launch does not visit"
        if d == left:
            add(crosses, d)
        else:
            add(crosses & ~implied_merge, d)
            left_out += int((crosses & implied_merge).sum())
    s, t = np.concatenate(src), np.concatenate(dst)
    return s, t, len(s), left_out


def replay(vol, threshold, connectivity):
    with np.errstate(invalid="ignore"):
        mask = np.asarray(vol) > np.float32(threshold)
    s, t, made, left_out = kernel_edges(mask, R.LEVEL[connectivity])
    n = mask.size
    _, comp = connected_components(coo_matrix((np.ones(len(s), dtype=np.int8), (s, t)), shape=(n, n)), directed=False)
    flat = mask.ravel()
    # number the components by their lowest linear index: the first voxel of a component in raster order is its root
    first = np.full(comp.max() + 1, n, dtype=np.int64)
    fg = np.flatnonzero(flat)
    np.minimum.at(first, comp[fg], fg)
    roots = np.sort(first[first < n])
    labels = np.zeros(n, dtype=np.int32)
    labels[fg] = np.searchsorted(roots, first[comp[fg]]) + 1
    return labels.reshape(mask.shape), len(roots), made, left_out


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_the_edges_the_kernels_unite_give_scipys_labels(name, connectivity):
    case = C.case(name)
    want, n_want = R.case_labels(name, connectivity)
    got, n, made, left_out = replay(case["vol"], case["threshold"], connectivity)
    print(f"{name}-{connectivity}: {made} edges united, {left_out} left out as implied")
    assert n == n_want and np.array_equal(got, want)


def test_the_rule_leaves_edges_out_where_it_should_and_only_there():
    # all foreground: the runs take the x edges inside the tiles, and of the others all but the first columns' are implied
    vol = C.case("all_fg")["vol"]
    for k in C.CONNECTIVITIES:
        _, n, made, left_out = replay(vol, 0.5, k)
        assert n == 1 and left_out > made
    # the checkerboard under 6 has no edge at all, and nothing to leave out
    board = C.case("checkerboard")["vol"]
    assert replay(board, 0.5, 6)[2:] == (0, 0)
    # an edge is left out only if the two that imply it are foreground: a lone diagonal pair is always united
    for name in C.NAMES:
        if name.startswith("pair_"):
            assert replay(C.case(name)["vol"], 0.5, 26)[2:] == (1, 0), name
