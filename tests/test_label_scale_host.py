"""Labelling AT SCALE on the host (``tests/label_scale_cases.py``): that every case crosses what it says it crosses, asserted from
the exported launch geometry; that no case holds a long component (the rule of the cases module: the GPU tests rely on it);
the twin against ``scipy.ndimage.label`` element for element at these sizes; ``label_ref.filter_labels`` and the twins of the
table, the relabelling and the expansion on what the GPU tests compare the kernels with.
"""

import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import segment as S
from tests import label_cases as SMALL
from tests import label_ref as R
from tests import label_scale_cases as C
from tests import test_label_host as H


def test_the_cases_cross_the_caps_and_the_scan_edges():
    T, CH, SC, B, TB = C.G
    assert C.G == S.launch_geometry() and min(C.G) >= 1 and CH % T == 0
    assert (C.TZ, C.TY, C.TX) == S.tile_shape()
    x = {name: C.crossings(name) for name in C.NAMES}
    # what the small cases never reach: one count per scan thread, and not all threads busy
    small = max(c["vol"].size for c in SMALL.CASES)
    assert C.ceil_div(small, CH) < SC and C.ceil_div(small, T) < B
    # scan_exact: per == 1 with every scan thread busy; scan_plus_one: per == 2, thread S / 2 holds one count, the rest none
    assert x["scan_exact"]["blocks"] == SC and x["scan_exact"]["per"] == 1
    assert x["scan_plus_one"]["blocks"] == SC + 1 and x["scan_plus_one"]["per"] == 2
    per, blocks = 2, SC + 1
    held = [max(0, min(blocks, per * (t + 1)) - min(blocks, per * t)) for t in range(SC)]
    assert held[:SC // 2] == [2] * (SC // 2) and held[SC // 2] == 1 and not any(held[SC // 2 + 1:])
    for name in ("scan_exact", "scan_plus_one"):
        assert all(n % t for n, t in zip(C.shape(name), (C.TZ, C.TY, C.TX))), "no extent is a multiple of the tile's"
        assert x[name]["units"] <= B and x[name]["voxel_groups"] <= B and x[name]["tiles"] <= TB      # nothing else is crossed there
    # merge_wrap: more (row, piece) units than B with one piece per row; merge_wrap_pieces: with two
    assert x["merge_wrap"]["units"] > B and x["merge_wrap"]["pieces"] == 1 and x["merge_wrap"]["voxel_groups"] <= B
    assert x["merge_wrap_pieces"]["units"] > B and x["merge_wrap_pieces"]["pieces"] == 2 and x["merge_wrap_pieces"]["voxel_groups"] <= B
    assert C.shape("merge_wrap_pieces")[2] % T, "the second piece of a row is partial"
    # voxel_wrap: flatten, final, regions, remap and expand go round
    assert x["voxel_wrap"]["voxel_groups"] > B and x["voxel_wrap"]["tiles"] <= TB
    # tile_wrap: the local launch goes round, with a partial last tile, and the merge launch has a unit per voxel
    assert x["tile_wrap"]["tiles"] == TB + 2 > TB and C.shape("tile_wrap")[0] % C.TZ and x["tile_wrap"]["units"] == x["tile_wrap"]["n"] > B
    # ... and each is past the scan's first edge by the `per` the module's docstring names (2, 3, 5, 5 with today's numbers)
    for name in ("merge_wrap", "merge_wrap_pieces", "voxel_wrap", "tile_wrap"):
        assert x[name]["per"] >= 2 and x[name]["per"] * (SC - 1) > x[name]["blocks"], "the last scan threads begin past the counts"
    if C.G == (256, 4096, 1024, 1 << 16, 1 << 22) and C.TZ == 4:
        assert C.shapes() == {"scan_exact": (9, 70, 6652), "scan_plus_one": (9, 70, 6658), "merge_wrap": (33, 2000, 70),
                              "merge_wrap_pieces": (2, 17000, 260), "voxel_wrap": (65, 2000, 130), "tile_wrap": (2 ** 24 + 5, 1, 1)}
        assert [x[n]["per"] for n in ("merge_wrap", "merge_wrap_pieces", "voxel_wrap", "tile_wrap")] == [2, 3, 5, 5]
    # the column: runs of 7 behind gaps of 4 start at every phase of the tile's z edge
    column = C.case("tile_wrap")["vol"].ravel() > 0.5
    starts = np.flatnonzero(column[1:] & ~column[:-1])[:64] + 1
    assert set((starts % C.TZ).tolist()) == set(range(C.TZ)) and column[:7].all() and not column[7:11].any()
    # one scratch buffer of the small tests' size serves every case
    assert max(_lib.call_value("lsr_label_scratch_bytes", *C.shape(name)) for name in C.NAMES) <= 1 << 16


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_no_case_holds_a_long_component_and_the_arithmetic_at_size_is_met(name, connectivity):
    labels, n, largest = C.case_labels(name, connectivity)
    assert 0 < largest < C.MAX_COMPONENT
    T, CH, SC, B, TB = C.G
    roots = np.flatnonzero(np.diff(np.concatenate([[0], np.maximum.accumulate(labels.ravel())])))      # each component's first voxel
    assert len(roots) == n
    if name in ("voxel_wrap", "tile_wrap"):
        assert roots[-1] // CH >= SC, "roots in chunk S and later"
        assert labels.ravel()[B * T:].any(), "... and foreground beyond the first trip of the voxel walks"
    if name == "voxel_wrap":
        assert roots[-1] >= B * T, "... roots among it"
    if (name, connectivity) in (("voxel_wrap", 6), ("tile_wrap", 6)):
        assert n > 10 ** 6, "more than a million -(rank + 2) encodings"
    assert n > 4 * CH, "rank offsets far beyond a few thousand"


@pytest.mark.parametrize("name,connectivity", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_equals_scipy_label_at_scale(name, connectivity):
    case = C.case(name)
    want, n_want, _ = C.case_labels(name, connectivity)
    got, n, guard = H.twin_label(case["vol"], case["thresholds"][connectivity], connectivity)
    assert np.all(guard == H.FILL), "the twin wrote behind its output"
    assert not np.any(got == H.FILL), "a voxel was not written"
    assert n == n_want
    assert np.array_equal(got, want)


def test_filter_labels_at_this_size():
    """1.45 million objects: the restatement against its own rule stated once more, and the twin of the relabelling against it."""
    labels, n, _ = C.case_labels("voxel_wrap", 6)
    volume = np.bincount(labels.ravel(), minlength=n + 1)
    want, m = R.filter_labels(labels, 2, False)
    kept = volume >= 2
    kept[0] = False
    assert m == int(kept.sum()) and 0 < m < n
    assert np.array_equal(want > 0, kept[labels])
    old_of_new = np.flatnonzero(kept)                                     # the kept labels keep their order
    assert np.array_equal(old_of_new[want[want > 0] - 1], labels[want > 0])
    work = torch.from_numpy(np.array(labels))
    got, table, m_got = S.filter_objects(work, S.region_table(work, n), 2, False)
    assert m_got == m and np.array_equal(got.numpy(), want) and np.array_equal(table["volume"], volume[kept])
    one, m1 = R.filter_labels(labels, 0, True)
    assert m1 == 1 and np.array_equal(one > 0, labels == int(np.argmax(volume[1:])) + 1)


def test_twins_on_the_synthetic_labels_table_filter_and_expansion():
    labels, n = C.synthetic_labels()
    zs, ys, xs = labels.shape
    assert n == C.N_SYNTHETIC == 13 * 4 and labels.shape == C.shape("voxel_wrap")
    edge = C.B * C.T                                                      # where the voxel walks begin their second trip
    past = np.unique(labels.ravel()[edge:])
    past = past[past > 0]
    assert len(past) >= 2 and all(np.any(labels.ravel()[:edge] == k) for k in past), "objects with voxels on both sides of voxel B T"
    # label_ref's premise: a float32 times a coordinate is exact in float64 -- 24 significant bits times fewer than 2^11
    assert max(labels.shape) <= 2 ** 11
    want = C.synthetic_table()
    t_labels, t_inten = torch.from_numpy(np.array(labels)), torch.from_numpy(np.array(C.synthetic_intensity()))
    worst = R.check_table(S.region_table(t_labels, n, t_inten), want)
    print(f"synthetic: {n} objects, worst float64 sum error / bound = {worst:.3f}")
    plain = S.region_table(t_labels, n)
    R.check_table(plain, {k: want[k] for k in C.PLAIN_KEYS})
    for min_volume, keep_largest in filter_params(want["volume"]):
        work = t_labels.clone()
        got, _, m = S.filter_objects(work, plain, min_volume, keep_largest)
        ref, m_want = R.filter_labels(labels, min_volume, keep_largest)
        assert m == m_want and 0 < m < n and np.array_equal(got.numpy(), ref)
    # the expansion: offsets 0 and 1 along x are admitted, 2 is refused
    nearest = C.expand_nearest()
    ref = C.expand_restatement(labels, nearest, C.EXPAND_SAMPLING, C.EXPAND_DISTANCE)
    x = np.arange(xs)
    assert np.array_equal(ref[..., x % 3 < 2], labels[..., (x - x % 3)[x % 3 < 2]]) and not ref[..., x % 3 == 2].any()
    assert ref.any() and np.any(ref != labels)
    out = np.full(labels.size + H.GUARD, H.FILL, dtype=np.int32)
    _lib.call("lsr_label_expand_i32_cpu", labels.ctypes.data, nearest.ctypes.data, zs, ys, xs, (ctypes.c_double * 3)(*C.EXPAND_SAMPLING),
              ctypes.c_double(C.EXPAND_DISTANCE), out.ctypes.data, None)
    assert np.all(out[labels.size:] == H.FILL) and np.array_equal(out[:labels.size].reshape(labels.shape), ref)


def filter_params(volumes):
    """``(min_volume, keep_largest)`` of the filter on the synthetic labels, from the reference's volumes: the median drops about
    half of the objects, and the largest alone."""
    return [(int(np.median(volumes)), False), (0, True)]
