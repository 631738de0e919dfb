"""The distance transform on the host: the twins (``lsr_edt_f32_cpu``, ``lsr_edt_labels_i32_cpu``, ``lsr_label_expand_i32_cpu``)
against ``tests/edt_ref.py`` -- distances against ``scipy.ndimage.distance_transform_edt`` (bit for bit under the exact samplings,
within one float32 ulp under (0.4, 0.116, 0.116), no voxel excluded), ``nearest`` against a brute-force search (the tie rule:
the smallest linear index) --, the entry statuses of twin and device entry alike, ``shrimpy_amd.distance`` on CPU tensors, the
two distance settings of ``segment_zyx`` and of the ``segment`` command.

Cases: ``tests/edt_cases.py``, sized from the exported tiling.  Measured on the host twin, every case and sampling: 0 ulp.
"""

import csv
import ctypes

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch
import yaml

from shrimpy_amd import _lib
from shrimpy_amd import distance as D
from shrimpy_amd import segment as S
from shrimpy_amd.settings import SegmentSettings
from tests import edt_cases as C
from tests import edt_ref as R
from tests import label_ref as LR
from tests import test_label_host as LH

GUARD = 64
FILL_I = -7
FILL_F = np.float32(-7.5)


def scratch_bytes_of_the_cases():
    return max(_lib.call_value("lsr_edt_scratch_bytes", *c["vol"].shape) for c in C.CASES)


# one scratch buffer for every call of this module, never cleared between them (and poisoned to begin with)
SCRATCH = np.full(scratch_bytes_of_the_cases(), 0xA5, dtype=np.uint8)


def _c3(sampling):
    return (ctypes.c_double * 3)(*sampling)


def twin_edt(vol, threshold, invert, sampling, want_dist=True, want_nearest=True, labels=False):
    """A twin through the C ABI into poisoned buffers with 64 guard words behind each: (dist, nearest, guards).  ``labels``:
    ``vol`` is an int32 label volume and the entry ``lsr_edt_labels_i32_cpu``."""
    vol = np.ascontiguousarray(vol, dtype=np.int32 if labels else np.float32)
    z, y, x = vol.shape
    assert 0 < _lib.call_value("lsr_edt_scratch_bytes", z, y, x) <= SCRATCH.nbytes
    dist = np.full(vol.size + GUARD, FILL_F, dtype=np.float32)
    nearest = np.full(vol.size + GUARD, FILL_I, dtype=np.int32)
    head = () if labels else (ctypes.c_float(threshold),)
    _lib.call("lsr_edt_labels_i32_cpu" if labels else "lsr_edt_f32_cpu", vol.ctypes.data, z, y, x, *head, int(invert), _c3(sampling),
              dist.ctypes.data if want_dist else None, nearest.ctypes.data if want_nearest else None, SCRATCH.ctypes.data, None)
    return dist[:vol.size].reshape(vol.shape), nearest[:vol.size].reshape(vol.shape), (dist[vol.size:], nearest[vol.size:])


def check_buffers(dist, nearest, guards):
    assert np.all(guards[0] == FILL_F) and np.all(guards[1] == FILL_I), "something was written behind an output"
    assert not np.any(dist == FILL_F) and not np.any(nearest == FILL_I), "a voxel was not written"


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))            # (a copy: the shared cases and references are read-only)


# ---- the twin against scipy and the brute force ---------------------------------------------------------------------------------


@pytest.mark.parametrize("name,sampling,invert", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_equals_the_oracles(name, sampling, invert):
    case = C.case(name)
    dist, nearest, guards = twin_edt(case["vol"], case["threshold"], invert, sampling)
    check_buffers(dist, nearest, guards)
    R.check(name, sampling, invert, dist, nearest)
    again = twin_edt(case["vol"], case["threshold"], invert, sampling)
    assert dist.tobytes() == again[0].tobytes() and nearest.tobytes() == again[1].tobytes()


def test_the_cases_aim_at_the_tiling():
    assert (C.CHUNK, C.TILE) == (64, 256) and C.ROWS_AT_ONCE % 4 == 0 and C.LINES_AT_ONCE % C.TILE == 0
    assert [C.case(f"extent_x{x}")["vol"].shape[2] for x in C.X_EXTENTS] == [1, 63, 64, 65, 135]
    assert [C.case(f"extent_y{y}")["vol"].shape[1] for y in C.LINE_EXTENTS] == [1, 2, C.TILE + 1]
    assert [C.case(f"extent_z{z}")["vol"].shape[0] for z in C.LINE_EXTENTS] == [1, 2, C.TILE + 1]
    z, y, x = C.case("second_rows")["vol"].shape
    assert z * y > C.ROWS_AT_ONCE
    z, y, x = C.case("second_lines_y")["vol"].shape
    assert z * x > C.LINES_AT_ONCE and y > 1
    z, y, x = C.case("second_lines_z")["vol"].shape
    assert y * x > C.LINES_AT_ONCE and z > 1
    z, y, x = C.case("noise_p0.5")["vol"].shape                       # more than one workgroup of lines in both passes
    assert z * x > C.TILE and y * x > C.TILE and z * y * x <= C.BRUTE_VOXELS
    assert max(c["vol"].size for c in C.CASES if not c["name"].startswith("second_")) <= 60000
    for k in range(8):                                                 # one site, in each corner in turn
        name = "corner_" + format(k, "03b")
        site = C.sites(name, False)
        assert site.sum() == 1 and site[tuple(-int(c) for c in format(k, "03b"))]
    assert not C.sites("no_site", False).any() and C.sites("all_sites", False).all()
    assert C.sites("one_plane", False)[[0, 1, 3, 4]].sum() == 0 and C.sites("one_plane", False)[2].any()
    # every voxel of the checkerboard and the middle planes of the mirrored cases have tied candidates
    for name in ("checkerboard", "mirror_corners", "mirror_pairs"):
        site = C.sites(name, False)
        pos = np.argwhere(site)
        vox = np.argwhere(~site)[:: max(1, (~site).sum() // 50)]
        sq = ((vox[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)
        tied = (sq == sq.min(axis=1, keepdims=True)).sum(axis=1)
        assert (tied > 1).any() if name != "checkerboard" else (tied > 1).all(), name


def test_the_tie_rule_differs_from_scipys_indices():
    """The reason the index oracle is the brute force: scipy's ``return_indices`` takes other sites among equals."""
    site = C.sites("checkerboard", False)
    _, idx = ndi.distance_transform_edt(~site, return_indices=True)
    lin = (idx[0] * site.shape[1] + idx[1]) * site.shape[2] + idx[2]
    mine = R.case_nearest("checkerboard", (1.0, 1.0, 1.0), False)
    assert (lin != mine).any() and np.all(mine <= lin)


def test_threshold_semantics_by_hand():
    vol = np.array([[[0.0, np.nan, np.inf, -np.inf, -0.0, 1e-45, 1.0, 0.0, 2.0]]], dtype=np.float32)
    dist, nearest, _ = twin_edt(vol, 0.0, False, (1, 1, 1))             # sites: !(v > 0) -- NaN and the threshold itself
    assert dist.ravel().tolist() == [0, 0, 1, 0, 0, 1, 1, 0, 1] and nearest.ravel().tolist() == [0, 1, 1, 3, 4, 4, 7, 7, 7]
    dist, nearest, _ = twin_edt(vol, 0.0, True, (1, 1, 1))              # sites: v > 0
    assert dist.ravel().tolist() == [2, 1, 0, 1, 1, 0, 0, 1, 0] and nearest.ravel().tolist() == [2, 2, 2, 2, 5, 5, 6, 6, 8]
    dist, nearest, _ = twin_edt(vol, float("nan"), True, (1, 1, 1))     # nothing is greater than NaN: no site
    assert np.all(np.isposinf(dist)) and np.all(nearest == -1)
    labels = np.array([[[0, 3, 0, 0, -2, 0]]], dtype=np.int32)
    dist, nearest, _ = twin_edt(labels, None, False, (1, 1, 0.5), labels=True)          # sites: labels != 0
    assert dist.ravel().tolist() == [0.5, 0, 0.5, 0.5, 0, 0.5] and nearest.ravel().tolist() == [1, 1, 1, 4, 4, 4]
    dist, nearest, _ = twin_edt(labels, None, True, (1, 1, 0.5), labels=True)           # sites: labels == 0
    assert dist.ravel().tolist() == [0, 0.5, 0, 0, 0.5, 0] and nearest.ravel().tolist() == [0, 0, 2, 3, 3, 5]


@pytest.mark.parametrize("name", ["noise_p0.9", "checkerboard", "threshold_semantics"])
def test_the_label_entry_equals_the_float_entry(name):
    case, labels = C.case(name), C.label_volume(name)
    for invert in (False, True):
        for sampling in ((1.5, 0.5, 0.25), C.INEXACT):
            # labels != 0 is the case's foreground: the label entry's sites are the float entry's with the other `invert`
            want = twin_edt(case["vol"], case["threshold"], not invert, sampling)
            got = twin_edt(labels, None, invert, sampling, labels=True)
            check_buffers(*got)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            R.check(name, sampling, not invert, got[0], got[1])


def test_a_null_output_leaves_the_other_unchanged():
    case = C.case("noise_p0.9")
    both = twin_edt(case["vol"], case["threshold"], False, C.INEXACT)
    only_dist = twin_edt(case["vol"], case["threshold"], False, C.INEXACT, want_nearest=False)
    only_nearest = twin_edt(case["vol"], case["threshold"], False, C.INEXACT, want_dist=False)
    assert only_dist[0].tobytes() == both[0].tobytes() and np.all(only_dist[1] == FILL_I) and np.all(only_dist[2][0] == FILL_F)
    assert only_nearest[1].tobytes() == both[1].tobytes() and np.all(only_nearest[0] == FILL_F) and np.all(only_nearest[2][1] == FILL_I)


# ---- label expansion ------------------------------------------------------------------------------------------------------------------


def expand_cases():
    """(name, labels, sampling, distance) of the label-expansion tests; the volumes are small enough for the brute force."""
    gap = np.zeros((1, 3, 9), dtype=np.int32)                # labels 7 and 3 at equal distance from the voxels between them
    gap[0, :, 2], gap[0, :, 6] = 7, 3
    rng = np.random.default_rng(11)
    blobs = np.zeros((5, 12, CHUNK_PLUS), dtype=np.int32)
    for k in range(1, 9):
        z, y, x = (int(rng.integers(0, n)) for n in blobs.shape)
        blobs[z:z + 2, y:y + 3, x:x + 4] = k
    return [("equal_distance", gap, (1.0, 1.0, 1.0), 2.0), ("zero", blobs, (1.0, 1.0, 1.0), 0.0),
            ("beyond_the_volume", blobs, (1.0, 1.0, 1.0), 1e6), ("anisotropic", blobs, (2.0, 0.5, 0.25), 1.75),
            ("inexact_sampling", blobs, C.INEXACT, 0.5), ("no_label", np.zeros((2, 3, 4), dtype=np.int32), (1.0, 1.0, 1.0), 3.0)]


CHUNK_PLUS = C.CHUNK + 6
EXPAND_CASES = expand_cases()


def twin_expand(labels, nearest, sampling, distance):
    out = np.full(labels.size + GUARD, FILL_I, dtype=np.int32)
    z, y, x = labels.shape
    _lib.call("lsr_label_expand_i32_cpu", labels.ctypes.data, nearest.ctypes.data, z, y, x, _c3(sampling), ctypes.c_double(distance),
              out.ctypes.data, None)
    assert np.all(out[labels.size:] == FILL_I) and not np.any(out[:labels.size] == FILL_I)
    return out[:labels.size].reshape(labels.shape)


@pytest.mark.parametrize("name,labels,sampling,distance", EXPAND_CASES, ids=[c[0] for c in EXPAND_CASES])
def test_twin_expansion_equals_the_restatement(name, labels, sampling, distance):
    want_nearest = R.brute_nearest(labels != 0, sampling)
    _, nearest, _ = twin_edt(labels, None, False, sampling, want_dist=False, labels=True)
    if sampling in C.EXACT or sampling == (2.0, 0.5, 0.25):
        assert np.array_equal(nearest, want_nearest)
    want = R.expand(labels, want_nearest if sampling != C.INEXACT else nearest, sampling, distance)
    got = twin_expand(labels, nearest, sampling, distance)
    assert np.array_equal(got, want)
    assert np.array_equal(got[labels != 0], labels[labels != 0]), "a labelled voxel changed"
    assert np.array_equal(D.expand_labels(_t(labels), distance, sampling).numpy(), want)
    if name == "equal_distance":
        assert got[0, 1].tolist() == [7, 7, 7, 7, 7, 3, 3, 3, 3]        # x = 4 is tied: label 7's voxel has the smaller index
    if name == "zero":
        assert np.array_equal(got, labels)
    if name == "beyond_the_volume":
        assert got.all()
    if name == "no_label":
        assert not got.any()


# ---- entry statuses -----------------------------------------------------------------------------------------------------------------


def test_entry_statuses():
    lib = _lib.load()
    four = (ctypes.c_int * 4)()
    assert lib.lsr_edt_tiling(four) == 0 and tuple(four) == D.tiling() and lib.lsr_edt_tiling(None) == -1
    assert lib.lsr_edt_scratch_bytes(4, 5, 6) == 256 * 5 * 12
    assert lib.lsr_edt_scratch_bytes(0, 5, 6) == -2 and lib.lsr_edt_scratch_bytes(2 ** 11, 2 ** 10, 2 ** 10) == -3
    big = lib.lsr_edt_scratch_bytes(171, 2048, 2270)                    # the config-2 deskewed grid: past 2^31 bytes
    assert big == C.LINES_AT_ONCE * 2048 * 12 and big > 2 ** 31
    vol = np.ones((2, 3, 4), dtype=np.float32)
    labels = np.ones((2, 3, 4), dtype=np.int32)
    dist = np.full(24, FILL_F, dtype=np.float32)
    near = np.full(24, FILL_I, dtype=np.int32)
    v, lb, d, n, s = vol.ctypes.data, labels.ctypes.data, dist.ctypes.data, near.ctypes.data, SCRATCH.ctypes.data
    thr, unit = ctypes.c_float(0.5), _c3((1, 1, 1))
    bad_samplings = [(0.0, 1, 1), (1, -1.0, 1), (1, 1, float("nan")), (float("inf"), 1, 1), (1, 1, -float("inf"))]

    def common(fn, src, head):                                  # (checked before anything is launched: safe without a GPU)
        assert fn(None, 2, 3, 4, *head, 0, unit, d, n, s, None) == -1
        assert fn(src, 2, 3, 4, *head, 0, None, d, n, s, None) == -1
        assert fn(src, 2, 3, 4, *head, 0, unit, None, None, s, None) == -1 and b"both NULL" in lib.lsr_last_error()
        assert fn(src, 2, 3, 4, *head, 0, unit, d, n, None, None) == -1 and b"scratch is NULL" in lib.lsr_last_error()
        assert fn(src, 0, 3, 4, *head, 0, unit, d, n, s, None) == -2
        assert fn(src, 2, -3, 4, *head, 0, unit, d, n, s, None) == -2
        assert fn(src, 2, 3, 0, *head, 0, unit, d, n, s, None) == -2
        assert fn(src, 2 ** 11, 2 ** 10, 2 ** 10, *head, 0, unit, d, n, s, None) == -3          # 2^31 voxels: one too many
        assert fn(src, 2 ** 40, 2 ** 40, 2 ** 40, *head, 0, unit, d, n, s, None) == -3
        for bad in bad_samplings:
            assert fn(src, 2, 3, 4, *head, 0, _c3(bad), d, n, s, None) == -4 and b"sampling" in lib.lsr_last_error()
        assert fn(src, 0, 3, 4, *head, 0, _c3(bad_samplings[0]), d, n, s, None) == -2          # the shape is checked first

    for name in ("lsr_edt_f32_cpu", "lsr_edt_f32"):
        common(getattr(lib, name), v, (thr,))
    for name in ("lsr_edt_labels_i32_cpu", "lsr_edt_labels_i32"):
        common(getattr(lib, name), lb, ())
    # the timing entry of tools/bench_kernels.py --edt: lsr_edt_f32's checks, then its own pointer
    ms3 = (ctypes.c_float * 3)(*([-1.0] * 3))
    fn = lib.lsr_edt_profile_f32
    assert fn(None, 2, 3, 4, thr, 0, unit, d, n, s, ms3, None) == -1 and fn(v, 2, 3, 4, thr, 0, unit, None, None, s, ms3, None) == -1
    assert fn(v, 2, 0, 4, thr, 0, unit, d, n, s, ms3, None) == -2 and fn(v, 2 ** 11, 2 ** 10, 2 ** 10, thr, 0, unit, d, n, s, ms3, None) == -3
    assert fn(v, 2, 3, 4, thr, 0, _c3((1, 0, 1)), d, n, s, ms3, None) == -4
    assert fn(v, 2, 3, 4, thr, 0, unit, d, n, s, None, None) == -1 and b"ms3 is NULL" in lib.lsr_last_error()
    assert list(ms3) == [-1.0] * 3
    out = np.full(24, FILL_I, dtype=np.int32)
    o, two = out.ctypes.data, ctypes.c_double(2.0)
    for name in ("lsr_label_expand_i32_cpu", "lsr_label_expand_i32"):
        fn = getattr(lib, name)
        assert fn(None, n, 2, 3, 4, unit, two, o, None) == -1 and fn(lb, None, 2, 3, 4, unit, two, o, None) == -1
        assert fn(lb, n, 2, 3, 4, None, two, o, None) == -1 and fn(lb, n, 2, 3, 4, unit, two, None, None) == -1
        assert fn(lb, n, 2, 3, 0, unit, two, o, None) == -2 and fn(lb, n, 2 ** 11, 2 ** 10, 2 ** 10, unit, two, o, None) == -3
        for bad in bad_samplings:
            assert fn(lb, n, 2, 3, 4, _c3(bad), two, o, None) == -4
        assert fn(lb, n, 2, 3, 4, unit, ctypes.c_double(-0.5), o, None) == -4 and b"distance" in lib.lsr_last_error()
        assert fn(lb, n, 2, 3, 4, unit, ctypes.c_double(float("nan")), o, None) == -4
        assert fn(lb, n, 2, 3, 4, unit, two, lb, None) == -4 and b"alias" in lib.lsr_last_error()
    assert np.all(dist == FILL_F) and np.all(near == FILL_I) and np.all(out == FILL_I) and np.all(labels == 1), "a refused call wrote something"
    assert lib.lsr_edt_f32_cpu(v, 2, 3, 4, thr, 1, unit, d, n, s, None) == 0 and np.all(dist == 0) and near.tolist() == list(range(24))


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------


def test_distance_functions_on_cpu_tensors():
    case = C.case("noise_p0.9")
    for sampling in ((2.0, 1.0, 1.0), C.INEXACT):
        dist, nearest = D.distance_transform(_t(case["vol"]), case["threshold"], sampling, return_indices=True)
        assert dist.dtype == torch.float32 and nearest.dtype == torch.int32 and dist.device.type == "cpu" and dist.shape == case["vol"].shape
        R.check("noise_p0.9", sampling, False, dist.numpy(), nearest.numpy())
        alone = D.distance_transform(_t(case["vol"]), case["threshold"], sampling)
        assert isinstance(alone, torch.Tensor) and alone.numpy().tobytes() == dist.numpy().tobytes()
        inv = D.distance_transform(_t(case["vol"]), case["threshold"], sampling, invert=True)
        assert inv.numpy().tobytes() == R.case_edt("noise_p0.9", sampling, True).tobytes() or sampling == C.INEXACT
        labels = _t(C.label_volume("noise_p0.9"))
        got = D.distance_transform_labels(labels, sampling, invert=True)          # the depth inside the objects
        assert got.numpy().tobytes() == dist.numpy().tobytes()
    assert D.distance_transform(_t(case["vol"]), case["threshold"]).numpy().tobytes() == R.case_edt("noise_p0.9", (1.0, 1.0, 1.0), False).tobytes()
    with pytest.raises(TypeError):
        D.distance_transform(_t(case["vol"].astype(np.float64)), 0.5)
    with pytest.raises(TypeError):
        D.distance_transform_labels(_t(case["vol"]))
    with pytest.raises(ValueError):
        D.distance_transform(_t(case["vol"][0]), 0.5)
    for bad in ((1, 1), (1, 0, 1), (1, 1, float("nan")), (-1, 1, 1)):
        with pytest.raises(ValueError):
            D.distance_transform(_t(case["vol"]), 0.5, sampling=bad)
    with pytest.raises(ValueError):
        D.expand_labels(_t(C.label_volume("noise_p0.9")), -1.0)
    with pytest.raises(ValueError):
        D.expand_labels(_t(C.label_volume("noise_p0.9")), float("nan"))


# ---- segment_zyx and the command ----------------------------------------------------------------------------------------------------

SAMPLING = LH.SCALE[2:]                  # (0.5, 0.25, 0.25): the positions' (z, y, x) scale
EXPAND = 0.75                            # micrometres: three voxels along y and x, one along z


def reference_expansion(vol, settings, sampling, distance):
    """(labels before the expansion, labels after it): the restated rule on the reference segmentation."""
    before, m, _ = LH.reference_segmentation(vol, settings)
    return before, R.expand(before, R.brute_nearest(before != 0, sampling), sampling, distance), m


def reference_radius(labels, m, sampling):
    depth = ndi.distance_transform_edt(labels > 0, sampling=sampling).astype(np.float32)
    return np.array([depth[labels == k].max() for k in range(1, m + 1)], dtype=np.float32)


def check_segment_zyx(device):
    """Shared with tests/test_edt_gpu.py: the two distance settings of ``segment_zyx`` on ``device``."""
    vol = LH.blob_volume(5)
    d_vol = _t(vol).to(device)
    plain, table0, n0 = S.segment_zyx(d_vol, SegmentSettings(**LH.SETTINGS))
    again, table1, n1 = S.segment_zyx(d_vol, SegmentSettings(**LH.SETTINGS), sampling=SAMPLING)      # the defaults change nothing
    want0, m, n_before = LH.reference_segmentation(vol, LH.SETTINGS)
    assert n0 == n1 == m == 3 and n_before > 3 and np.array_equal(plain.cpu().numpy(), want0) and np.array_equal(again.cpu().numpy(), want0)
    assert sorted(table0) == sorted(table1) and "inscribed_radius" not in table0
    # the inscribed radius of the unexpanded objects
    labels, table, n = S.segment_zyx(d_vol, SegmentSettings(**LH.SETTINGS, inscribed_radius=True), sampling=SAMPLING)
    assert n == 3 and np.array_equal(labels.cpu().numpy(), want0)
    assert table["inscribed_radius"].dtype == np.float32
    assert table["inscribed_radius"].tobytes() == reference_radius(want0, 3, SAMPLING).tobytes()
    assert np.array_equal(table["volume"], table0["volume"])
    # the expansion: after the filter (the debris that passes the threshold claims no space), the table of the grown labels
    before, want, m = reference_expansion(vol, LH.SETTINGS, SAMPLING, EXPAND)
    assert (want != 0).sum() > (before != 0).sum()
    unfiltered = dict(LH.SETTINGS, min_volume=0)
    _, grown_debris, m_all = reference_expansion(vol, unfiltered, SAMPLING, EXPAND)
    assert m_all > 3 and (grown_debris != 0).sum() > (want != 0).sum(), "the debris must be there to claim space if it were kept"
    labels, table, n = S.segment_zyx(d_vol, SegmentSettings(**LH.SETTINGS, expand_distance=EXPAND, inscribed_radius=True),
                                     sampling=SAMPLING)
    assert n == 3 and labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want)
    LR.check_table({k: v for k, v in table.items() if k != "inscribed_radius"}, LR.table(want, 3, vol))
    assert np.array_equal(table["volume"], np.bincount(want.ravel(), minlength=4)[1:])
    assert table["inscribed_radius"].tobytes() == reference_radius(want, 3, SAMPLING).tobytes()
    # unit sampling is the default
    labels, _, _ = S.segment_zyx(d_vol, SegmentSettings(**LH.SETTINGS, expand_distance=2.0))
    assert np.array_equal(labels.cpu().numpy(), reference_expansion(vol, LH.SETTINGS, (1.0, 1.0, 1.0), 2.0)[1])
    empty, table, n = S.segment_zyx(_t(np.full((3, 4, 5), 7.0, dtype=np.float32)).to(device),
                                    SegmentSettings(**LH.SETTINGS, expand_distance=2.0, inscribed_radius=True))
    assert n == 0 and not empty.any() and len(table["inscribed_radius"]) == 0


def test_segment_zyx_distance_settings_on_the_host():
    check_segment_zyx(torch.device("cpu"))


def test_settings():
    s = SegmentSettings(channel_name="GFP", threshold=1.0)
    assert s.inscribed_radius is False and s.expand_distance == 0.0
    assert "expand_labels" in SegmentSettings.__doc__ and "inscribed_radius_um" in SegmentSettings.__doc__
    assert SegmentSettings(channel_name="GFP", threshold=1.0, expand_distance=2, inscribed_radius=True).expand_distance == 2.0
    for bad in (dict(expand_distance=-0.5), dict(inscribed_radius="maybe"), dict(expand_distance="far")):
        with pytest.raises(ValueError):
            SegmentSettings(**{"channel_name": "GFP", "threshold": 1.0, **bad})


def check_segment_command(cli, tmp_path):
    """Shared with tests/test_edt_gpu.py: the ``segment`` command with the two distance settings on a temporary store."""
    from click.testing import CliRunner

    from shrimpy_amd.cli import OBJECT_COLUMNS
    from shrimpy_amd.io.omezarr import open_ome_zarr

    vols = LH.make_store(tmp_path / "in.zarr")

    def run(name, settings):
        cfg = tmp_path / f"{name}.yml"
        cfg.write_text(yaml.safe_dump(settings))
        r = CliRunner().invoke(cli.cli, ["segment", "-i", str(tmp_path / "in.zarr"), "-c", str(cfg), "-o", str(tmp_path / f"{name}.zarr"),
                                         "--compression", "zstd"])
        assert r.exit_code == 0, r.output
        return tmp_path / f"{name}.zarr"

    # the defaults, spelled out or left out: the same labels and the same objects.csv, byte for byte, under OBJECT_COLUMNS
    plain = run("plain", LH.SETTINGS)
    spelled = run("spelled", dict(LH.SETTINGS, inscribed_radius=False, expand_distance=0.0))
    grown = run("grown", dict(LH.SETTINGS, inscribed_radius=True, expand_distance=EXPAND))
    with open_ome_zarr(plain, prefer_iohub=False) as a, open_ome_zarr(spelled, prefer_iohub=False) as b, \
            open_ome_zarr(grown, prefer_iohub=False) as c:
        pa, pb, pc = dict(a.positions()), dict(b.positions()), dict(c.positions())
        for key in LH.TRANSLATION:
            text = (plain / key / "objects.csv").read_bytes()
            assert text == (spelled / key / "objects.csv").read_bytes()
            assert tuple(text.decode().splitlines()[0].split(",")) == OBJECT_COLUMNS
            with open(grown / key / "objects.csv", newline="") as fh:
                rows = list(csv.DictReader(fh))
            assert tuple(rows[0]) == OBJECT_COLUMNS + ("inscribed_radius_um",) and len(rows) == 6
            for t in range(2):
                want0, m, _ = LH.reference_segmentation(vols[key, t], LH.SETTINGS)
                assert np.array_equal(pa[key]["0"].read_volume(t, 0), want0) and np.array_equal(pb[key]["0"].read_volume(t, 0), want0)
                _, want, _ = reference_expansion(vols[key, t], LH.SETTINGS, SAMPLING, EXPAND)
                assert np.array_equal(pc[key]["0"].read_volume(t, 0), want)
                radius = reference_radius(want, 3, SAMPLING)
                mine = [row for row in rows if int(row["t"]) == t]
                assert [int(row["volume_voxels"]) for row in mine] == np.bincount(want.ravel(), minlength=4)[1:].tolist()
                assert [np.float32(row["inscribed_radius_um"]) for row in mine] == radius.tolist()


def test_cli_segment_distance_settings(tmp_path, cpu_cli):
    check_segment_command(cpu_cli, tmp_path)


cpu_cli = LH.cpu_cli
