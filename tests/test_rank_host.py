"""Rank filters on the host: the twin ``lsr_rank_filter_f32_cpu`` against ``tests/rank_ref.py`` -- ``scipy.ndimage.rank_filter`` by
value on the NaN-free cases, the restated rule (a full sort) byte for byte on every case --, the entry statuses of twin and device
entry alike, ``shrimpy_amd.rank`` on CPU tensors (the rank and percentile conventions against scipy, ``half_widths_of``), the spike
scene, ``median_radius`` of ``segment_zyx`` and the ``despeckle`` command.

Cases: ``tests/rank_cases.py``, sized from the exported tiling.
"""

import ctypes
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch
import yaml

from shrimpy_amd import _lib
from shrimpy_amd import morphology as M
from shrimpy_amd import rank as K
from shrimpy_amd import segment as S
from shrimpy_amd.settings import DespeckleSettings, SegmentSettings
from tests import rank_cases as C
from tests import rank_ref as R
from tests import test_label_host as LH

GUARD = 64
FILL = np.float32(-7.53125)                 # (no case holds it: the ramp moves in quarters)


def twin_rank(vol, r, rank, op, threshold=C.THRESHOLD, variant=0):
    """The twin through the C ABI into a poisoned buffer with 64 guard words behind it: (out, guard)."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    z, y, x = vol.shape
    out = np.full(vol.size + GUARD, FILL, dtype=np.float32)
    before = vol.tobytes()
    _lib.call("lsr_rank_filter_f32_cpu", vol.ctypes.data, out.ctypes.data, z, y, x, *r, rank, C.OPS.index(op),
              ctypes.c_float(threshold), variant, None)
    assert vol.tobytes() == before, "the input was written"
    return out[:vol.size].reshape(vol.shape), out[vol.size:]


@functools.lru_cache(maxsize=None)
def case_twin(shape, content, r, rank, op):
    """The twin's answer on a case, computed once (read-only; tests/test_rank_gpu.py holds the device to it)."""
    out, guard = twin_rank(C.volume(shape, content), r, rank, op)
    check_buffer(out, guard)
    out.setflags(write=False)
    return out


def check_buffer(out, guard):
    assert np.all(guard == FILL), "something was written behind the output"
    assert not np.any(out == FILL), "a voxel was not written"


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))            # (a copy: the shared cases are read-only)


# ---- the twin against scipy and the restatement ---------------------------------------------------------------------------------


@pytest.mark.parametrize("shape,r", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_equals_scipy_and_the_restatement(shape, r):
    for content, rank, op in C.calls_of(r):
        R.check(shape, content, r, rank, op, case_twin(shape, content, r, rank, op))


def test_the_cases_aim_at_the_tiling():
    assert (C.R, C.TZ, C.TY, C.TX) == (3, 4, 8, 64) == K.tiling() and K.max_half_width() == C.R
    for axis, t in enumerate((C.TZ, C.TY, C.TX)):
        assert {1, 2, t - 1, t, t + 1, 2 * t + 1} <= {s[axis] for s in C.SHAPES}
    assert any(all(n > t for n, t in zip(s, (C.TZ, C.TY, C.TX))) for s in C.SHAPES)
    assert max(int(np.prod(s)) for s in C.SHAPES) <= 400000
    assert set(C.REGISTER) == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)} - {(0, 0, 0)}
    assert {(0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 2), (3, 3, 3), (3, 0, 1)} <= set(C.HALF_WIDTHS)
    assert C.ranks_of((0, 0, 0)) == [0] and C.ranks_of((0, 0, 1)) == [0, 1, 2] and C.ranks_of((1, 1, 1)) == [0, 1, 13, 25, 26]
    nan = C.volume((5, 9, 65), "nan")
    assert np.isnan(nan).sum() > 100 and len(set(nan.view(np.uint32)[np.isnan(nan)].tolist())) == 2
    zeros = C.volume((5, 9, 65), "zeros")
    assert np.signbit(zeros).any() and not np.signbit(zeros).all() and not zeros.any()
    # the threshold splits the spike content: the ops change some voxels and keep others
    spikes = C.volume((5, 9, 65), "spikes")
    for op in C.OPS[1:]:
        changed = case_twin((5, 9, 65), "spikes", (0, 1, 1), 4, op) != spikes
        assert 20 < changed.sum() < spikes.size // 10
    # a fold that repeats: a window of 7 over an axis of 1 and of 2
    assert R.fold(np.arange(-3, 4), 1).tolist() == [0] * 7 and R.fold(np.arange(-3, 5), 2).tolist() == [1, 1, 0, 0, 1, 1, 0, 0]


def test_the_order_the_nan_rule_and_the_ops_by_hand():
    v = np.array([[[0.0, -0.0, 1.0, -np.inf, np.inf, 5.0, np.nan, 7.0, 8.0]]], dtype=np.float32)
    lo, mid, hi = (twin_rank(v, (0, 0, 1), k, "value")[0].view(np.uint32).ravel().tolist() for k in (0, 1, 2))
    # windows (reflect): [0 0 -0] [0 -0 1] [-0 1 -inf] [1 -inf inf] [-inf inf 5] [inf 5 nan] [5 nan 7] [nan 7 8] [7 8 8]
    assert lo == [0x80000000, 0x80000000, 0xFF800000, 0xFF800000, 0xFF800000, 0x40A00000, 0x40A00000, 0x40E00000, 0x40E00000]
    assert mid == [0, 0, 0x80000000, 0x3F800000, 0x40A00000, 0x7F800000, 0x40E00000, 0x41000000, 0x41000000]
    assert hi == [0, 0x3F800000, 0x3F800000, 0x7F800000, 0x7F800000, 0x7FC00000, 0x7FC00000, 0x7FC00000, 0x41000000]
    payload = np.array([0xFFC00001, 0x3F800000, 0x80000000], dtype=np.uint32).view(np.float32).reshape(1, 3, 1)
    copy, _ = twin_rank(payload, (0, 0, 0), 0, "value")
    assert copy.view(np.uint32).ravel().tolist() == [0x7FC00000, 0x3F800000, 0x80000000], "n = 1: a copy, a NaN the canonical one"
    for op in C.OPS[1:]:
        for t in (0.0, -1.0, np.inf):
            assert twin_rank(payload, (0, 0, 0), 0, op, t)[0].tobytes() == payload.tobytes(), "n = 1: the ops copy v bit for bit"
    # v = [0 10 0 0 -10 0], medians of 3 all 0: bright takes the 10, dark the -10, both both; a NaN voxel and a NaN median stay
    w = np.array([[[0.0, 10.0, 0.0, 0.0, -10.0, 0.0]]], dtype=np.float32)
    assert twin_rank(w, (0, 0, 1), 1, "remove_bright", 5.0)[0].ravel().tolist() == [0, 0, 0, 0, -10, 0]
    assert twin_rank(w, (0, 0, 1), 1, "remove_dark", 5.0)[0].ravel().tolist() == [0, 10, 0, 0, 0, 0]
    assert twin_rank(w, (0, 0, 1), 1, "remove_both", 5.0)[0].ravel().tolist() == [0, 0, 0, 0, 0, 0]
    assert twin_rank(w, (0, 0, 1), 1, "remove_both", 10.0)[0].tobytes() == w.tobytes(), "the comparison is strict"
    # medians of [n' 3 nan 1 50 2]: n', nan, 3, 50, 2, 2 -- the NaN voxels stay as they are, the 3 under a NaN median stays
    n = np.array([[[np.nan, 3.0, np.nan, 1.0, 50.0, 2.0]]], dtype=np.float32).view(np.uint32)
    n[0, 0, 0] = 0xFFC00001
    n = n.view(np.float32)
    assert twin_rank(n, (0, 0, 1), 1, "remove_both", 5.0)[0].view(np.uint32).ravel().tolist() == \
        [0xFFC00001, 0x40400000, 0x7FC00000, 0x42480000, 0x40000000, 0x40000000]


# ---- entry statuses -------------------------------------------------------------------------------------------------------------


def test_entry_statuses():
    lib = _lib.load()
    four = (ctypes.c_int * 4)()
    assert lib.lsr_rank_filter_tiling(four) == 0 and tuple(four) == K.tiling() and lib.lsr_rank_filter_tiling(None) == -1
    vol = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    out = np.full(24, FILL, dtype=np.float32)
    v, o, cap, t = vol.ctypes.data, out.ctypes.data, four[0], ctypes.c_float(1.0)
    for name in ("lsr_rank_filter_f32_cpu", "lsr_rank_filter_f32"):            # (checked before anything is launched)
        fn = getattr(lib, name)
        assert fn(None, o, 2, 3, 4, 1, 1, 1, 0, 0, t, 0, None) == -1 and fn(v, None, 2, 3, 4, 1, 1, 1, 0, 0, t, 0, None) == -1
        assert fn(v, v, 2, 3, 4, 1, 1, 1, 0, 0, t, 0, None) == -4 and b"alias" in lib.lsr_last_error()
        assert fn(v, o, 0, 3, 4, 1, 1, 1, 0, 0, t, 0, None) == -2 and fn(v, o, 2, -3, 4, 1, 1, 1, 0, 0, t, 0, None) == -2
        assert fn(v, o, 2 ** 30, 3, 4, 1, 1, 1, 0, 0, t, 0, None) == -3
        assert fn(v, o, 2 ** 20, 2 ** 20, 2 ** 20, 1, 1, 1, 0, 0, t, 0, None) == -3
        for bad in ((-1, 0, 0), (0, -1, 0), (0, 0, -2)):
            assert fn(v, o, 2, 3, 4, *bad, 0, 0, t, 0, None) == -4 and b"must be >= 0" in lib.lsr_last_error()
        for bad in ((cap + 1, 0, 0), (0, cap + 1, 0), (0, 0, 2 ** 30)):
            assert fn(v, o, 2, 3, 4, *bad, 0, 0, t, 0, None) == -3 and f"at most {cap} per axis".encode() in lib.lsr_last_error()
        for r, bad in (((1, 1, 1), 27), ((1, 1, 1), -1), ((0, 0, 0), 1), ((0, 1, 0), 3), ((3, 3, 3), 343)):
            assert fn(v, o, 2, 3, 4, *r, bad, 0, t, 0, None) == -4 and b"rank" in lib.lsr_last_error()
        for bad in (-1, 4, 99):
            assert fn(v, o, 2, 3, 4, 1, 1, 1, 0, bad, t, 0, None) == -4 and b"op" in lib.lsr_last_error()
        for bad in (-1, 2):
            assert fn(v, o, 2, 3, 4, 1, 1, 1, 0, 0, t, bad, None) == -4 and b"variant" in lib.lsr_last_error()
        for op in (1, 2, 3):
            assert fn(v, o, 2, 3, 4, 1, 1, 1, 0, op, ctypes.c_float(np.nan), 0, None) == -4 and b"threshold" in lib.lsr_last_error()
    assert np.all(out == FILL) and np.array_equal(vol.ravel(), np.arange(24)), "a refused call wrote something"
    # a NaN threshold does not matter to op 0; variant 1 is accepted by the twin; the last rank of the cap is the maximum
    assert lib.lsr_rank_filter_f32_cpu(v, o, 2, 3, 4, cap, cap, cap, 342, 0, ctypes.c_float(np.nan), 1, None) == 0 and np.all(out == 23.0)


# ---- the Python layer -----------------------------------------------------------------------------------------------------------


def test_rank_functions_on_cpu_tensors():
    shape, r = (5, 9, 65), (1, 1, 1)
    v = C.volume(shape, "noise")
    vol = _t(v)
    size = (3, 3, 3)
    for got, want in ((K.rank_filter(vol, 5, r), ndi.rank_filter(v, 5, size=size)),
                      (K.rank_filter(vol, -2, r), ndi.rank_filter(v, -2, size=size)),
                      (K.median_filter(vol, r), ndi.median_filter(v, size=size)),
                      (K.percentile_filter(vol, 30, r), ndi.percentile_filter(v, 30, size=size)),
                      (K.median_filter(vol, (0, 1, 1)), ndi.median_filter(v, size=(1, 3, 3), mode="reflect")),
                      (K.median_filter(vol, (0, 0, 0)), v)):
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device.type == "cpu" and got.shape == vol.shape
        assert got.data_ptr() != vol.data_ptr() and np.array_equal(got.numpy(), want)
    assert np.array_equal(vol.numpy(), v)
    med = ndi.median_filter(v, size=size)
    for which, take in (("bright", v - med > 0.5), ("dark", med - v > 0.5), ("both", np.abs(v - med) > 0.5)):
        assert np.array_equal(K.remove_outliers(vol, r, 0.5, which).numpy(), np.where(take, med, v))
    assert np.array_equal(K.remove_outliers(vol, r, 0.5).numpy(), K.remove_outliers(vol, r, 0.5, "bright").numpy())
    with pytest.raises(TypeError):
        K.median_filter(_t(v.astype(np.float64)), r)
    with pytest.raises(ValueError):
        K.median_filter(vol[0], r)
    for bad in ((1, 1), (1, -1, 1), (1.5, 1, 1), (C.R + 1, 0, 0)):
        with pytest.raises(ValueError):
            K.median_filter(vol, bad)
    with pytest.raises(ValueError, match=f"at most {C.R} per axis"):
        K.rank_filter(vol, 0, (0, 0, C.R + 1))
    for bad in (dict(which="hot"), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            K.remove_outliers(vol, r, **{"threshold": 1.0, **bad})


def test_rank_and_percentile_conventions_are_scipys():
    v = C.volume((3, 7, 63), "noise")
    vol = _t(v)
    for r in ((0, 1, 1), (1, 1, 1), (1, 1, 2), (2, 0, 3)):
        size, n = tuple(2 * k + 1 for k in r), C.window_size(r)
        for rank in (0, 1, n // 2, n - 1, -1, -2, -n):
            assert np.array_equal(K.rank_filter(vol, rank, r).numpy(), ndi.rank_filter(v, rank, size=size)), (r, rank)
        for bad in (n, n + 5, -n - 1):
            with pytest.raises(ValueError, match="rank"):
                K.rank_filter(vol, bad, r)
            with pytest.raises(RuntimeError):
                ndi.rank_filter(v, bad, size=size)
        for p in (0, 10, 25, 50, 75, 99.9, 100, -20, -100, 33.3):
            assert np.array_equal(K.percentile_filter(vol, p, r).numpy(), ndi.percentile_filter(v, p, size=size)), (r, p)
        for bad in (100.5, -100.5, 250, float("nan")):
            with pytest.raises(ValueError, match="percentile"):
                K.percentile_filter(vol, bad, r)
        for bad in (100.5, -100.5, 250):
            with pytest.raises(RuntimeError):
                ndi.percentile_filter(v, bad, size=size)
        assert np.array_equal(K.median_filter(vol, r).numpy(), ndi.median_filter(v, size=size))
    assert K.rank_of_percentile(50, 27) == 13 and K.rank_of_percentile(99.9, 9) == 8 and K.rank_of_percentile(-20, 343) == 274
    for bad in (1.5, True, "1"):
        with pytest.raises((ValueError, TypeError)):
            K.rank_filter(vol, bad, (1, 1, 1))


def test_half_widths_of():
    assert K.half_widths_of(3) == (3, 3, 3) and K.half_widths_of(0) == (0, 0, 0)
    assert K.half_widths_of(0.5, (0.5, 0.25, 0.25)) == (1, 2, 2) and K.half_widths_of((0, 1, 1)) == (0, 1, 1)
    assert K.half_widths_of(2.5) == (3, 3, 3) and K.half_widths_of(0.49) == (0, 0, 0) and K.half_widths_of(3.49) == (3, 3, 3)
    with pytest.raises(ValueError, match=f"at most {C.R} per axis"):
        K.half_widths_of(3.5)
    with pytest.raises(ValueError, match=f"at most {C.R} per axis"):
        K.half_widths_of((0, 0, 1.0), (1, 1, 0.25))
    for bad in (-1, (1, 2), float("nan")):
        with pytest.raises(ValueError):
            K.half_widths_of(bad)
    # morphology's own function is what it was: its cap, and this module's only on request
    assert M.half_widths_of(100) == (100, 100, 100) and M.half_widths_of(2.5, cap=3) == (3, 3, 3)
    with pytest.raises(ValueError, match="at most 3 per axis"):
        M.half_widths_of(100, cap=3)


def check_spike_scene(device):
    """Shared with tests/test_rank_gpu.py: ``remove_outliers`` changes exactly the 40 spikes, to scipy's median."""
    vol, at = C.spike_scene()
    assert vol.shape == (6, 20, 24) and len(at) == 40 and float(vol.max()) > 3000.0
    got = K.remove_outliers(_t(vol).to(device), (0, 1, 1), C.SPIKE_THRESHOLD, "bright").cpu().numpy()
    changed = np.flatnonzero(got.view(np.uint32).ravel() != vol.view(np.uint32).ravel())
    assert np.array_equal(changed, at), "exactly the raised voxels change, every other voxel keeps its bytes"
    assert np.array_equal(got.ravel()[at], ndi.median_filter(vol, size=(1, 3, 3)).ravel()[at])
    assert float(got.max()) < 200.0
    # a dark removal finds nothing to do here, and the plain median changes nearly everything
    assert K.remove_outliers(_t(vol).to(device), (0, 1, 1), C.SPIKE_THRESHOLD, "dark").cpu().numpy().tobytes() == vol.tobytes()
    assert (K.median_filter(_t(vol).to(device), (0, 1, 1)).cpu().numpy() != vol).mean() > 0.8


def test_the_spike_scene_on_the_host():
    check_spike_scene(torch.device("cpu"))


# ---- segment_zyx and the commands -----------------------------------------------------------------------------------------------

BALLS = dict(channel_name="GFP", threshold=C.BALL_THRESHOLD)


def check_segment_zyx(device):
    """Shared with tests/test_rank_gpu.py: ``median_radius`` of ``segment_zyx`` on ``device``."""
    vol = C.speckled_balls()
    d_vol = _t(vol).to(device)
    _, _, n_plain = S.segment_zyx(d_vol, SegmentSettings(**BALLS))
    assert n_plain == ndi.label(vol > C.BALL_THRESHOLD)[1] > 50, "the speckle is labelled"
    want, m = ndi.label(ndi.median_filter(vol, size=3) > C.BALL_THRESHOLD)
    labels, table, n = S.segment_zyx(d_vol, SegmentSettings(**BALLS, median_radius=1))
    assert n == m == 2 and labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want)
    assert float(table["intensity_max"].max()) >= 1000.0, "the table's intensities are the input's"
    # the radius is measured in the sampling; a zero component means no window on that axis
    labels, _, n = S.segment_zyx(d_vol, SegmentSettings(**BALLS, median_radius=0.5), sampling=(0.5, 0.5, 0.5))
    assert n == 2 and np.array_equal(labels.cpu().numpy(), want)
    want_yx, m_yx = ndi.label(ndi.median_filter(vol, size=(1, 3, 3)) > C.BALL_THRESHOLD)
    labels, _, n = S.segment_zyx(d_vol, SegmentSettings(**BALLS, median_radius=[0, 1, 1]))
    assert n == m_yx and np.array_equal(labels.cpu().numpy(), want_yx)
    with pytest.raises(ValueError, match="at most 3 per axis"):
        S.segment_zyx(d_vol, SegmentSettings(**BALLS, median_radius=4))
    # the defaults, spelled out or left out: the labels and the table of an existing scene
    blobs = LH.blob_volume(5)
    want0, m0, _ = LH.reference_segmentation(blobs, LH.SETTINGS)
    a = S.segment_zyx(_t(blobs).to(device), SegmentSettings(**LH.SETTINGS))
    b = S.segment_zyx(_t(blobs).to(device), SegmentSettings(**LH.SETTINGS, median_radius=0.0))
    c = S.segment_zyx(_t(blobs).to(device), SegmentSettings(**LH.SETTINGS, median_radius=[0, 0, 0]))
    for labels, table, n in (a, b, c):
        assert n == m0 and np.array_equal(labels.cpu().numpy(), want0)
        assert sorted(table) == sorted(a[1]) and all(np.array_equal(table[k], a[1][k], equal_nan=True) for k in table)


def test_segment_zyx_median_radius_on_the_host():
    check_segment_zyx(torch.device("cpu"))


def test_settings():
    s = SegmentSettings(channel_name="GFP", threshold=1.0)
    assert s.median_radius == 0.0 and "median_radius" in SegmentSettings.__doc__
    assert SegmentSettings(channel_name="GFP", threshold=1.0, median_radius=[0, 0.5, 0.5]).median_radius == (0.0, 0.5, 0.5)
    for bad in (dict(median_radius=-1.0), dict(median_radius=[1, 2]), dict(median_radius=float("inf")), dict(median_radius="wide")):
        with pytest.raises(ValueError):
            SegmentSettings(**{"channel_name": "GFP", "threshold": 1.0, **bad})
    d = DespeckleSettings(channel_names=["GFP"], half_widths=[0, 1, 1], threshold=200)
    assert d.op == "remove_bright" and d.half_widths == (0, 1, 1) and d.radius is None and d.percentile is None
    assert DespeckleSettings(channel_names=["GFP"], radius=0.5, op="median").radius == 0.5
    assert DespeckleSettings(channel_names=["GFP"], radius=[0, 1, 1], op="median", percentile=25).percentile == 25.0
    ok = dict(channel_names=["GFP"], half_widths=[0, 1, 1], threshold=200.0)
    for bad in (dict(channel_names=[]), dict(radius=1.0), dict(half_widths=None), dict(half_widths=[0, 0, 0]),
                dict(half_widths=[1, 1]), dict(half_widths=[1, -1, 1]), dict(half_widths=[0.5, 1, 1]), dict(threshold=None),
                dict(threshold=-1.0), dict(threshold=float("inf")), dict(op="median"), dict(op="remove_hot"),
                dict(percentile=50.0), dict(op="median", threshold=None, percentile=101.0), dict(sigma=1.0),
                dict(half_widths=None, radius=0.0), dict(half_widths=None, radius=[1, 2])):
        with pytest.raises(ValueError):
            DespeckleSettings(**{**ok, **bad})


HALF_WIDTHS = (0, 1, 1)
RADIUS_UM = 0.5                           # micrometres: (1, 2, 2) voxels at the store's (0.5, 0.25, 0.25) scale


def check_commands(cli, tmp_path):
    """Shared with tests/test_rank_gpu.py: ``despeckle`` and ``segment`` with ``median_radius`` on a temporary store."""
    from click.testing import CliRunner

    from shrimpy_amd.io.omezarr import open_ome_zarr

    vols = LH.make_store(tmp_path / "in.zarr")
    assert K.half_widths_of(RADIUS_UM, LH.SCALE[2:]) == (1, 2, 2)

    def run(command, name, settings, *extra, ok=True, fresh=True):
        cfg = tmp_path / f"{name}.yml"
        cfg.write_text(yaml.safe_dump(settings))
        out = tmp_path / f"{name}.zarr"
        r = CliRunner().invoke(cli.cli, [command, "-i", str(tmp_path / "in.zarr"), "-c", str(cfg), "-o", str(out), "--compression",
                                         "zstd", *extra])
        if ok:
            assert r.exit_code == 0, r.output
            return out, r.output
        assert r.exit_code != 0 and r.exception.__class__ is SystemExit and "Traceback" not in r.output, r.output
        assert not fresh or not out.exists(), "nothing is written"
        return r.output

    # the named channel is filtered, the other copied byte for byte; --levels 2 writes the second level
    settings = dict(channel_names=["GFP"], half_widths=list(HALF_WIDTHS), threshold=1000.0)
    out, _ = run("despeckle", "bright", settings, "--levels", "2")
    med, _ = run("despeckle", "median", dict(channel_names=["GFP"], radius=RADIUS_UM, op="median"))
    low, _ = run("despeckle", "low", dict(channel_names=["GFP"], radius=[0.0, 0.25, 0.25], op="median", percentile=25))
    with open_ome_zarr(out, prefer_iohub=False) as a, open_ome_zarr(med, prefer_iohub=False) as b, \
            open_ome_zarr(low, prefer_iohub=False) as c:
        pa, pb, pc = dict(a.positions()), dict(b.positions()), dict(c.positions())
        assert list(pa[next(iter(pa))].channel_names) == ["BF", "GFP"]
        for key in LH.TRANSLATION:
            for t in range(2):
                v = vols[key, t]
                m = ndi.median_filter(v, size=(1, 3, 3))
                got = pa[key]["0"].read_volume(t, 1)
                assert got.dtype == np.float32 and np.array_equal(got, np.where(v - m > 1000.0, m, v))
                assert all(got[at] < 8.0 < v[at] for at in ((1, 34, 40), (10, 3, 25), (6, 35, 4))), "the debris goes"
                assert (got != v).sum() < 40, "the blobs stay (but for the in-plane corners of the two brightest)"
                assert np.array_equal(pb[key]["0"].read_volume(t, 1), ndi.median_filter(v, size=(3, 5, 5)))
                assert np.array_equal(pc[key]["0"].read_volume(t, 1), ndi.percentile_filter(v, 25, size=(1, 3, 3)))
                assert np.array_equal(pa[key]["0"].read_volume(t, 0), np.full((12, 40, 48), 7, dtype=np.float32))
                level1 = pa[key]["1"].read_volume(t, 1)
                assert level1.shape == (6, 20, 24) and np.isfinite(level1).all() and level1.any()
    # --resume on a finished store does nothing; with other settings it is another run
    first = {(k, t): pa[k]["0"].read_volume(t, 1) for k in LH.TRANSLATION for t in range(2)}
    _, text = run("despeckle", "bright", settings, "--levels", "2", "--resume")
    assert "'units': 0," in text and "'units_skipped': 8" in text, text
    with open_ome_zarr(out, prefer_iohub=False) as a:
        pa = dict(a.positions())
        assert all(np.array_equal(pa[k]["0"].read_volume(t, 1), first[k, t]) for k, t in first)
    assert "different settings" in run("despeckle", "bright", dict(settings, threshold=500.0), "--levels", "2", "--resume", ok=False,
                                       fresh=False)
    # everything is checked before the output store is created
    assert "channel_names ['RFP'] not in the store" in run("despeckle", "unknown", dict(settings, channel_names=["RFP"]), ok=False)
    message = run("despeckle", "wide", dict(channel_names=["GFP"], radius=1.0, op="median"), ok=False)
    assert "position A/1/0" in message and f"at most {C.R} per axis" in message
    message = run("despeckle", "wide_voxels", dict(settings, half_widths=[0, 4, 4]), ok=False)
    assert "position A/1/0" in message and f"at most {C.R} per axis" in message
    assert "threshold" in run("despeckle", "no_threshold", dict(channel_names=["GFP"], half_widths=[0, 1, 1]), ok=False)
    assert "exactly one of radius and half_widths" in run("despeckle", "both", dict(settings, radius=0.5), ok=False)
    assert "positions ['Z/9/9'] not found" in run("despeckle", "nowhere", settings, "-p", "Z/9/9", ok=False)

    # segment: median_radius at its default, spelled out or left out, gives the same labels and the same objects.csv; a
    # median_radius beyond the cap is refused before the store exists
    plain, _ = run("segment", "plain", LH.SETTINGS)
    spelled, _ = run("segment", "spelled", dict(LH.SETTINGS, median_radius=0.0))
    smooth, _ = run("segment", "smooth", dict(channel_name="GFP", threshold=400.0, median_radius=[0.0, 0.25, 0.25]))
    with open_ome_zarr(plain, prefer_iohub=False) as a, open_ome_zarr(spelled, prefer_iohub=False) as b, \
            open_ome_zarr(smooth, prefer_iohub=False) as c:
        pa, pb, pc = dict(a.positions()), dict(b.positions()), dict(c.positions())
        for key in LH.TRANSLATION:
            assert (plain / key / "objects.csv").read_bytes() == (spelled / key / "objects.csv").read_bytes()
            for t in range(2):
                want0, _, _ = LH.reference_segmentation(vols[key, t], LH.SETTINGS)
                assert np.array_equal(pa[key]["0"].read_volume(t, 0), want0) and np.array_equal(pb[key]["0"].read_volume(t, 0), want0)
                want, m = ndi.label(ndi.median_filter(vols[key, t], size=(1, 3, 3)) > 400.0)
                assert m == 3 and np.array_equal(pc[key]["0"].read_volume(t, 0), want), "the debris is gone before the threshold"
    message = run("segment", "wide_median", dict(LH.SETTINGS, median_radius=1.0), ok=False)
    assert "position A/1/0: median_radius" in message and f"at most {C.R} per axis" in message


def test_cli_despeckle_and_segment(tmp_path, cpu_cli):
    check_commands(cpu_cli, tmp_path)


def test_help_texts_name_the_new_command_and_setting(cpu_cli):
    from click.testing import CliRunner

    r = CliRunner().invoke(cpu_cli.cli, ["segment", "-h"])
    assert r.exit_code == 0 and "median_radius" in r.output
    r = CliRunner().invoke(cpu_cli.cli, ["despeckle", "-h"])
    assert r.exit_code == 0 and "--levels" in r.output and "--resume" in r.output and "--on-error" in r.output and "median" in r.output


cpu_cli = LH.cpu_cli
