"""Grey morphology on the host: the twin ``lsr_grey_morph_f32_cpu`` against ``tests/morphology_ref.py`` -- ``scipy.ndimage`` element
for element on the NaN-free cases, the restated rule byte for byte on every case, a brute force on the smallest shapes --, the
algebra of the operators, the entry statuses of twin and device entry alike, ``shrimpy_amd.morphology`` on CPU tensors
(``half_widths_of``, ``fill_holes``), the two new settings of ``segment_zyx`` and the ``segment`` and ``subtract-background``
commands.

Cases: ``tests/morphology_cases.py``, sized from the exported tiling.
"""

import ctypes

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch
import yaml

from shrimpy_amd import _lib
from shrimpy_amd import morphology as M
from shrimpy_amd import segment as S
from shrimpy_amd.settings import BackgroundSettings, SegmentSettings
from tests import morphology_cases as C
from tests import morphology_ref as R
from tests import test_label_host as LH

GUARD = 64
FILL = np.float32(-7.5)


def scratch_bytes_of_the_cases():
    return max(_lib.call_value("lsr_grey_morph_scratch_bytes", *shape) for shape in C.SHAPES + [C.RAMP_SHAPE])


# one scratch buffer for every call of this module, never cleared between them (and poisoned to begin with)
SCRATCH = np.full(scratch_bytes_of_the_cases(), 0xA5, dtype=np.uint8)


def twin_morph(vol, r, op):
    """The twin through the C ABI into a poisoned buffer with 64 guard words behind it: (out, guard)."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    z, y, x = vol.shape
    assert 0 < _lib.call_value("lsr_grey_morph_scratch_bytes", z, y, x) <= SCRATCH.nbytes
    out = np.full(vol.size + GUARD, FILL, dtype=np.float32)
    before = vol.tobytes()
    _lib.call("lsr_grey_morph_f32_cpu", vol.ctypes.data, out.ctypes.data, z, y, x, *r, C.OPS.index(op), SCRATCH.ctypes.data, None)
    assert vol.tobytes() == before, "the input was written"
    return out[:vol.size].reshape(vol.shape), out[vol.size:]


def check_buffer(out, guard):
    assert np.all(guard == FILL), "something was written behind the output"
    assert not np.any(out == FILL), "a voxel was not written"


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))            # (a copy: the shared cases are read-only)


# ---- the twin against scipy, the restatement and the brute force ----------------------------------------------------------------


@pytest.mark.parametrize("shape,r", C.PARAMS, ids=C.PARAM_IDS)
def test_twin_equals_scipy_and_the_restatement(shape, r):
    for content in C.CONTENTS:
        for op in C.OPS:
            out, guard = twin_morph(C.volume(shape, content), r, op)
            check_buffer(out, guard)
            R.check(shape, content, r, op, out)


def test_the_cases_aim_at_the_tiling():
    assert C.R >= 128 and C.COLUMNS == 64 and C.SEGMENT >= 2 * C.R
    assert M.max_half_width() == C.R
    for shape in C.SHAPES:
        rs = C.half_widths_of_shape(shape)
        assert any(max(r) == C.R and sorted(r)[:2] == [0, 0] for r in rs)
        assert all(a >= min(n, C.R) for a, n in zip(rs[-1], shape))
    assert sum(C.R in r for r in C.half_widths_of_shape((5, 9, 13))) >= 3
    assert max(int(np.prod(s)) for s in C.SHAPES) <= 40000
    nan = C.volume((5, 9, 13), "nan")
    assert np.isnan(nan).sum() > 20 and len(set(nan.view(np.uint32)[np.isnan(nan)].tolist())) == 2
    zeros = C.volume((5, 9, 13), "zeros")
    assert np.signbit(zeros).any() and not np.signbit(zeros).all() and not zeros.any()


@pytest.mark.parametrize("shape", C.SMALLEST, ids=str)
def test_a_brute_force_agrees_with_the_restatement(shape):
    for content in ("noise", "small_integers", "inf", "nan", "zeros"):
        v = C.volume(shape, content)
        for r in C.half_widths_of_shape(shape)[1:4] + [(1, 2, 3), tuple(shape)]:
            assert R.same_bytes(R.brute(v, r, False), R.erode(v, r)) and R.same_bytes(R.brute(v, r, True), R.dilate(v, r))
            assert R.brute(v, r, False).tobytes() == R.erode(v, r).tobytes()            # (the canonical NaN included)


def test_the_order_and_the_nan_rule_by_hand():
    v = np.array([[[0.0, -0.0, 1.0, -np.inf, np.inf, 5.0, np.nan, 7.0, 8.0]]], dtype=np.float32)
    lo, _ = twin_morph(v, (0, 0, 1), "grey_erosion")
    hi, _ = twin_morph(v, (0, 0, 1), "grey_dilation")
    assert lo.view(np.uint32).ravel()[:5].tolist() == [0x80000000, 0x80000000, 0xFF800000, 0xFF800000, 0xFF800000]
    assert hi.view(np.uint32).ravel()[:5].tolist() == [0, 0x3F800000, 0x3F800000, 0x7F800000, 0x7F800000]
    assert lo.view(np.uint32).ravel()[5:].tolist() == [0x7FC00000, 0x7FC00000, 0x7FC00000, 0x40E00000]
    assert hi.view(np.uint32).ravel()[5:].tolist() == [0x7FC00000, 0x7FC00000, 0x7FC00000, 0x41000000]
    payload = np.array([0xFFC00001, 0x3F800000], dtype=np.uint32).view(np.float32).reshape(1, 1, 2)
    copy, _ = twin_morph(payload, (0, 0, 0), "grey_closing")
    assert copy.tobytes() == payload.tobytes(), "no window: a copy, bit for bit"
    zero, _ = twin_morph(np.full((1, 2, 2), 3.0, dtype=np.float32), (0, 0, 0), "white_tophat")
    assert zero.view(np.uint32).tolist() == [[[0, 0], [0, 0]]]


@pytest.mark.parametrize("shape", [(5, 9, 13), (3, 4, C.COLUMNS + 6), (C.W5, C.W5 + 1, 2 * C.W5 - 1)], ids=str)
def test_the_algebra_holds_bit_for_bit(shape):
    for content in C.NAN_FREE:
        v = C.volume(shape, content)
        for r in [(1, 0, 2), (2, 2, 2), (7, 1, 3)]:
            opened, closed = twin_morph(v, r, "grey_opening")[0], twin_morph(v, r, "grey_closing")[0]
            assert twin_morph(opened, r, "grey_opening")[0].tobytes() == opened.tobytes()
            assert twin_morph(closed, r, "grey_closing")[0].tobytes() == closed.tobytes()
            assert np.all(R.float_key(opened) <= R.float_key(v)) and np.all(R.float_key(v) <= R.float_key(closed))
            assert twin_morph(v, r, "grey_dilation")[0].tobytes() == (-twin_morph(-v, r, "grey_erosion")[0]).tobytes()


# ---- entry statuses -------------------------------------------------------------------------------------------------------------


def test_entry_statuses():
    lib = _lib.load()
    four = (ctypes.c_int * 4)()
    assert lib.lsr_grey_morph_tiling(four) == 0 and tuple(four) == M.tiling() and lib.lsr_grey_morph_tiling(None) == -1
    assert four[0] >= 128
    six = (ctypes.c_int * 6)()
    assert lib.lsr_grey_morph_dispatch(six) == 0 and tuple(six) == M.dispatch() and lib.lsr_grey_morph_dispatch(None) == -1
    assert 0 < six[0] < six[1] < four[0] and six[2] > 0 and 0 < six[3] < six[4] < six[5]
    assert lib.lsr_grey_morph_scratch_bytes(4, 5, 6) == 2 * 4 * 120
    assert lib.lsr_grey_morph_scratch_bytes(0, 5, 6) == -2 and lib.lsr_grey_morph_scratch_bytes(2 ** 30, 5, 6) == -3
    assert lib.lsr_grey_morph_scratch_bytes(171, 2048, 2270) == 8 * 171 * 2048 * 2270 > 2 ** 31     # the config-2 deskewed grid
    vol = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    out = np.full(24, FILL, dtype=np.float32)
    v, o, s, cap = vol.ctypes.data, out.ctypes.data, SCRATCH.ctypes.data, four[0]
    for name in ("lsr_grey_morph_f32_cpu", "lsr_grey_morph_f32"):            # (checked before anything is launched)
        fn = getattr(lib, name)
        assert fn(None, o, 2, 3, 4, 1, 1, 1, 0, s, None) == -1 and fn(v, None, 2, 3, 4, 1, 1, 1, 0, s, None) == -1
        assert fn(v, o, 2, 3, 4, 1, 1, 1, 0, None, None) == -1 and b"scratch is NULL" in lib.lsr_last_error()
        assert fn(v, v, 2, 3, 4, 1, 1, 1, 0, s, None) == -4 and b"alias" in lib.lsr_last_error()
        assert fn(v, o, 0, 3, 4, 1, 1, 1, 0, s, None) == -2 and fn(v, o, 2, -3, 4, 1, 1, 1, 0, s, None) == -2
        assert fn(v, o, 2 ** 30, 3, 4, 1, 1, 1, 0, s, None) == -3 and fn(v, o, 2 ** 20, 2 ** 20, 2 ** 20, 1, 1, 1, 0, s, None) == -3
        for bad in ((-1, 0, 0), (0, -1, 0), (0, 0, -2)):
            assert fn(v, o, 2, 3, 4, *bad, 0, s, None) == -4 and b"must be >= 0" in lib.lsr_last_error()
        for bad in ((cap + 1, 0, 0), (0, cap + 1, 0), (0, 0, 2 ** 30)):
            assert fn(v, o, 2, 3, 4, *bad, 0, s, None) == -3 and f"at most {cap} per axis".encode() in lib.lsr_last_error()
        for bad in (-1, 6, 99):
            assert fn(v, o, 2, 3, 4, 1, 1, 1, bad, s, None) == -4 and b"op" in lib.lsr_last_error()
    assert np.all(out == FILL) and np.array_equal(vol.ravel(), np.arange(24)), "a refused call wrote something"
    assert lib.lsr_grey_morph_f32_cpu(v, o, 2, 3, 4, cap, cap, cap, 1, s, None) == 0 and np.all(out == 23.0)


# ---- the Python layer -----------------------------------------------------------------------------------------------------------


def test_morphology_functions_on_cpu_tensors():
    shape, r = (5, 9, 13), (2, 2, 2)
    vol = _t(C.volume(shape, "noise"))
    for op in C.OPS:
        got = getattr(M, op)(vol, r)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device.type == "cpu" and got.shape == vol.shape
        R.check(shape, "noise", r, op, got.numpy())
        assert got.data_ptr() != vol.data_ptr() and np.array_equal(vol.numpy(), C.volume(shape, "noise"))
    assert M.subtract_background(vol, 1.0, (0.5, 0.5, 0.5)).numpy().tobytes() == M.white_tophat(vol, r).numpy().tobytes()
    assert M.subtract_background(vol, 2.0).numpy().tobytes() == M.white_tophat(vol, r).numpy().tobytes()
    with pytest.raises(TypeError):
        M.grey_erosion(_t(C.volume(shape, "noise").astype(np.float64)), r)
    with pytest.raises(ValueError):
        M.grey_erosion(vol[0], r)
    for bad in ((1, 1), (1, -1, 1), (1.5, 1, 1), (C.R + 1, 0, 0)):
        with pytest.raises(ValueError):
            M.grey_dilation(vol, bad)
    with pytest.raises(ValueError, match=f"at most {C.R} per axis"):
        M.white_tophat(vol, (0, 0, C.R + 1))


def test_half_widths_of():
    assert M.half_widths_of(5) == (5, 5, 5) and M.half_widths_of(0) == (0, 0, 0)
    assert M.half_widths_of(5.0, (0.5, 0.25, 0.25)) == (10, 20, 20)
    assert M.half_widths_of((0, 2, 3)) == (0, 2, 3)
    # floor(radius / s + 0.5): halves round up, whatever the parity of the result
    assert M.half_widths_of(2.5) == (3, 3, 3) and M.half_widths_of(3.5) == (4, 4, 4) and M.half_widths_of(0.5) == (1, 1, 1)
    assert M.half_widths_of(0.49) == (0, 0, 0) and M.half_widths_of((1.0, 1.0, 1.25), (0.4, 2.0, 0.5)) == (3, 1, 3)
    assert M.half_widths_of(C.R + 0.49) == (C.R,) * 3
    with pytest.raises(ValueError, match=f"at most {C.R} per axis"):
        M.half_widths_of(C.R + 0.5)
    with pytest.raises(ValueError, match=f"at most {C.R} per axis"):
        M.half_widths_of((0, 0, 1.0), (1, 1, 1.0 / (C.R + 1)))
    for bad in (-1, (1, 2), (1, 2, -3), float("nan"), float("inf")):
        with pytest.raises(ValueError):
            M.half_widths_of(bad)
    for bad in ((1, 1), (1, 0, 1), (1, 1, float("nan"))):
        with pytest.raises(ValueError):
            M.half_widths_of(1.0, bad)


def check_fill_holes(device):
    """Shared with tests/test_morphology_gpu.py: ``fill_holes`` against ``scipy.ndimage.binary_fill_holes`` on ``device``."""
    for seed in range(4):
        mask = np.random.default_rng(seed).random((6, 9, 11)) < 0.6
        got = M.fill_holes(torch.from_numpy(mask).to(device))
        assert got.dtype == torch.bool and got.device.type == torch.device(device).type
        assert np.array_equal(got.cpu().numpy(), ndi.binary_fill_holes(mask))
    assert any((ndi.binary_fill_holes(np.random.default_rng(s).random((6, 9, 11)) < 0.6)
                != (np.random.default_rng(s).random((6, 9, 11)) < 0.6)).any() for s in range(4)), "no hole to fill"
    shell = C.shell_mask()
    filled = M.fill_holes(torch.from_numpy(shell.copy()).to(device)).cpu().numpy()
    assert shell.sum() == 674 and filled.sum() == 925 and np.array_equal(filled, ndi.binary_fill_holes(shell))
    assert np.array_equal(filled, C.ball(C.SHELL_SHAPE, (7, 8, 8), 36))
    opened = C.open_shell_mask()
    got = M.fill_holes(torch.from_numpy(opened.copy()).to(device)).cpu().numpy()
    assert np.array_equal(got, opened) and np.array_equal(got, ndi.binary_fill_holes(opened)), "a hole that touches a face stays open"
    for trivial in (np.zeros((2, 3, 4), dtype=bool), np.ones((2, 3, 4), dtype=bool)):
        assert np.array_equal(M.fill_holes(torch.from_numpy(trivial).to(device)).cpu().numpy(), trivial)


def test_fill_holes_on_the_host():
    check_fill_holes(torch.device("cpu"))
    with pytest.raises(TypeError):
        M.fill_holes(torch.zeros((2, 3, 4), dtype=torch.float32))


# ---- segment_zyx and the commands -----------------------------------------------------------------------------------------------

RAMP = dict(channel_name="GFP", threshold=C.RAMP_THRESHOLD)


def check_segment_zyx(device):
    """Shared with tests/test_morphology_gpu.py: the two new settings of ``segment_zyx`` on ``device``."""
    vol = C.ramp_scene()
    d_vol = _t(vol).to(device)
    assert float(ndi.white_tophat(np.broadcast_to(vol[0, 0], vol.shape).copy(), size=11).max()) == 20.0   # the ramp's own top-hat
    _, _, n_plain = S.segment_zyx(d_vol, SegmentSettings(**RAMP))
    assert n_plain == 1 == ndi.label(vol > C.RAMP_THRESHOLD)[1]
    want, m = ndi.label(ndi.white_tophat(vol, size=11) > C.RAMP_THRESHOLD)
    labels, table, n = S.segment_zyx(d_vol, SegmentSettings(**RAMP, background_radius=5))
    assert n == m == 6 and labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want)
    assert table["volume"].tolist() == [123] * 6
    assert np.all(table["intensity_min"] >= 60.0), "the table's intensities are the input's"
    # the radius is measured in the sampling; a zero component means no window on that axis
    labels, _, n = S.segment_zyx(d_vol, SegmentSettings(**RAMP, background_radius=2.5), sampling=(0.5, 0.5, 0.5))
    assert n == 6 and np.array_equal(labels.cpu().numpy(), want)
    want_yx, m_yx = ndi.label(ndi.white_tophat(vol, size=(1, 11, 11)) > C.RAMP_THRESHOLD)
    labels, _, n = S.segment_zyx(d_vol, SegmentSettings(**RAMP, background_radius=[0, 5, 5]))
    assert n == m_yx and np.array_equal(labels.cpu().numpy(), want_yx)
    # fill_holes: the shell's object has the solid ball's volume, under every connectivity
    shell = np.where(C.shell_mask(), np.float32(100.0), np.float32(0.0))
    d_shell = _t(shell).to(device)
    _, table, n = S.segment_zyx(d_shell, SegmentSettings(channel_name="GFP", threshold=50.0))
    assert n == 1 and table["volume"].tolist() == [674]
    for connectivity in (6, 18, 26):
        labels, table, n = S.segment_zyx(d_shell, SegmentSettings(channel_name="GFP", threshold=50.0, fill_holes=True,
                                                                  connectivity=connectivity))
        assert n == 1 and table["volume"].tolist() == [925]
        assert np.array_equal(labels.cpu().numpy(), ndi.binary_fill_holes(C.shell_mask()).astype(np.int32))
    # the defaults, spelled out or left out: the labels and the table of an existing scene
    blobs = LH.blob_volume(5)
    want0, m0, _ = LH.reference_segmentation(blobs, LH.SETTINGS)
    a = S.segment_zyx(_t(blobs).to(device), SegmentSettings(**LH.SETTINGS))
    b = S.segment_zyx(_t(blobs).to(device), SegmentSettings(**LH.SETTINGS, background_radius=0.0, fill_holes=False))
    c = S.segment_zyx(_t(blobs).to(device), SegmentSettings(**LH.SETTINGS, background_radius=[0, 0, 0]))
    for labels, table, n in (a, b, c):
        assert n == m0 and np.array_equal(labels.cpu().numpy(), want0)
        assert sorted(table) == sorted(a[1]) and all(np.array_equal(table[k], a[1][k], equal_nan=True) for k in table)


def test_segment_zyx_background_and_holes_on_the_host():
    check_segment_zyx(torch.device("cpu"))


def test_settings():
    s = SegmentSettings(channel_name="GFP", threshold=1.0)
    assert s.background_radius == 0.0 and s.fill_holes is False
    assert "background_radius" in SegmentSettings.__doc__ and "fill_holes" in SegmentSettings.__doc__
    assert SegmentSettings(channel_name="GFP", threshold=1.0, background_radius=[0, 2, 3.5]).background_radius == (0.0, 2.0, 3.5)
    assert SegmentSettings(channel_name="GFP", threshold=1.0, background_radius=4).background_radius == 4.0
    for bad in (dict(background_radius=-1.0), dict(background_radius=[1, 2]), dict(background_radius=[1, -2, 3]),
                dict(background_radius=float("inf")), dict(fill_holes="maybe"), dict(background_radius="wide")):
        with pytest.raises(ValueError):
            SegmentSettings(**{"channel_name": "GFP", "threshold": 1.0, **bad})
    b = BackgroundSettings(channel_names=["GFP"], radius=2.0)
    assert b.op == "white_tophat" and BackgroundSettings(channel_names=["GFP"], radius=[0, 1, 1], op="black_tophat").radius == (0.0, 1.0, 1.0)
    for bad in (dict(channel_names=[]), dict(radius=0.0), dict(radius=[0, 0, 0]), dict(radius=-1), dict(op="rolling_ball"),
                dict(radius=[1, 2]), dict(sigma=1.0)):
        with pytest.raises(ValueError):
            BackgroundSettings(**{"channel_names": ["GFP"], "radius": 2.0, **bad})


RADIUS_UM = 0.5                           # micrometres: (1, 2, 2) voxels at the store's (0.5, 0.25, 0.25) scale
HALF_WIDTHS = (1, 2, 2)


def check_commands(cli, tmp_path):
    """Shared with tests/test_morphology_gpu.py: ``segment`` with the new settings and ``subtract-background`` on a temporary
    store."""
    from click.testing import CliRunner

    from shrimpy_amd.io.omezarr import open_ome_zarr

    vols = LH.make_store(tmp_path / "in.zarr")
    assert M.half_widths_of(RADIUS_UM, LH.SCALE[2:]) == HALF_WIDTHS
    size = tuple(2 * r + 1 for r in HALF_WIDTHS)

    def run(command, name, settings, *extra, ok=True):
        cfg = tmp_path / f"{name}.yml"
        cfg.write_text(yaml.safe_dump(settings))
        out = tmp_path / f"{name}.zarr"
        r = CliRunner().invoke(cli.cli, [command, "-i", str(tmp_path / "in.zarr"), "-c", str(cfg), "-o", str(out), "--compression",
                                         "zstd", *extra])
        if ok:
            assert r.exit_code == 0, r.output
            return out
        assert r.exit_code != 0 and r.exception.__class__ is SystemExit and "Traceback" not in r.output, r.output
        assert not out.exists(), "nothing is written"
        return r.output

    # segment: the defaults, spelled out or left out, give the same labels and the same objects.csv, byte for byte
    plain = run("segment", "plain", LH.SETTINGS)
    spelled = run("segment", "spelled", dict(LH.SETTINGS, background_radius=0.0, fill_holes=False))
    flat = run("segment", "flat", dict(channel_name="GFP", threshold=400.0, background_radius=[0.0, 3.0, 3.0], fill_holes=True))
    with open_ome_zarr(plain, prefer_iohub=False) as a, open_ome_zarr(spelled, prefer_iohub=False) as b, \
            open_ome_zarr(flat, prefer_iohub=False) as c:
        pa, pb, pc = dict(a.positions()), dict(b.positions()), dict(c.positions())
        for key in LH.TRANSLATION:
            assert (plain / key / "objects.csv").read_bytes() == (spelled / key / "objects.csv").read_bytes()
            for t in range(2):
                want0, _, _ = LH.reference_segmentation(vols[key, t], LH.SETTINGS)
                assert np.array_equal(pa[key]["0"].read_volume(t, 0), want0) and np.array_equal(pb[key]["0"].read_volume(t, 0), want0)
                top = ndi.white_tophat(vols[key, t], size=(1, 25, 25))             # 3 um at 0.25 um: 12 voxels to each side
                want, _ = ndi.label(ndi.binary_fill_holes(top > 400.0))
                assert want.max() >= 3 and np.array_equal(pc[key]["0"].read_volume(t, 0), want)

    message = run("segment", "wide", dict(LH.SETTINGS, background_radius=0.25 * (C.R + 1)), ok=False)
    assert "position A/1/0: background_radius" in message and f"at most {C.R} per axis" in message

    # subtract-background: the named channel is scipy's top-hat, the other its input; --levels 2 writes the second level
    settings = dict(channel_names=["GFP"], radius=RADIUS_UM)
    out = run("subtract-background", "white", settings, "--levels", "2")
    black = run("subtract-background", "black", dict(settings, op="black_tophat", radius=[RADIUS_UM] * 3))
    with open_ome_zarr(out, prefer_iohub=False) as w, open_ome_zarr(black, prefer_iohub=False) as k:
        pw, pk = dict(w.positions()), dict(k.positions())
        assert list(pw[next(iter(pw))].channel_names) == ["BF", "GFP"]
        for key in LH.TRANSLATION:
            for t in range(2):
                got = pw[key]["0"].read_volume(t, 1)
                assert got.dtype == np.float32 and np.array_equal(got, ndi.white_tophat(vols[key, t], size=size))
                assert np.array_equal(pk[key]["0"].read_volume(t, 1), ndi.black_tophat(vols[key, t], size=size))
                assert np.array_equal(pw[key]["0"].read_volume(t, 0), np.full((12, 40, 48), 7, dtype=np.float32))
                level1 = pw[key]["1"].read_volume(t, 1)
                assert level1.shape == (6, 20, 24) and np.isfinite(level1).all() and level1.any()
    # everything is checked before the output store is created
    assert "channel_names ['RFP'] not in the store" in run("subtract-background", "unknown", dict(settings, channel_names=["RFP"]), ok=False)
    message = run("subtract-background", "wide", dict(settings, radius=0.25 * (C.R + 1)), ok=False)
    assert "position A/1/0" in message and f"at most {C.R} per axis" in message
    assert "radius" in run("subtract-background", "none", dict(settings, radius=0.0), ok=False)
    assert "positions ['Z/9/9'] not found" in run("subtract-background", "nowhere", settings, "-p", "Z/9/9", ok=False)


def test_cli_segment_and_subtract_background(tmp_path, cpu_cli):
    check_commands(cpu_cli, tmp_path)


def test_help_texts_name_the_new_settings(cpu_cli):
    from click.testing import CliRunner

    r = CliRunner().invoke(cpu_cli.cli, ["segment", "-h"])
    assert r.exit_code == 0 and "background_radius" in r.output and "fill_holes" in r.output
    r = CliRunner().invoke(cpu_cli.cli, ["subtract-background", "-h"])
    assert r.exit_code == 0 and "--levels" in r.output and "--resume" in r.output and "--on-error" in r.output and "top-hat" in r.output


cpu_cli = LH.cpu_cli
