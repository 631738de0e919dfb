"""Stitching on the host: the twin of the compositing kernel (``lsr_stitch_f32_cpu``) against ``tests/stitch_ref.py``, the
canvas geometry, banded composition, the entry statuses, the settings, the placement estimate and the two commands.

biahub is not installed: PARITY IS UNPINNED and ``stitch_ref`` (float64 NumPy) is the oracle.  The float32 bound is a-priori
(``stitch_ref``'s docstring derives it from the operation count of ``csrc/stitch.hpp``), never a measured number.
"""

import ctypes
import logging

import numpy as np
import pytest
import torch
import yaml

from shrimpy_amd import _lib
from shrimpy_amd import stitch as S
from shrimpy_amd.settings import EstimateStitchSettings, StitchSettings
from tests import stitch_ref as R


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _stitch(tiles, translations, p=1, cval=0.0, box=None):
    return S.stitch_tiles([_t(a) for a in tiles], translations, p, cval, box=box).numpy()


# ---- geometry -------------------------------------------------------------------------------------------------------------


def test_canvas_geometry_with_negative_and_fractional_translations():
    shapes = [(3, 5, 7), (2, 4, 6)]
    tr = [(-1.5, 0.0, 2.25), (0.0, -3.0, 4.5)]
    shape, origin = S.canvas_geometry(shapes, tr)
    assert origin == (-2, -3, 2)                       # floor(min t)
    assert shape == (2 + 2, 5 + 3, 11 - 2)             # ceil(max(t + n)) - origin: z 2, y 5, x max(9.25, 10.5) -> 11
    assert (shape, origin) == R.canvas_geometry(shapes, tr)
    assert S.canvas_geometry([(1, 1, 1)], [(5, -6, 7)]) == ((1, 1, 1), (5, -6, 7))
    with pytest.raises(ValueError):
        S.canvas_geometry([(1, 1, 1)], [(0, 0, 0), (1, 1, 1)])


# ---- the rule, by hand ------------------------------------------------------------------------------------------------------


def test_single_tile_at_an_integer_translation_is_a_bit_exact_copy_in_a_sea_of_cval():
    tile = R.f32_tile((3, 5, 7), 1)
    got = _stitch([tile], [(2, -3, 4)], p=1, cval=-1.25, box=((1, -5, 2), (5, 9, 12)))
    want = np.full((5, 9, 12), -1.25, dtype=np.float32)
    want[1:4, 2:7, 2:9] = tile
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_two_tiles_p0_average_in_the_overlap_and_copy_elsewhere():
    a, b = R.f32_tile((2, 6, 9), 2), R.f32_tile((2, 6, 9), 3)
    got = _stitch([a, b], [(0, 0, 0), (0, 2, 5)], p=0, cval=np.nan)
    assert got.shape == (2, 8, 14)
    mean = (a[:, 2:, 5:] + b[:, :4, :4]) / np.float32(2.0)        # float32: (1 * a + 1 * b) / (1 + 1)
    assert np.array_equal(got[:, 2:6, 5:9].view(np.uint32), mean.view(np.uint32))
    only_a = np.ones((2, 6, 9), dtype=bool)
    only_a[:, 2:, 5:] = False
    assert np.array_equal(got[:, :6, :9][only_a].view(np.uint32), a[only_a].view(np.uint32))
    only_b = np.ones((2, 6, 9), dtype=bool)
    only_b[:, :4, :4] = False
    assert np.array_equal(got[:, 2:, 5:][only_b].view(np.uint32), b[only_b].view(np.uint32))
    assert np.isnan(got[:, :2, 9:]).all() and np.isnan(got[:, 6:, :5]).all()


def test_p1_weights_at_a_hand_computed_voxel():
    a, b = R.f32_tile((1, 6, 9), 4), R.f32_tile((1, 6, 9), 5)
    got = _stitch([a, b], [(0, 0, 0), (0, 2, 5)], p=1)
    # canvas (0, 4, 7): a at (4, 7): dy = min(5, 2) = 2, dx = min(8, 2) = 2, w = 4; b at (2, 2): dy = min(3, 4) = 3, dx = 3, w = 9
    f = np.float32
    want = (f(4) * a[0, 4, 7] + f(9) * b[0, 2, 2]) / f(13)
    assert got[0, 4, 7].view(np.uint32) == f(want).view(np.uint32)
    # p = 4: (dy dx)^4 by repeated multiplication
    got4 = _stitch([a, b], [(0, 0, 0), (0, 2, 5)], p=4)
    want4 = (f(256) * a[0, 4, 7] + f(6561) * b[0, 2, 2]) / f(6817)
    assert got4[0, 4, 7].view(np.uint32) == f(want4).view(np.uint32)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_fraction_on_one_axis_interpolates_that_axis_only_and_loses_one_voxel_of_it(axis):
    tile = R.f32_tile((4, 5, 6), 6 + axis)
    t = [1.0, 2.0, 3.0]
    t[axis] += 0.25
    got = _stitch([tile], [tuple(t)], cval=np.nan)
    shape, origin = S.canvas_geometry([tile.shape], [tuple(t)])
    assert origin == (1, 2, 3) and shape == tuple(n + (1 if a == axis else 0) for a, n in enumerate(tile.shape))
    covered = ~np.isnan(got)
    want_cov = np.zeros(shape, dtype=bool)
    inner = [slice(0, n) for n in tile.shape]
    inner[axis] = slice(1, tile.shape[axis])          # j = 1 .. n - 1: one voxel fewer than the tile has
    want_cov[tuple(inner)] = True
    assert np.array_equal(covered, want_cov)
    lo, hi = [slice(None)] * 3, [slice(None)] * 3
    lo[axis], hi[axis] = slice(0, -1), slice(1, None)
    f = np.float32
    want = f(0.25) * tile[tuple(lo)] + f(0.75) * tile[tuple(hi)]       # taps j - 1 and j, weights tf and 1 - tf
    assert np.array_equal(got[tuple(inner)].view(np.uint32), want.astype(np.float32).view(np.uint32))


# ---- against the float64 restatement ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=[c["name"] for c in R.CASES])
def test_the_twin_stays_within_the_a_priori_bound_of_the_float64_rule(index):
    case = R.CASES[index]
    tiles, tr, got = R.twin_case(index)
    ref, bound, n_cover = R.stitch_f64(tiles, tr, case["p"], case["cval"], case["box"])
    assert got.shape == ref.shape
    assert np.all(got[n_cover == 0] == np.float32(case["cval"]))
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))
    print(f"{case['name']}: worst |got - ref| / bound = {ratio:.3f}, up to {int(n_cover.max())} tiles on a voxel")
    assert np.all(err <= bound)
    assert n_cover.max() >= (5 if case["name"] == "five_cover" else 1)


def test_zeros_stay_zeros_and_a_nan_stays_under_its_tile():
    shapes, tr = [(2, 6, 40), (2, 6, 40)], [(0, 0, 0), (0, 2.5, 30)]
    got = _stitch([np.zeros(s, dtype=np.float32) for s in shapes], tr, p=1, cval=3.0)
    _, _, n_cover = R.stitch_f64([np.zeros(s) for s in shapes], tr, 1, 3.0)
    assert np.array_equal(got[n_cover > 0].view(np.uint32), np.zeros(int((n_cover > 0).sum()), dtype=np.uint32))
    tiles = [R.f32_tile(s, 9 + k) for k, s in enumerate(shapes)]
    tiles[1][1, 3, 5] = np.nan
    got = _stitch(tiles, tr, p=1, cval=0.0)
    want = np.zeros(got.shape, dtype=bool)
    want[1, 5:7, 35] = True                 # the taps j - 1 and j along y: canvas rows 3 + 2 and 3 + 3
    assert np.array_equal(np.isnan(got), want)


# ---- bands --------------------------------------------------------------------------------------------------------------------


def test_banded_equals_whole_bit_for_bit_and_keeps_tile_order():
    case = R.CASES[[c["name"] for c in R.CASES].index("five_cover")]
    tiles, tr = R.make_case(case)
    shapes = [t.shape for t in tiles]
    whole = _stitch(tiles, tr, case["p"], case["cval"])
    ny = whole.shape[1]
    for rows in (1, 3, ny):
        loads = []

        def load(k):
            loads.append(k)
            return _t(tiles[k])

        got = S.stitch_banded(load, shapes, tr, case["p"], case["cval"], band_rows=rows).numpy()
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), f"bands of {rows} rows"
        assert sorted(loads) == list(range(len(tiles))), "every tile is loaded exactly once"
        plan = S.band_plan(shapes, tr, rows)
        assert all(ks == sorted(ks) for _, _, ks in plan)
        assert plan[0][0] == S.canvas_geometry(shapes, tr)[1][1] and plan[-1][1] == plan[0][0] + ny
        first = np.floor(np.asarray(tr)[:, 1])
        for y0, y1, ks in plan:
            assert ks == [k for k in range(len(tiles)) if first[k] < y1 and first[k] + shapes[k][1] - 1 >= y0]
    # a budget picks the band height; one that not even single rows meet is refused
    peak = 4 * (whole.size + sum(int(np.prod(s)) for s in shapes))
    got = S.stitch_banded(lambda k: _t(tiles[k]), shapes, tr, case["p"], case["cval"], max_resident_bytes=peak).numpy()
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    with pytest.raises(ValueError):
        S.stitch_banded(lambda k: _t(tiles[k]), shapes, tr, case["p"], case["cval"], max_resident_bytes=4 * whole.size)


# ---- entry statuses -------------------------------------------------------------------------------------------------------------


def test_entry_statuses():
    lib = _lib.load()
    cap = lib.lsr_stitch_max_tiles()
    assert cap >= 64 and lib.lsr_stitch_table_bytes(2) == 2 * lib.lsr_stitch_table_bytes(1) > 0
    assert lib.lsr_stitch_table_bytes(cap + 1) == 0 and lib.lsr_stitch_table_bytes(0) == 0
    i64p, f64p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    tile = np.ones((2, 3, 4), dtype=np.float32)
    out = np.full((2, 3, 4), 9.0, dtype=np.float32)
    n = cap + 1
    table = np.zeros(lib.lsr_stitch_table_bytes(1) * n, dtype=np.uint8)

    def prepare(ptrs, shapes, trs, count):
        shp, tr = np.asarray(shapes, dtype=np.int64), np.asarray(trs, dtype=np.float64)
        return lib.lsr_stitch_prepare_table((ctypes.c_void_p * len(ptrs))(*ptrs), shp.ctypes.data_as(i64p),
                                            tr.ctypes.data_as(f64p), count, table.ctypes.data)

    p = tile.ctypes.data
    assert prepare([p] * n, [(2, 3, 4)] * n, [(0, 0, 0)] * n, n) == -3 and b"at most" in lib.lsr_last_error()
    assert prepare([p, None], [(2, 3, 4)] * 2, [(0, 0, 0)] * 2, 2) == -1 and b"tile 1 is NULL" in lib.lsr_last_error()
    assert prepare([p, p], [(2, 3, 4), (2, 0, 4)], [(0, 0, 0)] * 2, 2) == -2
    assert prepare([p], [(2, 3, 4)], [(0, np.inf, 0)], 1) == -4
    assert prepare([p], [(1, 2 ** 24 + 1, 1)], [(0, 0, 0)], 1) == -3          # (y, x extents: exact float conversions)
    assert prepare([p], [(1, 1, 2 ** 24 + 1)], [(0, 0, 0)], 1) == -3
    assert prepare([p], [(2, 3, 4)], [(0, 0, 0)], 0) == -2
    assert prepare([p], [(2, 3, 4)], [(0, 0, 0)], 1) == 0
    o3, s3 = (ctypes.c_int64 * 3)(0, 0, 0), (ctypes.c_int64 * 3)(2, 3, 4)
    for name in ("lsr_stitch_f32_cpu", "lsr_stitch_f32"):        # (checked before anything is launched: safe without a GPU)
        fn = getattr(lib, name)
        assert fn(table.ctypes.data, n, out.ctypes.data, o3, s3, 1, 0.0, None) == -3
        assert fn(None, 1, out.ctypes.data, o3, s3, 1, 0.0, None) == -1
        assert fn(table.ctypes.data, 1, None, o3, s3, 1, 0.0, None) == -1
        assert fn(table.ctypes.data, 1, out.ctypes.data, o3, (ctypes.c_int64 * 3)(2, 0, 4), 1, 0.0, None) == -2
        assert fn(table.ctypes.data, 1, out.ctypes.data, o3, s3, 5, 0.0, None) == -4
    assert np.all(out == 9.0), "a refused call wrote something"
    # the twin reads its table: a null tile and a non-positive extent in it are statuses too
    good = table[:lib.lsr_stitch_table_bytes(1)].copy()
    bad = good.copy()
    bad[:8] = 0
    assert lib.lsr_stitch_f32_cpu(bad.ctypes.data, 1, out.ctypes.data, o3, s3, 1, 0.0, None) == -1
    bad = good.copy()
    bad[8:16] = 0
    assert lib.lsr_stitch_f32_cpu(bad.ctypes.data, 1, out.ctypes.data, o3, s3, 1, 0.0, None) == -2
    assert lib.lsr_stitch_f32_cpu(good.ctypes.data, 1, out.ctypes.data, o3, s3, 1, 0.0, None) == 0 and np.all(out == 1.0)
    with pytest.raises(_lib.LsrError):
        S.stitch_tiles([_t(tile)], [(0, 0, 0)], blending_exponent=7)
    with pytest.raises(TypeError):
        S.stitch_tiles([_t(tile.astype(np.float64))], [(0, 0, 0)])


# ---- settings -------------------------------------------------------------------------------------------------------------------


def test_settings_round_trip(tmp_path):
    est = EstimateStitchSettings(channel="GFP", initial_placement="grid", grid_columns=2, percent_overlap=10.0)
    est.to_yaml(tmp_path / "est.yml")
    assert EstimateStitchSettings.from_yaml(tmp_path / "est.yml") == est
    with pytest.raises(ValueError):
        EstimateStitchSettings(channel="GFP", initial_placement="grid")
    with pytest.raises(ValueError):
        EstimateStitchSettings(channel="GFP", unknown_field=1)
    s = StitchSettings(total_translation={"A/1/000": [0, 0, 0], "A/1/001": [0.0, 1.5, 40.0]}, blending_exponent=2, cval=1.0)
    s.to_yaml(tmp_path / "stitch.yml")
    again = StitchSettings.from_yaml(tmp_path / "stitch.yml")
    assert again == s and again.total_translation["A/1/001"] == [0.0, 1.5, 40.0]
    for bad in (dict(total_translation={}), dict(total_translation={"a": [0, 0]}),
                dict(total_translation={"a": [0, 0, 0]}, blending_exponent=5)):
        with pytest.raises(ValueError):
            StitchSettings(**bad)


# ---- the placement estimate -------------------------------------------------------------------------------------------------------

ESTIMATE, grid = R.ESTIMATE, R.grid


@pytest.mark.parametrize("rows,cols", [(2, 2), (2, 3)])
def test_estimate_translations_recovers_the_true_offsets_exactly(rows, cols):
    names, tiles, nominal, true = grid(rows, cols)
    assert any(tuple(nominal[n]) != tuple(true[n]) for n in names[1:])
    got = S.estimate_translations({n: _t(tiles[n]) for n in names}, {n: tiles[n].shape for n in names}, nominal, ESTIMATE)
    assert list(got) == names and got[names[0]] == nominal[names[0]]             # tile 0 is pinned
    for n in names:
        rel = tuple(a - b for a, b in zip(got[n], got[names[0]]))
        assert rel == tuple(float(a - b) for a, b in zip(true[n], true[names[0]])), n
    # the loader form asks for the overlaps only
    asked = []

    order = []

    def loader(name, sl):
        asked.append(tuple(s.stop - s.start for s in sl))
        order.append(name)
        return tiles[name][sl]

    assert S.estimate_translations(loader, [tiles[n].shape for n in names], nominal, ESTIMATE) == got
    assert asked and all(int(np.prod(a)) < tiles[names[0]].size // 2 for a in asked)
    # ... all of one tile in a row, so a loader that reads whole volumes reads each once
    assert [n for k, n in enumerate(order) if k == 0 or order[k - 1] != n] == names
    # the stitched canvas is the scene where one tile covers it
    tr = [got[n] for n in names]
    canvas = S.stitch_tiles([_t(tiles[n]) for n in names], tr, 0).numpy()
    _, origin = S.canvas_geometry([tiles[n].shape for n in names], tr)
    a = tiles[names[-1]]
    o = [int(t - g) for t, g in zip(tr[-1], origin)]
    corner = canvas[o[0]:o[0] + a.shape[0], o[1]:o[1] + a.shape[1], o[2]:o[2] + a.shape[2]]
    assert np.array_equal(corner[:, -8:, -8:], a[:, -8:, -8:])


def test_a_featureless_pair_is_rejected_and_a_lone_tile_keeps_its_placement(caplog):
    names, tiles, nominal, true = grid(2, 2)
    tiles = dict(tiles)
    tiles[names[3]] = np.full_like(tiles[names[3]], 5.0)              # a constant tile: nothing to correlate
    with caplog.at_level(logging.INFO, logger="shrimpy_amd"):
        got = S.estimate_translations({n: _t(tiles[n]) for n in names}, {n: tiles[n].shape for n in names}, nominal, ESTIMATE)
    assert got[names[3]] == nominal[names[3]]
    assert any("without a pair" in r.message and names[3] in r.getMessage() for r in caplog.records)
    assert sum("featureless" in r.message for r in caplog.records) == 3
    for n in names[:3]:                                               # the others are where they were without it
        rel = tuple(a - b for a, b in zip(got[n], got[names[0]]))
        assert rel == tuple(float(a - b) for a, b in zip(true[n], true[names[0]]))


def test_solve_placement_drops_outliers_and_pins_unconnected_groups():
    anchors = [(0, 0, 0), (0, 0, 10), (0, 10, 0), (0, 10, 10), (5, 5, 5)]
    meas = [(0, 1, (0, 1, 12)), (0, 2, (1, 11, 0)), (1, 3, (1, 11, 0)), (2, 3, (0, 1, 12)),
            (0, 3, (9, 2, 2))]                                         # the last one contradicts the other four
    t, kept, pinned = S.solve_placement(5, anchors, meas, 1.0)
    assert len(kept) == 4 and pinned == [4]
    assert np.allclose(t, [(0, 0, 0), (0, 1, 12), (1, 11, 0), (1, 12, 12), (5, 5, 5)], atol=1e-12)
    assert S.grid_placement([(4, 100, 200)] * 3, 2, 10.0) == [(0.0, 0.0, 0.0), (0.0, 0.0, 180.0), (0.0, 90.0, 0.0)]


# ---- the commands ---------------------------------------------------------------------------------------------------------------

SCALE = (1.0, 1.0, 0.5, 0.25, 0.25)


@pytest.fixture
def cpu_cli(monkeypatch):
    import shrimpy_amd.cli as cli

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return cli


def make_tiled_plate(path, wells=("A/1", "B/2"), dtype=np.uint16):
    """Two wells of 2 x 2 tiles cut from a scene each; NGFF translations hold the NOMINAL stage positions.  Returns
    ``{well: (names, tiles, nominal, true)}`` with uint16-valued tiles."""
    from shrimpy_amd.io.omezarr import open_ome_zarr

    truth = {}
    with open_ome_zarr(path, layout="hcs", mode="w", channel_names=["GFP", "BF"], version="0.5", prefer_iohub=False) as plate:
        for w, well in enumerate(wells):
            names, tiles, nominal, true = R.grid_tiles(2, 2, seed=30 + w, tile=(8, 40, 48), step=30, jitter=2)
            row, col = well.split("/")
            keys = [f"{well}/{n.rsplit('/', 1)[1]}" for n in names]
            tiles = {k: np.clip(np.rint(tiles[n]), 0, 65535).astype(dtype) for k, n in zip(keys, names)}
            for k, n in zip(keys, names):
                tr = [0.0, 0.0] + [v * s for v, s in zip(nominal[n], SCALE[2:])]
                arr = plate.create_position(row, col, k.rsplit("/", 1)[1]).create_zeros(
                    "0", shape=(2, 2) + tiles[k].shape, dtype=dtype, scale=SCALE, translation=tr)
                for t in range(2):
                    arr.write_volume(t, 0, tiles[k] + dtype(t))
                    arr.write_volume(t, 1, tiles[k] // dtype(2))
            truth[well] = (keys, tiles, {k: nominal[n] for k, n in zip(keys, names)}, {k: true[n] for k, n in zip(keys, names)})
    return truth


def test_cli_estimate_stitch_then_stitch_with_two_levels(tmp_path, cpu_cli):
    from click.testing import CliRunner

    from shrimpy_amd import pyramid as P
    from shrimpy_amd.io.omezarr import open_ome_zarr

    truth = make_tiled_plate(tmp_path / "tiles.zarr")
    cfg = tmp_path / "estimate.yml"
    cfg.write_text(yaml.safe_dump(dict(ESTIMATE, initial_placement="metadata")))
    r = CliRunner().invoke(cpu_cli.cli, ["estimate-stitch", "-i", str(tmp_path / "tiles.zarr"), "-c", str(cfg), "-o",
                                         str(tmp_path / "stitch.yml")])
    assert r.exit_code == 0, r.output
    settings = StitchSettings.from_yaml(tmp_path / "stitch.yml")          # what estimate-stitch wrote loads unchanged
    assert sorted(settings.total_translation) == sorted(k for w in truth.values() for k in w[0])
    for keys, _, _, true in truth.values():
        for k in keys:
            rel = [a - b for a, b in zip(settings.total_translation[k], settings.total_translation[keys[0]])]
            assert rel == [float(a - b) for a, b in zip(true[k], true[keys[0]])]
    out = tmp_path / "out.zarr"
    r = CliRunner().invoke(cpu_cli.cli, ["stitch", "-i", str(tmp_path / "tiles.zarr"), "-c", str(tmp_path / "stitch.yml"), "-o",
                                         str(out), "--levels", "2"])
    assert r.exit_code == 0, r.output
    with open_ome_zarr(out, prefer_iohub=False) as plate:
        positions = dict(plate.positions())
        assert sorted(positions) == ["A/1/0", "B/2/0"]                  # one position per well
        for well, (keys, tiles, _, _) in truth.items():
            pos = positions[well + "/0"]
            tr = [settings.total_translation[k] for k in keys]
            shape, origin = S.canvas_geometry([tiles[k].shape for k in keys], tr)
            assert pos.levels == ["0", "1"] and list(pos.channel_names) == ["GFP", "BF"]
            assert pos["0"].shape == (2, 2) + shape and pos["0"].dtype == np.float32
            d0, d1 = pos.zattrs["multiscales"][0]["datasets"]
            assert d0["coordinateTransformations"][0]["scale"] == list(SCALE)
            want_tr = [0.0, 0.0] + [o * s for o, s in zip(origin, SCALE[2:])]
            got_tr = [t for t in d0["coordinateTransformations"] if t["type"] == "translation"]
            assert (got_tr[0]["translation"] if got_tr else [0.0] * 5) == pytest.approx(want_tr, abs=1e-12)
            assert d1["coordinateTransformations"][0]["scale"] == [1.0, 1.0, 1.0, 0.5, 0.5]
            for t, c in ((0, 0), (1, 0), (1, 1)):
                vols = [(tiles[k] + np.uint16(t) if c == 0 else tiles[k] // np.uint16(2)).astype(np.float32) for k in keys]
                want = S.stitch_tiles([_t(v) for v in vols], tr, settings.blending_exponent, settings.cval)
                got = pos["0"].read_volume(t, c)
                assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
                assert np.array_equal(pos["1"].read_volume(t, c), P.downsample2(want, 2).numpy())
    # the output is never overwritten
    r = CliRunner().invoke(cpu_cli.cli, ["stitch", "-i", str(tmp_path / "tiles.zarr"), "-c", str(tmp_path / "stitch.yml"), "-o",
                                         str(out)])
    assert r.exit_code != 0
