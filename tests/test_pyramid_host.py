"""Multiscale pyramids on the host: the twins of the downsampling kernel (``lsr_downsample2_*_cpu``) against
``tests/pyramid_ref.py``, the level geometry, the store metadata, ``--levels`` through the CLI and the ``pyramid`` command.

iohub is not installed: PARITY IS UNPINNED and ``pyramid_ref`` (float64 / int64 NumPy) is the oracle.  The float32 bound is
a-priori (three roundings, ``pyramid_ref``'s docstring); the uint16 result is exact.
"""

import ctypes
import json

import numpy as np
import pytest
import torch
import yaml

from shrimpy_amd import _lib
from shrimpy_amd import pyramid as P
from shrimpy_amd.io.omezarr import create_level, create_pyramid, open_ome_zarr
from tests import pyramid_ref as R

CASES = [(s, fz) for s in R.SHAPES for fz in R.FZ]


def _twin(vol: np.ndarray, fz: int, fill) -> np.ndarray:
    """The host twin through the C ABI, into a buffer that is `fill` everywhere before the call."""
    name = {"float32": "lsr_downsample2_f32_cpu", "uint16": "lsr_downsample2_u16_cpu"}[vol.dtype.name]
    out = np.full(R.out_shape(vol.shape, fz), fill, dtype=vol.dtype)
    _lib.call(name, vol.ctypes.data, *vol.shape, out.ctypes.data, fz, None)
    return out


@pytest.mark.parametrize("shape,fz", CASES)
def test_float32_twin_is_within_three_roundings_of_the_float64_mean(shape, fz):
    vol = R.f32_volume(shape, seed=sum(shape) + fz)
    got = _twin(vol, fz, np.nan)
    assert not np.isnan(got).any(), "an output voxel was not written"
    err = np.abs(got.astype(np.float64) - R.downsample2_f64(vol, fz))
    bound = R.bound_f32(vol, fz)
    print(f"{shape} fz={fz}: worst |got - ref| / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # ... and the public function is that twin
    assert np.array_equal(P.downsample2(torch.from_numpy(vol), fz).numpy(), got)


@pytest.mark.parametrize("shape,fz", CASES)
def test_uint16_twin_equals_the_integer_formula(shape, fz):
    vol = R.u16_volume(shape, seed=sum(shape) + fz)
    got = _twin(vol, fz, 12345)
    assert np.array_equal(got, R.downsample2_u16(vol, fz))
    assert np.array_equal(P.downsample2(torch.from_numpy(vol), fz).numpy(), got)


@pytest.mark.parametrize("fz", R.FZ)
@pytest.mark.parametrize("at", [(1, 2, 3), (4, 6, 8), (2, 6, 3), (4, 1, 8)])    # a full window; corner, y-edge and z/x-edge partials
def test_a_nan_reaches_exactly_the_window_that_holds_it(at, fz):
    vol = R.f32_volume((5, 7, 9), seed=3)
    vol[at] = np.nan
    got = _twin(vol, fz, 0.0)
    want = np.zeros(got.shape, dtype=bool)
    want[at[0] // fz, at[1] // 2, at[2] // 2] = True
    assert np.array_equal(np.isnan(got), want)
    clean = R.f32_volume((5, 7, 9), seed=3)
    assert np.array_equal(got[~want], _twin(clean, fz, 0.0)[~want])


def test_level_shapes_are_ceilings_and_levels_cascade():
    for shape in R.SHAPES:
        for fz in R.FZ:
            shapes, factors = P.level_shapes(shape, 4, fz)
            for k in range(4):
                assert shapes[k] == tuple(-(-n // f ** k) for n, f in zip(shape, (fz, 2, 2)))
                assert factors[k] == (fz ** k, 2 ** k, 2 ** k)
    vol = torch.from_numpy(R.f32_volume((7, 33, 67), seed=1))
    for fz in R.FZ:
        levels = P.build_levels(vol, 3, fz)
        assert [tuple(lv.shape) for lv in levels] == P.level_shapes(vol.shape, 3, fz)[0][1:]
        assert torch.equal(levels[1], P.downsample2(P.downsample2(vol, fz), fz))
    assert P.build_levels(vol, 1) == []
    for bad in (0, 9):
        with pytest.raises(ValueError):
            P.level_shapes((4, 4, 4), bad)
    with pytest.raises(ValueError):
        P.downsample2(vol, 3)
    with pytest.raises(TypeError):
        P.downsample2(vol.to(torch.float64))


def test_entry_points_refuse_bad_arguments_with_a_message():
    lib = _lib.load()
    vol = np.ones((2, 2, 2), dtype=np.float32)
    out = np.ones((2, 2, 2), dtype=np.float32)
    out3 = (ctypes.c_int64 * 3)()

    def refused(rc):
        assert rc < 0
        assert lib.lsr_last_error().decode()
        return rc

    for name in ("lsr_downsample2_f32_cpu", "lsr_downsample2_u16_cpu", "lsr_downsample2_f32", "lsr_downsample2_u16"):
        fn = getattr(lib, name)
        for fz in (0, 3, -1):
            assert refused(fn(vol.ctypes.data, 2, 2, 2, out.ctypes.data, fz, None)) == -4
        for shape in ((0, 2, 2), (2, 0, 2), (2, 2, -1)):
            assert refused(fn(vol.ctypes.data, *shape, out.ctypes.data, 2, None)) == -2
        assert refused(fn(None, 2, 2, 2, out.ctypes.data, 2, None)) == -1
        assert refused(fn(vol.ctypes.data, 2, 2, 2, None, 2, None)) == -1
        assert refused(fn(vol.ctypes.data, 2, 2, 2, vol.ctypes.data, 2, None)) == -4
    assert refused(lib.lsr_downsample2_shape(2, 2, 2, 3, out3)) == -4
    assert refused(lib.lsr_downsample2_shape(0, 2, 2, 2, out3)) == -2
    assert refused(lib.lsr_downsample2_shape(2, 2, 2, 2, None)) == -1
    assert lib.lsr_downsample2_shape(5, 7, 9, 1, out3) == 0 and tuple(out3) == (5, 4, 5)
    assert np.all(out == 1.0), "a refused call wrote something"


# ---- store metadata -------------------------------------------------------------------------------------------------

SCALE = (1.0, 1.0, 0.4, 0.1133, 0.1133)


def _group_json(pos_path, version):
    return (pos_path / ("zarr.json" if version == "0.5" else ".zattrs")).read_text()


@pytest.mark.parametrize("version", ["0.4", "0.5"])
@pytest.mark.parametrize("fz", R.FZ)
def test_create_pyramid_lists_every_level_with_its_scale_and_translation(tmp_path, version, fz):
    shape5 = (2, 1, 5, 7, 9)
    base_tr = [0.0, 0.0, 0.8, -1.133, 0.0]
    with open_ome_zarr(tmp_path / "p.zarr", layout="hcs", mode="w", channel_names=["A"], version=version,
                       prefer_iohub=False) as plate:
        pos = plate.create_position("0", "0", "0")
        arrays = create_pyramid(pos, shape5, "float32", SCALE, 3, fz, translation=base_tr, compress="zstd")
    assert [a.shape for a in arrays] == [(2, 1) + s for s in P.level_shapes(shape5[2:], 3, fz)[0]]
    with open_ome_zarr(tmp_path / "p.zarr", prefer_iohub=False) as plate:
        pos = plate["0/0/0"]
        assert pos.levels == ["0", "1", "2"]
        assert pos.scale == SCALE                                     # level 0, as before
        ms = pos.zattrs["multiscales"]
        assert len(ms) == 1 and ms[0]["type"] == "mean" and len(ms[0]["datasets"]) == 3
        for k, d in enumerate(ms[0]["datasets"]):
            f = (1, 1, fz ** k, 2 ** k, 2 ** k)
            scale, tr = d["coordinateTransformations"]
            assert d["path"] == str(k) and scale["type"] == "scale" and tr["type"] == "translation"
            assert scale["scale"] == pytest.approx([s * q for s, q in zip(SCALE, f)], rel=1e-15)
            assert tr["translation"] == pytest.approx(
                [b + ((q - 1) / 2.0 * s if i >= 2 else 0.0) for i, (b, s, q) in enumerate(zip(base_tr, SCALE, f))], rel=1e-15)
            assert pos[str(k)].shape == arrays[k].shape and pos[str(k)].dtype == np.float32
    # without a translation level 0 has none and the lower levels the half-voxel offsets alone
    with open_ome_zarr(tmp_path / "q.zarr", layout="hcs", mode="w", channel_names=["A"], version=version,
                       prefer_iohub=False) as plate:
        create_pyramid(plate.create_position("0", "0", "0"), shape5, "uint16", SCALE, 2, fz)
    with open_ome_zarr(tmp_path / "q.zarr", prefer_iohub=False) as plate:
        d0, d1 = plate["0/0/0"].zattrs["multiscales"][0]["datasets"]
        assert [t["type"] for t in d0["coordinateTransformations"]] == ["scale"]
        assert d1["coordinateTransformations"][1]["translation"] == pytest.approx(
            [0.0, 0.0, (fz - 1) / 2.0 * SCALE[2], 0.5 * SCALE[3], 0.5 * SCALE[4]], rel=1e-15)


@pytest.mark.parametrize("version", ["0.4", "0.5"])
def test_one_level_is_create_level_byte_for_byte(tmp_path, version):
    shape5 = (1, 2, 5, 7, 9)
    texts = []
    for name, make in (("a", lambda pos: create_level(pos, shape5, "float32", SCALE, compress="zstd")),
                       ("b", lambda pos: create_pyramid(pos, shape5, "float32", SCALE, 1, 2, compress="zstd"))):
        with open_ome_zarr(tmp_path / f"{name}.zarr", layout="hcs", mode="w", channel_names=["A", "B"], version=version,
                           prefer_iohub=False) as plate:
            pos = plate.create_position("0", "0", "0")
            make(pos)
            assert pos.levels == ["0"]
        root = tmp_path / f"{name}.zarr" / "0" / "0" / "0"
        texts.append((_group_json(root, version), sorted(p.name for p in root.iterdir()),
                      (root / "0" / ("zarr.json" if version == "0.5" else ".zarray")).read_text()))
    assert texts[0] == texts[1]
    doc = json.loads(texts[1][0])
    assert "type" not in (doc["attributes"]["ome"] if version == "0.5" else doc)["multiscales"][0]


# ---- the command line on the CPU --------------------------------------------------------------------------------------

KEYS = ["0/0/000", "0/1/000"]
RAW = (24, 8, 20)


@pytest.fixture
def cpu_cli(monkeypatch):
    import shrimpy_amd.cli as cli

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return cli


def make_raw_plate(path, dtype=np.uint16, n_t=2, compress=None, version="0.5"):
    rng = np.random.default_rng(11)
    with open_ome_zarr(path, layout="hcs", mode="w", channel_names=["BF"], version=version, prefer_iohub=False) as plate:
        for key in KEYS:
            arr = plate.create_position(*key.split("/")).create_zeros(
                "0", shape=(n_t, 1) + RAW, dtype=dtype, scale=(1, 1, 0.15, 0.1133, 0.1133), compress=compress)
            for t in range(n_t):
                arr.write_volume(t, 0, rng.integers(80, 60000, RAW).astype(dtype))
    return path


def deskew_config(tmp_path):
    cfg = tmp_path / "deskew.yml"
    cfg.write_text(yaml.safe_dump(dict(pixel_size_um=0.1133, ls_angle_deg=30.0, scan_step_um=0.15, keep_overhang=True,
                                       average_n_slices=3)))
    return cfg


def read_levels(path):
    """{key: [[level k of (t, 0) for t] for k]} and {key: attributes}."""
    data, attrs = {}, {}
    with open_ome_zarr(path, prefer_iohub=False) as plate:
        for key, pos in plate.positions():
            attrs[key] = pos.zattrs
            data[key] = [[pos[lv].read_volume(t, 0) for t in range(pos[lv].shape[0])] for lv in pos.levels]
    return data, attrs


def check_cascade(data, attrs, levels, fz):
    for key in KEYS:
        assert len(attrs[key]["multiscales"][0]["datasets"]) == levels == len(data[key])
        for k in range(1, levels):
            for above, got in zip(data[key][k - 1], data[key][k]):
                want = P.downsample2(torch.from_numpy(np.ascontiguousarray(above)), fz).numpy()
                assert got.dtype == above.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("compression", ["blosc-zstd", "none"])
def test_cli_deskew_writes_three_levels_that_cascade(tmp_path, cpu_cli, compression):
    from click.testing import CliRunner

    src, cfg = make_raw_plate(tmp_path / "raw.zarr"), deskew_config(tmp_path)
    out = tmp_path / "out.zarr"
    r = CliRunner().invoke(cpu_cli.cli, ["deskew", "-i", str(src), "-c", str(cfg), "-o", str(out), "--levels", "3",
                                         "--compression", compression])
    assert r.exit_code == 0, r.output
    data, attrs = read_levels(out)
    check_cascade(data, attrs, 3, 2)
    assert data[KEYS[0]][0][0].dtype == np.float32 and np.abs(data[KEYS[0]][2][1]).max() > 0
    assert attrs[KEYS[0]]["multiscales"][0]["type"] == "mean"


def test_cli_level_factor_z_one_keeps_the_z_extent(tmp_path, cpu_cli):
    from click.testing import CliRunner

    src, cfg = make_raw_plate(tmp_path / "raw.zarr"), deskew_config(tmp_path)
    out = tmp_path / "out.zarr"
    r = CliRunner().invoke(cpu_cli.cli, ["deskew", "-i", str(src), "-c", str(cfg), "-o", str(out), "--levels", "2",
                                         "--level-factor-z", "1", "--zarr-version", "0.4"])
    assert r.exit_code == 0, r.output
    data, attrs = read_levels(out)
    check_cascade(data, attrs, 2, 1)
    assert data[KEYS[0]][1][0].shape[0] == data[KEYS[0]][0][0].shape[0]


def test_cli_one_level_is_the_run_without_the_option(tmp_path, cpu_cli):
    from click.testing import CliRunner

    src, cfg = make_raw_plate(tmp_path / "raw.zarr"), deskew_config(tmp_path)
    for name, extra in (("plain", []), ("one", ["--levels", "1", "--level-factor-z", "1"])):
        r = CliRunner().invoke(cpu_cli.cli, ["deskew", "-i", str(src), "-c", str(cfg), "-o", str(tmp_path / name), *extra])
        assert r.exit_code == 0, r.output
    files = {}
    for name in ("plain", "one"):
        root = tmp_path / name
        files[name] = {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}
    assert files["plain"].keys() == files["one"].keys()
    assert files["plain"] == files["one"]          # arrays, metadata and the run's fingerprint


def test_resume_rewrites_every_level_of_an_unfinished_unit_and_refuses_other_levels(tmp_path, cpu_cli):
    from click.testing import CliRunner

    src, cfg = make_raw_plate(tmp_path / "raw.zarr"), deskew_config(tmp_path)
    out = tmp_path / "out.zarr"
    args = ["deskew", "-i", str(src), "-c", str(cfg), "-o", str(out)]
    r = CliRunner().invoke(cpu_cli.cli, args + ["--levels", "3"])
    assert r.exit_code == 0, r.output
    first, _ = read_levels(out)
    # unit (KEYS[1], t = 1) loses its completion record, and every level of it its content
    (out / ".lsr_done" / KEYS[1].replace("/", "__") / "t1_c0").unlink()
    with open_ome_zarr(out, mode="a", prefer_iohub=False) as plate:
        pos = plate[KEYS[1]]
        for lv in pos.levels:
            pos[lv].write_volume(1, 0, np.zeros(pos[lv].shape[2:], dtype=np.float32))
    damaged, _ = read_levels(out)
    assert all(not damaged[KEYS[1]][k][1].any() for k in range(3))
    r = CliRunner().invoke(cpu_cli.cli, args + ["--levels", "3", "--resume"])
    assert r.exit_code == 0, r.output
    assert "'units': 1," in r.output and "'units_skipped': 3" in r.output
    again, _ = read_levels(out)
    for key in KEYS:
        for k in range(3):
            for a, b in zip(first[key][k], again[key][k]):
                assert np.array_equal(a, b)
    # another --levels is another run
    for other in ("2", "1", "4"):
        r = CliRunner().invoke(cpu_cli.cli, args + ["--levels", other, "--resume"])
        assert r.exit_code != 0 and "different input or with different settings" in r.output, r.output


def test_levels_through_iohub_are_refused(tmp_path, cpu_cli):
    from click.testing import CliRunner

    src, cfg = make_raw_plate(tmp_path / "raw.zarr"), deskew_config(tmp_path)
    r = CliRunner().invoke(cpu_cli.cli, ["deskew", "-i", str(src), "-c", str(cfg), "-o", str(tmp_path / "o.zarr"),
                                         "--io", "iohub", "--levels", "2"])
    assert r.exit_code != 0 and "--io iohub" in r.output and "--levels" in r.output
    assert len(r.output.strip().splitlines()) <= 2 and not (tmp_path / "o.zarr").exists()
    r = CliRunner().invoke(cpu_cli.cli, ["deskew", "-i", str(src), "-c", str(cfg), "-o", str(tmp_path / "o.zarr"),
                                         "--levels", "9"])
    assert r.exit_code == 2                         # click's own range check


# ---- the pyramid command ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,compress,version", [(np.uint16, "blosc-zstd", "0.5"), (np.float32, None, "0.4"),
                                                    (np.float32, "zstd", "0.5")])
def test_pyramid_command_adds_levels_in_place(tmp_path, cpu_cli, dtype, compress, version):
    from click.testing import CliRunner

    store = make_raw_plate(tmp_path / "s.zarr", dtype=dtype, compress=compress, version=version)
    before = {p: (p.stat().st_mtime_ns, p.read_bytes()) for key in KEYS for p in sorted((store / key / "0").rglob("*"))
              if p.is_file()}                                                       # level 0's files
    assert before
    _, attrs0 = read_levels(store)
    r = CliRunner().invoke(cpu_cli.cli, ["pyramid", "-i", str(store), "--levels", "3"])
    assert r.exit_code == 0, r.output
    data, attrs = read_levels(store)
    check_cascade(data, attrs, 3, 2)
    assert data[KEYS[0]][1][0].dtype == np.dtype(dtype)
    for p, (mtime, blob) in before.items():
        assert p.stat().st_mtime_ns == mtime and p.read_bytes() == blob, f"{p} was touched"
    for key in KEYS:
        ms = attrs[key]["multiscales"][0]
        assert ms["type"] == "mean" and ms["datasets"][0] == attrs0[key]["multiscales"][0]["datasets"][0]
        assert attrs[key]["omero"] == attrs0[key]["omero"]
        assert ms["datasets"][2]["coordinateTransformations"][0]["scale"] == pytest.approx(
            [1, 1, 0.15 * 4, 0.1133 * 4, 0.1133 * 4], rel=1e-15)
        assert ms["datasets"][2]["coordinateTransformations"][1]["translation"] == pytest.approx(
            [0, 0, 0.15 * 1.5, 0.1133 * 1.5, 0.1133 * 1.5], rel=1e-15)
    with open_ome_zarr(store, prefer_iohub=False) as plate:
        pos = plate[KEYS[0]]
        assert pos["1"]._codec.kind == pos["0"]._codec.kind and pos["1"]._codec.params == pos["0"]._codec.params
    # a second run only finds stores that have their levels
    r = CliRunner().invoke(cpu_cli.cli, ["pyramid", "-i", str(store), "--levels", "4"])
    assert r.exit_code != 0 and "already has a level '1'" in r.output
    after, _ = read_levels(store)
    assert len(after[KEYS[0]]) == 3


def test_pyramid_command_refuses_other_data_types_and_one_position(tmp_path, cpu_cli):
    from click.testing import CliRunner

    store = make_raw_plate(tmp_path / "s.zarr", dtype=np.int32)
    r = CliRunner().invoke(cpu_cli.cli, ["pyramid", "-i", str(store), "--levels", "2"])
    assert r.exit_code != 0 and "uint16 and float32" in r.output
    assert not (store / KEYS[0] / "1").exists()
    # -p restricts the command to one position
    store = make_raw_plate(tmp_path / "t.zarr", n_t=1)
    r = CliRunner().invoke(cpu_cli.cli, ["pyramid", "-i", str(store), "-p", KEYS[1], "--levels", "2", "--level-factor-z", "1"])
    assert r.exit_code == 0, r.output
    with open_ome_zarr(store, prefer_iohub=False) as plate:
        assert plate[KEYS[0]].levels == ["0"] and plate[KEYS[1]].levels == ["0", "1"]
        assert plate[KEYS[1]]["1"].shape == (1, 1, 24, 4, 10)


def test_metadata_json_is_plain():
    """(the level factors are written as Python floats: what json round-trips)"""
    from shrimpy_amd.io.omezarr import pyramid_datasets

    plan = pyramid_datasets((1, 1, 5, 7, 9), SCALE, 3, 2)
    assert json.loads(json.dumps(plan[2][1])) == plan[2][1] and plan[2][0] == (1, 1, 2, 2, 3)
