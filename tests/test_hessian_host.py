"""The Hessian-eigenvalue responses on the host: the twin ``lsr_hessian_response_f32_cpu`` against ``tests/hessian_ref.py`` --
``np.gradient`` twice and ``np.linalg.eigvalsh`` in float64 -- inside ``2^-23 scale ||H||_F`` on every voxel of every case, the
ordering, the NaN rule against the restated stencil, measures 3 to 7 byte for byte the numpy float32 function of the twin's own
eigenvalues, the exact quadratics, the accumulation, the entry statuses of twin and device entry alike, ``shrimpy_amd.hessian`` on
CPU tensors, the structure scene and ``enhance`` of ``segment_zyx``.

Cases: ``tests/hessian_cases.py``, sized from the exported tiling.  Worst eigenvalue error reached by the twin over all of them:
0.497 of the bound (the float32 rounding of the output alone is up to 0.5; printed by ``test_eigenvalues_within_the_bound``).
"""

import ctypes
import functools
import itertools

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from shrimpy_amd import _lib
from shrimpy_amd import hessian as K
from shrimpy_amd import segment as S
from shrimpy_amd.settings import EnhanceSettings, SegmentSettings
from tests import hessian_cases as C
from tests import hessian_ref as R
from tests import test_label_host as LH

GUARD = 64
FILL = np.float32(-7.53125)
NAN_BITS = int(R.CANONICAL_NAN)
BOUND = 2.0 ** -23


def twin_response(g, sampling, scale, measure, dark=False, accumulate=False, out=None, entry="lsr_hessian_response_f32_cpu"):
    """The twin through the C ABI into a poisoned buffer (or ``out``) with 64 guard words behind it: (out, guard)."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    z, y, x = g.shape
    buf = np.full(g.size + GUARD, FILL, dtype=np.float32)
    if out is not None:
        buf[:g.size] = np.asarray(out, dtype=np.float32).ravel()
    before = g.tobytes()
    _lib.call(entry, g.ctypes.data, buf.ctypes.data, z, y, x, *(ctypes.c_double(s) for s in sampling), ctypes.c_double(scale),
              int(measure), int(dark), int(accumulate), None)
    assert g.tobytes() == before, "the input was written"
    return buf[:g.size].reshape(g.shape), buf[g.size:]


def check_buffer(out, guard):
    assert np.all(guard == FILL), "something was written behind the output"
    assert not np.any(out == FILL), "a voxel was not written"


@functools.lru_cache(maxsize=None)
def case_twin(shape, content, sampling, measure, dark):
    """The twin's answer on a case, computed once (read-only; tests/test_hessian_gpu.py holds the device to it)."""
    out, guard = twin_response(C.case_volume(shape, content, sampling), sampling, C.SCALE, measure, dark)
    check_buffer(out, guard)
    out.setflags(write=False)
    return out


def check_eigenvalues(shape, content, sampling, dark, e):
    """``e`` -- three float32 volumes -- against the reference: the bound with no voxel excluded, exact zeros where H is 0, the
    order, the canonical NaN exactly on the restated stencil.  Returns the worst error reached in units of the bound."""
    l, norm, mask = C.reference(shape, content, sampling, dark)
    worst = 0.0
    for k in range(3):
        bits = e[k].view(np.uint32)
        assert np.array_equal(np.isnan(e[k]), mask), f"{content} dark {dark} e{k + 1}: a NaN where the stencil is finite, or none"
        assert np.all(bits[mask] == NAN_BITS), f"{content}: not the canonical NaN"
        err = np.abs(e[k].astype(np.float64) - C.SCALE * l[..., k])[~mask]
        bound = (BOUND * C.SCALE * norm)[~mask]
        assert np.all(err <= bound), f"{content} dark {dark} e{k + 1}: {np.max(err / np.maximum(bound, 1e-300)):.3f} of the bound"
        assert np.all(e[k][~mask][bound == 0] == 0), f"{content}: H is 0 and e{k + 1} is not"
        if np.any(bound > 0):
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    keep = ~mask
    assert np.all(e[0][keep] <= e[1][keep]) and np.all(e[1][keep] <= e[2][keep]), f"{content} dark {dark}: the order"
    return worst


# ---- the twin against the restatement ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape,sampling", C.PARAMS, ids=C.PARAM_IDS)
def test_eigenvalues_within_the_bound(shape, sampling):
    worst = 0.0
    for content, dark in itertools.product(C.CONTENTS, (False, True)):
        e = [case_twin(shape, content, sampling, k, dark) for k in range(3)]
        worst = max(worst, check_eigenvalues(shape, content, sampling, dark, e))
        for measure in range(3, 8):
            want = R.response(*e, measure)
            got = case_twin(shape, content, sampling, measure, dark)
            assert got.tobytes() == want.tobytes(), f"{content} dark {dark}: {R.MEASURES[measure]} is not the function of e1, e2, e3"
    print(f"worst eigenvalue error over the case: {worst:.4f} of the bound")


@pytest.mark.parametrize("sampling", C.DYADIC, ids=["iso", "dyadic"])
def test_exact_quadratics(sampling):
    h = C.HALO
    inner = (slice(h, -h),) * 3
    for shape in (C.LARGEST, (C.TZ + 1, C.TY + 1, C.TX + 1), (5, 5, 5)):
        for content, A in C.QUADRATICS.items():
            if shape == (5, 5, 5):
                g = np.ascontiguousarray(C.volume(C.LARGEST, content, sampling)[:5, :5, :5])
                e = [twin_response(g, sampling, C.SCALE, k)[0] for k in range(3)]
                e_dark = [twin_response(g, sampling, C.SCALE, k, True)[0] for k in range(3)]
            else:
                e = [case_twin(shape, content, sampling, k, False) for k in range(3)]
                e_dark = [case_twin(shape, content, sampling, k, True) for k in range(3)]
            for outs, M in ((e, A), (e_dark, -A)):
                l = np.linalg.eigvalsh(M.astype(np.float64))
                for k in range(3):
                    got = outs[k][inner]
                    assert got.size > 0
                    if np.count_nonzero(A - np.diag(np.diag(A))) == 0:
                        assert np.all(got == np.float32(C.SCALE * l[k])), f"{content} e{k + 1}: a diagonal H is exact"
                    else:
                        err = np.abs(got.astype(np.float64) - C.SCALE * l[k])
                        assert np.all(err <= BOUND * C.SCALE * np.linalg.norm(A)), f"{content} e{k + 1}"


def test_the_derivative_and_the_nan_rule_by_hand():
    # x^2 along x on 5 voxels, s = 1: numpy's D = [1 2 4 6 7], D D = [1 1.5 2 1.5 1]; the only entry, so e3 = H_xx, e1 = e2 = 0
    g = (np.arange(5, dtype=np.float32) ** 2).reshape(1, 1, 5)
    assert twin_response(g, (1, 1, 1), 1.0, 2)[0].ravel().tolist() == [1.0, 1.5, 2.0, 1.5, 1.0]
    assert twin_response(g, (1, 1, 1), 1.0, 0)[0].ravel().tolist() == [0.0] * 5
    assert twin_response(g, (1, 1, 0.5), 2.0, 2)[0].ravel().tolist() == [8.0, 12.0, 16.0, 12.0, 8.0]
    assert twin_response(g, (1, 1, 1), 1.0, 0, dark=True)[0].ravel().tolist() == [-1.0, -1.5, -2.0, -1.5, -1.0]
    # ridge and log of the dark volume; a single voxel has no derivative
    assert twin_response(-g, (1, 1, 1), 1.0, 3)[0].ravel().tolist() == [1.0, 1.5, 2.0, 1.5, 1.0]
    assert twin_response(g, (1, 1, 1), 1.0, 7)[0].ravel().tolist() == [-1.0, -1.5, -2.0, -1.5, -1.0]
    assert twin_response(np.full((1, 1, 1), np.inf, np.float32), (1, 1, 1), 1.0, 0)[0].view(np.uint32).ravel().tolist() == [0]
    # the straight stencil of an interior voxel is itself and two steps away: a NaN one step away is not read
    line = np.zeros((1, 1, 9), dtype=np.float32)
    line[0, 0, 4] = np.nan
    got = np.isnan(twin_response(line, (1, 1, 1), 1.0, 0)[0]).ravel().tolist()
    assert got == [False, False, True, False, True, False, True, False, False]
    line[0, 0, 4], line[0, 0, 0] = 0.0, -np.inf                 # at the face: D(0) and D(1) read voxel 0, so H(0), H(1), H(2) do
    got = twin_response(line, (1, 1, 1), 1.0, 4)[0].view(np.uint32).ravel().tolist()
    assert got == [NAN_BITS] * 3 + [0] * 6


def test_accumulate_is_numpy_maximum_with_the_nan_rule():
    shape, sampling = (C.TZ + 1, C.TY + 1, C.TX + 1), C.SAMPLINGS[1]
    rng = np.random.default_rng(3)
    for content, measure in (("noise", 4), ("nonfinite", 0), ("zeros", 3), ("beads", 7)):
        stored = rng.normal(size=shape).astype(np.float32)
        stored[rng.random(size=shape) < 0.05] = np.nan
        stored[rng.random(size=shape) < 0.2] = -0.0
        stored[rng.random(size=shape) < 0.2] = 0.0
        r = case_twin(shape, content, sampling, measure, False)
        out, guard = twin_response(C.case_volume(shape, content, sampling), sampling, C.SCALE, measure, accumulate=True, out=stored)
        check_buffer(out, guard)
        assert out.tobytes() == R.accumulate(stored, r).tobytes(), f"{content} {R.MEASURES[measure]}"


def test_the_cases_aim_at_the_tiling():
    assert (C.HALO, C.TZ, C.TY, C.TX) == (2, 8, 8, 64) == K.tiling()
    for axis, t in enumerate(C.TILE):
        assert {1, 2, 3, 4, 5, t - 1, t, t + 1, 2 * t + 1} <= {s[axis] for s in C.SHAPES}
    assert max(int(np.prod(s)) for s in C.SHAPES) <= 200000 and len(C.SHAPES) <= 12
    assert tuple(R.MEASURES) == tuple(K.MEASURES) and list(K.MEASURES.values()) == list(range(8))
    # the census: per axis, every pair of distances to the volume's faces (0, 1, 2 or more on either side); every position in a
    # tile (first, second, inside, before the last, last) on an inside voxel and on the volume's last voxel
    for axis, t in enumerate(C.TILE):
        seen = {tuple(row) for s in C.SHAPES for row in C.face_classes(s[axis], t).tolist()}
        assert {c[:2] for c in seen} == set(itertools.product(range(3), repeat=2))
        tile_classes = {(0, 2), (1, 2), (2, 2), (2, 1), (2, 0)}
        assert {c[2:] for c in seen if c[:2] == (2, 2)} >= tile_classes
        assert {(min(p, 2), min(t - 1 - p, 2)) for p in ((s[axis] - 1) % t for s in C.SHAPES)} >= tile_classes
    # ... and in the largest shape, under every sampling, all of an axis's classes meet all of the other axes'
    per_axis = [np.unique(C.face_classes(n, t), axis=0) for n, t in zip(C.LARGEST, C.TILE)]
    assert all(len(p) >= 9 for p in per_axis) and (C.LARGEST, C.SAMPLINGS[2]) in C.PARAMS
    grid = np.stack(np.meshgrid(*(np.arange(n) for n in C.LARGEST), indexing="ij"), axis=-1).reshape(-1, 3)
    combined = np.concatenate([C.face_classes(n, t)[grid[:, a]] for a, (n, t) in enumerate(zip(C.LARGEST, C.TILE))], axis=1)
    assert len(np.unique(combined, axis=0)) == np.prod([len(p) for p in per_axis])
    # the non-finite sites are apart where the shape allows, and the stencil mask is neither empty nor everything
    assert len(set(C.nonfinite_sites(C.LARGEST))) == 3
    mask = R.stencil_mask(C.volume(C.LARGEST, "nonfinite"))
    assert mask.sum() == 19 + 19 + 10 and not mask[3, 0, 0]      # (two inside stencils of 19 voxels, 10 at the corner)
    # under dyadic sampling the quadratics are exact in float32
    for content, A in C.QUADRATICS.items():
        for s in C.DYADIC:
            H = R.hessian(C.volume(C.LARGEST, content, s), s)[2:-2, 2:-2, 2:-2]
            assert np.all(H == A.astype(np.float64)), content


# ---- entry statuses -------------------------------------------------------------------------------------------------------------


def test_entry_statuses():
    lib = _lib.load()
    four = (ctypes.c_int * 4)()
    assert lib.lsr_hessian_tiling(four) == 0 and tuple(four) == K.tiling() and lib.lsr_hessian_tiling(None) == -1
    vol = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    out = np.full(24, FILL, dtype=np.float32)
    v, o = vol.ctypes.data, out.ctypes.data
    d = ctypes.c_double
    ok = (d(1.0), d(1.0), d(1.0), d(2.25), 4, 0, 0, None)

    def args(**change):
        a = dict(zip(("sz", "sy", "sx", "scale", "measure", "dark", "accumulate", "stream"), ok))
        a.update(change)
        return tuple(a.values())

    for name in ("lsr_hessian_response_f32_cpu", "lsr_hessian_response_f32"):      # (checked before anything is launched)
        fn = getattr(lib, name)
        assert fn(None, o, 2, 3, 4, *ok) == -1 and fn(v, None, 2, 3, 4, *ok) == -1
        assert fn(v, v, 2, 3, 4, *ok) == -4 and b"alias" in lib.lsr_last_error()
        assert fn(v, o, 0, 3, 4, *ok) == -2 and fn(v, o, 2, -3, 4, *ok) == -2 and fn(v, o, 2, 3, 0, *ok) == -2
        assert fn(v, o, 2 ** 30, 3, 4, *ok) == -3
        assert fn(v, o, 2048, 1024, 1024, *ok) == -3 and b"2^31 - 1" in lib.lsr_last_error()
        for key in ("sz", "sy", "sx"):
            for bad in (0.0, -1.0, float("inf"), float("nan")):
                assert fn(v, o, 2, 3, 4, *args(**{key: d(bad)})) == -4 and b"sampling" in lib.lsr_last_error()
        for bad in (float("inf"), float("-inf"), float("nan")):
            assert fn(v, o, 2, 3, 4, *args(scale=d(bad))) == -4 and b"scale" in lib.lsr_last_error()
        for key, values in (("measure", (-1, 8)), ("dark", (-1, 2)), ("accumulate", (-1, 2))):
            for bad in values:
                assert fn(v, o, 2, 3, 4, *args(**{key: bad})) == -4 and key.encode() in lib.lsr_last_error()
        assert np.all(out == FILL), "a refused call wrote"
    assert lib.lsr_hessian_response_f32_cpu(v, o, 2, 3, 4, *args(scale=d(-1.0), measure=7, dark=1, accumulate=1)) == 0


# ---- the Python layer -------------------------------------------------------------------------------------------------------------


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))            # (a copy: the shared cases are read-only)


def check_python_layer(device):
    """Shared with tests/test_hessian_gpu.py: ``shrimpy_amd.hessian`` on ``device``."""
    shape = (C.TZ + 1, C.TY + 1, C.TX + 1)
    vol = _t(C.volume(shape, "beads")).to(device)
    sampling = (2.0, 0.5, 0.5)
    sigmas = (0.75, 1.0, 1.5)
    singles = [K.hessian_response(vol, s, "tube", sampling) for s in sigmas]
    for t in singles:
        assert t.device == vol.device and t.dtype == torch.float32 and t.is_contiguous() and t.shape == vol.shape
    want = singles[0].cpu().numpy()
    for t in singles[1:]:
        want = R.accumulate(want, t.cpu().numpy())
    got = K.enhance(vol, "tube", sigmas, sampling)
    assert got.cpu().numpy().tobytes() == want.tobytes(), "enhance is the maximum of the single calls"
    assert float(got.max()) > 0 and got.data_ptr() != vol.data_ptr()
    # with `out` it accumulates, in place
    out = singles[0].clone()
    assert K.hessian_response(vol, sigmas[1], "tube", sampling, out=out) is out
    assert out.cpu().numpy().tobytes() == R.accumulate(singles[0].cpu().numpy(), singles[1].cpu().numpy()).tobytes()
    # the eigenvalues are those of the entry on the package's own blur, scale sigma^2, and the measure their function
    e = [t.cpu().numpy() for t in K.hessian_eigenvalues(vol, 1.5, sampling)]
    g = K._blur(vol, 1.5, sampling, K._buffers(vol)).cpu().numpy()
    for k in range(3):
        assert e[k].tobytes() == twin_response(g, sampling, 2.25, k)[0].tobytes()
    assert singles[2].cpu().numpy().tobytes() == R.response(*e, 4).tobytes()
    bright, dark = K.hessian_eigenvalues(vol, 1.5, sampling), K.hessian_eigenvalues(-vol, 1.5, sampling, dark=True)
    assert all(torch.equal(a, b) for a, b in zip(bright, dark)), "dark is the negated volume"
    with pytest.raises(ValueError, match="measure must be one of"):
        K.hessian_response(vol, 1.0, "frangi")
    with pytest.raises(ValueError, match="cap is 64"):
        K.hessian_response(vol, 16.2, "tube")
    with pytest.raises(ValueError, match="cap is 64"):
        K.enhance(vol, "tube", (1.0, 2.0), (1.0, 1.0, 0.1))
    assert K.blur_radii(16.1) == (64, 64, 64) and K.blur_radii(1.5, (2.0, 0.5, 0.5)) == (3, 12, 12)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma must be positive"):
            K.hessian_response(vol, bad, "tube")
    with pytest.raises(ValueError, match="sigmas is empty"):
        K.enhance(vol, "tube", ())
    with pytest.raises(ValueError, match="sampling"):
        K.hessian_response(vol, 1.0, "tube", (1.0, 0.0, 1.0))
    with pytest.raises(TypeError):
        K.hessian_response(vol.double(), 1.0, "tube")
    with pytest.raises(ValueError, match="does not match"):
        K.hessian_response(vol, 1.0, "tube", out=torch.empty((2, 2, 2), dtype=torch.float32, device=device))
    with pytest.raises(ValueError, match="out must not be vol"):
        K.hessian_response(vol, 1.0, "tube", out=vol)
    if torch.device(device).type != "cpu":
        with pytest.raises(ValueError, match="does not match"):
            K.hessian_response(vol, 1.0, "tube", out=torch.empty(shape, dtype=torch.float32))


def test_python_layer_on_the_host():
    check_python_layer(torch.device("cpu"))


def check_structures(device):
    """Shared with tests/test_hessian_gpu.py: a tube, a plate and a ball at sigma 1.5 (expected, computed with scipy's
    reflect blur: sheet 0 / 37.5 / 0, blob 0 / 0 / 25.8, tube 28.2 / 0.5 / 25.8 at the tube's, plate's and ball's centre)."""
    vol = _t(C.structures()).to(device)
    got = {m: K.hessian_response(vol, 1.5, m).cpu().numpy() for m in ("ridge", "tube", "sheet", "blob")}
    at = {m: {name: float(got[m][site]) for name, site in (("tube", C.TUBE_CENTRE), ("plate", C.PLATE_CENTRE),
                                                             ("ball", C.BALL_CENTRE), ("background", C.BACKGROUND))} for m in got}
    print(at)
    assert at["sheet"]["plate"] > 30 and max(at["sheet"]["tube"], at["sheet"]["ball"]) < 0.01 * at["sheet"]["plate"]
    assert at["blob"]["ball"] > 20 and max(at["blob"]["tube"], at["blob"]["plate"]) < 0.01 * at["blob"]["ball"]
    assert at["tube"]["tube"] > 20 and at["tube"]["plate"] < 0.05 * at["tube"]["tube"]
    assert all(at[m]["background"] == 0.0 for m in got)
    assert abs(at["sheet"]["plate"] - 37.5) < 0.5 and abs(at["blob"]["ball"] - 25.8) < 0.5 and abs(at["tube"]["tube"] - 28.2) < 0.5


def test_structures_on_the_host():
    check_structures(torch.device("cpu"))


# ---- settings and segment_zyx -------------------------------------------------------------------------------------------------


def test_settings():
    s = SegmentSettings(channel_name="GFP", threshold=1.0)
    assert s.enhance is None and "enhance" in SegmentSettings.__doc__
    e = SegmentSettings(channel_name="GFP", threshold=5.0, enhance=dict(measure="tube", sigmas=[2])).enhance
    assert isinstance(e, EnhanceSettings) and e.sigmas == [2.0] and e.sigmas_um is None and e.dark is False and e.channels == []
    assert e.scales((0.4, 0.1, 0.1)) == ([2.0], (1.0, 1.0, 1.0))
    um = EnhanceSettings(channels=["GFP"], measure="log", sigmas_um=[0.5, 1.0], dark=True)
    assert um.scales((0.4, 0.1, 0.1)) == ([0.5, 1.0], (0.4, 0.1, 0.1))
    for name in K.MEASURES:
        assert EnhanceSettings(measure=name, sigmas=[1]).measure == name
    ok = dict(measure="tube", sigmas=[1.0, 2.0])
    for bad in (dict(measure="frangi"), dict(sigmas=[]), dict(sigmas=[0.0]), dict(sigmas=[-1.0]), dict(sigmas=[float("inf")]),
                dict(sigmas=None), dict(sigmas_um=[1.0]), dict(sigmas=None, sigmas_um=[]), dict(dark="very"), dict(radius=1.0)):
        with pytest.raises(ValueError):
            EnhanceSettings(**{**ok, **bad})


TUBES = dict(channel_name="GFP")


def check_segment_zyx(device):
    """Shared with tests/test_hessian_gpu.py: ``enhance`` of ``segment_zyx`` on ``device``."""
    vol, tubes = C.tubes_on_a_ramp()
    d_vol = _t(vol).to(device)
    # no threshold of the intensity separates the tubes from the ramp
    assert S.segment_zyx(d_vol, SegmentSettings(**TUBES, threshold=30.0))[2] == ndi.label(vol > 30.0)[1] == 3
    assert S.segment_zyx(d_vol, SegmentSettings(**TUBES, threshold=200.0))[2] == ndi.label(vol > 200.0)[1] == 1
    settings = SegmentSettings(**TUBES, threshold=5.0, enhance=dict(measure="tube", sigmas=[2]))
    labels, table, n = S.segment_zyx(d_vol, settings)
    labels = labels.cpu().numpy()
    assert n == 2 and labels.dtype == np.int32
    assert np.all(labels[tubes] > 0), "every voxel of each tube is labelled"
    assert not np.any(labels[~ndi.binary_dilation(tubes, iterations=3)]), "nothing beyond 3 voxels of the tubes"
    assert len(set(labels[tubes & (np.arange(vol.shape[1])[None, :, None] < 15)].tolist())) == 1
    response = K.enhance(d_vol, "tube", [2.0]).cpu().numpy()
    want, m = ndi.label(response > 5.0)
    assert m == 2 and np.array_equal(labels, want)
    assert float(table["intensity_max"].max()) > 300.0, "the table's intensities are the input's"
    # sigmas_um at the sampling: the same response on a grid of half the spacing
    half = SegmentSettings(**TUBES, threshold=5.0, enhance=dict(measure="tube", sigmas_um=[1.0]))
    labels_um, _, n_um = S.segment_zyx(d_vol, half, sampling=(0.5, 0.5, 0.5))
    assert n_um == 2 and np.array_equal(labels_um.cpu().numpy(), labels)
    # unset, spelled out or never mentioned: the labels and the table of an existing scene
    blobs = LH.blob_volume(5)
    want0, m0, _ = LH.reference_segmentation(blobs, LH.SETTINGS)
    a = S.segment_zyx(_t(blobs).to(device), SegmentSettings(**LH.SETTINGS))
    b = S.segment_zyx(_t(blobs).to(device), SegmentSettings(**LH.SETTINGS, enhance=None))
    for labels0, table0, n0 in (a, b):
        assert n0 == m0 and np.array_equal(labels0.cpu().numpy(), want0)
        assert sorted(table0) == sorted(a[1]) and all(np.array_equal(table0[k], a[1][k], equal_nan=True) for k in table0)


def test_segment_zyx_enhance_on_the_host():
    check_segment_zyx(torch.device("cpu"))
