"""RL-TV on CPU tensors: the host twin of the total-variation launch (``lsr_rl_tv_scale_f32_cpu``) against the float64
restatement ``tests/rl_tv_ref.py``, its exact properties, the wiring of ``host.richardson_lucy(tv_lambda=)``, the
settings and the ``deconvolve`` command.

The per-voxel bound.  Inputs are float32 and non-negative; the reference is the same arithmetic in float64 on the same
arrays; ``ref == 0`` must give an exact 0, elsewhere ``|got - ref| <= C u ref`` with ``u = 2^-24``.  A priori, for the
twin's (= the kernel's) operation order, with one rounding of relative size ``u`` per operation:

    d_a = u(r + e_a) - u(r)                                   1 u on each difference
    s   = ((dz dz + dy dy) + dx dx) + eps2                    2 u from the d's, 1 per product, 3 sums: <= 6 u on s
    inv = 1 / sqrt(s)                                         3 u from s, 1 for the root, 1 for the reciprocal: 5 u
    p_a = d_a * inv                                           1 + 5 + 1 = 7 u, and |p_a| <= 1
    div = ((pz - pz') + (py - py')) + (px - px')              six p's of 7 u absolute each (42 u) and five sums of
                                                              partial results of magnitude <= 2, 2, 4, 2, 6 (16 u): < 80 u
    den = 1 - lambda * div                                    lambda * 80 u absolute, + 2 u for product and difference,
                                                              against den >= 1 - 6 lambda
    out = v / den                                             + 1 u

so ``C <= 4 + 80 lambda / (1 - 6 lambda)`` (``rl_tv_ref.ceiling``).  The pinned ``C`` per ``lambda`` is four times the worst
value measured over this file's cases (the convention of ``tests/test_rl_fp64_gpu.py``), capped by that ceiling -- at the
two small ``lambda`` the ceiling (4.16, 5.82) is the tighter of the two.
"""
import ctypes

import numpy as np
import pytest
import torch
import yaml

from oracle import cpu_ref as o
from shrimpy_amd import _lib, host
from shrimpy_amd.deconvolve import check_tv, richardson_lucy
from tests import rl_fp64_cases as c
from tests import rl_tv_ref as r

# lambda -> (worst C measured for the twin on this file's cases, x86-64 host), pinned at min(4 x worst, ceiling)
MEASURED = {0.002: 1.993, 0.02: 1.996, 0.1: 2.952, 0.16: 5.693}
CPU = torch.device("cpu")


def bound(lam, measured=MEASURED):
    return min(4.0 * measured[lam], r.ceiling(lam))


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a))


def pin_cases(device, seeds=(0, 1, 2, 3)):
    """``(label, u, v, lam, got)`` over every shape, seed and lambda: dense volumes, and -- on the even seeds --
    strided views inside NaN-filled allocations with ``out`` aliasing ``v``."""
    for shape in r.SHAPES:
        for seed in seeds:
            u, v = c.make_inputs(shape, (3, 3, 3), seed, tile=r.TILE)
            for lam in r.LAMBDAS:
                ud, vd = _t(u).to(device), _t(v).to(device)
                out = torch.full(shape, float("nan"), dtype=torch.float32, device=device)
                yield f"dense {shape} seed {seed} lambda {lam}", u, v, lam, r.tv_call(ud, vd, out, lam).cpu().numpy()
                if seed % 2 == 0:
                    _, uv = r.framed(u, device)
                    full, vv = r.framed(v, device)
                    r.tv_call(uv, vv, vv, lam)
                    rim = full.clone()
                    rim[:shape[0], 3:3 + shape[1], 5:5 + shape[2]] = float("nan")
                    assert torch.isnan(rim).all(), "written outside the logical volume"
                    yield f"strided in place {shape} seed {seed} lambda {lam}", u, v, lam, vv.cpu().numpy()


def hold_pin(device, measured, worst_seen):
    for label, u, v, lam, got in pin_cases(device):
        ref = r.tv_scale(u, v, np.float32(lam), np.float32(1e-6))
        worst, idx, leak = c.worst_voxel(got, ref)
        worst_seen[lam] = max(worst_seen.get(lam, 0.0), worst)
        print(f"{label}: {worst:.3f} u at {idx}")
        assert leak is None, f"{label}: non-zero where the float64 result is exactly 0, voxel {leak}"
        assert worst <= bound(lam, measured), f"{label}: {worst:.3g} u (bound {bound(lam, measured):.3g} u) at voxel {idx}"


def test_the_pinned_bounds_lie_below_the_a_priori_ceiling():
    for lam in r.LAMBDAS:
        assert MEASURED[lam] < bound(lam) <= r.ceiling(lam)


def test_twin_against_float64_voxel_by_voxel():
    _lib.call("lsr_set_host_threads", 4)
    seen = {}
    hold_pin(CPU, MEASURED, seen)
    print("worst per lambda:", seen)


def exact_properties(device):
    """Shared with the GPU file: constant u, constant outside a box, out aliasing v."""
    rng = np.random.default_rng(5)
    shape = (7, 37, 133)
    v = _t(rng.uniform(0.5, 50.0, shape).astype(np.float32)).to(device)
    flat = torch.full(shape, 3.25, dtype=torch.float32, device=device)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=device)
    assert torch.equal(r.tv_call(flat, v, out, 0.1), v), "a constant u must leave v bit for bit"
    box = (slice(2, 5), slice(15, 19), slice(62, 67))
    grown = (slice(1, 6), slice(14, 20), slice(61, 68))
    bumpy = flat.clone()
    bumpy[box] = _t(rng.uniform(1.0, 9.0, (3, 4, 5)).astype(np.float32)).to(device)
    out = r.tv_call(bumpy, v, torch.empty_like(v), 0.1)
    same = out == v
    assert not same[box].all(), "nothing changed inside the box"
    same[grown] = True
    assert same.all(), "changed outside the box grown by one voxel"
    u = _t(c.make_inputs(shape, (3, 3, 3), 9, tile=r.TILE)[0]).to(device)
    apart = r.tv_call(u, v, torch.empty_like(v), 0.16)
    alias = v.clone()
    r.tv_call(u, alias, alias, 0.16)
    assert torch.equal(apart, alias), "out aliasing v differs from the result into a separate volume"
    zero_v = r.tv_call(u, torch.zeros_like(v), torch.empty_like(v), 0.16)
    assert not zero_v.any()


def test_twin_exact_properties():
    _lib.call("lsr_set_host_threads", 3)
    exact_properties(CPU)


def test_twin_does_not_depend_on_the_thread_count():
    u, v = (_t(a) for a in c.make_inputs((9, 21, 71), (3, 3, 3), 1, tile=r.TILE))
    outs = []
    for n in (1, 5):
        _lib.call("lsr_set_host_threads", n)
        st = torch.zeros(2, dtype=torch.float64)
        outs.append((r.tv_call(u, v, torch.empty_like(v), 0.05, stats=st), st))
    assert torch.equal(outs[0][0], outs[1][0])
    np.testing.assert_allclose(outs[0][1].numpy(), outs[1][1].numpy(), rtol=1e-13)
    got = outs[0][0].double()
    np.testing.assert_allclose(outs[0][1].numpy(), [float((got - u.double()).abs().sum()), float(got.sum())], rtol=1e-12)


def _scene(shape=(10, 20, 33), seed=0):
    ks = [np.array([0.25, 0.5, 0.25], np.float32), np.array([0.1, 0.2, 0.4, 0.2, 0.1], np.float32),
          np.array([0.3, 0.4, 0.3], np.float32)]
    y = o.bead_scene(shape, seed, psf_factors=ks, density=2e-3)
    return _t(y), ks


PSFS = {"separable": dict(), "dense": dict(separable="never")}


@pytest.mark.parametrize("kind", list(PSFS))
def test_tv_lambda_zero_is_the_plain_run_bit_for_bit(kind):
    y, ks = _scene()
    psf = ks[0][:, None, None] * ks[1][None, :, None] * ks[2][None, None, :]
    plain = richardson_lucy(y, psf, iterations=4, **PSFS[kind])
    assert torch.equal(richardson_lucy(y, psf, iterations=4, tv_lambda=0.0, **PSFS[kind]), plain)
    assert torch.equal(host.richardson_lucy(y, psf, iterations=4, tv_lambda=0.0, tv_eps=1e-3, **PSFS[kind]), plain)


@pytest.mark.parametrize("kind", list(PSFS))
def test_host_route_equals_chaining_plain_iterations_and_the_twin(kind):
    y, ks = _scene()
    psf = ks[0][:, None, None] * ks[1][None, :, None] * ks[2][None, None, :]
    got, stats = richardson_lucy(y, psf, iterations=3, tv_lambda=0.01, return_stats=True, **PSFS[kind])
    x = y
    for k in range(3):
        v, plain = richardson_lucy(y, psf, iterations=1, x0=x, return_stats=True, **PSFS[kind])
        nxt = r.tv_call(x, v, torch.empty_like(v), 0.01)
        np.testing.assert_allclose(stats.flux[k], plain.flux[0], rtol=1e-12)
        np.testing.assert_allclose(stats.change[k], float((nxt.double() - x.double()).abs().sum()), rtol=1e-12)
        np.testing.assert_allclose(stats.total[k], float(nxt.double().sum()), rtol=1e-12)
        x = nxt
    assert torch.equal(got, x)
    assert stats.iterations == 3 and not stats.stopped_by_tol


@pytest.mark.parametrize("kind", list(PSFS))
def test_tol_stops_one_iteration_after_the_first_that_met_it(kind):
    y, ks = _scene()
    psf = ks[0][:, None, None] * ks[1][None, :, None] * ks[2][None, None, :]
    _, full = richardson_lucy(y, psf, iterations=12, tv_lambda=0.02, return_stats=True, **PSFS[kind])
    tol = float(np.sqrt(full.rel_change[4] * full.rel_change[5]))
    first = int(np.argmax(full.rel_change < tol))
    assert 0 < first < 10
    got, s = richardson_lucy(y, psf, iterations=12, tv_lambda=0.02, tol=tol, return_stats=True, **PSFS[kind])
    assert s.stopped_by_tol and s.iterations == first + 2
    assert torch.equal(got, richardson_lucy(y, psf, iterations=first + 2, tv_lambda=0.02, **PSFS[kind]))
    np.testing.assert_array_equal(s.change, full.change[:first + 2])


def regularises(device):
    """Shared with the GPU file: total variation of the result falls as tv_lambda rises."""
    shape = (24, 48, 64)
    from shrimpy_amd.pipeline import gaussian_psf_factors

    ks = gaussian_psf_factors((9, 7, 7), (2.0, 1.2, 1.2))
    y = _t(o.bead_scene(shape, 3, psf_factors=ks, density=1e-3)).to(device)
    tv = []
    for lam in (0.0, 0.01, 0.05):
        x = richardson_lucy(y, psf_factors=ks, iterations=20, tv_lambda=lam).cpu().numpy()
        assert np.isfinite(x).all() and (x >= 0).all()
        tv.append(r.total_variation(x))
    print("total variation at tv_lambda 0 / 0.01 / 0.05:", tv)
    assert tv[0] > tv[1] > tv[2]


def test_it_regularises():
    regularises(CPU)


def test_errors():
    y, ks = _scene((4, 6, 9))
    for bad in (-0.01, 1.0 / 6.0, 0.2, float("nan")):
        with pytest.raises(ValueError, match="tv_lambda"):
            richardson_lucy(y, psf_factors=ks, iterations=1, tv_lambda=bad)
        with pytest.raises(ValueError, match="tv_lambda"):
            host.richardson_lucy(y, psf_factors=ks, iterations=1, tv_lambda=bad)
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tv_eps"):
            richardson_lucy(y, psf_factors=ks, iterations=1, tv_lambda=0.01, tv_eps=bad)
    assert check_tv(0.16, 1e-6) == (0.16, 1e-6)
    # the C ABI itself: a negative status and a message
    u = torch.ones((3, 4, 5))
    v, out = u.clone(), torch.empty_like(u)
    lib = _lib.load()

    def status(uu, vv, oo, lam, eps):
        return lib.lsr_rl_tv_scale_f32_cpu(uu.data_ptr(), 5, 20, vv.data_ptr(), 5, 20, oo.data_ptr(), 5, 20, 3, 4, 5,
                                           ctypes.c_float(lam), ctypes.c_float(eps), None)

    assert status(u, v, out, 0.1, 1e-6) == 0
    for lam, eps in ((-0.1, 1e-6), (1.0 / 6.0, 1e-6), (float("nan"), 1e-6), (0.1, 0.0), (0.1, -1.0), (0.1, 1e-30)):
        assert status(u, v, out, lam, eps) < 0, (lam, eps)
    assert status(u, v, u, 0.1, 1e-6) < 0
    assert "out overlaps u" in lib.lsr_last_error().decode()
    assert status(u, v, v, 0.1, 1e-6) == 0
    from shrimpy_amd.slab import run_slabs_in_process

    with pytest.raises(ValueError, match="slab"):
        run_slabs_in_process([], iterations=1, tv_lambda=0.01)


def test_settings_round_trip_and_validation(tmp_path):
    from shrimpy_amd.settings import DeconvolveSettings

    s = DeconvolveSettings(iterations=3, tv_lambda=0.01, tv_eps=1e-5)
    path = tmp_path / "dec.yml"
    path.write_text(yaml.safe_dump(s.model_dump()))
    back = DeconvolveSettings.from_yaml(path)
    assert (back.tv_lambda, back.tv_eps) == (0.01, 1e-5) and back == s
    old = tmp_path / "old.yml"
    old.write_text(yaml.safe_dump(dict(iterations=3)))
    assert (DeconvolveSettings.from_yaml(old).tv_lambda, DeconvolveSettings.from_yaml(old).tv_eps) == (0.0, 1e-6)
    for bad in (dict(tv_lambda=0.2), dict(tv_lambda=-0.1), dict(tv_lambda=1.0 / 6.0), dict(tv_eps=0.0)):
        path.write_text(yaml.safe_dump(dict(iterations=3, **bad)))
        with pytest.raises(Exception, match="tv_lambda|tv_eps"):
            DeconvolveSettings.from_yaml(path)


def test_cli_deconvolve_with_tv_lambda(tmp_path, monkeypatch):
    """``deconvolve`` on a tiny store: ``tv_lambda: 0.01`` in the settings file gives ``richardson_lucy(..., tv_lambda=0.01)``
    of the same array, a file without the keys today's output."""
    from click.testing import CliRunner

    import shrimpy_amd.cli as cli
    from shrimpy_amd.io.omezarr import open_ome_zarr
    from shrimpy_amd.pipeline import gaussian_psf_factors

    monkeypatch.setattr(cli, "_distributed", lambda: (0, 1, torch.device("cpu"), False))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    shape = (8, 12, 20)
    ks = gaussian_psf_factors((5, 3, 3), (1.0, 0.8, 0.8))
    vol = o.bead_scene(shape, 1, psf_factors=ks, density=5e-3)
    src = tmp_path / "raw.zarr"
    with open_ome_zarr(src, layout="hcs", mode="w", channel_names=["GFP"], prefer_iohub=False) as plate:
        arr = plate.create_position("0", "0", "000").create_zeros("0", shape=(1, 1) + shape, dtype=np.float32)
        arr.write_volume(0, 0, vol)
    base = dict(iterations=4, gaussian_shape_zyx=[5, 3, 3], gaussian_sigma_zyx=[1.0, 0.8, 0.8])
    results = {}
    for name, extra in (("plain", {}), ("tv", dict(tv_lambda=0.01))):
        cfg = tmp_path / f"{name}.yml"
        cfg.write_text(yaml.safe_dump(dict(base, **extra)))
        res = CliRunner().invoke(cli.cli, ["deconvolve", "-i", str(src), "-c", str(cfg), "-o", str(tmp_path / f"{name}.zarr")])
        assert res.exit_code == 0, res.output
        with open_ome_zarr(tmp_path / f"{name}.zarr", prefer_iohub=False) as plate:
            results[name] = dict(plate.positions())["0/0/000"]["0"].read_volume(0, 0)
    y = _t(vol)
    np.testing.assert_array_equal(results["plain"], richardson_lucy(y, psf_factors=ks, iterations=4).numpy())
    np.testing.assert_array_equal(results["tv"], richardson_lucy(y, psf_factors=ks, iterations=4, tv_lambda=0.01).numpy())
    assert not np.array_equal(results["tv"], results["plain"])
