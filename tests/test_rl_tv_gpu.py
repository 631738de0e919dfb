"""RL-TV on the device: the total-variation kernel ``csrc/rl_tv.hip`` against the float64 restatement
``tests/rl_tv_ref.py`` voxel by voxel, its exact properties, and the wiring of ``tv_lambda`` through every plan kind.

The bound is that of ``tests/test_rl_tv_host.py`` (its docstring derives ``C <= 4 + 80 lambda / (1 - 6 lambda)`` for
the operation order kernel and twin share); the kernel uses correctly rounded float32 square roots and divisions and no
contraction, as the twin does, so the two agree bit for bit and the measured ``C`` are the twin's.  Shapes
(``rl_tv_ref.SHAPES``) are taken from the kernel's 16 x 64 tile: smaller than a tile, ragged in rows and columns, each
axis degenerate alone, and 5 x 3 tiles with 19 planes; ``make_inputs`` puts its 1e4 spikes on the tile's corners.
"""
import ctypes

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd.deconvolve import RichardsonLucyPlan, factor_psf_y, prepare_psf, richardson_lucy
from shrimpy_amd.deconvolve_fft import FftRichardsonLucyPlan
from tests import rl_fp64_cases as c
from tests import rl_tv_ref as r
from tests import test_rl_tv_host as h

pytestmark = pytest.mark.gpu

# lambda -> worst C measured for the kernel on an MI355X over this file's cases; pinned at min(4 x worst, ceiling)
MEASURED = {0.002: 1.993, 0.02: 1.996, 0.1: 2.952, 0.16: 5.693}
RTOL = 1e-5          # the relative tolerance tests/test_rl_stats_gpu.py holds the plain rows to


def _dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), device=device)


def test_the_pinned_bounds_lie_below_the_a_priori_ceiling():
    for lam in r.LAMBDAS:
        assert MEASURED[lam] < h.bound(lam, MEASURED) <= r.ceiling(lam)


def test_kernel_against_float64_voxel_by_voxel(device):
    seen = {}
    h.hold_pin(device, MEASURED, seen)
    print("worst per lambda:", seen)


def test_kernel_on_z_chunks_and_padded_working_volumes(device):
    """A column tall enough to be cut into z chunks (few tiles, 70 planes: each chunk restarts one plane early for its
    p_z), between real padded working volumes with ``out`` aliasing ``v``: the zero halo is not read."""
    from shrimpy_amd.deconvolve import PaddedVolume, padded_shape

    shape = (70, 21, 71)
    u, v = c.make_inputs(shape, (3, 3, 3), 7, tile=r.TILE)
    for lam in r.LAMBDAS:
        up, vp = PaddedVolume(shape, (9, 7, 7), device), PaddedVolume(shape, (9, 7, 7), device)
        up.view.copy_(_dev(u, device))
        vp.view.copy_(_dev(v, device))
        r.tv_call(up.view, vp.view, vp.view, lam)
        ref = r.tv_scale(u, v, np.float32(lam), np.float32(1e-6))
        worst, idx, leak = c.worst_voxel(vp.view.cpu().numpy(), ref)
        print(f"padded, z chunks, lambda {lam}: {worst:.3f} u at {idx}")
        assert leak is None and worst <= h.bound(lam, MEASURED), (lam, worst, idx, leak)
        dense = r.tv_call(_dev(u, device), _dev(v, device), torch.empty(shape, device=device), lam)
        assert torch.equal(dense, vp.view)
        rim = vp.full.clone()
        _, _, oy, ox = padded_shape(shape, (9, 7, 7))
        rim[:, oy:oy + shape[1], ox:ox + shape[2]] = 0
        assert not rim.any(), "the halo of the padded volume was written"


def test_kernel_and_twin_agree_bit_for_bit(device):
    _lib.call("lsr_set_host_threads", 4)
    for shape in r.SHAPES + [(40, 21, 71)]:
        u, v = c.make_inputs(shape, (3, 3, 3), 11, tile=r.TILE)
        for lam in (0.02, 0.16):
            got = r.tv_call(_dev(u, device), _dev(v, device), torch.empty(shape, device=device), lam)
            twin = r.tv_call(torch.as_tensor(u), torch.as_tensor(v), torch.empty(shape), lam)
            assert torch.equal(got.cpu(), twin), (shape, lam)


def test_kernel_exact_properties(device):
    h.exact_properties(device)


def test_it_regularises(device):
    h.regularises(device)


# ---------------------------------------------------------------- the wiring, plan kind by plan kind


def _ysep_psf(ps, seed):
    rng = np.random.default_rng(seed)
    pz, py, px = ps
    return (c.taps_1d(py, rng)[None, :, None].astype(np.float64) * c.taps_nd((pz, px), rng)[:, None, :]).astype(np.float32)


def _sep(ps, seed):
    rng = np.random.default_rng(seed)
    return [c.taps_1d(n, rng) for n in ps]


def make_kind(kind, shape, device):
    if kind == "fused":
        plan = RichardsonLucyPlan(shape, None, device, psf_factors=_sep((9, 7, 7), 1), fused="always")
    elif kind == "separable":
        plan = RichardsonLucyPlan(shape, None, device, psf_factors=_sep((9, 7, 7), 1), fused="never")
    elif kind == "long z":
        plan = RichardsonLucyPlan(shape, None, device, psf_factors=_sep((17, 5, 3), 2))
    elif kind == "y-separable (fused)":
        plan = RichardsonLucyPlan(shape, _ysep_psf((5, 5, 3), 3), device)
    elif kind == "y-separable":
        plan = RichardsonLucyPlan(shape, _ysep_psf((5, 5, 3), 3), device, fused="never")
    elif kind == "dense":
        plan = RichardsonLucyPlan(shape, c.taps_nd((5, 7, 5), np.random.default_rng(4)), device, separable="never")
    elif kind == "generic":
        plan = RichardsonLucyPlan(shape, c.taps_nd((13, 11, 5), np.random.default_rng(5)), device, separable="never")
    else:
        return FftRichardsonLucyPlan(shape, c.taps_nd((7, 9, 5), np.random.default_rng(6)), device)
    want = {"long z": "separable (long z, 4 launches)"}.get(kind, kind)
    assert plan.path == want, (kind, plan.path)
    return plan


KINDS = ["fused", "y-separable (fused)", "separable", "dense", "y-separable", "long z", "generic", "fft"]


def _volumes(shape, device, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.poisson(rng.uniform(20.0, 200.0, shape)).astype(np.float32) + 1.0
    x0 = rng.uniform(10.0, 150.0, shape).astype(np.float32)
    return _dev(y, device), _dev(x0, device)


def _chain(plan, y, x0, n, lam, tv_eps=1e-6):
    """``n`` times: one plain iteration of ``plan`` from x_k, then one ``lsr_rl_tv_scale_f32`` call.  Returns every iterate
    and the plain call's stats per step."""
    xs, plain = [y if x0 is None else x0], []
    for k in range(n):
        v = plan(y, iterations=1, x0=None if (k == 0 and x0 is None) else xs[-1], stats=True).clone()
        plain.append(plan.last_stats)
        xs.append(r.tv_call(xs[-1], v, torch.empty_like(v), lam, tv_eps))
    return xs, plain


@pytest.mark.parametrize("kind", KINDS)
def test_every_plan_kind_equals_chaining_plain_iterations_and_the_tv_launch(device, kind):
    """Which buffer is x_k, the first iteration from y (dense, padded) or from x0, the dense last write: independent of
    the arithmetic, bit for bit."""
    shape = (37, 35, 133)
    plan = make_kind(kind, shape, device)
    y, x0 = _volumes(shape, device)
    lam = 0.01
    from_y, _ = _chain(plan, y, None, 3, lam)
    out = torch.full(shape, float("nan"), device=device)
    got = plan(y, iterations=3, tv_lambda=lam, out=out)
    assert got is out and torch.equal(got, from_y[3]), f"{kind}: three RL-TV iterations from y differ from the chain"
    assert torch.equal(plan(y, iterations=2, tv_lambda=lam, stats=True), from_y[2]), f"{kind}: two iterations, stats on"
    from_x0, _ = _chain(plan, y, x0, 3, lam, 1e-4)
    assert torch.equal(plan(y, iterations=3, x0=x0, tv_lambda=lam, tv_eps=1e-4), from_x0[3]), f"{kind}: from x0"
    if getattr(plan, "padded_input", False):
        y_pad = plan.new_padded_input()
        y_pad.view.copy_(y)
        assert torch.equal(plan(y_pad, iterations=3, tv_lambda=lam), from_y[3]), f"{kind}: from a padded y"
        assert torch.equal(y_pad.view, y), "the padded y was written"
    # x0 that is also the output tensor: x_0 is copied aside
    buf = x0.clone()
    assert torch.equal(plan(y, iterations=3, x0=buf, out=buf, tv_lambda=lam, tv_eps=1e-4), from_x0[3]), f"{kind}: out is x0"


@pytest.mark.parametrize("kind", KINDS)
def test_tv_lambda_zero_is_the_plain_run_and_launches_no_tv_kernel(device, kind, monkeypatch):
    shape = (12, 35, 133)
    plan = make_kind(kind, shape, device)
    y, _ = _volumes(shape, device, 1)
    plain = plan(y, iterations=3).clone()
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    assert torch.equal(plan(y, iterations=3, tv_lambda=0.0), plain)
    assert called and "lsr_rl_tv_scale_f32" not in called
    launches = len(called)
    called.clear()
    plan(y, iterations=3)
    assert len(called) == launches, "tv_lambda=0.0 changed the launch sequence"
    called.clear()
    plan(y, iterations=3, tv_lambda=0.01)
    assert called.count("lsr_rl_tv_scale_f32") == 3


def test_richardson_lucy_tv_lambda_zero_is_bit_identical(device, monkeypatch):
    shape = (12, 35, 133)
    y, _ = _volumes(shape, device, 2)
    ks = _sep((9, 7, 7), 1)
    plain = richardson_lucy(y, psf_factors=ks, iterations=3)
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    assert torch.equal(richardson_lucy(y, psf_factors=ks, iterations=3, tv_lambda=0.0), plain)
    assert "lsr_rl_tv_scale_f32" not in called
    tv = richardson_lucy(y, psf_factors=ks, iterations=3, tv_lambda=0.01)
    assert called.count("lsr_rl_tv_scale_f32") == 3 and not torch.equal(tv, plain)


@pytest.mark.parametrize("kind", ["fused", "separable", "generic", "fft"])
def test_stats_describe_the_regularised_iterate(device, kind):
    """``change[k] = sum |x_{k+1} - x_k|`` and ``total[k] = sum x_{k+1}`` over the iterates the caller gets (float64 sums
    of the results of k and k + 1 iterations); ``flux[k]`` is what a plain iteration from x_k reports."""
    shape = (20, 35, 133)
    plan = make_kind(kind, shape, device)
    y, _ = _volumes(shape, device, 3)
    lam, n = 0.02, 4
    plan(y, iterations=n, tv_lambda=lam, stats=True)
    s = plan.last_stats
    assert s.iterations == n and tuple(plan.stats_device.shape) == (n, 3)
    xs, plain = _chain(plan, y, None, n, lam)
    for k in range(n):
        assert torch.equal(plan(y, iterations=k + 1, tv_lambda=lam), xs[k + 1])
        np.testing.assert_allclose(s.change[k], float((xs[k + 1].double() - xs[k].double()).abs().sum()), rtol=RTOL)
        np.testing.assert_allclose(s.total[k], float(xs[k + 1].double().sum()), rtol=RTOL)
        np.testing.assert_allclose(s.flux[k], plain[k].flux[0], rtol=RTOL)


@pytest.mark.parametrize("kind", ["fused", "separable", "generic", "fft"])
def test_tol_stops_one_iteration_after_the_first_that_met_it(device, kind):
    shape = (20, 35, 133)
    plan = make_kind(kind, shape, device)
    y, _ = _volumes(shape, device, 4)
    lam = 0.02
    plan(y, iterations=12, tv_lambda=lam, stats=True)
    full = plan.last_stats
    tol = float(np.sqrt(full.rel_change[4] * full.rel_change[5]))
    first = int(np.argmax(full.rel_change < tol))
    assert 0 < first < 10
    got = plan(y, iterations=12, tv_lambda=lam, tol=tol).clone()
    s = plan.last_stats
    assert s.stopped_by_tol and s.iterations == first + 2
    assert torch.equal(got, plan(y, iterations=first + 2, tv_lambda=lam))
    np.testing.assert_allclose(s.change, full.change[:first + 2], rtol=1e-12)


def test_errors(device):
    shape = (4, 6, 9)
    y, _ = _volumes(shape, device, 5)
    plan = make_kind("fused", shape, device)
    fft = FftRichardsonLucyPlan(shape, c.taps_nd((3, 3, 3), np.random.default_rng(0)), device)
    for bad in (-0.01, 1.0 / 6.0, 0.2, float("nan")):
        for p in (plan, fft):
            with pytest.raises(ValueError, match="tv_lambda"):
                p(y, iterations=1, tv_lambda=bad)
        with pytest.raises(ValueError, match="tv_lambda"):
            richardson_lucy(y, psf_factors=_sep((3, 3, 3), 0), iterations=1, tv_lambda=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="tv_eps"):
            plan(y, iterations=1, tv_lambda=0.01, tv_eps=bad)
    lib = _lib.load()
    u, v, out = y.clone(), y.clone(), torch.empty_like(y)

    def status(uu, vv, oo, lam, eps):
        with torch.cuda.device(device):
            return lib.lsr_rl_tv_scale_f32(uu.data_ptr(), 9, 54, vv.data_ptr(), 9, 54, oo.data_ptr(), 9, 54, 4, 6, 9,
                                           ctypes.c_float(lam), ctypes.c_float(eps), None, _lib.stream_ptr(device))

    assert status(u, v, out, 0.1, 1e-6) == 0
    for lam, eps in ((-0.1, 1e-6), (1.0 / 6.0, 1e-6), (float("nan"), 1e-6), (0.1, 0.0), (0.1, -1.0)):
        assert status(u, v, out, lam, eps) < 0, (lam, eps)
    assert status(u, v, u, 0.1, 1e-6) < 0
    assert "out overlaps u" in lib.lsr_last_error().decode()
    assert status(u, v, v, 0.1, 1e-6) == 0
    torch.cuda.synchronize()
