"""Accelerated Richardson-Lucy (Biggs & Andrews 1997) on the device: the two kernels of ``csrc/rl_accel.hip`` per voxel
and per sum, bit for bit against their host twins, the wiring of ``acceleration="biggs-andrews"`` through every plan
kind, the run against the float64 restatement ``tests/rl_accel_ref.py`` and that it accelerates.  Bounds and shared
checks: ``tests/test_rl_accel_host.py`` (its docstring derives them).
"""
import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd.deconvolve import PaddedVolume, make_plan, padded_shape, richardson_lucy
from shrimpy_amd.deconvolve_fft import FftRichardsonLucyPlan
from tests import rl_accel_ref as r
from tests import rl_fp64_cases as c
from tests import test_rl_accel_host as h
from tests import test_rl_tv_gpu as tvg

pytestmark = pytest.mark.gpu

# case -> worst C (units of 2^-24 of the float64 reference) of a 10-iteration accelerated run on an MI355X; pinned at
# four times that
MEASURED = {"ramp, separable": 76.08, "ramp, rotated": 79.85, "beads, separable": 67.31, "beads, rotated": 83.12}


def _dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), device=device)


def test_dots_kernel_per_voxel_per_sum_and_reproducible(device):
    h.dots_hold(device)


def test_dots_kernel_on_many_rows_per_workgroup_and_padded_working_volumes(device):
    """More rows than workgroups (2048), so every workgroup strides; x1 and p real padded working volumes, g dense with
    rows that start on 8-byte boundaries only (X = 70): the halo is not read, the sums hold, two runs agree bit for bit."""
    shape = (40, 130, 70)
    x1, p, g_prev = h._inputs(shape, 5)
    g_ref = np.float32(x1) - np.float32(p)
    gd, hd = g_ref.astype(np.float64), g_prev.astype(np.float64)
    want = np.array([(gd * hd).sum(), (gd * gd).sum()])
    slack = g_ref.size * 2.0 ** -53 * np.array([np.abs(gd * hd).sum(), (gd * gd).sum()])
    xp, pp = PaddedVolume(shape, (9, 7, 7), device), PaddedVolume(shape, (9, 7, 7), device)
    for v in (xp, pp):
        v.full.fill_(float("nan"))
    xp.view.copy_(_dev(x1, device))
    pp.view.copy_(_dev(p, device))
    seen = []
    for _ in range(2):
        g = _dev(g_prev.copy(), device)
        dots = torch.zeros(2, dtype=torch.float64, device=device)
        r.dots_call(xp.view, pp.view, g, False, dots)
        assert np.array_equal(g.cpu().numpy().view(np.uint32), g_ref.view(np.uint32))
        got = dots.cpu().numpy()
        assert np.all(np.abs(got - want) <= slack), (got, want, slack)
        seen.append(got.view(np.uint64).copy())
    assert np.array_equal(seen[0], seen[1])
    # the prediction between the same padded volumes: only the logical window of x0 changes
    pp.full.nan_to_num_(nan=0.0)
    xp.full.nan_to_num_(nan=0.0)
    num, den = (torch.tensor([v], dtype=torch.float64, device=device) for v in (0.6, 1.0))
    r.predict_call(xp.view, pp.view, num, den)
    twin = r.predict_call(torch.as_tensor(x1), torch.as_tensor(p.copy()), num.cpu(), den.cpu())
    assert torch.equal(pp.view.cpu(), twin)
    rim = pp.full.clone()
    _, _, oy, ox = padded_shape(shape, (9, 7, 7))
    rim[:, oy:oy + shape[1], ox:ox + shape[2]] = 0
    assert not rim.any(), "the halo of the padded volume was written"


def test_predict_kernel_and_twin_agree_bit_for_bit(device):
    _lib.call("lsr_set_host_threads", 4)
    got, twin = h.predict_hold(device), h.predict_hold(h.CPU)
    assert len(got) == len(twin) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, twin))


def test_g_of_kernel_and_twin_agree_bit_for_bit(device):
    for shape in r.SHAPES:
        x1, p, g_prev = h._inputs(shape, 7)
        outs = []
        for dev in (device, h.CPU):
            g = _dev(g_prev.copy(), dev)
            dots = torch.zeros(2, dtype=torch.float64, device=dev)
            r.dots_call(_dev(x1, dev), _dev(p, dev), g, False, dots)
            outs.append((g.cpu(), dots.cpu().numpy()))
        assert torch.equal(outs[0][0], outs[1][0])
        np.testing.assert_allclose(outs[0][1], outs[1][1], rtol=1e-12)


# ---------------------------------------------------------------- the wiring, plan kind by plan kind

@pytest.mark.parametrize("kind", tvg.KINDS)
def test_every_plan_kind_equals_chaining_plain_iterations_and_the_two_launches(device, kind):
    """Which buffer holds p_k, x_k and x_{k+1}, the first iteration from y (dense, padded) or from x0, the dense last
    write: independent of the arithmetic, bit for bit."""
    shape = (37, 35, 133)
    plan = tvg.make_kind(kind, shape, device)
    y, x0 = tvg._volumes(shape, device)
    acc = dict(acceleration="biggs-andrews")

    def one(p):
        return plan(y, iterations=1, x0=p)

    want, alphas = h.chain(one, y, None, 4)
    out = torch.full(shape, float("nan"), device=device)
    got = plan(y, iterations=4, out=out, **acc)
    assert got is out and torch.equal(got, want), f"{kind}: four accelerated iterations from y differ from the chain"
    np.testing.assert_array_equal(plan.last_alphas, alphas)
    assert plan.last_alphas.dtype == np.float64 and plan.last_alphas.shape == (3,) and plan.last_alphas[0] == 0
    assert torch.equal(plan(y, iterations=4, stats=True, **acc), want), f"{kind}: stats on"
    want3, _ = h.chain(one, y, None, 3)
    assert torch.equal(plan(y, iterations=3, **acc), want3), f"{kind}: three iterations"
    from_x0, _ = h.chain(one, y, x0, 4)
    assert torch.equal(plan(y, iterations=4, x0=x0, **acc), from_x0), f"{kind}: from x0"
    if getattr(plan, "padded_input", False):
        y_pad = plan.new_padded_input()
        y_pad.view.copy_(y)
        assert torch.equal(plan(y_pad, iterations=4, **acc), want), f"{kind}: from a padded y"
        assert torch.equal(y_pad.view, y), "the padded y was written"
    buf = x0.clone()
    assert torch.equal(plan(y, iterations=4, x0=buf, out=buf, **acc), from_x0), f"{kind}: out is x0"
    assert torch.equal(plan(y, iterations=1, **acc), plan(y, iterations=1))
    # and the plain run is undisturbed by the accelerated ones before it
    assert torch.equal(plan(y, iterations=3), plan(y, iterations=3, acceleration="none"))


@pytest.mark.parametrize("kind", tvg.KINDS)
def test_acceleration_none_is_the_plain_run_launch_for_launch(device, kind, monkeypatch):
    shape = (12, 35, 133)
    plan = tvg.make_kind(kind, shape, device)
    y, _ = tvg._volumes(shape, device, 1)
    plain = plan(y, iterations=3).clone()
    plan(y, iterations=3, stats=True)
    plain_stats = plan.last_stats
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    plan(y, iterations=3)
    sequence = list(called)
    called.clear()
    assert torch.equal(plan(y, iterations=3, acceleration="none"), plain)
    assert called == sequence and not any("accel" in n for n in called) and plan.last_alphas is None
    assert torch.equal(plan(y, iterations=3, acceleration="none", stats=True), plain)
    np.testing.assert_allclose(plan.last_stats.change, plain_stats.change, rtol=1e-12)
    called.clear()
    plan(y, iterations=3, acceleration="biggs-andrews")
    assert called.count("lsr_rl_accel_dots_f32") == 2 and called.count("lsr_rl_accel_predict_f32") == 2


@pytest.mark.parametrize("kind", ["fused", "separable", "generic", "fft"])
def test_stats_and_tol(device, kind):
    """``change[k] = sum |x_{k+1} - p_k|`` as the RL launch sums it, ``total[k] = sum x_{k+1}``; ``tol`` stops one iteration
    after the first that met it and returns that iteration's estimate."""
    shape = (20, 35, 133)
    plan = tvg.make_kind(kind, shape, device)
    y, _ = tvg._volumes(shape, device, 3)
    acc = dict(acceleration="biggs-andrews")
    plan(y, iterations=12, stats=True, **acc)
    full = plan.last_stats
    assert full.iterations == 12 and tuple(plan.stats_device.shape) == (12, 3)
    for k in (1, 4):
        xk = plan(y, iterations=k + 1, **acc)
        np.testing.assert_allclose(full.total[k], float(xk.double().sum()), rtol=tvg.RTOL)
    tol = float(np.sqrt(full.rel_change[4] * full.rel_change[5]))
    first = int(np.argmax(full.rel_change < tol))
    assert 0 < first < 10
    got = plan(y, iterations=12, tol=tol, **acc).clone()
    s = plan.last_stats
    assert s.stopped_by_tol and s.iterations == first + 2 and len(plan.last_alphas) == first + 1
    assert torch.equal(got, plan(y, iterations=first + 2, **acc))
    np.testing.assert_allclose(s.change, full.change[:first + 2], rtol=1e-12)


def test_richardson_lucy_and_make_plan_take_the_keyword(device):
    shape = (12, 35, 133)
    y, _ = tvg._volumes(shape, device, 2)
    ks = tvg._sep((9, 7, 7), 1)
    plan = make_plan(shape, None, device, psf_factors=ks)
    want = plan(y, iterations=5, acceleration="biggs-andrews").clone()
    got, stats = richardson_lucy(y, psf_factors=ks, iterations=5, acceleration="biggs-andrews", return_stats=True)
    assert torch.equal(got, want) and not torch.equal(got, richardson_lucy(y, psf_factors=ks, iterations=5))
    np.testing.assert_array_equal(stats.alphas, plan.last_alphas)
    assert torch.equal(richardson_lucy(y, psf_factors=ks, iterations=5, acceleration="none"),
                       richardson_lucy(y, psf_factors=ks, iterations=5))
    plan.release()
    assert not plan._path._sides      # g_k, the third padded volume, the dense copies: all dropped


# ---------------------------------------------------------------- against float64, and that it accelerates

def test_ten_accelerated_iterations_against_float64_voxel_by_voxel(device):
    """Worst per case on an MI355X: see ``MEASURED``."""

    def run(y, kw):
        plan = make_plan(y.shape, kw.get("psf"), device, psf_factors=kw.get("psf_factors"))
        x = plan(_dev(y, device), iterations=10, acceleration="biggs-andrews")
        print("path:", plan.path)
        return x.cpu().numpy(), plan.last_alphas

    print("worst per case:", h.hold_float64_pin(run, MEASURED))


def test_it_accelerates(device):
    h.accelerates(device)


def test_errors(device):
    shape = (4, 6, 9)
    y, _ = tvg._volumes(shape, device, 5)
    plan = tvg.make_kind("fused", shape, device)
    fft = FftRichardsonLucyPlan(shape, c.taps_nd((3, 3, 3), np.random.default_rng(0)), device)
    for p in (plan, fft):
        with pytest.raises(ValueError, match="acceleration"):
            p(y, iterations=2, acceleration="nesterov")
        with pytest.raises(ValueError, match="tv_lambda"):
            p(y, iterations=2, acceleration="biggs-andrews", tv_lambda=0.01)
        assert torch.equal(p(y, iterations=0, acceleration="biggs-andrews"), y) and len(p.last_alphas) == 0
    with pytest.raises(ValueError, match="acceleration"):
        richardson_lucy(y, psf_factors=tvg._sep((3, 3, 3), 0), iterations=1, acceleration="fast")
    lib = _lib.load()
    a, b, g = y.clone(), y.clone(), torch.zeros_like(y)
    dots = torch.zeros(2, dtype=torch.float64, device=device)
    work = torch.zeros(2 * 24, dtype=torch.float64, device=device)
    assert lib.lsr_rl_accel_workspace_bytes(4, 6, 9) == 24 * 16

    def dots_status(aa, bb, gg, ws=work):
        with torch.cuda.device(device):
            return lib.lsr_rl_accel_dots_f32(aa.data_ptr(), 9, 54, bb.data_ptr(), 9, 54, gg.data_ptr(), 4, 6, 9, 0,
                                             dots.data_ptr(), None if ws is None else ws.data_ptr(), _lib.stream_ptr(device))

    assert dots_status(a, b, g) == 0
    assert dots_status(a, b, a) < 0 and "g overlaps" in lib.lsr_last_error().decode()
    assert dots_status(a, b, g, ws=None) < 0

    def predict_status(aa, bb, num, den):
        with torch.cuda.device(device):
            return lib.lsr_rl_accel_predict_f32(aa.data_ptr(), 9, 54, bb.data_ptr(), 9, 54, 4, 6, 9, num, den, None,
                                                _lib.stream_ptr(device))

    assert predict_status(a, b, None, None) == 0
    assert predict_status(a, a, None, None) < 0 and "x0 overlaps x1" in lib.lsr_last_error().decode()
    assert predict_status(a, b, None, dots.data_ptr()) < 0
    torch.cuda.synchronize()

