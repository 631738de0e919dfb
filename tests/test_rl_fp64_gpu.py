"""Every spatial Richardson-Lucy kernel against a float64 restatement of ONE iteration
(``oracle.cpu_ref.rl_iteration_f64``), voxel by voxel: ``rl_fused_sep.hip`` and ``rl_fused_ysep.hip`` at every
compiled instance, the two-launch separable and ``ky (x) kzx`` kernels, the z-march of long axial factors, the tuned and
the generic dense stencil.  Agreement between two kernels that share their tap preparation, border normalisation,
reciprocal and ``eps`` handling proves none of those; this file compares each with arithmetic that shares nothing.

Inputs (``tests/rl_fp64_cases.py``) are float32 and non-negative, so nothing cancels and each voxel is held to

    ref == 0  ->  got == 0 exactly            (x = 0 stays 0, nothing leaks across a mask)
    ref  > 0  ->  |got - ref| <= C u ref      u = 2^-24

with no term in the volume's maximum and no voxel left out; outputs are NaN-filled first, so an unwritten voxel
shows.  ``C`` is one constant per path family, at most four times the worst ratio observed on an MI355X over this
file (recorded beside it), and never above the a-priori ``2 T + 16`` of the instance (``T`` taps per correlation).
Volume shapes are derived from each instance's own tile; a failure names path, taps, shape, voxel, tile, z chunk and
the error in units of ``u``.

What the bound resolves: ``eps`` doubled in the ratio, one border norm entry or the prefix-table norm off by 10 ppm,
an outermost tap scaled by ``1 + 3e-6`` each fail a third or more of this file while the kernels still agree with
each other bit for bit.  Dropping the Newton step of the update's reciprocals does NOT show: ``v_rcp_f32`` is good to
one ulp, which is inside the 9 u the separable paths already spend.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cpu_ref as o
from shrimpy_amd import _lib
from shrimpy_amd.deconvolve import PaddedVolume, RichardsonLucyPlan, _axis_norm, factor_psf_y, padded_shape, prepare_psf
from tests import rl_fp64_cases as c

pytestmark = pytest.mark.gpu

EPS = c.EPS

# Bounds in units of u * ref per voxel, with the worst ratio observed on an MI355X over this whole file beside each
# (each constant at most four times it).  Every bound is also capped by the instance's own 2 T + 16, and the families
# whose T spans two orders of magnitude carry a second constant, a share of 2 T + 16 (``_bound``).
C_SEP = 32.0           # fused / separable (T = pz + py + px): worst 8.91 u; of 2 T + 16: worst 0.239
C_LONGZ = 32.0         # separable with 17 .. 31 z taps, four launches: worst 8.92 u; of 2 T + 16: worst 0.113
C_YSEP = 60.0          # ky (x) kzx, all three forms (T = pz px + py): worst 15.7 u ...
F_YSEP = 0.58          # ... and of 2 T + 16: worst 0.147
C_DENSE = 160.0        # tuned and generic dense (T = pz py px): worst 42.1 u ...
F_DENSE = 0.62         # ... and of 2 T + 16: worst 0.160

# the worst ratio seen per family in this process (read back when the constants above are re-measured)
WORST: dict = {}

ODD = (3, 5, 7, 9, 11, 13, 15)
FUSED = [(pz, pyx) for pz in ODD for pyx in ODD if not (pz == 15 and pyx >= 11)]
YSEP = [(pz, pyx) for pz in ODD[:5] for pyx in ODD[:4]]
DENSE = [(pz, pyx) for pz in ODD[:5] for pyx in ODD[:4]]


def fused_tile_rows(pz, pyx):
    """``8 * fused_run(PZ, PYX)`` of ``csrc/correlate_common.hpp``."""
    if pz >= 11 and pyx >= 11:
        return 16
    by_z = 4 if pz <= 9 else (3 if pz <= 11 else 2)
    by_yx = 4 if pyx <= 9 else (3 if pyx <= 11 else 2)
    return 8 * min(by_z, by_yx)


def ysep_tile_rows(pz, pyx):
    return 32 if pz <= 9 and not (pz == 9 and pyx == 9) else 24


def sep_tile_rows(pz):
    return 32 if pz <= 9 else 24


def fused_split(tiles_xy, z, pz, cus):
    """``plan_fused_split`` of ``csrc/correlate.hip``: ``(n_full, pieces, z_chunk)``."""
    min_chunk = max(2 * (pz - 1), 8)
    full = tiles_xy // cus * cus
    rest = tiles_xy - full
    if full == 0:
        rest = tiles_xy
    k = max(1, cus // rest if rest > 0 else 1)
    chunk = -(-z // k)
    if chunk < min_chunk:
        chunk = min(min_chunk, z)
    return full, -(-z // chunk), chunk


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def shapes_for(pz, tile, i, cap=220_000):
    """Six (Z, Y, X) for an instance with ``pz`` z taps and ``tile = (rows, columns)``: Y in {1, TY-1, TY, TY+1,
    2 TY + 1}, X in {1, 3, TX-1, TX, TX+1, 2 TX + 1}, Z in {1, PZ-1, PZ, 2 (PZ-1) + 9, 40}, paired differently from
    instance to instance (``i``) and kept below ``cap`` voxels by stepping Z down."""
    ty, tx = tile
    ys = [1, ty - 1, ty, ty + 1, 2 * ty + 1]
    xs = [1, 3, tx - 1, tx, tx + 1, 2 * tx + 1]
    zs = [1, max(1, pz - 1), pz, 2 * (pz - 1) + 9, 40]
    out = []
    for j, zi in enumerate([3, 4, 2, 1, 0, 2]):
        yy, xx = ys[(j + i) % 5], xs[(j + 2 * i + 4) % 6]
        while zi > 0 and zs[zi] * yy * xx > cap:
            zi -= 1
        out.append((zs[zi], yy, xx))
    return out


def _dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), device=device)


def _nan(shape, device):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=device)


def _bound(family, t):
    if family == "dense":
        return min(C_DENSE, F_DENSE * c.ceiling(t))
    if family == "y-separable":
        return min(C_YSEP, F_YSEP * c.ceiling(t))
    return min({"separable": C_SEP, "long-z": C_LONGZ}[family], c.ceiling(t))


def _hold(family, label, got, ref, t, tile=None, pz=None):
    """The per-voxel bound; ``label`` names path, taps and shape, the message adds voxel, tile and z chunk."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    worst, idx, leak = c.worst_voxel(got, ref)
    WORST[family] = max(WORST.get(family, 0.0), worst)
    WORST[family + " / (2T+16)"] = max(WORST.get(family + " / (2T+16)", 0.0), worst / c.ceiling(t))

    def where(v):
        s = f"voxel (z, y, x) = {v}"
        if tile is not None:
            ty, tx = tile
            s += f", tile (row, column) = ({v[1] // ty}, {v[2] // tx}) of {ty} x {tx}"
            if pz is not None:
                z, yy, xx = ref.shape
                n_full, pieces, chunk = fused_split(-(-yy // ty) * -(-xx // tx), z, pz, _cus())
                s += f", z chunk {v[0] // chunk} of {pieces} ({chunk} planes, where the column is cut; n_full {n_full})"
        return s

    assert leak is None, f"{label}: non-zero where the float64 iteration is exactly 0, {where(leak)}"
    bound = _bound(family, t)
    assert worst <= bound, f"{label}: {worst:.3g} u (bound {bound:.3g} u) at {where(idx)}"


def _one(plan, x, y, device, **kw):
    """One iteration from ``x`` into a NaN-filled dense output."""
    out = _nan(plan.shape, device)
    got = plan(_dev(y, device), iterations=1, eps=EPS, x0=None if x is None else _dev(x, device), out=out, **kw)
    assert got is out
    return got


def _sep_taps(pz, py, px, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [c.taps_1d(pz, rng, scale), c.taps_1d(py, rng), c.taps_1d(px, rng)]


def _in_plane(pyx, i):
    """py != px with max(py, px) = pyx, alternating which one is shorter (the centred embedding into the square
    compiled extent)."""
    return (pyx, pyx - 2) if i % 2 == 0 else (pyx - 2, pyx)


# ---------------------------------------------------------------- the sweep itself


def test_the_sweep_covers_every_instance_the_kernels_compile():
    assert len(FUSED) == 46 and len(YSEP) == 20 and len(DENSE) == 20
    odd = range(1, 19, 2)
    lib = _lib.load()
    got = sorted({(max(3, pz), max(3, pyx)) for pz in odd for pyx in odd
                  if _lib.call_value("lsr_rl_sep_fused_supported", pz, pyx, pyx)})
    assert got == sorted(FUSED)
    got = sorted({(max(3, pz), max(3, pyx)) for pz in odd for pyx in odd
                  if _lib.call_value("lsr_rl_ysep_fused_supported", pz, pyx, pyx)})
    assert got == sorted(YSEP)
    got = sorted({(max(3, pz), max(3, pyx)) for pz in odd for pyx in odd if lib.lsr_dense_taps_count(pz, pyx, pyx) > 0})
    assert got == sorted(DENSE)
    assert all(pz * pyx * pyx <= 900 for pz, pyx in DENSE)
    # in-plane extents that differ by two still land in the instance of the larger one
    for pz, pyx in FUSED:
        assert _lib.call_value("lsr_rl_sep_fused_supported", pz, *_in_plane(pyx, 0))
    assert {fused_tile_rows(*p) for p in FUSED} == {32, 24, 16}
    assert {ysep_tile_rows(*p) for p in YSEP} == {32, 24}


# ---------------------------------------------------------------- separable: fused and two-launch, every instance


@pytest.mark.parametrize("pz,pyx", FUSED)
def test_fused_separable_every_instance(device, pz, pyx):
    """``rl_fused_sep_kernel<PZ, PYX, STATS>`` for both values of STATS, six shapes from the instance's own tile; the
    3 x 3 instance also takes tap counts of 1; every fifth instance has taps that sum to 1.7."""
    i = FUSED.index((pz, pyx))
    tile = (fused_tile_rows(pz, pyx), 128)
    py, px = _in_plane(pyx, i)
    psfs = [(pz, py, px)] + ([(1, 1, 1), (1, 3, 1), (3, 1, 1), (1, 1, 3)] if (pz, pyx) == (3, 3) else [])
    for ps in psfs:
        ks = _sep_taps(*ps, seed=100 * pz + pyx, scale=1.7 if i % 5 == 0 else 1.0)
        for shape in shapes_for(pz, tile, i):
            x, y = c.make_inputs(shape, ps, seed=sum(shape) + i, tile=tile)
            ref = o.rl_iteration_f64(x, y, factors=ks, eps=EPS)[2]
            plan = RichardsonLucyPlan(shape, None, device, psf_factors=ks, fused="always")
            assert plan.path == "fused"
            for stats in (False, True):
                got = _one(plan, x, y, device, stats=stats)
                _hold("separable", f"fused stats={stats} taps {ps} shape {shape}", got, ref, sum(ps), tile, pz)


@pytest.mark.parametrize("pz,pyx", FUSED + [(15, 11), (15, 13), (15, 15)])
def test_two_launch_separable_every_instance(device, pz, pyx):
    """``lsr_rl_sep_stats_f32`` (ratio launch, update launch) with the fused sweep's PSFs, plus 15 z taps with 11 .. 15
    in plane, which only this path takes; three shapes per instance."""
    i = (FUSED + [(15, 11), (15, 13), (15, 15)]).index((pz, pyx))
    tile = (sep_tile_rows(pz), 128)
    ps = (pz, pyx, pyx) if (pz, pyx) in ((15, 15), (15, 11)) else (pz,) + _in_plane(pyx, i)
    ks = _sep_taps(*ps, seed=100 * pz + pyx, scale=1.7 if i % 5 == 0 else 1.0)
    for shape in shapes_for(pz, tile, i)[:3]:
        x, y = c.make_inputs(shape, ps, seed=sum(shape) + i, tile=tile)
        ref = o.rl_iteration_f64(x, y, factors=ks, eps=EPS)[2]
        plan = RichardsonLucyPlan(shape, None, device, psf_factors=ks, fused="never")
        assert plan.path == "separable"
        got = _one(plan, x, y, device, stats=bool(i % 2))
        _hold("separable", f"separable taps {ps} shape {shape}", got, ref, sum(ps), tile)


@pytest.mark.parametrize("pz", [17, 23, 31])
@pytest.mark.parametrize("pyx", [3, 7, 15])
def test_long_z_separable(device, pz, pyx):
    """17 .. 31 z taps: the in-plane launch with one z tap, then ``lsr_correlate_z_f32`` carrying the epilogue."""
    ps = (pz,) + _in_plane(pyx, pz)
    ks = _sep_taps(*ps, seed=pz + pyx)
    tile = (32, 128)
    for shape in [(2 * (pz - 1) + 9, 33, 65), (pz - 1, 31, 129), (40, 1, 257), (1, 65, 3)]:
        x, y = c.make_inputs(shape, ps, seed=sum(shape), tile=tile)
        ref = o.rl_iteration_f64(x, y, factors=ks, eps=EPS)[2]
        plan = RichardsonLucyPlan(shape, None, device, psf_factors=ks)
        assert plan.path == "separable (long z, 4 launches)"
        got = _one(plan, x, y, device, stats=bool(pyx == 7))
        _hold("long-z", f"long z taps {ps} shape {shape}", got, ref, sum(ps), tile)


@pytest.mark.parametrize("fused", ["always", "never"])
def test_y_window_plans_take_the_taller_volumes_norm(device, fused):
    """First, middle and last row slab of a taller volume (``shrimpy_amd.slab``): the y factor of ``H^T 1`` is the
    taller volume's, so only the volume's own top or bottom border is normalised."""
    ps = (5, 9, 7)
    ks = _sep_taps(*ps, seed=3)
    tile = (32, 128)
    shape = (12, 33, 130)
    for first, total in ((0, 99), (33, 99), (66, 99), (2, 36)):
        x, y = c.make_inputs(shape, ps, seed=first + total, tile=tile)
        ref = o.rl_iteration_f64(x, y, factors=ks, eps=EPS, y_window=(first, total))[2]
        plan = RichardsonLucyPlan(shape, None, device, psf_factors=ks, fused=fused, y_window=(first, total))
        assert plan.path == ("fused" if fused == "always" else "separable")
        _hold("separable", f"{plan.path} y_window {(first, total)} taps {ps} shape {shape}", _one(plan, x, y, device), ref,
              sum(ps), tile, ps[0] if fused == "always" else None)


# ---------------------------------------------------------------- ky (x) kzx: one launch, two launches, four launches


def _ysep_psf(ps, seed):
    """A ``ky (x) kzx`` PSF with a full-rank ``kzx``, and the float32 factors the plan hands its kernels."""
    rng = np.random.default_rng(seed)
    pz, py, px = ps
    psf = (c.taps_1d(py, rng)[None, :, None].astype(np.float64) * c.taps_nd((pz, px), rng)[:, None, :]).astype(np.float32)
    ky, kzx = factor_psf_y(prepare_psf(psf))
    return psf, (ky, kzx)


def _ysep_in_plane(pyx, i):
    return (3, 3) if pyx == 3 else _in_plane(pyx, i)          # (one x tap would make kzx rank 1: a separable PSF)


@pytest.mark.parametrize("pz,pyx", YSEP)
def test_y_separable_every_instance(device, pz, pyx):
    """``rl_fused_ysep_kernel`` (one launch, with and without the sums) and ``lsr_correlate_zxy_padded_f32`` (two) at
    all 20 instances; the reference is the y pass and the (z, x) stencil of the plan's own float32 factors."""
    i = YSEP.index((pz, pyx))
    tile = (ysep_tile_rows(pz, pyx), 128)
    ps = (pz,) + _ysep_in_plane(pyx, i)
    psf, factors = _ysep_psf(ps, 100 * pz + pyx)
    t = ps[0] * ps[2] + ps[1]
    for j, shape in enumerate(shapes_for(pz, tile, i, cap=120_000)):
        x, y = c.make_inputs(shape, ps, seed=sum(shape) + i, tile=tile)
        ref = o.rl_iteration_f64(x, y, factors=factors, eps=EPS)[2]
        plan = RichardsonLucyPlan(shape, psf, device)
        assert plan.path == "y-separable (fused)"
        for stats in (False, True):
            got = _one(plan, x, y, device, stats=stats)
            _hold("y-separable", f"y-separable (fused) stats={stats} taps {ps} shape {shape}", got, ref, t, tile, pz)
        if j < 3:
            plan = RichardsonLucyPlan(shape, psf, device, fused="never")
            assert plan.path == "y-separable"
            _hold("y-separable", f"y-separable taps {ps} shape {shape}", _one(plan, x, y, device, stats=bool(j % 2)), ref, t,
                  (32, 64))


@pytest.mark.parametrize("ps", [(3, 11, 3), (7, 13, 5), (11, 15, 9), (5, 11, 7)])
def test_y_separable_four_launches(device, ps):
    """11 .. 15 y taps: the (z, x) stencil and the y pass as separate launches."""
    psf, factors = _ysep_psf(ps, sum(ps))
    t = ps[0] * ps[2] + ps[1]
    for shape in [(2 * (ps[0] - 1) + 9, 33, 65), (ps[0], 31, 129), (1, 65, 64), (40, 1, 3)]:
        x, y = c.make_inputs(shape, ps, seed=sum(shape), tile=(32, 64))
        ref = o.rl_iteration_f64(x, y, factors=factors, eps=EPS)[2]
        plan = RichardsonLucyPlan(shape, psf, device)
        assert plan.path == "y-separable (4 launches)"
        got = _one(plan, x, y, device, stats=bool(ps[0] == 7))
        _hold("y-separable", f"y-separable (4 launches) taps {ps} shape {shape}", got, ref, t, (32, 64))


# ---------------------------------------------------------------- dense: tuned at every instance, generic past it


@pytest.mark.parametrize("pz,pyx", DENSE)
def test_dense_every_instance(device, pz, pyx):
    i = DENSE.index((pz, pyx))
    tile = (32, 64)
    ps = (pz,) + _in_plane(pyx, i)
    psf = c.taps_nd(ps, np.random.default_rng(100 * pz + pyx), 1.7 if i % 5 == 0 else 1.0)
    for shape in shapes_for(pz, tile, i, cap=40_000)[:4]:
        x, y = c.make_inputs(shape, ps, seed=sum(shape) + i, tile=tile)
        ref = o.rl_iteration_f64(x, y, psf=psf, eps=EPS)[2]
        plan = RichardsonLucyPlan(shape, psf, device, separable="never")
        assert plan.path == "dense"
        got = _one(plan, x, y, device, stats=bool(i % 2))
        _hold("dense", f"dense taps {ps} shape {shape}", got, ref, int(np.prod(ps)), tile)


def test_generic_dense_past_the_tuned_range(device):
    ps = (13, 11, 5)
    psf = c.taps_nd(ps, np.random.default_rng(7))
    for shape in [(14, 12, 30), (3, 33, 65), (25, 1, 17)]:
        x, y = c.make_inputs(shape, ps, seed=sum(shape), tile=(8, 32))
        ref = o.rl_iteration_f64(x, y, psf=psf, eps=EPS)[2]
        plan = RichardsonLucyPlan(shape, psf, device, separable="never")
        assert plan.path == "generic"
        for stats in (False, True):
            _hold("dense", f"generic taps {ps} shape {shape}", _one(plan, x, y, device, stats=stats), ref, int(np.prod(ps)))


# ---------------------------------------------------------------- the three regimes of the work split


def _regime(tiles_xy, z, pz):
    n_full, pieces, chunk = fused_split(tiles_xy, z, pz, _cus())
    if n_full > 0:
        return "full rounds + cut rest" if tiles_xy - n_full > 0 else "full rounds"
    return "cut, pieces > 1" if pieces > 1 else "cut, pieces == 1"


def test_the_fused_sweeps_hit_both_regimes_of_a_partial_round(device):
    for table, rows in ((FUSED, fused_tile_rows), (YSEP, ysep_tile_rows)):
        seen = set()
        for i, (pz, pyx) in enumerate(table):
            ty = rows(pz, pyx)
            for z, yy, xx in shapes_for(pz, (ty, 128), i, 220_000 if table is FUSED else 120_000):
                seen.add(_regime(-(-yy // ty) * -(-xx // 128), z, pz))
        assert {"cut, pieces > 1", "cut, pieces == 1"} <= seen


@pytest.mark.parametrize("kind", ["fused", "y-separable (fused)"])
def test_full_rounds_of_whole_columns_plus_a_cut_remainder(device, kind):
    """More tiles than CUs: ``n_full > 0`` whole columns and ``rest > 0`` columns cut along z (on 256 CUs: 264 tiles of
    16 or 32 rows by 128 columns, 20 planes)."""
    cus = _cus()
    ps = (3, 13, 11) if kind == "fused" else (3, 5, 3)
    ty = fused_tile_rows(3, 13) if kind == "fused" else ysep_tile_rows(3, 5)
    tiles = cus + 8                                              # one tile row: 5 rows of the volume
    shape = (20, 5, 128 * (tiles - 1) + 5)
    assert _regime(tiles, shape[0], ps[0]) == "full rounds + cut rest"
    n_full, pieces, _ = fused_split(tiles, shape[0], ps[0], cus)
    assert n_full == cus and pieces > 1
    x, y = c.make_inputs(shape, ps, seed=cus, tile=(ty, 128))
    if kind == "fused":
        ks = _sep_taps(*ps, seed=1)
        ref = o.rl_iteration_f64(x, y, factors=ks, eps=EPS)[2]
        plan = RichardsonLucyPlan(shape, None, device, psf_factors=ks, fused="always")
        family, t = "separable", sum(ps)
    else:
        psf, factors = _ysep_psf(ps, 1)
        ref = o.rl_iteration_f64(x, y, factors=factors, eps=EPS)[2]
        plan = RichardsonLucyPlan(shape, psf, device)
        family, t = "y-separable", ps[0] * ps[2] + ps[1]
    assert plan.path == kind
    for stats in (False, True):
        _hold(family, f"{kind} stats={stats} taps {ps} shape {shape}", _one(plan, x, y, device, stats=stats), ref, t,
              (ty, 128), ps[0])


# ---------------------------------------------------------------- calling conventions


CONVENTION_PLANS = [
    ("fused", (9, 7, 5), dict(fused="always")),
    ("fused", (13, 11, 13), dict(fused="always")),
    ("separable", (9, 7, 5), dict(fused="never")),
    ("y-separable (fused)", (9, 5, 7), dict()),
    ("y-separable", (9, 5, 7), dict(fused="never")),
    ("dense", (5, 7, 5), dict(separable="never")),
]


def _convention_case(path, ps, kw, device, shape):
    if path in ("fused", "separable"):
        ks = _sep_taps(*ps, seed=sum(ps))
        plan = RichardsonLucyPlan(shape, None, device, psf_factors=ks, **kw)
        ref_kw, family, t = dict(factors=ks), "separable", sum(ps)
    elif path.startswith("y-separable"):
        psf, factors = _ysep_psf(ps, sum(ps))
        plan = RichardsonLucyPlan(shape, psf, device, **kw)
        ref_kw, family, t = dict(factors=factors), "y-separable", ps[0] * ps[2] + ps[1]
    else:
        psf = c.taps_nd(ps, np.random.default_rng(sum(ps)))
        plan = RichardsonLucyPlan(shape, psf, device, **kw)
        ref_kw, family, t = dict(psf=psf), "dense", int(np.prod(ps))
    assert plan.path == path
    return plan, ref_kw, family, t


@pytest.mark.parametrize("path,ps,kw", CONVENTION_PLANS)
def test_x0_from_y_and_a_padded_y(device, path, ps, kw):
    """``x0 = None`` (the first iteration reads ``y`` as the estimate), ``y`` handed over as the plan's
    ``PaddedVolume`` with and without ``x0``."""
    shape = (2 * (ps[0] - 1) + 9, 34, 131)
    plan, ref_kw, family, t = _convention_case(path, ps, kw, device, shape)
    x, y = c.make_inputs(shape, ps, seed=5)
    y[y == 0] = 3.0                                  # (y is the estimate too: keep a zero box from x instead)
    y[x == 0] = 0.0
    from_y = o.rl_iteration_f64(y, y, eps=EPS, **ref_kw)[2]
    from_x = o.rl_iteration_f64(x, y, eps=EPS, **ref_kw)[2]
    _hold(family, f"{path} x0=None taps {ps} shape {shape}", _one(plan, None, y, device), from_y, t)
    y_pad = plan.new_padded_input()
    y_pad.view.copy_(_dev(y, device))
    out = _nan(shape, device)
    plan(y_pad, iterations=1, eps=EPS, out=out)
    _hold(family, f"{path} padded y, x0=None taps {ps} shape {shape}", out, from_y, t)
    out = _nan(shape, device)
    plan(y_pad, iterations=1, eps=EPS, x0=_dev(x, device), out=out, stats=True)
    _hold(family, f"{path} padded y taps {ps} shape {shape}", out, from_x, t)
    assert torch.equal(y_pad.view, _dev(y, device)), "the padded y was written"


@pytest.mark.parametrize("ps", [(9, 7, 5), (3, 15, 13), (13, 11, 9)])
def test_fused_entry_with_wider_y_strides_padded_and_dense_results(device, ps):
    """``lsr_rl_sep_fused_stats_f32`` itself: ``y`` in an allocation whose pitch and plane stride exceed what
    ``lsr_sep_padded_shape`` asks for; the result left in the padded working volume (``x_out = NULL``, unmasked
    stores) and written to a dense ``x_out`` (masked stores) are the same bits; the halo of both working volumes is
    still zero afterwards and the dense output is written nowhere outside ``(Z, Y, X)``."""
    ty = fused_tile_rows(ps[0], max(ps[1:]))
    shape = (2 * (ps[0] - 1) + 9, ty + 3, 133)
    z, yy, xx = shape
    ks = _sep_taps(*ps, seed=sum(ps), scale=1.7)
    x, y = c.make_inputs(shape, ps, seed=11, tile=(ty, 128))
    ref = o.rl_iteration_f64(x, y, factors=ks, eps=EPS)[2]
    rows, pitch, oy, ox = padded_shape(shape, ps)
    y_full = torch.zeros((z, rows + 3, pitch + 8), dtype=torch.float32, device=device)
    y_full[:, oy:oy + yy, ox:ox + xx] = _dev(y, device)
    y_ptr = y_full[0, oy, ox:].data_ptr()
    block = np.zeros(_lib.call_value("lsr_rl_sep_fused_taps_count"), np.float32)
    _lib.call("lsr_rl_sep_fused_prepare_taps", ks[0].ctypes.data, ps[0], ks[1].ctypes.data, ps[1], ks[2].ctypes.data, ps[2],
              block.ctypes.data)
    taps = _dev(block, device)
    norms = [_dev(_axis_norm(k, n), device) for k, n in zip(ks, shape)]
    guard = 4 * xx
    results = []
    for dense in (False, True):
        a, b = PaddedVolume(shape, ps, device), PaddedVolume(shape, ps, device)
        a.view.copy_(_dev(x, device))
        flat = _nan((guard + z * yy * xx + guard,), device)
        stats = torch.zeros(3, dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            _lib.call("lsr_rl_sep_fused_stats_f32", y_ptr, pitch + 8, (rows + 3) * (pitch + 8), 0, a.full.data_ptr(),
                      b.full.data_ptr(), flat[guard:].data_ptr() if dense else None, z, yy, xx, taps.data_ptr(), *ps,
                      *(n.data_ptr() for n in norms), 1, ctypes.c_float(EPS), stats.data_ptr(), _lib.stream_ptr(device))
        got = flat[guard:guard + z * yy * xx].reshape(shape) if dense else b.view
        _hold("separable", f"fused entry dense_out={dense} taps {ps} shape {shape}", got, ref, sum(ps), (ty, 128), ps[0])
        results.append(got.clone())
        if dense:
            assert torch.isnan(flat[:guard]).all() and torch.isnan(flat[guard + z * yy * xx:]).all(), \
                "the dense output was written outside (Z, Y, X)"
            assert not b.full.any(), "the unused working volume was written"
        else:
            halo = b.full.clone()
            halo[:, oy:oy + yy, ox:ox + xx] = 0
            assert not halo.any(), "the halo of the padded result is not zero"
            assert torch.isnan(flat).all()
        halo = a.full.clone()
        halo[:, oy:oy + yy, ox:ox + xx] = 0
        assert not halo.any() and torch.equal(a.view, _dev(x, device)), "the source working volume was written"
    assert torch.equal(results[0], results[1]), "padded and dense results differ"


@pytest.mark.parametrize("path,ps,kw", CONVENTION_PLANS)
def test_a_chain_of_single_iterations_and_the_ping_pong(device, path, ps, kw):
    """Six single iterations, each fed the device's own previous float32 estimate and checked against the float64
    iteration restarted from that estimate (the bound stays per iteration); ``plan(y, iterations=n)`` equals the
    chain's n-th estimate bit for bit for odd and even n (the working volumes ping-pong)."""
    shape = (2 * (ps[0] - 1) + 9, 33, 130)
    plan, ref_kw, family, t = _convention_case(path, ps, kw, device, shape)
    x, y = c.make_inputs(shape, ps, seed=23)
    yd, x0 = _dev(y, device), _dev(x, device)
    chain = [x0]
    for it in range(6):
        cur = chain[-1]
        ref = o.rl_iteration_f64(cur.cpu().numpy(), y, eps=EPS, **ref_kw)[2]
        out = _nan(shape, device)
        plan(yd, iterations=1, eps=EPS, x0=cur, out=out)
        _hold(family, f"{path} chain iteration {it} taps {ps} shape {shape}", out, ref, t)
        chain.append(out)
    for n in (5, 6):
        out = _nan(shape, device)
        plan(yd, iterations=n, eps=EPS, x0=x0, out=out)
        assert torch.equal(out, chain[n]), f"{path}: {n} iterations in one call differ from the chain of single ones"
