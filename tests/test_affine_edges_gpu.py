"""The three affine kernels on the MI355X (``csrc/affine.hip``, ``affine_planar.hip``, ``affine_box.hip``) against the restated rule
(``tests/affine_ref.py``) and the host twin, on every case of ``tests/affine_cases.py``: every planar tile under both wave counts at
its threshold, both rings, the z march at its chunk and volume edges, every patch decode, every box block shape, walk and block
kind with a corner on each value a kind is decided on, grid points, padded rows and planes on both sides, and the contents.

Exact mode has no tolerance anywhere and leaves no voxel out: the whole output window equals the restatement bit for bit (a NaN by
position) under both borders, through ``lsr_affine_pitched_f32`` and, for dense cases, ``lsr_affine_f32``; it equals the twin; every
word of the window is written and none outside it; the kernel that ran is the one the plan names and the case aims at; and the same
voxels through a source pitch neither LDS kernel takes -- the gather kernel -- give the same bits.

``tests/test_affine_host.py`` asserts that the cases reach what they aim at and that the staged boxes hold every tap.
"""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from tests import affine_cases as C
from tests import affine_ref as R
from tests import test_affine_host as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                # the unit roundoff of float32
F32_UNITS = 16.0                              # the bound of test_f32_mode_stays_within_its_a_priori_bound, in units of U max|tap|


def _d(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)


def run_kernel(c, mode, device, f32=False, dense_entry=False, pitch=None):
    """The whole output buffer (uint32 words, ``C.output_buffer``'s layout) after the entry ran on it under the environment as it
    stands; ``pitch``: the same voxels on another source pitch."""
    src = _d(C.source(c.name) if dense_entry else C.source_buffer(c, pitch), device)
    buf = _d(C.output_buffer(c).view(np.int32), device)
    code = C.MODE_CODE[mode] | (_lib.MODE_F32_INTERP if f32 else 0)
    with torch.cuda.device(device):
        stream = _lib.stream_ptr(device)
        if dense_entry:
            assert c.dense
            _lib.call("lsr_affine_f32", src.data_ptr(), *c.shape, buf.data_ptr(), *c.out_shape, _lib.matrix12(c.m), float(c.cval), code,
                      stream)
        else:
            _lib.call("lsr_affine_pitched_f32", src.data_ptr(), *c.shape, src.shape[2], src.shape[1] * src.shape[2], buf.data_ptr(),
                      *c.out_shape, c.out_pitch, c.out_plane, _lib.matrix12(c.m), float(c.cval), code, stream)
    torch.cuda.synchronize(device)
    return buf.cpu().numpy().view(np.uint32)


def switches(mp, c):
    """The case's measurement switches through ``monkeypatch``; asserts through the plan that they reach the launcher."""
    for k in C.SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in c.env:
        mp.setenv(k, v)
    p = C.raw_plan(c.shape, c.pitch, c.plane, c.out_shape, c.out_pitch, c.m, 0)
    assert p == c.plan() and p[0] == c.path, (c.name, p)
    env = dict(c.env)
    if "LSR_PLANAR_WAVES" in env and p[0] == 1 and c.aimed("at") != "next":      # (past the last four-wave tile: eight waves again)
        assert p[1] == int(env["LSR_PLANAR_WAVES"]), (c.name, p)
    if "LSR_PLANAR_PATCH" in env:
        assert "%d,%d" % (p[11], p[12]) == env["LSR_PLANAR_PATCH"], (c.name, p)
    if "LSR_BOX_LINEAR" in env:
        assert p[11] == int(env["LSR_BOX_LINEAR"]), (c.name, p)
    return p


def check_window(c, buf, mode, what):
    H.check(C.window(c, buf), c.name, mode, what)
    kept, written = C.padding_intact(c, buf)
    assert kept, f"{c.name} [{mode}] {what}: a word outside the output window was written"
    assert written, f"{c.name} [{mode}] {what}: a word of the output window was left unwritten"


@pytest.mark.parametrize("g", C.GROUPS)
def test_kernels_equal_the_restatement_and_the_twin_bit_for_bit(device, monkeypatch, g):
    """Non-finite volumes included: their cases hold no voxel with a coordinate exactly on ``n - 1`` (asserted on the host), so the
    rule of ``lsr_affine_f32``'s header leaves nothing out and all three kernels are compared on every voxel."""
    for name in C.group(g):
        c = C.case(name)
        with monkeypatch.context() as mp:
            switches(mp, c)
            for mode in R.MODES:
                buf = run_kernel(c, mode, device)
                check_window(c, buf, mode, f"lsr_affine_pitched_f32 (path {c.path})")
                out = C.window(c, buf)
                twin = H.case_twin(name, mode)
                assert R.same_bits(out, twin), f"{name} [{mode}]: kernel and twin differ: {R.describe_difference(out, twin)}"
                if c.dense:
                    check_window(c, run_kernel(c, mode, device, dense_entry=True), mode, f"lsr_affine_f32 (path {c.path})")
                if c.path != 0:
                    assert c.plan(mode, pitch=c.gather_pitch)[0] == 0
                    check_window(c, run_kernel(c, mode, device, pitch=c.gather_pitch), mode, "the gather kernel on the same voxels")


def f32_check(c, mode, device, pitch=None):
    """The worst ratio error / (U max|tap|) of a case under ``LSR_MODE_F32_INTERP``; asserts cval's bits outside and the window."""
    e = C.expected(c.name, mode)
    buf = run_kernel(c, mode, device, f32=True, pitch=pitch)
    assert C.padding_intact(c, buf) == (True, True), (c.name, mode)
    out = C.window(c, buf)
    if mode == "constant":
        assert (R.bits(out)[~e.inside] == R.bits(np.float32(c.cval))).all(), f"{c.name}: a voxel outside does not carry cval's bits"
    err = np.abs(out.astype(np.float64) - e.exact)[e.inside]
    scale = U * e.max_tap.astype(np.float64)[e.inside]
    assert (err <= F32_UNITS * scale).all(), (f"{c.name} [{mode}]: {int((err > F32_UNITS * scale).sum())} voxels beyond the bound, "
                                             f"worst {float((err / np.maximum(scale, 1e-300)).max()):.2f} units")
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


@pytest.mark.parametrize("g", C.GROUPS)
def test_f32_mode_stays_within_its_a_priori_bound(device, monkeypatch, g):
    """``LSR_MODE_F32_INTERP``: coordinates and border decisions in float64 (under "constant" a voxel the restatement calls outside
    carries cval's bits), then seven ``fmaf(w, hi - lo, lo)`` in float32 -- x, then y, then z -- with the float64 fractions rounded
    to float32 as weights (``trilinear_f32`` of csrc/resample.hpp; the gather kernel spells the same seven).  With ``M`` the largest
    magnitude among the voxel's eight taps (cval where a tap is outside) and ``U = 2^-24``, one level ``fmaf(w, b - a, a)`` adds

    * ``2 M U`` for the rounded difference ``b - a`` (``|b - a| <= 2 M``), times a weight of at most 1;
    * ``2 M U`` for the weight's own rounding (relative ``U``, times ``|b - a| <= 2 M``);
    * ``M U`` for the FMA's rounding of a result of magnitude at most ``M`` (a convex combination);

    5 units, and a level passes its inputs' errors on with weights that sum to 1: 5, 10, 15 units after x, y and z.  The reference
    is the restatement's float64 corner sum before its rounding (its own error, 8 roundings of float64, is 2^-29 units); the
    second-order terms (magnitudes up to ``M (1 + 10 U)``) are far below the unit left over.  Bound: 16 ``U M``, for all three
    kernels.  Volumes of ``+-3e38`` (whose differences overflow float32), denormals and non-finite values are not run in this mode.
    """
    worst = 0.0
    for name in C.group(g):
        c = C.case(name)
        if not c.f32:
            continue
        with monkeypatch.context() as mp:
            switches(mp, c)
            for mode in R.MODES:
                assert c.plan(mode, f32=True)[0] == c.path
                worst = max(worst, f32_check(c, mode, device))
                if c.path != 0:
                    worst = max(worst, f32_check(c, mode, device, pitch=c.gather_pitch))
    assert worst <= F32_UNITS
