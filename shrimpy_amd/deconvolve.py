"""Richardson-Lucy 3-D deconvolution on MI355X.

No reference symbol exists (``docs/data_structure.md:58-62``: "algorithms for deconvolution ...
are being developed"); the north-star defines the step: 20 iterations of

    x <- x * H^T( y / (H x + eps) ) / (H^T 1)

with a 3-D PSF stencil and zero-padded borders, CPU path = explicit loop over
``scipy.ndimage.convolve`` / ``correlate`` (``oracle/cpu_ref.py:richardson_lucy``, test-only).

Each iteration is two launches of the z-marching LDS stencil ``csrc/correlate.hip`` with fused
epilogues (ratio; multiplicative update with analytic ``H^T 1``): 12 algorithmic bytes per voxel
per launch.  Rank-1 (separable) PSFs run ``pz+py+px`` FMAs per voxel and are HBM-bound; dense
PSFs run ``pz*py*px`` FMAs per voxel and are fp32-VALU-bound.  float32 throughout; agreement
with the float64-accumulating scipy loop is stated in ``tests/test_gpu_parity.py``.
CPU tensors (no HIP device in play) run the native host twins of the same launches (``shrimpy_amd/host.py``).

``tv_lambda > 0`` adds total-variation regularisation in the multiplicative form of Dey et al. 2006 (RL-TV): the
iteration's result is divided voxel by voxel by ``1 - tv_lambda * div(grad x_k / |grad x_k|)`` (forward differences,
backward divergence, the volume's own borders; ``csrc/rl_tv.hip``, one more streaming launch of 12 bytes per voxel per
iteration behind the unchanged RL launches).  ``tv_lambda = 0`` (the default) is the plain iteration, launch for launch.

``acceleration="biggs-andrews"`` starts every iteration from a point extrapolated along the last change (Biggs & Andrews
1997; ``csrc/rl_accel.hip``: two more streaming launches per iteration, 16 + 12 bytes per voxel, no tuning parameter, no
host round trip) and reaches the likelihood of a plain run in a third to a half of its iterations.  ``"none"`` (the
default) is the plain run, launch for launch.
"""

from __future__ import annotations

import ctypes

from dataclasses import dataclass

import numpy as np

from . import _lib, rl_loop

__all__ = ["richardson_lucy", "RichardsonLucyPlan", "RLStats", "factor_psf", "correlate3d", "prepare_psf",
           "padded_shape", "PaddedVolume", "make_plan", "check_tv", "TV_LAMBDA_LIMIT", "check_acceleration",
           "ACCELERATIONS"]

TV_LAMBDA_LIMIT = 1.0 / 6.0     # |div(grad x / |grad x|)| <= 6: below this the RL-TV denominator is provably positive


def check_tv(tv_lambda, tv_eps) -> tuple[float, float]:
    """``(tv_lambda, tv_eps)`` as floats, or ``ValueError``: ``0 <= tv_lambda < 1/6`` (also as the float32 the kernels
    take), ``tv_eps > 0`` and finite.  NaN fails both."""
    lam, te = float(tv_lambda), float(tv_eps)
    if not (0.0 <= lam < TV_LAMBDA_LIMIT and np.float32(lam) < np.float32(1.0) / np.float32(6.0)):
        raise ValueError(f"tv_lambda must be in [0, 1/6), got {tv_lambda!r}")
    if not (te > 0.0 and np.isfinite(te)):
        raise ValueError(f"tv_eps must be a finite number > 0, got {tv_eps!r}")
    return lam, te


ACCELERATIONS = ("none", "biggs-andrews")


def check_acceleration(acceleration, tv_lambda: float = 0.0) -> bool:
    """Whether the Biggs-Andrews extrapolation is on, or ``ValueError``: an unknown name, or acceleration together with
    ``tv_lambda > 0`` (the TV factor changes the map whose fixed point the extrapolation heads for)."""
    if acceleration not in ACCELERATIONS:
        raise ValueError(f"acceleration must be one of {ACCELERATIONS}, got {acceleration!r}")
    on = acceleration == "biggs-andrews"
    if on and tv_lambda > 0:
        raise ValueError("acceleration='biggs-andrews' cannot be combined with tv_lambda > 0: the total-variation factor "
                         "breaks the fixed-point map the extrapolation assumes")
    return on


MAX_TAPS = 15
MAX_Z_TAPS = 31     # separable PSFs only: the z factor runs as its own launch (csrc/correlate_z.hip)


def prepare_psf(psf, max_in_plane: int = MAX_TAPS, max_z: int = MAX_Z_TAPS) -> np.ndarray:
    """float32 (pz, py, px) with every axis odd: even axes get one trailing zero plane.

    With ``center = size // 2`` the padded kernel produces the same correlation.
    """
    p = np.asarray(psf, dtype=np.float32)
    if p.ndim != 3:
        raise ValueError(f"psf must be 3-D (Z, Y, X), got shape {p.shape}")
    if not np.all(np.isfinite(p)):
        raise ValueError("psf contains non-finite values")
    pad = [(0, 1 - (s % 2)) for s in p.shape]
    if any(hi for _, hi in pad):
        p = np.pad(p, pad)
    if max(p.shape[1:]) > max_in_plane or p.shape[0] > max_z:
        raise ValueError(f"psf shape {p.shape} exceeds {max_in_plane} taps in plane / {max_z} along z")
    return np.ascontiguousarray(p)


def factor_psf(psf, rtol: float = 1e-6):
    """Rank-1 factorisation ``psf ~= kz x ky x kx`` or ``None``.

    Accepted when ``max|psf - kz*ky*kx| <= rtol * max|psf|`` (float64 check).  Factors are
    returned as float32 with the overall scale carried by ``kz``.
    """
    p = np.asarray(psf, dtype=np.float64)
    pz, py, px = p.shape
    peak = np.abs(p).max()
    if peak == 0:
        return None
    u, s, vt = np.linalg.svd(p.reshape(pz, py * px), full_matrices=False)
    kz = u[:, 0] * s[0]
    yx = vt[0].reshape(py, px)
    u2, s2, vt2 = np.linalg.svd(yx, full_matrices=False)
    ky = u2[:, 0] * s2[0]
    kx = vt2[0]
    # fix signs so the in-plane factors are predominantly positive
    if ky.sum() < 0:
        ky, kz = -ky, -kz
    if kx.sum() < 0:
        kx, kz = -kx, -kz
    # balance: in-plane factors sum to 1, scale stays in kz
    sy, sx = ky.sum(), kx.sum()
    if sy != 0 and sx != 0:
        ky, kx, kz = ky / sy, kx / sx, kz * sy * sx
    approx = kz[:, None, None] * ky[None, :, None] * kx[None, None, :]
    if np.abs(approx - p).max() > rtol * peak:
        return None
    return kz.astype(np.float32), ky.astype(np.float32), kx.astype(np.float32)


def factor_psf_y(psf: np.ndarray, rtol: float = 1e-6):
    """``(ky, kzx)`` with ``psf[z, y, x] == ky[y] * kzx[z, x]`` to within ``rtol * max|psf|``, or ``None``.

    The PSF of an oblique light sheet is tilted in the (z, x) plane and Gaussian along y: it does not
    factor into three 1-D kernels, but it does factor into a y kernel and a dense (z, x) stencil.
    ``ky`` is normalised to sum 1 (the scale stays in ``kzx``).
    """
    p = np.asarray(psf, dtype=np.float64)
    pz, py, px = p.shape
    peak = np.abs(p).max()
    if peak == 0 or py == 1:
        return None
    m = p.transpose(1, 0, 2).reshape(py, pz * px)
    u, sv, vt = np.linalg.svd(m, full_matrices=False)
    ky, kzx = u[:, 0] * sv[0], vt[0].reshape(pz, px)
    if ky.sum() < 0:
        ky, kzx = -ky, -kzx
    sy = ky.sum()
    if sy == 0:
        return None
    ky, kzx = ky / sy, kzx * sy
    if np.abs(ky[None, :, None] * kzx[:, None, :] - p).max() > rtol * peak:
        return None
    return ky.astype(np.float32), kzx.astype(np.float32)


def _axis_norm(k: np.ndarray, n: int) -> np.ndarray:
    """sum of the taps of a 1-D correlation kernel that land inside [0, n), per position."""
    p = len(k)
    c = p // 2
    cs = np.concatenate([[0.0], np.cumsum(k.astype(np.float64))])
    pos = np.arange(n)
    lo = np.maximum(0, c - pos)
    hi = np.minimum(p, n - pos + c)
    return (cs[hi] - cs[lo]).astype(np.float32)


def _prefix_table(w: np.ndarray) -> np.ndarray:
    pz, py, px = w.shape
    t = np.zeros((pz + 1, py + 1, px + 1), dtype=np.float64)
    t[1:, 1:, 1:] = w.astype(np.float64).cumsum(0).cumsum(1).cumsum(2)
    return t


def prepared_dense_taps(psf: np.ndarray):
    """``(taps, taps_flipped)`` host arrays in the tuned dense kernel's layout, or ``None`` when the
    PSF is outside its range (pz <= 11, py, px <= 9): see ``lsr_dense_prepare_taps``."""
    pz, py, px = (int(v) for v in psf.shape)
    lib = _lib.load()
    n = lib.lsr_dense_taps_count(pz, py, px)
    if n < 0:
        return None
    src = np.ascontiguousarray(psf, dtype=np.float32)
    out = []
    for flip in (0, 1):
        buf = np.empty(n, dtype=np.float32)
        _lib.call("lsr_dense_prepare_taps", src.ctypes.data, pz, py, px, flip, buf.ctypes.data)
        out.append(buf)
    return tuple(out)


def padded_shape(shape_zyx, psf_shape):
    """Padded plane geometry the tuned separable kernel reads through (``lsr_sep_padded_shape``).

    Returns ``(rows, pitch, origin_row, origin_col)``: a padded volume is ``(Z, rows, pitch)``
    float32 with the logical ``(Y, X)`` window at ``[origin_row:, origin_col:]`` and zeros elsewhere.
    """
    out = (ctypes.c_int64 * 4)()
    _lib.call("lsr_sep_padded_shape", int(shape_zyx[1]), int(shape_zyx[2]), int(psf_shape[0]),
              int(psf_shape[1]), int(psf_shape[2]), out)
    return tuple(int(v) for v in out)


class PaddedVolume:
    """A zero-haloed working volume: ``.full`` is the allocation, ``.view`` the logical window."""

    def __init__(self, shape_zyx, psf_shape, device):
        import torch

        z, y, x = (int(v) for v in shape_zyx)
        rows, pitch, oy, ox = padded_shape(shape_zyx, psf_shape)
        self.full = torch.zeros((z, rows, pitch), dtype=torch.float32, device=device)
        self.view = self.full[:, oy:oy + y, ox:ox + x]
        self.pitch, self.plane = pitch, rows * pitch

    def logical_ptr(self) -> int:
        return self.view.data_ptr()


@dataclass
class RLStats:
    """Per-iteration reduction scalars of a Richardson-Lucy run (``include/lsrecon.h``, ``lsr_rl_*_stats_f32``), summed
    by the kernels in the epilogue that writes the new estimate -- no extra pass over the volume.

    ``flux[i]   = sum x_i * H^T(ratio_i) = sum x_{i+1} * H^T 1`` (what the update conserves; ``-> sum y`` as ``eps -> 0``),
    ``change[i] = sum |x_{i+1} - x_i|``, ``total[i] = sum x_{i+1}``; ``rel_change = change / total`` is what ``tol`` tests.
    ``iterations`` = launches that ran (``< `` the requested count when ``tol`` stopped the loop).

    With ``tv_lambda > 0`` the iterate is the RL update divided by the total-variation factor: ``change`` and ``total``
    are then summed by the TV launch over the iterate the caller gets (``lsr_rl_tv_scale_f32``), and ``tol`` tests
    those.  ``flux`` has no counterpart there: it stays the RL launch's value, i.e. the flux BEFORE the TV factor.

    With ``acceleration="biggs-andrews"`` the scalars keep the RL launch's meaning, and that launch reads the
    extrapolated point ``p_i``: ``change[i] = sum |x_{i+1} - p_i|`` (``p_0 = x_0``), ``flux`` and ``total`` describe
    ``x_{i+1}``.  ``alphas`` (host route; the plans keep ``plan.last_alphas``) are the step lengths a_1 .. used."""

    flux: np.ndarray
    change: np.ndarray
    total: np.ndarray
    iterations: int
    stopped_by_tol: bool = False
    alphas: np.ndarray | None = None

    @property
    def rel_change(self) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.total > 0, self.change / self.total, 0.0)

    @classmethod
    def from_array(cls, a, iterations: int, stopped: bool = False) -> "RLStats":
        a = np.asarray(a, dtype=np.float64).reshape(-1, 3)[:iterations]
        return cls(flux=a[:, 0].copy(), change=a[:, 1].copy(), total=a[:, 2].copy(), iterations=int(iterations),
                   stopped_by_tol=bool(stopped))



def fused_pays(pz: int, py: int, px: int) -> bool:
    """Whether the one-launch iteration beats the ratio / update pair for a separable PSF of this extent.

    Its tile shrinks from 32 x 128 to 16 x 128 as the in-plane extent grows (the window's halo takes the LDS), and
    with 13 or 15 in-plane taps and a short z extent the pair is ~10 % faster; everywhere else the fused launch wins
    by 20-40 % (config-2 grid, ``tools/bench_kernels.py --psf-sweep --psf-sweep-wide``,
    ``profiles/r03_rl_psf_sweep.jsonl``: e.g. 5x13x13 4.79 vs 4.28 ms, 11x13x13 5.14 vs 5.34, 9x7x7 2.50 vs 4.31)."""
    return max(py, px) <= 11 or pz >= 11


def _dev(a, device, dtype=np.float32):
    import torch

    # (np.array copies: a reversed 1-element view keeps its negative stride otherwise)
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device=device)


class _Path(rl_loop.InPlace):
    """One way of running RL iterations on the device -- the stepper ``rl_loop.run`` drives: its tap and normalisation
    tensors, its scratch and its launches.  Working volumes carry a zero halo (the kernels never bounds-check a load);
    unless the path ``rotates`` between the two, the estimate lives in the first and the second takes the ratio."""

    name = ""
    separable = False          # three 1-D factors
    padded = True              # works in padded volumes and takes a padded y
    needs_padded_y = False     # ... and reads y on the tile grown by the PSF radius: a dense y is copied into one
    reads_y = True             # iteration 0 can take x_0 = y from a padded y (no copy into the working volume)
    dense_out = True           # the last launch can write a dense volume

    def __init__(self, shape, psf_shape, device):
        super().__init__(shape, device)
        self.psf_shape = tuple(int(v) for v in psf_shape)
        self.pad_psf_shape = self.psf_shape     # the PSF extents the padded volumes are laid out for
        self._vols = None

    def volumes(self):
        if self._vols is None:
            self._vols = [PaddedVolume(self.shape, self.pad_psf_shape, self.device) for _ in range(2)]
        return self._vols

    @property
    def cur(self):
        return self.volumes()[0]

    def release(self) -> None:
        self._vols = None
        self.drop_sides()

    def begin(self, y, from_y: bool, eps: float, stream) -> None:
        """The run that follows: ``y`` as (pointer, pitch, plane); ``from_y``: iteration 0 reads it as x_0."""
        self.y, self.from_y, self.eps, self.stream = y, from_y, ctypes.c_float(eps), stream
        self.restart()

    def load(self, init, out) -> None:
        self.cur.view.copy_(init)

    def _target(self, x_out):
        return rl_loop.tri(self.cur if x_out is None else x_out)


class _Rotating(_Path):
    """One launch per iteration, from one padded volume into the other (and a third in an accelerated run)."""

    rotates = True
    needs_padded_y = True

    def third(self):
        if "third" not in self._sides:
            self._sides["third"] = PaddedVolume(self.shape, self.pad_psf_shape, self.device)
        return self._sides["third"]

    def run(self, it0, n, x_out, rows, ab=None) -> None:
        rd, wr = ab or self.volumes()
        self.launch(self.y, int(self.from_y and it0 == 0), rd, wr, x_out, n, self.eps, rl_loop.row_ptr(rows, it0),
                    self.stream)


class _Fused(_Rotating):
    name = "fused"
    separable = True

    def __init__(self, shape, device, factors, norm):
        super().__init__(shape, [len(k) for k in factors], device)
        kz, ky, kx = (np.ascontiguousarray(k, dtype=np.float32) for k in factors)
        block = np.zeros(_lib.call_value("lsr_rl_sep_fused_taps_count"), np.float32)
        _lib.call("lsr_rl_sep_fused_prepare_taps", kz.ctypes.data, len(kz), ky.ctypes.data, len(ky),
                  kx.ctypes.data, len(kx), block.ctypes.data)
        self.taps, self.norm = _dev(block, device), norm

    def launch(self, y, from_y, rd, wr, x_out, n, eps, sp, stream) -> None:
        """Iteration i reads ``rd`` when i is even and ``wr`` when odd, and writes the other."""
        nz, ny, nx = self.norm
        _lib.call("lsr_rl_sep_fused_stats_f32", *y, from_y, rd.full.data_ptr(), wr.full.data_ptr(),
                  None if x_out is None else x_out.data_ptr(), *self.shape, self.taps.data_ptr(), *self.psf_shape,
                  nz.data_ptr(), ny.data_ptr(), nx.data_ptr(), n, eps, sp, stream)


class _FusedYsep(_Rotating):
    name = "y-separable (fused)"

    def __init__(self, shape, device, ky, kzx, norm_table, norm_full):
        super().__init__(shape, (kzx.shape[0], len(ky), kzx.shape[1]), device)
        ky_c, kzx_c = np.ascontiguousarray(ky, dtype=np.float32), np.ascontiguousarray(kzx, dtype=np.float32)
        block = np.zeros(_lib.call_value("lsr_rl_ysep_fused_taps_count"), np.float32)
        _lib.call("lsr_rl_ysep_fused_prepare_taps", ky_c.ctypes.data, len(ky_c), kzx_c.ctypes.data,
                  kzx_c.shape[0], kzx_c.shape[1], block.ctypes.data)
        self.taps, self.norm_table, self.norm_full = _dev(block, device), norm_table, norm_full

    def launch(self, y, from_y, rd, wr, x_out, n, eps, sp, stream) -> None:
        _lib.call("lsr_rl_ysep_fused_stats_f32", *y, from_y, rd.full.data_ptr(), wr.full.data_ptr(),
                  None if x_out is None else x_out.data_ptr(), *self.shape, self.taps.data_ptr(), *self.psf_shape,
                  self.norm_table.data_ptr(), ctypes.c_float(self.norm_full), n, eps, sp, stream)


class _SeparablePair(_Path):
    """The ratio / update pair of the tiled separable kernel."""

    name = "separable"
    separable = True

    def __init__(self, shape, device, factors, norm):
        super().__init__(shape, [len(k) for k in factors], device)
        self.k = tuple(_dev(k, device) for k in factors)
        self.k_flipped = tuple(_dev(k[::-1], device) for k in factors)
        self.norm = norm

    def run(self, it0, n, x_out, rows, ab=None) -> None:
        x_pad, ratio_pad = self.volumes()
        (kz, ky, kx), (fz, fy, fx) = self.k, self.k_flipped
        nz, ny, nx = self.norm
        pz, py, px = self.psf_shape
        _lib.call("lsr_rl_sep_stats_f32", *self.y, int(self.from_y and it0 == 0), x_pad.full.data_ptr(),
                  ratio_pad.full.data_ptr(), None if x_out is None else x_out.data_ptr(), *self.shape, kz.data_ptr(),
                  fz.data_ptr(), pz, ky.data_ptr(), fy.data_ptr(), py, kx.data_ptr(), fx.data_ptr(), px,
                  nz.data_ptr(), ny.data_ptr(), nx.data_ptr(), n, self.eps, rl_loop.row_ptr(rows, it0), self.stream)


class _LongZ(_SeparablePair):
    """A separable PSF with 17 .. 31 z taps: H x = Cz(Cyx(x)) -- the in-plane factors through the tiled separable kernel
    with a single z tap, the z factor through ``lsr_correlate_z_f32`` (a register march, no halo), which also carries
    the epilogues.  Four launches and 48 algorithmic bytes per voxel and iteration."""

    name = "separable (long z, 4 launches)"
    reads_y = False

    def __init__(self, shape, device, factors, norm):
        super().__init__(shape, device, factors, norm)
        # (the z extent is not the tiled kernels' business: they run with one z tap)
        self.pad_psf_shape = (1,) + self.psf_shape[1:]
        self.one = _dev(np.ones(1, np.float32), device)

    def run(self, it0, n, x_out, rows, ab=None) -> None:
        x_pad, ratio_pad = self.volumes()
        t = self.side("t")
        z, yy, xx = self.shape
        (kz, ky, kx), (fz, fy, fx) = self.k, self.k_flipped
        nz, ny, nx = self.norm
        pz, py, px = self.psf_shape
        x3, r3, t3, f0 = rl_loop.tri(x_pad), rl_loop.tri(ratio_pad), rl_loop.tri(t), ctypes.c_float(0.0)
        for it in range(it0, it0 + n):
            out3 = self._target(x_out if it + 1 == it0 + n else None)
            for src3, wy, wx, wz, epi, aux3, dst3 in ((x3, fy, fx, fz, _lib.EPI_RATIO, self.y, r3),
                                                      (r3, ky, kx, kz, _lib.EPI_UPDATE, x3, out3)):
                _lib.call("lsr_correlate_sep_strided_f32", *src3, None, 0, 0, *t3, z, yy, xx, self.one.data_ptr(), 1,
                          wy.data_ptr(), py, wx.data_ptr(), px, _lib.EPI_NONE, f0, None, None, None, self.stream)
                _lib.call("lsr_correlate_z_f32", *t3, *aux3, *dst3, z, yy, xx, wz.data_ptr(), pz, epi, self.eps,
                          nz.data_ptr(), ny.data_ptr(), nx.data_ptr(),
                          rl_loop.row_ptr(rows, it) if epi == _lib.EPI_UPDATE else None, self.stream)


class _Dense(_Path):
    """The tuned dense stencil (pz <= 11, py, px <= 9) on padded volumes."""

    name = "dense"

    def __init__(self, shape, device, w, taps):
        super().__init__(shape, w.shape, device)
        self.taps, self.taps_flipped = _dev(taps[0], device), _dev(taps[1], device)
        self.norm_table = _dev(_prefix_table(w).ravel(), device, np.float64)
        self.norm_full = float(w.astype(np.float64).sum())

    def run(self, it0, n, x_out, rows, ab=None) -> None:
        x_pad, ratio_pad = self.volumes()
        _lib.call("lsr_rl_dense_padded_stats_f32", *self.y, int(self.from_y and it0 == 0), x_pad.full.data_ptr(),
                  ratio_pad.full.data_ptr(), None if x_out is None else x_out.data_ptr(), *self.shape,
                  self.taps.data_ptr(), self.taps_flipped.data_ptr(), *self.psf_shape, self.norm_table.data_ptr(),
                  ctypes.c_float(self.norm_full), n, self.eps, rl_loop.row_ptr(rows, it0), self.stream)


class _Generic(_Path):
    """The bounds-checked dense stencil: dense volumes, x updated in place in the output tensor."""

    name = "generic"
    padded = reads_y = dense_out = False
    cur = None

    def __init__(self, shape, device, w):
        super().__init__(shape, w.shape, device)
        self.w, self.w_flipped = _dev(w.ravel(), device), _dev(w[::-1, ::-1, ::-1].ravel(), device)
        self.norm_table = _dev(_prefix_table(w).ravel(), device, np.float64)

    def volumes(self):
        return self.cur, self.side("ratio")

    def load(self, init, out) -> None:
        self.cur = out
        out.copy_(init)

    def run(self, it0, n, x_out, rows, ab=None) -> None:
        _lib.call("lsr_rl_dense_stats_f32", self.y[0], self.cur.data_ptr(), self.side("ratio").data_ptr(), *self.shape,
                  self.w.data_ptr(), self.w_flipped.data_ptr(), *self.psf_shape, self.norm_table.data_ptr(), n,
                  self.eps, rl_loop.row_ptr(rows, it0), self.stream)


class _YsepPair(_Path):
    """``psf = ky (x) kzx``: each correlation is the dense (z, x) stencil (PZ * PX FMAs per voxel instead of
    PZ * PY * PX) and the y pass that carries the epilogue -- ``H x = Y~(ZX~(x))`` with ``ratio = y / (. + eps)`` in the
    y pass; ``H^T r = Y(ZX(r))`` with the (z, x) border normalisation in the stencil launch (``LSR_EPI_SCALE``) and
    ``x * . / ny`` in the y pass.  Two launches per iteration where both factors fit one kernel
    (``lsr_correlate_zxy_padded_f32``: the y pass runs inside the stencil kernel, wave by wave, on the staged plane),
    otherwise four."""

    reads_y = False

    def __init__(self, shape, device, psf, ky, kzx, zx_taps, both):
        super().__init__(shape, psf.shape, device)
        self.name = "y-separable" if both is not None else "y-separable (4 launches)"
        self.both = both      # (taps, flipped taps, norm table, norm_full) of the two-launch form, or None
        self.ky, self.ky_flipped = _dev(ky, device), _dev(ky[::-1], device)
        if both is None:
            z, y, x = self.shape
            zx = np.ascontiguousarray(kzx[:, None, :])                     # a (pz, 1, px) PSF
            self.kzx = psf.astype(np.float64).sum(axis=1)                  # ky sums to 1: the (z, x) stencil
            self.taps, self.taps_flipped = _dev(zx_taps[0], device), _dev(zx_taps[1], device)
            self.norm_table = _dev(_prefix_table(zx).ravel(), device, np.float64)
            self.norm_full = float(zx.astype(np.float64).sum())
            self.one = _dev(np.ones(1, np.float32), device)
            self.ny = _dev(_axis_norm(ky, y), device)
            self.ones_z, self.ones_x = _dev(np.ones(z, np.float32), device), _dev(np.ones(x, np.float32), device)
            self._nzx = None

    def release(self) -> None:
        super().release()
        self._nzx = None

    def nzx(self):
        """(Z, X) table of the (z, x) stencil's border normalisation (sum of the kzx taps that land inside), float64 on
        the device -- only the four-launch form's flux needs it (its last launch divides by ny alone)."""
        import torch

        if self._nzx is None:
            z, _, x = self.shape
            pz, px = self.kzx.shape
            cs = np.zeros((pz + 1, px + 1))
            cs[1:, 1:] = self.kzx.cumsum(0).cumsum(1)
            zi, xi = np.arange(z), np.arange(x)
            a0, a1 = np.maximum(0, pz // 2 - zi), np.minimum(pz, z - zi + pz // 2)
            c0, c1 = np.maximum(0, px // 2 - xi), np.minimum(px, x - xi + px // 2)
            t = cs[a1][:, c1] - cs[a0][:, c1] - cs[a1][:, c0] + cs[a0][:, c0]
            self._nzx = torch.as_tensor(t, device=self.device)
        return self._nzx

    def run(self, it0, n, x_out, rows, ab=None) -> None:
        import torch

        x_pad, ratio_pad = self.volumes()
        z, yy, xx = self.shape
        pz, py, px = self.psf_shape
        x3, r3, eps, stream = rl_loop.tri(x_pad), rl_loop.tri(ratio_pad), self.eps, self.stream
        for it in range(it0, it0 + n):
            last = x_out if it + 1 == it0 + n else None
            out3, sp = self._target(last), rl_loop.row_ptr(rows, it)
            if self.both is not None:
                taps, taps_flipped, norm_table, norm_full = self.both
                _lib.call("lsr_correlate_zxy_padded_f32", *x3, *self.y, *r3, z, yy, xx, taps_flipped.data_ptr(),
                          self.ky_flipped.data_ptr(), pz, py, px, _lib.EPI_RATIO, eps, None, ctypes.c_float(1.0), stream)
                _lib.call("lsr_correlate_zxy_padded_stats_f32", *r3, *x3, *out3, z, yy, xx, taps.data_ptr(),
                          self.ky.data_ptr(), pz, py, px, _lib.EPI_UPDATE, eps, norm_table.data_ptr(),
                          ctypes.c_float(norm_full), sp, stream)
                continue
            if "t" not in self._sides:
                self._sides["t"] = PaddedVolume(self.shape, self.psf_shape, self.device)
            t3, one, f0 = rl_loop.tri(self._sides["t"]), self.one.data_ptr(), ctypes.c_float(0.0)
            _lib.call("lsr_correlate_dense_padded_f32", *x3, None, 0, 0, *t3, z, yy, xx, self.taps_flipped.data_ptr(),
                      pz, 1, px, _lib.EPI_NONE, f0, None, ctypes.c_float(1.0), stream)
            _lib.call("lsr_correlate_sep_strided_f32", *t3, *self.y, *r3, z, yy, xx, one, 1,
                      self.ky_flipped.data_ptr(), py, one, 1, _lib.EPI_RATIO, eps, None, None, None, stream)
            _lib.call("lsr_correlate_dense_padded_f32", *r3, None, 0, 0, *t3, z, yy, xx, self.taps.data_ptr(), pz, 1, px,
                      _lib.EPI_SCALE, f0, self.norm_table.data_ptr(), ctypes.c_float(self.norm_full), stream)
            _lib.call("lsr_correlate_sep_strided_stats_f32", *t3, *x3, *out3, z, yy, xx, one, 1, self.ky.data_ptr(), py,
                      one, 1, _lib.EPI_UPDATE, eps, self.ones_z.data_ptr(), self.ny.data_ptr(), self.ones_x.data_ptr(),
                      sp, stream)
            if rows is not None:
                # this launch's x * u is x * H^T(ratio) / nzx (the (z, x) normalisation went into the stencil launch): the
                # flux of the full update, sum x_new * nzx * ny, is formed here from the new estimate -- this path is the
                # fallback for y extents beyond the one-launch kernels, an extra reduction does not matter to it
                x_new = x_pad.view if last is None else last
                rows[it, 0] = (torch.einsum("zyx,y->zx", x_new, self.ny).double() * self.nzx()).sum()


class RichardsonLucyPlan:
    """PSF taps, border normalisation and scratch for one (volume shape, PSF, device).

    ``plan(y)`` runs ``iterations`` RL iterations and returns the estimate (a new tensor).
    """

    def __init__(self, shape_zyx, psf, device, *, separable: str = "auto",
                 separable_rtol: float = 1e-6, psf_factors=None, fused: str = "auto",
                 y_window: tuple[int, int] | None = None):
        """``y_window = (first_row, total_rows)``: this plan's volume is the row slab
        ``[first_row, first_row + shape_zyx[1])`` of a taller volume of ``total_rows`` rows; the
        border normalisation along y is then the taller volume's (``shrimpy_amd.slab``)."""
        import torch

        if fused not in ("auto", "never", "always"):
            raise ValueError("fused must be 'auto', 'never' or 'always'")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LsrError("RichardsonLucyPlan", -1,
                                f"device {self.device} is not a GPU: the plan owns padded DEVICE volumes; CPU tensors run the host "
                                "twins through richardson_lucy() / shrimpy_amd.host")
        self.shape = tuple(int(v) for v in shape_zyx)
        if len(self.shape) != 3 or min(self.shape) <= 0:
            raise ValueError(f"shape_zyx must be three positive ints, got {self.shape}")
        if separable not in ("auto", "force", "never"):
            raise ValueError("separable must be 'auto', 'force' or 'never'")

        factors = None
        if psf_factors is not None:
            factors = tuple(np.asarray(k, dtype=np.float32).ravel() for k in psf_factors)
            if (len(factors) != 3 or any(len(k) % 2 == 0 for k in factors) or len(factors[0]) > MAX_Z_TAPS
                    or max(len(factors[1]), len(factors[2])) > MAX_TAPS):
                raise ValueError("psf_factors must be three odd-length 1-D kernels (<= 31 taps along z, <= 15 in plane)")
            self.psf = (factors[0][:, None, None] * factors[1][None, :, None]
                        * factors[2][None, None, :]).astype(np.float32)
        else:
            self.psf = prepare_psf(psf)
            if separable != "never":
                factors = factor_psf(self.psf, separable_rtol)
                if factors is None and separable == "force":
                    raise ValueError("psf is not rank-1 within separable_rtol")
            if factors is None and self.psf.shape[0] > MAX_TAPS:
                raise ValueError(f"a PSF with {self.psf.shape[0]} z taps must be separable (kz x ky x kx within "
                                 f"separable_rtol): the dense and ky (x) kzx stencils hold <= {MAX_TAPS} taps per axis")
        self.psf_shape = tuple(int(v) for v in self.psf.shape) if factors is None else tuple(len(k) for k in factors)
        self._y_pad = None   # the paths that need a padded y: padded copy of a dense one
        self.last_stats = self.stats_device = self.last_alphas = None
        if factors is not None:
            self._path = self._separable_path(factors, fused, y_window)
        else:
            ysep = factor_psf_y(self.psf, separable_rtol) if separable == "auto" and y_window is None else None
            self._path = self._dense_path(ysep, fused)

    def _separable_path(self, factors, fused: str, y_window):
        z, y, x = self.shape
        kz, ky, kx = factors
        ny = _axis_norm(ky, y)
        if y_window is not None:
            first, total = (int(v) for v in y_window)
            if first < 0 or first + y > total:
                raise ValueError(f"y_window {y_window} does not contain {y} rows")
            ny = _axis_norm(ky, total)[first:first + y]
        norm = tuple(_dev(n, self.device) for n in (_axis_norm(kz, z), ny, _axis_norm(kx, x)))
        # an axial factor beyond the tiled kernels' 15 taps: every correlation = in-plane launch + z launch
        if len(kz) > MAX_TAPS:
            return _LongZ(self.shape, self.device, factors, norm)
        # one launch per iteration (rl_fused_sep.hip) where the PSF fits its specialisations
        if (fused in ("auto", "always") and _lib.call_value("lsr_rl_sep_fused_supported", *self.psf_shape)
                and (fused == "always" or fused_pays(*self.psf_shape))):
            return _Fused(self.shape, self.device, factors, norm)
        return _SeparablePair(self.shape, self.device, factors, norm)

    def _dense_path(self, ysep, fused: str):
        w, device = self.psf, self.device
        if ysep is not None and len(ysep[0]) <= MAX_TAPS:
            ky, kzx = ysep
            zx_taps = prepared_dense_taps(np.ascontiguousarray(kzx[:, None, :]))      # a (pz, 1, px) PSF
            if zx_taps is not None:                                        # pz <= 11, px <= 9
                emb = np.zeros(w.shape, np.float32)                        # kzx in the centre y row
                emb[:, w.shape[1] // 2, :] = kzx
                both_taps = prepared_dense_taps(emb)                       # also needs py <= 9
                both = None
                if both_taps is not None:
                    full = ky.astype(np.float64)[None, :, None] * kzx.astype(np.float64)[:, None, :]
                    both = (_dev(both_taps[0], device), _dev(both_taps[1], device),
                            _dev(_prefix_table(ky[None, :, None] * kzx[:, None, :]).ravel(), device, np.float64),
                            float(full.sum()))
                # ky (x) kzx with both factors inside the kernels' range: one launch per ITERATION (rl_fused_ysep.hip;
                # results bit-identical to the pair) -- since round 4 the faster form at every compiled extent (config-2
                # grid, ms per iteration, one launch / pair: 3x3x3 2.27 / 4.71, 5x5x5 2.82 / 4.57, 9x7x7 4.37 / 5.02,
                # 9x9x9 5.14 / 5.46, 11x9x9 6.19 / 6.95; profiles/r04_ysep_sweep.jsonl).  fused="never" keeps one launch
                # per correlation.
                if (both is not None and fused in ("auto", "always")
                        and _lib.call_value("lsr_rl_ysep_fused_supported", *self.psf_shape)):
                    return _FusedYsep(self.shape, device, ky, kzx, both[2], both[3])
                return _YsepPair(self.shape, device, w, ky, kzx, zx_taps, both)
        taps = prepared_dense_taps(w)
        if taps is not None:  # PSF small enough for the tuned dense kernel
            return _Dense(self.shape, device, w, taps)
        return _Generic(self.shape, device, w)

    @property
    def separable(self) -> bool:
        return self._path.separable

    @property
    def fused(self) -> bool:
        return isinstance(self._path, _Fused)

    @property
    def fused_ysep(self) -> bool:
        return isinstance(self._path, _FusedYsep)

    @property
    def padded_input(self) -> bool:
        """``plan(y)`` can take a zero-haloed :class:`PaddedVolume` written in place by the producer of ``y``."""
        return self._path.padded

    @property
    def path(self) -> str:
        """Which kernels an iteration runs: ``fused`` (one launch), ``separable`` (ratio / update
        pair), ``y-separable`` ((z, x) stencil + y pass, twice), ``dense`` or ``generic``."""
        return self._path.name

    def _scratch(self):
        """The two working volumes of the path."""
        return tuple(self._path.volumes())

    def padded_geometry(self):
        """(pitch, plane, rows, origin_row, origin_col) of this plan's padded working volumes."""
        rows, pitch, oy, ox = padded_shape(self.shape, self._path.pad_psf_shape)
        return pitch, rows * pitch, rows, oy, ox

    def new_padded_input(self) -> "PaddedVolume":
        """A zero-haloed volume in this plan's geometry, for a producer (the deskew kernel) to write
        ``y`` into; pass it to ``plan(...)`` to skip both the pad copy and the ``x0 = y`` copy."""
        return PaddedVolume(self.shape, self._path.pad_psf_shape, self.device)

    def iterate_padded(self, y_pad: "PaddedVolume", src: "PaddedVolume", dst: "PaddedVolume",
                       eps: float = 1e-6, stats=None) -> None:
        """One fused RL iteration between padded volumes of this plan's geometry: reads ``src``
        (and ``y_pad``), writes the logical window of ``dst``; no copies, no allocation.  The
        building block of the slab split (``shrimpy_amd.slab``), where halo rows are refreshed
        between iterations.  ``stats``: a float64 device tensor of 3 elements that receives this
        iteration's (flux, change, total) over THIS volume (a slab's share: sum over the slabs)."""
        import torch

        if not self.fused:
            raise _lib.LsrUnsupported("iterate_padded", _lib.E_UNSUPPORTED,
                                      "needs the fused separable path (PSF within its specialisations)")
        geo = self.padded_geometry()[:2]
        for v, name in ((y_pad, "y_pad"), (src, "src"), (dst, "dst")):
            if (v.pitch, v.plane) != geo or tuple(v.view.shape) != self.shape:
                raise ValueError(f"{name} does not have this plan's padded geometry")
        if src is dst:
            raise ValueError("src and dst must be different volumes")
        with torch.cuda.device(self.device):
            if stats is not None and (stats.dtype != torch.float64 or stats.numel() < 3 or stats.device != self.device):
                raise ValueError("stats must be a float64 tensor of >= 3 elements on the plan's device")
            self._path.launch(rl_loop.tri(y_pad), 0, src, dst, None, 1, ctypes.c_float(eps),
                              None if stats is None else stats.data_ptr(), _lib.stream_ptr(self.device))

    def release(self) -> None:
        """Drop the scratch volumes."""
        self._y_pad = None
        self._path.release()

    def __call__(self, y, iterations: int = 20, eps: float = 1e-6, x0=None, out=None, events=None, *,
                 stats: bool = False, tol: float | None = None, tv_lambda: float = 0.0, tv_eps: float = 1e-6,
                 acceleration: str = "none"):
        """Run RL.  ``events`` = optional ``(start, end)`` torch events recorded on the launch
        stream right around the kernel launches (``iterations`` fused launches, or
        ``2 * iterations`` ratio / update launches) -- what ``bench.py`` times.

        ``stats=True``: the kernels also sum the iteration's reduction scalars in their epilogues
        (:class:`RLStats`; read them afterwards from ``plan.last_stats`` -- the device tensor is
        ``plan.stats_device``, one row per iteration).  ``tol``: stop as soon as the relative change
        ``sum|x_new - x| / sum x_new`` of an iteration falls below it.  The scalars of iteration i are read back while
        iteration i + 1 runs, so the GPU never waits for the host; the estimate returned is therefore the one
        iteration past the first that met ``tol`` (``plan.last_stats.iterations`` says how many ran).

        ``tv_lambda`` in ``(0, 1/6)``: RL-TV -- one RL iteration at a time, each followed by the total-variation launch
        (``lsr_rl_tv_scale_f32``) on the same stream; ``change`` / ``total`` and ``tol`` then describe the regularised
        iterate (:class:`RLStats`).  ``0`` (default): the plain run, launch for launch.

        ``acceleration="biggs-andrews"``: one RL iteration at a time, each but the last followed by the two launches of
        ``csrc/rl_accel.hip`` on the same stream; the next iteration starts from the extrapolated point they leave.  The
        fused kinds rotate three padded volumes (no copy); the kinds that update x in place keep p_k and x_k in two dense
        volumes (two copies per iteration).  ``plan.last_alphas``: the step lengths used (float64, a_1 = 0 first).
        ``stats`` / ``tol`` keep the RL launch's meaning (:class:`RLStats`).  ``"none"`` (default): the plain run.

        The loop itself is ``shrimpy_amd.rl_loop.run``; the launches are the path's."""
        import torch

        path = self._path
        y_padded = None
        if isinstance(y, PaddedVolume):  # e.g. written in place by the deskew kernel
            if not path.padded:
                y = y.view.contiguous()
            else:
                y_padded, y = y, y.view
        else:
            y = _lib.require_device_f32(y, "y")
        if tuple(y.shape) != self.shape or y.device != self.device:
            raise ValueError(f"y must be {self.shape} on {self.device}, got {tuple(y.shape)} on {y.device}")
        if y_padded is not None and (y_padded.pitch, y_padded.plane) != self.padded_geometry()[:2]:
            raise ValueError("the padded y does not have this plan's padded geometry")
        req = rl_loop.check_run(y, iterations, eps, x0, out, stats, tol, tv_lambda, tv_eps, acceleration,
                                _lib.require_device_f32)
        if req.out is None:
            req.out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        self.last_stats = self.stats_device = self.last_alphas = None

        def begin():
            y_vol = y if y_padded is None else y_padded
            if path.needs_padded_y and y_padded is None:
                if self._y_pad is None:
                    self._y_pad = PaddedVolume(self.shape, path.pad_psf_shape, self.device)
                self._y_pad.view.copy_(y)
                y_vol = self._y_pad
            # x0 = y with a padded y needs no initial copy: the first iteration reads y directly
            from_y = path.reads_y and x0 is None and y_vol is not y
            path.begin(rl_loop.tri(y_vol), from_y, req.eps, _lib.stream_ptr(self.device))
            if not from_y:
                path.load(req.init, req.out)
            # x_0 as the first TV (dots) launch reads it: y itself (dense or padded) or the caller's x0 -- unless that is
            # also the output tensor, which the RL launches write; a path that rotates has it in the volume it reads
            if path.rotates:
                u0 = y_vol if from_y else None
            elif x0 is None:
                u0 = y_vol
            else:
                u0 = None if req.init.data_ptr() == req.out.data_ptr() else req.init
            return path, rl_loop.DeviceBackend(self.shape, self.device), u0, lambda: path.side("g")

        with torch.cuda.device(self.device):
            res = rl_loop.run(req, begin, events)
        self.last_stats, self.stats_device, self.last_alphas = res.stats, res.rows, res.alphas
        _lib.mark_written(res.x)
        return res.x


def make_plan(shape_zyx, psf, device, *, separable: str = "auto", separable_rtol: float = 1e-6, psf_factors=None,
              fused: str = "auto", method: str = "auto"):
    """The plan that runs RL for this volume shape and PSF on a HIP device.

    ``method="direct"``: the stencil kernels (:class:`RichardsonLucyPlan`; PSFs up to 15 taps per axis, 31 along z
    when separable).  ``"fft"``: the two convolutions of an iteration as products of spectra
    (:class:`shrimpy_amd.deconvolve_fft.FftRichardsonLucyPlan`; any PSF the transform grid holds).  ``"auto"``: the
    stencil kernels wherever a tuned one takes the PSF (three 1-D factors, ``ky (x) kzx``, dense up to 11 x 9 x 9);
    a dense PSF beyond them -- a measured bead PSF -- goes to the Fourier domain, where its size costs nothing
    (``profiles/r04_rl_fft.jsonl``), and only falls back to the bounds-checked generic stencil when the grid is
    outside the transform kernels' lengths."""
    if method not in ("auto", "direct", "fft"):
        raise ValueError("method must be 'auto', 'direct' or 'fft'")
    from .deconvolve_fft import MAX_FFT_TAPS, FftRichardsonLucyPlan, fft_supported

    def dense_psf():
        if psf_factors is not None:
            kz, ky, kx = (np.asarray(k, dtype=np.float32).ravel() for k in psf_factors)
            return (kz[:, None, None] * ky[None, :, None] * kx[None, None, :]).astype(np.float32)
        return prepare_psf(psf, MAX_FFT_TAPS, MAX_FFT_TAPS)

    if method == "fft":
        return FftRichardsonLucyPlan(shape_zyx, dense_psf(), device)
    direct, refused = None, None
    try:
        direct = RichardsonLucyPlan(shape_zyx, psf, device, separable=separable, separable_rtol=separable_rtol,
                                    psf_factors=psf_factors, fused=fused)
    except ValueError as exc:      # more taps than the stencil kernels hold
        if method == "direct" or psf_factors is not None or psf is None:
            raise
        refused = exc
    # (the tuned dense stencil costs one FMA per tap: at 11 x 9 x 9 = 891 taps it is the slower route -- 26.9 against
    # 23.1 ms per iteration on the config-2 grid, 15.2 against 23.0 ms at 9 x 7 x 7; profiles/r04_rl_fft.jsonl)
    if method == "direct" or (direct is not None and direct.path != "generic"
                              and not (direct.path == "dense" and int(np.prod(direct.psf.shape)) > 800)):
        return direct
    w = dense_psf()
    if fft_supported(shape_zyx, w.shape):
        return FftRichardsonLucyPlan(shape_zyx, w, device)
    if direct is None:
        raise refused
    return direct


def richardson_lucy(y, psf=None, iterations: int = 20, eps: float = 1e-6, x0=None, *,
                    separable: str = "auto", separable_rtol: float = 1e-6, psf_factors=None,
                    tol: float | None = None, return_stats: bool = False, method: str = "auto",
                    tv_lambda: float = 0.0, tv_eps: float = 1e-6, acceleration: str = "none"):
    """Richardson-Lucy deconvolution of a (Z, Y, X) float32 device tensor; returns a new tensor.

    ``psf`` is used as given (normalise it to sum 1 for flux conservation).  ``x0`` defaults to
    ``y``.  ``separable="auto"`` takes the rank-1 fast path when the PSF factorises within
    ``separable_rtol``; pass ``psf_factors=(kz, ky, kx)`` to skip the test.

    ``method``: ``"auto"`` (default) runs the stencil kernels where a tuned one takes the PSF and the Fourier-domain
    iteration for dense PSFs beyond them (:func:`make_plan`); ``"direct"`` / ``"fft"`` insist on one.  CPU tensors
    always run the host twins of the stencil arithmetic.

    ``tol``: stop before ``iterations`` once an iteration's relative change ``sum|x_new - x| / sum x_new`` is below
    it (the kernels sum both in their epilogues; see :class:`RLStats`).  ``return_stats=True`` returns
    ``(estimate, RLStats)`` -- flux, change and total per iteration that ran.

    ``tv_lambda`` in ``[0, 1/6)``: total-variation regularisation (RL-TV, Dey et al. 2006): every iteration's result is
    divided by ``1 - tv_lambda * div(grad x / |grad x|)`` with the gradient norm floored by ``tv_eps``; typical values
    are 0.001 .. 0.05.  ``0`` (default) is plain RL.

    ``acceleration="biggs-andrews"``: the vector extrapolation of Biggs & Andrews (1997) -- every iteration starts from a
    point extrapolated along the last change, with a step length taken from the last two changes; about 10 iterations
    reach the likelihood of 20 plain ones.  A different path up the same likelihood, not the plain run's numbers; not
    together with ``tv_lambda > 0``.  With ``return_stats=True`` the step lengths are ``RLStats.alphas``.
    """
    import torch

    tv_lambda, tv_eps = check_tv(tv_lambda, tv_eps)
    tv = dict(tv_lambda=tv_lambda, tv_eps=tv_eps) if tv_lambda > 0 else {}
    if check_acceleration(acceleration, tv_lambda):
        tv["acceleration"] = acceleration

    if not isinstance(y, torch.Tensor):
        raise TypeError(f"y must be a torch.Tensor, got {type(y).__name__}")
    if y.dim() != 3:
        raise ValueError(f"y must be (Z, Y, X), got shape {tuple(y.shape)}")
    if y.dtype != torch.float32:
        y = y.to(torch.float32)
    y = y.contiguous()
    if y.device.type == "cpu":     # no HIP device in play: the host twins of the two launches per iteration
        from . import host

        return host.richardson_lucy(y, psf, iterations, eps, x0, separable=separable, separable_rtol=separable_rtol,
                                    psf_factors=psf_factors, tol=tol, return_stats=return_stats, **tv)
    plan = make_plan(tuple(y.shape), psf, y.device, separable=separable, separable_rtol=separable_rtol,
                     psf_factors=psf_factors, method=method)
    x = plan(y, iterations=iterations, eps=eps, x0=x0, stats=return_stats, tol=tol, **tv)
    if return_stats and plan.last_alphas is not None:
        plan.last_stats.alphas = plan.last_alphas
    return (x, plan.last_stats) if return_stats else x


def correlate3d(volume, weights=None, *, weight_factors=None, tuned: bool = True):
    """``scipy.ndimage.correlate(volume, weights, mode="constant", cval=0)`` on the device.

    Pass ``weight_factors=(wz, wy, wx)`` for the separable kernel.  ``tuned=False`` forces the
    generic bounds-checked dense kernel (any size up to 15 taps per axis).  (The un-fused building
    block of the RL launches; also used for PSF-blurring synthetic scenes.)
    """
    import torch

    if isinstance(volume, torch.Tensor) and volume.device.type == "cpu":
        from . import host

        return host.correlate3d(volume, weights, weight_factors)
    vol = _lib.require_device_f32(volume, "volume")
    if vol.dim() != 3:
        raise ValueError("volume must be (Z, Y, X)")
    out = torch.empty_like(vol)
    z, y, x = (int(v) for v in vol.shape)

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=vol.device)

    with torch.cuda.device(vol.device):
        stream = _lib.stream_ptr(vol.device)
        if weight_factors is not None:
            wz, wy, wx = (np.asarray(k, dtype=np.float32).ravel() for k in weight_factors)
            dz, dy, dx = dev(wz), dev(wy), dev(wx)
            pad = PaddedVolume(vol.shape, (len(wz), len(wy), len(wx)), vol.device)
            pad.view.copy_(vol)
            _lib.call(
                "lsr_correlate_sep_strided_f32", pad.logical_ptr(), pad.pitch, pad.plane, None, 0, 0,
                out.data_ptr(), x, y * x, z, y, x, dz.data_ptr(), len(wz), dy.data_ptr(), len(wy),
                dx.data_ptr(), len(wx), _lib.EPI_NONE, ctypes.c_float(0.0), None, None, None, stream,
            )
        else:
            w = prepare_psf(weights)
            taps = prepared_dense_taps(w) if tuned else None
            if taps is not None:
                dt = dev(taps[0])
                pad = PaddedVolume(vol.shape, w.shape, vol.device)
                pad.view.copy_(vol)
                _lib.call(
                    "lsr_correlate_dense_padded_f32", pad.logical_ptr(), pad.pitch, pad.plane, None, 0, 0,
                    out.data_ptr(), x, y * x, z, y, x, dt.data_ptr(), w.shape[0], w.shape[1], w.shape[2],
                    _lib.EPI_NONE, ctypes.c_float(0.0), None, ctypes.c_float(1.0), stream,
                )
            else:
                dw = dev(w.ravel())
                _lib.call(
                    "lsr_correlate_dense_f32", vol.data_ptr(), out.data_ptr(), None, z, y, x,
                    dw.data_ptr(), w.shape[0], w.shape[1], w.shape[2], _lib.EPI_NONE,
                    ctypes.c_float(0.0), None, stream,
                )
        # the tap tensors must outlive the launch: the caching allocator keeps their blocks on
        # this stream, so reuse after free is stream-ordered
    return out
