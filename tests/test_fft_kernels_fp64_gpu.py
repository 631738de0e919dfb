"""The LDS-resident FFT kernels (``csrc/rfft_rows.hip``, ``csrc/zcorr.hip`` over the Stockham passes of
``csrc/fft_lds.hpp``) against float64 restatements of their contracts (``oracle/cpu_ref.py``: ``rows_rfft_t``,
``rows_irfft_t``, ``z_leg``, ``rl_norm_direct``), called through the C entries directly -- no rocFFT between the
kernel and the reference, and no need for hipFFT's C API.

Every length the kernels accept is swept: each has its own radix sequence, butterflies per thread and ``r / s``
division by float reciprocal.  Inputs are zero-mean (standard normal rows, random Hermitian spectra) plus structured
rows that isolate pairing and twiddle errors (impulses at 0, 1 and n - 1, tones at bins 0, 1, M / 2, M - 1, M).  Each
transformed row or column is held to

    ||got - ref||_2            <= C_L2  * u * log2(n) * ||ref||_2
    max_k |got_k - ref_k|      <= C_MAX * u * log2(n) * rms(ref)          u = 2^-24

(``||ref||_2 = sqrt(n) ||x||_2`` by Parseval: the usual FFT bound, scaled to the output).  The constants are four
times the worst ratio observed over all lengths on an MI355X, at most (recorded beside each constant).  Buffers are
filled with NaN first, so a coefficient that is not written, or a plane that must stay untouched, shows.  The whole
file takes a few seconds on one card.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import cpu_ref as o
from shrimpy_amd import _lib
from shrimpy_amd.deconvolve import _prefix_table

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24

# Bounds in units of u * log2(n); worst observed ratio over every accepted length in the comments.
C_L2_ROWS, C_MAX_ROWS = 2.5, 32.0        # x leg, forward and inverse: worst 0.655 (X = 20), 8.30 (X = 1152)
C_L2_Z, C_MAX_Z = 5.0, 6.5               # z leg, the two transforms and the product: worst 1.36 (N = 2), 1.75 (N = 2)
C_EPI_UPDATE = 1e-6                      # RL epilogues, of the row's largest |expected|: worst 2.5e-7
C_EPI_RATIO = 3e-6                       # worst 8.1e-7

# the worst ratio seen per family in this process (read back when the constants above are re-measured)
WORST: dict = {}


def _smooth(n):
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


ROW_X = [x for x in range(8, 4097, 4) if _smooth(x // 2)]     # the rule lsr_rfft_rows_supported states
Z_N = [n for n in range(2, 257) if _smooth(n)]                 # ... and lsr_cross_correlate_z_supported


@pytest.fixture(autouse=True)
def _hermetic(monkeypatch):
    monkeypatch.delenv("LSR_ZCORR_ORDER", raising=False)
    monkeypatch.delenv("LSR_FFT_RL_CHAIN", raising=False)


def _stream():
    return _lib.stream_ptr(DEV)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _row_tables(x):
    """The entry's documented twiddles: exp(-2 pi i k / (X/2)), k < X/4, and exp(-2 pi i k / X), k <= X/2."""
    m = x // 2
    half = np.exp(-2j * np.pi * np.arange(m // 2) / m).astype(np.complex64)
    full = np.exp(-2j * np.pi * np.arange(m + 1) / x).astype(np.complex64)
    return _dev(half), _dev(full)


def _record(family, value):
    WORST[family] = max(WORST.get(family, 0.0), float(value))


def _check_rows(family, got, want, n, c_l2, c_max, scale=None):
    """Bound every row (last axis) of ``got`` against float64 ``want``, relative to ``||want||_2`` per row or to the given
    per-row ``scale``; all-zero reference rows must come out zero."""
    got = np.asarray(got).astype(np.complex128)
    want = np.asarray(want).astype(np.complex128)
    assert np.isfinite(got).all(), f"{family}: non-finite output (an unwritten coefficient?)"
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    ref_norm = np.linalg.norm(want, axis=1)
    norm = ref_norm if scale is None else np.asarray(scale, np.float64).reshape(-1)
    live = ref_norm > 0
    assert np.array_equal(got[~live], np.zeros_like(got[~live])), f"{family}: a zero row is not zero"
    err = np.abs(got[live] - want[live])
    unit = U * math.log2(n) * norm[live]
    l2 = np.linalg.norm(err, axis=1) / unit
    mx = err.max(axis=1) / (unit / math.sqrt(want.shape[1]))
    _record(family + " l2", l2.max())
    _record(family + " max", mx.max())
    assert l2.max() <= c_l2, f"{family}: ||err||_2 = {l2.max():.3g} u log2(n) ||ref||_2 (row {int(np.argmax(l2))})"
    assert mx.max() <= c_max, f"{family}: max|err| = {mx.max():.3g} u log2(n) rms(ref) (row {int(np.argmax(mx))})"


def _row_inputs(x_len, width, rows, rng):
    """``rows`` float32 rows of ``width`` samples: impulses at 0, 1, width - 1, tones (period ``x_len``) at bins
    0, 1, M/2, M-1, M (cos) and 1, M-1 (sin), real parts of random Hermitian spectra, then standard normal rows."""
    m = x_len // 2
    n = np.arange(width)
    s = [np.eye(1, width, k)[0] for k in (0, 1, width - 1)]
    s += [np.cos(2 * np.pi * b * n / x_len) for b in (0, 1, m // 2, m - 1, m)]
    s += [np.sin(2 * np.pi * b * n / x_len) for b in (1, m - 1)]
    out = rng.standard_normal((rows, width))
    herm = np.fft.irfft(rng.standard_normal((2, m + 1)) + 1j * rng.standard_normal((2, m + 1)), n=x_len)[:, :width]
    out[: len(s)] = s
    out[len(s): len(s) + 2] = herm * math.sqrt(x_len)
    return out.astype(np.float32)


def _hermitian(shape_zyx, rng):
    """A random spectrum of a real (Z, Y, X) grid in the ``[Z][XC][Y]`` layout, complex64, DC and Nyquist real."""
    z, y, x = shape_zyx
    s = rng.standard_normal((z, y, x // 2 + 1)) + 1j * rng.standard_normal((z, y, x // 2 + 1))
    s[..., 0] = s[..., 0].real
    s[..., -1] = s[..., -1].real
    return np.ascontiguousarray(s.astype(np.complex64).transpose(0, 2, 1))


def _unit_psf():
    """pz = py = px = 1, one tap of weight 1: H^T 1 = 1 everywhere, so the UPDATE epilogue with aux = 1 stores v."""
    return _dev(_prefix_table(np.ones((1, 1, 1), np.float32)).ravel())


def test_the_sweep_covers_every_length_the_kernels_accept():
    assert len(ROW_X) == 86 and len(Z_N) == 51
    assert [x for x in range(0, 4200) if _lib.call_value("lsr_rfft_rows_supported", x)] == ROW_X
    assert [n for n in range(0, 300) if _lib.call_value("lsr_cross_correlate_z_supported", n)] == Z_N


# ---------------------------------------------------------------- x leg, forward and inverse, every length


@pytest.mark.parametrize("x_len", ROW_X)
def test_forward_row_leg_every_length(x_len):
    """``lsr_rfft_rows_t_c64`` (source = grid) and ``lsr_rfft_rows_zero_t_c64`` (source (2, 13, X - 1) in a (3, 17, X)
    grid: an odd last pair, padding rows inside a source tile and a tile of pure padding, a plane behind the source)."""
    rng = np.random.default_rng(x_len)
    half, full = _row_tables(x_len)
    xc = x_len // 2 + 1
    z, y = 2, 17                                                          # 17: ragged against the 8-row tiles
    src = _row_inputs(x_len, x_len, z * y, rng).reshape(z, y, x_len)
    spec, src_d = _nan((z, xc, y), torch.complex64), _dev(src)
    _lib.call("lsr_rfft_rows_t_c64", src_d.data_ptr(), z, y, x_len, spec.data_ptr(), z, y, x_len, half.data_ptr(),
              full.data_ptr(), _stream())
    want = o.rows_rfft_t(src, (z, y, x_len))
    _check_rows("rows forward", spec.cpu().numpy().transpose(0, 2, 1), want.transpose(0, 2, 1), x_len, C_L2_ROWS,
                C_MAX_ROWS)

    zi, yi, xi, gz = 2, 13, x_len - 1, 3
    src0 = _row_inputs(x_len, xi, zi * yi, rng).reshape(zi, yi, xi)
    spec0, src0_d = _nan((gz, xc, y), torch.complex64), _dev(src0)
    _lib.call("lsr_rfft_rows_zero_t_c64", src0_d.data_ptr(), zi, yi, xi, spec0.data_ptr(), gz, y, x_len,
              half.data_ptr(), full.data_ptr(), _stream())
    got0 = spec0.cpu().numpy()
    assert np.isnan(got0[zi:]).all(), "a plane behind the source was written"
    assert np.array_equal(got0[:zi, :, yi:], np.zeros_like(got0[:zi, :, yi:])), "padding rows beside the source"
    want0 = o.rows_rfft_t(src0, (gz, y, x_len), zero=True)
    _check_rows("rows forward zero", got0[:zi, :, :yi].transpose(0, 2, 1), want0[:zi, :, :yi].transpose(0, 2, 1), x_len,
                C_L2_ROWS, C_MAX_ROWS)


@pytest.mark.parametrize("x_len", ROW_X)
def test_inverse_row_leg_every_length(x_len):
    """The inverse x leg alone: ``lsr_irfft_rows_rl_f32``'s UPDATE epilogue with a one-tap PSF, aux = 1 and scale = 1
    stores v = X * irfft(spec) itself.  Spectra of the structured rows, and random Hermitian spectra."""
    rng = np.random.default_rng(1000 + x_len)
    half, full = _row_tables(x_len)
    z, y = 2, 17
    spec = _hermitian((z, y, x_len), rng)                                # plane 1: random Hermitian spectra
    sr = np.fft.rfft(_row_inputs(x_len, x_len, y, rng).astype(np.float64), axis=-1).astype(np.complex64)
    sr[:, 0] = sr[:, 0].real
    sr[:, -1] = sr[:, -1].real
    spec[0] = sr.T                                                        # plane 0: spectra of the structured rows
    aux = torch.ones((z, y, x_len), dtype=torch.float32, device=DEV)
    out, spec_d, unit = _nan((z, y, x_len), torch.float32), _dev(spec), _unit_psf()
    _lib.call("lsr_irfft_rows_rl_f32", spec_d.data_ptr(), z, y, x_len, half.data_ptr(), full.data_ptr(),
              _lib.EPI_UPDATE, aux.data_ptr(), out.data_ptr(), z, y, x_len, 1.0, 1e-6, 1, 1, 1, unit.data_ptr(), 1.0,
              None, _stream())
    _check_rows("rows inverse", out.cpu().numpy(), o.rows_irfft_t(spec, x_len), x_len, C_L2_ROWS, C_MAX_ROWS)


@pytest.mark.parametrize("x_len", ROW_X)
def test_chained_rl_rows_leave_the_forward_legs_spectrum(x_len):
    """``lsr_rl_rows_chain_f32`` (RATIO and UPDATE with stats) stores the same ``out`` as the unchained
    ``lsr_irfft_rows_rl_f32`` and leaves ``spec`` bit-identical to ``lsr_rfft_rows_zero_t_c64(out)``; planes behind the
    volume keep what they held."""
    rng = np.random.default_rng(2000 + x_len)
    half, full = _row_tables(x_len)
    gz, gy, xc = 3, 17, x_len // 2 + 1
    zo, yo, xo = 2, 13, x_len - 3
    spec_in = _dev(_hermitian((gz, gy, x_len), rng))
    psf = rng.uniform(0.2, 1.0, (3, 3, 5)).astype(np.float32)
    psf /= psf.sum()
    table = _dev(_prefix_table(psf).ravel())
    norm_full = float(psf.astype(np.float64).sum())
    scale = 1.0 / (gz * gy * x_len)
    for epi in (_lib.EPI_RATIO, _lib.EPI_UPDATE):
        aux = _dev(rng.uniform(0.5, 2.0, (zo, yo, xo)).astype(np.float32))
        stats = torch.zeros(3, dtype=torch.float64, device=DEV) if epi == _lib.EPI_UPDATE else None
        args = (epi, aux.data_ptr())
        tail = (zo, yo, xo, scale, 1e-3, 3, 3, 5, table.data_ptr(), norm_full)
        plain = _nan((zo, yo, xo), torch.float32)
        _lib.call("lsr_irfft_rows_rl_f32", spec_in.data_ptr(), gz, gy, x_len, half.data_ptr(), full.data_ptr(), *args,
                  plain.data_ptr(), *tail, None, _stream())
        chained_spec = spec_in.clone()
        out = _nan((zo, yo, xo), torch.float32)
        _lib.call("lsr_rl_rows_chain_f32", chained_spec.data_ptr(), gz, gy, x_len, half.data_ptr(), full.data_ptr(),
                  *args, out.data_ptr(), *tail, None if stats is None else stats.data_ptr(), _stream())
        assert torch.equal(out, plain), f"epilogue {epi}: the chained kernel's out differs from the unchained one"
        fresh = _nan((gz, xc, gy), torch.complex64)
        _lib.call("lsr_rfft_rows_zero_t_c64", out.data_ptr(), zo, yo, xo, fresh.data_ptr(), gz, gy, x_len, half.data_ptr(),
                  full.data_ptr(), _stream())
        assert torch.equal(chained_spec[:zo], fresh[:zo]), f"epilogue {epi}: spec is not the forward leg of out"
        assert torch.equal(chained_spec[zo:], spec_in[zo:]), f"epilogue {epi}: a plane behind the volume was written"


@pytest.mark.parametrize("src_shape,grid", [((5, 20, 37), (8, 17, 48)), ((11, 6, 101), (9, 9, 80)),
                                            ((2, 9, 5), (3, 9, 8)), ((3, 30, 251), (4, 25, 240)),
                                            ((7, 4, 1500), (6, 7, 1536)), ((2, 3, 2270), (3, 4, 2304))])
def test_forward_row_leg_reflect_pad_and_crop_map(src_shape, grid):
    """``lsr_rfft_rows_t_c64`` from sources larger than the grid on some axes and smaller on others, by odd and even
    differences: the transform of ``dt_match_shape(src, grid)``."""
    rng = np.random.default_rng(sum(src_shape))
    z, y, x = grid
    half, full = _row_tables(x)
    src = rng.standard_normal(src_shape).astype(np.float32)
    spec, src_d = _nan((z, x // 2 + 1, y), torch.complex64), _dev(src)
    _lib.call("lsr_rfft_rows_t_c64", src_d.data_ptr(), *src_shape, spec.data_ptr(), z, y, x, half.data_ptr(),
              full.data_ptr(), _stream())
    _check_rows("rows forward pad/crop", spec.cpu().numpy().transpose(0, 2, 1), o.rows_rfft_t(src, grid).transpose(0, 2, 1),
                x, C_L2_ROWS, C_MAX_ROWS)


# ---------------------------------------------------------------- z leg, every length, three modes


@pytest.mark.parametrize("n", Z_N)
def test_z_leg_every_length_and_mode(n):
    """``lsr_cross_correlate_z_c64`` (mode 0) and ``lsr_spectrum_multiply_z_c64`` (conj_f1 = 0, 1) on 2 x 17 columns
    (17: ragged against the 16-column tiles), whole and with z_valid / z_keep: planes at or beyond z_valid hold NaN
    (never read), planes at or beyond z_keep keep their bits.

    The scale of a column is ``N max|f1| ||g||_2`` (what bounds ``||ref||_2`` by Parseval), not ``||ref||_2``: a tone in g
    meets one bin of f1, and where that bin is small the reference is small while the rounding of the other bins is
    not (N = 24: the tone at bin 1 meets |f1| = 0.8 % of its column's largest)."""
    rng = np.random.default_rng(n)
    xc, y = 2, 17
    tw = _dev(np.exp(-2j * np.pi * np.arange(n) / n).astype(np.complex64))
    f1 = (rng.standard_normal((xc, y, n)) + 1j * rng.standard_normal((xc, y, n))).astype(np.complex64)
    g = (rng.standard_normal((n, xc, y)) + 1j * rng.standard_normal((n, xc, y))).astype(np.complex64)
    k = np.arange(n)
    cols = [np.eye(1, n, j)[0] for j in (0, 1, n - 1)] + [np.exp(2j * np.pi * b * k / n) for b in (0, 1, n // 2, n - 1)]
    for i, c in enumerate(cols):
        g[:, i // y, i % y] = c
    f1_d = _dev(f1)
    for mode in (0, 1, 2):
        spans = [(n, n)] if mode == 0 else [(n, n), (max(1, (2 * n) // 3), max(1, n // 2 + 1)), (1, n)]
        for z_valid, z_keep in spans:
            gin = g.copy()
            gin[z_valid:] = np.nan
            gd = _dev(gin)
            if mode == 0:
                _lib.call("lsr_cross_correlate_z_c64", f1_d.data_ptr(), gd.data_ptr(), tw.data_ptr(), n, y, xc, _stream())
            else:
                _lib.call("lsr_spectrum_multiply_z_c64", f1_d.data_ptr(), gd.data_ptr(), tw.data_ptr(), n, y, xc, mode - 1,
                          z_valid, z_keep, _stream())
            got = gd.cpu().numpy()
            assert np.array_equal(got[z_keep:], gin[z_keep:], equal_nan=True), f"mode {mode}: a plane >= z_keep changed"
            want = o.z_leg(f1, gin, mode, z_valid, z_keep)
            gv = np.where(np.isnan(gin), 0, gin)[:z_valid]
            scale = n * np.abs(f1).max(axis=2) * np.linalg.norm(gv, axis=0)          # [XC][Y]
            # columns along the last axis: [XC][Y][z]
            _check_rows(f"z leg mode {mode}", got[:z_keep].transpose(1, 2, 0), want.transpose(1, 2, 0), n, C_L2_Z, C_MAX_Z,
                        scale)


# ---------------------------------------------------------------- peak of the inverse leg


PEAK_GRIDS = [(9, 15, 12), (15, 9, 20), (8, 16, 16), (45, 75, 24), (75, 45, 40)]


def _wrap_positions(n):
    return sorted({0, n // 2, n // 2 - 1, (n // 2 + 1) % n, n - 1})


@pytest.mark.parametrize("grid", PEAK_GRIDS)
def test_inverse_row_leg_peak_in_fftshift_order(grid):
    """``lsr_irfft_rows_peak``: the flat index of argmax(fftshift(|corr|)) of the float64 inverse, for one planted
    maximum at the wrap positions 0, n//2, n//2 +- 1, n - 1 of every axis (all combinations on the small grids)."""
    z, y, x = grid
    half, full = _row_tables(x)
    rng = np.random.default_rng(z * y * x)
    pz, py, px = (_wrap_positions(v) for v in grid)
    if z * y * x <= 4096:
        positions = [(a, b, c) for a in pz for b in py for c in px]
    else:
        positions = [(a, py[(i + 1) % len(py)], px[(i + 2) % len(px)]) for i, a in enumerate(pz)]
        positions += [(pz[(i + 2) % len(pz)], b, px[i % len(px)]) for i, b in enumerate(py)]
    nb = z * -(-y // 8)
    scratch = torch.empty((nb * 16,), dtype=torch.uint8, device=DEV)        # as fft3.correlation_peak allocates it
    lib = _lib.load()
    lib.lsr_rfft_rows_scratch_bytes.restype = ctypes.c_int64
    assert lib.lsr_rfft_rows_scratch_bytes(z, y) == scratch.numel()
    peaks = torch.empty((len(positions),), dtype=torch.int64, device=DEV)
    want, specs = [], []
    for i, pos in enumerate(positions):
        c = 0.1 * rng.standard_normal(grid)
        c[pos] = 10.0 * rng.choice((-1.0, 1.0))
        spec = np.ascontiguousarray(np.fft.rfft(c, axis=-1).astype(np.complex64).transpose(0, 2, 1))
        corr = o.rows_irfft_t(spec, x)
        flat = int(np.argmax(np.fft.fftshift(np.abs(corr))))
        assert flat == np.ravel_multi_index(tuple((p + s // 2) % s for p, s in zip(pos, grid)), grid)
        want.append(flat)
        specs.append(_dev(spec))                                          # alive until the launches have run
        _lib.call("lsr_irfft_rows_peak", specs[-1].data_ptr(), z, y, x, half.data_ptr(), full.data_ptr(),
                  peaks[i:].data_ptr(), scratch.data_ptr(), _stream())
    got = peaks.cpu().numpy().tolist()
    bad = [(positions[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} peaks misplaced, e.g. (planted, got, want) {bad[:3]}"


# ---------------------------------------------------------------- RL epilogues without FFT error


def _grid_x(n):
    return next(x for x in ROW_X if x >= n + 1)


EPI_CASES = [((1, 1, 1), (2, 9, 37)), ((3, 5, 3), (4, 11, 5)),
             ((3, 3, 63), (4, 9, 25)), ((5, 3, 63), (6, 10, 45)), ((1, 5, 63), (3, 12, 201)),
             ((3, 1, 65), (4, 9, 61)),
             ((3, 3, 127), (4, 9, 31)), ((7, 3, 127), (8, 11, 125)), ((3, 5, 127), (3, 10, 391)),
             ((3, 3, 129), (4, 9, 63)), ((5, 1, 129), (6, 9, 127)), ((1, 3, 129), (3, 17, 1001))]


@pytest.mark.parametrize("psf_shape,vol", EPI_CASES)
def test_rl_epilogues_against_float64(psf_shape, vol):
    """``lsr_irfft_rows_rl_f32`` fed the float64 x-leg spectrum of a known positive volume v (so the only float32
    transform is the inverse row leg the sweep checks): UPDATE out = aux v / H^T 1 with H^T 1 summed tap by tap
    (``rl_norm_direct``, not the prefix table the kernel reads), with and without the iteration's sums; RATIO out =
    aux / (v + eps).  PSFs up to 129 taps along x, volumes narrower than one and than two PSF radii (the left and right
    borders overlap), interior and border rows."""
    zo, yo, xo = vol
    rng = np.random.default_rng(xo * 7 + psf_shape[2])
    grid = (zo + 1, yo + 3, _grid_x(xo))
    gz, gy, gx = grid
    half, full = _row_tables(gx)
    psf = rng.uniform(0.2, 1.0, psf_shape).astype(np.float32)
    psf /= psf.sum()
    table = _dev(_prefix_table(psf).ravel())
    norm_full = float(psf.astype(np.float64).sum())
    v = np.zeros(grid)
    v[:zo, :yo, :xo] = rng.uniform(0.5, 2.0, vol)
    spec = _dev(np.ascontiguousarray(np.fft.rfft(v, axis=-1).astype(np.complex64).transpose(0, 2, 1)))
    aux = rng.uniform(0.5, 2.0, vol).astype(np.float32)
    aux_d = _dev(aux)
    v = v[:zo, :yo, :xo]
    a64 = aux.astype(np.float64)
    ht1 = o.rl_norm_direct(vol, psf.astype(np.float64))
    eps = 1e-3

    def run(epi, stats=None):
        out = _nan(vol, torch.float32)
        _lib.call("lsr_irfft_rows_rl_f32", spec.data_ptr(), gz, gy, gx, half.data_ptr(), full.data_ptr(), epi,
                  aux_d.data_ptr(), out.data_ptr(), zo, yo, xo, 1.0 / gx, eps, *psf_shape, table.data_ptr(), norm_full,
                  None if stats is None else stats.data_ptr(), _stream())
        return out

    def check(name, got, want, bound):
        got = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), f"{name}: a voxel was not written"
        err = np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)
        _record(name, err.max())
        z, yy = np.unravel_index(int(np.argmax(err)), err.shape)
        x = int(np.argmax(np.abs(got[z, yy] - want[z, yy])))
        assert err.max() <= bound, f"{name}: {err.max():.3g} of the row's max at (z, y, x) = ({z}, {yy}, {x})"

    want_u = a64 * v / ht1
    out_u = run(_lib.EPI_UPDATE)
    check("epilogue update", out_u, want_u, C_EPI_UPDATE)
    stats = torch.zeros(3, dtype=torch.float64, device=DEV)
    out_s = run(_lib.EPI_UPDATE, stats)
    assert torch.equal(out_s, out_u), "the stats variant stores different values"
    flux, change, total = stats.cpu().numpy()
    np.testing.assert_allclose([flux, change, total], [(a64 * v).sum(), np.abs(want_u - a64).sum(), want_u.sum()],
                               rtol=1e-5)
    check("epilogue ratio", run(_lib.EPI_RATIO), a64 / (v + np.float64(np.float32(eps))), C_EPI_RATIO)
