"""The flat-field on the host: the restated rule (``tests/flatfield_ref.py``) against ``torch.quantile`` bit for bit, the twins
``lsr_flatfield_pattern_*_cpu`` / ``lsr_flatfield_apply_*_cpu`` against the restatement on every case (zeros and denormals included),
the twin's mean against an ``fsum`` inside an a-priori bound, and a census: every class of column, every ``Z``, every fallback position
and every bin parity the cases aim at is present, computed from the definitions and never from the library.

Cases: ``tests/flatfield_cases.py``, sized from the exported tiling.
"""

import functools

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import flatfield as F
from tests import flatfield_cases as C
from tests import flatfield_ref as R


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))                # (a copy: the shared cases are read-only)


@functools.lru_cache(maxsize=None)
def case_twin(name, u16=False):
    """``(pattern, mean)`` of the twin on a case, computed once (read-only; tests/test_flatfield_gpu.py holds the device to it)."""
    ff = F.flat_field_pattern(_t(C.volume_u16(name) if u16 else C.volume(name)))
    pattern, mean = ff.pattern.numpy(), ff.mean.numpy()
    pattern.setflags(write=False)
    mean.setflags(write=False)
    return pattern, mean


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_pattern(got, name, what):
    want = C.expected(name)
    assert R.same_bits(got, want), (
        f"{what} on {name!r}: {int((bits(got) != bits(want)).sum())} of {want.size} pixels differ, the first at "
        f"{np.argwhere(bits(got) != bits(want))[:3].tolist()}")
    nan = np.isnan(C.volume(name)).any(axis=0)
    assert np.all(bits(got)[nan] == R.CANONICAL_NAN), f"{what} on {name!r}: the NaN of a column that holds one is not the canonical one"


def check_against_torch(got, name, what):
    """``torch.quantile``'s answer against the restatement: bit for bit, but NaN where an odd ``Z`` has an infinite median."""
    want = C.expected(name)
    quirk = np.isinf(want) & bool(C.volume(name).shape[0] % 2)
    assert np.isnan(got[quirk]).all(), f"{what} on {name!r}: an infinite median of an odd count is not NaN"
    assert R.same_bits(got[~quirk], want[~quirk]), (
        f"{what} on {name!r}: {int((bits(got) != bits(want))[~quirk].sum())} of {want.size} pixels differ")


def check_mean(got, pattern, what):
    """``|got - fsum mean| <= 2^-24 |m| + n 2^-53 mean|p|``; returns the error as a fraction of the bound."""
    want = R.mean(pattern)
    if not np.isfinite(want):
        assert np.isnan(got) if np.isnan(want) else got == np.float32(want), f"{what}: mean {got} of a pattern whose mean is {want}"
        return 0.0
    err, bound = abs(float(got) - want), R.mean_bound(pattern)
    assert err <= bound, f"{what}: mean {float(got)!r}, fsum {want!r}: off by {err:.3e}, {err / bound:.3f} of the bound {bound:.3e}"
    return err / bound


# ---- the restatement against torch -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("prefix", C.GROUPS)
def test_the_restatement_is_torch_quantile_bit_for_bit(prefix):
    """Every NaN-free case without zeros of both signs, the denormal stacks included: one rounding after the difference.

    One disagreement is torch's own arithmetic and is asserted as such: for an odd ``Z`` torch still evaluates
    ``lerp(a, a, 0) = a + 0 * (a - a)``, which is NaN for an infinite middle element (``inf - inf``); the rule gives ``a``."""
    names = [n for n in C.group(prefix) if C.torch_comparable(n)]
    assert names or prefix in ("nan", "zeros")
    for name in names:
        check_against_torch(torch.quantile(_t(C.volume(name)), 0.5, dim=0).numpy(), name, "torch.quantile on the host")


def test_the_rule_by_hand():
    f = np.float32
    assert R.key(f([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf])).tolist() == [0x007FFFFF, 0x407FFFFF, 0x7FFFFFFF, 0x80000000, 0xBF800000,
                                                                          0xFF800000]
    assert np.array_equal(R.value(R.key(f([-0.0, 1.5, -np.inf]))).view(np.uint32), f([-0.0, 1.5, -np.inf]).view(np.uint32))
    col = lambda *v: np.array(v, dtype=np.float32).reshape(-1, 1, 1)           # noqa: E731
    assert bits(R.pattern(col(3, 1, 2))).tolist() == [[0x40000000]]
    assert bits(R.pattern(col(4, 1, 2, 3))).tolist() == [[0x40200000]]
    assert bits(R.pattern(col(0.0, -0.0, -0.0))).tolist() == [[0x80000000]], "-0.0 sorts below +0.0: the middle of three"
    assert bits(R.pattern(col(0.0, -0.0))).tolist() == [[0x00000000]], "0 - (0 - -0) / 2"
    assert bits(R.pattern(col(-0.0, -0.0))).tolist() == [[0x80000000]]
    assert bits(R.pattern(col(1, np.nan, 2))).tolist() == [[0x7FC00000]]
    assert np.isnan(R.pattern(col(np.inf, np.inf))).all() and bits(R.pattern(col(np.inf, np.inf, 1))).tolist() == [[0x7F800000]]
    # among the denormals (b - a) / 2 need not be a float32: a = 0, b = 3 steps: 3 - 1.5 = 1.5 -> 2 (even) in one rounding; in two,
    # 3 / 2 -> 2 and 3 - 2 = 1
    tiny = np.array([0, 3], dtype=np.uint32).view(np.float32)
    assert bits(R.lerp_half(tiny[0], tiny[1])).tolist() == [2]
    d = tiny[1] - tiny[0]
    assert bits(tiny[1] - d * f(0.5)).tolist() == [1], "(what two roundings give)"
    # a sum float64 cannot hold: b = 2^-100, b - a = 2^60 (a = -2^60): the exact 2^-100 - 2^59 rounds to -2^59
    assert float(R.lerp_half(f(-2.0 ** 60), f(2.0 ** -100))) == -2.0 ** 59
    assert R.split_level([1.0, 1.5]) == 1 and R.split_level([1.0, 1.5, 2.0]) is None and R.split_level([2.0, 2.0]) is None
    assert R.split_level([255, 256], count=True) == 2 and R.split_level([300, 301], count=True) == 3
    assert R.is_count(f([0.0, 65535.0, -0.0, 65536.0, 0.5, -1.0, np.inf, np.nan, 1e-40])).tolist() == [True, True] + [False] * 7
    vol = np.zeros((2, 1, 5), dtype=np.float32)
    vol[1, 0, 4] = -0.0
    assert R.takes_count_mode(vol, 2).tolist() == [True, True, False]
    assert R.mean(f([1e30, 1.5, -1e30, 2.5])) == 1.0 and R.apply(f([[[6.0]]]), f([[3.0]]), 1.5).tolist() == [[[3.0]]]


# ---- the census -------------------------------------------------------------------------------------------------------------


def test_the_cases_aim_at_the_tiling():
    c, g, u = C.COLS, C.PHASES, C.LOADS
    assert (c, g, u, C.REFUSED_Z) == (128, 4, 16, 65536) == F.tiling()
    assert C.Z_LIST == [1, 2, 3, 4, 5, 60, 61, 63, 64, 65, 67, 68, 124, 125, 128, 129, 300]
    assert C.NPIX == 259 == 2 * c + 3
    assert sorted(n for prefix in C.GROUPS for n in C.group(prefix)) == sorted(C.CASES), "the groups the tests run hold every case once"
    # the full-batch condition z + (u - 1) g < Z on both sides, and every tail length of a phase
    assert {z > (u - 1) * g + p for z in C.Z_BATCH for p in range(g)} == {True, False}
    assert {len(range(p, z, g)) % u for z in C.Z_BATCH + C.Z_TWO for p in range(g)} >= {0, 1, u - 1}
    assert any(z < g for z in C.Z_SMALL), "a phase without a sample"
    for count in (False, True):
        for z in C.Z_LIST:
            assert f"engineered {'count' if count else 'float'} Z={z}" in C.CASES
        assert all(C.class_of_pixel(i, count) != C.class_of_pixel(i + 1, count) for i in range(C.NPIX - 1))
        assert len(C.COUNT_CLASSES if count else C.FLOAT_CLASSES) <= 32, "every class within half a wavefront"


def test_every_class_of_column_is_present():
    """``split_level`` of the engineered columns, at every ``Z``: the level the class names for an even ``Z``, none for an odd one;
    both parities of the lower middle element's bin at every level; the decoys where the column has room."""
    parities = set()
    for count in (False, True):
        classes = C.COUNT_CLASSES if count else C.FLOAT_CLASSES
        assert {cls[4] for cls in classes} == ({None, 2, 3} if count else {None, 0, 1, 2, 3})
        for z in C.Z_LIST:
            vol = C.volume(f"engineered {'count' if count else 'float'} Z={z}").reshape(z, -1)
            assert R.takes_count_mode(vol, C.COLS).tolist() == [count] * 3
            for i in range(len(classes)):
                name, _, ka, kb, level = classes[i]
                for pixel in (i, i + len(classes) * ((C.NPIX - 1 - i) // len(classes))):      # the first and the last of the class
                    assert C.class_of_pixel(pixel, count) is classes[i]
                    column = vol[:, pixel]
                    keys, a, b = R.select_keys(column, count)
                    assert a == ka and (b == kb or z % 2), (name, z)
                    assert R.split_level(column, count) == (level if z % 2 == 0 else None), (name, z)
                    if level is None or z % 2 or z < C.Z_DECOYS:
                        continue
                    parities.add((count, level, R.bin_at(a, level) & 1))
                    shares = R.prefix_at(keys, level) == R.prefix_at(a, level)
                    lower = shares & (R.bin_at(keys, level) < R.bin_at(a, level))
                    assert {int(p) for p in R.bin_at(keys[lower], level) & 1} == {0, 1} or R.bin_at(a, level) < 2, \
                        (name, z, "lower bins of both parities under the shared prefix")
                    if "bin" not in name and "negative" not in name:
                        continue                                           # (the literal pairs: a is the least key of its bin)
                    if level < 3:
                        in_a = R.prefix_at(keys, level + 1) == R.prefix_at(a, level + 1)
                        in_b = R.prefix_at(keys, level + 1) == R.prefix_at(b, level + 1)
                        assert (keys[in_a] < a).any() and (keys[in_b] > b).any(), (name, z, "decoys in the bins of a and b")
                    if level >= 1 and (level - 1 >= 2 or not count):
                        same_byte = (R.bin_at(keys, level) == R.bin_at(a, level)) & ~shares
                        assert same_byte.any(), (name, z, "a sample equal to a in the byte of the split, not in the one before")
    assert parities == {(False, lv, p) for lv in range(4) for p in (0, 1)} | {(True, lv, p) for lv in (2, 3) for p in (0, 1)}


def test_every_run_pattern_fallback_and_special_value_is_present():
    c, g, u = C.COLS, C.PHASES, C.LOADS
    # run counting: the first-pass bin along the samples of a phase
    for count in (False, True):
        vol = C.volume(f"runs {'count' if count else 'float'} Z=300").reshape(300, -1)
        assert R.takes_count_mode(vol, c).tolist() == [count] * 3
        seen = set()
        for pixel in range(10):
            keys, _, _ = R.select_keys(vol[:, pixel], count)
            bins = R.bin_at(keys, 2 if count else 0)
            changes = [np.flatnonzero(np.diff(bins[p::g])) + 1 for p in range(g)]
            kind = C.RUN_KINDS[pixel % 5]
            if kind == "every sample":
                assert all(len(ch) == len(bins[p::g]) - 1 for p, ch in enumerate(changes))
            elif kind == "per phase":
                assert all(len(ch) == 0 for ch in changes) and len({int(bins[p]) for p in range(g)}) == g
            else:
                at = {"break at u - 1": u - 1, "break at u": u, "break at u + 1": u + 1}[kind]
                assert all(ch.tolist() == [at] for ch in changes)
            seen.add(kind)
        assert seen == set(C.RUN_KINDS)
    # fallbacks: one non-count, at every position, in the first, the ragged or every workgroup
    expect = {"first": [False, True, True], "ragged": [True, True, False], "every": [False, False, False]}
    assert C.FALLBACK_WHERE["ragged"] == [C.NPIX - 1] and C.FALLBACK_WHERE["first"][0] < c
    assert [len({i // c for i in C.FALLBACK_WHERE[w]}) for w in ("first", "ragged", "every")] == [1, 1, 3]
    assert {v for v, _ in C.NON_COUNTS} == {"0.5", "-1", "65536", "65535.5", "-0.0", "+inf", "nan", "denormal"}
    for z in C.FALLBACK_Z:
        base = C.volume(f"counts Z={z}")
        assert R.takes_count_mode(base, c).tolist() == [True] * 3 and (base == 0).any() and (base == 65535).any()
        for value, pattern_bits in C.NON_COUNTS:
            for at, zi in zip(C.FALLBACK_AT, (0, 1, 2, 3, g, z - 1)):
                for where, modes in expect.items():
                    vol = C.volume(f"fallback Z={z} {value} at {at} in {where}")
                    assert R.takes_count_mode(vol, c).tolist() == modes
                    bad = np.argwhere(~R.is_count(vol.reshape(z, -1)))
                    assert bad.tolist() == [[zi, i] for i in C.FALLBACK_WHERE[where]]
                    assert bits(vol.reshape(z, -1)[zi, bad[0, 1]]) == pattern_bits
    # NaNs of each sign, in a count-like and in a float stack, in the ragged workgroup too
    for name in C.group("nan"):
        vol = C.volume(name).reshape(C.volume(name).shape[0], -1)
        at = np.isnan(vol)
        assert set(bits(vol)[at].tolist()) == set(C.NAN_BITS) and at[:, 2 * c:].any() and at[:, :c].any() and at.sum() == 4
        clean = np.where(at, np.float32(1.0), vol)
        assert R.takes_count_mode(clean, c).all() == ("counts" in name)
    # other values
    assert all(np.isinf(C.volume(n)).any() and not np.isnan(C.volume(n)).any() for n in C.group("inf"))
    assert all((C.volume(n) < 0).all() for n in C.group("negative"))
    for n in C.group("denormal"):
        v = C.volume(n)
        assert (np.abs(v[v != 0]) < np.finfo(np.float32).tiny).mean() > 0.5 and C.torch_comparable(n)
    assert [C.volume(n).shape[0] for n in C.group("denormal")] == [2, 4, g * u]
    for n in C.group("zeros"):
        v = C.volume(n).reshape(C.volume(n).shape[0], -1)
        assert C.has_mixed_zeros(n) and np.signbit(v[:, 3]).all() and not v[:, 3].any()
        if "beside" in n:
            assert R.takes_count_mode(v, c).tolist() == [False, True, False] and not v[:, c + 3].any()
            only = v.copy()
            only[:, [3, 4, C.NPIX - 2]] = 1.0
            assert R.takes_count_mode(only, c).all(), "the zero columns alone keep their workgroups off the count mode"
    assert {C.volume(n).shape[0] % 2 for n in C.group("zeros Z")} == {0, 1} == {C.volume(n).shape[0] % 2 for n in C.group("zeros beside")}
    # the counter limit: one counter of 16 bits holds Z - 1 = 65535 in either half of its word
    for count in (False, True):
        vol = C.volume(f"limit {'count' if count else 'float'}")
        assert vol.shape == (C.REFUSED_Z - 1, 1, 3) and R.takes_count_mode(vol, c).tolist() == [count]
        level = 2 if count else 0
        first = [set(R.bin_at(R.select_keys(vol[:, 0, i], count)[0], level).tolist()) for i in range(3)]
        assert [len(s) for s in first] == [1, 1, 2] and min(first[0]) % 2 == 0 and min(first[1]) % 2 == 1 and first[2] == first[0] | first[1]
    # uint16: the count cases, 0 and 65535 among them
    assert len(C.U16_CASES) == len(C.Z_LIST) + len(C.Z_BATCH + C.Z_TWO) + 1 + len(C.FALLBACK_Z) + 1
    assert all((C.volume_u16(n) == 0).any() and (C.volume_u16(n) == 65535).any() for n in C.U16_CASES
               if n.startswith(("engineered count Z=300", "counts")))
    # the mean and the division
    assert [p[0] * p[1] for p in C.MEAN_PLANES] == [1, 255, 256, 257, 259, 256 * 256 + 1]
    big = C.mean_plane(C.MEAN_PLANES[-1], "cancelling")
    assert (np.abs(big) == np.float32(1e30)).sum() == 2 * (big.size // 4) and 0.5 < R.mean(big) < 1.0
    assert {(s[1] * s[2]) % 4 for s in C.APPLY_SHAPES} == {0, 1, 2, 3} and any(int(np.prod(s)) % 4 for s in C.APPLY_SHAPES)
    assert int(np.prod(C.APPLY_BIG["float32"])) > 256 * 64 * 256 * 4 and int(np.prod(C.APPLY_BIG["uint16"])) > 256 * 64 * 256
    _, pat = C.apply_case(C.APPLY_SHAPES[0], "float32")
    assert {0x00000000, 0x80000000, 0x00012345, 0x7FC00000} <= set(bits(pat).ravel().tolist())


# ---- the twin against the restatement -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("prefix", C.GROUPS)
def test_twin_pattern_equals_the_restatement_bit_for_bit(prefix):
    worst = 0.0
    for name in C.group(prefix):
        pattern, mean = case_twin(name)
        check_pattern(pattern, name, "twin")
        worst = max(worst, check_mean(mean[0], pattern, f"twin on {name!r}"))
        if C.is_u16_case(name):
            p16, m16 = case_twin(name, True)
            assert p16.tobytes() == pattern.tobytes() and m16.tobytes() == mean.tobytes(), f"{name}: uint16 and float32 differ"
    print(f"{prefix}: worst mean error {worst:.4f} of the bound")


@pytest.mark.parametrize("content", C.MEAN_CONTENTS)
def test_twin_mean_is_within_the_bound_of_an_fsum(content):
    for plane in C.MEAN_PLANES:
        vol = C.mean_plane(plane, content)
        ff = F.flat_field_pattern(_t(vol))
        assert ff.pattern.numpy().tobytes() == vol.tobytes(), "Z = 1: the pattern is the stack"
        frac = check_mean(ff.mean.numpy()[0], vol, f"twin on {plane} {content}")
        print(f"{plane} {content}: mean error {frac:.4f} of the bound")


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_twin_apply_is_the_restatement_byte_for_byte(dtype):
    for shape in C.APPLY_SHAPES + [C.APPLY_BIG[dtype]]:
        vol, pat = C.apply_case(shape, dtype)
        want = R.apply(vol, pat, C.APPLY_MEAN)
        ff = F.FlatFieldPattern(_t(pat), torch.tensor([C.APPLY_MEAN]))
        out = ff.apply(_t(vol))
        assert out.numpy().tobytes() == want.tobytes(), (shape, dtype)
        if dtype == "float32":
            t = _t(vol)
            assert ff.apply(t, out=t) is t and t.numpy().tobytes() == want.tobytes(), (shape, "in place")


def test_twin_refuses_the_first_z_the_counters_cannot_hold():
    vol = np.ones((C.REFUSED_Z, 1, 3), dtype=np.float32)
    pattern, mean = np.full(3, np.nan, dtype=np.float32), np.full(1, np.nan, dtype=np.float32)
    for entry, data in (("lsr_flatfield_pattern_f32_cpu", vol), ("lsr_flatfield_pattern_u16_cpu", vol.astype(np.uint16))):
        with pytest.raises(_lib.LsrUnsupported):
            _lib.call(entry, data.ctypes.data, C.REFUSED_Z, 1, 3, pattern.ctypes.data, mean.ctypes.data, None, None)
        assert np.isnan(pattern).all() and np.isnan(mean).all()
