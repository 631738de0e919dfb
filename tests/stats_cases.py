"""The cases the statistics tests share (tests/test_stats_host.py on the twins, tests/test_stats_gpu.py on the kernels): sizes
from ``lsr_volume_stats_geometry``, contents, ranks and the checks against tests/stats_ref.py.  Nothing needs more than a few
tens of thousands of voxels."""

import functools

import numpy as np

from shrimpy_amd import stats as ST
from tests import stats_ref as R

G = ST.geometry()
W, S, K, BITS, BINS = G["wave_step"], G["step"], G["K"], G["digit_bits"], G["bins"]
# n: below, at and past a wave step (W) and one workgroup's stride (S); the last is three strides per workgroup at cap 2
SIZES = sorted({1, 2, 63, 64, 65, W - 1, W + 1, S - 1, S, S + 1, 2 * S + 1, 5 * S + 7})
MULTI_SPAN = 5 * S + 7
CAPS = (1, 2, 0)
FORMS = (ST.FORM_RUNS, ST.FORM_PLAIN)
GUARD, FILL = 64, -7

F32_CONTENTS = ("constant", "one_differs", "permutation", "two_values", "signed_zeros", "infinities", "some_nans", "all_nans",
                "nan_ends", "denormals", "offset", "last_digit", "first_digit", "runs", "parting")
U16_CONTENTS = ("zeros", "full", "random", "two_low")


def passes(arr) -> int:
    return G["passes_u16"] if arr.dtype == np.uint16 else G["passes_f32"]


def _bits(b) -> np.ndarray:
    return np.asarray(b, dtype=np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def volume(content: str, n: int) -> np.ndarray:
    """The case's array (read-only: shared between the tests)."""
    rng = np.random.default_rng(1000 * n + sum(map(ord, content)))
    if content == "constant":
        a = np.full(n, 3.5, np.float32)
    elif content == "one_differs":
        a = np.full(n, 3.5, np.float32)
        a[n // 2] = -2.25
    elif content == "permutation":
        a = (rng.permutation(n).astype(np.float32) - np.float32(n // 3)) * np.float32(0.5)
    elif content == "two_values":
        a = rng.choice(_bits([0x3F800000, 0x3F800001]), n)
    elif content == "signed_zeros":
        a = rng.choice(np.array([-0.0, 0.0], np.float32), n)
    elif content == "infinities":
        a = rng.normal(0, 1, n).astype(np.float32)
        a[rng.random(n) < 0.1] = np.inf
        a[rng.random(n) < 0.1] = -np.inf
    elif content == "some_nans":
        a = rng.normal(0, 1, n).astype(np.float32)
        a[rng.random(n) < 0.1] = np.nan
        a[rng.random(n) < 0.1] = _bits([0xFFC00001])[0]             # (a NaN with the sign bit set: its key is below -inf's)
    elif content == "all_nans":
        a = np.full(n, np.nan, np.float32)
    elif content == "nan_ends":
        a = rng.normal(0, 1, n).astype(np.float32)
        a[0] = a[-1] = np.nan
    elif content == "denormals":
        a = _bits(rng.integers(1, 1000, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)))
    elif content == "offset":
        a = (1e4 + rng.normal(0, 1, n)).astype(np.float32)
    elif content == "last_digit":
        a = _bits(np.uint32(0x40490F00) | rng.integers(0, BINS, n).astype(np.uint32))
    elif content == "first_digit":
        a = _bits((rng.integers(0, BINS, n).astype(np.uint32) << np.uint32(32 - BITS)) | np.uint32(0x00345678))
    elif content == "runs":                    # runs of 1 .. 130 equal values, one after another across the wave steps
        lengths = np.arange(1, 131)
        values = (np.arange(130) % 7).astype(np.float32) * np.float32(1.25) - np.float32(2)
        a = np.resize(np.repeat(values, lengths), n).astype(np.float32)
    elif content == "parting":                 # five keys: one parts from the rest at each digit in turn
        base = 0x40000000
        keys = [base] + [base ^ (1 << (32 - BITS * (d + 1))) for d in range(32 // BITS)]
        a = np.resize(R.values_of(keys, np.float32), n)
    elif content == "zeros":
        a = np.zeros(n, np.uint16)
    elif content == "full":
        a = np.full(n, 65535, np.uint16)
    elif content == "random":
        a = rng.integers(0, 65536, n).astype(np.uint16)
    elif content == "two_low":
        a = rng.choice(np.array([1000, 1001], np.uint16), n)
    else:
        raise KeyError(content)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def edge_ranks(m: int) -> list[int]:
    """0, 1, m//2 - 1, m//2, m - 2, m - 1 of a multiset of ``m``, inside it, then two of them again: K ranks with duplicates."""
    r = [min(max(v, 0), m - 1) for v in (0, 1, m // 2 - 1, m // 2, m - 2, m - 1)]
    return (r + r[:2])[:K]


def many_ranks(m: int) -> list[int]:
    """The edge ranks and K + 1 spread ones: more than one group, with duplicates."""
    return edge_ranks(m) + [int(v) for v in np.linspace(0, m - 1, K + 1)]


def plan_of(arr, ranks, pass_index: int):
    """(prefixes, table_of_rank) of ``ranks`` in pass ``pass_index``, from the sorted keys."""
    keys = R.sorted_keys([arr])
    kbits = R.key_bits(arr.dtype)
    prefixes = [R.prefix_of(keys[r], pass_index, BITS, kbits) for r in ranks]
    distinct = sorted(set(prefixes))
    return prefixes, [distinct.index(p) for p in prefixes]


def preload(k: int) -> np.ndarray:
    """Counts the tables hold before a call: they must come back with the new counts added."""
    return (np.arange(k * BINS, dtype=np.int64) * 3 + 1) % 1000


def check_moments(got: dict, arrs, what: str) -> dict:
    """A decoded record (``stats.moments``) against the restatement: counts and extremes exactly, float64 sums inside
    ``2 n 2^-53 sum|terms|``, uint16 sums as integers."""
    want = R.moments(arrs)
    assert got["count"] == want["count"] and got["nan_count"] == want["nan_count"], what
    if want["count"] == 0:
        assert np.isnan(got["min"]) and np.isnan(got["max"]) and np.isnan(got["mean"]), what
        return want
    dtype = arrs[0].dtype
    assert np.asarray(got["min"], dtype).tobytes() == want["min"].tobytes(), f"{what}: min {got['min']!r} != {want['min']!r}"
    assert np.asarray(got["max"], dtype).tobytes() == want["max"].tobytes(), f"{what}: max {got['max']!r} != {want['max']!r}"
    if dtype == np.uint16:
        assert got["sum"] == want["sum"] and got["sum_sq"] == want["sum_sq"], what
    elif want["finite"]:
        n = want["count"]
        for f in ("sum", "sum_sq"):
            bound = 2 * n * 2.0**-53 * want[f + "_abs"]
            assert abs(got[f] - want[f]) <= bound, f"{what}: {f} {got[f]!r} is {abs(got[f] - want[f]):.3e} from {want[f]!r}, bound {bound:.3e}"
    return want


QS = (0.0, 0.001, 0.01, 0.25, 0.5, 0.75, 0.99, 0.999, 1.0, 1 / 3)


def check_quantiles(got, arrs, qs, what: str) -> int:
    """``stats.quantiles`` against numpy on the float64 copy: the bracketing order statistics exactly (``method="lower"`` /
    ``"higher"``) and the interpolated value inside ``8 2^-53 max(|a|, |b|)``.  Returns how many were bit-equal."""
    x = np.concatenate([R.non_nan(a) for a in arrs]).astype(np.float64)
    if x.size == 0:
        assert all(np.isnan(v) for v in got), what
        return len(got)
    keys = R.sorted_keys(arrs)
    equal = 0
    for q, v in zip(qs, got):
        j, j1, g = R.bracket(q, x.size)
        a, b = (float(t) for t in R.values_of([keys[j], keys[j1]], arrs[0].dtype))
        assert a == np.quantile(x, q, method="lower"), f"{what}: q {q} lower"
        assert (b if g > 0.0 else a) == np.quantile(x, q, method="higher"), f"{what}: q {q} higher"      # (ceil(h) is j at g == 0)
        assert np.float64(v).tobytes() == np.float64(R.interpolate(a, b, g)).tobytes() or (np.isnan(v) and np.isnan(R.interpolate(a, b, g))), \
            f"{what}: q {q}: {v!r} is not the rule's {R.interpolate(a, b, g)!r}"
        if not (np.isfinite(a) and np.isfinite(b)):
            continue
        with np.errstate(all="ignore"):
            want = float(np.quantile(x, q))
        assert abs(v - want) <= 8 * 2.0**-53 * max(abs(a), abs(b)), f"{what}: q {q}: {v!r} vs numpy's {want!r}"
        equal += np.float64(v).tobytes() == np.float64(want).tobytes() or v == want
    return equal
