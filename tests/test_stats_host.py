"""The whole-volume statistics on the CPU: the host twins (``lsr_digit_histogram_f32_cpu`` / ``_u16_cpu``, ``lsr_rescale_*_cpu``)
and ``shrimpy_amd.stats`` on top of them, on every case of tests/stats_cases.py against the numpy restatement
(tests/stats_ref.py): tables equal as integers (pre-loaded counts kept, guard words intact), order statistics byte for byte,
moments inside the bounds of ``csrc/stats.hpp``, quantiles against ``np.quantile``, the rescale bit for bit, the entry checks.
The helpers take a device: tests/test_stats_gpu.py runs them on the kernels."""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import stats as ST
from tests import stats_cases as C
from tests import stats_ref as R

CPU = torch.device("cpu")
E_ARG = -4


def upload(arr, device):
    return torch.from_numpy(np.array(arr)).to(device)


def raw_pass(t_vol, pass_index, prefixes, table_of, device, cap=0, form=ST.FORM_RUNS, flush=0, record=False):
    """One call of the raw entry on pre-loaded tables (and a pre-loaded record) between guard words: what the call added to the
    tables (uint64 [k, bins]) and to the record's first two words."""
    k = len(prefixes)
    before = C.preload(k)
    buf = torch.full((2 * C.GUARD + k * C.BINS,), C.FILL, dtype=torch.int64)
    buf[C.GUARD:C.GUARD + k * C.BINS] = torch.from_numpy(before)
    buf = buf.to(device)
    rec = torch.full((2 * C.GUARD + ST.RECORD_WORDS,), C.FILL, dtype=torch.int64)
    rec[C.GUARD:C.GUARD + ST.RECORD_WORDS] = torch.tensor([5, 7, 0, 0, 0])
    rec = rec.to(device)
    ST.digit_histogram(t_vol, pass_index, prefixes, table_of, buf[C.GUARD:C.GUARD + k * C.BINS],
                       rec[C.GUARD:C.GUARD + ST.RECORD_WORDS] if record else None, cap, form, flush)
    host, hrec = buf.cpu().numpy(), rec.cpu().numpy()
    assert np.all(host[:C.GUARD] == C.FILL) and np.all(host[C.GUARD + k * C.BINS:] == C.FILL), "written outside the tables"
    assert np.all(hrec[:C.GUARD] == C.FILL) and np.all(hrec[C.GUARD + ST.RECORD_WORDS:] == C.FILL), "written outside the record"
    added = (host[C.GUARD:C.GUARD + k * C.BINS] - before).view(np.uint64).reshape(k, C.BINS)
    counts = hrec[C.GUARD:C.GUARD + 2] - np.array([5, 7])
    if not record:
        assert np.array_equal(hrec[C.GUARD:C.GUARD + ST.RECORD_WORDS], [5, 7, 0, 0, 0]), "the record was touched"
    return added, counts


def ranks_of_case(content, arr, m):
    if content == "parting":                  # one rank in each of the five keys
        return [int(i) for i in np.unique(R.sorted_keys([arr]), return_index=True)[1]]
    return C.edge_ranks(m)


def check_tables(content, n, device, caps=(0,), forms=(ST.FORM_RUNS,)):
    arr = C.volume(content, n)
    t_vol = upload(arr, device)
    m = R.non_nan(arr).size
    ranks = ranks_of_case(content, arr, m) if m else None
    for p in range(C.passes(arr)):
        prefixes, table_of = C.plan_of(arr, ranks, p) if m else ([0], [0])
        if content == "parting" and n >= 5:
            assert len(set(table_of)) == min(p + 1, 4), "the prefixes part at each pass in turn"
        want = R.digit_tables(arr, p, prefixes, table_of, C.BITS)
        for cap in caps:
            for form in forms:
                got, counts = raw_pass(t_vol, p, prefixes, table_of, device, cap, form, record=(p == 0))
                assert np.array_equal(got, want), f"{content}, n {n}, pass {p}, cap {cap}, form {form}"
                if p == 0:
                    assert counts.tolist() == [m, arr.size - m], f"{content}, n {n}, cap {cap}, form {form}: counts"


def check_select(content, n, device, cap=0, form=ST.FORM_RUNS):
    """Order statistics, moments and quantiles of one case: how many interpolated quantiles were bit-equal to numpy's, of how
    many."""
    arr = C.volume(content, n)
    t_vol = upload(arr, device)
    what = f"{content}, n {n}, cap {cap}, form {form}"
    m = R.non_nan(arr).size
    C.check_moments(ST.moments(t_vol, cap, form), [arr], what)
    got_q = ST.quantiles(t_vol, C.QS, cap, form)
    equal = C.check_quantiles(got_q, [arr], C.QS, what)
    if m == 0:
        with pytest.raises(ValueError):
            ST.order_statistics(t_vol, [0], cap, form)
        return equal, len(C.QS)
    ranks = C.many_ranks(m)
    got = ST.order_statistics(t_vol, ranks, cap, form)
    assert got.dtype == arr.dtype and got.tobytes() == R.order_statistics([arr], ranks).tobytes(), what
    assert np.array_equal(got, np.sort(R.non_nan(arr))[ranks]), f"{what}: by value against np.sort"
    return equal, len(C.QS)


@pytest.mark.parametrize("content", C.F32_CONTENTS + C.U16_CONTENTS)
def test_twin_tables_equal_the_restatement(content):
    for n in C.SIZES:
        check_tables(content, n, CPU)


@pytest.mark.parametrize("content", C.F32_CONTENTS + C.U16_CONTENTS)
def test_order_statistics_moments_and_quantiles(content):
    equal = total = 0
    for n in C.SIZES:
        e, t = check_select(content, n, CPU)
        equal, total = equal + e, total + t
    print(f"{content}: {equal} of {total} checked quantiles bit-equal to np.quantile")


def check_pooling(device, dtype_content, cap=0):
    arrs = [C.volume(dtype_content, n) for n in (C.S + 1, 65, 2 * C.S + 1)]
    vols = [upload(a, device) for a in arrs]
    whole = np.concatenate(arrs)
    m = R.non_nan(whole).size
    ranks = C.many_ranks(m)
    pooled = ST.order_statistics(vols, ranks, cap)
    assert pooled.tobytes() == R.order_statistics([whole], ranks).tobytes()
    assert pooled.tobytes() == ST.order_statistics(upload(whole, device), ranks, cap).tobytes()
    C.check_moments(ST.moments(vols, cap), arrs, "pooled")
    C.check_quantiles(ST.quantiles(iter(vols), C.QS, cap), [whole], C.QS, "pooled")
    s = ST.summary(vols, [0.01, 0.99], cap)
    assert s["median"] == s["quantiles"][0.5] and s["iqr"] == s["quantiles"][0.75] - s["quantiles"][0.25]
    assert sorted(s["quantiles"]) == [0.01, 0.25, 0.5, 0.75, 0.99] and s["count"] == m


@pytest.mark.parametrize("content", ["some_nans", "offset", "random"])
def test_three_volumes_pool_into_their_concatenation(content):
    check_pooling(CPU, content)


def check_flush(device):
    """A workgroup of five strides that flushes its LDS tables after every stride, and after every second one."""
    for content in ("offset", "random"):
        arr = C.volume(content, C.MULTI_SPAN)
        t_vol = upload(arr, device)
        ranks = C.edge_ranks(arr.size)
        for p in range(C.passes(arr)):
            prefixes, table_of = C.plan_of(arr, ranks, p)
            want = R.digit_tables(arr, p, prefixes, table_of, C.BITS)
            for form in C.FORMS:
                for flush in (1, 2):
                    got, _ = raw_pass(t_vol, p, prefixes, table_of, device, 1, form, flush)
                    assert np.array_equal(got, want), f"{content}, pass {p}, form {form}, flush every {flush}"


def test_flush_period_changes_nothing():
    check_flush(CPU)


def check_census(device):
    """Every pass in both forms, on a workgroup of several strides."""
    ST.CENSUS.clear()
    for content in ("offset", "random"):
        arr = C.volume(content, C.MULTI_SPAN)
        for form in C.FORMS:
            ranks = C.many_ranks(arr.size)
            got = ST.order_statistics(upload(arr, device), ranks, 2, form)
            assert got.tobytes() == R.order_statistics([arr], ranks).tobytes()
            # ... and the same volume as ONE workgroup of five strides that flushes its LDS tables in the middle of its span
            prefixes, table_of = C.plan_of(arr, C.edge_ranks(arr.size), 1)
            got, _ = raw_pass(upload(arr, device), 1, prefixes, table_of, device, 1, form, flush=2)
            assert np.array_equal(got, R.digit_tables(arr, 1, prefixes, table_of, C.BITS))
    for form in C.FORMS:
        assert ST.CENSUS[("flush", form)] > 0, f"the mid-span flush in form {form} was not reached"
        for p in range(C.G["passes_f32"]):
            assert ST.CENSUS[(p, form)] > 0, f"pass {p} in form {form} was not reached"
    assert C.MULTI_SPAN > 2 * 2 * C.S, "at grid cap 2 a workgroup takes more than one stride"
    # a set without a non-NaN voxel: pass 0 and nothing after it
    ST.CENSUS.clear()
    got = ST.quantiles(upload(C.volume("all_nans", 65), device), C.QS)
    assert all(np.isnan(v) for v in got) and dict(ST.CENSUS) == {(0, ST.FORM_RUNS): 1}


def test_census():
    check_census(CPU)


def test_positive_infinity_alone_gives_an_infinite_mean():
    a = np.abs(C.volume("offset", 65)).copy()
    a[7] = np.inf
    got = ST.moments(upload(a, CPU))
    assert got["mean"] == np.inf and got["max"] == np.inf and got["count"] == 65


RESCALES = [(100.0, 7.5, None), (0.1, 3.0, (0.0, 1.0)), (-2.5, 0.3, (-1.0, 2.0)), (1.0, 0.0, None), (0.0, 1.0, (-0.0, 0.0))]


def check_rescale(device):
    rng = np.random.default_rng(5)
    for n in (1, 3, 4, 7, 8, 9, 1023, 1025, C.S + 5):
        f = rng.normal(1, 2, n).astype(np.float32)
        f[rng.random(n) < 0.1] = np.nan
        f[rng.random(n) < 0.05] = np.inf
        f[rng.random(n) < 0.05] = -np.inf
        f[rng.random(n) < 0.05] = -0.0
        f[rng.random(n) < 0.05] = 1.0
        u = rng.integers(0, 65536, n).astype(np.uint16)
        for v in (f, u):
            for sub, div, clip in RESCALES:
                want = R.rescale(v, sub, div, clip)
                got = ST.rescale(upload(v, device), sub, div, clip)
                assert got.dtype == torch.float32 and got.cpu().numpy().tobytes() == want.tobytes(), f"{v.dtype}, n {n}, {sub}, {div}, {clip}"
        t = upload(f, device)
        assert ST.rescale(t, 0.1, 3.0, (0.0, 1.0), out=t) is t and t.cpu().numpy().tobytes() == R.rescale(f, 0.1, 3.0, (0.0, 1.0)).tobytes()


def test_rescale_is_numpys_expression_bit_for_bit():
    check_rescale(CPU)


def test_normalize_methods():
    arr = C.volume("offset", C.S + 1)
    t = upload(arr, CPU)
    x = arr.astype(np.float64)
    out, how = ST.normalize(t, "percentile", 1, 99.9, clip=True)
    lo, hi = np.quantile(x, [0.01, 0.999])
    assert abs(how["sub"] - lo) <= 1e-9 and abs(how["div"] - (hi - lo)) <= 1e-9 and not how["degenerate"]
    assert out.cpu().numpy().tobytes() == R.rescale(arr, how["sub"], how["div"], (0.0, 1.0)).tobytes()
    _, how = ST.normalize(t, "zscore")
    assert abs(how["sub"] - x.mean()) <= 1e-6 and abs(how["div"] - x.std()) <= 1e-6
    _, how = ST.normalize(t, "robust")
    assert abs(how["sub"] - np.median(x)) <= 1e-9
    out, how = ST.normalize(upload(C.volume("constant", 65), CPU), "robust")
    assert how["degenerate"] and how["div"] == 1.0 and not out.numpy().any()


def entry_check_calls(vol_ptr, tables_ptr, record_ptr, u16):
    """(what, status, the arguments in front of the stream) of calls the histogram entry must refuse: only calls whose pointers
    are valid for the stated size, or that are refused for the size before anything is read."""
    pre = np.zeros(C.K + 1, np.uint32)
    tab = np.zeros(C.K + 1, np.int32)
    bad_tab, bad_pre, split = tab.copy(), pre.copy(), tab.copy()
    bad_tab[0] = 1
    bad_pre[0] = C.BINS
    split[1] = 1
    passes = C.G["passes_u16"] if u16 else C.G["passes_f32"]
    ok = dict(vol=vol_ptr, n=64, p=0, pre=pre, tab=tab, k=1, tables=tables_ptr, rec=record_ptr, cap=0, form=0)
    cases = [
        ("n == 0", E_ARG, dict(n=0)), ("n < 0", E_ARG, dict(n=-1)), ("k == 0", E_ARG, dict(k=0)), ("k == K + 1", E_ARG, dict(k=C.K + 1)),
        ("pass < 0", E_ARG, dict(p=-1)), ("pass past the key", E_ARG, dict(p=passes, rec=None)),
        ("NULL in", E_ARG, dict(vol=None)), ("NULL tables", E_ARG, dict(tables=None)), ("NULL prefixes", E_ARG, dict(pre=None)),
        ("NULL table_of_rank", E_ARG, dict(tab=None)), ("misaligned in", E_ARG, dict(vol=vol_ptr + 2)),
        ("misaligned tables", E_ARG, dict(tables=tables_ptr + 4)), ("misaligned record", E_ARG, dict(rec=record_ptr + 4)),
        ("a table outside 0 .. k - 1", E_ARG, dict(tab=bad_tab)), ("a prefix in pass 0", E_ARG, dict(pre=bad_pre)),
        ("a prefix pass 1 cannot have", E_ARG, dict(pre=bad_pre, p=1, rec=None)),
        ("two tables, one prefix", E_ARG, dict(k=2, tab=split)), ("a record after pass 0", E_ARG, dict(p=1)),
        ("grid_cap < 0", E_ARG, dict(cap=-1)), ("an unknown form", E_ARG, dict(form=2)), ("form < 0", E_ARG, dict(form=-256)),
        ("n == 2^48", _lib.E_UNSUPPORTED, dict(n=2**48)),
    ]
    if u16:
        cases.append(("65535^2 n >= 2^64", _lib.E_UNSUPPORTED, dict(n=2**64 // 65535**2 + 1)))
    for what, status, change in cases:
        a = dict(ok, **change)
        yield what, status, (a["vol"], a["n"], a["p"], None if a["pre"] is None else a["pre"].ctypes.data,
                             None if a["tab"] is None else a["tab"].ctypes.data, a["k"], a["tables"], a["rec"], a["cap"], a["form"]), (a["pre"], a["tab"])


def rescale_check_calls(vol_ptr, out_ptr, u16):
    nan = float("nan")
    ok = dict(vol=vol_ptr, n=64, sub=0.0, div=1.0, clip=1, lo=0.0, hi=1.0, out=out_ptr)
    cases = [("n == 0", E_ARG, dict(n=0)), ("NULL in", E_ARG, dict(vol=None)), ("NULL out", E_ARG, dict(out=None)),
             ("misaligned in", E_ARG, dict(vol=vol_ptr + 4)), ("misaligned out", E_ARG, dict(out=out_ptr + 8)),
             ("clip 2", E_ARG, dict(clip=2)), ("lo > hi", E_ARG, dict(lo=2.0)), ("a NaN bound", E_ARG, dict(hi=nan)),
             ("out inside in", E_ARG, dict(out=vol_ptr + 16)), ("n == 2^48", _lib.E_UNSUPPORTED, dict(n=2**48))]
    if u16:
        cases.append(("uint16 in place", E_ARG, dict(out=vol_ptr)))
    for what, status, change in cases:
        a = dict(ok, **change)
        yield what, status, (a["vol"], a["n"], a["sub"], a["div"], a["clip"], a["lo"], a["hi"], a["out"])


def check_entries(device, u16, suffix, stream):
    vol = upload(np.ones(256, np.uint16 if u16 else np.float32), device)
    tables = torch.zeros((C.K * C.BINS,), dtype=torch.int64, device=device)
    record = torch.zeros((8,), dtype=torch.int64, device=device)
    out = torch.zeros((256,), dtype=torch.float32, device=device)
    kind = "u16" if u16 else "f32"
    for what, status, args, _keep in entry_check_calls(vol.data_ptr(), tables.data_ptr(), record.data_ptr(), u16):
        with pytest.raises(_lib.LsrError) as err:
            _lib.call(f"lsr_digit_histogram_{kind}{suffix}", *args, stream)
        assert err.value.code == status, what
    for what, status, args in rescale_check_calls(vol.data_ptr(), out.data_ptr(), u16):
        with pytest.raises(_lib.LsrError) as err:
            _lib.call(f"lsr_rescale_{kind}{suffix}", *args, stream)
        assert err.value.code == status, what
    assert not tables.cpu().numpy().any() and not record.cpu().numpy().any() and not out.cpu().numpy().any()
    assert np.all(vol.cpu().numpy() == 1)


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_entry_checks(u16):
    check_entries(CPU, u16, "_cpu", None)


def test_geometry_and_python_checks():
    g = ST.geometry()
    assert 8 <= g["digit_bits"] <= 11 and g["bins"] == 1 << g["digit_bits"] and g["passes_f32"] == -(-32 // g["digit_bits"])
    assert g["step"] == g["wave_step"] * g["threads"] // 64 and g["lds_bytes"] == g["K"] * g["bins"] * 4
    t = upload(C.volume("offset", 65), CPU)
    with pytest.raises(ValueError):
        ST.order_statistics(t, [65])
    with pytest.raises(ValueError):
        ST.quantiles(t, [1.5])
    with pytest.raises(TypeError):
        ST.quantiles(t.double(), [0.5])
    with pytest.raises(ValueError):
        ST.quantiles([t, upload(C.volume("random", 65), CPU)], [0.5])
    assert ST.order_statistics(t[1:], [0, 63]).tobytes() == R.order_statistics([C.volume("offset", 65)[1:]], [0, 63]).tobytes()
