"""The whole-volume statistics kernels (``csrc/stats.hip``) on the device, on every case of tests/stats_cases.py (sized from
``lsr_volume_stats_geometry``) at every grid cap and in both forms: tables equal to the numpy restatement (tests/stats_ref.py)
and to the host twin as integers, pre-loaded counts kept and guard words intact; order statistics byte for byte; moments inside
the bounds of ``csrc/stats.hpp``; quantiles against ``np.quantile``; the rescale bit for bit; the entry checks.  The checks are
tests/test_stats_host.py's, handed the device.  Every test is a few hundred launches on at most 20 487 voxels."""

import numpy as np
import pytest
import torch

from shrimpy_amd import _lib
from shrimpy_amd import stats as ST
from tests import stats_cases as C
from tests import stats_ref as R
from tests import test_stats_host as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("content", C.F32_CONTENTS + C.U16_CONTENTS)
def test_kernel_tables_equal_the_restatement_at_every_cap_in_both_forms(content, device):
    for n in C.SIZES:
        H.check_tables(content, n, device, C.CAPS, C.FORMS)


@pytest.mark.parametrize("content", C.F32_CONTENTS + C.U16_CONTENTS)
def test_kernel_tables_equal_the_twins(content, device):
    for n in (65, C.S + 1, C.MULTI_SPAN):
        arr = C.volume(content, n)
        m = R.non_nan(arr).size
        ranks = H.ranks_of_case(content, arr, m) if m else None
        for p in range(C.passes(arr)):
            prefixes, table_of = C.plan_of(arr, ranks, p) if m else ([0], [0])
            twin, twin_counts = H.raw_pass(H.upload(arr, H.CPU), p, prefixes, table_of, H.CPU, record=(p == 0))
            for form in C.FORMS:
                got, counts = H.raw_pass(H.upload(arr, device), p, prefixes, table_of, device, 2, form, record=(p == 0))
                assert np.array_equal(got, twin) and np.array_equal(counts, twin_counts), f"{content}, n {n}, pass {p}, form {form}"


@pytest.mark.parametrize("content", C.F32_CONTENTS + C.U16_CONTENTS)
def test_order_statistics_moments_and_quantiles(content, device):
    equal = total = 0
    for n in C.SIZES:
        for cap, form in ((0, ST.FORM_RUNS), (2, ST.FORM_RUNS), (1, ST.FORM_PLAIN)):
            e, t = H.check_select(content, n, device, cap, form)
            equal, total = equal + e, total + t
    print(f"{content}: {equal} of {total} checked quantiles bit-equal to np.quantile")


@pytest.mark.parametrize("content", ["some_nans", "offset", "random"])
def test_three_volumes_pool_into_their_concatenation(content, device):
    for cap in (0, 2):
        H.check_pooling(device, content, cap)


def test_flush_period_changes_nothing(device):
    H.check_flush(device)


def test_census(device):
    H.check_census(device)


def test_positive_infinity_alone_gives_an_infinite_mean(device):
    a = np.abs(C.volume("offset", C.S + 1)).copy()
    a[7] = np.inf
    got = ST.moments(H.upload(a, device))
    assert got["mean"] == np.inf and got["max"] == np.inf and got["count"] == a.size


def test_rescale_is_numpys_expression_bit_for_bit(device):
    H.check_rescale(device)


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_entry_checks(u16, device):
    with torch.cuda.device(device):
        H.check_entries(device, u16, "", _lib.stream_ptr(device))
