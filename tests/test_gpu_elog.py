"""``clv_elog2cbs`` (csrc/elog.hip) against the model of tests/elog_ref.py on every sort path of
``rocprim::radix_sort_pairs`` (one block up to 1,024 events, merge sort up to 1,048,576, onesweep
above) and at the edges of the conversion: shuffled rows, dropped customers, events on and beyond
T_cal / T_tot, T_cal > T_tot, negative nanosecond timestamps, full-range signed ids, one event, one
customer, one day, all singletons.  Integer columns equal, ratio and sales columns bit for bit, litt
within (litt_terms + 2) * 2^-52 * litt_abs; no row is set aside."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest

from tests import elog_ref as E

pytestmark = pytest.mark.gpu

EXACT = set(E.INT_COLS + E.BIT_COLS + E.HOLD_INT_COLS + E.HOLD_BIT_COLS) | {"rows"}
WRAPPER_CASES = [k for k in E.ELOG_CASES if k != "signed"]


@pytest.fixture(scope="module", autouse=True)
def device():
    from mcmc_clv_model_amd import _lib
    _lib.lib()
    assert _lib.device_count() >= 1, "no HIP device: GPU tests must run on an MI355X"


@functools.lru_cache(maxsize=None)
def case(name):
    return E.ELOG_CASES[name]()[0]


@functools.lru_cache(maxsize=None)
def model(name, with_sales=True):
    vec = E.elog_model_vec if name in E.VEC_CASES else None
    return E.run_model(case(name), model=vec, with_sales=with_sales, raw_ids=name == "signed")


def frame(inputs, with_sales=True):
    cust, date_ns, sales, *_ = inputs
    df = pd.DataFrame(dict(cust=cust, date=pd.to_datetime(date_ns)))
    if with_sales:
        df["sales"] = sales
    return df


def run_wrapper(inputs, with_sales=True):
    from mcmc_clv_model_amd.data import elog2cbs
    return elog2cbs(frame(inputs, with_sales), units=inputs[3], T_cal=inputs[4], T_tot=inputs[5])


@functools.lru_cache(maxsize=None)
def device_cbs(name):
    return run_wrapper(case(name))


def run_c_abi(inputs):
    """clv_elog2cbs itself: the ids reach the kernels as they are."""
    from mcmc_clv_model_amd import _lib
    L = _lib.lib()
    cust, date_ns, sales, units, T_cal, T_tot = inputs
    Tc, Tt = E.resolve_T(date_ns, T_cal, T_tot)
    n = len(cust)
    cust, date_ns, sales = (np.ascontiguousarray(a, dtype=t) for a, t in
                            ((cust, np.int64), (date_ns, np.int64), (sales, np.float64)))
    ints, dbls = ("cust", "x", "first", "x_star"), ("t_x", "litt", "sales", "sales_x", "T_cal", "T_star", "sales_star")
    o = {c: np.full(n, -7, np.int64) for c in ints}
    o.update({c: np.full(n, np.nan) for c in dbls})
    nc = ctypes.c_int64(-1)
    i64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))  # noqa: E731
    dp = _lib.dptr
    _lib.check(L.clv_elog2cbs(-1, n, i64(cust), i64(date_ns), dp(sales), E.unit_ns(units), Tc, Tt, ctypes.byref(nc),
                              i64(o["cust"]), i64(o["x"]), dp(o["t_x"]), dp(o["litt"]), dp(o["sales"]),
                              dp(o["sales_x"]), i64(o["first"]), dp(o["T_cal"]), dp(o["T_star"]), i64(o["x_star"]),
                              dp(o["sales_star"])))
    k = nc.value
    assert 0 <= k <= n
    for c in ints:  # rows past the count are untouched
        assert (o[c][k:] == -7).all(), c
    out = {c: v[:k] for c, v in o.items()}
    if not Tc < Tt:
        assert not out["T_star"].any() and not out["x_star"].any() and not out["sales_star"].any()
        for c in E.HOLD_INT_COLS + E.HOLD_BIT_COLS:
            del out[c]
    return out


@pytest.mark.parametrize("name", WRAPPER_CASES)
def test_wrapper_matches_model(name):
    got, want = device_cbs(name), model(name)
    ratio = []
    bad = E.mismatches(E.frame_columns(got), want, ratio)
    print(f"elog {name}: {len(got)} rows, litt ratio {ratio[0] if ratio else 0.0:.3f}")
    assert bad == []
    exp = E.expected_dtypes(want["holdout"], True, bool((want["x"] > 0).any()))
    assert list(got.columns) == [c for c, _ in exp]
    assert [got[c].dtype.kind for c, _ in exp[1:]] == [k for _, k in exp[1:]]
    assert got["cust"].dtype == frame(case(name))["cust"].dtype
    assert isinstance(got.index, pd.RangeIndex)


def test_signed_ids_through_the_c_abi():
    got, want = run_c_abi(case("signed")), model("signed")
    assert got["cust"][0] == E.INT64_MIN and got["cust"][-1] == E.INT64_MAX
    ratio = []
    assert E.mismatches(got, want, ratio) == []
    print(f"elog signed: {len(got['cust'])} rows, litt ratio {ratio[0]:.3f}")


def test_c_abi_equals_wrapper_on_codes():
    """The same log through the C ABI with its raw ids and through the wrapper's sorted codes."""
    a, b = run_c_abi(case("shuffled")), E.frame_columns(device_cbs("shuffled"))
    assert a.keys() == b.keys()
    for c in a:
        assert np.asarray(a[c], dtype=b[c].dtype).tobytes() == b[c].tobytes(), c


def test_without_sales():
    got, want = run_wrapper(case("shuffled"), with_sales=False), model("shuffled", False)
    assert E.mismatches(E.frame_columns(got), want) == []
    exp = E.expected_dtypes(True, with_sales=False)
    assert list(got.columns) == [c for c, _ in exp]
    assert [got[c].dtype.kind for c, _ in exp[1:]] == [k for _, k in exp[1:]]
    for c in ("x", "sales", "sales_x"):
        assert got[c].dtype == np.int64 and np.array_equal(got[c].to_numpy(), want[c]), c
    # event counts: at least one per run, and more than the runs where same-day events were merged
    assert (got["sales"] >= got["x"] + 1).all() and (got["sales"] > got["x"] + 1).any()
    assert (got["sales_star"] >= got["x_star"]).all() and got["sales_star"].dtype == np.float64


def test_row_permutations_leave_the_cbs_unchanged():
    """Exact sales make every sum order-free, so the CBS of ``shuffled`` is bit-identical under
    permutations of its rows: the two stable sorts compose to the (customer, date) order."""
    cust, date_ns, sales, units, T_cal, T_tot = case("shuffled")
    base = E.frame_columns(device_cbs("shuffled"))
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(len(cust))
        assert not np.array_equal(p, np.arange(len(cust)))
        got = E.frame_columns(run_wrapper((cust[p], date_ns[p], sales[p], units, T_cal, T_tot)))
        assert got.keys() == base.keys()
        for c in base:
            assert got[c].dtype == base[c].dtype and got[c].tobytes() == base[c].tobytes(), (seed, c)


@pytest.mark.parametrize("wrong,name", [("lt_cal", "shuffled"), ("keep_nocal", "shuffled"), ("keep_nocal", "singletons"),
                                        ("reverse_day", "order"), ("trunc_delta", "ns_h")])
def test_comparison_can_fail(wrong, name):
    """The device output misses a model with one thing wrong, in a column compared exactly."""
    bad = E.mismatches(E.frame_columns(device_cbs(name)), E.run_model(case(name), wrong=wrong))
    assert set(bad) & EXACT, (wrong, name, bad)
