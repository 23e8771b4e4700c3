"""The model of the event log -> CBS conversion (tests/elog_ref.py) pinned without a GPU: against the
reference's own outputs (tests/golden/elog_cases.npz, written by make_goldens.py), the vectorised
model against the loop model, the geometry every case promises, and the power of the comparison:
each of nine wrong models must differ from the right one in a column that is compared exactly."""
import functools

import numpy as np
import pytest

from tests import elog_ref as E
from tests.helpers import golden

EXACT = set(E.INT_COLS + E.BIT_COLS + E.HOLD_INT_COLS + E.HOLD_BIT_COLS) | {"rows"}


@functools.lru_cache(maxsize=None)
def case(name):
    return E.ELOG_CASES[name]()


@functools.lru_cache(maxsize=None)
def model(name, raw_ids=False):
    return E.run_model(case(name)[0], raw_ids=raw_ids)


def fixture_case(f, name):
    cols = [str(c) for c in f[f"{name}__columns"]]
    got = {c: f[f"{name}__{c}"] for c in cols}
    if got["cust"].dtype.kind == "U":
        got["cust"] = got["cust"].astype(object)
    return cols, [str(k) for k in f[f"{name}__kinds"]], got


@pytest.mark.parametrize("name", E.REFERENCE_CASES + ("shuffled_nosales",))
def test_model_matches_reference(name):
    """Row count, cust, x, first, x_star equal; t_x, T_cal, T_star and the sales columns bit for bit;
    litt within (litt_terms + 2) * 2^-52 * litt_abs (one ulp per log, fsum against pandas' sum);
    the column set and dtypes are the ones the device wrapper is held to."""
    f = golden("elog_cases.npz")
    with_sales = name != "shuffled_nosales"
    cols, kinds, got = fixture_case(f, name)
    want = E.run_model(case(name.replace("_nosales", ""))[0], with_sales=with_sales)
    ratio = []
    assert E.mismatches(got, want, ratio) == []
    assert ratio[0] <= float(f["litt_ratio_max"])  # the largest ratio the fixture step recorded
    exp = E.expected_dtypes(want["holdout"], with_sales, bool((want["x"] > 0).any()))
    assert cols == [c for c, _ in exp]
    assert kinds[1:] == [k for _, k in exp[1:]]


def test_reference_rows_are_what_the_cases_say():
    f = golden("elog_cases.npz")
    assert len(f["one__x"]) == 1 and f["one__x"][0] == 0 and f["one__t_x"][0] == 0.0 and f["one__litt"][0] == 0.0
    assert len(f["oneday__x"]) == 1 and f["oneday__x"][0] == 0 and f["oneday__t_x"][0] == 0.0
    inputs, _ = case("hog")
    g = E.geometry(inputs[0][inputs[0] == 7], inputs[1][inputs[0] == 7], *E.resolve_T(inputs[1], inputs[4], inputs[5]))
    hog = {c: f[f"hog__{c}"][f["hog__cust"] == 7] for c in ("x", "x_star")}
    assert 0 < hog["x"][0] + 1 + hog["x_star"][0] <= 3000 - g["merged"] < 3000
    assert "inverted__x_star" not in f.files and "nocal__x_star" not in f.files and "shuffled__x_star" in f.files
    assert list(f["labels__cust"]) == sorted(f["labels__cust"]) != sorted(f["labels__cust"], key=lambda s: int(s[1:]))


@pytest.mark.parametrize("name", ["shuffled", "ns_h", "hog", "singletons", "big_cut"])
def test_vectorised_model_equals_loop_model(name):
    if name == "big_cut":
        c, d, s, units, T_cal, T_tot = case("big")[0]
        inputs = (c[:20_000], d[:20_000], s[:20_000], units, T_cal, T_tot)
    else:
        inputs = case(name)[0]
    a, b = E.run_model(inputs), E.run_model(inputs, model=E.elog_model_vec)
    assert a.keys() == b.keys() and a["holdout"] == b["holdout"]
    for k in a:
        if k != "holdout":
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert a[k].tobytes() == b[k].tobytes(), k


def test_vectorised_model_refuses_inexact_sales():
    c, d, s, units, T_cal, T_tot = case("order")[0]
    with pytest.raises(AssertionError):
        E.run_model((c, d, s, units, T_cal, T_tot), model=E.elog_model_vec)
    with pytest.raises(AssertionError):
        E.run_model((c, d, s * 0 + 0.1, units, T_cal, T_tot), model=E.elog_model_vec)


@pytest.mark.parametrize("name", list(E.ELOG_CASES))
def test_geometry(name):
    """Every case has the geometry it promises (counts are lower bounds; events and customers exact)."""
    inputs, promise = case(name)
    cust, date_ns, sales, units, T_cal, T_tot = inputs
    assert len(cust) == len(date_ns) == len(sales)
    g = E.geometry(cust, date_ns, *E.resolve_T(date_ns, T_cal, T_tot))
    for k, v in promise.items():
        assert (g[k] == v) if k in ("events", "customers") else (g[k] >= v), (k, g[k], v)
    if g["events"] > 1 and g["customers"] > 1:
        assert not g["identity"]
    if name != "order":
        assert np.array_equal(sales * 4, np.rint(sales * 4)) and np.abs(sales).max() <= 1e6


def test_case_sizes_straddle_the_sort_limits():
    sizes = {k: case(k)[1]["events"] for k in E.ELOG_CASES}
    assert [sizes[f"edge256_{n}"] for n in (255, 256, 257)] == [255, 256, 257]
    assert [sizes[f"block_{n}"] for n in (1023, 1024, 1025)] == [E.BLOCK_SORT_LIMIT - 1, E.BLOCK_SORT_LIMIT,
                                                                E.BLOCK_SORT_LIMIT + 1] == [1023, 1024, 1025]
    assert [sizes[f"merge_edge_{n}"] for n in (1048576, 1048577)] == [E.MERGE_SORT_LIMIT, E.MERGE_SORT_LIMIT + 1]
    assert sizes["big"] == 1_300_000 > E.MERGE_SORT_LIMIT and case("big")[1]["customers"] == 160_000
    assert sizes["one"] == 1 and sizes["oneday"] == 500 and sizes["singletons"] == 2000 and sizes["order"] == 600


def test_shuffled_family_shares_one_log():
    a = case("shuffled")[0]
    for other in ("inverted", "nocal", "labels"):
        b = case(other)[0]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[0], np.array([int(s[1:]) for s in b[0]]) if other == "labels" else b[0])
    labels = case("labels")[0][0]
    first_seen = list(dict.fromkeys(labels.tolist()))
    assert first_seen != sorted(first_seen)


def test_order_case_shows_the_summation_order():
    """Each multi-event day of ``order`` is the triple (2^60, 1, -2^60); both day sums occur."""
    c, d, s, *_ = case("order")[0]
    days = {}
    for cc, dd, ss in zip(c.tolist(), d.tolist(), s.tolist()):
        days.setdefault((cc, dd), []).append(ss)
    multi = [v for v in days.values() if len(v) > 1]
    assert len(multi) == 100 and all(sorted(v) == [-2.0 ** 60, 1.0, 2.0 ** 60] for v in multi)
    sums = [(v[0] + v[1]) + v[2] for v in multi]
    assert set(sums) == {0.0, 1.0} and min(sums.count(0.0), sums.count(1.0)) >= 10


POWER = [("lt_cal", "shuffled"), ("lt_tot", "shuffled"), ("keep_nocal", "shuffled"), ("keep_nocal", "singletons"),
         ("unsigned_date", "ns_h"), ("unsigned_date", "ns_W"), ("unsigned_cust", "signed"), ("reverse_day", "order"),
         ("first_input", "shuffled"), ("trunc_delta", "ns_h"), ("trunc_delta", "ns_W"), ("no_merge", "shuffled")]


@pytest.mark.parametrize("wrong,name", POWER)
def test_power(wrong, name):
    """One thing wrong in the model is seen by the comparison, in a column compared exactly."""
    raw = name == "signed"
    bad = E.mismatches(E.run_model(case(name)[0], wrong=wrong, raw_ids=raw), model(name, raw))
    assert set(bad) & EXACT, (wrong, name, bad)


def test_signed_ids_order_as_signed():
    out = model("signed", True)
    assert out["cust"][0] == E.INT64_MIN and out["cust"][-1] == E.INT64_MAX and np.all(np.diff(out["cust"].astype(object)) > 0)
    assert {-5, 0, 7} <= set(out["cust"].tolist())
