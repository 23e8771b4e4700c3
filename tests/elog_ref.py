"""Yardstick of the event log -> CBS conversion (csrc/elog.hip ``clv_elog2cbs``, reached through
``data.elog2cbs``): a plain model of utils/elog2cbs2param.py:33-94 written from its equations, with
Python ints for every timestamp, plus the seeded cases the kernels are held to.

``elog_model``      the loop model (any input; the wrong models of the power checks are variants).
``elog_model_vec``  the same model in numpy (lexsort, add.reduceat) for the large cases; valid only
                    when every sales sum is exact in any order, which it asserts.
``ELOG_CASES``      name -> builder of ``(cust, date_ns, sales, units, T_cal, T_tot), geometry``.
``mismatches``      the comparison every test uses: integer columns equal, ratio and sales columns
                    bit for bit, litt within (litt_terms + 2) * 2^-52 * litt_abs.

Sales of every case but ``order`` are integers / 4 of magnitude <= 1e6, so each sum is exact in any
order and the sales columns are compared bit for bit; ``order`` holds (2^60, 1, -2^60) on each
multi-event day, so its day sums show the summation order.
"""
from __future__ import annotations

import math

import numpy as np

INT_COLS = ("cust", "x", "first")
BIT_COLS = ("t_x", "T_cal", "sales", "sales_x")
HOLD_INT_COLS = ("x_star",)
HOLD_BIT_COLS = ("T_star", "sales_star")
EPS = 2.0 ** -52
WRONG = ("lt_cal", "lt_tot", "keep_nocal", "unsigned_date", "unsigned_cust", "reverse_day", "first_input",
         "trunc_delta", "no_merge")


def unit_ns(units) -> int:
    return int(np.timedelta64(1, units).astype("timedelta64[ns]").astype(np.int64))


def stamp_ns(s) -> int:
    """Nanoseconds since the epoch of an ISO date string."""
    return int(np.datetime64(s, "ns").astype(np.int64))


def resolve_T(date_ns, T_cal, T_tot):
    """The reference's defaults (elog2cbs2param.py:49-57): a missing bound is the last event."""
    last = int(np.max(date_ns))
    return (last if T_cal is None else stamp_ns(T_cal)), (last if T_tot is None else stamp_ns(T_tot))


def _trunc_float(n: int) -> float:
    f = float(n)
    if abs(int(f)) > abs(n):
        f = math.nextafter(f, 0.0)
    return f


def elog_model(cust, date_ns, sales, unit_ns, T_cal_ns, T_tot_ns, wrong=None):
    """CBS of an event log.  ``cust`` and ``date_ns`` are integers (customers order as signed ints),
    ``sales`` floats or None (1 per event, integer sums).  Returns a dict of arrays, one row per
    customer with a calibration run, in customer order.  ``wrong`` names one deliberate defect."""
    assert wrong is None or wrong in WRONG
    cust = [int(c) for c in cust]
    date = [int(d) for d in date_ns]
    n = len(cust)
    one = sales is None
    val = [1] * n if one else [float(s) for s in sales]
    T_cal, T_tot, unit = int(T_cal_ns), int(T_tot_ns), float(int(unit_ns))
    ck = (lambda c: c % 2 ** 64) if wrong == "unsigned_cust" else (lambda c: c)
    dk = (lambda d: d % 2 ** 64) if wrong == "unsigned_date" else (lambda d: d)
    order = sorted(range(n), key=lambda i: (ck(cust[i]), dk(date[i]), i))
    # same-(cust, date) runs, sales summed sequentially in input order
    runs = []  # [cust, date, sum]
    for i in order:
        if runs and wrong != "no_merge" and runs[-1][0] == cust[i] and runs[-1][1] == date[i]:
            runs[-1][3].append(val[i])
        else:
            runs.append([cust[i], date[i], None, [val[i]]])
    for r in runs:
        s = 0 if one else 0.0
        for v in (reversed(r[3]) if wrong == "reverse_day" else r[3]):
            s += v
        r[2] = s
    first_in = {}
    for c, d in zip(cust, date):
        first_in.setdefault(c, d)
    to_f = _trunc_float if wrong == "trunc_delta" else float
    in_cal = (lambda d: d < T_cal) if wrong == "lt_cal" else (lambda d: d <= T_cal)
    in_tot = (lambda d: d < T_tot) if wrong == "lt_tot" else (lambda d: d <= T_tot)
    holdout = T_cal < T_tot
    zero = 0 if one else 0.0
    rows = []
    a = 0
    while a < len(runs):
        b = a
        while b < len(runs) and runs[b][0] == runs[a][0]:
            b += 1
        c = runs[a][0]
        first = first_in[c] if wrong == "first_input" else min((runs[k][1] for k in range(a, b)), key=dk)
        count = x_star = 0
        t_x, logs = -math.inf, []
        s_all, s_x, s_star = zero, zero, zero
        t_prev = 0.0
        for k in range(a, b):
            d, s = runs[k][1], runs[k][2]
            t = to_f(d - first) / unit
            itt = 0.0 if k == a else t - t_prev
            t_prev = t
            if in_cal(d):
                count += 1
                t_x = max(t_x, t)
                if itt > 0.0:
                    logs.append(math.log(itt))
                s_all += s
                if k > a:
                    s_x += s
            elif holdout and in_tot(d):
                x_star += 1
                s_star += s
        if count > 0 or wrong == "keep_nocal":
            Tc = to_f(T_cal - first) / unit
            rows.append((c, count - 1, t_x, math.fsum(logs), s_all, s_x, first, Tc,
                         to_f(T_tot - first) / unit - Tc, x_star, float(s_star),
                         math.fsum(abs(v) for v in logs), len(logs)))
        a = b
    return _pack(rows, holdout, one)


_ROW = ("cust", "x", "t_x", "litt", "sales", "sales_x", "first", "T_cal", "T_star", "x_star", "sales_star",
        "litt_abs", "litt_terms")
_I64 = ("cust", "x", "first", "x_star", "litt_terms")


def _pack(rows, holdout, one):
    cols = list(zip(*rows)) if rows else [()] * len(_ROW)
    out = {}
    for name, v in zip(_ROW, cols):
        isint = name in _I64 or (one and name in ("sales", "sales_x"))
        out[name] = np.array(v, dtype=np.int64 if isint else np.float64)
    if not holdout:
        for name in HOLD_INT_COLS + HOLD_BIT_COLS:
            del out[name]
    out["holdout"] = bool(holdout)
    return out


def elog_model_vec(cust, date_ns, sales, unit_ns, T_cal_ns, T_tot_ns):
    """``elog_model`` in numpy.  Sums go through add.reduceat in run order, which equals the loop
    model's sequential sums only when every partial sum is exact: sales must be multiples of 1/4
    whose absolute sum stays below 2^51."""
    cust = np.asarray(cust, dtype=np.int64)
    date = np.asarray(date_ns, dtype=np.int64)
    sales = np.asarray(sales, dtype=np.float64)
    assert np.array_equal(sales * 4.0, np.rint(sales * 4.0)), "sales are not multiples of 1/4"
    assert float(np.abs(sales).sum()) < 2.0 ** 51, "sales sums are not exact"
    assert int(date.max()) - int(date.min()) < 2 ** 63, "date differences overflow int64"
    T_cal, T_tot, unit = int(T_cal_ns), int(T_tot_ns), float(int(unit_ns))
    n = cust.size
    o = np.lexsort((date, cust))  # stable: ties keep input order
    cs, ds, ss = cust[o], date[o], sales[o]
    newc = np.ones(n, bool)
    newc[1:] = cs[1:] != cs[:-1]
    newr = newc.copy()
    newr[1:] |= ds[1:] != ds[:-1]
    rs = np.flatnonzero(newr)
    r_date, r_sum = ds[rs], np.add.reduceat(ss, rs)
    r_newc = newc[rs]
    c0 = np.flatnonzero(r_newc)  # first run of each customer
    seg = np.cumsum(r_newc) - 1
    first = r_date[c0]
    t = (r_date - first[seg]).astype(np.float64) / unit
    itt = np.zeros_like(t)
    itt[1:] = t[1:] - t[:-1]
    itt[c0] = 0.0
    holdout = T_cal < T_tot
    cal = r_date <= T_cal
    hold = ~cal & (r_date <= T_tot) if holdout else np.zeros_like(cal)
    count = np.add.reduceat(cal.astype(np.int64), c0)
    keep = count > 0
    pos = cal & (itt > 0.0)
    logs = [math.log(v) for v in itt[pos].tolist()]
    off = np.concatenate([[0], np.cumsum(np.add.reduceat(pos.astype(np.int64), c0))]).tolist()
    litt = np.array([math.fsum(logs[a:b]) for a, b in zip(off[:-1], off[1:])])
    labs = np.array([math.fsum(map(abs, logs[a:b])) for a, b in zip(off[:-1], off[1:])])
    Tc = (T_cal - first).astype(np.float64) / unit
    out = dict(cust=cs[rs][c0], x=count - 1, t_x=np.maximum.reduceat(np.where(cal, t, -np.inf), c0), litt=litt,
               sales=np.add.reduceat(np.where(cal, r_sum, 0.0), c0),
               sales_x=np.add.reduceat(np.where(cal & ~r_newc, r_sum, 0.0), c0), first=first, T_cal=Tc)
    if holdout:
        out.update(T_star=(T_tot - first).astype(np.float64) / unit - Tc,
                   x_star=np.add.reduceat(hold.astype(np.int64), c0),
                   sales_star=np.add.reduceat(np.where(hold, r_sum, 0.0), c0))
    out.update(litt_abs=labs, litt_terms=np.diff(np.asarray(off, dtype=np.int64)))
    out = {k: v[keep] for k, v in out.items()}
    out["holdout"] = bool(holdout)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mismatches(got, want, litt_ratio=None):
    """Names of the columns of ``got`` that miss ``want`` (a model's output): a different column set
    or row count reports "columns" / "rows"; integer columns must be equal, ratio and sales columns
    equal bit for bit, litt within (litt_terms + 2) * 2^-52 * litt_abs.  ``litt_ratio``, a list,
    receives the largest |litt - want| / (2^-52 * litt_abs)."""
    hold = (HOLD_INT_COLS + HOLD_BIT_COLS) if want["holdout"] else ()
    if any((c in got) != (c in hold) for c in HOLD_INT_COLS + HOLD_BIT_COLS):
        return ["columns"]
    if len(got["cust"]) != len(want["cust"]):
        return ["rows"]
    bad = []
    for c in INT_COLS + tuple(h for h in hold if h in HOLD_INT_COLS):
        if not np.array_equal(np.asarray(got[c]), np.asarray(want[c])):
            bad.append(c)
    for c in BIT_COLS + tuple(h for h in hold if h in HOLD_BIT_COLS):
        if not np.array_equal(bits(got[c]), bits(want[c])):
            bad.append(c)
    err = np.abs(np.asarray(got["litt"], dtype=np.float64) - want["litt"])
    if not np.all(err <= (want["litt_terms"] + 2) * EPS * want["litt_abs"]):
        bad.append("litt")
    if litt_ratio is not None and err.size:
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err > 0, err / (EPS * want["litt_abs"]), 0.0)
        litt_ratio.append(float(r.max()))
    return bad


def frame_columns(df):
    """A CBS DataFrame (the reference's or ``data.elog2cbs``'s) as the dict ``mismatches`` takes."""
    out = {}
    for c in df.columns:
        out[c] = df[c].to_numpy(dtype="datetime64[ns]").view(np.int64) if c == "first" else df[c].to_numpy()
    return out


def expected_dtypes(holdout, with_sales=True, any_repeat=True):
    """Column order and dtype kinds of the reference's CBS (``cust`` follows the input's labels).
    ``any_repeat``: some row has x > 0; when none has, every sales_x is the integer 0 of
    elog2cbs2param.py:79 and the reference's column is int64."""
    s = "f" if with_sales else "i"
    cols = [("cust", None), ("x", "i"), ("t_x", "f"), ("litt", "f"), ("sales", s),
            ("sales_x", s if any_repeat else "i"), ("first", "M"), ("T_cal", "f")]
    if holdout:
        cols += [("T_star", "f"), ("x_star", "f"), ("sales_star", "f")]
    return cols


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
DAY = 86_400 * 10 ** 9
D1997 = stamp_ns("1997-01-01")


def _sales(rng, n):
    return rng.integers(-4_000_000, 4_000_001, size=n).astype(np.float64) / 4.0


def _log(rng, n, n_cust, n_days=540, birth_days=400, base=D1997):
    """n events of n_cust customers at midnights: every customer has at least one event, a birth day
    in [0, birth_days) and its events uniform on [birth, n_days); rows in random order."""
    c = np.concatenate([np.arange(n_cust), rng.integers(0, n_cust, size=n - n_cust)])
    c = c[rng.permutation(n)]
    birth = rng.integers(0, birth_days, size=n_cust)
    day = birth[c] + np.floor(rng.random(n) * (n_days - birth[c])).astype(np.int64)
    ids = rng.permutation(n_cust).astype(np.int64) * 3 + 11  # ids in neither input nor code order
    return ids[c], base + day * DAY, _sales(rng, n)


def geometry(cust, date_ns, T_cal_ns, T_tot_ns):
    """Facts about a log that the cases promise (dates within a few centuries of each other)."""
    cust = encode(cust)[0]
    date = np.asarray(date_ns, dtype=np.int64)
    n = cust.size
    o = np.lexsort((date, cust))
    by_c = np.argsort(cust, kind="stable")  # input order within each customer
    same = cust[by_c][1:] == cust[by_c][:-1]
    cs, ds = cust[o], date[o]
    newc = np.ones(n, bool)
    newc[1:] = cs[1:] != cs[:-1]
    newr = newc.copy()
    newr[1:] |= ds[1:] != ds[:-1]
    run_len = np.diff(np.append(np.flatnonzero(newr), n))
    firsts = ds[newc]  # by code
    delta = date - firsts[cust]
    return dict(events=n, customers=int(firsts.size), identity=bool(np.array_equal(o, np.arange(n))),
                inversions=int(np.sum(same & (date[by_c][1:] < date[by_c][:-1]))),
                dropped=int(np.sum(firsts > T_cal_ns)),
                after_tot=int(np.sum(date > T_tot_ns)), on_cal=int(np.sum(date == T_cal_ns)),
                on_tot=int(np.sum(date == T_tot_ns)), runs_ge3=int(np.sum(run_len >= 3)),
                merged=int(n - newr.sum()), negative=int(np.sum(date < 0)),
                big_odd_delta=int(np.sum((delta > 2 ** 53) & (delta % 2 == 1))))


def case_one():
    return ((np.array([42]), np.array([D1997 + 17 * DAY]), np.array([12.25]), "W", None, None),
            dict(events=1, customers=1))


def _sized(seed, n, n_cust):
    def build():
        rng = np.random.default_rng(seed)
        c, d, s = _log(rng, n, n_cust)
        return (c, d, s, "W", "1997-09-30", "1998-03-31"), dict(events=n, customers=n_cust, inversions=1, dropped=1)
    return build


def case_shuffled(units="W", T_cal="1997-09-30", T_tot="1998-03-31", labels=False):
    rng = np.random.default_rng(20261104)
    n, n_cust = 3000, 300
    c, d, s = _log(rng, n, n_cust)
    on_cal, on_tot = stamp_ns("1997-09-30"), stamp_ns("1998-03-31")
    # same-day runs of three: the first three events (input order) of 40 customers share a date
    by_c = np.argsort(c, kind="stable")
    starts = np.flatnonzero(np.r_[True, c[by_c][1:] != c[by_c][:-1]])
    sizes = np.diff(np.append(starts, n))
    free = np.ones(n, bool)
    for k in rng.permutation(np.flatnonzero(sizes >= 6))[:40]:
        i = by_c[starts[k]:starts[k] + 3]
        d[i] = d[i].max()
        free[i] = False
    # 30 events exactly on T_cal and 30 on T_tot, of customers born earlier, never a customer's first
    born = {}
    for cc, dd in zip(c.tolist(), d.tolist()):
        born[cc] = min(born.get(cc, dd), dd)
    born = np.array([born[cc] for cc in c.tolist()])
    for target in (on_cal, on_tot):
        ok = np.flatnonzero(free & (born < on_cal) & (d != born))
        pick = rng.permutation(ok)[:30]
        d[pick] = target
        free[pick] = False
    if labels:
        c = np.array([f"c{v}" for v in c.tolist()], dtype=object)
    promise = dict(events=n, customers=n_cust, inversions=100, runs_ge3=20)
    if (T_cal, T_tot) == ("1997-09-30", "1998-03-31"):
        promise.update(dropped=20, after_tot=20, on_cal=20, on_tot=20)
    return (c, d, s, units, T_cal, T_tot), promise


def case_inverted():
    return case_shuffled("D", "1998-03-31", "1997-09-30")


def case_nocal():
    return case_shuffled("W", None, None)


def case_labels():
    return case_shuffled(labels=True)


def _case_ns(units):
    def build():
        rng = np.random.default_rng(20261105)
        n, n_cust = 3000, 200
        base = stamp_ns("1969-06-01")
        c = np.concatenate([np.arange(n_cust), rng.integers(0, n_cust, size=n - n_cust)])[rng.permutation(n)]
        c = c.astype(np.int64) * 5 - 300
        d = base + rng.integers(0, 400 * DAY, size=n)
        dup = rng.permutation(n)[:n // 5]  # exact duplicates of another event's (cust, date)
        src = rng.integers(0, n, size=dup.size)
        c[dup], d[dup] = c[src], d[src]
        T_cal, T_tot = "1970-01-15 03:04:05.000000007", "1970-05-01 12:00:00.000000003"
        edge = rng.permutation(n)[:12]  # six events on each bound, to the nanosecond
        d[edge[:6]], d[edge[6:]] = stamp_ns(T_cal), stamp_ns(T_tot)
        return ((c, d, _sales(rng, n), units, T_cal, T_tot),
                dict(events=n, inversions=100, negative=100, big_odd_delta=1, merged=300, after_tot=20, on_cal=6,
                     on_tot=6))
    return build


def case_hog():
    rng = np.random.default_rng(20261106)
    base = stamp_ns("1995-01-01")
    c = np.concatenate([np.full(3000, 7), 1000 + np.arange(50)]).astype(np.int64)
    day = np.concatenate([rng.integers(0, 1500, size=3000), rng.integers(0, 1500, size=50)])
    p = rng.permutation(3050)
    return ((c[p], base + day[p] * DAY, _sales(rng, 3050), "D", "1998-01-01", "1998-12-31"),
            dict(events=3050, customers=51, inversions=100, merged=100, dropped=1))


def case_oneday():
    rng = np.random.default_rng(20261107)
    return ((np.full(500, 3), np.full(500, D1997 + 100 * DAY), _sales(rng, 500), "W", None, None),
            dict(events=500, customers=1, merged=499))


def case_singletons():
    rng = np.random.default_rng(20261108)
    n = 2000
    c = rng.permutation(n).astype(np.int64) + 1
    day = rng.integers(0, 400, size=n)
    return ((c, D1997 + day * DAY, _sales(rng, n), "W", "1997-07-20", "1997-12-31"),
            dict(events=n, customers=n, dropped=900, after_tot=50))


def case_order():
    """600 events of 40 customers: 100 days hold the triple (2^60, 1, -2^60) in seeded order, 300 days
    one event; a day sum is 1 when the two large terms meet first and 0 otherwise."""
    rng = np.random.default_rng(20261109)
    c, d, s = [], [], []
    for k in range(400):
        cust, day = k % 40, (k // 40) * 7 + (k % 40) % 5
        vals = rng.permutation([2.0 ** 60, 1.0, -2.0 ** 60]).tolist() if k % 4 == 0 else [float(rng.integers(-400, 401)) / 4.0]
        for v in vals:
            c.append(cust), d.append(D1997 + day * DAY), s.append(v)
    p = rng.permutation(len(c))
    return ((np.array(c, dtype=np.int64)[p], np.array(d, dtype=np.int64)[p], np.array(s)[p], "D", "1997-02-05",
             "1997-03-01"), dict(events=600, customers=40, runs_ge3=100, inversions=100))


INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


def case_signed():
    """2,000 events whose customer ids span the int64 range (C ABI only: no factorisation)."""
    rng = np.random.default_rng(20261110)
    ids = np.concatenate([np.array([INT64_MIN, -5, 0, 7, INT64_MAX], dtype=np.int64),
                          rng.integers(INT64_MIN, INT64_MAX, size=95, dtype=np.int64, endpoint=True)])
    n = 2000
    c = ids[np.concatenate([np.arange(100), rng.integers(0, 100, size=n - 100)])[rng.permutation(n)]]
    day = rng.integers(0, 540, size=n)
    return ((c, D1997 + day * DAY, _sales(rng, n), "W", "1997-09-30", "1998-03-31"),
            dict(events=n, customers=100, inversions=100))


def _big(seed, n, n_cust):
    def build():
        rng = np.random.default_rng(seed)
        c, d, s = _log(rng, n, n_cust)
        return ((c, d, s, "W", "1997-09-30", "1998-03-31"),
                dict(events=n, customers=n_cust, inversions=1000, dropped=1000, after_tot=1000))
    return build


BLOCK_SORT_LIMIT = 1024          # rocprim::radix_sort_pairs: one-block sort up to 256 x 4 items
MERGE_SORT_LIMIT = 1024 * 1024   # merge sort up to here, onesweep above

ELOG_CASES = {
    "one": case_one,
    "edge256_255": _sized(101, 255, 60), "edge256_256": _sized(102, 256, 60), "edge256_257": _sized(103, 257, 60),
    "block_1023": _sized(111, BLOCK_SORT_LIMIT - 1, 120), "block_1024": _sized(112, BLOCK_SORT_LIMIT, 120),
    "block_1025": _sized(113, BLOCK_SORT_LIMIT + 1, 120),
    "shuffled": case_shuffled, "inverted": case_inverted, "nocal": case_nocal,
    "ns_h": _case_ns("h"), "ns_W": _case_ns("W"),
    "hog": case_hog, "oneday": case_oneday, "singletons": case_singletons, "labels": case_labels,
    "order": case_order, "signed": case_signed,
    "big": _big(141, 1_300_000, 160_000),
    "merge_edge_1048576": _big(151, MERGE_SORT_LIMIT, 100_000),
    "merge_edge_1048577": _big(152, MERGE_SORT_LIMIT + 1, 100_000),
}
REFERENCE_CASES = tuple(k for k in ELOG_CASES if k not in ("order", "signed", "big") and not k.startswith("merge_edge"))
VEC_CASES = ("big", "merge_edge_1048576", "merge_edge_1048577")


def encode(cust):
    """(codes, labels): labels sorted, as ``pd.factorize(sort=True)`` orders them."""
    labels, codes = np.unique(np.asarray(cust), return_inverse=True)
    return codes.astype(np.int64), labels


def run_model(inputs, model=None, wrong=None, with_sales=True, raw_ids=False):
    """A case's inputs through a model.  The customers reach it as sorted codes, as they reach the
    kernel through ``data.elog2cbs``, and come back as the input's labels; ``raw_ids`` passes the
    integer ids themselves, as the C ABI takes them."""
    cust, date_ns, sales, units, T_cal, T_tot = inputs
    codes, labels = (np.asarray(cust, dtype=np.int64), None) if raw_ids else encode(cust)
    Tc, Tt = resolve_T(date_ns, T_cal, T_tot)
    if model is elog_model_vec:
        assert with_sales and wrong is None
        out = elog_model_vec(codes, date_ns, sales, unit_ns(units), Tc, Tt)
    else:
        out = elog_model(codes, date_ns, sales if with_sales else None, unit_ns(units), Tc, Tt, wrong=wrong)
    if labels is not None:
        out["cust"] = labels[out["cust"]]
    return out
