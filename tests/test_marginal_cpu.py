"""The marginal likelihood without a GPU: the Gauss-Hermite table, the float64
model (tests/marginal_ref.py) against the exact fixture and its 40-digit twin, the spend term's closed
form, the argument checks of the C ABI and of the Python layer, compare_models' refusal to mix kinds,
the maximum-likelihood entry and the statistics of a model matrix."""
import ctypes
import functools
import importlib.util
import math
import os

import numpy as np
import pandas as pd
import pytest

from tests import helpers, ic_ref, pnbd_ref
from tests import marginal_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "clvmcmc.h")
NEW_SYMBOLS = ("clv_marginal_loglik", "clv_marginal_information_criteria", "clv_marginal_information_criteria_sampler",
               "clv_marginal_info", "clv_debug_marginal_loglik")
TARGET = 1e-6   # the quadrature error the default order meets on the CDNOW-like family (absolute, in l_marg)


@functools.lru_cache(maxsize=None)
def exact():
    return helpers.golden("marginal_exact.npz")


@functools.lru_cache(maxsize=None)
def model_bi(nodes):
    f = exact()
    return M.marginal_loglik(f["bi_k1_level2"], 2, 1, None, f["bi_k1_x"], f["bi_k1_t_x"], f["bi_k1_T_cal"], nodes=nodes)


@functools.lru_cache(maxsize=None)
def model_tri(nodes, spend):
    f = exact()
    return M.marginal_loglik(f["tri_k3_level2"], 3, 3, f["tri_k3_cov"], f["tri_k3_x"], f["tri_k3_t_x"], f["tri_k3_T_cal"],
                             f["tri_k3_log_s"] if spend else None, float(f["tri_k3_omega2"]), nodes=nodes)


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_symbols():
    import mcmc_clv_model_amd as pkg
    from mcmc_clv_model_amd import _lib, analysis
    names = _lib.exported_symbols()
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} not declared in include/clvmcmc.h"
        assert hasattr(L, n), f"{n} not exported by the library"
    with open(HDR) as f:
        text = " ".join(f.read().split())
    assert "#define CLV_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2   # additions only: no bump
    assert f"#define CLV_MARGINAL_DEFAULT_NODES {_lib.MARGINAL_DEFAULT_NODES}" in text
    assert f"#define CLV_MARGINAL_NEWTON {_lib.MARGINAL_NEWTON}" in text
    for fn in ("marginal_log_likelihood", "marginal_information_criteria", "marginal_log_score"):
        assert fn in analysis.__all__ and fn in pkg.__all__ and callable(getattr(pkg, fn))
    info = _lib.marginal_info()
    assert info["orders"] == _lib.MARGINAL_ORDERS == M.ORDERS
    assert info["default_nodes"] == _lib.MARGINAL_DEFAULT_NODES == M.DEFAULT_ORDER
    assert info["newton"] == _lib.MARGINAL_NEWTON == M.NEWTON_STEPS
    assert (info["block"], info["max_records"]) == (_lib.MARGINAL_BLOCK, _lib.MARGINAL_MAX_RECORDS)
    assert L.clv_marginal_info(None) == -1


def test_c_abi_rejects_bad_arguments_before_any_device_call():
    from mcmc_clv_model_amd import _lib
    from mcmc_clv_model_amd._lib import dptr
    L = _lib.lib()
    n, R = 3, 8
    l2, l3 = np.ones((R, 5)), np.ones((R, 9))
    cov = np.zeros((1, n))
    x = np.zeros(n, np.int32)
    tx, T, ls = np.zeros(n), np.ones(n), np.zeros(n)
    out, ic = np.empty((R, n)), np.empty((n, 7))
    i32 = x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def args(l2p=dptr(l2), D=2, K=1, covp=None, R_=R, n_=n, xp=i32, txp=dptr(tx), Tp=dptr(T), lsp=None, w2=1.0, nodes=0):
        return (0, l2p, D, K, covp, R_, n_, xp, txp, Tp, lsp, w2, nodes)
    bads = (dict(l2p=None), dict(D=1), dict(D=4), dict(K=0), dict(K=10), dict(K=2), dict(covp=dptr(cov)),
            dict(lsp=dptr(ls)), dict(l2p=dptr(l3), D=3, lsp=dptr(ls), w2=0.0),
            dict(l2p=dptr(l3), D=3, lsp=dptr(ls), w2=float("nan")), dict(nodes=12), dict(nodes=-8), dict(nodes=64),
            dict(R_=0), dict(n_=0), dict(R_=(1 << 20) + 1), dict(n_=1 << 31), dict(xp=None), dict(txp=None), dict(Tp=None))
    for bad in bads:
        assert L.clv_marginal_loglik(*args(**bad), dptr(out)) == -1, bad
        assert L.clv_last_error()
        assert L.clv_marginal_information_criteria(*args(**bad), 1.0, dptr(ic)) == -1, bad
        assert L.clv_debug_marginal_loglik(*args(**bad), 0, 0, dptr(out), None) == -1, bad
    assert L.clv_marginal_loglik(*args(), None) == -1
    assert L.clv_debug_marginal_loglik(*args(), -1, 0, dptr(out), None) == -1
    assert L.clv_debug_marginal_loglik(*args(), 0, -1, dptr(out), None) == -1
    # the fused entry: the S limits of clv_ic_info and reff
    for bad, reff in ((dict(R_=7), 1.0), (dict(), 0.0), (dict(), float("inf")), (dict(R_=1 << 20), 1e-6)):
        assert L.clv_marginal_information_criteria(*args(**bad), reff, dptr(ic)) == -1, (bad, reff)
    assert L.clv_marginal_information_criteria(*args(), 1.0, None) == -1
    assert L.clv_marginal_information_criteria_sampler(None, 0, 1.0, 1.0, 0, dptr(ic)) == -1


# ---- the table -------------------------------------------------------------------------------------
def test_gauss_hermite_table_against_numpy_and_the_monomials():
    import mpmath as mp
    mp.mp.dps = 40
    tabs = M.gh_tables()
    assert tuple(tabs) == M.ORDERS
    for Q, (t, w, c) in tabs.items():
        tn, wn = np.polynomial.hermite.hermgauss(Q)
        # numpy's own nodes and weights are good to a few ulp of the largest node and to about 1e-14
        assert np.abs(t - tn).max() <= 4 * np.spacing(np.abs(tn).max())
        assert np.abs(w / wn - 1.0).max() <= 1e-13
        assert np.all(np.diff(t) > 0) and np.array_equal(t, -t[::-1]) and np.array_equal(w, w[::-1])
        tm, wm = [mp.mpf(float(v)) for v in t], [mp.mpf(float(v)) for v in w]
        # c is log(w) + t^2 rounded once from 40 digits; t and w were rounded before: 2 |t| ulp(t) + ulp(w) / w
        for tj, wj, cj in zip(tm, wm, c):
            assert abs(mp.log(wj) + tj * tj - mp.mpf(float(cj))) <= 2.0 ** -52 * (2 * tj * tj + 2) + 2.0 ** -53 * abs(float(cj))
        # the rule is exact for the monomials up to degree 2 Q - 1: int t^k exp(-t^2) = Gamma((k + 1) / 2), k even.
        # With nodes and weights rounded to double each term moves by (k + 1) ulp at the most.
        for k in range(2 * Q):
            terms = [wj * tj ** k for tj, wj in zip(tm, wm)]
            want = mp.gamma(mp.mpf(k + 1) / 2) if k % 2 == 0 else mp.mpf(0)
            assert abs(mp.fsum(terms) - want) <= (k + 1) * 2.0 ** -52 * mp.fsum(abs(v) for v in terms), (Q, k)


def test_gauss_hermite_header_is_what_the_tool_writes():
    spec = importlib.util.spec_from_file_location("make_gauss_hermite", os.path.join(ROOT, "tools", "make_gauss_hermite.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.HEADER) as f:
        assert f.read() == tool.render()


# ---- the model against the exact integral ----------------------------------------------------------
def quadrature_errors():
    """{order: (worst CDNOW-like, worst wide)} |model - exact| over the fixture."""
    f = exact()
    fam = f["bi_k1_family"]
    out = {}
    for Q in M.ORDERS:
        e_bi = np.abs(model_bi(Q)[0] - f["bi_k1_exact"])
        e_tri = max(np.abs(model_tri(Q, True)[0] - f["tri_k3_exact"]).max(),
                    np.abs(model_tri(Q, False)[0] - f["tri_k3_exact_tx"]).max())
        out[Q] = (max(e_bi[fam == 0].max(), e_tri), e_bi[fam == 1].max())
    return out


def test_fixture_is_what_the_issue_asks_for():
    f = exact()
    assert float(f["panel_gap"]) < 1e-14                      # doubling the panels changed nothing
    x, tx, T = f["bi_k1_x"], f["bi_k1_t_x"], f["bi_k1_T_cal"]
    rows = set(zip(x.tolist(), tx.tolist(), T.tolist()))
    assert (0, 0.0, 39.0) in rows and (1, 39.0, 39.0) in rows and (40, 2.0, 39.0) in rows
    assert (2000, 3649.0, 3650.0) in rows and any(r[0] == 20000 for r in rows)
    assert any(r[0] == 1 and 0 < r[2] - r[1] < 1e-9 for r in rows)     # t_x just under T_cal
    assert set(f["bi_k1_family"].tolist()) == {0, 1}
    for k in ("bi_k1_exact", "tri_k3_exact", "tri_k3_exact_tx"):
        assert np.isfinite(f[k]).all()


def test_model_meets_the_target_at_the_default_order_and_not_below():
    err = quadrature_errors()
    for Q in M.ORDERS:
        print(f"order {Q}: worst |model - exact|  CDNOW-like {err[Q][0]:.3g}  wide {err[Q][1]:.3g}")
    assert err[M.DEFAULT_ORDER][0] <= TARGET
    for Q in M.ORDERS:
        if Q < M.DEFAULT_ORDER:
            assert err[Q][0] > TARGET, f"order {Q} already meets the target: it should be the default"
    for a, b in zip(M.ORDERS[:-1], M.ORDERS[1:]):            # more nodes never hurt, in either family
        assert err[b][0] <= err[a][0] and err[b][1] <= err[a][1]


def test_newton_reaches_the_mode_within_its_budget():
    for cen in (model_bi(M.DEFAULT_ORDER)[1], model_tri(M.DEFAULT_ORDER, True)[1]):
        assert cen[..., 5].max() < M.NEWTON_STEPS - 2 and cen[..., 11].max() < M.NEWTON_STEPS - 2
        assert np.all(cen[..., [2, 4, 8, 10]] > 0)


def test_rounding_unit_against_the_twin():
    """The model's deviation from the same rule summed in 40 digits at the model's own centre, relative
    to max(1, |l_marg|): every bivariate cell at order 8, every fourth at the default order, the
    trivariate cells with the spend term at order 8."""
    f = exact()
    worst = 0.0
    R, n = f["bi_k1_exact"].shape
    every = [(r, i) for r in range(R) for i in range(n)]
    for Q, cells in ((8, every), (M.DEFAULT_ORDER, every[::4])):
        lm, cen = model_bi(Q)
        tw = M.twin(f["bi_k1_level2"], 2, 1, None, f["bi_k1_x"], f["bi_k1_t_x"], f["bi_k1_T_cal"], None, 1.0, Q, cen, cells)
        got = np.array([lm[r, i] for r, i in cells])
        worst = max(worst, float((np.abs(got - tw) / np.maximum(1.0, np.abs(tw))).max()))
    lm, cen = model_tri(8, True)
    cells = [(r, i) for r in range(lm.shape[0]) for i in range(lm.shape[1])]
    tw = M.twin(f["tri_k3_level2"], 3, 3, f["tri_k3_cov"], f["tri_k3_x"], f["tri_k3_t_x"], f["tri_k3_T_cal"],
                f["tri_k3_log_s"], float(f["tri_k3_omega2"]), 8, cen, cells)
    got = np.array([lm[r, i] for r, i in cells])
    worst = max(worst, float((np.abs(got - tw) / np.maximum(1.0, np.abs(tw))).max()))
    print(f"rounding unit: {worst:.3g} (recorded: {M.UNIT_REL:.3g})")
    assert worst <= M.UNIT_REL


def test_spend_term_alone_is_the_closed_form_normal_density():
    """x = 0 and t_x = T_cal = 0: the transaction likelihood is 1, so the integral is
    N(log_s; m_3, Sigma_33 + omega2).  The two components (mu / (lambda + mu) and lambda / (lambda + mu))
    are still integrated by quadrature: held to the accuracy target."""
    f = exact()
    rec, cov = f["tri_k3_level2"], f["tri_k3_cov"]
    n = cov.shape[1]
    ls, w2 = f["tri_k3_log_s"], float(f["tri_k3_omega2"])
    zero = np.zeros(n)
    lm, _ = M.marginal_loglik(rec, 3, 3, cov, np.zeros(n, np.int32), zero, zero, ls, w2)
    for r in range(rec.shape[0]):
        beta, Sigma = rec[r, :9].reshape(3, 3).T, rec[r, 14]
        m3 = beta[0, 2] + cov[0] * beta[1, 2] + cov[1] * beta[2, 2]
        v = Sigma + w2
        want = -0.5 * np.log(2.0 * np.pi * v) - (ls - m3) ** 2 / (2.0 * v)
        assert np.abs(lm[r] - want).max() <= TARGET
    # and without the spend term the integral of the prior alone is 1
    lm0, _ = M.marginal_loglik(rec, 3, 3, cov, np.zeros(n, np.int32), zero, zero)
    assert np.abs(lm0).max() <= TARGET


def test_nan_cells_of_the_model():
    f = exact()
    rec = f["bi_k1_level2"][:3].copy()
    rec[1, 3] = 2.0 * np.sqrt(rec[1, 2] * rec[1, 4])          # |rho| = 2: not positive definite
    tx = f["bi_k1_t_x"].copy()
    tx[4] = np.nan
    lm, _ = M.marginal_loglik(rec, 2, 1, None, f["bi_k1_x"], tx, f["bi_k1_T_cal"])
    bad = np.zeros(lm.shape, bool)
    bad[1, :] = True
    bad[:, 4] = True
    assert np.array_equal(np.isnan(lm), bad)
    assert np.array_equal(lm[0, [0, 1, 2, 3, 5]], model_bi(M.DEFAULT_ORDER)[0][0, [0, 1, 2, 3, 5]])


# ---- the Python layer ------------------------------------------------------------------------------
def frames(elpd, kind=None):
    from mcmc_clv_model_amd import analysis as A
    stats = np.zeros((len(elpd), 7))
    stats[:, 2] = stats[:, 3] = elpd
    out = A.ic_frames(stats, 100)
    if kind:
        out["kind"] = kind
    return out


def test_compare_models_refuses_to_mix_kinds():
    from mcmc_clv_model_amd import analysis as A
    a, b = frames(np.array([-1.0, -2.0, -3.0])), frames(np.array([-1.5, -2.0, -2.0]))
    m1, m2 = frames(np.array([-1.0, -2.5, -3.0]), "marginal"), frames(np.array([-1.5, -2.0, -2.5]), "marginal")
    assert list(A.compare_models({"a": a, "b": b}).index) == ["b", "a"]            # today's calls: untouched
    assert list(A.compare_models({"a": a, "c": frames(np.array([-9.0, 0.0, 0.0]), "conditional")}).index) == ["a", "c"]
    assert list(A.compare_models({"m1": m1, "m2": m2}).index) == ["m2", "m1"]
    with pytest.raises(ValueError, match="marginal.*conditional|conditional.*marginal") as e:
        A.compare_models({"a": a, "m1": m1})
    assert "'a'" in str(e.value) and "'m1'" in str(e.value)


def test_mle_entry_totals_and_comparison():
    from mcmc_clv_model_amd import analysis as A
    from mcmc_clv_model_amd import mle
    df = helpers.cdnow("abe", 300)
    x, tx, T = df["x"].to_numpy(), df["t_x"].to_numpy(float), df["T_cal"].to_numpy(float)
    params = np.array([0.55, 10.6, 0.61, 11.7])
    ll = pnbd_ref.model_customers(x, tx, T, params)["logL"]
    ic = mle.mle_information_criteria(ll)
    assert ic["kind"] == "marginal" and list(ic["pointwise"].columns) == list(A.ic_frames(np.zeros((1, 7)), 100)["pointwise"].columns)
    total = pnbd_ref.device_sum(ll)                               # eval's sums[0] (unit weights), in its order
    for key in ("waic", "loo"):
        row = ic[key].iloc[0]
        assert abs(row["elpd"] - (total - 4.0)) <= 8 * np.spacing(abs(total))
        assert abs(row["p"] - 4.0) <= 1e-12 and row["n_data_points"] == 300 and not row["warning"] and row["n_bad_k"] == 0
    assert np.isnan(ic["pointwise"]["pareto_k"]).all()
    assert np.array_equal(ic["pointwise"]["lppd"].to_numpy(), ll)
    hb = frames(ll + 0.01, "marginal")
    assert list(A.compare_models({"HB": hb, "Pareto/NBD (MLE)": ic}).index) == ["HB", "Pareto/NBD (MLE)"]
    with pytest.raises(ValueError):
        A.compare_models({"HB conditional": frames(ll), "Pareto/NBD (MLE)": ic})
    assert "in-sample" in mle.ParetoNBDFitter.information_criteria.__doc__.lower()


@pytest.mark.parametrize("kw, match", [
    (dict(nodes=12), "nodes"), (dict(nodes=24.5), "nodes"), (dict(spend=True), "trivariate"),
    (dict(omega2=1.0), "omega2"), (dict(covariates=["nope"], K=2), "no column"), (dict(covariates=["c1"]), "match neither")])
def test_python_rejects_bad_arguments(kw, match):
    from mcmc_clv_model_amd import analysis as A
    df, _ = M.case_customers(10, 2, 3)
    kw = dict(kw)
    draws = dict(level_2=[M.case_records(8, 2, kw.pop("K", 1), 5)])
    cov = kw.pop("covariates", None)
    for fn in (A.marginal_log_likelihood, A.marginal_information_criteria, A.marginal_log_score):
        with pytest.raises(ValueError, match=match):
            fn(draws, df, cov, **kw)


def test_python_rejects_bad_shapes():
    from mcmc_clv_model_amd import analysis as A
    df, _ = M.case_customers(10, 2, 3)
    draws = dict(level_2=[M.case_records(8, 2, 1, 5)])
    with pytest.raises(ValueError, match="reff"):
        A.marginal_information_criteria(draws, df, reff=0.0)
    with pytest.raises(ValueError, match="stacked draws"):
        A.marginal_information_criteria(dict(level_2=[M.case_records(7, 2, 1, 5)]), df)
    with pytest.raises(ValueError, match="log_s"):
        A.marginal_log_likelihood(dict(level_2=[M.case_records(8, 3, 1, 5)]), df.drop(columns=["log_s"]), spend=True)


def test_fit_keyword_is_validated_before_the_run():
    from mcmc_clv_model_amd import sampler as S
    assert S.marginal_information_criteria_kwargs(None, "full", 2) is None
    assert S.marginal_information_criteria_kwargs(True, "full", 2) == {}
    assert S.marginal_information_criteria_kwargs(dict(nodes=32, reff=0.5), "full", 2) == dict(nodes=32, reff=0.5)
    for bad, sink, D in ((True, "summary", 2), (dict(spend=True), "full", 2), (dict(nodes=7), "full", 2),
                         (dict(reff=-1.0), "full", 3), (dict(k_hist=3), "full", 2), ("yes", "full", 2)):
        with pytest.raises(ValueError):
            S.marginal_information_criteria_kwargs(bad, sink, D)


# ---- the statistics of a model matrix --------------------------------------------------------------
def test_statistics_of_a_model_matrix():
    """WAIC / PSIS-LOO of the model's matrix through tests/ic_ref.py: lppd is the log score of the
    records, a NaN cell voids its customer alone, and with the records this close together the
    importance ratios are nearly flat — p_loo is a small fraction of one observation."""
    df, names = M.case_customers(40, 1, 3)
    cov, x, tx, T, _ = M.case_arrays(df, names, False)
    recs = M.case_records(32, 2, 1, 9)
    lm, _ = M.marginal_loglik(recs, 2, 1, cov, x, tx, T)
    st = ic_ref.model(lm)
    assert np.isfinite(st[:, :5]).all()
    assert np.abs(st[:, 0] - M.log_score(lm)).max() <= 1e-12 * np.abs(st[:, 0]).max()
    assert np.all(st[:, 4] < 0.5) and np.all(st[:, 1] < 0.5)
    lm[3, 7] = np.nan
    st2 = ic_ref.model(lm)
    assert np.isnan(st2[7]).all() and np.array_equal(np.delete(st2, 7, 0), np.delete(st, 7, 0))
    from mcmc_clv_model_amd import analysis as A
    out = A.marginal_frames(st, 32)
    assert out["kind"] == "marginal" and set(out) == {"pointwise", "waic", "loo", "kind"}
    assert math.isclose(out["loo"]["elpd"].iloc[0], st[:, 3].sum(), rel_tol=1e-12)
