"""Test helpers: golden-fixture loading and CBS DataFrames (test infrastructure)."""
from __future__ import annotations

import os

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name: str):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def cdnow(name: str = "abe", n: int | None = None) -> pd.DataFrame:
    """CDNOW CBS (data/processed/cdnow_{abe,full}CBS.csv columns) + driver-side log_s / gender_F
    (trivariate/run_mcmc_full.py:60-67, trivariate/run_mcmc_abe.py:100-105)."""
    d = golden(f"cdnow_{name}_cbs.npz")
    df = pd.DataFrame({k: d[k] for k in d.files})
    if n is not None:
        df = df.iloc[:n].copy().reset_index(drop=True)
    with np.errstate(divide="ignore"):
        df["log_s"] = np.log(df["sales"] / (df["x"] + 1)).replace(-np.inf, 0.0).fillna(0.0)
    df["gender_F"] = 1 - df["gender_binary"]
    return df


def cdnow_tiled(n: int) -> pd.DataFrame:
    """cdnow("full") rows taken cyclically up to n, index reset: a deterministic CBS of any size that
    keeps the real x = 0 / t_x = 0 / t_x near T rows."""
    df = cdnow("full")
    return df.iloc[np.arange(n) % len(df)].copy().reset_index(drop=True)


EDGE_T = (0.01, 1.0, 39.0, 520.0, 3650.0)
EDGE_X = (50, 400, 2000, 20000)
EDGE_LOG_S = (-12.0, 0.0, 14.0)


def edge_archetypes():
    """(x, t_x, T_cal) of the edge frame: for every span T no purchase at all, one purchase at T (alive for
    certain), at T (1 - 2^-40), at 1e-9 T, three by T / 2; then heavy buyers on a weekly and a daily
    clock.  41 rows, no random numbers."""
    rows = []
    for T in EDGE_T:
        rows += [(0, 0.0, T), (1, T, T), (1, T * (1.0 - 2.0 ** -40), T), (1, 1e-9 * T, T), (3, T / 2, T)]
    for x in EDGE_X:
        rows += [(x, 38.9, 39.0), (x, 20.0, 39.0), (x, 3649.0, 3650.0), (x, 0.5, 39.0)]
    return rows


def edge_cbs(n: int) -> pd.DataFrame:
    """The edge archetypes taken cyclically up to n (as cdnow_tiled): customers far from CDNOW — daily
    units, long histories, heavy buyers, spans of 0 and of 2^-40 T.  ``sales`` is set so that log_s, derived
    as cdnow() derives it, cycles through -12, 0 and +14 along the frame and is 0 where x = 0 (no sales)."""
    rows = edge_archetypes()
    a = [rows[i % len(rows)] for i in range(n)]
    x = np.array([r[0] for r in a], dtype=np.int64)
    target = np.array([EDGE_LOG_S[i % len(EDGE_LOG_S)] for i in range(n)])
    df = pd.DataFrame(dict(x=x, t_x=np.array([r[1] for r in a], dtype=np.float64),
                           T_cal=np.array([r[2] for r in a], dtype=np.float64),
                           sales=np.where(x == 0, 0.0, (x + 1) * np.exp(target))))
    with np.errstate(divide="ignore"):
        df["log_s"] = np.log(df["sales"] / (df["x"] + 1)).replace(-np.inf, 0.0).fillna(0.0)
    return df


def with_covariates(df: pd.DataFrame, n_cov: int, seed: int = 4242) -> pd.DataFrame:
    """c1..c{n_cov}: U(-1,1) covariate columns (the c4/c5 covariate model) added to a CBS."""
    df = df.copy()
    cov = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(len(df), n_cov))
    for k in range(n_cov):
        df[f"c{k + 1}"] = cov[:, k]
    return df


def replay_case(name: str):
    """(DataFrame, covariates, fixture) of a G2 replay fixture."""
    f = golden(f"replay_{name}.npz")
    cols = dict(x=f["x"], t_x=f["t_x"], T_cal=f["T_cal"], log_s=f["log_s"])
    covs = [str(c) for c in f["covariates"]]
    for c in covs:
        cols[c] = f["cov_" + c]
    return pd.DataFrame(cols), covs, f


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
