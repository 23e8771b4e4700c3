"""Float64 model of the posterior predictive replicate of csrc/ppc.hip — TEST
INFRASTRUCTURE ONLY, plain numpy, vectorised — built on tests/analysis_stream_ref.py (``block``,
``poisson``) and oracle/philox.py.

The replicate of customer i under flat draw d: Philox4x32-10 keyed by the seed, counter
(customer_offset + i, d, slot, 5).

    level 0   lambda = level1[d, i, 0], mu = level1[d, i, 1]
    level 1   (beta, Sigma) = l2_unpack(level2[d]); m_j = sum_k X_ik beta_kj (k ascending, X_i0 = 1);
              l00 = sqrt(S00), l10 = S01 / l00, l11 = sqrt(S11 - l10^2); (n0, n1) the Box-Muller pair
              (cos, sin) of slot 1 as analysis_stream_ref.gen_mvn builds it;
              lambda = exp(m0 + l00 n0), mu = exp(m1 + l10 n0 + l11 n1)
    slot 0    E = -log(u53_open0(x, y)), U = u53_open0(z, w); tau = E / mu; alive = tau > T;
              L = alive ? T : tau
    x_rep     = Poisson(lambda L) from slots 16 + attempt (analysis_stream_ref.poisson)
    t_x_rep   = x_rep > 0 ? L exp(log(U) / x_rep) : 0

Every decision compares two computed numbers; ``margin`` is the smallest relative distance by which a
decision on the replicate's path was taken: tau from T, the Poisson branch (the mean from 10, unless
the mean is the exact product of a level-1 lambda and T) and every Poisson decision, and t_x_rep from
the observed t_x (0 <= 0 of two exact zeros carries none).  A lane is *clear* when margin > RTOL.
"""
from __future__ import annotations

import numpy as np

from oracle import philox as oph
from tests import analysis_stream_ref as AR
from tests.philox_sweep_ref import BORDERLINE_CAP, RTOL, l2_record, l2_unpack  # noqa: F401

SEEDS = AR.SEEDS
STREAM_PPC = 5
SLOT_LIFE, SLOT_NORMAL, SLOT_POISSON0 = 0, 1, 16
BLOCK = 256
STATS = ("x_rep_mean", "p_x_lt", "p_x_eq", "p_zero", "tx_rep_mean", "p_tx_le", "p_alive_rep")
DRAW_INTS = ("sum_x", "sum_x2", "max_x", "n_alive")
MAX_K = 4096


def _rel(a, b):
    """|a - b| / (|a| + |b|); inf where either is infinite, 0 where NaN."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - b) / (np.abs(a) + np.abs(b))
    r = np.where(np.isinf(a) | np.isinf(b), np.inf, r)
    return np.where(np.isnan(r), 0.0, r)


def population_params(level2, D, K, cov, seed, a, d, stream=STREAM_PPC):
    """(lambda, mu, m (.., 2), chol (l00, l10, l11)) of the mixed replicate: level2 (n_draws, width),
    cov (K - 1, n) or None, a / d the (n_draws, n) counter words."""
    nd, n = a.shape
    lam, mu = np.empty((nd, n)), np.empty((nd, n))
    r = AR.block(seed, a, d, SLOT_NORMAL, stream)
    rad = np.sqrt(-2.0 * np.log(oph.u53_open0(r[..., 0], r[..., 1])))
    ang = 2.0 * np.pi * oph.u53(r[..., 2], r[..., 3])
    n0, n1 = rad * np.cos(ang), rad * np.sin(ang)
    ms = np.empty((nd, n, 2))
    ch = np.empty((nd, 3))
    for q in range(nd):
        beta, Sigma = l2_unpack(np.asarray(level2[q], dtype=np.float64), D, K)
        m0, m1 = np.full(n, beta[0, 0]), np.full(n, beta[0, 1])
        for k in range(1, K):
            m0 = m0 + cov[k - 1] * beta[k, 0]
            m1 = m1 + cov[k - 1] * beta[k, 1]
        l00 = np.sqrt(Sigma[0, 0])
        l10 = Sigma[0, 1] / l00
        l11 = np.sqrt(Sigma[1, 1] - l10 * l10)
        lam[q] = np.exp(m0 + l00 * n0[q])
        mu[q] = np.exp(m1 + l10 * n0[q] + l11 * n1[q])
        ms[q, :, 0], ms[q, :, 1] = m0, m1
        ch[q] = l00, l10, l11
    return lam, mu, ms, ch


def replicate(level, seed, t_x, T, *, level1=None, level2=None, D=2, K=1, cov=None, offset=0, swap_counter=False,
              stream=STREAM_PPC, recency_half=1):
    """The replicates of every (flat draw, customer): dict(x_rep int64, t_x_rep, alive, margin, lam,
    mu, tau, L), each (n_draws, n).  ``swap_counter`` / ``stream`` / ``recency_half`` are the power
    checks' wrong layouts."""
    t_x, T = np.asarray(t_x, dtype=np.float64), np.asarray(T, dtype=np.float64)
    n = T.shape[0]
    nd = np.asarray(level1).shape[0] if level == 0 else np.asarray(level2).shape[0]
    cust, draw = np.broadcast_arrays(np.arange(n)[None, :] + int(offset), np.arange(nd)[:, None])
    a, d = (draw, cust) if swap_counter else (cust, draw)
    if level == 0:
        l1 = np.asarray(level1, dtype=np.float64)
        lam, mu = l1[..., 0], l1[..., 1]
    else:
        lam, mu, _, _ = population_params(level2, D, K, cov, seed, a, d, stream)
    r = AR.block(seed, a, d, SLOT_LIFE, stream)
    E = -np.log(oph.u53_open0(r[..., 0], r[..., 1]))
    h = 2 * recency_half
    U = oph.u53_open0(r[..., h], r[..., h + 1])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tau = E / mu
        alive = tau > T[None, :]
        L = np.where(alive, T[None, :], tau)
        m = lam * L
    x_rep, pm = AR.poisson(m, seed, a, d, SLOT_POISSON0, stream)
    with np.errstate(divide="ignore", invalid="ignore"):
        tq = np.where(x_rep > 0, L * np.exp(np.log(U) / np.where(x_rep > 0, x_rep, 1)), 0.0)
    margin = np.minimum(_rel(tau, T[None, :]), pm)
    exact_mean = alive if level == 0 else np.zeros_like(alive)
    with np.errstate(invalid="ignore"):
        branch = np.where(exact_mean | ~(m > 0.0), np.inf, _rel(m, 10.0))
    margin = np.minimum(margin, branch)
    both_zero = (tq == 0.0) & (t_x[None, :] == 0.0)
    margin = np.minimum(margin, np.where(both_zero, np.inf, _rel(tq, t_x[None, :])))
    return dict(x_rep=x_rep, t_x_rep=tq, alive=alive, margin=margin, lam=lam, mu=mu, tau=tau, L=L)


# ---------------------------------------------------------------------------------------------
# the aggregates of clv_ppc
# ---------------------------------------------------------------------------------------------
def _tree(a):
    off = BLOCK // 2
    while off:
        a = a[..., :off] + a[..., off:2 * off]
        off >>= 1
    return a[..., 0]


def fixed_order_rows(v):
    """Per row of v (n_draws, n): zero-padded 256-customer blocks by the 256-tree (s[e] += s[e + off],
    off = 128 ... 1), then lane t adds the block partials t, t + 256, ... in turn from zero and the
    lanes go through the same tree (csrc/ltv.hip ltv_final_kernel)."""
    v = np.asarray(v, dtype=np.float64)
    nd, n = v.shape
    nb = -(-n // BLOCK)
    part = _tree(np.pad(v, ((0, 0), (0, nb * BLOCK - n))).reshape(nd, nb, BLOCK))
    rows = np.pad(part, ((0, 0), (0, -(-nb // BLOCK) * BLOCK - nb))).reshape(nd, -1, BLOCK)
    acc = np.zeros((nd, BLOCK))
    for q in range(rows.shape[1]):
        acc = acc + rows[:, q]
    return _tree(acc)


def aggregates(x_rep, t_x_rep, alive, x, t_x, k_hist):
    """dict(customers (n, 7), draws_int (n_draws, k_hist + 5), sum_tx (n_draws,)) from replicates."""
    x_rep = np.asarray(x_rep, dtype=np.int64)
    nd, n = x_rep.shape
    x, t_x = np.asarray(x, dtype=np.int64), np.asarray(t_x, dtype=np.float64)
    S = float(nd)
    cust = np.empty((n, len(STATS)))
    cust[:, 0] = x_rep.sum(axis=0).astype(np.float64) / S
    cust[:, 1] = (x_rep < x[None, :]).sum(axis=0) / S
    cust[:, 2] = (x_rep == x[None, :]).sum(axis=0) / S
    cust[:, 3] = (x_rep == 0).sum(axis=0) / S
    cust[:, 4] = np.add.accumulate(np.asarray(t_x_rep, dtype=np.float64), axis=0)[-1] / S   # in draw order
    cust[:, 5] = (t_x_rep <= t_x[None, :]).sum(axis=0) / S
    cust[:, 6] = np.asarray(alive).sum(axis=0) / S
    di = np.zeros((nd, k_hist + 1 + len(DRAW_INTS)), np.int64)
    b = np.minimum(x_rep, k_hist)
    for q in range(nd):
        di[q, :k_hist + 1] = np.bincount(b[q], minlength=k_hist + 1)
    di[:, k_hist + 1] = x_rep.sum(axis=1)
    di[:, k_hist + 2] = (x_rep * x_rep).sum(axis=1)
    di[:, k_hist + 3] = x_rep.max(axis=1)
    di[:, k_hist + 4] = np.asarray(alive).sum(axis=1)
    return dict(customers=cust, draws_int=di, sum_tx=fixed_order_rows(t_x_rep))


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_ppc.py (tests/test_ppc_cpu.py asserts the borderline cap of the model
# alone on exactly these inputs)
# ---------------------------------------------------------------------------------------------
C1_MEANS = (0.0, 0.3, 9.99, float(np.nextafter(10.0, 0.0)), 10.0, 37.5, 600.0, 1e5)
C1_MU_T = (1e-3, 0.5, 3.0, 50.0)
C1_T = (32.0, 16.0, 64.0)     # powers of two: lambda = mean / T gives lambda T = the mean exactly


def observed(n, T):
    """x, t_x of n customers: a third have x = 0, t_x = 0; the rest 1 .. 13 purchases, the last inside
    (0, T)."""
    i = np.arange(n)
    x = np.where(i % 3 == 0, 0, 1 + (i * 7) % 13).astype(np.int32)
    t_x = np.where(x == 0, 0.0, T * (((i * 37) % 100 + 1) / 101.0))
    return x, t_x


def customer_case(width=4, n=513, chains=2, per_chain=3):
    """n = 513 (two full blocks and one lane), 2 chains x 3 draws.  Target means lambda T cycle through
    C1_MEANS, mu T through C1_MU_T: both Poisson branches and both sides of tau vs T occur."""
    nd = chains * per_chain
    i, d = np.meshgrid(np.arange(n), np.arange(nd))
    T = np.array(C1_T)[np.arange(n) % 3]
    l1 = np.zeros((nd, n, width))
    l1[..., 0] = np.array(C1_MEANS)[(i + d) % 8] / T[None, :]
    l1[..., 1] = np.array(C1_MU_T)[(i // 8 + d) % 4] / T[None, :]
    l1[..., 2] = 50.0
    l1[..., 3] = 1.0
    if width > 4:
        l1[..., 4] = 0.5
    x, t_x = observed(n, T)
    return dict(level=0, level1=l1, width=width, x=x, t_x=t_x, T_cal=T, chains=chains)


def population_case(D, K, n=300, chains=2, per_chain=3):
    """2 x 3 level-2 records of a (D, K) fit; record 1 has correlation 0.999, record 2 variances 1e-8."""
    rng = np.random.default_rng(1000 + 10 * D + K)
    nd = chains * per_chain
    cov = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (K - 1, n))) if K > 1 else None
    recs = []
    for q in range(nd):
        beta = np.zeros((K, D))
        beta[0, :2] = (-2.4 + 0.1 * q, -3.6 + 0.15 * q)
        if K > 1:
            beta[1:, :2] = rng.normal(0.0, 0.3, (K - 1, 2))
        s0, s1, rho = 0.8 + 0.1 * q, 1.2 - 0.1 * q, 0.2 * (q - 2)
        if q == 1:
            rho = 0.999
        if q == 2:
            s0 = s1 = 1e-8
        Sigma = np.eye(D)
        Sigma[0, 0], Sigma[1, 1] = s0, s1
        Sigma[0, 1] = Sigma[1, 0] = rho * np.sqrt(s0 * s1)
        if D == 3:
            beta[:, 2] = rng.normal(3.0, 0.2, K)
            Sigma[2, 2] = 0.5
            Sigma[0, 2] = Sigma[2, 0] = 0.1 * np.sqrt(s0 * 0.5)
            Sigma[1, 2] = Sigma[2, 1] = -0.1 * np.sqrt(s1 * 0.5)
        recs.append(l2_record(beta, Sigma))
    T = np.array(C1_T)[np.arange(n) % 3] + 7.0 * (np.arange(n) % 2)
    x, t_x = observed(n, T)
    return dict(level=1, level2=np.ascontiguousarray(np.array(recs)), D=D, K=K, cov=cov, x=x, t_x=t_x, T_cal=T,
                chains=chains)


POPULATION_DK = ((2, 1), (2, 3), (3, 2))
S5_MEANS = (0.3, 4.0, 9.99, 12.0, 37.5, 600.0)


def long_case(nd=65537):
    """n = 1 with 65,537 draws (more than a grid's extent of draw chunks)."""
    l1 = np.zeros((nd, 1, 4))
    l1[:, 0, 0] = np.array(S5_MEANS)[np.arange(nd) % 6] / 32.0
    l1[:, 0, 1] = np.array(C1_MU_T)[(np.arange(nd) // 6) % 4] / 32.0
    l1[:, 0, 2], l1[:, 0, 3] = 50.0, 1.0
    return dict(level=0, level1=l1, width=4, x=np.array([3], np.int32), t_x=np.array([20.0]), T_cal=np.array([32.0]),
                chains=1)


def edge_case(n=64, nd=4):
    """Edge draws: mu = 1e-300 (tau = E / mu beyond any T: alive), mu = 1e300 (L about 0, x_rep = 0),
    NaN lambda (x_rep = 0), by customer i % 3."""
    i = np.arange(n)
    l1 = np.zeros((nd, n, 4))
    l1[..., 0] = np.where(i % 3 == 2, np.nan, 0.4)[None, :]
    l1[..., 1] = np.select([i % 3 == 0, i % 3 == 1], [1e-300, 1e300], 0.05)[None, :]
    l1[..., 2], l1[..., 3] = 50.0, 1.0
    T = np.full(n, 32.0)
    x, t_x = observed(n, T)
    return dict(level=0, level1=l1, width=4, x=x, t_x=t_x, T_cal=T, chains=1)


def model(case, seed, **kw):
    """replicate() of a case."""
    if case["level"] == 0:
        return replicate(0, seed, case["t_x"], case["T_cal"], level1=case["level1"], **kw)
    return replicate(1, seed, case["t_x"], case["T_cal"], level2=case["level2"], D=case["D"], K=case["K"],
                     cov=case["cov"], **kw)


def gpu_cases():
    """name -> case: every input the GPU tests compare value by value."""
    out = {"customer_w4": customer_case(4), "customer_w5": customer_case(5), "long": long_case(), "edge": edge_case()}
    for D, K in POPULATION_DK:
        out[f"population_{D}{K}"] = population_case(D, K)
    return out
