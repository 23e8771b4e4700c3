#!/usr/bin/env python3
"""Writes mcmc_clv_model_amd/csrc/gauss_hermite.h: the Gauss-Hermite rules (weight exp(-t^2)) of the
orders csrc/marginal.hip supports, from 40-digit mpmath.

Per order Q, nodes ascending: t_j, w_j and c_j = log(w_j) + t_j^2 (what the adaptive rule adds to the
integrand's logarithm), each rounded once from 40 digits to the nearest double and written as a
hexadecimal literal.  The nodes are the roots of the orthonormal Hermite polynomial h_Q (recurrence
h_{k+1} = t sqrt(2 / (k + 1)) h_k - sqrt(k / (k + 1)) h_{k-1}, h_0 = pi^(-1/4)), polished by Newton
from numpy's double nodes; w_j = 1 / (Q h_{Q-1}(t_j)^2).

    python tools/make_gauss_hermite.py            # rewrites the header
    python tools/make_gauss_hermite.py --check    # exits 1 if the header differs
"""
from __future__ import annotations

import os
import sys

import mpmath as mp
import numpy as np

ORDERS = (8, 16, 24, 32)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmc_clv_model_amd", "csrc",
                      "gauss_hermite.h")


def orthonormal(Q: int, t):
    """(h_Q(t), h_{Q-1}(t)) of the orthonormal Hermite polynomials."""
    h0, h1 = mp.mpf(0), mp.pi ** mp.mpf(-0.25)
    for k in range(Q):
        h0, h1 = h1, t * mp.sqrt(mp.mpf(2) / (k + 1)) * h1 - mp.sqrt(mp.mpf(k) / (k + 1)) * h0
    return h1, h0


def rule(Q: int):
    """The order-Q rule at 40 digits: lists t, w, c."""
    mp.mp.dps = 40
    ts, ws, cs = [], [], []
    for t0 in np.polynomial.hermite.hermgauss(Q)[0]:
        t = mp.mpf(float(t0))
        for _ in range(8):  # h_Q' = sqrt(2 Q) h_{Q-1}
            hq, hq1 = orthonormal(Q, t)
            t = t - hq / (mp.sqrt(2 * Q) * hq1)
        _, hq1 = orthonormal(Q, t)
        w = 1 / (Q * hq1 * hq1)
        ts.append(t)
        ws.append(w)
        cs.append(mp.log(w) + t * t)
    if Q % 2:
        ts[Q // 2] = mp.mpf(0)
    return ts, ws, cs


def render() -> str:
    out = ["// Gauss-Hermite rules (weight exp(-t^2)) of the orders csrc/marginal.hip supports: per order Q the",
           "// nodes t_j ascending, the weights w_j and c_j = log(w_j) + t_j^2, rounded once from 40 digits.",
           "// Written by tools/make_gauss_hermite.py; do not edit.  tests/test_marginal_cpu.py checks it against",
           "// numpy's hermgauss and the monomials up to degree 2 Q - 1.",
           "#pragma once",
           "",
           "#define CLV_GH_ORDERS {" + ", ".join(str(q) for q in ORDERS) + "}",
           f"#define CLV_GH_N_ORDERS {len(ORDERS)}",
           f"#define CLV_GH_TOTAL {sum(ORDERS)}  // entries of each table: the orders' rules one after another",
           ""]
    cols = {"T": [], "W": [], "C": []}
    for Q in ORDERS:
        t, w, c = rule(Q)
        cols["T"] += [(Q, v) for v in t]
        cols["W"] += [(Q, v) for v in w]
        cols["C"] += [(Q, v) for v in c]
    names = {"T": "nodes", "W": "weights", "C": "log(w) + t^2"}
    for key in ("T", "W", "C"):
        out.append(f"// {names[key]}")
        out.append(f"#define CLV_GH_{key}_INIT {{ \\")
        last = None
        for Q, v in cols[key]:
            if Q != last:
                out.append(f"  /* Q = {Q} */ \\")
                last = Q
            out.append(f"  {float(v).hex()}, \\")
        out.append("}")
        out.append("")
    return "\n".join(out)


def main() -> int:
    text = render()
    if "--check" in sys.argv[1:]:
        with open(HEADER) as f:
            same = f.read() == text
        print("gauss_hermite.h is up to date" if same else "gauss_hermite.h differs from the 40-digit rules")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
