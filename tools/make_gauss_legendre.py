#!/usr/bin/env python3
"""Writes mcmc_clv_model_amd/csrc/gauss_legendre.h: the 16-point Gauss-Legendre rule on [-1, 1] that
csrc/pnbd.hip integrates the DERT integrand with, from 40-digit mpmath.

Nodes ascending, x_j and w_j rounded once from 40 digits to the nearest double and written as
hexadecimal literals.  The nodes are the roots of P_16 (recurrence (k + 1) P_{k+1} = (2k + 1) x P_k -
k P_{k-1}), polished by Newton from numpy's double nodes; w_j = 2 / ((1 - x_j^2) P_16'(x_j)^2).

    python tools/make_gauss_legendre.py            # rewrites the header
    python tools/make_gauss_legendre.py --check    # exits 1 if the header differs
"""
from __future__ import annotations

import os
import sys

import mpmath as mp
import numpy as np

Q = 16
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmc_clv_model_amd", "csrc",
                      "gauss_legendre.h")


def legendre(x):
    """(P_Q(x), P_Q'(x))."""
    p0, p1 = mp.mpf(1), x
    for k in range(1, Q):
        p0, p1 = p1, ((2 * k + 1) * x * p1 - k * p0) / (k + 1)
    return p1, Q * (x * p1 - p0) / (x * x - 1)


def rule():
    mp.mp.dps = 40
    xs, ws = [], []
    for x0 in np.polynomial.legendre.leggauss(Q)[0]:
        x = mp.mpf(float(x0))
        for _ in range(8):
            p, dp = legendre(x)
            x = x - p / dp
        _, dp = legendre(x)
        xs.append(x)
        ws.append(2 / ((1 - x * x) * dp * dp))
    return xs, ws


def render() -> str:
    xs, ws = rule()
    out = ["// The 16-point Gauss-Legendre rule on [-1, 1]: nodes x_j ascending and weights w_j, rounded once from",
           "// 40 digits.  Written by tools/make_gauss_legendre.py; do not edit.  tests/test_mle_ext_cpu.py checks it",
           "// against numpy's leggauss and the monomials up to degree 31.",
           "#pragma once",
           "",
           f"#define CLV_GL_Q {Q}",
           "#define CLV_GL_X_INIT { \\"]
    out += [f"  {float(x).hex()}, \\" for x in xs]
    out += ["}", "#define CLV_GL_W_INIT { \\"]
    out += [f"  {float(w).hex()}, \\" for w in ws]
    out += ["}", ""]
    return "\n".join(out)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        with open(HEADER) as f:
            sys.exit(0 if f.read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
