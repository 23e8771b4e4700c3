// What csrc/marginal.hip and csrc/mml.hip (section 4n) share: a level-2 record's
// constants, the two log-concave components of a customer's Pareto/NBD likelihood, their Newton
// centring and the Gauss-Hermite rule through a running maximum.  marginal.hip's header comment has
// the formulas.  One body serves both files, so the log of a component's integral is the same bits
// in both: with MOM > 0 the loop carries, next to the sum s, the sums of the standardised coordinates
// (mml.hip), which take no part in s or the maximum.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "gauss_hermite.h"
#include "internal.h"

namespace {

constexpr int MARG_NEWTON = CLV_MARGINAL_NEWTON;         // Newton steps per component
constexpr double MARG_STEP_CAP = 2.0;    // the most a step moves either coordinate
constexpr double MARG_STEP_DONE = 1e-9;  // "steps used": the first step below this (reported only)
constexpr int MARG_NC = 11;              // P00 P01 P11 H00 H01 H11 c0 sc1 sc2 v cs
constexpr double LOG_2PI = 0x1.d67f1c864beb5p+0;
constexpr double SQRT2 = 0x1.6a09e667f3bcdp+0;
constexpr int GH_ORDERS[CLV_GH_N_ORDERS] = CLV_GH_ORDERS;
constexpr int MARG_MOM = 6;              // E[da], E[db], E[da da], E[da db], E[db db], E[g] of a component

__constant__ double GH_T[CLV_GH_TOTAL] = CLV_GH_T_INIT;
__constant__ double GH_C[CLV_GH_TOTAL] = CLV_GH_C_INIT;

struct MargArgs {
  const double* level2;  // [n_rec][l2w]
  const double* consts;  // [n_rec][MARG_NC]
  const double* cov;     // [K - 1][n] or null
  const int32_t* x;
  const double *tx, *T, *logs;  // logs null: no spend term
  int64_t n_rec, n;
  int D, K, Q, q_at;  // q_at: where the order-Q rule starts in the tables
  double omega2;
};

struct Rc {  // a record's constants
  double P00, P01, P11, H00, H01, H11, c0, sc1, sc2, v, cs;
};

struct Cp {  // a component of one customer
  double xa, xb, t, m0, m1, r0;
};

__global__ void marg_prepare_kernel(MargArgs A, double* consts) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n_rec) return;
  const int l2w = A.D * A.K + A.D * (A.D + 1) / 2;
  const double* sg = A.level2 + r * l2w + A.D * A.K;  // Sigma's upper triangle, row by row
  const double s00 = sg[0], s01 = sg[1], s11 = A.D == 2 ? sg[2] : sg[3];
  const double det = s00 * s11 - s01 * s01;
  bool ok = (s00 > 0.0) && (det > 0.0);
  Rc c;
  c.P00 = s11 / det;
  c.P01 = -(s01 / det);
  c.P11 = s00 / det;
  c.c0 = -LOG_2PI - 0.5 * log(det);
  c.H00 = c.P00, c.H01 = c.P01, c.H11 = c.P11;
  c.sc1 = c.sc2 = c.cs = 0.0;
  c.v = 1.0;
  if (A.logs) {
    const double s02 = sg[2], s12 = sg[4], s22 = sg[5];
    c.sc1 = (s02 * s11 - s12 * s01) / det;
    c.sc2 = (s12 * s00 - s02 * s01) / det;
    c.v = (s22 - (c.sc1 * s02 + c.sc2 * s12)) + A.omega2;
    ok = ok && (c.v > 0.0);
    c.cs = -0.5 * (LOG_2PI + log(c.v));
    c.H00 = c.P00 + (c.sc1 * c.sc1) / c.v;
    c.H01 = c.P01 + (c.sc1 * c.sc2) / c.v;
    c.H11 = c.P11 + (c.sc2 * c.sc2) / c.v;
  }
  double* o = consts + r * MARG_NC;
  const double v[MARG_NC] = {c.P00, c.P01, c.P11, c.H00, c.H01, c.H11, c.c0, c.sc1, c.sc2, c.v, c.cs};
#pragma unroll
  for (int k = 0; k < MARG_NC; ++k) o[k] = ok ? v[k] : std::numeric_limits<double>::quiet_NaN();
}

// h(a, b) with lam = exp(a) given; mu takes exp(b).
template <bool SPEND>
__device__ __forceinline__ double marg_h(const Rc& c, const Cp& p, double a, double b, double lam, double& mu) {
  const double da = a - p.m0, db = b - p.m1;
  const double quad = (c.P00 * da * da + 2.0 * c.P01 * da * db) + c.P11 * db * db;
  mu = exp(b);
  const double ml = lam + mu;
  const double lik = ((p.xa * a + p.xb * b) - log(ml)) - ml * p.t;
  double h = lik + (c.c0 - 0.5 * quad);
  if (SPEND) {
    const double r = (p.r0 - c.sc1 * da) - c.sc2 * db;
    h = h + (c.cs - (r * r) / (2.0 * c.v));
  }
  return h;
}

// The gradient (ga, gb) and the negative Hessian (n00, n01, n11; det its determinant) of h at (a, b);
// where det is not positive, the gaussian part's H alone.
template <bool SPEND>
__device__ __forceinline__ void marg_derivs(const Rc& c, const Cp& p, double a, double b, double& ga, double& gb,
                                            double& n00, double& n01, double& n11, double& det) {
  const double da = a - p.m0, db = b - p.m1;
  const double lam = exp(a), mu = exp(b);
  const double ml = lam + mu;
  const double q = lam / ml, qm = mu / ml;
  ga = ((p.xa - q) - lam * p.t) - (c.P00 * da + c.P01 * db);
  gb = ((p.xb - qm) - mu * p.t) - (c.P01 * da + c.P11 * db);
  if (SPEND) {
    const double rv = ((p.r0 - c.sc1 * da) - c.sc2 * db) / c.v;
    ga = ga + c.sc1 * rv;
    gb = gb + c.sc2 * rv;
  }
  const double qq = q * qm;
  n00 = (qq + lam * p.t) + c.H00;
  n01 = c.H01 - qq;
  n11 = (qq + mu * p.t) + c.H11;
  det = n00 * n11 - n01 * n01;
  if (!(det > 0.0) && det == det) {
    n00 = c.H00, n01 = c.H01, n11 = c.H11;
    det = c.H00 * c.H11 - c.H01 * c.H01;
  }
}

// log of the component's integral by the order-Q rule that starts at q_at in the tables; cen (or
// null) takes a, b, L00, L10, L11, steps used.  MOM = 0: nothing else.  MOM >= 1: mo[0..5) = the
// component's own E[da], E[db], E[da da], E[da db], E[db db], (da, db) = theta - (m0, m1): the sums of
// u = t_j, w = L10 t_j + L11 t_k, u u, u w, w w weighted as s is and rescaled with it when the maximum
// moves, mapped through theta - m = (centre - m) + sqrt2 (L00 u, w) at the end.  MOM = 2: mo[5] = the
// mean of g = e^(a - b) (1 - exp(-e^b t_star)) as well (lambda / mu times the chance of dropping out
// within t_star: the expected purchases in (T, T + t_star] of a customer alive at T).
template <bool SPEND, int MOM>
__device__ __forceinline__ double marg_component(int Q, int q_at, const Rc& c, const Cp& p, double* cen, double t_star,
                                                 double* mo) {
  double a = p.m0, b = p.m1;
  double ga, gb, n00, n01, n11, det;
  int used = MARG_NEWTON;
  for (int it = 0; it < MARG_NEWTON; ++it) {
    marg_derivs<SPEND>(c, p, a, b, ga, gb, n00, n01, n11, det);
    double sa = (n11 * ga - n01 * gb) / det;
    double sb = (n00 * gb - n01 * ga) / det;
    const double mx = fmax(fabs(sa), fabs(sb));
    if (mx > MARG_STEP_CAP) {
      const double scale = MARG_STEP_CAP / mx;
      sa = sa * scale;
      sb = sb * scale;
    }
    a = a + sa;
    b = b + sb;
    if (mx < MARG_STEP_DONE && used == MARG_NEWTON) used = it + 1;
  }
  marg_derivs<SPEND>(c, p, a, b, ga, gb, n00, n01, n11, det);
  const double L00 = sqrt(n11 / det);
  const double L10 = -(n01 / det) / L00;
  const double L11 = 1.0 / sqrt(n11);
  if (cen) {
    cen[0] = a, cen[1] = b, cen[2] = L00, cen[3] = L10, cen[4] = L11, cen[5] = (double)used;
  }
  double m = -std::numeric_limits<double>::infinity(), s = 0.0;
  double su = 0.0, sw = 0.0, suu = 0.0, suw = 0.0, sww = 0.0, sg = 0.0;
  const double* gt = GH_T + q_at;
  const double* gc = GH_C + q_at;
  for (int j = 0; j < Q; ++j) {
    const double tj = gt[j], cj = gc[j];
    const double aj = a + SQRT2 * (L00 * tj);
    const double lam = exp(aj);
#pragma unroll 2
    for (int k = 0; k < Q; ++k) {
      const double wk = L10 * tj + L11 * gt[k];
      const double bk = b + SQRT2 * wk;
      double mu;
      const double v = (cj + gc[k]) + marg_h<SPEND>(c, p, aj, bk, lam, mu);
      const bool up = v > m;
      const double e = exp(up ? m - v : v - m);
      s = up ? s * e + 1.0 : s + e;
      if (MOM >= 1) {
        su = up ? su * e + tj : su + e * tj;
        sw = up ? sw * e + wk : sw + e * wk;
        suu = up ? suu * e + tj * tj : suu + e * (tj * tj);
        suw = up ? suw * e + tj * wk : suw + e * (tj * wk);
        sww = up ? sww * e + wk * wk : sww + e * (wk * wk);
      }
      if (MOM >= 2) {
        const double y = mu * t_star;
        const double g = y > 0.0 ? (lam / mu) * -expm1(-y) : lam * t_star;
        sg = up ? sg * e + g : sg + e * g;
      }
      m = up ? v : m;
    }
  }
  if (MOM >= 1) {
    const double U = su / s, W = sw / s, UU = suu / s, UW = suw / s, WW = sww / s;
    const double ca = a - p.m0, cb = b - p.m1, k0 = SQRT2 * L00;
    mo[0] = ca + k0 * U;
    mo[1] = cb + SQRT2 * W;
    mo[2] = (ca * ca + 2.0 * (ca * k0) * U) + (k0 * k0) * UU;
    mo[3] = ((ca * cb + (ca * SQRT2) * W) + (cb * k0) * U) + (k0 * SQRT2) * UW;
    mo[4] = (cb * cb + 2.0 * (cb * SQRT2) * W) + 2.0 * WW;
    mo[5] = MOM >= 2 ? sg / s : 0.0;
  }
  return log(2.0 * (L00 * L11)) + (m + log(s));
}

// The order `nodes` (0: the default) and where its rule starts in the tables.
inline int order_at(int32_t nodes, int* Q, int* at) {
  const int want = nodes == 0 ? CLV_MARGINAL_DEFAULT_NODES : nodes;
  int off = 0;
  for (int k = 0; k < CLV_GH_N_ORDERS; ++k) {
    if (GH_ORDERS[k] == want) {
      *Q = want;
      *at = off;
      return CLV_OK;
    }
    off += GH_ORDERS[k];
  }
  return clv::fail(CLV_EINVAL, "nodes must be 0 (the default), 8, 16, 24 or 32");
}

}  // namespace
