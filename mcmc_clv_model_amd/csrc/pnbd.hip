// The classical Pareto/NBD likelihood on device: the maximum-likelihood baseline the reference takes
// from lifetimes.ParetoNBDFitter (bivariate/analysis_abe.py:205-217, :426-438; full_analysis.py:245,
// :437).  DESIGN.md section 4e; float64 model: tests/pnbd_ref.py.
//
//   clv_pnbd_create / _destroy   the CBS columns (x, t_x, T, weights) resident for a fit
//   clv_pnbd_eval                sum w log L and its gradient with respect to log(r, alpha, s, beta)
//   clv_pnbd_customers           per customer log L, P(alive), E[Y(t*) | x, t_x, T]
//   clv_pnbd_track               cum[j] = sum_i E[X(max(times[j] - birth_week[i], 0))]
//   clv_pnbd_set_covariates      time-invariant covariates (Fader & Hardie 2007) resident in the handle
//   clv_pnbd_eval_cov / _customers_cov / _track_cov   the same three with alpha_i = alpha0 exp(-gamma1' z_i),
//                                beta_i = beta0 exp(-gamma2' z_i): DESIGN.md section 4m
//   clv_pnbd_set_integral        how the handle's evaluations form I: the series below (the default), or a
//                                Gauss-Legendre quadrature of I itself for the customers the series cannot
//                                reach (z(t_x) above 0.9 in "auto", everyone in "quadrature"): DESIGN.md
//                                section 4o, pnbd_si_quadrature; float64 model: tests/pnbd_tail_ref.py
//
// Per customer, with theta = (r, alpha, s, beta), a = r + s + x, M = max(alpha, beta) and
// z(t) = |alpha - beta| / (M + t) in [0, 1):
//   L = Gamma(r+x) alpha^r beta^s / Gamma(r) { (alpha+T)^-(r+x) (beta+T)^-s + s I }
//   I = int_{t_x}^{T} (alpha+y)^-(r+x) (beta+y)^-(s+1) dy = [H(t_x) - H(T)] / a
//   H(t) = 2F1(a, b; a+1; z(t)) / (M+t)^a,  b = s+1 if alpha >= beta, r+x otherwise
// 2F1 is never summed directly (with b = r+x its terms grow before they decay and overflow for x
// in the hundreds): Euler's transformation gives 2F1(a, b; a+1; z) = (1-z)^(1-b) G(a+1-b, a+1; z),
// G(c1, c; z) = sum_n (c1)_n / (c)_n z^n, whose terms are positive with ratios < z, so the remainder
// after u_n is at most u_n z / (1 - z): an exact stopping rule.  Everything is carried in logs.
// The gradient comes from the same loop: du_n/dc1 = u_n sum_{k<n} 1/(c1+k), du_n/dc =
// -u_n sum_{k<n} 1/(c+k), du_n/dz = n u_n / z, and psi(r+x) - psi(r) = sum_{k<x} 1/(r+k).
//
// One lane per customer.  No float atomics: each 256-customer block reduces its lanes by an LDS
// tree, and a second kernel adds the block partials in a fixed order (lane t takes partials
// t, t + 256, ... in turn, then the same tree), so the sums do not depend on the grid size and are
// bitwise the same on every call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "gauss_legendre.h"
#include "internal.h"
#include "pnbd_sum.h"

using namespace clv;

struct clv_pnbd {
  int device = 0;
  int64_t n = 0, nb = 0;  // customers, 256-customer blocks
  DevBuf x;               // int32
  DevBuf tx, T, w;        // double; w null: every weight 1
  DevBuf part;            // [nb][PNBD_NS] block partials
  DevBuf out;             // [PNBD_NS]
  // covariates (clv_pnbd_set_covariates): [k][n] each, a wavefront reads a covariate row coalesced
  bool has_cov = false;
  int32_t k1 = 0, k2 = 0;
  DevBuf z1, z2;
  DevBuf partc;  // [nb][PNBD_NS + k1 + k2]
  DevBuf outc;   // [PNBD_NS + k1 + k2]
  int32_t integral = CLV_PNBD_INTEGRAL_SERIES;  // clv_pnbd_set_integral
};

namespace {

constexpr int PNBD_NS = 7;            // sum w log L, 4 gradient sums, sum w, unconverged customers
constexpr int PNBD_TERM_CAP = 2048;   // series terms after u_0 (reaches z of about 0.98)
constexpr double PNBD_EPS = 0x1p-53;  // relative remainder at which the series stops
constexpr int PNBD_MAX_COV = 8;      // covariate columns per process
constexpr int PNBD_COV_GROUP = 8;     // covariate sums reduced per pass over the LDS tile
// How I is evaluated (clv_pnbd_set_integral): a template parameter of the kernel family, as Src is, so the
// series instances are the code they were before the quadrature existed.
constexpr int PNBD_SERIES = CLV_PNBD_INTEGRAL_SERIES, PNBD_AUTO = CLV_PNBD_INTEGRAL_AUTO,
              PNBD_QUADRATURE = CLV_PNBD_INTEGRAL_QUADRATURE;
constexpr double PNBD_Z_SWITCH = 0.9;   // auto: the series up to this z(t_x) (at most about 370 terms), the quadrature past it
constexpr double PNBD_Q_SLOPE = 4.0;    // a panel is at most PNBD_Q_SLOPE / |d log integrand / dd| wide, and at most 1
constexpr double PNBD_Q_SPAN = 40.0;    // the panels may stop once the integrand is exp(-40) below its start
constexpr int PNBD_Q_PANEL_CAP = 4096;  // never reached by a finite width: the integrand falls at least as exp(-(r + s + x) d)

struct Params {
  double r, a, s, b;
};

// log G(c1, c; z) and d log G / d(c1, c, z); conv = the remainder rule was met within the cap.
struct Series {
  double lg, gc1, gc, gz;
  bool conv;
};

__host__ __device__ inline Series pnbd_series(double c1, double c, double z) {
  double u = 1.0, G = 1.0, s1 = 0.0, s2 = 0.0, d1 = 0.0, d2 = 0.0, dz = 0.0;
  const double q = z / (1.0 - z);
  bool conv = false;
  for (int n = 0;; ++n) {
    if (u * q <= PNBD_EPS * G) {
      conv = true;
      break;
    }
    if (n == PNBD_TERM_CAP) break;
    const double i1 = 1.0 / (c1 + n), i2 = 1.0 / (c + n);
    s1 += i1;
    s2 += i2;
    u = u * (((c1 + n) * i2) * z);
    G += u;
    d1 += u * s1;
    d2 += u * s2;
    dz += (n + 1.0) * u;
  }
  Series o;
  o.lg = log(G);
  o.gc1 = d1 / G;
  o.gc = -d2 / G;
  o.gz = (z > 0.0 ? dz / z : c1 / c) / G;
  o.conv = conv;
  return o;
}

// log H(t) and its derivatives with respect to (r, alpha, s, beta).
struct LogH {
  double lh, d[4];
  bool conv;
};

__host__ __device__ inline LogH pnbd_log_h(double t, double x, const Params& p) {
  const bool swap = p.a < p.b;
  const double M = (swap ? p.b : p.a) + t;
  const double z = fabs(p.a - p.b) / M;
  const double aa = p.r + p.s + x;
  const Series g = pnbd_series(swap ? p.s + 1.0 : p.r + x, aa + 1.0, z);
  const double bm1 = swap ? p.r + x - 1.0 : p.s;  // b - 1
  const double l1z = log1p(-z), lM = log(M);
  LogH o;
  o.conv = g.conv;
  o.lh = g.lg - bm1 * l1z - aa * lM;
  const double w = g.gz + bm1 / (1.0 - z);                // d log H / dz
  const double z_big = (1.0 - z) / M, z_small = -1.0 / M;  // dz / d(larger of alpha, beta), d(smaller)
  if (swap) {
    o.d[0] = g.gc - l1z - lM;
    o.d[2] = g.gc1 + g.gc - lM;
    o.d[1] = w * z_small;
    o.d[3] = w * z_big - aa / M;
  } else {
    o.d[0] = g.gc1 + g.gc - lM;
    o.d[2] = g.gc - l1z - lM;
    o.d[1] = w * z_big - aa / M;
    o.d[3] = w * z_small;
  }
  return o;
}

// log(s I) and d log(s I) / d(r, alpha, s, beta) by Gauss-Legendre quadrature of I itself, for t_x < T and any
// z.  With m = min(alpha, beta), Delta = |alpha - beta|, e0 = m + t_x and
// d = log((m + y) / e0) the integrand over its value at t_x is
//   g(d) = exp((1 - p_m) d - p_M log1p(q expm1(d))),  q = e0 / (e0 + Delta) = 1 - z(t_x),
// p_m the exponent of the factor with the smaller offset (r + x or s + 1), p_M the other one: positive,
// analytic in d (the nearest singularity is pi off the real axis) and free of both scales.  The panels walk d
// from 0 to log1p((T - t_x) / e0) -- the offset, never log(m + y) itself, so a width of 1e-12 keeps its
// digits -- each at most 1 wide and at most PNBD_Q_SLOPE / |g' / g| wide, and stop early where g has fallen
// by exp(-PNBD_Q_SPAN) and a panel no longer changes the sum.  The gradient is taken under the integral at
// the same nodes: the means under g of log(m + y) = log e0 + d, log(M + y) = log(e0 + Delta) + log1p(q expm1(d))
// and the two reciprocals.  No difference of two H values is formed.  ok = false: alpha_i or beta_i is not a
// positive finite number any more.
__host__ __device__ inline bool pnbd_si_quadrature(double x, double tx, double T, const Params& p, double* logsI,
                                                   double dI[4]) {
  constexpr double X[CLV_GL_Q] = CLV_GL_X_INIT, W[CLV_GL_Q] = CLV_GL_W_INIT;
  const bool swap = p.a < p.b;  // alpha is the smaller offset
  const double m = swap ? p.a : p.b;
  const double pm = swap ? p.r + x : p.s + 1.0, pM = swap ? p.s + 1.0 : p.r + x;
  const double e0 = m + tx, eD = e0 + fabs(p.a - p.b);
  const double D = log1p((T - tx) / e0);
  if (!(e0 > 0.0) || !(eD < INFINITY) || !(D < INFINITY)) return false;
  const double q = e0 / eD;
  double d = 0.0, Q = 0.0, Sd = 0.0, SL = 0.0, Sm = 0.0, SM = 0.0;
  bool grew = true;
  for (int k = 0; k < PNBD_Q_PANEL_CAP && d < D; ++k) {
    const double em = expm1(d);
    if ((1.0 - pm) * d - pM * log1p(q * em) < -PNBD_Q_SPAN && !grew) break;
    const double slope = (1.0 - pm) - pM * (q * (em + 1.0) / (1.0 + q * em));
    double hi = d + fmin(1.0, PNBD_Q_SLOPE / fabs(slope));
    if (!(hi < D)) hi = D;
    const double mid = 0.5 * (d + hi), half = 0.5 * (hi - d);
    double c = 0.0, cd = 0.0, cL = 0.0, cm = 0.0, cM = 0.0;
    for (int j = 0; j < CLV_GL_Q; ++j) {
      const double dj = mid + half * X[j];
      const double ej = expm1(dj), u = q * ej;
      const double Lj = log1p(u);
      const double g = W[j] * exp((1.0 - pm) * dj - pM * Lj);
      c += g;
      cd += g * dj;
      cL += g * Lj;
      cm += g / (e0 * (ej + 1.0));
      cM += g / (eD * (1.0 + u));
    }
    const double nQ = Q + c * half;
    grew = nQ != Q;
    Q = nQ;
    Sd += cd * half;
    SL += cL * half;
    Sm += cm * half;
    SM += cM * half;
    d = hi;
  }
  *logsI = -INFINITY;
  for (int j = 0; j < 4; ++j) dI[j] = 0.0;
  if (Q > 0.0) {
    const double l0 = log(e0), lD = log(eD);
    *logsI = log(p.s) + (((1.0 - pm) * l0 - pM * lD) + log(Q));
    const double lm = l0 + Sd / Q, lM = lD + SL / Q, im = Sm / Q, iM = SM / Q;
    const double rx = p.r + x, s1 = p.s + 1.0;
    dI[0] = -(swap ? lm : lM);
    dI[1] = -rx * (swap ? im : iM);
    dI[2] = -(swap ? lM : lm) + 1.0 / p.s;
    dI[3] = -s1 * (swap ? iM : im);
  }
  return true;
}

// One customer: log L, its gradient with respect to log(r, alpha, s, beta), and P(alive) =
// A / (A + s I) with A the survivor term.  A series that hit the cap makes all of them NaN.  MODE: where
// s I comes from.  PNBD_SERIES: the series, whatever it needs.  PNBD_AUTO: the series as above where
// z(t_x) <= PNBD_Z_SWITCH, the quadrature otherwise.  PNBD_QUADRATURE: the quadrature wherever t_x < T.
// On the quadrature path conv = every result is finite.
struct Point {
  double logL, g[4], p_alive;
  bool conv;
};

template <int MODE = PNBD_SERIES>
__host__ __device__ inline Point pnbd_point(int32_t xi, double tx, double T, const Params& p) {
  const double x = (double)xi, rx = p.r + x;
  double dig = 0.0;  // psi(r + x) - psi(r)
  for (int32_t k = 0; k < xi; ++k) dig += 1.0 / (p.r + k);
  const double laT = log(p.a + T), lbT = log(p.b + T);
  const double logA = -rx * laT - p.s * lbT;
  const double dA[4] = {-laT, -rx / (p.a + T), -lbT, -p.s / (p.b + T)};
  double logsI = -INFINITY;
  double dI[4] = {0.0, 0.0, 0.0, 0.0};
  bool conv = true;
  bool quad = false;
  if constexpr (MODE == PNBD_QUADRATURE) quad = tx < T;
  if constexpr (MODE == PNBD_AUTO)
    quad = tx < T && !(fabs(p.a - p.b) / ((p.a < p.b ? p.b : p.a) + tx) <= PNBD_Z_SWITCH);
  if (MODE != PNBD_SERIES && quad) {
    if (!pnbd_si_quadrature(x, tx, T, p, &logsI, dI)) logsI = std::numeric_limits<double>::quiet_NaN();
  } else if (tx < T) {
    const LogH h1 = pnbd_log_h(tx, x, p), h2 = pnbd_log_h(T, x, p);
    conv = h1.conv && h2.conv;
    const double d = h2.lh - h1.lh;
    const double e = exp(d), om = -expm1(d);  // 1 - H(T) / H(t_x)
    const double aa = p.r + p.s + x;
    if (om > 0.0) {
      logsI = log(p.s) + h1.lh + log(om) - log(aa);
      for (int j = 0; j < 4; ++j) dI[j] = (h1.d[j] - e * h2.d[j]) / om;
      dI[0] -= 1.0 / aa;
      dI[2] += 1.0 / p.s - 1.0 / aa;
    }
  }
  const double mx = fmax(logA, logsI);
  const double eA = exp(logA - mx), eI = exp(logsI - mx);
  const double den = eA + eI;
  const double wA = eA / den, wI = eI / den;
  Point o;
  o.conv = conv;
  o.logL = lgamma(rx) - lgamma(p.r) + p.r * log(p.a) + p.s * log(p.b) + (mx + log(den));
  const double base[4] = {dig + log(p.a), p.r / p.a, log(p.b), p.s / p.b};
  const double scale[4] = {p.r, p.a, p.s, p.b};
  for (int j = 0; j < 4; ++j) o.g[j] = (base[j] + wA * dA[j] + wI * dI[j]) * scale[j];
  o.p_alive = wA;
  if (MODE != PNBD_SERIES && quad) {
    conv = (o.logL - o.logL == 0.0) & (wA - wA == 0.0);
    for (int j = 0; j < 4; ++j) conv = conv & (o.g[j] - o.g[j] == 0.0);
    o.conv = conv;
  }
  if (!conv) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    o.logL = o.p_alive = nan;
    for (int j = 0; j < 4; ++j) o.g[j] = nan;
  }
  return o;
}

// -expm1(-k l) / k, and l at k = 0.
__host__ __device__ inline double pnbd_phi(double k, double l) { return k == 0.0 ? l : -expm1(-k * l) / k; }

// E[X(t)] = r beta / alpha phi(s - 1, log((beta + t) / beta)).
__host__ __device__ inline double pnbd_expected(double t, const Params& p) {
  return p.r * p.b / p.a * pnbd_phi(p.s - 1.0, log1p(t / p.b));
}

// theta of the covariate model: the four baseline parameters and the coefficients of each process.
struct CovParams {
  double r, a0, s, b0;
  int32_t k1, k2;
  double g1[PNBD_MAX_COV], g2[PNBD_MAX_COV];
};

// (r, alpha_i, s, beta_i) of customer i: alpha_i = alpha0 exp(-gamma1' z1_i), beta_i = beta0 exp(-gamma2' z2_i)
// (Fader & Hardie 2007, equations 1 and 2).  gamma = 0 or no column: exp(-0) = 1, the baseline bits.
__device__ inline Params pnbd_cov_params(const CovParams& c, const double* z1, const double* z2, int64_t n,
                                         int64_t i) {
  double e1 = 0.0, e2 = 0.0;
  for (int k = 0; k < c.k1; ++k) e1 += c.g1[k] * z1[(int64_t)k * n + i];
  for (int k = 0; k < c.k2; ++k) e2 += c.g2[k] * z2[(int64_t)k * n + i];
  return Params{c.r, c.a0 * exp(-e1), c.s, c.b0 * exp(-e2)};
}

// Where a kernel takes customer i's (r, alpha_i, s, beta_i) from: every kernel below is one body
// compiled for the two sources.  Plain: the same four for every customer, from the kernel arguments.
struct PlainSource {
  static constexpr bool COV = false;
  Params p;
  __device__ Params at(int64_t) const { return p; }
};

// Covariates: the customer's own alpha_i and beta_i, formed per lane from the covariate rows z [k][n].
struct CovSource {
  static constexpr bool COV = true;
  CovParams c;
  const double *z1, *z2;
  int64_t n;
  __device__ Params at(int64_t i) const { return pnbd_cov_params(c, z1, z2, n, i); }
};

// part[b][0..7) = block b's tree sums of w log L, the four w g, w and the unconverged count.  With
// covariates, part[b][7 + k] = tree sum of w g_logalpha,i (-z1[k][i]) for k < k1 and of
// w g_logbeta,i (-z2[k - k1][i]) after them, through the tile in groups of PNBD_COV_GROUP rows (the tile
// is 8 rows high then, 7 without); a row's tree does not see the other rows, so the grouping is not in
// the bits, and the first seven are the plain instance's.
template <class Src, int MODE>
__global__ __launch_bounds__(256) void pnbd_eval_kernel(const int32_t* x, const double* tx, const double* T,
                                                        const double* w, int64_t n, int64_t nb, Src src,
                                                        double* part /*[nb][PNBD_NS + k1 + k2]*/) {
  static_assert(PNBD_COV_GROUP >= PNBD_NS, "the tile holds the seven baseline sums");
  __shared__ double red[Src::COV ? PNBD_COV_GROUP : PNBD_NS][256];
  int nc = 0;
  if constexpr (Src::COV) nc = src.c.k1 + src.c.k2;
  const int ns = PNBD_NS + nc;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t i = b * 256 + threadIdx.x;
    double v[PNBD_NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n) {
      const Params p = src.at(i);
      const Point q = pnbd_point<MODE>(x[i], tx[i], T[i], p);
      const double wi = w ? w[i] : 1.0;
      v[0] = wi * q.logL;
      for (int j = 0; j < 4; ++j) v[1 + j] = wi * q.g[j];
      v[5] = wi;
      v[6] = q.conv ? 0.0 : 1.0;
    }
    for (int k = 0; k < PNBD_NS; ++k) red[k][threadIdx.x] = v[k];
    tree256(red, PNBD_NS);
    if (threadIdx.x < PNBD_NS) part[b * ns + threadIdx.x] = red[threadIdx.x][0];
    __syncthreads();
    if constexpr (Src::COV) {
      for (int k0 = 0; k0 < nc; k0 += PNBD_COV_GROUP) {
        const int m = nc - k0 < PNBD_COV_GROUP ? nc - k0 : PNBD_COV_GROUP;
        for (int j = 0; j < m; ++j) {
          const int k = k0 + j;
          double t = 0.0;
          if (i < n)
            t = k < src.c.k1 ? v[2] * -src.z1[(int64_t)k * n + i] : v[4] * -src.z2[(int64_t)(k - src.c.k1) * n + i];
          red[j][threadIdx.x] = t;
        }
        tree256(red, m);
        if ((int)threadIdx.x < m) part[b * ns + PNBD_NS + k0 + threadIdx.x] = red[threadIdx.x][0];
        __syncthreads();
      }
    }
  }
}

// out[i] = log L, P(alive), E[Y(t*) | x, t_x, T]; with covariates E[Y(t*) | x, t_x, T, z_i] and then the
// score components d log L_i / d log(r, alpha_i, s, beta_i).
template <class Src, int MODE>
__global__ __launch_bounds__(256) void pnbd_customers_kernel(const int32_t* x, const double* tx, const double* T,
                                                             int64_t n, Src src, double t_star,
                                                             double* out /*[n][3], with covariates [n][7]*/) {
  constexpr int W = Src::COV ? 7 : 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const Params p = src.at(i);
    const Point q = pnbd_point<MODE>(x[i], tx[i], T[i], p);
    const double Ti = T[i];
    out[i * W + 0] = q.logL;
    out[i * W + 1] = q.p_alive;
    out[i * W + 2] = q.p_alive * (p.r + (double)x[i]) * (p.b + Ti) / (p.a + Ti) *
                     pnbd_phi(p.s - 1.0, log1p(t_star / (p.b + Ti)));
    if constexpr (Src::COV)
      for (int j = 0; j < 4; ++j) out[i * W + 3 + j] = q.g[j];
  }
}

// part[j][b] = tree sum over block b's customers of E[X(max(times[j] - birth, 0))], with covariates of
// E[X(t) | z_i] = r beta_i / alpha_i phi(s - 1, log((beta_i + t) / beta_i)); grid (blocks, times).
template <class Src>
__global__ __launch_bounds__(256) void pnbd_track_kernel(const double* birth, const double* times, int64_t n,
                                                         int64_t nb, Src src, double* part /*[n_times][nb]*/) {
  __shared__ double red[1][256];
  const double tj = times[blockIdx.y];
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t i = b * 256 + threadIdx.x;
    red[0][threadIdx.x] = i < n ? pnbd_expected(fmax(tj - birth[i], 0.0), src.at(i)) : 0.0;
    tree256(red, 1);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * nb + b] = red[0][0];
    __syncthreads();
  }
}

// sum_j w_j f(x_j) over one 16-point Gauss-Legendre panel [lo, hi].
template <class F>
__host__ __device__ inline double pnbd_gl16(double lo, double hi, F f) {
  constexpr double X[CLV_GL_Q] = CLV_GL_X_INIT, W[CLV_GL_Q] = CLV_GL_W_INIT;
  const double mid = 0.5 * (lo + hi), half = 0.5 * (hi - lo);
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < CLV_GL_Q; ++j) acc += W[j] * f(mid + half * X[j]);
  return acc * half;
}

constexpr double DERT_U_SPLIT = 4.0;   // u = delta (B + t) at which the panels change from log to linear
constexpr double DERT_D_SPAN = 64.0;   // the linear panels stop exp(-64) below their start

// J = int_0^H exp(-delta t) (B / (B + t))^s dt = B int_0^V exp(-z v) (1 + v)^-s dv, z = delta B, V = H / B.
// The integrand has two scales, 1 / z for the exponential and 1 + v for the power, so the panels follow
// u = z (1 + v): while u <= 4 they are uniform in y = log(1 + v), at most 1/2 wide, with the integrand
// exp(-z expm1(y) + (1 - s) y) (entire in y); beyond, uniform in d = z v, at most 1 wide, with the
// integrand exp(-d - s log1p(d / z)) / z (the pole u = 0 is nine half-widths away), cut where exp(-d) has
// fallen by exp(-64).  Every term is positive: nothing cancels for any s, and a short horizon is one
// short panel.  H = inf needs z > 0 (the caller's check).
__host__ __device__ inline double pnbd_dert_integral(double s, double B, double delta, double H) {
  if (!(B > 0.0) || !(B < INFINITY)) return std::numeric_limits<double>::quiet_NaN();  // beta_i under- or overflowed
  const double z = delta * B, V = H / B;
  const double Y = log1p(V);                                    // inf with V
  const double yb = z < DERT_U_SPLIT ? log(DERT_U_SPLIT / z) : 0.0;  // inf at z = 0
  const double Yl = fmin(Y, yb);
  double acc = 0.0;
  if (Yl > 0.0) {
    const int np = (int)ceil(Yl / 0.5);
    const double wd = Yl / np;
    for (int k = 0; k < np; ++k)
      acc += pnbd_gl16(k * wd, k + 1 == np ? Yl : (k + 1) * wd,
                       [=](double y) { return exp(-z * expm1(y) + (1.0 - s) * y); });
  }
  if (Y > yb) {
    const double d0 = z < DERT_U_SPLIT ? DERT_U_SPLIT - z : 0.0;
    const double d1 = fmin(z * V, d0 + DERT_D_SPAN);
    if (d1 > d0) {
      const int np = (int)ceil(d1 - d0);
      const double wd = (d1 - d0) / np;
      double lin = 0.0;
      for (int k = 0; k < np; ++k)
        lin += pnbd_gl16(d0 + k * wd, k + 1 == np ? d1 : d0 + (k + 1) * wd,
                         [=](double d) { return exp(-d - s * log1p(d / z)); });
      acc += lin / z;
    }
  }
  return B * acc;
}

// out[i] = P(alive), DERT = P(alive) (r + x) / (alpha_i + T) J(s, beta_i + T, delta, H).
template <int MODE>
__global__ __launch_bounds__(256) void pnbd_dert_kernel(const int32_t* x, const double* tx, const double* T,
                                                        int64_t n, CovSource src, double delta, double H,
                                                        double* out /*[n][2]*/) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const Params p = src.at(i);
    const double Ti = T[i];
    const Point q = pnbd_point<MODE>(x[i], tx[i], Ti, p);
    out[i * 2 + 0] = q.p_alive;
    out[i * 2 + 1] = q.p_alive * (p.r + (double)x[i]) / (p.a + Ti) * pnbd_dert_integral(p.s, p.b + Ti, delta, H);
  }
}

__global__ __launch_bounds__(256) void pnbd_dert_integral_kernel(const double* s, const double* B, const double* delta,
                                                                 const double* H, int64_t n, double* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = pnbd_dert_integral(s[i], B[i], delta[i], H[i]);
}

int check_params(const double* params, Params* p) {
  if (!params) return fail(CLV_EINVAL, "pnbd: null params");
  for (int j = 0; j < 4; ++j)
    if (!(params[j] > 0.0) || !std::isfinite(params[j]))
      return fail(CLV_EINVAL, "pnbd: params (r, alpha, s, beta) must be positive and finite");
  *p = Params{params[0], params[1], params[2], params[3]};
  return CLV_OK;
}

// params = (r, alpha0, s, beta0, gamma1[k1], gamma2[k2]).
int check_cov_params(const double* params, int32_t k1, int32_t k2, CovParams* c) {
  Params p;
  int rc = check_params(params, &p);
  if (rc) return rc;
  for (int k = 0; k < k1 + k2; ++k)
    if (!std::isfinite(params[4 + k])) return fail(CLV_EINVAL, "pnbd: covariate coefficients must be finite");
  *c = CovParams{};
  c->r = p.r, c->a0 = p.a, c->s = p.s, c->b0 = p.b, c->k1 = k1, c->k2 = k2;
  for (int k = 0; k < k1; ++k) c->g1[k] = params[4 + k];
  for (int k = 0; k < k2; ++k) c->g2[k] = params[4 + k1 + k];
  return CLV_OK;
}

int check_covariates(int64_t n, int32_t k1, const double* z1, int32_t k2, const double* z2) {
  if (k1 < 0 || k2 < 0 || k1 > PNBD_MAX_COV || k2 > PNBD_MAX_COV)
    return fail(CLV_EINVAL, "pnbd: 0..8 covariate columns per process");
  if ((k1 > 0 && !z1) || (k2 > 0 && !z2)) return fail(CLV_EINVAL, "pnbd: null covariates");
  for (int64_t j = 0; j < (int64_t)k1 * n; ++j)
    if (!std::isfinite(z1[j])) return fail(CLV_EINVAL, "pnbd: non-finite purchase covariate");
  for (int64_t j = 0; j < (int64_t)k2 * n; ++j)
    if (!std::isfinite(z2[j])) return fail(CLV_EINVAL, "pnbd: non-finite dropout covariate");
  return CLV_OK;
}

int check_t_star(double t_star) {
  if (!(t_star >= 0.0) || !std::isfinite(t_star)) return fail(CLV_EINVAL, "pnbd: t_star must be >= 0 and finite");
  return CLV_OK;
}

// The two tracking entries: the arguments that need no data first, the values after the parameters.
int check_track_args(int64_t n, const double* birth_week, const double* times, int32_t n_times, const double* cum) {
  if (n <= 0 || n_times < 1 || n_times > 65535) return fail(CLV_EINVAL, "pnbd: n must be >= 1 and n_times in 1..65535");
  if (!birth_week || !times || !cum) return fail(CLV_EINVAL, "pnbd: null argument");
  return CLV_OK;
}

int check_track_values(int64_t n, const double* birth_week, const double* times, int32_t n_times) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(birth_week[i])) return fail(CLV_EINVAL, "pnbd: non-finite birth_week");
  for (int32_t j = 0; j < n_times; ++j)
    if (!std::isfinite(times[j])) return fail(CLV_EINVAL, "pnbd: non-finite time");
  return CLV_OK;
}

// f(integral constant of the handle's mode): the kernel instance is chosen on the host.
template <class F>
void with_integral(const clv_pnbd* h, F f) {
  switch (h->integral) {
    case PNBD_AUTO: f(std::integral_constant<int, PNBD_AUTO>{}); break;
    case PNBD_QUADRATURE: f(std::integral_constant<int, PNBD_QUADRATURE>{}); break;
    default: f(std::integral_constant<int, PNBD_SERIES>{}); break;
  }
}

CovSource cov_source(const clv_pnbd* h, const CovParams& c) {
  return CovSource{c, h->z1.as<const double>(), h->z2.as<const double>(), h->n};
}

// sums[0..6) and *n_unconverged from the seven baseline sums of the handle's customers at src, then the
// nc covariate sums; part and out are the handle's buffers of that width.
template <class Src>
int eval_sums(clv_pnbd* h, const Src& src, int nc, const DevBuf& part, const DevBuf& out, double* sums,
              int64_t* n_unconverged) {
  DeviceScope ds(h->device);
  double res[PNBD_NS + 2 * PNBD_MAX_COV];
  int rc = launch_sums(
      [&] {
        with_integral(h, [&](auto mode) {
          hipLaunchKernelGGL((pnbd_eval_kernel<Src, decltype(mode)::value>), dim3(grid_for(h->nb)), dim3(256), 0, nullptr,
                             h->x.as<const int32_t>(), h->tx.as<const double>(), h->T.as<const double>(),
                             h->w.as<const double>(), h->n, h->nb, src, part.as<double>());
        });
      },
      part.as<const double>(), h->nb, PNBD_NS + nc, 1, out.as<double>(), res);
  if (rc) return rc;
  for (int k = 0; k < 6; ++k) sums[k] = res[k];
  for (int k = 0; k < nc; ++k) sums[6 + k] = res[PNBD_NS + k];
  if (n_unconverged) *n_unconverged = (int64_t)res[6];
  return CLV_OK;
}

// out [n][3], with covariates [n][7]: pnbd_customers_kernel over the handle's customers.
template <class Src>
int customer_rows(clv_pnbd* h, const Src& src, double t_star, double* out) {
  DeviceScope ds(h->device);
  return launch_rows((Src::COV ? 7 : 3) * (size_t)h->n, out, [&](double* d) {
    with_integral(h, [&](auto mode) {
      hipLaunchKernelGGL((pnbd_customers_kernel<Src, decltype(mode)::value>), dim3(grid_for(h->nb)), dim3(256), 0, nullptr,
                         h->x.as<const int32_t>(), h->tx.as<const double>(), h->T.as<const double>(), h->n, src, t_star, d);
    });
  });
}

// cum [n_times] of pnbd_track_kernel at src, on the current device.
template <class Src>
int track_sums(int64_t n, const double* birth_week, const double* times, int32_t n_times, const Src& src, double* cum) {
  const int64_t nb = (n + 255) / 256;
  DevBuf bb, bt, bp, bo;
  int rc;
  if ((rc = upload(bb, birth_week, (size_t)n, nullptr)) || (rc = upload(bt, times, (size_t)n_times, nullptr))) return rc;
  CLV_HIP(hipMalloc(&bp.p, sizeof(double) * (size_t)n_times * (size_t)nb));
  CLV_HIP(hipMalloc(&bo.p, sizeof(double) * (size_t)n_times));
  return launch_sums(
      [&] {
        hipLaunchKernelGGL(pnbd_track_kernel<Src>, dim3(grid_for(nb), (unsigned)n_times), dim3(256), 0, nullptr,
                           bb.as<const double>(), bt.as<const double>(), n, nb, src, bp.as<double>());
      },
      bp.as<const double>(), nb, 1, n_times, bo.as<double>(), cum);
}

}  // namespace

extern "C" {

int clv_pnbd_create(int32_t device, int64_t n, const int32_t* x, const double* t_x, const double* T,
                    const double* weights, clv_pnbd** out) {
  if (!out) return fail(CLV_EINVAL, "pnbd: null handle pointer");
  *out = nullptr;
  if (n <= 0) return fail(CLV_EINVAL, "pnbd: n must be >= 1");
  if (!x || !t_x || !T) return fail(CLV_EINVAL, "pnbd: null x, t_x or T");
  for (int64_t i = 0; i < n; ++i) {
    if (x[i] < 0) return fail(CLV_EINVAL, "pnbd: negative x at customer " + std::to_string(i));
    if (!std::isfinite(t_x[i]) || !std::isfinite(T[i]))
      return fail(CLV_EINVAL, "pnbd: non-finite t_x or T at customer " + std::to_string(i));
    if (t_x[i] < 0.0 || t_x[i] > T[i])
      return fail(CLV_EINVAL, "pnbd: 0 <= t_x <= T violated at customer " + std::to_string(i));
    if (weights && (!std::isfinite(weights[i]) || weights[i] < 0.0))
      return fail(CLV_EINVAL, "pnbd: negative or non-finite weight at customer " + std::to_string(i));
  }
  int rc = check_device(device, "pnbd");
  if (rc) return rc;
  clv_pnbd* h = new clv_pnbd();
  h->n = n;
  h->nb = (n + 255) / 256;
  DeviceScope ds(device);
  rc = [&]() -> int {
    CLV_HIP(hipGetDevice(&h->device));
    int rc;
    if ((rc = upload(h->x, x, (size_t)n, nullptr)) || (rc = upload(h->tx, t_x, (size_t)n, nullptr)) ||
        (rc = upload(h->T, T, (size_t)n, nullptr)) || (rc = upload(h->w, weights, (size_t)n, nullptr)))
      return rc;
    CLV_HIP(hipMalloc(&h->part.p, sizeof(double) * (size_t)h->nb * PNBD_NS));
    CLV_HIP(hipMalloc(&h->out.p, sizeof(double) * PNBD_NS));
    CLV_HIP(hipStreamSynchronize(nullptr));  // the caller's arrays are read
    return CLV_OK;
  }();
  if (rc != CLV_OK) {
    clv_pnbd_destroy(h);
    return rc;
  }
  *out = h;
  return CLV_OK;
}

void clv_pnbd_destroy(clv_pnbd* h) {
  if (!h) return;
  DeviceScope ds(h->device);
  delete h;
}

int clv_pnbd_eval(clv_pnbd* h, const double* params, double* sums, int64_t* n_unconverged) {
  if (!h || !sums) return fail(CLV_EINVAL, "pnbd: null handle or sums");
  Params p;
  int rc = check_params(params, &p);
  if (rc) return rc;
  return eval_sums(h, PlainSource{p}, 0, h->part, h->out, sums, n_unconverged);
}

int clv_pnbd_customers(clv_pnbd* h, const double* params, double t_star, double* out) {
  if (!h || !out) return fail(CLV_EINVAL, "pnbd: null handle or output");
  Params p;
  int rc = check_params(params, &p);
  if (rc || (rc = check_t_star(t_star))) return rc;
  return customer_rows(h, PlainSource{p}, t_star, out);
}

// No device-count check here, and none of device against the count in clv_pnbd_track_cov: a call
// without a usable device fails at its first allocation.
int clv_pnbd_track(int32_t device, int64_t n, const double* birth_week, const double* times, int32_t n_times,
                   const double* params, double* cum) {
  int rc = check_track_args(n, birth_week, times, n_times, cum);
  if (rc) return rc;
  Params p;
  if ((rc = check_params(params, &p)) || (rc = check_track_values(n, birth_week, times, n_times))) return rc;
  DeviceScope ds(device);
  return track_sums(n, birth_week, times, n_times, PlainSource{p}, cum);
}

int clv_pnbd_set_covariates(clv_pnbd* h, int32_t k1, const double* z1, int32_t k2, const double* z2) {
  if (!h) return fail(CLV_EINVAL, "pnbd: null handle");
  int rc = check_covariates(h->n, k1, z1, k2, z2);
  if (rc) return rc;
  DeviceScope ds(h->device);
  DevBuf n1, n2, np, no;  // a failure frees them: the handle keeps what it had
  const size_t ns = (size_t)(PNBD_NS + k1 + k2);
  if ((k1 && (rc = upload(n1, z1, (size_t)k1 * (size_t)h->n, nullptr))) ||
      (k2 && (rc = upload(n2, z2, (size_t)k2 * (size_t)h->n, nullptr))))
    return rc;
  CLV_HIP(hipMalloc(&np.p, sizeof(double) * (size_t)h->nb * ns));
  CLV_HIP(hipMalloc(&no.p, sizeof(double) * ns));
  CLV_HIP(hipStreamSynchronize(nullptr));  // the caller's arrays are read
  std::swap(h->z1.p, n1.p);                // the locals free what the handle had
  std::swap(h->z2.p, n2.p);
  std::swap(h->partc.p, np.p);
  std::swap(h->outc.p, no.p);
  h->k1 = k1, h->k2 = k2, h->has_cov = true;
  return CLV_OK;
}

int clv_pnbd_set_integral(clv_pnbd* h, int32_t mode) {
  if (mode != CLV_PNBD_INTEGRAL_SERIES && mode != CLV_PNBD_INTEGRAL_AUTO && mode != CLV_PNBD_INTEGRAL_QUADRATURE)
    return fail(CLV_EINVAL, "pnbd: integral mode must be CLV_PNBD_INTEGRAL_SERIES, _AUTO or _QUADRATURE");
  if (!h) return fail(CLV_EINVAL, "pnbd: null handle");
  h->integral = mode;
  return CLV_OK;
}

int clv_pnbd_eval_cov(clv_pnbd* h, const double* params, double* sums, int64_t* n_unconverged) {
  if (!h || !sums) return fail(CLV_EINVAL, "pnbd: null handle or sums");
  if (!h->has_cov) return fail(CLV_EINVAL, "pnbd: the handle has no covariates (clv_pnbd_set_covariates)");
  CovParams c;
  int rc = check_cov_params(params, h->k1, h->k2, &c);
  if (rc) return rc;
  return eval_sums(h, cov_source(h, c), h->k1 + h->k2, h->partc, h->outc, sums, n_unconverged);
}

int clv_pnbd_customers_cov(clv_pnbd* h, const double* params, double t_star, double* out) {
  if (!h || !out) return fail(CLV_EINVAL, "pnbd: null handle or output");
  if (!h->has_cov) return fail(CLV_EINVAL, "pnbd: the handle has no covariates (clv_pnbd_set_covariates)");
  CovParams c;
  int rc = check_cov_params(params, h->k1, h->k2, &c);
  if (rc || (rc = check_t_star(t_star))) return rc;
  return customer_rows(h, cov_source(h, c), t_star, out);
}

int clv_pnbd_dert(clv_pnbd* h, const double* params, double delta, double horizon, double* out) {
  if (!h || !out) return fail(CLV_EINVAL, "pnbd: null handle or output");
  CovParams c;
  int rc = check_cov_params(params, h->k1, h->k2, &c);  // k1 = k2 = 0 on a handle without covariates
  if (rc) return rc;
  if (!(delta >= 0.0) || !std::isfinite(delta)) return fail(CLV_EINVAL, "pnbd: delta must be >= 0 and finite");
  if (!(horizon > 0.0)) return fail(CLV_EINVAL, "pnbd: horizon must be > 0 (+inf for an infinite one)");
  if (std::isinf(horizon) && delta == 0.0)
    return fail(CLV_EINVAL, "pnbd: an infinite horizon needs a discount rate > 0");
  DeviceScope ds(h->device);
  return launch_rows(2 * (size_t)h->n, out, [&](double* d) {
    with_integral(h, [&](auto mode) {
      hipLaunchKernelGGL(pnbd_dert_kernel<decltype(mode)::value>, dim3(grid_for(h->nb)), dim3(256), 0, nullptr,
                         h->x.as<const int32_t>(), h->tx.as<const double>(), h->T.as<const double>(), h->n,
                         cov_source(h, c), delta, horizon, d);
    });
  });
}

int clv_dert_integral(int32_t device, int64_t n, const double* s, const double* B, const double* delta,
                      const double* horizon, double* out) {
  if (n <= 0) return fail(CLV_EINVAL, "dert: n must be >= 1");
  if (!s || !B || !delta || !horizon || !out) return fail(CLV_EINVAL, "dert: null argument");
  for (int64_t i = 0; i < n; ++i) {
    if (!(s[i] > 0.0) || !std::isfinite(s[i]) || !(B[i] > 0.0) || !std::isfinite(B[i]))
      return fail(CLV_EINVAL, "dert: s and B must be positive and finite");
    if (!(delta[i] >= 0.0) || !std::isfinite(delta[i])) return fail(CLV_EINVAL, "dert: delta must be >= 0 and finite");
    if (!(horizon[i] > 0.0)) return fail(CLV_EINVAL, "dert: horizon must be > 0 (+inf for an infinite one)");
    if (std::isinf(horizon[i]) && delta[i] == 0.0)
      return fail(CLV_EINVAL, "dert: an infinite horizon needs a discount rate > 0");
  }
  int rc = check_device(device, "dert");
  if (rc) return rc;
  DeviceScope ds(device);
  DevBuf bs, bB, bd, bh;
  if ((rc = upload(bs, s, (size_t)n, nullptr)) || (rc = upload(bB, B, (size_t)n, nullptr)) ||
      (rc = upload(bd, delta, (size_t)n, nullptr)) || (rc = upload(bh, horizon, (size_t)n, nullptr)))
    return rc;
  return launch_rows((size_t)n, out, [&](double* d) {
    hipLaunchKernelGGL(pnbd_dert_integral_kernel, dim3(grid_for((n + 255) / 256)), dim3(256), 0, nullptr,
                       bs.as<const double>(), bB.as<const double>(), bd.as<const double>(), bh.as<const double>(), n, d);
  });
}

int clv_pnbd_track_cov(int32_t device, int64_t n, const double* birth_week, const double* times, int32_t n_times,
                       const double* params, int32_t k1, const double* z1, int32_t k2, const double* z2, double* cum) {
  int rc = check_track_args(n, birth_week, times, n_times, cum);
  if (rc) return rc;
  CovParams c;
  if ((rc = check_covariates(n, k1, z1, k2, z2)) || (rc = check_cov_params(params, k1, k2, &c)) ||
      (rc = check_track_values(n, birth_week, times, n_times)) || (rc = check_device(-1, "pnbd")))
    return rc;
  DeviceScope ds(device);
  DevBuf b1, b2;
  if ((k1 && (rc = upload(b1, z1, (size_t)k1 * (size_t)n, nullptr))) ||
      (k2 && (rc = upload(b2, z2, (size_t)k2 * (size_t)n, nullptr))))
    return rc;
  return track_sums(n, birth_week, times, n_times, CovSource{c, b1.as<const double>(), b2.as<const double>(), n}, cum);
}

}  // extern "C"
