// The closed-form holdout predictive distribution and its forecast scores (DESIGN.md section 4i;
// float64 model: tests/forecast_ref.py).
//
//   clv_forecast / _sampler    per customer: the posterior mean pmf of the holdout count X*, its mean,
//                              P(alive), quantiles, the tail mass and, with x_star, the log score, the
//                              PIT interval and the ranked probability score
//   clv_forecast_info          the limits of this file, for the tests
//   clv_debug_forecast         the same with the customer batch and the grid overridden
//
// Given a draw's (lambda, mu), t = T_star, ml = lambda + mu, y = ml t, a = lambda t, r = lambda / ml,
// w = mu / ml (include/clvmcmc.h):
//   pmf_alive(k) = g_k + v_k,   g_k = exp(-y) a^k / k!,   v_k = w r^k P(k + 1, y).
// Both sequences obey first-order recurrences that run downward in k with positive terms only:
//   g_{k-1} = g_k (k / a),      v_{k-1} = (v_k + w g_k) / r         (P(k, y) = P(k + 1, y) + pi_k).
// fc_draw starts them at k_max - 1 and walks to 0.  The pair is kept as (gh, vh) 2^e with one shared
// integer exponent e, renormalised whenever the larger of the two leaves [2^-128, 2^128): neither
// exp(-y) underflowing (lambda t = 780) nor r^k underflowing loses a value that matters lower down,
// and a member that underflows relative to the other is below 2^-900 of the sum.
// The start:
//   g      at its mode m = min(floor(a), k_max - 1) in the log domain, (m log a - lgamma(m + 1)) - y
//          (arguments of the size of the draw, not of k_max), then multiplied up to k_max - 1;
//   v      = w g S with S = sum_{j >= 1} y^j / (K (K + 1) ... (K + j - 1)), K = k_max, added until the
//          remainder is below 2^-60 of the sum, at most FC_SER_CAP terms;
//   closed branch 1: y > K and y - K - K log(y / K) > 45 (Chernoff: 1 - P(K, y) <= exp(-(y - K - K log(y / K)))
//          = 3e-20; log lambda = 70 lands here): v = w r^(K - 1) from the log domain, no series.  What
//          the branch leaves has S <= 1 / pi_(K-1)(y) < e^45 sqrt(2 pi K): the series cannot overflow,
//          and it is over within (y - K) + sqrt(2 y 42) < 1400 terms at any K <= 4096;
//   a draw with p_alive = 0 exactly (exp(-(ml (T_cal - t_x))) underflows) adds 1 at k = 0 and +0.0
//          elsewhere: the recurrence is skipped;
//   closed branch 2: a < 2^-800 or r < 2^-800 (every pmf_alive(k >= 1) is below 2^-800): k = 0 from
//          its closed form exp(-y) + w (1 - exp(-y)), the rest 0.
// Every loop's trip count is bounded by k_max <= FC_MAX_K or by FC_SER_CAP, whatever the draw.
//
// fc_kernel: a 256-lane workgroup owns a 256-customer block, lane t one customer.  The lane walks the
// draws d = 0 ... n_draws - 1 in order and adds each draw's pmf into its own accumulator row
// acc[k][customer] (global memory, coalesced over the lanes, zeroed by the lane itself), then divides
// by n_draws, forms the statistics in k order and writes its rows.  No lane touches another's
// accumulators: no atomics, no LDS, no barrier; nothing depends on the grid or on the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "analysis_host.h"

using namespace clv;

namespace {

constexpr int FC_BLOCK = 256;                          // customers per workgroup
constexpr int FC_MAX_K = 4096;                         // the largest k_max
constexpr int64_t FC_MAX_DRAWS = 0x7fffffffLL;
constexpr int FC_SER_CAP = 4096;                       // terms of the starting series at most
constexpr int64_t FC_BATCH_DOUBLES = int64_t(1) << 25; // accumulator doubles per batch (256 MiB)
constexpr int FC_MAX_GRID = 1 << 16;
constexpr int FC_CHUNK = 16;                           // recurrence steps per accumulator round trip
constexpr double FC_TINY = 0x1p-800;
constexpr double FC_P1_EXPONENT = 45.0;                // closed branch 1: 1 - P(K, y) <= e^-45
constexpr double FC_LOG2E = 0x1.71547652b82fep+0, FC_LN2 = 0x1.62e42fefa39efp-1;

struct FcArgs {
  const double* level1;  // [n_draws][n][width]
  const double *tx, *T;
  const int32_t* xs;     // x_star or null
  int64_t n_draws, n;
  int width, k_max;
  double t;
};

// exp(l) as m 2^e with m in [1/2, 2] (e = 0 while l > -700); 0 for l below -1e8 or NaN.
__device__ __forceinline__ double exp_scaled(double l, int& e) {
  e = 0;
  if (!(l > -1e8)) return 0.0;
  if (l >= -700.0) return exp(l);
  const double nd = rint(l * FC_LOG2E);
  e = (int)nd;
  return exp(l - nd * FC_LN2);
}

// One draw of one customer: acc[k * stride] += pmf(d, i, k) for k < k_max; the draw's p_alive and
// mean are added to s_pa and s_mean.
__device__ __forceinline__ void fc_draw(const FcArgs& A, double lam, double mu, double dT, double* acc, int64_t stride,
                                        double& s_pa, double& s_mean) {
  const double t = A.t;
  const double ml = lam + mu;
  const double E = exp(-(ml * dT));
  const double den = mu + lam * E;
  const double pa = (ml * E) / den;
  const double pd = (mu * (-expm1(-(ml * dT)))) / den;  // 1 - p_alive without its cancellation
  s_pa = s_pa + pa;
  s_mean = s_mean + (pa * (lam / mu)) * (-expm1(-(mu * t)));
  const double y = ml * t, a = lam * t, w = mu / ml, r = lam / ml;
  if (pa == 0.0) {  // every term below is +0.0
    acc[0] = acc[0] + pd;
    return;
  }
  if (!((a >= FC_TINY) & (r >= FC_TINY))) {
    acc[0] = acc[0] + (pa * (exp(-y) + w * (-expm1(-y))) + pd);
    return;
  }
  const double rinv = ml / lam, ainv = 1.0 / a;
  const int K = A.k_max, top = K - 1;
  const double dK = (double)K;
  // g at its mode, then up to k_max - 1
  const int m = (int)fmin(floor(a), (double)top);
  int e = 0;
  double gh = exp_scaled(m > 0 ? ((double)m * log(a) - lgamma((double)m + 1.0)) - y : -y, e);
  for (int k = m; k < top; ++k) {
    gh = gh * (a / (double)(k + 1));
    if ((gh < 0x1p-128) & (gh > 0.0)) {
      const int s = ilogb(gh);
      gh = ldexp(gh, -s);
      e += s;
    }
  }
  double vh;
  if (y > 1e300 || (y > dK && (y - dK) - dK * log(y / dK) > FC_P1_EXPONENT)) {
    int ev = 0;
    const double vm = exp_scaled(log(w) + (double)top * (-log1p(mu / lam)), ev);
    if (gh == 0.0) {
      e = ev;
      vh = vm;
    } else if (vm == 0.0) {
      vh = 0.0;
    } else if (ev >= e) {
      gh = ldexp(gh, max(e - ev, -2000));
      e = ev;
      vh = vm;
    } else {
      vh = ldexp(vm, max(ev - e, -2000));
    }
  } else {
    double term = y / dK, S = term;
    for (int j = 1; j < FC_SER_CAP; ++j) {
      const double kj = dK + (double)j;
      term = term * (y / kj);
      S = S + term;
      // the terms left add up to less than term y / (kj + 1 - y) once kj + 1 > y
      if ((kj + 1.0 > y) && (term * y < (0x1p-60 * S) * ((kj + 1.0) - y))) break;
    }
    vh = (w * S) * gh;
  }
  // FC_CHUNK steps at a time: the chunk's accumulators are loaded together before the steps and
  // stored together after them, so one memory round trip serves FC_CHUNK steps (a load-add-store
  // inside the recurrence put a full L2 latency into every step); each accumulator still takes
  // exactly one addition per draw
  for (int k0 = top; k0 >= 0; k0 -= FC_CHUNK) {
    double sum[FC_CHUNK];
#pragma unroll
    for (int j = 0; j < FC_CHUNK; ++j) sum[j] = k0 - j >= 0 ? acc[(int64_t)(k0 - j) * stride] : 0.0;
#pragma unroll
    for (int j = 0; j < FC_CHUNK; ++j) {
      const int k = k0 - j;
      if (k >= 0) {
        const double mx = fmax(gh, vh);
        if ((mx >= 0x1p128) | ((mx < 0x1p-128) & (mx > 0.0))) {
          const int s = ilogb(mx);
          gh = ldexp(gh, -s);
          vh = ldexp(vh, -s);
          e += s;
        }
        double tk = pa * ldexp(gh + vh, e);
        if (k == 0) tk = tk + pd;
        sum[j] = sum[j] + tk;
        vh = (vh + w * gh) * rinv;
        gh = gh * ((double)k * ainv);
      }
    }
#pragma unroll
    for (int j = 0; j < FC_CHUNK; ++j)
      if (k0 - j >= 0) acc[(int64_t)(k0 - j) * stride] = sum[j];
  }
}

// Customers [i0, i0 + nc): one workgroup per 256-customer block of the batch; acc [k_max][stride].
__global__ __launch_bounds__(FC_BLOCK) void fc_kernel(FcArgs A, int64_t i0, int64_t nc, int64_t stride, double* acc,
                                                      double* out /*[n][CLV_N_FC_STATS]*/, double* out_pmf) {
  const int t = threadIdx.x;
  const int K = A.k_max;
  const int64_t nblk = (nc + FC_BLOCK - 1) / FC_BLOCK;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double inf = std::numeric_limits<double>::infinity();
  for (int64_t bl = blockIdx.x; bl < nblk; bl += gridDim.x) {
    const int64_t c = bl * FC_BLOCK + t;
    if (c >= nc) continue;
    const int64_t i = i0 + c;
    double* a = acc + c;
    for (int k = 0; k < K; ++k) a[k * stride] = 0.0;
    const double dT = A.T[i] - A.tx[i];
    double s_pa = 0.0, s_mean = 0.0;
    bool bad = false;
    const double* row = A.level1 + i * A.width;
    const int64_t step = A.n * A.width;
    double lam = row[0], mu = row[1];
    for (int64_t d = 0; d < A.n_draws; ++d) {
      double lam_n = 1.0, mu_n = 1.0;
      if (d + 1 < A.n_draws) {  // the next row is in flight during this draw's recurrence
        row += step;
        lam_n = row[0];
        mu_n = row[1];
      }
      if ((lam > 0.0) & (lam < inf) & (mu > 0.0) & (mu < inf) & (lam + mu < inf))
        fc_draw(A, lam, mu, dT, a, stride, s_pa, s_mean);
      else
        bad = true;
      lam = lam_n;
      mu = mu_n;
    }
    const double Sd = (double)A.n_draws;
    const int xs = A.xs ? A.xs[i] : -1;
    double F = 0.0, rps = 0.0, ls = nan, pit_lo = nan, pit_hi = nan;
    int q05 = K, q50 = K, q95 = K;
    for (int k = 0; k < K; ++k) {
      const double p = a[k * stride] / Sd;
      if (out_pmf) out_pmf[i * K + k] = bad ? nan : p;
      if (k == xs) {
        pit_lo = F;
        ls = log(p);
      }
      F = F + p;
      if (k == xs) pit_hi = F;
      if (q05 == K && F >= 0.05) q05 = k;
      if (q50 == K && F >= 0.5) q50 = k;
      if (q95 == K && F >= 0.95) q95 = k;
      const double dev = F - ((xs >= 0 && k >= xs) ? 1.0 : 0.0);
      rps = rps + dev * dev;
    }
    double* o = out + i * CLV_N_FC_STATS;
    o[CLV_FC_XSTAR_MEAN] = bad ? nan : s_mean / Sd;
    o[CLV_FC_P_ALIVE] = bad ? nan : s_pa / Sd;
    o[CLV_FC_P_ZERO] = bad ? nan : a[0] / Sd;
    o[CLV_FC_Q05] = bad ? nan : (double)q05;
    o[CLV_FC_Q50] = bad ? nan : (double)q50;
    o[CLV_FC_Q95] = bad ? nan : (double)q95;
    o[CLV_FC_TAIL_MASS] = bad ? nan : fmax(0.0, 1.0 - F);
    o[CLV_FC_LOG_SCORE] = bad ? nan : ls;
    o[CLV_FC_PIT_LO] = bad ? nan : pit_lo;
    o[CLV_FC_PIT_HI] = bad ? nan : pit_hi;
    o[CLV_FC_RPS] = (bad || xs < 0) ? nan : rps;
  }
}

int check_args(int64_t n_draws, int64_t n, int32_t width, double T_star, int32_t k_max, const int32_t* x_star) {
  if (n_draws < 1 || n < 1) return fail(CLV_EINVAL, "bad shape: no draw or no customer");
  if (n_draws > FC_MAX_DRAWS || n > 0x7fffffffLL)
    return fail(CLV_EINVAL, "bad shape: more than 2^31 - 1 stacked draws or customers");
  if (width != 4 && width != 5) return fail(CLV_EINVAL, "bad level-1 width");
  if (!(T_star > 0.0 && std::isfinite(T_star))) return fail(CLV_EINVAL, "T_star must be finite and > 0");
  if (k_max < 1 || k_max > FC_MAX_K) return fail(CLV_EINVAL, "k_max must be in [1, 4096]");
  if (x_star)
    for (int64_t i = 0; i < n; ++i)
      if (x_star[i] < 0 || x_star[i] >= k_max) return fail(CLV_EINVAL, "x_star outside [0, k_max)");
  return CLV_OK;
}

// level1, tx, T of A on the device; x_star, out and out_pmf on the host.  batch_customers / grid 0:
// the defaults.
int fc_dev(FcArgs A, const int32_t* x_star, int64_t batch_customers, int32_t grid, double* out, double* out_pmf,
           hipStream_t st) {
  const int64_t n = A.n, K = A.k_max;
  const int64_t nb = (n + FC_BLOCK - 1) / FC_BLOCK;
  const int64_t want = batch_customers > 0 ? (batch_customers + FC_BLOCK - 1) / FC_BLOCK
                                           : std::max<int64_t>(1, FC_BATCH_DOUBLES / K / FC_BLOCK);
  const int64_t per_batch = std::min(want, nb) * FC_BLOCK;
  const int64_t max_grid = grid > 0 ? grid : FC_MAX_GRID;
  DevBuf bacc, bo, bp, bxs;
  CLV_HIP(hipMalloc(&bacc.p, sizeof(double) * (size_t)per_batch * K));
  CLV_HIP(hipMalloc(&bo.p, sizeof(double) * (size_t)n * CLV_N_FC_STATS));
  if (out_pmf) CLV_HIP(hipMalloc(&bp.p, sizeof(double) * (size_t)n * K));
  int rc = upload(bxs, x_star, (size_t)n, st);
  if (rc) return rc;
  A.xs = (const int32_t*)bxs.p;
  for (int64_t i0 = 0; i0 < n; i0 += per_batch) {
    const int64_t nc = std::min<int64_t>(per_batch, n - i0);
    const int64_t nblk = (nc + FC_BLOCK - 1) / FC_BLOCK;
    hipLaunchKernelGGL(fc_kernel, dim3((unsigned)std::min<int64_t>(nblk, max_grid)), dim3(FC_BLOCK), 0, st, A, i0, nc,
                       per_batch, (double*)bacc.p, (double*)bo.p, (double*)bp.p);
    CLV_HIP(hipGetLastError());
  }
  CLV_HIP(hipMemcpyAsync(out, bo.p, sizeof(double) * (size_t)n * CLV_N_FC_STATS, hipMemcpyDeviceToHost, st));
  if (out_pmf) CLV_HIP(hipMemcpyAsync(out_pmf, bp.p, sizeof(double) * (size_t)n * K, hipMemcpyDeviceToHost, st));
  CLV_HIP(hipStreamSynchronize(st));
  return CLV_OK;
}

FcArgs make_args(int64_t n_draws, int64_t n, int32_t width, double T_star, int32_t k_max) {
  FcArgs A{};
  A.n_draws = n_draws;
  A.n = n;
  A.width = width;
  A.k_max = k_max;
  A.t = T_star;
  return A;
}

int fc_host(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width, const int32_t* x,
            const double* t_x, const double* T_cal, double T_star, int32_t k_max, const int32_t* x_star,
            int64_t batch_customers, int32_t grid, double* out, double* out_pmf) {
  if (!level1 || !x || !t_x || !T_cal || !out) return fail(CLV_EINVAL, "null argument");
  int rc = check_args(n_draws, n, width, T_star, k_max, x_star);
  if (rc) return rc;
  if (batch_customers < 0 || grid < 0) return fail(CLV_EINVAL, "batch_customers and grid must be >= 0");
  DeviceScope ds(device);
  FcArgs A = make_args(n_draws, n, width, T_star, k_max);
  DevBuf bl, btx, bT;
  if ((rc = upload(bl, level1, (size_t)n_draws * n * width, nullptr)) || (rc = upload(btx, t_x, (size_t)n, nullptr)) ||
      (rc = upload(bT, T_cal, (size_t)n, nullptr)))
    return rc;
  A.level1 = (const double*)bl.p;
  A.tx = (const double*)btx.p;
  A.T = (const double*)bT.p;
  return fc_dev(A, x_star, batch_customers, grid, out, out_pmf, nullptr);
}

}  // namespace

extern "C" {

int clv_forecast_info(int64_t* out) {
  if (!out) return fail(CLV_EINVAL, "null argument");
  out[0] = FC_BLOCK;
  out[1] = FC_MAX_K;
  out[2] = FC_MAX_DRAWS;
  out[3] = FC_SER_CAP;
  out[4] = FC_BATCH_DOUBLES;
  return CLV_OK;
}

int clv_forecast(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width, const int32_t* x,
                 const double* t_x, const double* T_cal, double T_star, int32_t k_max, const int32_t* x_star,
                 double* out, double* out_pmf) {
  return fc_host(device, level1, n_draws, n, width, x, t_x, T_cal, T_star, k_max, x_star, 0, 0, out, out_pmf);
}

int clv_debug_forecast(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                       const int32_t* x, const double* t_x, const double* T_cal, double T_star, int32_t k_max,
                       const int32_t* x_star, int64_t batch_customers, int32_t grid, double* out, double* out_pmf) {
  return fc_host(device, level1, n_draws, n, width, x, t_x, T_cal, T_star, k_max, x_star, batch_customers, grid, out,
                 out_pmf);
}

int clv_forecast_sampler(clv_sampler* s, double T_star, int32_t k_max, const int32_t* x_star, double* out,
                         double* out_pmf) {
  const double* l1;
  int64_t nd;
  int32_t w;
  if (!s || !out) return fail(CLV_EINVAL, "null argument");
  int rc = check_args(1, 1, 4, T_star, k_max, nullptr);  // what needs no sampler, before any device call
  if (rc) return rc;
  rc = sampler_l1(s, &l1, &nd, &w);
  if (rc) return rc;
  rc = check_args(nd, s->g.n, w, T_star, k_max, x_star);
  if (rc) return rc;
  FcArgs A = make_args(nd, s->g.n, w, T_star, k_max);
  A.level1 = l1;
  A.tx = s->d_tx;
  A.T = s->d_T;
  return fc_dev(A, x_star, 0, 0, out, out_pmf, s->stream);
}

}  // extern "C"
