// The Gamma-Gamma model of spend per transaction on device (Fader, Hardie & Lee 2005; Fader & Hardie
// 2013, "The Gamma-Gamma model of monetary value"): the classical opponent of the trivariate model's
// spend dimension, and the expected spend that DERT is multiplied by.  DESIGN.md section 4m; float64
// model: tests/mle_ext_ref.py.
//
//   clv_gg_create / _destroy   frequency n_i >= 1, mean spend m_i > 0 and weights resident for a fit
//   clv_gg_eval                sum w log L and its gradient with respect to log(p, q, gamma)
//   clv_gg_customers           per customer log L and its gradient
//   clv_digamma                the device digamma on an array (the function under test)
//
// Per customer, with a = p n and u = n m / gamma:
//   log L = lnGamma(a + q) - lnGamma(a) - lnGamma(q) + q ln gamma + (a - 1) ln m + a ln n - (a + q) ln(gamma + n m)
//         = D(a, q) - lnGamma(q) - ln m - a log1p(1 / u) - q log1p(u),
// the second line because a ln(n m) - a ln(gamma + n m) and q ln gamma - q ln(gamma + n m) each cancel
// to the size of a logarithm of a ratio: a heavy buyer (a of 1e5..1e6) or a gamma far from n m loses
// nothing.  D(a, q) = lnGamma(a + q) - lnGamma(a) is one function: from a = 32 on, Stirling's series
// differenced term by term, (a - 1/2) log1p(q / a) - q + q ln(a + q) + S(a + q) - S(a), whose error is
// a few ulp of q ln(a + q) and not of lnGamma(a); below 32 the two lgammas are of order 100 at most.
// psi(a + q) - psi(a) likewise: log1p(q / a) + q / (2 a (a + q)) + R(a) - R(a + q).
//   d log L / d log p     = a (psi(a + q) - psi(a) - log1p(1 / u))
//   d log L / d log q     = q (psi(q + a) - psi(q) - log1p(u))
//   d log L / d log gamma = (q u - a) / (1 + u)
// One lane per customer; the sums as csrc/pnbd.hip forms them (pnbd_sum.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "internal.h"
#include "pnbd_sum.h"

using namespace clv;

struct clv_gg {
  int device = 0;
  int64_t n = 0, nb = 0;  // customers, 256-customer blocks
  DevBuf nn;    // int32
  DevBuf m, w;  // double; w null: every weight 1
  DevBuf part;  // [nb][GG_NS]
  DevBuf out;   // [GG_NS]
};

namespace {

constexpr int GG_NS = 5;  // sum w log L, 3 gradient sums, sum w
constexpr double GG_STIRLING_FROM = 32.0;  // a from which the differences use the asymptotic series
constexpr double GG_PSI_SHIFT_TO = 10.0;   // digamma: psi(x) = psi(x + 1) - 1 / x up to here

// R(x) = sum_k B_2k / (2k x^2k), k = 1..7: psi(x) = ln x - 1 / (2x) - R(x); the first term left out at
// x = 10 is 3617 / 8160 x^-16 < 5e-17.
__host__ __device__ inline double gg_psi_tail(double x) {
  const double i2 = 1.0 / (x * x);
  return i2 * (1.0 / 12.0 -
               i2 * (1.0 / 120.0 -
                     i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 - i2 * (691.0 / 32760.0 - i2 / 12.0))))));
}

// psi(x), x > 0: upward shift to 10, then the asymptotic series.
__host__ __device__ inline double gg_digamma(double x) {
  double shift = 0.0;
  while (x < GG_PSI_SHIFT_TO) {
    shift += 1.0 / x;
    x += 1.0;
  }
  return (log(x) - 0.5 / x - gg_psi_tail(x)) - shift;
}

// S(x) = sum_k B_2k / (2k (2k - 1) x^(2k-1)), k = 1..5: lnGamma(x) = (x - 1/2) ln x - x + ln(2 pi) / 2 +
// S(x); the first term left out at x = 32 is 691 / 360360 x^-11 < 6e-20.
__host__ __device__ inline double gg_stirling(double x) {
  const double i = 1.0 / x, i2 = i * i;
  return i * (1.0 / 12.0 - i2 * (1.0 / 360.0 - i2 * (1.0 / 1260.0 - i2 * (1.0 / 1680.0 - i2 / 1188.0))));
}

// lnGamma(a + d) - lnGamma(a), a, d > 0.
__host__ __device__ inline double gg_lgamma_diff(double a, double d) {
  if (a < GG_STIRLING_FROM) return lgamma(a + d) - lgamma(a);
  const double b = a + d;
  return ((a - 0.5) * log1p(d / a) - d) + d * log(b) + (gg_stirling(b) - gg_stirling(a));
}

// psi(a + d) - psi(a), a, d > 0.
__host__ __device__ inline double gg_digamma_diff(double a, double d) {
  if (a < GG_STIRLING_FROM) return gg_digamma(a + d) - gg_digamma(a);
  const double b = a + d;
  return log1p(d / a) + d / (2.0 * a * b) + (gg_psi_tail(a) - gg_psi_tail(b));
}

struct GgPoint {
  double logL, g[3];
};

__host__ __device__ inline GgPoint gg_point(int32_t ni, double m, double p, double q, double gam) {
  const double n = (double)ni, a = p * n;
  const double u = n * m / gam;
  const double l1 = log1p(1.0 / u), l2 = log1p(u);  // log((gamma + n m) / (n m)), log((gamma + n m) / gamma)
  GgPoint o;
  o.logL = gg_lgamma_diff(a, q) - lgamma(q) - log(m) - a * l1 - q * l2;
  o.g[0] = a * (gg_digamma_diff(a, q) - l1);
  o.g[1] = q * (gg_digamma_diff(q, a) - l2);
  o.g[2] = (q * u - a) / (1.0 + u);
  return o;
}

__global__ __launch_bounds__(256) void gg_eval_kernel(const int32_t* nn, const double* m, const double* w, int64_t n,
                                                      int64_t nb, double p, double q, double gam,
                                                      double* part /*[nb][GG_NS]*/) {
  __shared__ double red[GG_NS][256];
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t i = b * 256 + threadIdx.x;
    double v[GG_NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n) {
      const GgPoint t = gg_point(nn[i], m[i], p, q, gam);
      const double wi = w ? w[i] : 1.0;
      v[0] = wi * t.logL;
      for (int j = 0; j < 3; ++j) v[1 + j] = wi * t.g[j];
      v[4] = wi;
    }
    for (int k = 0; k < GG_NS; ++k) red[k][threadIdx.x] = v[k];
    tree256(red, GG_NS);
    if (threadIdx.x < GG_NS) part[b * GG_NS + threadIdx.x] = red[threadIdx.x][0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void gg_customers_kernel(const int32_t* nn, const double* m, int64_t n, double p,
                                                           double q, double gam, double* out /*[n][4]*/) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const GgPoint t = gg_point(nn[i], m[i], p, q, gam);
    out[i * 4 + 0] = t.logL;
    for (int j = 0; j < 3; ++j) out[i * 4 + 1 + j] = t.g[j];
  }
}

__global__ __launch_bounds__(256) void gg_digamma_kernel(const double* x, int64_t n, double* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = gg_digamma(x[i]);
}

int gg_check_params(const double* params) {
  if (!params) return fail(CLV_EINVAL, "gg: null params");
  for (int j = 0; j < 3; ++j)
    if (!(params[j] > 0.0) || !std::isfinite(params[j]))
      return fail(CLV_EINVAL, "gg: params (p, q, gamma) must be positive and finite");
  return CLV_OK;
}

}  // namespace

extern "C" {

int clv_gg_create(int32_t device, int64_t n, const int32_t* frequency, const double* monetary, const double* weights,
                  clv_gg** out) {
  if (!out) return fail(CLV_EINVAL, "gg: null handle pointer");
  *out = nullptr;
  if (n <= 0) return fail(CLV_EINVAL, "gg: n must be >= 1");
  if (!frequency || !monetary) return fail(CLV_EINVAL, "gg: null frequency or monetary");
  for (int64_t i = 0; i < n; ++i) {
    if (frequency[i] < 1) return fail(CLV_EINVAL, "gg: frequency < 1 at customer " + std::to_string(i));
    if (!(monetary[i] > 0.0) || !std::isfinite(monetary[i]))
      return fail(CLV_EINVAL, "gg: monetary value must be > 0 and finite at customer " + std::to_string(i));
    if (weights && (!std::isfinite(weights[i]) || weights[i] < 0.0))
      return fail(CLV_EINVAL, "gg: negative or non-finite weight at customer " + std::to_string(i));
  }
  int rc = check_device(device, "gg");
  if (rc) return rc;
  clv_gg* h = new clv_gg();
  h->n = n;
  h->nb = (n + 255) / 256;
  DeviceScope ds(device);
  rc = [&]() -> int {
    CLV_HIP(hipGetDevice(&h->device));
    int rc;
    if ((rc = upload(h->nn, frequency, (size_t)n, nullptr)) || (rc = upload(h->m, monetary, (size_t)n, nullptr)) ||
        (rc = upload(h->w, weights, (size_t)n, nullptr)))
      return rc;
    CLV_HIP(hipMalloc(&h->part.p, sizeof(double) * (size_t)h->nb * GG_NS));
    CLV_HIP(hipMalloc(&h->out.p, sizeof(double) * GG_NS));
    CLV_HIP(hipStreamSynchronize(nullptr));  // the caller's arrays are read
    return CLV_OK;
  }();
  if (rc != CLV_OK) {
    clv_gg_destroy(h);
    return rc;
  }
  *out = h;
  return CLV_OK;
}

void clv_gg_destroy(clv_gg* h) {
  if (!h) return;
  DeviceScope ds(h->device);
  delete h;
}

int clv_gg_eval(clv_gg* h, const double* params, double* sums) {
  if (!h || !sums) return fail(CLV_EINVAL, "gg: null handle or sums");
  int rc = gg_check_params(params);
  if (rc) return rc;
  DeviceScope ds(h->device);
  return launch_sums(
      [&] {
        hipLaunchKernelGGL(gg_eval_kernel, dim3(grid_for(h->nb)), dim3(256), 0, nullptr, h->nn.as<const int32_t>(),
                           h->m.as<const double>(), h->w.as<const double>(), h->n, h->nb, params[0], params[1], params[2],
                           h->part.as<double>());
      },
      h->part.as<const double>(), h->nb, GG_NS, 1, h->out.as<double>(), sums);
}

int clv_gg_customers(clv_gg* h, const double* params, double* out) {
  if (!h || !out) return fail(CLV_EINVAL, "gg: null handle or output");
  int rc = gg_check_params(params);
  if (rc) return rc;
  DeviceScope ds(h->device);
  return launch_rows(4 * (size_t)h->n, out, [&](double* d) {
    hipLaunchKernelGGL(gg_customers_kernel, dim3(grid_for(h->nb)), dim3(256), 0, nullptr, h->nn.as<const int32_t>(),
                       h->m.as<const double>(), h->n, params[0], params[1], params[2], d);
  });
}

int clv_digamma(int32_t device, int64_t n, const double* x, double* out) {
  if (n <= 0) return fail(CLV_EINVAL, "digamma: n must be >= 1");
  if (!x || !out) return fail(CLV_EINVAL, "digamma: null argument");
  for (int64_t i = 0; i < n; ++i)
    if (!(x[i] > 0.0) || !std::isfinite(x[i])) return fail(CLV_EINVAL, "digamma: arguments must be positive and finite");
  int rc = check_device(device, "digamma");
  if (rc) return rc;
  DeviceScope ds(device);
  DevBuf bi;
  if ((rc = upload(bi, x, (size_t)n, nullptr))) return rc;
  return launch_rows((size_t)n, out, [&](double* d) {
    hipLaunchKernelGGL(gg_digamma_kernel, dim3(grid_for((n + 255) / 256)), dim3(256), 0, nullptr, bi.as<const double>(), n,
                       d);
  });
}

}  // extern "C"
