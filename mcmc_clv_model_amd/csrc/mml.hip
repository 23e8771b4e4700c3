// The log-normal-mixed Pareto/NBD fitted by maximum marginal likelihood: the value and, by Fisher's
// identity, the score of sum_i w_i l_i(beta, Sigma), l_i = log int L_i(a, b) N2((a, b); m_i, Sigma) da db
// the marginal likelihood of csrc/marginal.hip under one record (float64
// model: tests/mml_ref.py).
//
//   clv_mml_create / _destroy   x, t_x, T, weights and the covariate rows [K - 1][n] resident for a fit
//   clv_mml_eval                the 2K + 6 fixed-order sums at one record (beta, Sigma)
//   clv_mml_customers           per customer l_i, P(alive), the five posterior moments, E[X*(t*)]
//   clv_debug_mml_eval          clv_mml_eval with the grid overridden
//   clv_mml_info                the block, VGPRs and scratch bytes per lane of the two kernels, the last eval's device time
//
// With E_i the customer's posterior given the record, (da, db) = (log lambda, log mu) - m_i and P = Sigma^-1,
//   d l_i / d m_i = P E_i[(da, db)],   d l_i / d Sigma = P (S_i - Sigma) P / 2,   S_i = E_i[(da, db)(da, db)'].
// The moments come out of the quadrature loop that forms l_i (marginal_core.h: the same body as
// marginal.hip's, so l_i is its bits): each component's own moments, mixed by wD = exp(iD - l_i) and
// wA = exp(iA - l_i); wA is P(alive | data, record).  The 2 x 2 algebra with P and the chain rule to
// the optimiser's parameters run on the host (mle.py).
//
// Shape.  A 512-lane workgroup takes 256 customers: lane t < 256 integrates customer t's dropped-out
// component, lane 256 + t its alive component (whole waves per component, so no wave diverges), and
// the two meet through LDS, where lane t mixes them.  How the work is spread is not in the bits: a
// component's value depends on the customer and the record alone.  The sums are pnbd_sum.h's: the
// 256-lane tree per block over the first 256 lanes, then pnbd_final_kernel over the block partials.
// No float atomics, no scratch memory.  A customer whose l_i is not finite has a NaN row, makes the
// sums NaN and is counted; it is never dropped.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "marginal_core.h"
#include "pnbd_sum.h"

using namespace clv;

struct clv_mml {
  int device = 0;
  int64_t n = 0, nb = 0;  // customers, 256-customer blocks
  int32_t K = 1;
  DevBuf x;               // int32
  DevBuf tx, T, w, cov;   // double; w null: every weight 1; cov [K - 1][n], null for K = 1
  DevBuf rec, consts;     // [2K + 3], [MARG_NC]
  DevBuf part, out;       // [nb][2K + 6], [2K + 6]
};

namespace {

constexpr int MML_CUST = 256;            // customers per workgroup
constexpr int MML_BLOCK = 2 * MML_CUST;  // lanes: a customer's two components side by side
constexpr int MML_BASE = 6;              // sum w l, sum w, non-finite customers, sum w S (3)
constexpr int MML_GROUP = 8;             // rows of the LDS tile
constexpr int MML_ROW = 8;               // l, P(alive), E[da], E[db], E[da da], E[da db], E[db db], E[X*(t*)]
constexpr int MML_COMP = 1 + MARG_MOM;   // log I and the component's moments

// The device time of the eval kernel of this thread's last clv_mml_eval, in ns (clv_mml_info).
thread_local int64_t last_eval_ns = -1;

struct Events {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~Events() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// Customer lane t's row from its two components in LDS (comp[q][.][t]).
__device__ __forceinline__ void mml_mix(const double (*comp)[MML_COMP][MML_CUST], int t, double* row) {
  const double iD = comp[0][0][t], iA = comp[1][0][t];
  const double hi = fmax(iD, iA), lo = fmin(iD, iA);
  const double l = hi + log1p(exp(lo - hi));
  const bool fin = fabs(iD) <= std::numeric_limits<double>::max() && fabs(iA) <= std::numeric_limits<double>::max();
  const double wD = exp(iD - l), wA = exp(iA - l);
  row[0] = l;
  row[1] = wA;
  for (int k = 0; k < 5; ++k) row[2 + k] = wD * comp[0][1 + k][t] + wA * comp[1][1 + k][t];
  row[7] = wA * comp[1][6][t];
  if (!fin)
    for (int k = 0; k < MML_ROW; ++k) row[k] = std::numeric_limits<double>::quiet_NaN();
}

// The component of lane `lane` (its customer lane % 256, dropped out below 256, alive above) into LDS.
template <int MOM_ALIVE>
__device__ __forceinline__ void mml_component(const MargArgs& A, int64_t i, int lane, double t_star,
                                              double (*comp)[MML_COMP][MML_CUST]) {
  const int q = lane / MML_CUST, t = lane - q * MML_CUST;
  const int K = A.K;
  const double* rec = A.level2;
  const double* rc = A.consts;
  const Rc cs{rc[0], rc[1], rc[2], rc[3], rc[4], rc[5], rc[6], rc[7], rc[8], rc[9], rc[10]};
  double m0 = rec[0], m1 = rec[K];
  for (int k = 1; k < K; ++k) {
    const double xk = A.cov[(int64_t)(k - 1) * A.n + i];
    m0 = m0 + xk * rec[k];
    m1 = m1 + xk * rec[K + k];
  }
  const double x = (double)A.x[i];
  double mo[MARG_MOM];
  double li;
  if (q == 0)
    li = marg_component<false, 1>(A.Q, A.q_at, cs, Cp{x, 1.0, A.tx[i], m0, m1, 0.0}, nullptr, t_star, mo);
  else
    li = marg_component<false, MOM_ALIVE>(A.Q, A.q_at, cs, Cp{x + 1.0, 0.0, A.T[i], m0, m1, 0.0}, nullptr, t_star, mo);
  comp[q][0][t] = li;
#pragma unroll
  for (int k = 0; k < MARG_MOM; ++k) comp[q][1 + k][t] = mo[k];
}

// part[b][0..6) = block b's tree sums of w l, w, the non-finite count and w S (00, 01, 11); then
// part[b][6 + k] = tree sum of w d_ik E_i[da] for k < K and part[b][6 + K + k] of w d_ik E_i[db]
// (d_i0 = 1, d_ik = cov[k - 1][i]), through the tile in groups of MML_GROUP rows; a row's tree does not
// see the other rows.
__global__ __launch_bounds__(MML_BLOCK) void mml_eval_kernel(MargArgs A, const double* w, int64_t nb,
                                                             double* part /*[nb][2K + 6]*/) {
  __shared__ double comp[2][MML_COMP][MML_CUST];
  __shared__ double red[MML_GROUP][256];
  const int lane = threadIdx.x, t = lane % MML_CUST;
  const int nc = 2 * A.K, ns = MML_BASE + nc;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t i = b * MML_CUST + t;
    if (i < A.n) mml_component<1>(A, i, lane, 0.0, comp);
    __syncthreads();
    double row[MML_ROW] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double wi = 0.0;
    const bool own = lane < MML_CUST && i < A.n;
    if (own) {
      mml_mix(comp, t, row);
      wi = w ? w[i] : 1.0;
    }
    if (lane < MML_CUST) {
      red[0][t] = own ? wi * row[0] : 0.0;
      red[1][t] = wi;
      red[2][t] = own && !(fabs(row[0]) <= std::numeric_limits<double>::max()) ? 1.0 : 0.0;
      red[3][t] = own ? wi * row[4] : 0.0;
      red[4][t] = own ? wi * row[5] : 0.0;
      red[5][t] = own ? wi * row[6] : 0.0;
    }
    tree256(red, MML_BASE);
    if (lane < MML_BASE) part[b * ns + lane] = red[lane][0];
    __syncthreads();
    for (int k0 = 0; k0 < nc; k0 += MML_GROUP) {
      const int m = nc - k0 < MML_GROUP ? nc - k0 : MML_GROUP;
      if (lane < MML_CUST)
        for (int j = 0; j < m; ++j) {
          const int k = k0 + j, kk = k < A.K ? k : k - A.K;
          double v = 0.0;
          if (own) {
            const double d = kk == 0 ? 1.0 : A.cov[(int64_t)(kk - 1) * A.n + i];
            v = (wi * d) * (k < A.K ? row[2] : row[3]);
          }
          red[j][t] = v;
        }
      tree256(red, m);
      if (lane < m) part[b * ns + MML_BASE + k0 + lane] = red[lane][0];
      __syncthreads();
    }
  }
}

// out[i][0..8) = l_i, P(alive), E[da], E[db], E[da da], E[da db], E[db db], E[X*(t_star) | data, record].
__global__ __launch_bounds__(MML_BLOCK) void mml_customers_kernel(MargArgs A, int64_t nb, double t_star,
                                                                  double* out /*[n][8]*/) {
  __shared__ double comp[2][MML_COMP][MML_CUST];
  const int lane = threadIdx.x, t = lane % MML_CUST;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t i = b * MML_CUST + t;
    if (i < A.n) mml_component<2>(A, i, lane, t_star, comp);
    __syncthreads();
    if (lane < MML_CUST && i < A.n) {
      double row[MML_ROW];
      mml_mix(comp, t, row);
      for (int k = 0; k < MML_ROW; ++k) out[i * MML_ROW + k] = row[k];
    }
    __syncthreads();  // comp is rewritten by the next block
  }
}

// The record to the device, its constants by marg_prepare_kernel, and the kernels' arguments.
int mml_args(clv_mml* h, const double* record, int32_t nodes, MargArgs* out) {
  MargArgs A{};
  int rc = order_at(nodes, &A.Q, &A.q_at);
  if (rc) return rc;
  CLV_HIP(hipMemcpy(h->rec.p, record, sizeof(double) * (size_t)(2 * h->K + 3), hipMemcpyHostToDevice));
  A.level2 = h->rec.as<const double>();
  A.consts = h->consts.as<const double>();
  A.cov = h->cov.as<const double>();
  A.x = h->x.as<const int32_t>();
  A.tx = h->tx.as<const double>();
  A.T = h->T.as<const double>();
  A.logs = nullptr;
  A.n_rec = 1;
  A.n = h->n;
  A.D = 2;
  A.K = h->K;
  A.omega2 = 1.0;
  hipLaunchKernelGGL(marg_prepare_kernel, dim3(1), dim3(256), 0, nullptr, A, h->consts.as<double>());
  CLV_HIP(hipGetLastError());
  *out = A;
  return CLV_OK;
}

int mml_eval(clv_mml* h, const double* record, int32_t nodes, int32_t grid, double* sums, int64_t* n_nonfinite) {
  if (!h || !record || !sums) return fail(CLV_EINVAL, "mml: null handle, record or sums");
  if (grid < 0) return fail(CLV_EINVAL, "mml: grid must be >= 0");
  DeviceScope ds(h->device);
  MargArgs A;
  int rc = mml_args(h, record, nodes, &A);
  if (rc) return rc;
  const int ns = MML_BASE + 2 * h->K;
  const unsigned g = grid > 0 ? (unsigned)std::min<int64_t>(grid, h->nb) : grid_for(h->nb);
  double res[MML_BASE + 2 * CLV_MAX_K];
  Events ev;
  CLV_HIP(hipEventCreate(&ev.e0));
  CLV_HIP(hipEventCreate(&ev.e1));
  rc = launch_sums(
      [&] {
        (void)hipEventRecord(ev.e0, nullptr);
        hipLaunchKernelGGL(mml_eval_kernel, dim3(g), dim3(MML_BLOCK), 0, nullptr, A, h->w.as<const double>(), h->nb,
                           h->part.as<double>());
        (void)hipEventRecord(ev.e1, nullptr);
      },
      h->part.as<const double>(), h->nb, ns, 1, h->out.as<double>(), res);
  if (rc) return rc;
  float ms = 0.0f;
  CLV_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  last_eval_ns = (int64_t)std::llround((double)ms * 1e6);
  for (int k = 0; k < ns; ++k) sums[k] = res[k];
  if (n_nonfinite) *n_nonfinite = (int64_t)res[2];
  return CLV_OK;
}

}  // namespace

extern "C" {

int clv_mml_create(int32_t device, int64_t n, const int32_t* x, const double* t_x, const double* T,
                   const double* weights, int32_t K, const double* cov, clv_mml** out) {
  if (!out) return fail(CLV_EINVAL, "mml: null handle pointer");
  *out = nullptr;
  if (n <= 0 || n > 0x7fffffffLL) return fail(CLV_EINVAL, "mml: n must be in 1 .. 2^31 - 1");
  if (K < 1 || K > CLV_MAX_K) return fail(CLV_EINVAL, "mml: K must be 1 .. 9");
  if ((K > 1) != (cov != nullptr))
    return fail(CLV_EINVAL, "mml: covariates do not match K (K - 1 rows of n, none for K = 1)");
  if (!x || !t_x || !T) return fail(CLV_EINVAL, "mml: null x, t_x or T");
  for (int64_t i = 0; i < n; ++i) {
    if (x[i] < 0) return fail(CLV_EINVAL, "mml: negative x at customer " + std::to_string(i));
    if (!std::isfinite(t_x[i]) || !std::isfinite(T[i]))
      return fail(CLV_EINVAL, "mml: non-finite t_x or T at customer " + std::to_string(i));
    if (t_x[i] < 0.0 || t_x[i] > T[i])
      return fail(CLV_EINVAL, "mml: 0 <= t_x <= T violated at customer " + std::to_string(i));
    if (weights && (!std::isfinite(weights[i]) || weights[i] < 0.0))
      return fail(CLV_EINVAL, "mml: negative or non-finite weight at customer " + std::to_string(i));
  }
  int rc = check_device(device, "mml");
  if (rc) return rc;
  clv_mml* h = new clv_mml();
  h->n = n;
  h->nb = (n + MML_CUST - 1) / MML_CUST;
  h->K = K;
  DeviceScope ds(device);
  rc = [&]() -> int {
    CLV_HIP(hipGetDevice(&h->device));
    int rc;
    if ((rc = upload(h->x, x, (size_t)n, nullptr)) || (rc = upload(h->tx, t_x, (size_t)n, nullptr)) ||
        (rc = upload(h->T, T, (size_t)n, nullptr)) || (rc = upload(h->w, weights, (size_t)n, nullptr)) ||
        (rc = upload(h->cov, cov, (size_t)(K - 1) * (size_t)n, nullptr)))
      return rc;
    const size_t ns = (size_t)(MML_BASE + 2 * K);
    CLV_HIP(hipMalloc(&h->rec.p, sizeof(double) * (size_t)(2 * K + 3)));
    CLV_HIP(hipMalloc(&h->consts.p, sizeof(double) * MARG_NC));
    CLV_HIP(hipMalloc(&h->part.p, sizeof(double) * (size_t)h->nb * ns));
    CLV_HIP(hipMalloc(&h->out.p, sizeof(double) * ns));
    CLV_HIP(hipStreamSynchronize(nullptr));  // the caller's arrays are read
    return CLV_OK;
  }();
  if (rc != CLV_OK) {
    clv_mml_destroy(h);
    return rc;
  }
  *out = h;
  return CLV_OK;
}

void clv_mml_destroy(clv_mml* h) {
  if (!h) return;
  DeviceScope ds(h->device);
  delete h;
}

int clv_mml_eval(clv_mml* h, const double* record, int32_t nodes, double* sums, int64_t* n_nonfinite) {
  return mml_eval(h, record, nodes, 0, sums, n_nonfinite);
}

int clv_debug_mml_eval(clv_mml* h, const double* record, int32_t nodes, int32_t grid, double* sums,
                       int64_t* n_nonfinite) {
  return mml_eval(h, record, nodes, grid, sums, n_nonfinite);
}

int clv_mml_customers(clv_mml* h, const double* record, int32_t nodes, double t_star, double* out) {
  if (!h || !record || !out) return fail(CLV_EINVAL, "mml: null handle, record or output");
  if (!(t_star >= 0.0) || !std::isfinite(t_star)) return fail(CLV_EINVAL, "mml: t_star must be >= 0 and finite");
  DeviceScope ds(h->device);
  MargArgs A;
  int rc = mml_args(h, record, nodes, &A);
  if (rc) return rc;
  return launch_rows(MML_ROW * (size_t)h->n, out, [&](double* d) {
    hipLaunchKernelGGL(mml_customers_kernel, dim3(grid_for(h->nb)), dim3(MML_BLOCK), 0, nullptr, A, h->nb, t_star, d);
  });
}

int clv_mml_info(int64_t* out) {
  if (!out) return fail(CLV_EINVAL, "null argument");
  hipFuncAttributes fe{}, fc{};
  CLV_HIP(hipFuncGetAttributes(&fe, reinterpret_cast<const void*>(mml_eval_kernel)));
  CLV_HIP(hipFuncGetAttributes(&fc, reinterpret_cast<const void*>(mml_customers_kernel)));
  out[0] = MML_CUST;
  out[1] = MML_BLOCK;
  out[2] = fe.numRegs;
  out[3] = (int64_t)fe.localSizeBytes;
  out[4] = fc.numRegs;
  out[5] = (int64_t)fc.localSizeBytes;
  out[6] = last_eval_ns;
  return CLV_OK;
}

}  // extern "C"
