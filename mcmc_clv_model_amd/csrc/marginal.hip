// The marginal likelihood of a customer under a level-2 record — the customer's own (lambda, mu)
// integrated out against the record's population distribution — and WAIC / PSIS-LOO from it
// (float64 model: tests/marginal_ref.py).
//
//   clv_marginal_loglik                            l_marg[r][i] = log p(x_i, t_x,i, T_i [, log_s_i] | beta_r, Sigma_r)
//   clv_marginal_information_criteria / _sampler   that matrix kept on the device and fed to the
//                                                  statistics of ic.hip (clv_psis_loo): the same bits
//   clv_marginal_info                              the limits of this file and what the last call launched
//   clv_debug_marginal_loglik                      the customer batch and the grid overridden, the centres
//
// With theta = (a, b) = (log lambda, log mu), ml = lambda + mu, the Pareto/NBD individual likelihood is
// the sum of two log-concave components
//   dropped out   lambda^x mu / ml exp(-ml t_x)          (xa, xb, t) = (x, 1, t_x)
//   alive         lambda^(x + 1) / ml exp(-ml T_cal)     (xa, xb, t) = (x + 1, 0, T_cal)
// and each is integrated on its own, the two joined by logaddexp:
//   h(a, b) = (((xa a + xb b) - log(ml)) - ml t) + (c0 - quad / 2) [+ (cs - r r / (2 v))]
//   quad = (P00 da da + 2 P01 da db) + P11 db db, (da, db) = (a - m0, b - m1), P = Sigma_12^-1,
//   c0 = -log(2 pi) - log(det Sigma_12) / 2, m_j = sum_k X_ik beta_kj (k ascending, X_i0 = 1);
//   the spend term (D = 3, log_s given) is log N(log_s; m2 + sc . (da, db), v), sc = Sigma_3,12 P,
//   v = (Sigma_33 - sc . Sigma_12,3) + omega2, r = ((log_s - m2) - sc1 da) - sc2 db: eta integrated out
//   analytically.  h is strictly concave: its negative Hessian is
//   N = [[q qm + lambda t, -q qm], [-q qm, q qm + mu t]] + H,  q = lambda / ml, qm = mu / ml,
//   H = P [+ sc sc' / v]  (where rounding leaves det N <= 0, H alone is used).
// Per component: MARG_NEWTON Newton steps from (m0, m1), a step's larger coordinate capped at
// MARG_STEP_CAP, no early exit (so the centre does not hang on a convergence test that two roundings
// could decide differently); L = the Cholesky factor of N^-1 at the centre (L00 = sqrt(N11 / det),
// L10 = -(N01 / det) / L00, L11 = 1 / sqrt(N11)); then the order-Q Gauss-Hermite rule of
// gauss_hermite.h:
//   log I = log(2 (L00 L11)) + logsumexp_jk((c_j + c_k) + h(a0 + sqrt2 (L00 t_j), b0 + sqrt2 (L10 t_j + L11 t_k)))
// the Q^2 terms through a running maximum in (j, k) order.  Every value is a function of the
// customer's data and covariates and the record alone: nothing depends on the grid or the batch.
//
// The record's constants, the components and the rule live in marginal_core.h, which csrc/mml.hip
// shares (the same bits of l_marg there).
//
// Shape.  marg_prepare_kernel: one lane per record, the record's constants [MARG_NC].
// marg_kernel: a 256-lane workgroup takes a work item = (record, 256-customer block), lane t the
// block's customer t, so the stores to l_marg[r][.] are coalesced and the record's constants and
// the rule's tables are read at wave-uniform addresses (scalar loads).  Grid-stride over the items.
// No atomics, no scratch memory.  A record whose Sigma_12 is not positive definite (or whose v is
// not positive) has NaN constants; a non-finite result is stored as NaN.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "analysis_host.h"
#include "marginal_core.h"

using namespace clv;

namespace {

constexpr int MARG_BLOCK = 256;          // customers per workgroup
constexpr int MARG_MAX_GRID = 1 << 16;
constexpr int64_t MARG_MAX_RECORDS = int64_t(1) << 20;
constexpr int MARG_CENTRE = 12;          // per component: a, b, L00, L10, L11, steps used

// What the last clv_marginal* call of this thread launched (clv_marginal_info).
thread_local int64_t last_info[3] = {-1, -1, -1};  // VGPRs, scratch bytes, kernel ns

// Customers [i0, i0 + nc) of every record: out [n_rec][n]; centre (or null) [n_rec][n][MARG_CENTRE].
template <bool SPEND>
__global__ __launch_bounds__(MARG_BLOCK) void marg_kernel(MargArgs A, int64_t i0, int64_t nc, double* out,
                                                          double* centre) {
  const int t = threadIdx.x;
  const int64_t nblk = (nc + MARG_BLOCK - 1) / MARG_BLOCK;
  const int64_t items = A.n_rec * nblk;
  const int K = A.K;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t r = it / nblk, bl = it - r * nblk;
    const int64_t c = bl * MARG_BLOCK + t;
    if (c >= nc) continue;  // no barrier in this kernel
    const int64_t i = i0 + c;
    const double* rec = A.level2 + r * (A.D * K + A.D * (A.D + 1) / 2);
    const double* rc = A.consts + r * MARG_NC;
    const Rc cs{rc[0], rc[1], rc[2], rc[3], rc[4], rc[5], rc[6], rc[7], rc[8], rc[9], rc[10]};
    double m0 = rec[0], m1 = rec[K], m2 = SPEND ? rec[2 * K] : 0.0;
    for (int k = 1; k < K; ++k) {
      const double xk = A.cov[(int64_t)(k - 1) * A.n + i];
      m0 = m0 + xk * rec[k];
      m1 = m1 + xk * rec[K + k];
      if (SPEND) m2 = m2 + xk * rec[2 * K + k];
    }
    const double x = (double)A.x[i];
    const double r0 = SPEND ? A.logs[i] - m2 : 0.0;
    double* cen = centre ? centre + (r * A.n + i) * MARG_CENTRE : nullptr;
    const double iD = marg_component<SPEND, 0>(A.Q, A.q_at, cs, Cp{x, 1.0, A.tx[i], m0, m1, r0}, cen, 0.0, nullptr);
    const double iA = marg_component<SPEND, 0>(A.Q, A.q_at, cs, Cp{x + 1.0, 0.0, A.T[i], m0, m1, r0},
                                               cen ? cen + 6 : nullptr, 0.0, nullptr);
    const double hi = fmax(iD, iA), lo = fmin(iD, iA);
    const double l = hi + log1p(exp(lo - hi));
    const bool fin = fabs(iD) <= std::numeric_limits<double>::max() && fabs(iA) <= std::numeric_limits<double>::max();
    out[r * A.n + i] = fin ? l : std::numeric_limits<double>::quiet_NaN();
  }
}

// What needs no data, before any device call.
int check_args(int32_t D, int32_t K, bool has_cov, bool spend, double omega2, int64_t n_rec, int64_t n,
               int32_t nodes) {
  if (D != 2 && D != 3) return fail(CLV_EINVAL, "D must be 2 or 3");
  if (K < 1 || K > CLV_MAX_K) return fail(CLV_EINVAL, "K must be 1 .. 9");
  if ((K > 1) != has_cov) return fail(CLV_EINVAL, "covariates do not match K (K - 1 rows of n, none for K = 1)");
  if (spend && D != 3) return fail(CLV_EINVAL, "the spend term (log_s) needs D = 3");
  if (spend && !(omega2 > 0.0 && std::isfinite(omega2))) return fail(CLV_EINVAL, "omega2 must be finite and > 0");
  if (n_rec < 1 || n < 1) return fail(CLV_EINVAL, "bad shape: no record or no customer");
  if (n_rec > MARG_MAX_RECORDS || n > 0x7fffffffLL)
    return fail(CLV_EINVAL, "bad shape: more than 2^20 records or 2^31 - 1 customers");
  int Q, at;
  return order_at(nodes, &Q, &at);
}

// Every pointer of A on the device.  d_out [n_rec][n] on the device; d_centre null or
// [n_rec][n][MARG_CENTRE].  batch_customers / grid 0: the defaults.  Queued on st, not synchronised;
// e0 / e1 (or null) are recorded around the kernels.
int marg_dev(MargArgs A, int32_t nodes, int64_t batch_customers, int32_t grid, double* d_out, double* d_centre,
             DevBuf& consts, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  int rc = order_at(nodes, &A.Q, &A.q_at);
  if (rc) return rc;
  const int64_t nb = (A.n + MARG_BLOCK - 1) / MARG_BLOCK;
  const int64_t want = batch_customers > 0 ? (batch_customers + MARG_BLOCK - 1) / MARG_BLOCK : nb;
  const int64_t per_batch = std::min(want, nb) * MARG_BLOCK;
  const int64_t max_grid = grid > 0 ? grid : MARG_MAX_GRID;
  CLV_HIP(hipMalloc(&consts.p, sizeof(double) * (size_t)A.n_rec * MARG_NC));
  if (e0) CLV_HIP(hipEventRecord(e0, st));
  hipLaunchKernelGGL(marg_prepare_kernel, dim3((unsigned)((A.n_rec + 255) / 256)), dim3(256), 0, st, A,
                     consts.as<double>());
  CLV_HIP(hipGetLastError());
  A.consts = consts.as<double>();
  for (int64_t i0 = 0; i0 < A.n; i0 += per_batch) {
    const int64_t nc = std::min<int64_t>(per_batch, A.n - i0);
    const int64_t items = A.n_rec * ((nc + MARG_BLOCK - 1) / MARG_BLOCK);
    const dim3 g((unsigned)std::min<int64_t>(items, max_grid));
    if (A.logs)
      hipLaunchKernelGGL(marg_kernel<true>, g, dim3(MARG_BLOCK), 0, st, A, i0, nc, d_out, d_centre);
    else
      hipLaunchKernelGGL(marg_kernel<false>, g, dim3(MARG_BLOCK), 0, st, A, i0, nc, d_out, d_centre);
    CLV_HIP(hipGetLastError());
  }
  if (e1) CLV_HIP(hipEventRecord(e1, st));
  return CLV_OK;
}

struct Events {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~Events() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// After the stream has been synchronised: what the call launched.
int note_info(bool spend, const Events& ev) {
  float ms = 0.0f;
  CLV_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  hipFuncAttributes fa{};
  CLV_HIP(hipFuncGetAttributes(&fa, spend ? reinterpret_cast<const void*>(marg_kernel<true>)
                                          : reinterpret_cast<const void*>(marg_kernel<false>)));
  last_info[0] = fa.numRegs;
  last_info[1] = (int64_t)fa.localSizeBytes;
  last_info[2] = (int64_t)std::llround((double)ms * 1e6);
  return CLV_OK;
}

// The matrix (and the centres) of device arrays to the host, or (reff > 0) the statistics of the
// matrix kept on the device.
int marg_run(MargArgs A, int32_t nodes, int64_t batch_customers, int32_t grid, double reff, double* out,
             double* out_centre, hipStream_t st) {
  const size_t cells = (size_t)A.n_rec * (size_t)A.n;
  DevBuf bout, bcen, bconst;
  CLV_HIP(hipMalloc(&bout.p, sizeof(double) * cells));
  if (out_centre) CLV_HIP(hipMalloc(&bcen.p, sizeof(double) * cells * MARG_CENTRE));
  Events ev;
  CLV_HIP(hipEventCreate(&ev.e0));
  CLV_HIP(hipEventCreate(&ev.e1));
  int rc = marg_dev(A, nodes, batch_customers, grid, bout.as<double>(), bcen.as<double>(), bconst, st, ev.e0, ev.e1);
  if (rc) return rc;
  if (reff > 0.0) {
    if ((rc = ic_matrix_dev(bout.as<double>(), A.n_rec, A.n, reff, out, st))) return rc;  // synchronises
  } else {
    CLV_HIP(hipMemcpyAsync(out, bout.p, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    if (out_centre)
      CLV_HIP(hipMemcpyAsync(out_centre, bcen.p, sizeof(double) * cells * MARG_CENTRE, hipMemcpyDeviceToHost, st));
    CLV_HIP(hipStreamSynchronize(st));
  }
  return note_info(A.logs != nullptr, ev);
}

int marg_host(int32_t device, const double* level2, int32_t D, int32_t K, const double* cov, int64_t n_rec, int64_t n,
              const int32_t* x, const double* t_x, const double* T_cal, const double* log_s, double omega2,
              int32_t nodes, int64_t batch_customers, int32_t grid, double reff, double* out, double* out_centre) {
  int rc = check_args(D, K, cov != nullptr, log_s != nullptr, omega2, n_rec, n, nodes);
  if (rc) return rc;
  if (reff > 0.0 && (rc = ic_matrix_check(n_rec, n, reff))) return rc;
  if (!level2 || !x || !t_x || !T_cal || !out) return fail(CLV_EINVAL, "null argument");
  if (batch_customers < 0 || grid < 0) return fail(CLV_EINVAL, "batch_customers and grid must be >= 0");
  DeviceScope ds(device);
  MargArgs A{};
  A.n_rec = n_rec;
  A.n = n;
  A.D = D;
  A.K = K;
  A.omega2 = log_s ? omega2 : 1.0;
  DevBuf b2, bc, bx, btx, bT, bl;
  if ((rc = upload(b2, level2, (size_t)n_rec * (D * K + D * (D + 1) / 2), nullptr)) ||
      (rc = upload(bc, cov, (size_t)(K - 1) * n, nullptr)) || (rc = upload(bx, x, (size_t)n, nullptr)) ||
      (rc = upload(btx, t_x, (size_t)n, nullptr)) || (rc = upload(bT, T_cal, (size_t)n, nullptr)) ||
      (rc = upload(bl, log_s, (size_t)n, nullptr)))
    return rc;
  A.level2 = b2.as<double>();
  A.cov = bc.as<double>();
  A.x = bx.as<int32_t>();
  A.tx = btx.as<double>();
  A.T = bT.as<double>();
  A.logs = bl.as<double>();
  return marg_run(A, nodes, batch_customers, grid, reff, out, out_centre, nullptr);
}

}  // namespace

extern "C" {

int clv_marginal_info(int64_t* out) {
  if (!out) return fail(CLV_EINVAL, "null argument");
  for (int k = 0; k < CLV_GH_N_ORDERS; ++k) out[k] = GH_ORDERS[k];
  out[4] = CLV_MARGINAL_DEFAULT_NODES;
  out[5] = MARG_NEWTON;
  out[6] = MARG_BLOCK;
  out[7] = MARG_MAX_RECORDS;
  out[8] = last_info[0];
  out[9] = last_info[1];
  out[10] = last_info[2];
  return CLV_OK;
}

int clv_marginal_loglik(int32_t device, const double* level2, int32_t D, int32_t K, const double* cov,
                        int64_t n_records, int64_t n, const int32_t* x, const double* t_x, const double* T_cal,
                        const double* log_s, double omega2, int32_t nodes, double* out) {
  return marg_host(device, level2, D, K, cov, n_records, n, x, t_x, T_cal, log_s, omega2, nodes, 0, 0, 0.0, out,
                   nullptr);
}

int clv_debug_marginal_loglik(int32_t device, const double* level2, int32_t D, int32_t K, const double* cov,
                              int64_t n_records, int64_t n, const int32_t* x, const double* t_x, const double* T_cal,
                              const double* log_s, double omega2, int32_t nodes, int64_t batch_customers, int32_t grid,
                              double* out, double* out_centre) {
  return marg_host(device, level2, D, K, cov, n_records, n, x, t_x, T_cal, log_s, omega2, nodes, batch_customers, grid,
                   0.0, out, out_centre);
}

int clv_marginal_information_criteria(int32_t device, const double* level2, int32_t D, int32_t K, const double* cov,
                                      int64_t n_records, int64_t n, const int32_t* x, const double* t_x,
                                      const double* T_cal, const double* log_s, double omega2, int32_t nodes,
                                      double reff, double* out) {
  if (!(reff > 0.0 && std::isfinite(reff))) return fail(CLV_EINVAL, "reff must be finite and > 0");
  return marg_host(device, level2, D, K, cov, n_records, n, x, t_x, T_cal, log_s, omega2, nodes, 0, 0, reff, out,
                   nullptr);
}

int clv_marginal_information_criteria_sampler(clv_sampler* s, int32_t spend, double omega2, double reff, int32_t nodes,
                                              double* out) {
  if (!s || !out) return fail(CLV_EINVAL, "null argument");
  const Geometry& g = s->g;
  const int64_t n_rec = (int64_t)g.n_chains * g.n_draws;
  int rc = check_args(g.D, g.K, g.K > 1, spend != 0, omega2, n_rec, g.n, nodes);
  if (rc) return rc;
  if (!(reff > 0.0 && std::isfinite(reff))) return fail(CLV_EINVAL, "reff must be finite and > 0");
  if ((rc = ic_matrix_check(n_rec, g.n, reff))) return rc;
  if (spend && !s->d_logs) return fail(CLV_ESTATE, "the sampler holds no log_s");
  MargArgs A{};
  if ((rc = sampler_l2(s, &A.level2, "the run has not stored all of its level-2 records yet"))) return rc;
  A.n_rec = n_rec;
  A.n = g.n;
  A.D = g.D;
  A.K = g.K;
  A.omega2 = spend ? omega2 : 1.0;
  A.cov = s->d_cov;
  A.x = s->d_x;
  A.tx = s->d_tx;
  A.T = s->d_T;
  A.logs = spend ? s->d_logs : nullptr;
  return marg_run(A, nodes, 0, 0, reff, out, nullptr, s->stream);
}

}  // extern "C"
