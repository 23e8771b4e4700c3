// Model comparison on device: pointwise log-likelihood, WAIC and Pareto-smoothed importance-sampling
// leave-one-out (PSIS-LOO; Vehtari, Gelman & Gabry 2017) per customer (float64
// model: tests/ic_ref.py).
//
//   clv_pointwise_loglik                  l[d][i], the Pareto/NBD individual likelihood of customer i
//                                         under draw d's (lambda, mu), marginal over z and tau, plus
//                                         (log_s given) one observation of log_s ~ N(log eta, omega2)
//   clv_psis_loo                          the statistics below from any [n_draws][n] matrix
//   clv_information_criteria / _sampler   the two fused: the matrix never leaves the device
//   clv_ic_info                           the limits of this file, for the tests
//
// With ml = lambda + mu:
//   l = ((x log(lambda) - log(ml)) - ml t_x) + log(mu + lambda exp(-(ml (T_cal - t_x))))
//       [+ (c - ((log_s - log(eta)) (log_s - log(eta))) / (2 omega2)),  c = -log(2 pi omega2) / 2]
//
// ic_pass_kernel: a 256-lane workgroup owns the 256-customer block b, lane t customer 256 b + t, and
// walks the draws in order, IC_TILE at a time.  The owning lane keeps the WAIC accumulators in draw
// order: the running maximum m and sum of exp(l - m) (rescaled when m rises), and Welford's mean and
// sum of squared deviations of l - l_0 (l_0 the first draw's value, so the running mean's rounding
// stays at the deviations' scale); both sums carry Neumaier's compensation.  Per tile the l go through
// LDS as [customer][draw] (rows padded to 17 doubles: conflict-free both ways) and out transposed to
// seg[customer][draw], 16 lanes storing the 128 bytes of one customer's tile; the rows of the next
// tile are loaded before the LDS work.  The same kernel reads l from a caller's matrix instead of
// forming it (clv_psis_loo), so both routes give the same bits.  A non-finite l marks the customer:
// its whole row is NaN.
// The series are sorted exactly (rocprim segmented radix sort, customers in batches of at most
// IC_BATCH_KEYS keys, whole 256-customer blocks).
// ic_fit_kernel: one wavefront per customer.  From the ascending series a: x_j = a_0 - a_j (the log
// ratio minus its maximum), cutoff = max(x_M, log(DBL_MIN)), tail = the n leading j with x_j > cutoff.
// The tail values t = exp(cutoff) expm1(a_M - a_j) (ascending) sit in LDS.  Zhang & Stephens' grid:
// lane j takes grid points j, j + 64, ... and adds log(1 - b_j t_i) over i = 0 ... n - 1 in that order
// with Neumaier's compensation (the profile likelihood multiplies the sum's error by n), then its
// weight 1 / sum_i exp(L_i - L_j) over i in index order, compensated likewise.  The sums over the
// grid (the weights' renormalisation, b), the posterior k (compensated per lane) and the sums over
// the S draws (the two logsumexp) are per lane over the terms lane, lane + 64, ... in turn, then over
// the lanes by the xor tree (offsets 32 ... 1).  No atomics; no sum depends on the grid or on the
// batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "analysis_host.h"

using namespace clv;

namespace {

constexpr int IC_BLOCK = 256;                         // customers per workgroup of the pass
constexpr int IC_TILE = 16;                           // draws per LDS tile of the pass
constexpr int IC_ROW = IC_TILE + 1;                   // its padded row
constexpr int64_t IC_BATCH_KEYS = int64_t(1) << 27;   // keys per sort call (1 GiB of doubles)
constexpr int64_t IC_MIN_DRAWS = 8;
constexpr int64_t IC_MAX_DRAWS = int64_t(1) << 20;    // 256 customers x draws stay below 2^31 keys
constexpr int64_t IC_MAX_TAIL = 4096;                 // tail values a wavefront holds in LDS
constexpr int IC_MAX_POINTS = 30 + 64;                // grid points at the longest tail
constexpr int IC_MAX_GRID = 1 << 16;
constexpr int IC_MIN_FIT = 5;                         // shortest tail that is fitted
constexpr double IC_LOG_TINY = -0x1.6232bdd7abcd2p+9; // log(DBL_MIN)
constexpr double IC_EPS = 0x1p-52;

struct IcArgs {
  const double* level1;  // [n_draws][n][width], or null with ll
  const double* ll;      // [n_draws][n], or null with level1
  const int32_t* x;
  const double *tx, *T, *logs;  // logs null: the transaction part only
  int64_t n_draws, n;
  int width;
  double omega2, c_spend;
};

struct IcData {
  double x, tx, dT, logs;
};

// The log-likelihood of one customer under one draw's row.
__device__ __forceinline__ double ic_loglik(const IcArgs& A, const IcData& c, double lam, double mu, double eta) {
  const double ml = lam + mu;
  double l = ((c.x * log(lam) - log(ml)) - ml * c.tx) + log(mu + lam * exp(-(ml * c.dT)));
  if (A.logs) {
    const double d = c.logs - log(eta);
    l = l + (A.c_spend - (d * d) / (2.0 * A.omega2));
  }
  return l;
}

// acc += v with Neumaier's compensation carried in comp: acc + comp is the sum rounded about once.
__device__ __forceinline__ void nadd(double& acc, double& comp, double v) {
  const double s = acc + v;
  comp = comp + (fabs(acc) >= fabs(v) ? (acc - s) + v : (v - s) + acc);
  acc = s;
}

struct IcRows {
  double a[IC_TILE], b[IC_TILE], c[IC_TILE];  // (lambda, mu, eta), or a = l of the caller's matrix
};

// The rows of draws [d0, d0 + IC_TILE) of customer i; a draw past the end or a customer past n reads
// nothing.
__device__ __forceinline__ void ic_load(const IcArgs& A, int64_t i, bool live, int64_t d0, IcRows& r) {
#pragma unroll
  for (int k = 0; k < IC_TILE; ++k) {
    r.a[k] = 1.0, r.b[k] = 1.0, r.c[k] = 1.0;
    if (live && d0 + k < A.n_draws) {
      if (A.ll) {
        r.a[k] = A.ll[(d0 + k) * A.n + i];
      } else {
        const double* row = A.level1 + ((d0 + k) * A.n + i) * A.width;
        r.a[k] = row[0];
        r.b[k] = row[1];
        if (A.logs) r.c[k] = row[4];
      }
    }
  }
}

// Customers [i0, i0 + nc), i0 a multiple of 256: one workgroup per 256-customer block.  seg (or null)
// takes the batch's series [customer - i0][draw], out (or null) the WAIC columns, ll_out (or null) the
// matrix [draw][customer].
__global__ __launch_bounds__(IC_BLOCK) void ic_pass_kernel(IcArgs A, int64_t i0, int64_t nc, double* seg,
                                                           double* out /*[n][CLV_N_IC_STATS]*/, double* ll_out) {
  __shared__ double lds[IC_BLOCK * IC_ROW];
  const int t = threadIdx.x;
  const int64_t nblk = (nc + IC_BLOCK - 1) / IC_BLOCK;
  for (int64_t bl = blockIdx.x; bl < nblk; bl += gridDim.x) {
    const int64_t c0 = i0 + bl * IC_BLOCK;
    const int64_t i = c0 + t;
    const bool live = i < A.n;
    IcData c{0.0, 0.0, 0.0, 0.0};
    if (live && !A.ll) {
      c.x = (double)A.x[i];
      c.tx = A.tx[i];
      c.dT = A.T[i] - c.tx;
      if (A.logs) c.logs = A.logs[i];
    }
    double m = -std::numeric_limits<double>::infinity(), s = 0.0, sc = 0.0, mean = 0.0, m2 = 0.0, m2c = 0.0, l0 = 0.0;
    bool bad = false;
    IcRows cur, next;
    ic_load(A, i, live, 0, cur);
    for (int64_t d0 = 0; d0 < A.n_draws; d0 += IC_TILE) {
      const int nd = (int)std::min<int64_t>(IC_TILE, A.n_draws - d0);
      double l[IC_TILE];
#pragma unroll
      for (int k = 0; k < IC_TILE; ++k) {
        l[k] = A.ll ? cur.a[k] : ic_loglik(A, c, cur.a[k], cur.b[k], cur.c[k]);
        if (live && k < nd) {
          if (!(fabs(l[k]) <= std::numeric_limits<double>::max())) {
            bad = true;
          } else {
            if (l[k] > m) {
              const double e = exp(m - l[k]);
              s = s * e + 1.0;
              sc = sc * e;
              m = l[k];
            } else {
              nadd(s, sc, exp(l[k] - m));
            }
            // Welford on l - l_0: the running mean stays of the deviations' size, so its rounding does
            // not enter the variance at the scale of l
            if (d0 + k == 0) l0 = l[k];
            const double y = l[k] - l0;
            const double dev = y - mean;
            mean = mean + dev / (double)(d0 + k + 1);
            nadd(m2, m2c, dev * (y - mean));
          }
          if (ll_out) ll_out[(d0 + k) * A.n + i] = l[k];
        }
      }
      ic_load(A, i, live, d0 + IC_TILE, next);  // in flight during the LDS work below
      if (seg) {
#pragma unroll
        for (int k = 0; k < IC_TILE; ++k) lds[t * IC_ROW + k] = l[k];
        __syncthreads();
        // 16 consecutive lanes store the 16 draws of one customer (128 bytes)
        const int dd = t & (IC_TILE - 1);
        if (dd < nd)
          for (int r = t / IC_TILE; r < IC_BLOCK; r += IC_BLOCK / IC_TILE) {
            const int64_t ci = c0 + r;
            if (ci < A.n) seg[(ci - i0) * A.n_draws + d0 + dd] = lds[r * IC_ROW + dd];
          }
        __syncthreads();
      }
      cur = next;
    }
    if (live && out) {
      double* o = out + i * CLV_N_IC_STATS;
      const double nan = std::numeric_limits<double>::quiet_NaN();
      const double S = (double)A.n_draws;
      const double lppd = (m + log(s + sc)) - log(S), pw = (m2 + m2c) / S;
      o[CLV_IC_LPPD] = bad ? nan : lppd;
      o[CLV_IC_P_WAIC] = bad ? nan : pw;
      o[CLV_IC_ELPD_WAIC] = bad ? nan : lppd - pw;
      if (bad) o[CLV_IC_ELPD_LOO] = o[CLV_IC_P_LOO] = o[CLV_IC_PARETO_K] = o[CLV_IC_TAIL_LEN] = nan;
    }
  }
}

// The 64 lanes' values added (or their maximum taken) by the xor tree, offsets 32 ... 1: every lane
// ends with the same bits.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// log(1 - b t) for b = c + 1 / tn (c <= 0 on the grid): log1p(-(b t)) while b t < 1/2; nearer 1 the
// argument is formed as (tn - t) / tn - c t, two terms of one sign, not as the difference of two
// near-equal numbers.
__device__ __forceinline__ double log_1mbt(double b, double c, double t, double tn) {
  const double bt = b * t;
  return bt < 0.5 ? log1p(-bt) : log((tn - t) / tn - c * t);
}

// mean over i = 0 ... n - 1 of log(1 - b t_i), the terms added in index order with Neumaier's
// compensation (the sum's rounding error, times n in the profile likelihood, would otherwise set the
// accuracy of pareto_k).
__device__ __forceinline__ double mean_log1p(double b, double c, const double* t, int n) {
  double acc = 0.0, comp = 0.0;
  const double tn = t[n - 1];
  for (int i = 0; i < n; ++i) nadd(acc, comp, log_1mbt(b, c, t[i], tn));
  return (acc + comp) / (double)n;
}

// One wavefront per customer of the batch: sorted [nc][S] ascending.  Dynamic LDS: tail[M] (the tail
// values, then the smoothed log weights), bs, Ls, ws, cs[IC_MAX_POINTS] (the grid b = c + 1 / t_n,
// its profile likelihoods, its weights, c).
__global__ __launch_bounds__(64) void ic_fit_kernel(const double* sorted, int64_t nc, int64_t S, int64_t M, int64_t i0,
                                                    double* out) {
  extern __shared__ __attribute__((aligned(16))) double ic_lds[];
  double* tail = ic_lds;
  double* bs = ic_lds + M;
  double* Ls = bs + IC_MAX_POINTS;
  double* ws = Ls + IC_MAX_POINTS;
  double* cs = ws + IC_MAX_POINTS;
  const int lane = threadIdx.x;
  const double inf = std::numeric_limits<double>::infinity();
  for (int64_t c = blockIdx.x; c < nc; c += gridDim.x) {
    double* o = out + (i0 + c) * CLV_N_IC_STATS;
    const double lppd = o[CLV_IC_LPPD];
    if (lppd != lppd) continue;  // a non-finite l: the pass has written the row
    const double* a = sorted + c * S;
    const double a0 = a[0];
    const double cutoff = fmax(a0 - a[M], IC_LOG_TINY);
    // the tail: the leading j < M with x_j > cutoff (x descends, so they are a prefix)
    int cnt = 0;
    for (int64_t j = lane; j < M; j += 64) cnt += (a0 - a[j]) > cutoff ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    const int n = cnt;
    double khat = inf;
    if (n >= IC_MIN_FIT) {
      const double ec = exp(cutoff);
      // t = exp(x) - exp(cutoff), ascending, as exp(cutoff) expm1(x - cutoff): no cancellation where a
      // value sits just above the cutoff; x - cutoff = a_M - a_j from the values themselves (one
      // rounding) unless the cutoff is the floor log(DBL_MIN)
      const double aM = a[M];
      const bool at_xM = cutoff == a0 - aM;
      for (int q = lane; q < n; q += 64) {
        const double aj = a[n - 1 - q];
        tail[q] = ec * expm1(at_xM ? aM - aj : (a0 - aj) - cutoff);
      }
      __syncthreads();
      const int mp = 30 + (int)floor(sqrt((double)n));
      const double tq = tail[(int)floor((double)n / 4.0 + 0.5) - 1], tn = tail[n - 1];
      const double dn = (double)n;
      for (int j = lane; j < mp; j += 64) {
        const double cj = (1.0 - sqrt((double)mp / ((double)(j + 1) - 0.5))) / (3.0 * tq);
        const double b = cj + 1.0 / tn;
        const double k = mean_log1p(b, cj, tail, n);
        bs[j] = b;
        cs[j] = cj;
        Ls[j] = dn * ((log(-(b / k)) - k) - 1.0);
      }
      __syncthreads();
      // lane j: the weight of grid point j, the sum over the grid in index order (compensated); a
      // weight below 10 eps is dropped (a NaN weight stays and ends in khat)
      for (int j = lane; j < mp; j += 64) {
        double den = 0.0, denc = 0.0;
        for (int i = 0; i < mp; ++i) nadd(den, denc, exp(Ls[i] - Ls[j]));
        const double w = 1.0 / (den + denc);
        ws[j] = w < 10.0 * IC_EPS ? 0.0 : w;
      }
      __syncthreads();
      // the sums over the grid and the posterior k: lane l takes the terms l, l + 64, ... in turn,
      // the lanes go through the xor tree
      double part = 0.0;
      for (int j = lane; j < mp; j += 64) part = part + ws[j];
      const double wsum = wave_sum(part);
      part = 0.0;
      for (int j = lane; j < mp; j += 64) part = part + bs[j] * (ws[j] / wsum);
      const double bhat = wave_sum(part);
      part = 0.0;
      for (int j = lane; j < mp; j += 64) part = part + cs[j] * (ws[j] / wsum);
      const double chat = wave_sum(part);
      double acc = 0.0, comp = 0.0;
      for (int i = lane; i < n; i += 64) nadd(acc, comp, log_1mbt(bhat, chat, tail[i], tn));
      const double k = wave_sum(acc + comp) / dn;
      const double sigma = -(k / bhat);
      khat = (dn * k + 5.0) / (dn + 10.0);
      __syncthreads();  // tail is read above by every lane, overwritten below
      if (fabs(khat) <= std::numeric_limits<double>::max()) {
        for (int q = lane; q < n; q += 64) {
          const double lp = log1p(-(((double)(q + 1) - 0.5) / dn));
          const double g = fabs(khat) < IC_EPS ? -(sigma * lp) : (sigma * expm1(-(khat * lp))) / khat;
          tail[q] = fmin(log(g + ec), 0.0);
        }
      } else {
        khat = inf;
      }
      __syncthreads();
    }
    const bool smooth = khat < inf;
    auto lw = [&](int64_t j) { return (smooth && j < n) ? tail[n - 1 - j] : a0 - a[j]; };
    // log weights x - logsumexp(x), then elpd_loo = logsumexp(log weight + l)
    double mx = -inf;
    for (int64_t j = lane; j < S; j += 64) mx = fmax(mx, lw(j));
    mx = wave_max(mx);
    double sm = 0.0;
    for (int64_t j = lane; j < S; j += 64) sm = sm + exp(lw(j) - mx);
    const double lse = mx + log(wave_sum(sm));
    double mx2 = -inf;
    for (int64_t j = lane; j < S; j += 64) mx2 = fmax(mx2, (lw(j) - lse) + a[j]);
    mx2 = wave_max(mx2);
    double sm2 = 0.0;
    for (int64_t j = lane; j < S; j += 64) sm2 = sm2 + exp(((lw(j) - lse) + a[j]) - mx2);
    const double elpd = mx2 + log(wave_sum(sm2));
    if (lane == 0) {
      o[CLV_IC_ELPD_LOO] = elpd;
      o[CLV_IC_P_LOO] = lppd - elpd;
      o[CLV_IC_PARETO_K] = khat;
      o[CLV_IC_TAIL_LEN] = (double)n;
    }
    __syncthreads();  // the next customer overwrites tail
  }
}

// M = ceil(min(S / 5, 3 sqrt(S / reff))), the most tail values of a series of S draws.
int64_t tail_max(int64_t S, double reff) {
  return (int64_t)std::ceil(std::min((double)S / 5.0, 3.0 * std::sqrt((double)S / reff)));
}

int check_shape(int64_t n_draws, int64_t n) {
  if (n_draws < IC_MIN_DRAWS || n < 1) return fail(CLV_EINVAL, "bad shape: fewer than 8 draws or no customer");
  if (n_draws > IC_MAX_DRAWS || n > 0x7fffffffLL)
    return fail(CLV_EINVAL, "bad shape: more than 2^20 stacked draws or 2^31 - 1 customers");
  return CLV_OK;
}

int check_l1_args(int64_t n_draws, int64_t n, int32_t width, bool spend, double omega2) {
  int rc = check_shape(n_draws, n);
  if (rc) return rc;
  if (width != 4 && width != 5) return fail(CLV_EINVAL, "bad level-1 width");
  if (spend && width != 5) return fail(CLV_EINVAL, "the spend term needs the eta column (width 5)");
  if (spend && !(omega2 > 0.0 && std::isfinite(omega2))) return fail(CLV_EINVAL, "omega2 must be finite and > 0");
  return CLV_OK;
}

int check_reff(int64_t n_draws, double reff) {
  if (!(reff > 0.0 && std::isfinite(reff))) return fail(CLV_EINVAL, "reff must be finite and > 0");
  if (tail_max(n_draws, reff) > IC_MAX_TAIL) return fail(CLV_EINVAL, "reff gives a tail of more than 4096 draws");
  return CLV_OK;
}

// Every pointer of A on the device; out on the host.  batch_keys / grid 0: the defaults.
int ic_dev(IcArgs A, double reff, int64_t batch_keys, int32_t grid, double* out, hipStream_t st) {
  const int64_t n = A.n, S = A.n_draws;
  const int64_t M = tail_max(S, reff);
  const int64_t nb = (n + IC_BLOCK - 1) / IC_BLOCK;
  const int64_t bk = batch_keys > 0 ? std::min(batch_keys, IC_BATCH_KEYS) : IC_BATCH_KEYS;
  const int64_t per_batch = std::min<int64_t>(std::max<int64_t>(1, bk / S / IC_BLOCK), nb) * IC_BLOCK;
  const int64_t nc_max = std::min<int64_t>(per_batch, n);
  const int64_t max_grid = grid > 0 ? grid : IC_MAX_GRID;
  DevBuf bo, bseg;
  CLV_HIP(hipMalloc(&bo.p, sizeof(double) * n * CLV_N_IC_STATS));
  CLV_HIP(hipMalloc(&bseg.p, sizeof(double) * (size_t)nc_max * S));
  SegSorter<double> sorter;
  int rc = sorter.init(nc_max, S, st);
  if (rc) return rc;
  double* dout = (double*)bo.p;
  const size_t fit_lds = sizeof(double) * (size_t)(M + 4 * IC_MAX_POINTS);
  for (int64_t i0 = 0; i0 < n; i0 += per_batch) {
    const int64_t nc = std::min<int64_t>(per_batch, n - i0);
    const int64_t nblk = (nc + IC_BLOCK - 1) / IC_BLOCK;
    hipLaunchKernelGGL(ic_pass_kernel, dim3((unsigned)std::min<int64_t>(nblk, max_grid)), dim3(IC_BLOCK), 0, st, A, i0,
                       nc, (double*)bseg.p, dout, (double*)nullptr);
    CLV_HIP(hipGetLastError());
    const double* sorted;
    if ((rc = sorter.sort((const double*)bseg.p, nc, &sorted))) return rc;
    hipLaunchKernelGGL(ic_fit_kernel, dim3((unsigned)std::min<int64_t>(nc, max_grid)), dim3(64), fit_lds, st, sorted,
                       nc, S, M, i0, dout);
    CLV_HIP(hipGetLastError());
  }
  CLV_HIP(hipMemcpyAsync(out, dout, sizeof(double) * n * CLV_N_IC_STATS, hipMemcpyDeviceToHost, st));
  CLV_HIP(hipStreamSynchronize(st));
  return CLV_OK;
}

// The customers' data and (optionally) the level-1 draws of host arrays, staged on the device.
struct Staged {
  DevBuf l1, x, tx, T, logs;
};

int stage(IcArgs& A, Staged& b, const double* level1, const int32_t* x, const double* t_x, const double* T_cal,
          const double* log_s, hipStream_t st) {
  const size_t n = (size_t)A.n;
  int rc;
  if ((rc = upload(b.l1, level1, (size_t)A.n_draws * n * A.width, st)) || (rc = upload(b.x, x, n, st)) ||
      (rc = upload(b.tx, t_x, n, st)) || (rc = upload(b.T, T_cal, n, st)) || (rc = upload(b.logs, log_s, n, st)))
    return rc;
  A.level1 = (const double*)b.l1.p;
  A.x = (const int32_t*)b.x.p;
  A.tx = (const double*)b.tx.p;
  A.T = (const double*)b.T.p;
  A.logs = (const double*)b.logs.p;
  return CLV_OK;
}

IcArgs make_args(int64_t n_draws, int64_t n, int32_t width, bool spend, double omega2) {
  IcArgs A{};
  A.n_draws = n_draws;
  A.n = n;
  A.width = width;
  A.omega2 = spend ? omega2 : 1.0;
  A.c_spend = spend ? -0.5 * std::log(2.0 * M_PI * omega2) : 0.0;
  return A;
}

int ic_host(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width, const int32_t* x,
            const double* t_x, const double* T_cal, const double* log_s, double omega2, double reff,
            int64_t batch_keys, int32_t grid, double* out) {
  int rc = check_l1_args(n_draws, n, width, log_s != nullptr, omega2);
  if (rc) return rc;
  rc = check_reff(n_draws, reff);
  if (rc) return rc;
  if (batch_keys < 0 || grid < 0) return fail(CLV_EINVAL, "batch_keys and grid must be >= 0");
  if (!level1 || !x || !t_x || !T_cal || !out) return fail(CLV_EINVAL, "null argument");
  DeviceScope ds(device);
  IcArgs A = make_args(n_draws, n, width, log_s != nullptr, omega2);
  Staged b;
  rc = stage(A, b, level1, x, t_x, T_cal, log_s, nullptr);
  if (rc) return rc;
  return ic_dev(A, reff, batch_keys, grid, out, nullptr);
}

}  // namespace

namespace clv {

int ic_matrix_check(int64_t n_draws, int64_t n, double reff) {
  int rc = check_shape(n_draws, n);
  if (rc) return rc;
  return check_reff(n_draws, reff);
}

int ic_matrix_dev(const double* d_loglik, int64_t n_draws, int64_t n, double reff, double* out, hipStream_t st) {
  IcArgs A = make_args(n_draws, n, 0, false, 1.0);
  A.ll = d_loglik;
  return ic_dev(A, reff, 0, 0, out, st);
}

}  // namespace clv

extern "C" {

int clv_ic_info(int64_t* out) {
  if (!out) return fail(CLV_EINVAL, "null argument");
  out[0] = IC_BLOCK;
  out[1] = IC_TILE;
  out[2] = IC_BATCH_KEYS;
  out[3] = IC_MIN_DRAWS;
  out[4] = IC_MAX_DRAWS;
  out[5] = IC_MAX_TAIL;
  out[6] = IC_MIN_FIT;
  return CLV_OK;
}

int clv_pointwise_loglik(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                         const int32_t* x, const double* t_x, const double* T_cal, const double* log_s,
                         double omega2, double* out) {
  int rc = check_l1_args(n_draws, n, width, log_s != nullptr, omega2);
  if (rc) return rc;
  if (!level1 || !x || !t_x || !T_cal || !out) return fail(CLV_EINVAL, "null argument");
  DeviceScope ds(device);
  IcArgs A = make_args(n_draws, n, width, log_s != nullptr, omega2);
  Staged b;
  rc = stage(A, b, level1, x, t_x, T_cal, log_s, nullptr);
  if (rc) return rc;
  DevBuf bl;
  const size_t bytes = sizeof(double) * (size_t)n_draws * n;
  CLV_HIP(hipMalloc(&bl.p, bytes));
  const int64_t nblk = (n + IC_BLOCK - 1) / IC_BLOCK;
  hipLaunchKernelGGL(ic_pass_kernel, dim3((unsigned)std::min<int64_t>(nblk, IC_MAX_GRID)), dim3(IC_BLOCK), 0, nullptr, A,
                     (int64_t)0, n, (double*)nullptr, (double*)nullptr, (double*)bl.p);
  CLV_HIP(hipGetLastError());
  CLV_HIP(hipMemcpyAsync(out, bl.p, bytes, hipMemcpyDeviceToHost, nullptr));
  CLV_HIP(hipStreamSynchronize(nullptr));
  return CLV_OK;
}

int clv_psis_loo(int32_t device, const double* loglik, int64_t n_draws, int64_t n, double reff, double* out) {
  int rc = check_shape(n_draws, n);
  if (rc) return rc;
  rc = check_reff(n_draws, reff);
  if (rc) return rc;
  if (!loglik || !out) return fail(CLV_EINVAL, "null argument");
  DeviceScope ds(device);
  DevBuf bl;
  if ((rc = upload(bl, loglik, (size_t)n_draws * n, nullptr))) return rc;
  return ic_matrix_dev((const double*)bl.p, n_draws, n, reff, out, nullptr);
}

int clv_information_criteria(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                             const int32_t* x, const double* t_x, const double* T_cal, const double* log_s,
                             double omega2, double reff, double* out) {
  return ic_host(device, level1, n_draws, n, width, x, t_x, T_cal, log_s, omega2, reff, 0, 0, out);
}

int clv_debug_information_criteria(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                                   const int32_t* x, const double* t_x, const double* T_cal, const double* log_s,
                                   double omega2, double reff, int64_t batch_keys, int32_t grid, double* out) {
  return ic_host(device, level1, n_draws, n, width, x, t_x, T_cal, log_s, omega2, reff, batch_keys, grid, out);
}

int clv_information_criteria_sampler(clv_sampler* s, int32_t spend, double omega2, double reff, double* out) {
  const double* l1;
  int64_t nd;
  int32_t w;
  int rc = sampler_l1(s, &l1, &nd, &w);
  if (rc) return rc;
  rc = check_l1_args(nd, s->g.n, w, spend != 0, omega2);
  if (rc) return rc;
  rc = check_reff(nd, reff);
  if (rc) return rc;
  if (!out) return fail(CLV_EINVAL, "null argument");
  if (spend && !s->d_logs) return fail(CLV_ESTATE, "the sampler holds no log_s");
  IcArgs A = make_args(nd, s->g.n, w, spend != 0, omega2);
  A.level1 = l1;
  A.x = s->d_x;
  A.tx = s->d_tx;
  A.T = s->d_T;
  A.logs = spend ? s->d_logs : nullptr;
  return ic_dev(A, reff, 0, 0, out, s->stream);
}

}  // extern "C"
