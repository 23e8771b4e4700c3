// MCMC convergence diagnostics on device: per series of m chains x n draws
// the split-chain R-hat and the mean effective sample size of BDA3 / Stan / ArviZ (no rank
// normalisation: az.summary reports the rank-normalised variants), with mean, sd and MCSE, and the
// per-chain autocorrelation function of az.plot_autocorr.  The reference runs ArviZ on its level-2
// draws only (bivariate/analysis_abe.py:651-706); here every customer's (lambda, mu, tau, z, eta) is
// a series too.
//
//   clv_diagnostics          host array [chain][draw][n_series]  -> [n_series][CLV_N_DIAG_STATS]
//   clv_diagnostics_sampler  the level-1 / level-2 draws a sampler holds in HBM (no host copy)
//   clv_autocorr             host array -> [chain][n_series][max_lag + 1]
//   clv_rank_diagnostics[_sampler]  the rank-normalised columns of az.summary (rank R-hat, bulk and
//                            tail ESS, MCSE of the sd, HDI, median): a workgroup per series, see
//                            "Rank-normalised diagnostics" below -> [n_series][CLV_N_RANK_STATS]
//
// Batches of series are transposed to contiguous [series][chain][draw] (the log of the logged
// series taken on the way), then one wavefront owns a series: it stages it in LDS (series of more
// than DIAG_LDS_ELEMS values stay in global memory, same code), centres the split chains in place
// and evaluates the autocovariance 64 lags at a time, one lag per lane — c[i] is a broadcast read,
// c[i + t] a conflict-free one — only as far as Geyer's initial positive sequence asks.  Every sum
// runs in an order fixed by (m, n) alone: lanes stride the series and combine in a xor butterfly,
// a lag's products are added in draw order, split chains in chain order.  Plain launches only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "fastmath.h"
#include "analysis_host.h"

using namespace clv;

namespace {

constexpr int DIAG_LANES = 64;
constexpr int64_t DIAG_LDS_ELEMS = 8192;              // 64 KiB of doubles: 4 x 1000 draws take half
constexpr int64_t DIAG_BATCH_ELEMS = int64_t(1) << 27;  // scratch bound per batch (1 GiB of doubles)
constexpr int DIAG_TILE = 32;

// [chain * draw][n_series] -> [series of the batch][chain * draw] through a 32 x 32 LDS tile (both
// sides move 256-byte rows); series s is logged when bit s % period of log_mask is set.
__global__ __launch_bounds__(256) void diag_gather_kernel(const double* in, int64_t mn, int64_t n_series, int64_t s0,
                                                          int64_t nc, int period, uint32_t log_mask, double* seg) {
  __shared__ double tile[DIAG_TILE][DIAG_TILE + 1];
  const int64_t tiles_s = (nc + DIAG_TILE - 1) / DIAG_TILE;
  const int64_t td = (int64_t)blockIdx.x / tiles_s, ts = (int64_t)blockIdx.x - td * tiles_s;
  const int tx = threadIdx.x & (DIAG_TILE - 1), ty = threadIdx.x / DIAG_TILE;
  for (int r = ty; r < DIAG_TILE; r += 256 / DIAG_TILE) {
    const int64_t d = td * DIAG_TILE + r, c = ts * DIAG_TILE + tx;
    if (d < mn && c < nc) {
      double v = in[d * n_series + s0 + c];
      if ((log_mask >> (uint32_t)((s0 + c) % period)) & 1u) v = log(v);
      tile[r][tx] = v;
    }
  }
  __syncthreads();
  for (int r = ty; r < DIAG_TILE; r += 256 / DIAG_TILE) {
    const int64_t c = ts * DIAG_TILE + r, d = td * DIAG_TILE + tx;
    if (c < nc && d < mn) seg[c * mn + d] = tile[tx][r];
  }
}

// Sum over the wavefront, the same bits in every lane (a + b == b + a at every butterfly level).
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = DIAG_LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, DIAG_LANES);
  return v;
}

// One segment's biased autocovariance at this lane's lag t (tbase = lane 0's): (1/h) sum_{i < h - t}
// c[i] c[i + t], the products added in draw order.  Lanes with t >= h return 0.
__device__ __forceinline__ double lag_chain(const double* c, int64_t h, int64_t t, int64_t tbase) {
  const int64_t full = std::max<int64_t>(0, h - tbase - (DIAG_LANES - 1));  // i + t < h in every lane
  const int64_t any = std::max<int64_t>(0, h - tbase);                      // i + t < h in lane 0
  double acc = 0.0;
#pragma unroll 4
  for (int64_t i = 0; i < full; ++i) acc += c[i] * c[i + t];
  for (int64_t i = full; i < any; ++i)
    if (i + t < h) acc += c[i] * c[i + t];
  return acc / (double)h;
}

// Mean over the nseg segments of lag_chain, added in segment order.  Segment j begins at (j / 2) n +
// (j % 2) (n - h): the split chains of [chain][n] draws, or (nseg 1, h == n) one whole chain.
__device__ __forceinline__ double lag_block(const double* buf, int nseg, int64_t n, int64_t h, int64_t t,
                                            int64_t tbase) {
  double asum = 0.0;
  for (int j = 0; j < nseg; ++j)
    asum += lag_chain(buf + (int64_t)(j >> 1) * n + (int64_t)(j & 1) * (n - h), h, t, tbase);
  return asum / (double)nseg;
}

// The estimator's tail, by one wavefront on split chains already centred in buf (segments as in
// lag_block), varmu the variance of their means: W, V (R-hat = sqrt(V / W)) and, when full, the
// effective sample size with its truncation lag T.  False when W == 0 (no within-chain variance).
// a_first is the caller's lag_block(buf, M, n, h, lane, 0), the first 64 lags.
__device__ __forceinline__ bool geyer_ess(const double* buf, int M, int64_t n, int64_t h, double varmu, int lane,
                                          bool full, double a_first, double& W, double& V, double& ess, int64_t& T) {
  int64_t tbase = 0;
  double a = a_first;
  const double a0 = __shfl(a, 0, DIAG_LANES);
  W = a0 * (double)h / (double)(h - 1);
  V = a0 + varmu;
  if (W == 0.0) return false;
  if (!full) return true;
  // rho(t) for non-decreasing t: the next 64 lags are evaluated when t leaves the block in hand
  auto rho = [&](int64_t t) -> double {
    while (t >= tbase + DIAG_LANES) {
      tbase += DIAG_LANES;
      a = lag_block(buf, M, n, h, tbase + lane, tbase);
    }
    return 1.0 - (W - __shfl(a, (int)(t - tbase), DIAG_LANES)) / V;
  };
  // Geyer's initial positive sequence with the initial monotone sequence applied as pairs are
  // passed: a pair (r[t-1], r[t]) enters the sum S = sum_{0..T} r once the pair after it has been
  // evaluated, capped by the pair before it; the last pair evaluated, (r[T+1], r[T+2]), never does.
  double even = 1.0, odd = rho(1);
  int64_t t = 1;
  double S = 0.0, pe = 0.0, po = 0.0;
  bool have_prev = false, stored = true;
  while (t < h - 3 && even + odd > 0.0) {
    double le = even, lo = odd;
    if (have_prev && le + lo > pe + po) le = lo = (pe + po) / 2.0;
    S += le;
    S += lo;
    pe = le;
    po = lo;
    have_prev = true;
    even = rho(t + 1);
    odd = rho(t + 2);
    stored = even + odd >= 0.0;
    t += 2;
  }
  T = t - 2;
  double r_last = stored ? even : 0.0;  // r[T+1]
  if (even > 0.0) r_last = even;
  double tau = -1.0 + 2.0 * S + r_last;
  const double Mh = (double)M * (double)h;
  tau = fmax(tau, 1.0 / log10(Mh));
  ess = Mh / tau;
  return true;
}

// One wavefront per series of the batch; seg [series][chain][n] (centred in place on the global path).
template <bool LDS>
__global__ __launch_bounds__(DIAG_LANES) void diag_kernel(double* seg, int m, int64_t n, int64_t nc, int64_t s0,
                                                          double* out /*[n_series][CLV_N_DIAG_STATS]*/) {
  extern __shared__ double diag_smem[];
  const int64_t sidx = blockIdx.x;
  if (sidx >= nc) return;
  const int lane = threadIdx.x;
  const int64_t mn = (int64_t)m * n;
  double* g = seg + sidx * mn;
  double* buf = LDS ? diag_smem : g;
  double* o = out + (s0 + sidx) * CLV_N_DIAG_STATS;

  double s = 0.0;
  int bad = 0;
  for (int64_t i = lane; i < mn; i += DIAG_LANES) {
    const double v = g[i];
    if (LDS) buf[i] = v;
    s += v;
    bad |= !std::isfinite(v);
  }
  if (__any(bad)) {
    if (lane < CLV_N_DIAG_STATS) o[lane] = NAN;
    return;
  }
  __syncthreads();
  const double mean = wave_sum(s) / (double)mn;
  double ss = 0.0;
  for (int64_t i = lane; i < mn; i += DIAG_LANES) {
    const double d = buf[i] - mean;
    ss += d * d;
  }
  const double sd = sqrt(wave_sum(ss) / (double)(mn - 1));

  // split chains: means (twice, for their variance about the grand mean), then centred in place
  const int M = 2 * m;
  const int64_t h = n / 2;
  double musum = 0.0;
  for (int j = 0; j < M; ++j) {
    const double* c = buf + (int64_t)(j >> 1) * n + (int64_t)(j & 1) * (n - h);
    double a = 0.0;
    for (int64_t i = lane; i < h; i += DIAG_LANES) a += c[i];
    musum += wave_sum(a) / (double)h;
  }
  const double mubar = musum / (double)M;
  double muss = 0.0;
  for (int j = 0; j < M; ++j) {
    double* c = buf + (int64_t)(j >> 1) * n + (int64_t)(j & 1) * (n - h);
    double a = 0.0;
    for (int64_t i = lane; i < h; i += DIAG_LANES) a += c[i];
    const double mu = wave_sum(a) / (double)h;
    muss += (mu - mubar) * (mu - mubar);
    for (int64_t i = lane; i < h; i += DIAG_LANES) c[i] -= mu;
  }
  __syncthreads();
  const double varmu = muss / (double)(M - 1);

  double W, V, ess;
  int64_t T;
  if (!geyer_ess(buf, M, n, h, varmu, lane, true, lag_block(buf, M, n, h, lane, 0), W, V, ess, T)) {
    if (lane < CLV_N_DIAG_STATS) o[lane] = NAN;
    return;
  }
  if (lane == 0) {
    o[CLV_DIAG_MEAN] = mean;
    o[CLV_DIAG_SD] = sd;
    o[CLV_DIAG_MCSE] = sd / sqrt(ess);
    o[CLV_DIAG_ESS] = ess;
    o[CLV_DIAG_RHAT] = sqrt(V / W);
    o[CLV_DIAG_LAG] = (double)T;
  }
}

// acf_c(t) = A_c(t) / A_c(0) of every unsplit chain (centred at the chain mean, divisor n).
template <bool LDS>
__global__ __launch_bounds__(DIAG_LANES) void acf_kernel(double* seg, int m, int64_t n, int64_t nc, int64_t s0,
                                                         int64_t n_series, int max_lag,
                                                         double* out /*[chain][n_series][max_lag + 1]*/) {
  extern __shared__ double diag_smem[];
  const int64_t sidx = blockIdx.x;
  if (sidx >= nc) return;
  const int lane = threadIdx.x;
  const int64_t mn = (int64_t)m * n;
  double* g = seg + sidx * mn;
  double* buf = LDS ? diag_smem : g;
  if (LDS) {
    for (int64_t i = lane; i < mn; i += DIAG_LANES) buf[i] = g[i];
    __syncthreads();
  }
  for (int c = 0; c < m; ++c) {
    double* y = buf + (int64_t)c * n;
    double s = 0.0;
    for (int64_t i = lane; i < n; i += DIAG_LANES) s += y[i];
    const double mu = wave_sum(s) / (double)n;
    for (int64_t i = lane; i < n; i += DIAG_LANES) y[i] -= mu;
    __syncthreads();
    double* oc = out + ((int64_t)c * n_series + s0 + sidx) * ((int64_t)max_lag + 1);
    double a0 = 0.0;
    for (int64_t tbase = 0; tbase <= max_lag; tbase += DIAG_LANES) {
      const int64_t t = tbase + lane;
      const double a = lag_block(y, 1, n, n, t, tbase);
      if (tbase == 0) a0 = __shfl(a, 0, DIAG_LANES);
      if (t <= max_lag) oc[t] = a / a0;
    }
  }
}

// ---- Rank-normalised diagnostics (Vehtari et al. 2021 as ArviZ implements them; clvmcmc.h) ----
// One workgroup of four wavefronts per series.  y stays where the gather put it (global memory,
// read-only here); the workgroup owns two buffers, T (the time-ordered transformed split chains,
// [2 m][h] contiguous) and P (the sorted pool), in LDS up to CLV_RANK_LDS_ELEMS values per series
// and in global scratch beyond.  P is sorted by a bitonic network whose compare-exchanges all put the
// smaller value at the lower index, so that a count that is no power of two needs no padding
// (the missing tail behaves as +inf and never moves); a value's average rank is (lb + ub + 1) / 2
// from its lower and upper bound in P.  Every transformed series then goes through the estimator
// of diag_kernel: split-chain means by one wavefront per split chain (lane-strided, wave_sum),
// the first 64 lags shared out the same way, then wavefront 0 alone runs geyer_ess (P, free by then,
// holds the means and the lag terms).  Sums over all m n values are lane-strided over the 256
// threads, wave_sum, then the four wavefronts in order.
constexpr int RANK_THREADS = 256;
constexpr int RANK_WAVES = RANK_THREADS / DIAG_LANES;
constexpr int RANK_SC = 32;  // doubles of workgroup scalars in front of T and P
static_assert((2 * CLV_RANK_LDS_ELEMS + RANK_SC) * sizeof(double) <= 64 * 1024, "the LDS path stays within 64 KiB");
enum { SC_RED = 0, SC_HDI_W = 4, SC_HDI_I = 8, SC_PASS = 12 /* rhat, ess, lag */ };

// Sum over the workgroup, the same bits in every thread (red: RANK_WAVES doubles of LDS).
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & (DIAG_LANES - 1)) == 0) red[threadIdx.x / DIAG_LANES] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < RANK_WAVES; ++w) s += red[w];
  return s;
}

// Whether flag is set in any thread of the workgroup (red as in block_sum).
__device__ __forceinline__ bool block_any(int flag, double* red) {
  return block_sum(__any(flag) ? 1.0 : 0.0, red) != 0.0;
}

// Ascending sort of p[0 .. cnt) by the whole workgroup; p is complete and visible on return.
__device__ __forceinline__ void sort_block(double* p, int64_t cnt) {
  __syncthreads();
  int64_t half = 1;  // half the power of two that covers cnt: compare-exchanges per step
  while (2 * half < cnt) half *= 2;
  auto cmpx = [&](int64_t l, int64_t r) {
    if (r < cnt) {
      const double a = p[l], b = p[r];
      if (b < a) {
        p[l] = b;
        p[r] = a;
      }
    }
  };
  for (int64_t k = 2; (k >> 1) < cnt; k <<= 1) {
    const int64_t kh = k >> 1;  // two sorted runs of kh: mirror merge, then half-cleaners
    for (int64_t t = threadIdx.x; t < half; t += RANK_THREADS) {
      const int64_t off = t & (kh - 1), base = (t - off) * 2;
      cmpx(base + off, base + k - 1 - off);
    }
    __syncthreads();
    for (int64_t j = k >> 2; j > 0; j >>= 1) {
      for (int64_t t = threadIdx.x; t < half; t += RANK_THREADS) {
        const int64_t off = t & (j - 1), l = (t - off) * 2 + off;
        cmpx(l, l + j);
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ double median_sorted(const double* p, int64_t cnt) {
  return (cnt & 1) ? p[cnt >> 1] : (p[(cnt >> 1) - 1] + p[cnt >> 1]) / 2.0;
}

// numpy's default (linear) quantile of the sorted p: virtual index q (cnt - 1), _lerp's two forms.
__device__ __forceinline__ double quantile_sorted(const double* p, int64_t cnt, double q) {
  const double vi = q * (double)(cnt - 1);
  const double fl = floor(vi), t = vi - fl;
  const int64_t lo = (int64_t)fl, hi = std::min<int64_t>(lo + 1, cnt - 1);
  const double a = p[lo], b = p[hi], d = b - a;
  return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// Split chain j of the [chain][n] series g.
__device__ __forceinline__ const double* split_chain(const double* g, int j, int64_t n, int64_t h) {
  return g + (int64_t)(j >> 1) * n + (int64_t)(j & 1) * (n - h);
}

// dst[j h + i] = f(split chain j, draw i) over the 2 m split chains.
template <class F>
__device__ __forceinline__ void map_split(const double* g, double* dst, int M, int64_t n, int64_t h, F f) {
  for (int j = 0; j < M; ++j) {
    const double* c = split_chain(g, j, n, h);
    for (int64_t i = threadIdx.x; i < h; i += RANK_THREADS) dst[(int64_t)j * h + i] = f(c[i]);
  }
}

// T[j h + i] = Phi^-1((r - 3/8) / (S + 1/4)), r the average rank of f(y) in the sorted pool P of S
// values; ranks and z also to ranks_out / z_out when given (clv_debug_zscale).
template <class F>
__device__ __forceinline__ void zscale_block(const double* g, const double* P, double* T, int M, int64_t n, int64_t h,
                                             F f, double* ranks_out, double* z_out) {
  const int64_t S = (int64_t)M * h;
  const double den = (double)S + 0.25;
  for (int j = 0; j < M; ++j) {
    const double* c = split_chain(g, j, n, h);
    for (int64_t i = threadIdx.x; i < h; i += RANK_THREADS) {
      const double v = f(c[i]);
      int64_t lo = 0, hi = S;
      while (lo < hi) {  // lower bound: values below v
        const int64_t mid = (lo + hi) >> 1;
        if (P[mid] < v) lo = mid + 1; else hi = mid;
      }
      const int64_t lb = lo;
      hi = S;
      while (lo < hi) {  // upper bound: values not above v
        const int64_t mid = (lo + hi) >> 1;
        if (P[mid] <= v) lo = mid + 1; else hi = mid;
      }
      const double r = (double)(lb + lo + 1) / 2.0;
      const double z = norm_ppf((r - 0.375) / den);
      T[(int64_t)j * h + i] = z;
      if (ranks_out) {
        ranks_out[(int64_t)j * h + i] = r;
        z_out[(int64_t)j * h + i] = z;
      }
    }
  }
}

// The estimator on the transformed split chains in T (centred in place; mus: cap doubles of
// scratch): res[0..2] = R-hat, ESS (when full), truncation lag, NaN when W == 0.  Called by the
// whole workgroup; T may be rewritten on return.  Where the scratch has room (2 m x 65 doubles: 130
// draws per chain) the first 64 lags, which is as far as nearly every series goes, are shared out: a
// wavefront per split chain leaves its lag_chain terms in the scratch and wavefront 0 adds them in
// chain order, lag_block's arithmetic.
__device__ __forceinline__ void split_pass(double* T, double* mus, int64_t cap, int M, int64_t h, bool full,
                                           double* res) {
  const int lane = threadIdx.x & (DIAG_LANES - 1), wave = threadIdx.x / DIAG_LANES;
  __syncthreads();
  for (int j = wave; j < M; j += RANK_WAVES) {
    double* c = T + (int64_t)j * h;
    double a = 0.0;
    for (int64_t i = lane; i < h; i += DIAG_LANES) a += c[i];
    const double mu = wave_sum(a) / (double)h;
    for (int64_t i = lane; i < h; i += DIAG_LANES) c[i] -= mu;
    if (lane == 0) mus[j] = mu;
  }
  __syncthreads();
  const bool shared_out = (int64_t)M * (DIAG_LANES + 1) <= cap;
  double* part = mus + M;
  if (shared_out) {
    for (int j = wave; j < M; j += RANK_WAVES)
      part[(int64_t)j * DIAG_LANES + lane] = lag_chain(T + (int64_t)j * h, h, lane, 0);
    __syncthreads();
  }
  if (wave == 0) {
    double a_first;
    if (shared_out) {
      double asum = 0.0;
      for (int j = 0; j < M; ++j) asum += part[(int64_t)j * DIAG_LANES + lane];
      a_first = asum / (double)M;
    } else {
      a_first = lag_block(T, M, 2 * h, h, lane, 0);
    }
    double musum = 0.0;
    for (int j = 0; j < M; ++j) musum += mus[j];
    const double mubar = musum / (double)M;
    double muss = 0.0;
    for (int j = 0; j < M; ++j) muss += (mus[j] - mubar) * (mus[j] - mubar);
    double W = 0.0, V = 0.0, ess = NAN;
    int64_t lag = 0;
    const bool ok = geyer_ess(T, M, 2 * h, h, muss / (double)(M - 1), lane, full, a_first, W, V, ess, lag);
    if (lane == 0) {
      res[0] = ok ? sqrt(V / W) : NAN;
      res[1] = ok ? ess : NAN;
      res[2] = ok ? (double)lag : NAN;
    }
  }
  __syncthreads();
}

// seg [series][chain][n] as gathered (read only); scratch [series][2 m n] on the global path.
template <bool LDS>
__global__ __launch_bounds__(RANK_THREADS) void rank_kernel(const double* seg, double* scratch, int m, int64_t n,
                                                            int64_t nc, int64_t s0, int64_t hdi_k,
                                                            double* out /*[n_series][CLV_N_RANK_STATS]*/) {
  extern __shared__ double rank_smem[];
  const int64_t sidx = blockIdx.x;
  if (sidx >= nc) return;
  const int tid = threadIdx.x;
  const int M = 2 * m;
  const int64_t N = (int64_t)m * n, h = n / 2, S = (int64_t)M * h;
  const double* g = seg + sidx * N;
  double* sc = rank_smem;
  double* T = LDS ? rank_smem + RANK_SC : scratch + sidx * 2 * N;
  double* P = T + N;
  double* o = out + (s0 + sidx) * CLV_N_RANK_STATS;

  double s = 0.0;
  int bad = 0;
  for (int64_t i = tid; i < N; i += RANK_THREADS) {
    const double v = g[i];
    P[i] = v;
    s += v;
    bad |= !std::isfinite(v);
  }
  if (block_any(bad, sc + SC_RED)) {
    if (tid < CLV_N_RANK_STATS) o[tid] = NAN;
    return;
  }
  const double mean = block_sum(s, sc + SC_RED) / (double)N;

  // all m n values sorted: median, the two tail quantiles, the narrowest interval of hdi_k steps
  sort_block(P, N);
  const double median = median_sorted(P, N);
  const double q05 = quantile_sorted(P, N, 0.05), q95 = quantile_sorted(P, N, 0.95);
  double bw = INFINITY;
  int64_t bi = INT64_MAX;
  for (int64_t i = tid; i < N - hdi_k; i += RANK_THREADS) {
    const double w = P[i + hdi_k] - P[i];
    if (w < bw) {
      bw = w;
      bi = i;
    }
  }
  for (int off = DIAG_LANES / 2; off > 0; off >>= 1) {
    const double ow = __shfl_xor(bw, off, DIAG_LANES);
    const long long oi = __shfl_xor((long long)bi, off, DIAG_LANES);
    if (ow < bw || (ow == bw && oi < bi)) {
      bw = ow;
      bi = oi;
    }
  }
  if ((tid & (DIAG_LANES - 1)) == 0) {
    sc[SC_HDI_W + tid / DIAG_LANES] = bw;
    sc[SC_HDI_I + tid / DIAG_LANES] = (double)bi;  // below 2^44: exact
  }
  __syncthreads();
  bw = sc[SC_HDI_W];
  double bid = sc[SC_HDI_I];
  for (int w = 1; w < RANK_WAVES; ++w)
    if (sc[SC_HDI_W + w] < bw || (sc[SC_HDI_W + w] == bw && sc[SC_HDI_I + w] < bid)) {
      bw = sc[SC_HDI_W + w];
      bid = sc[SC_HDI_I + w];
    }
  bi = bw < INFINITY ? (int64_t)bid : 0;  // (a width that overflowed: the first interval)
  const double hdi_lo = P[bi], hdi_hi = P[bi + hdi_k];

  // the pool of split values: all values unless an odd n drops the middle draws
  auto ident = [](double v) { return v; };
  if (S != N) {
    __syncthreads();
    map_split(g, P, M, n, h, ident);
    sort_block(P, S);
  }
  const double med = median_sorted(P, S);

  // bulk: z-scale of the split values
  zscale_block(g, P, T, M, n, h, ident, nullptr, nullptr);
  split_pass(T, P, N, M, h, true, sc + SC_PASS);
  const double rhat_bulk = sc[SC_PASS], ess_bulk = sc[SC_PASS + 1], lag_bulk = sc[SC_PASS + 2];

  // folded: z-scale of |split value - median of the pool|, R-hat only
  auto fold = [med](double v) { return fabs(v - med); };
  __syncthreads();
  map_split(g, P, M, n, h, fold);
  sort_block(P, S);
  zscale_block(g, P, T, M, n, h, fold, nullptr, nullptr);
  split_pass(T, P, N, M, h, false, sc + SC_PASS);
  const double rhat_folded = sc[SC_PASS];

  // tails: the indicators of y <= q05 and y <= q95
  __syncthreads();
  map_split(g, T, M, n, h, [q05](double v) { return v <= q05 ? 1.0 : 0.0; });
  split_pass(T, P, N, M, h, true, sc + SC_PASS);
  const double ess_q05 = sc[SC_PASS + 1];
  __syncthreads();
  map_split(g, T, M, n, h, [q95](double v) { return v <= q95 ? 1.0 : 0.0; });
  split_pass(T, P, N, M, h, true, sc + SC_PASS);
  const double ess_q95 = sc[SC_PASS + 1];

  // sd: the squared deviations from the mean
  __syncthreads();
  map_split(g, T, M, n, h, [mean](double v) { return (v - mean) * (v - mean); });
  split_pass(T, P, N, M, h, true, sc + SC_PASS);
  const double ess_sd = sc[SC_PASS + 1];
  double e2 = 0.0, e4 = 0.0;
  for (int64_t i = tid; i < N; i += RANK_THREADS) {
    const double d = g[i] - mean, c2 = d * d;
    e2 += c2;
    e4 += c2 * c2;
  }
  const double evar = block_sum(e2, sc + SC_RED) / (double)N;
  const double m4 = block_sum(e4, sc + SC_RED) / (double)N;
  const double varvar = (m4 - evar * evar) / ess_sd;

  if (tid == 0) {
    o[CLV_RANK_RHAT] = (rhat_bulk == rhat_bulk && rhat_folded == rhat_folded) ? fmax(rhat_bulk, rhat_folded) : NAN;
    o[CLV_RANK_RHAT_BULK] = rhat_bulk;
    o[CLV_RANK_RHAT_FOLDED] = rhat_folded;
    o[CLV_RANK_ESS_BULK] = ess_bulk;
    o[CLV_RANK_ESS_TAIL] = (ess_q05 == ess_q05 && ess_q95 == ess_q95) ? fmin(ess_q05, ess_q95) : NAN;
    o[CLV_RANK_ESS_Q05] = ess_q05;
    o[CLV_RANK_ESS_Q95] = ess_q95;
    o[CLV_RANK_ESS_SD] = ess_sd;
    o[CLV_RANK_MCSE_SD] = evar == 0.0 ? NAN : sqrt(varvar / evar / 4.0);
    o[CLV_RANK_HDI_LO] = hdi_lo;
    o[CLV_RANK_HDI_HI] = hdi_hi;
    o[CLV_RANK_MEDIAN] = median;
    o[CLV_RANK_LAG_BULK] = lag_bulk;
  }
}

// clv_debug_zscale: the sort and the rank transform of rank_kernel alone, ranks and z written out.
template <bool LDS>
__global__ __launch_bounds__(RANK_THREADS) void zscale_kernel(const double* seg, double* scratch, int m, int64_t n,
                                                              int64_t nc, int64_t s0, int folded, double* ranks_out,
                                                              double* z_out /*[n_series][2 m][h] each*/) {
  extern __shared__ double rank_smem[];
  const int64_t sidx = blockIdx.x;
  if (sidx >= nc) return;
  const int tid = threadIdx.x;
  const int M = 2 * m;
  const int64_t N = (int64_t)m * n, h = n / 2, S = (int64_t)M * h;
  const double* g = seg + sidx * N;
  double* T = LDS ? rank_smem + RANK_SC : scratch + sidx * 2 * N;
  double* P = T + N;
  double* ro = ranks_out + (s0 + sidx) * S;
  double* zo = z_out + (s0 + sidx) * S;
  int bad = 0;
  for (int64_t i = tid; i < N; i += RANK_THREADS) bad |= !std::isfinite(g[i]);
  if (block_any(bad, rank_smem + SC_RED)) {
    for (int64_t i = tid; i < S; i += RANK_THREADS) ro[i] = zo[i] = NAN;
    return;
  }
  auto ident = [](double v) { return v; };
  map_split(g, P, M, n, h, ident);
  sort_block(P, S);
  if (!folded) {
    zscale_block(g, P, T, M, n, h, ident, ro, zo);
    return;
  }
  const double med = median_sorted(P, S);
  auto fold = [med](double v) { return fabs(v - med); };
  __syncthreads();
  map_split(g, P, M, n, h, fold);
  sort_block(P, S);
  zscale_block(g, P, T, M, n, h, fold, ro, zo);
}

int check_series(int32_t n_chains, int64_t n_draws, int64_t n_series) {
  if (n_chains < 1) return fail(CLV_EINVAL, "n_chains must be >= 1");
  if (n_draws < 8) return fail(CLV_EINVAL, "diagnostics need n_draws >= 8");
  if (n_series < 1) return fail(CLV_EINVAL, "n_series must be >= 1");
  const int64_t cap = int64_t(1) << 44;  // elements: keeps every byte count far inside 64 bits
  if (n_draws > cap / n_chains || n_series > cap / (n_draws * n_chains))
    return fail(CLV_EINVAL, "series array too large");
  return CLV_OK;
}

// Series per batch: as many as DIAG_BATCH_ELEMS values hold (at least one); CLV_DIAG_BATCH (series)
// forces a smaller one — the tests' knob.  The batch loop and the global-path scratch both size
// themselves here.
int64_t batch_series(int64_t mn, int64_t n_series) {
  return lowered_by_env("CLV_DIAG_BATCH", std::max<int64_t>(1, std::min<int64_t>(n_series, DIAG_BATCH_ELEMS / mn)));
}

// Walks the series of d_in (device, [chain * draw][n_series]) in batches of batch_series: each batch
// [s0, s0 + nc) is gathered to seg [series][chain * draw] and handed to launch(seg, s0, nc), which
// launches the batch's kernel on st.
template <class F>
int for_series_batches(const double* d_in, int64_t mn, int64_t n_series, int period, uint32_t log_mask, hipStream_t st,
                       F launch) {
  const int64_t per_batch = batch_series(mn, n_series);
  DevBuf bseg;
  CLV_HIP(hipMalloc(&bseg.p, sizeof(double) * (size_t)(per_batch * mn)));
  for (int64_t s0 = 0; s0 < n_series; s0 += per_batch) {
    const int64_t nc = std::min<int64_t>(per_batch, n_series - s0);
    const int64_t tiles = ((nc + DIAG_TILE - 1) / DIAG_TILE) * ((mn + DIAG_TILE - 1) / DIAG_TILE);
    hipLaunchKernelGGL(diag_gather_kernel, dim3((unsigned)tiles), dim3(256), 0, st, d_in, mn, n_series, s0, nc, period,
                       log_mask, bseg.as<double>());
    CLV_HIP(hipGetLastError());
    launch(bseg.as<double>(), s0, nc);
    CLV_HIP(hipGetLastError());
  }
  return CLV_OK;
}

// d_in: device [chain][draw][n_series]; host_out [n_series][CLV_N_DIAG_STATS].
int diag_dev(const double* d_in, int32_t m, int64_t n, int64_t n_series, int period, uint32_t log_mask,
             double* host_out, hipStream_t st) {
  const int64_t mn = (int64_t)m * n;
  DevBuf bout;
  CLV_HIP(hipMalloc(&bout.p, sizeof(double) * (size_t)n_series * CLV_N_DIAG_STATS));
  const bool lds = mn <= DIAG_LDS_ELEMS;
  int rc = for_series_batches(d_in, mn, n_series, period, log_mask, st, [&](double* seg, int64_t s0, int64_t nc) {
    if (lds)
      hipLaunchKernelGGL(diag_kernel<true>, dim3((unsigned)nc), dim3(DIAG_LANES), sizeof(double) * (size_t)mn, st, seg,
                         (int)m, n, nc, s0, bout.as<double>());
    else
      hipLaunchKernelGGL(diag_kernel<false>, dim3((unsigned)nc), dim3(DIAG_LANES), 0, st, seg, (int)m, n, nc, s0,
                         bout.as<double>());
  });
  if (rc) return rc;
  CLV_HIP(hipMemcpyAsync(host_out, bout.p, sizeof(double) * (size_t)n_series * CLV_N_DIAG_STATS,
                         hipMemcpyDeviceToHost, st));
  CLV_HIP(hipStreamSynchronize(st));
  return CLV_OK;
}

int check_hdi_prob(double hdi_prob) {
  if (!(hdi_prob > 0.0 && hdi_prob < 1.0)) return fail(CLV_EINVAL, "hdi_prob must be in (0, 1)");
  return CLV_OK;
}

size_t rank_lds_bytes(bool lds, int64_t mn) { return sizeof(double) * (size_t)(RANK_SC + (lds ? 2 * mn : 0)); }

// d_in: device [chain][draw][n_series]; host_out [n_series][CLV_N_RANK_STATS].
int rank_dev(const double* d_in, int32_t m, int64_t n, int64_t n_series, int period, uint32_t log_mask,
             double hdi_prob, double* host_out, hipStream_t st) {
  const int64_t mn = (int64_t)m * n;
  const int64_t hdi_k = std::min<int64_t>((int64_t)std::floor(hdi_prob * (double)mn), mn - 1);
  const bool lds = mn <= CLV_RANK_LDS_ELEMS;
  DevBuf bscr, bout;
  if (!lds) CLV_HIP(hipMalloc(&bscr.p, sizeof(double) * (size_t)(2 * batch_series(mn, n_series) * mn)));
  CLV_HIP(hipMalloc(&bout.p, sizeof(double) * (size_t)n_series * CLV_N_RANK_STATS));
  int rc = for_series_batches(d_in, mn, n_series, period, log_mask, st, [&](double* seg, int64_t s0, int64_t nc) {
    if (lds)
      hipLaunchKernelGGL(rank_kernel<true>, dim3((unsigned)nc), dim3(RANK_THREADS), rank_lds_bytes(true, mn), st, seg,
                         (double*)nullptr, (int)m, n, nc, s0, hdi_k, bout.as<double>());
    else
      hipLaunchKernelGGL(rank_kernel<false>, dim3((unsigned)nc), dim3(RANK_THREADS), rank_lds_bytes(false, mn), st,
                         seg, bscr.as<double>(), (int)m, n, nc, s0, hdi_k, bout.as<double>());
  });
  if (rc) return rc;
  CLV_HIP(hipMemcpyAsync(host_out, bout.p, sizeof(double) * (size_t)n_series * CLV_N_RANK_STATS,
                         hipMemcpyDeviceToHost, st));
  CLV_HIP(hipStreamSynchronize(st));
  return CLV_OK;
}

// The body of the two *_sampler entry points: dev(d_in, n_series, period, log_mask, host_out) is
// diag_dev or rank_dev over the sampler's chains and draws.
template <class F>
int sampler_series(clv_sampler* s, uint32_t log_mask, double* level1_out, double* level2_out, F dev) {
  const Geometry& g = s->g;
  int rc;
  if (level1_out) {
    const double* l1;
    int64_t nd;
    int32_t w;
    if ((rc = sampler_l1(s, &l1, &nd, &w)) || (rc = check_series(g.n_chains, g.n_draws, g.n * w)) ||
        (rc = dev(l1, g.n * w, w, log_mask, level1_out)))
      return rc;
  }
  if (level2_out) {
    const double* l2;
    if ((rc = sampler_l2(s, &l2, "the run has not stored all of its draws yet")) ||
        (rc = check_series(g.n_chains, g.n_draws, g.l2w)) || (rc = dev(l2, g.l2w, 1, 0u, level2_out)))
      return rc;
  }
  return CLV_OK;
}

}  // namespace

extern "C" {

int clv_rank_diagnostics(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                         int32_t period, uint32_t log_mask, double hdi_prob, double* out) {
  if (!series || !out) return fail(CLV_EINVAL, "null argument");
  int rc = check_series(n_chains, n_draws, n_series);
  if (rc) return rc;
  if (period < 1 || period > 32) return fail(CLV_EINVAL, "period must be in 1..32");
  rc = check_hdi_prob(hdi_prob);
  if (rc) return rc;
  DeviceScope ds(device);
  DevBuf bin;
  if ((rc = upload(bin, series, (size_t)n_chains * n_draws * n_series, nullptr))) return rc;
  return rank_dev(bin.as<double>(), n_chains, n_draws, n_series, period, log_mask, hdi_prob, out, nullptr);
}

int clv_rank_diagnostics_sampler(clv_sampler* s, uint32_t log_mask, double hdi_prob, double* level1_out,
                                 double* level2_out) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (!level1_out && !level2_out) return fail(CLV_EINVAL, "null argument (no output asked for)");
  int rc = check_hdi_prob(hdi_prob);
  if (rc) return rc;
  return sampler_series(s, log_mask, level1_out, level2_out,
                        [&](const double* d_in, int64_t n_series, int period, uint32_t mask, double* out) {
                          return rank_dev(d_in, s->g.n_chains, s->g.n_draws, n_series, period, mask, hdi_prob, out,
                                          s->stream);
                        });
}

int clv_debug_zscale(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                     int32_t folded, double* ranks_out, double* z_out) {
  if (!series || !ranks_out || !z_out) return fail(CLV_EINVAL, "null argument");
  int rc = check_series(n_chains, n_draws, n_series);
  if (rc) return rc;
  DeviceScope ds(device);
  DevBuf bin, bscr, br, bz;
  if ((rc = upload(bin, series, (size_t)n_chains * n_draws * n_series, nullptr))) return rc;
  const int64_t mn = (int64_t)n_chains * n_draws, S = 2 * (int64_t)n_chains * (n_draws / 2);
  const bool lds = mn <= CLV_RANK_LDS_ELEMS;
  if (!lds) CLV_HIP(hipMalloc(&bscr.p, sizeof(double) * (size_t)(2 * batch_series(mn, n_series) * mn)));
  CLV_HIP(hipMalloc(&br.p, sizeof(double) * (size_t)(n_series * S)));
  CLV_HIP(hipMalloc(&bz.p, sizeof(double) * (size_t)(n_series * S)));
  rc = for_series_batches(bin.as<double>(), mn, n_series, 1, 0u, nullptr, [&](double* seg, int64_t s0, int64_t nc) {
    if (lds)
      hipLaunchKernelGGL(zscale_kernel<true>, dim3((unsigned)nc), dim3(RANK_THREADS), rank_lds_bytes(true, mn),
                         nullptr, seg, (double*)nullptr, (int)n_chains, n_draws, nc, s0, (int)folded, br.as<double>(),
                         bz.as<double>());
    else
      hipLaunchKernelGGL(zscale_kernel<false>, dim3((unsigned)nc), dim3(RANK_THREADS), rank_lds_bytes(false, mn),
                         nullptr, seg, bscr.as<double>(), (int)n_chains, n_draws, nc, s0, (int)folded, br.as<double>(),
                         bz.as<double>());
  });
  if (rc) return rc;
  CLV_HIP(hipMemcpy(ranks_out, br.p, sizeof(double) * (size_t)(n_series * S), hipMemcpyDeviceToHost));
  CLV_HIP(hipMemcpy(z_out, bz.p, sizeof(double) * (size_t)(n_series * S), hipMemcpyDeviceToHost));
  return CLV_OK;
}

int clv_diagnostics(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                    int32_t period, uint32_t log_mask, double* out) {
  if (!series || !out) return fail(CLV_EINVAL, "null argument");
  int rc = check_series(n_chains, n_draws, n_series);
  if (rc) return rc;
  if (period < 1 || period > 32) return fail(CLV_EINVAL, "period must be in 1..32");
  DeviceScope ds(device);
  DevBuf bin;
  if ((rc = upload(bin, series, (size_t)n_chains * n_draws * n_series, nullptr))) return rc;
  return diag_dev(bin.as<double>(), n_chains, n_draws, n_series, period, log_mask, out, nullptr);
}

int clv_diagnostics_sampler(clv_sampler* s, uint32_t log_mask, double* level1_out, double* level2_out) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (!level1_out && !level2_out) return fail(CLV_EINVAL, "null argument (no output asked for)");
  return sampler_series(s, log_mask, level1_out, level2_out,
                        [&](const double* d_in, int64_t n_series, int period, uint32_t mask, double* out) {
                          return diag_dev(d_in, s->g.n_chains, s->g.n_draws, n_series, period, mask, out, s->stream);
                        });
}

int clv_autocorr(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                 int32_t max_lag, double* out) {
  if (!series || !out) return fail(CLV_EINVAL, "null argument");
  int rc = check_series(n_chains, n_draws, n_series);
  if (rc) return rc;
  if (max_lag < 0 || max_lag > n_draws - 1) return fail(CLV_EINVAL, "max_lag must be in 0..n_draws-1");
  DeviceScope ds(device);
  DevBuf bin, bout;
  if ((rc = upload(bin, series, (size_t)n_chains * n_draws * n_series, nullptr))) return rc;
  const int64_t mn = (int64_t)n_chains * n_draws;
  const size_t n_out = (size_t)n_chains * n_series * ((size_t)max_lag + 1);
  CLV_HIP(hipMalloc(&bout.p, sizeof(double) * n_out));
  const bool lds = mn <= DIAG_LDS_ELEMS;
  rc = for_series_batches(bin.as<double>(), mn, n_series, 1, 0u, nullptr, [&](double* seg, int64_t s0, int64_t nc) {
    if (lds)
      hipLaunchKernelGGL(acf_kernel<true>, dim3((unsigned)nc), dim3(DIAG_LANES), sizeof(double) * (size_t)mn, nullptr,
                         seg, (int)n_chains, n_draws, nc, s0, n_series, (int)max_lag, bout.as<double>());
    else
      hipLaunchKernelGGL(acf_kernel<false>, dim3((unsigned)nc), dim3(DIAG_LANES), 0, nullptr, seg, (int)n_chains,
                         n_draws, nc, s0, n_series, (int)max_lag, bout.as<double>());
  });
  if (rc) return rc;
  CLV_HIP(hipMemcpy(out, bout.p, sizeof(double) * n_out, hipMemcpyDeviceToHost));
  return CLV_OK;
}

}  // extern "C"
