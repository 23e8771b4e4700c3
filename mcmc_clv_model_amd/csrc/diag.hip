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

#include "internal.h"

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

// Mean over the nseg segments of the biased autocovariance at this lane's lag t (tbase = lane 0's):
// (1/nseg) sum_j (1/h) sum_{i < h - t} c_j[i] c_j[i + t].  Segment j begins at (j / 2) n + (j % 2)
// (n - h): the split chains of [chain][n] draws, or (nseg 1, h == n) one whole chain.  Lanes with
// t >= h return 0.
__device__ __forceinline__ double lag_block(const double* buf, int nseg, int64_t n, int64_t h, int64_t t,
                                            int64_t tbase) {
  const int64_t full = std::max<int64_t>(0, h - tbase - (DIAG_LANES - 1));  // i + t < h in every lane
  const int64_t any = std::max<int64_t>(0, h - tbase);                      // i + t < h in lane 0
  double asum = 0.0;
  for (int j = 0; j < nseg; ++j) {
    const double* c = buf + (int64_t)(j >> 1) * n + (int64_t)(j & 1) * (n - h);
    double acc = 0.0;
#pragma unroll 4
    for (int64_t i = 0; i < full; ++i) acc += c[i] * c[i + t];
    for (int64_t i = full; i < any; ++i)
      if (i + t < h) acc += c[i] * c[i + t];
    asum += acc / (double)h;
  }
  return asum / (double)nseg;
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

  int64_t tbase = 0;
  double a = lag_block(buf, M, n, h, lane, 0);
  const double a0 = __shfl(a, 0, DIAG_LANES);
  const double W = a0 * (double)h / (double)(h - 1);
  const double V = a0 + varmu;
  if (W == 0.0) {
    if (lane < CLV_N_DIAG_STATS) o[lane] = NAN;
    return;
  }
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
  const int64_t T = t - 2;
  double r_last = stored ? even : 0.0;  // r[T+1]
  if (even > 0.0) r_last = even;
  double tau = -1.0 + 2.0 * S + r_last;
  const double Mh = (double)M * (double)h;
  tau = fmax(tau, 1.0 / log10(Mh));
  const double ess = Mh / tau;
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

int check_series(int32_t n_chains, int64_t n_draws, int64_t n_series) {
  if (n_chains < 1) return fail(CLV_EINVAL, "n_chains must be >= 1");
  if (n_draws < 8) return fail(CLV_EINVAL, "diagnostics need n_draws >= 8");
  if (n_series < 1) return fail(CLV_EINVAL, "n_series must be >= 1");
  const int64_t cap = int64_t(1) << 44;  // elements: keeps every byte count far inside 64 bits
  if (n_draws > cap / n_chains || n_series > cap / (n_draws * n_chains))
    return fail(CLV_EINVAL, "series array too large");
  return CLV_OK;
}

int64_t batch_series(int64_t mn, int64_t n_series) {
  return std::max<int64_t>(1, std::min<int64_t>(n_series, DIAG_BATCH_ELEMS / mn));
}

void launch_gather(const double* d_in, int64_t mn, int64_t n_series, int64_t s0, int64_t nc, int period,
                   uint32_t log_mask, double* seg, hipStream_t st) {
  const int64_t tiles = ((nc + DIAG_TILE - 1) / DIAG_TILE) * ((mn + DIAG_TILE - 1) / DIAG_TILE);
  hipLaunchKernelGGL(diag_gather_kernel, dim3((unsigned)tiles), dim3(256), 0, st, d_in, mn, n_series, s0, nc, period,
                     log_mask, seg);
}

// d_in: device [chain][draw][n_series]; host_out [n_series][CLV_N_DIAG_STATS].
int diag_dev(const double* d_in, int32_t m, int64_t n, int64_t n_series, int period, uint32_t log_mask,
             double* host_out, hipStream_t st) {
  const int64_t mn = (int64_t)m * n;
  const int64_t per_batch = batch_series(mn, n_series);
  DevBuf bseg, bout;
  CLV_HIP(hipMalloc(&bseg.p, sizeof(double) * (size_t)(per_batch * mn)));
  CLV_HIP(hipMalloc(&bout.p, sizeof(double) * (size_t)n_series * CLV_N_DIAG_STATS));
  const bool lds = mn <= DIAG_LDS_ELEMS;
  for (int64_t s0 = 0; s0 < n_series; s0 += per_batch) {
    const int64_t nc = std::min<int64_t>(per_batch, n_series - s0);
    launch_gather(d_in, mn, n_series, s0, nc, period, log_mask, bseg.as<double>(), st);
    CLV_HIP(hipGetLastError());
    if (lds)
      hipLaunchKernelGGL(diag_kernel<true>, dim3((unsigned)nc), dim3(DIAG_LANES), sizeof(double) * (size_t)mn, st,
                         bseg.as<double>(), (int)m, n, nc, s0, bout.as<double>());
    else
      hipLaunchKernelGGL(diag_kernel<false>, dim3((unsigned)nc), dim3(DIAG_LANES), 0, st, bseg.as<double>(), (int)m,
                         n, nc, s0, bout.as<double>());
    CLV_HIP(hipGetLastError());
  }
  CLV_HIP(hipMemcpyAsync(host_out, bout.p, sizeof(double) * (size_t)n_series * CLV_N_DIAG_STATS,
                         hipMemcpyDeviceToHost, st));
  CLV_HIP(hipStreamSynchronize(st));
  return CLV_OK;
}

int upload(const double* host, size_t count, DevBuf& buf) {
  CLV_HIP(hipMalloc(&buf.p, sizeof(double) * count));
  CLV_HIP(hipMemcpy(buf.p, host, sizeof(double) * count, hipMemcpyHostToDevice));
  return CLV_OK;
}

}  // namespace

extern "C" {

int clv_diagnostics(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                    int32_t period, uint32_t log_mask, double* out) {
  if (!series || !out) return fail(CLV_EINVAL, "null argument");
  int rc = check_series(n_chains, n_draws, n_series);
  if (rc) return rc;
  if (period < 1 || period > 32) return fail(CLV_EINVAL, "period must be in 1..32");
  DeviceScope ds(device);
  DevBuf bin;
  rc = upload(series, (size_t)n_chains * n_draws * n_series, bin);
  if (rc) return rc;
  return diag_dev(bin.as<double>(), n_chains, n_draws, n_series, period, log_mask, out, nullptr);
}

int clv_diagnostics_sampler(clv_sampler* s, uint32_t log_mask, double* level1_out, double* level2_out) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (!level1_out && !level2_out) return fail(CLV_EINVAL, "null argument (no output asked for)");
  const Geometry& g = s->g;
  if (level1_out) {
    const double* l1;
    int64_t nd;
    int32_t w;
    int rc = sampler_l1(s, &l1, &nd, &w);
    if (rc) return rc;
    rc = check_series(g.n_chains, g.n_draws, g.n * w);
    if (rc) return rc;
    rc = diag_dev(l1, g.n_chains, g.n_draws, g.n * w, w, log_mask, level1_out, s->stream);
    if (rc) return rc;
  }
  if (level2_out) {
    int64_t stored = 0;
    if (s->sweeps_done > g.burnin) stored = (s->sweeps_done - 1 - g.burnin) / g.thin + 1;
    if (!s->d_level2 || std::min<int64_t>(stored, g.n_draws) < (int64_t)g.n_draws)
      return fail(CLV_ESTATE, "the run has not stored all of its draws yet");
    int rc = check_series(g.n_chains, g.n_draws, g.l2w);
    if (rc) return rc;
    CLV_HIP(hipSetDevice(s->device));
    CLV_HIP(hipStreamSynchronize(s->stream));
    rc = persist_flush(s);  // the last level-2 record may still be pending
    if (rc) return rc;
    rc = diag_dev(s->d_level2, g.n_chains, g.n_draws, g.l2w, 1, 0u, level2_out, s->stream);
    if (rc) return rc;
  }
  return CLV_OK;
}

int clv_autocorr(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                 int32_t max_lag, double* out) {
  if (!series || !out) return fail(CLV_EINVAL, "null argument");
  int rc = check_series(n_chains, n_draws, n_series);
  if (rc) return rc;
  if (max_lag < 0 || max_lag > n_draws - 1) return fail(CLV_EINVAL, "max_lag must be in 0..n_draws-1");
  DeviceScope ds(device);
  DevBuf bin, bseg, bout;
  rc = upload(series, (size_t)n_chains * n_draws * n_series, bin);
  if (rc) return rc;
  const int64_t mn = (int64_t)n_chains * n_draws;
  const int64_t per_batch = batch_series(mn, n_series);
  const size_t n_out = (size_t)n_chains * n_series * ((size_t)max_lag + 1);
  CLV_HIP(hipMalloc(&bseg.p, sizeof(double) * (size_t)(per_batch * mn)));
  CLV_HIP(hipMalloc(&bout.p, sizeof(double) * n_out));
  const bool lds = mn <= DIAG_LDS_ELEMS;
  for (int64_t s0 = 0; s0 < n_series; s0 += per_batch) {
    const int64_t nc = std::min<int64_t>(per_batch, n_series - s0);
    launch_gather(bin.as<double>(), mn, n_series, s0, nc, 1, 0u, bseg.as<double>(), nullptr);
    CLV_HIP(hipGetLastError());
    if (lds)
      hipLaunchKernelGGL(acf_kernel<true>, dim3((unsigned)nc), dim3(DIAG_LANES), sizeof(double) * (size_t)mn, nullptr,
                         bseg.as<double>(), (int)n_chains, n_draws, nc, s0, n_series, (int)max_lag, bout.as<double>());
    else
      hipLaunchKernelGGL(acf_kernel<false>, dim3((unsigned)nc), dim3(DIAG_LANES), 0, nullptr, bseg.as<double>(),
                         (int)n_chains, n_draws, nc, s0, n_series, (int)max_lag, bout.as<double>());
    CLV_HIP(hipGetLastError());
  }
  CLV_HIP(hipMemcpy(out, bout.p, sizeof(double) * n_out, hipMemcpyDeviceToHost));
  return CLV_OK;
}

}  // extern "C"
