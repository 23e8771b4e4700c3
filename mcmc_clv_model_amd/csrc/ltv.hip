// Posterior customer lifetime value and customer equity on device (Abe 2015; DESIGN.md section 4f;
// float64 model: tests/ltv_ref.py).
//
//   clv_lifetime_value / _sampler   per customer the posterior of the discounted expected value
//                                   (mean, sd, 2.5 / 50 / 97.5 percentiles), of the value left after
//                                   T_cal, P(alive), expected lifetime and one-year survival; per
//                                   draw the customer equity and its companions
//   clv_ltv_info                    the limits of this file, for the tests
//
// Per draw d and customer i, from the level-1 row (lambda, mu, tau, z[, eta]), a = mu + delta:
//   value    = (lambda m) / a                          infinite horizon
//            = ((lambda m) (-expm1(-(a H)))) / a       horizon H
//   residual = z value
// with m = eta value_scale (width 5) or monetary[i] (width 4, 1 without it).
//
// One pass over the level-1 array (ltv_pass_kernel): a 256-lane workgroup owns the 256-customer
// block b (customers 256 b ...) and walks the draws in order, LTV_TILE at a time; lane l of
// wavefront w owns customer 4 l + w of the block.  With that assignment the levels 128 ... 4 of the
// 256-tree (offsets that are multiples of 4) stay inside a wavefront and only the last two cross
// wavefronts: per tile a wavefront lays a quantity out in LDS as [customer][draw], 16 of its lanes
// take one draw's 64 values each and add them in registers in the tree's order (lane offsets
// 32 ... 1), and 64 lanes finish (w0 + w2) + (w1 + w3) into the block partial of each draw.  The
// same LDS rows go out transposed to [customer][draw] for the sort, 16 lanes storing the 128 bytes
// of one customer's tile.  The rows of the next tile are loaded before the LDS work of this one, so
// their latency is covered; the per-customer sums are added in draw order by the owning lane.
// ltv_final_kernel adds the block partials in the order of pnbd.hip (lane t takes partials t,
// t + 256, ... in turn, then the same tree), so a per-draw sum does not depend on the launch
// geometry or on the customer batch.  The series are sorted exactly (rocprim segmented radix sort,
// customers in batches of at most LTV_BATCH_KEYS keys, whole 256-customer blocks); ltv_sd_kernel
// forms the sd from the unsorted series (numpy's std: deviations from the mean, squares, sum in
// draw order; one lane per series, the rows staged through LDS LTV_SD_TILE draws at a time) and
// percentile_kernel numpy's 'linear' percentiles from the sorted one.  No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "analysis_host.h"

using namespace clv;

namespace {

constexpr int LTV_BLOCK = 256;                            // customers per workgroup = reduction block
constexpr int LTV_TILE = 16;                              // draws per LDS tile of the pass
constexpr int LTV_ROW = LTV_TILE + 1;                     // its padded row (bank-conflict-free both ways)
constexpr int LTV_SD_TILE = 32;                           // draws per LDS tile of the sd kernel
constexpr int64_t LTV_BATCH_KEYS = int64_t(1) << 27;      // keys per sort call (1 GiB of doubles)
constexpr int64_t LTV_MAX_DRAWS = int64_t(1) << 22;       // 256 customers x draws stay below 2^31 keys
constexpr int LTV_MAX_GRID = 1 << 16;

struct LtvArgs {
  const double* level1;    // [n_draws][n][width]
  const double* monetary;  // [n] or null
  int64_t n_draws, n;
  int width;
  double delta, horizon, value_scale, ppy;
  int finite;              // horizon is finite
};

// The rows of draws [d0, d0 + LTV_TILE) of customer i; a draw past the end or a customer past n
// reads nothing and counts as lambda 0, mu 1, z 0.
struct LtvRows {
  double lam[LTV_TILE], mu[LTV_TILE], z[LTV_TILE], eta[LTV_TILE];
};

__device__ __forceinline__ void ltv_load(const LtvArgs& A, int64_t i, bool live, int64_t d0, LtvRows& r) {
#pragma unroll
  for (int k = 0; k < LTV_TILE; ++k) {
    r.lam[k] = 0.0, r.mu[k] = 1.0, r.z[k] = 0.0, r.eta[k] = 0.0;
    if (live && d0 + k < A.n_draws) {
      const double* row = A.level1 + ((d0 + k) * A.n + i) * A.width;
      r.lam[k] = row[0];
      r.mu[k] = row[1];
      r.z[k] = row[3];
      if (A.width > 4) r.eta[k] = row[4];
    }
  }
}

// A wavefront's LDS rows buf[lane's customer][draw] <- x.  The caller synchronises afterwards.
__device__ __forceinline__ void ltv_put(double* buf, int l, const double* x) {
#pragma unroll
  for (int k = 0; k < LTV_TILE; ++k) buf[l * LTV_ROW + k] = x[k];
}

// Lane k < LTV_TILE: draw k's 64 values of this wavefront added in the 256-tree's order (its levels
// 128 ... 4 are the lane offsets 32 ... 1 here) -> wp[k].
__device__ __forceinline__ void ltv_reduce(const double* buf, int l, double* wp) {
  if (l < LTV_TILE) {
    double a[32];
#pragma unroll
    for (int m = 0; m < 32; ++m) a[m] = buf[m * LTV_ROW + l] + buf[(m + 32) * LTV_ROW + l];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1)
#pragma unroll
      for (int m = 0; m < off; ++m) a[m] += a[m + off];
    wp[l] = a[0];
  }
}

// The wavefront's rows to seg[(customer of the batch)][draw]: 16 consecutive lanes store the 16
// draws of one customer (128 bytes).
__device__ __forceinline__ void ltv_store_transposed(const double* buf, int l, int w, int64_t d0, int nd, int64_t c0,
                                                     int64_t i0, int64_t n, int64_t n_draws, double* seg) {
  const int dd = l & (LTV_TILE - 1);
  if (dd < nd)
    for (int m = l / LTV_TILE; m < 64; m += 64 / LTV_TILE) {
      const int64_t i = c0 + 4 * m + w;
      if (i < n) seg[(i - i0) * n_draws + d0 + dd] = buf[m * LTV_ROW + dd];
    }
}

// Customers [i0, i0 + nc), i0 a multiple of 256: one workgroup per 256-customer block.
__global__ __launch_bounds__(LTV_BLOCK) void ltv_pass_kernel(LtvArgs A, int64_t i0, int64_t nc, int64_t nb,
                                                             double* seg_value, double* seg_resid,
                                                             double* part /*[4][n_draws][nb]*/,
                                                             double* out /*[n][CLV_N_LTV_STATS]*/) {
  __shared__ double lds[4][64 * LTV_ROW];
  __shared__ double wpart[CLV_N_LTV_DRAW_STATS][4][LTV_TILE];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  double* buf = lds[w];
  const int64_t nblk = (nc + LTV_BLOCK - 1) / LTV_BLOCK;
  for (int64_t bl = blockIdx.x; bl < nblk; bl += gridDim.x) {
    const int64_t c0 = i0 + bl * LTV_BLOCK, b = c0 / LTV_BLOCK;
    const int64_t i = c0 + 4 * l + w;
    const bool live = i < A.n;
    const double mon = (live && A.monetary) ? A.monetary[i] : 1.0;
    double sum_value = 0.0, sum_resid = 0.0, sum_z = 0.0, sum_life = 0.0, sum_surv = 0.0;
    LtvRows cur, next;
    ltv_load(A, i, live, 0, cur);
    for (int64_t d0 = 0; d0 < A.n_draws; d0 += LTV_TILE) {
      const int nd = (int)std::min<int64_t>(LTV_TILE, A.n_draws - d0);
      double value[LTV_TILE], resid[LTV_TILE], share[LTV_TILE];
#pragma unroll
      for (int k = 0; k < LTV_TILE; ++k) {
        const double a = cur.mu[k] + A.delta;
        const double m = A.width > 4 ? cur.eta[k] * A.value_scale : mon;
        double v = cur.lam[k] * m;
        if (A.finite) v = v * (-expm1(-(a * A.horizon)));
        v = v / a;
        const bool use = live && k < nd;
        value[k] = use ? v : 0.0;  // zero padding of the block and of the last tile
        resid[k] = use ? cur.z[k] * v : 0.0;
        share[k] = use ? cur.mu[k] / a : 0.0;
        if (use) {
          const double pm = A.ppy * cur.mu[k];
          sum_value += v;
          sum_resid += resid[k];
          sum_z += cur.z[k];
          sum_life += 1.0 / pm;
          sum_surv += exp(-pm);
        }
      }
      ltv_load(A, i, live, d0 + LTV_TILE, next);  // in flight during the LDS work below
      ltv_put(buf, l, value);
      __syncthreads();
      ltv_store_transposed(buf, l, w, d0, nd, c0, i0, A.n, A.n_draws, seg_value);
      ltv_reduce(buf, l, wpart[CLV_LTV_DRAW_VALUE_TOTAL][w]);
      __syncthreads();
      ltv_put(buf, l, resid);
      __syncthreads();
      ltv_store_transposed(buf, l, w, d0, nd, c0, i0, A.n, A.n_draws, seg_resid);
      ltv_reduce(buf, l, wpart[CLV_LTV_DRAW_EQUITY][w]);
      __syncthreads();
      ltv_put(buf, l, cur.z);
      __syncthreads();
      ltv_reduce(buf, l, wpart[CLV_LTV_DRAW_N_ALIVE][w]);
      __syncthreads();
      ltv_put(buf, l, share);
      __syncthreads();
      ltv_reduce(buf, l, wpart[CLV_LTV_DRAW_MU_SHARE][w]);
      __syncthreads();
      // the tree's last two levels, across the wavefronts; wpart is next written after a barrier
      if ((int)threadIdx.x < CLV_N_LTV_DRAW_STATS * LTV_TILE) {
        const int q = threadIdx.x / LTV_TILE, k = threadIdx.x & (LTV_TILE - 1);
        if (k < nd)
          part[((int64_t)q * A.n_draws + d0 + k) * nb + b] =
              (wpart[q][0][k] + wpart[q][2][k]) + (wpart[q][1][k] + wpart[q][3][k]);
      }
      cur = next;
    }
    if (live) {
      const double S = (double)A.n_draws;
      double* o = out + i * CLV_N_LTV_STATS;
      o[CLV_LTV_VALUE_MEAN] = sum_value / S;
      o[CLV_LTV_RESIDUAL_MEAN] = sum_resid / S;
      o[CLV_LTV_P_ALIVE] = sum_z / S;
      o[CLV_LTV_LIFETIME_YRS] = sum_life / S;
      o[CLV_LTV_SURVIVAL_1YR] = sum_surv / S;
    }
    __syncthreads();
  }
}

// out_draws[d][q] = fixed-order sum over the nb block partials (mu_share: divided by n); grid
// (n_draws, 4).
__global__ __launch_bounds__(LTV_BLOCK) void ltv_final_kernel(const double* part, int64_t n_draws, int64_t nb,
                                                              int64_t n, double* out_draws) {
  __shared__ double red[LTV_BLOCK];
  const int q = blockIdx.y;
  for (int64_t d = blockIdx.x; d < n_draws; d += gridDim.x) {
    const double* p = part + ((int64_t)q * n_draws + d) * nb;
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += LTV_BLOCK) acc += p[b];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = LTV_BLOCK / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) out_draws[d * CLV_N_LTV_DRAW_STATS + q] = q == CLV_LTV_DRAW_MU_SHARE ? red[0] / (double)n : red[0];
    __syncthreads();
  }
}

// sd (numpy's std, ddof 1) of the value series (blockIdx.y 0) and the residual series (1) of the
// batch from the series in draw order and the mean already in out: one lane per series, one
// wavefront per 64 customers.  A lane's series is a row of seg, so the 64 rows are read LTV_SD_TILE
// draws at a time through LDS (32 lanes load the 256 bytes of one customer's tile, lane c then takes
// its row in order); the next tile is loaded while this one is added.
__global__ __launch_bounds__(64) void ltv_sd_kernel(const double* seg_value, const double* seg_resid, int64_t nc,
                                                    int64_t n_draws, int64_t i0, double* out) {
  __shared__ double tile[64][LTV_SD_TILE + 1];
  const double* seg = blockIdx.y ? seg_resid : seg_value;
  const int col0 = blockIdx.y ? CLV_LTV_RESIDUAL_MEAN : CLV_LTV_VALUE_MEAN;
  const int l = threadIdx.x;
  const int64_t cw = (int64_t)blockIdx.x * 64, c = cw + l;
  const bool live = c < nc;
  double* o = out + (i0 + (live ? c : 0)) * CLV_N_LTV_STATS + col0;
  const double mean = live ? o[0] : 0.0;
  const int dd = l & (LTV_SD_TILE - 1), cq = l / LTV_SD_TILE;
  constexpr int NR = LTV_SD_TILE * 64 / 64;  // loads per lane and tile
  double cur[NR], next[NR];
  auto load = [&](int64_t d0, double* x) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t cc = cw + r * (64 / LTV_SD_TILE) + cq;
      x[r] = (cc < nc && d0 + dd < n_draws) ? seg[cc * n_draws + d0 + dd] : 0.0;
    }
  };
  load(0, cur);
  double acc = 0.0;
  for (int64_t d0 = 0; d0 < n_draws; d0 += LTV_SD_TILE) {
    const int nd = (int)std::min<int64_t>(LTV_SD_TILE, n_draws - d0);
#pragma unroll
    for (int r = 0; r < NR; ++r) tile[r * (64 / LTV_SD_TILE) + cq][dd] = cur[r];
    load(d0 + LTV_SD_TILE, next);
    __syncthreads();
    if (live)
      for (int k = 0; k < nd; ++k) {
        const double dev = tile[l][k] - mean;
        acc += dev * dev;
      }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; ++r) cur[r] = next[r];
  }
  if (live) o[1] = sqrt(acc / (double)(n_draws - 1));  // 0 / 0 = NaN at one draw, as numpy
}

// Customers per batch: whole 256-customer blocks within LTV_BATCH_KEYS keys (at least one block);
// CLV_LTV_BATCH (customers, rounded up to whole blocks) forces a smaller one — the tests' knob.
int64_t batch_customers(int64_t n_draws) {
  int64_t per = std::max<int64_t>(1, LTV_BATCH_KEYS / n_draws / LTV_BLOCK) * LTV_BLOCK;
  if (const char* e = std::getenv("CLV_LTV_BATCH")) {
    const long long v = std::atoll(e);
    if (v > 0) per = std::min<int64_t>(per, (v + LTV_BLOCK - 1) / LTV_BLOCK * LTV_BLOCK);
  }
  return per;
}

int check_args(int64_t n_draws, int64_t n, int32_t width, bool has_monetary, double delta, double horizon,
               double value_scale, double ppy) {
  if (n_draws < 1 || n < 1 || (width != 4 && width != 5)) return fail(CLV_EINVAL, "bad level-1 shape");
  if (n_draws > LTV_MAX_DRAWS || n > 0x7fffffffLL)
    return fail(CLV_EINVAL, "bad level-1 shape: more than 2^22 stacked draws or 2^31 - 1 customers");
  if (!std::isfinite(delta) || delta < 0.0) return fail(CLV_EINVAL, "delta must be finite and >= 0");
  if (std::isnan(horizon) || horizon <= 0.0) return fail(CLV_EINVAL, "horizon must be > 0 (infinity allowed)");
  if (!std::isfinite(value_scale)) return fail(CLV_EINVAL, "value_scale must be finite");
  if (!std::isfinite(ppy)) return fail(CLV_EINVAL, "periods_per_year must be finite");
  if (has_monetary && width == 5) return fail(CLV_EINVAL, "monetary is for width 4: width 5 takes the value from eta");
  return CLV_OK;
}

// l1 and monetary on the device; out_customers / out_draws on the host.
int ltv_dev(const double* l1, int64_t n_draws, int64_t n, int32_t width, const double* d_monetary, double delta,
            double horizon, double value_scale, double ppy, double* out_customers, double* out_draws,
            hipStream_t st) {
  LtvArgs A;
  A.level1 = l1;
  A.monetary = d_monetary;
  A.n_draws = n_draws;
  A.n = n;
  A.width = width;
  A.delta = delta;
  A.finite = std::isfinite(horizon) ? 1 : 0;
  A.horizon = A.finite ? horizon : 0.0;
  A.value_scale = value_scale;
  A.ppy = ppy;
  const int64_t nb = (n + LTV_BLOCK - 1) / LTV_BLOCK;
  const int64_t per_batch = std::min<int64_t>(batch_customers(n_draws), nb * LTV_BLOCK);
  const size_t keys = (size_t)std::min<int64_t>(per_batch, n) * n_draws;
  DevBuf bo, bd, bpart, bval, bres;
  CLV_HIP(hipMalloc(&bo.p, sizeof(double) * n * CLV_N_LTV_STATS));
  CLV_HIP(hipMalloc(&bd.p, sizeof(double) * n_draws * CLV_N_LTV_DRAW_STATS));
  CLV_HIP(hipMalloc(&bpart.p, sizeof(double) * CLV_N_LTV_DRAW_STATS * n_draws * nb));
  CLV_HIP(hipMalloc(&bval.p, sizeof(double) * keys));
  CLV_HIP(hipMalloc(&bres.p, sizeof(double) * keys));
  SegSorter<double> sorter;
  int rc = sorter.init(std::min<int64_t>(per_batch, n), n_draws, st);
  if (rc) return rc;
  double* dout = (double*)bo.p;
  for (int64_t i0 = 0; i0 < n; i0 += per_batch) {
    const int64_t nc = std::min<int64_t>(per_batch, n - i0);
    const int64_t nblk = (nc + LTV_BLOCK - 1) / LTV_BLOCK;
    hipLaunchKernelGGL(ltv_pass_kernel, dim3((unsigned)std::min<int64_t>(nblk, LTV_MAX_GRID)), dim3(LTV_BLOCK), 0, st,
                       A, i0, nc, nb, (double*)bval.p, (double*)bres.p, (double*)bpart.p, dout);
    CLV_HIP(hipGetLastError());
    hipLaunchKernelGGL(ltv_sd_kernel, dim3((unsigned)((nc + 63) / 64), 2), dim3(64), 0, st, (const double*)bval.p,
                       (const double*)bres.p, nc, n_draws, i0, dout);
    CLV_HIP(hipGetLastError());
    const double* series[2] = {(const double*)bval.p, (const double*)bres.p};
    const int col0[2] = {CLV_LTV_VALUE_MEAN, CLV_LTV_RESIDUAL_MEAN};
    for (int q = 0; q < 2; ++q) {  // the 2.5 / 50 / 97.5 percentiles: columns col0 + 2 .. + 4
      const PctCols pc{3, {2.5, 50.0, 97.5}, {col0[q] + 2, col0[q] + 3, col0[q] + 4}};
      const double* sorted;
      if ((rc = sorter.sort(series[q], nc, &sorted))) return rc;
      if ((rc = launch_percentiles(sorted, nc, n_draws, pc, i0, CLV_N_LTV_STATS, dout, st))) return rc;
    }
  }
  hipLaunchKernelGGL(ltv_final_kernel, dim3((unsigned)std::min<int64_t>(n_draws, LTV_MAX_GRID), CLV_N_LTV_DRAW_STATS),
                     dim3(LTV_BLOCK), 0, st, (const double*)bpart.p, n_draws, nb, n, (double*)bd.p);
  CLV_HIP(hipGetLastError());
  CLV_HIP(hipMemcpyAsync(out_customers, dout, sizeof(double) * n * CLV_N_LTV_STATS, hipMemcpyDeviceToHost, st));
  CLV_HIP(hipMemcpyAsync(out_draws, bd.p, sizeof(double) * n_draws * CLV_N_LTV_DRAW_STATS, hipMemcpyDeviceToHost, st));
  CLV_HIP(hipStreamSynchronize(st));
  return CLV_OK;
}

}  // namespace

extern "C" {

int clv_ltv_info(int64_t* out) {
  if (!out) return fail(CLV_EINVAL, "null argument");
  out[0] = LTV_BLOCK;
  out[1] = LTV_TILE;
  out[2] = LTV_BATCH_KEYS;
  out[3] = LTV_MAX_DRAWS;
  out[4] = LTV_SD_TILE;
  return CLV_OK;
}

int clv_lifetime_value(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                       const double* monetary, double delta, double horizon, double value_scale,
                       double periods_per_year, double* out_customers, double* out_draws) {
  int rc = check_args(n_draws, n, width, monetary != nullptr, delta, horizon, value_scale, periods_per_year);
  if (rc) return rc;
  if (!level1 || !out_customers || !out_draws) return fail(CLV_EINVAL, "null argument");
  DeviceScope ds(device);
  DevBuf b1, bm;
  if ((rc = upload(b1, level1, (size_t)n_draws * n * width, nullptr)) || (rc = upload(bm, monetary, n, nullptr))) return rc;
  return ltv_dev((const double*)b1.p, n_draws, n, width, (const double*)bm.p, delta, horizon, value_scale,
                 periods_per_year, out_customers, out_draws, nullptr);
}

int clv_lifetime_value_sampler(clv_sampler* s, const double* monetary, double delta, double horizon,
                               double value_scale, double periods_per_year, double* out_customers,
                               double* out_draws) {
  const double* l1;
  int64_t nd;
  int32_t w;
  int rc = sampler_l1(s, &l1, &nd, &w);
  if (rc) return rc;
  rc = check_args(nd, s->g.n, w, monetary != nullptr, delta, horizon, value_scale, periods_per_year);
  if (rc) return rc;
  if (!out_customers || !out_draws) return fail(CLV_EINVAL, "null argument");
  DevBuf bm;
  if ((rc = upload(bm, monetary, s->g.n, s->stream))) return rc;
  return ltv_dev(l1, nd, s->g.n, w, (const double*)bm.p, delta, horizon, value_scale, periods_per_year,
                 out_customers, out_draws, s->stream);
}

}  // extern "C"
