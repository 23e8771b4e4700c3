// Posterior predictive checks of the calibration data on device (float64
// model: tests/ppc_ref.py).
//
//   clv_ppc / _sampler   one replicate (x_rep, t_x_rep) of every customer's calibration data per
//                        stacked draw, at the customer level (the customer's own (lambda, mu)) or at
//                        the population level (a new (lambda, mu) ~ LogNormal(beta' d_i, Sigma) per
//                        level-2 record); per customer the statistics over the draws, per draw the
//                        statistics over the customers
//   clv_ppc_info         the limits of this file and what the last call launched, for the tests
//   clv_debug_ppc        the same with the customer batch and the grid overridden
//
// The replicate of customer i under flat draw d (Philox key = the seed, counter (customer_offset + i,
// d, slot, 5), include/clvmcmc.h):
//   level 1 only: (n0, n1) = Box-Muller (cos, sin) of slot 1; lambda = exp(m0 + l00 n0),
//                 mu = exp(m1 + l10 n0 + l11 n1), m = X_i beta, l = chol(Sigma[0:2, 0:2])
//   slot 0:  E = -log(u53_open0(x, y)), U = u53_open0(z, w); tau = E / mu; alive = tau > T;
//            L = alive ? T : tau
//   x_rep = poisson_draw(lambda L) from slots 16 + attempt;  t_x_rep = x_rep > 0 ? L exp(log(U) / x_rep) : 0
//
// Shape.  ppc_rep_kernel: a 256-lane workgroup takes a work item = (256-customer block, chunk of
// PPC_CHUNK consecutive draws), lane t the block's customer t, and walks the chunk's draws in order.
// A (block, all draws) workgroup — the lane owning every draw of its customer — would leave c2
// (93 blocks) on 93 of 256 CUs (measured 4 x slower: DESIGN.md section 4j; CLV_PPC_ITEM_DRAWS makes a
// work item span several chunks, for that measurement); the chunks give 125 times as many
// workgroups and nothing is lost, because every statistic but one is an integer and integers add
// exactly in any order:
//   per customer  the lane counts its chunk in registers and adds the counts to the customer's
//                 64-bit counters with one global atomic each per chunk;
//   per draw      the histogram's bins below PPC_LBINS go through an LDS histogram of the chunk
//                 (32-bit LDS atomics) that is flushed with one global atomic per non-empty bin,
//                 higher bins straight to global memory; SUM_X, SUM_X2, MAX_X are reduced over the
//                 wavefront by shuffles, N_ALIVE by a ballot, then over the workgroup in LDS and
//                 flushed the same way.
// The one floating-point statistic, t_x_rep, is stored as tmp[draw][customer of the batch] and summed
// by two kernels without atomics: ppc_cust_kernel adds a customer's column in draw order (one lane
// per customer, coalesced); ppc_block_sum_kernel adds a draw's zero-padded 256-customer block by the
// 256-tree (one wavefront per (draw, block): levels 128 and 64 in registers, 32 ... 1 by shuffles)
// and ppc_final_kernel the block partials by the scheme of ltv.hip — so SUM_TX depends neither on the
// grid nor on the batch.  Customers are taken in batches of whole blocks so that tmp stays within
// PPC_BATCH_DOUBLES doubles.  No workgroup waits for another; every loop is bounded by the chunk, the
// draws or POISSON_MAX_ITER.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "analysis_host.h"
#include "philox.h"
#include "poisson.h"

using namespace clv;

namespace {

constexpr int PPC_BLOCK = 256;                          // customers per workgroup = reduction block
constexpr int PPC_MAX_K = 4096;                         // the largest k_hist
constexpr int PPC_CHUNK = 32;                           // draws per work item
constexpr int PPC_LBINS = 64;                           // histogram bins kept in LDS per draw of the chunk
constexpr int64_t PPC_BATCH_DOUBLES = int64_t(1) << 27; // t_x_rep doubles per customer batch (1 GiB)
constexpr int64_t PPC_MAX_DRAWS = 0x7fffffffLL;
constexpr int PPC_MAX_GRID = 1 << 16;
constexpr int PPC_N_CUST_INTS = 6;                      // SUM_X, N_LT, N_EQ, N_ZERO, N_TX_LE, N_ALIVE
constexpr uint32_t STREAM_PPC = 5u;
constexpr uint32_t SLOT_LIFE = 0u, SLOT_NORMAL = 1u, SLOT_POISSON0 = 16u;

typedef unsigned long long u64;

// What the last clv_ppc* call of this thread launched (clv_ppc_info).
thread_local int64_t last_info[3] = {-1, -1, -1};  // VGPRs, scratch bytes, kernel ns

struct PpcArgs {
  const double* level1;  // level 0: [n_draws][n][width]
  const double* level2;  // level 1: [n_draws][l2w]
  const double* cov;     // level 1: [K - 1][n] or null
  const int32_t* x;
  const double *tx, *T;
  int64_t n_draws, n, offset;
  int width, D, K, k_hist;
  uint32_t k0, k1;
};

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (u64)__shfl_xor((long long)v, off, 64);
  return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = (u64)__shfl_xor((long long)v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// Customers [i0, i0 + nc) of the batch, i0 a multiple of 256; tmp [n_draws][stride]; cint
// [PPC_N_CUST_INTS][stride] (zeroed by the host); dint [n_draws][k_hist + 1 + CLV_N_PPC_DRAW_INTS]
// (zeroed by the host before the first batch).  A work item is a block and item_chunks consecutive
// chunks of PPC_CHUNK draws (1 by default; more: the profile's knob).
template <int LEVEL>
__global__ __launch_bounds__(PPC_BLOCK) void ppc_rep_kernel(PpcArgs A, int64_t i0, int64_t nc, int64_t stride,
                                                            int64_t item_chunks, double* tmp, u64* cint, u64* dint,
                                                            int64_t* xrep, double* txrep) {
  __shared__ unsigned int hist[PPC_CHUNK * PPC_LBINS];
  __shared__ u64 ist[PPC_CHUNK][3];
  __shared__ unsigned int nal[PPC_CHUNK];
  const int t = threadIdx.x, l = t & 63;
  const int64_t nblk = (nc + PPC_BLOCK - 1) / PPC_BLOCK;
  const int64_t nch = (A.n_draws + PPC_CHUNK - 1) / PPC_CHUNK;
  const int64_t items = nblk * ((nch + item_chunks - 1) / item_chunks);
  const int K = A.K, kh = A.k_hist;
  const int64_t W = (int64_t)kh + 1 + CLV_N_PPC_DRAW_INTS;
  const int l2w = A.D * K + A.D * (A.D + 1) / 2, s11_at = A.D == 2 ? 2 : 3;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t ig = it / nblk, bl = it - ig * nblk;
    const int64_t c = bl * PPC_BLOCK + t;
    const bool live = c < nc;
    const int64_t i = i0 + (live ? c : 0);
    const int64_t xi = A.x[i];
    const double txi = A.tx[i], Ti = A.T[i];
    const uint32_t ca = (uint32_t)(A.offset + i);
    double xr[CLV_MAX_K - 1];
    if (LEVEL == 1) {
#pragma unroll
      for (int k = 0; k < CLV_MAX_K - 1; ++k) xr[k] = k < K - 1 ? A.cov[(int64_t)k * A.n + i] : 0.0;
    }
    u64 c_sum = 0, c_lt = 0, c_eq = 0, c_zero = 0, c_le = 0, c_alive = 0;
    const int64_t ch_end = min(nch, (ig + 1) * item_chunks);
    for (int64_t ch = ig * item_chunks; ch < ch_end; ++ch) {
      const int64_t d0 = ch * PPC_CHUNK;
      const int nd = (int)min((int64_t)PPC_CHUNK, A.n_draws - d0);
      for (int q = t; q < PPC_CHUNK * PPC_LBINS; q += PPC_BLOCK) hist[q] = 0u;
      if (t < PPC_CHUNK) {
        ist[t][0] = ist[t][1] = ist[t][2] = 0ull;
        nal[t] = 0u;
      }
      __syncthreads();
      for (int k = 0; k < nd; ++k) {
        const int64_t d = d0 + k;
        int64_t xq = 0;
        double tq = 0.0;
        bool alive = false;
        if (live) {
          double lam, mu;
          if (LEVEL == 0) {
            const double* row = A.level1 + (d * A.n + i) * A.width;
            lam = row[0];
            mu = row[1];
          } else {
            const double* rec = A.level2 + d * l2w;
            double m0 = rec[0], m1 = rec[K];
#pragma unroll
            for (int j = 0; j < CLV_MAX_K - 1; ++j)
              if (j < K - 1) {
                m0 = m0 + xr[j] * rec[j + 1];
                m1 = m1 + xr[j] * rec[K + j + 1];
              }
            const double* sg = rec + A.D * K;
            const double l00 = sqrt(sg[0]);
            const double l10 = sg[1] / l00;
            const double l11 = sqrt(sg[s11_at] - l10 * l10);
            const u32x4 rn = pblock(A.k0, A.k1, ca, (uint32_t)d, SLOT_NORMAL, STREAM_PPC);
            const double rad = sqrt(-2.0 * log(u53_open0(rn.x, rn.y)));
            const double ang = 2.0 * u53(rn.z, rn.w);
            const double n0 = rad * cospi(ang), n1 = rad * sinpi(ang);
            lam = exp(m0 + l00 * n0);
            mu = exp(m1 + l10 * n0 + l11 * n1);
          }
          const u32x4 r = pblock(A.k0, A.k1, ca, (uint32_t)d, SLOT_LIFE, STREAM_PPC);
          const double E = -log(u53_open0(r.x, r.y));
          const double U = u53_open0(r.z, r.w);
          const double tau = E / mu;
          alive = tau > Ti;
          const double L = alive ? Ti : tau;
          xq = poisson_draw(lam * L, A.k0, A.k1, ca, (uint32_t)d, SLOT_POISSON0, STREAM_PPC);
          if (xq > 0) tq = L * exp(log(U) / (double)xq);
          c_sum += (u64)xq;
          c_lt += xq < xi;
          c_eq += xq == xi;
          c_zero += xq == 0;
          c_le += tq <= txi;
          c_alive += alive;
          if (xrep) xrep[d * A.n + i] = xq;
          if (txrep) txrep[d * A.n + i] = tq;
          const int64_t bin = xq < kh ? xq : (int64_t)kh;  // the last bin: x_rep >= k_hist
          if (bin < PPC_LBINS)
            atomicAdd(&hist[k * PPC_LBINS + (int)bin], 1u);
          else
            atomicAdd(&dint[d * W + bin], 1ull);
        }
        tmp[d * stride + c] = tq;  // 0 for the padding of the last block
        const u64 sx = wave_sum((u64)xq), sx2 = wave_sum((u64)xq * (u64)xq), mx = wave_max((u64)xq);
        const unsigned na = (unsigned)__popcll(__ballot(alive));
        if (l == 0) {
          if (sx) {
            atomicAdd(&ist[k][0], sx);
            atomicAdd(&ist[k][1], sx2);
            atomicMax(&ist[k][2], mx);
          }
          if (na) atomicAdd(&nal[k], na);
        }
      }
      __syncthreads();
      for (int q = t; q < nd * PPC_LBINS; q += PPC_BLOCK) {
        const unsigned v = hist[q];
        const int k = q / PPC_LBINS, b = q - k * PPC_LBINS;
        if (v) atomicAdd(&dint[(d0 + k) * W + b], (u64)v);
      }
      if (t < nd) {
        u64* o = dint + (d0 + t) * W + kh + 1;
        if (ist[t][0]) {
          atomicAdd(&o[CLV_PPC_DRAW_SUM_X], ist[t][0]);
          atomicAdd(&o[CLV_PPC_DRAW_SUM_X2], ist[t][1]);
          atomicMax(&o[CLV_PPC_DRAW_MAX_X], ist[t][2]);
        }
        if (nal[t]) atomicAdd(&o[CLV_PPC_DRAW_N_ALIVE], (u64)nal[t]);
      }
      __syncthreads();  // the LDS counters are cleared for the next chunk
    }
    if (live) {
      atomicAdd(&cint[0 * stride + c], c_sum);
      atomicAdd(&cint[1 * stride + c], c_lt);
      atomicAdd(&cint[2 * stride + c], c_eq);
      atomicAdd(&cint[3 * stride + c], c_zero);
      atomicAdd(&cint[4 * stride + c], c_le);
      atomicAdd(&cint[5 * stride + c], c_alive);
    }
  }
}

// The customer rows of the batch: counts / S and the sequential sum of t_x_rep in draw order / S.
__global__ __launch_bounds__(PPC_BLOCK) void ppc_cust_kernel(int64_t n_draws, int64_t i0, int64_t nc, int64_t stride,
                                                             const double* tmp, const u64* cint,
                                                             double* out /*[n][CLV_N_PPC_STATS]*/) {
  const int64_t c = (int64_t)blockIdx.x * PPC_BLOCK + threadIdx.x;
  if (c >= nc) return;
  double s = 0.0;
  for (int64_t d = 0; d < n_draws; ++d) s = s + tmp[d * stride + c];
  const double S = (double)n_draws;
  double* o = out + (i0 + c) * CLV_N_PPC_STATS;
  o[CLV_PPC_X_REP_MEAN] = (double)(int64_t)cint[0 * stride + c] / S;
  o[CLV_PPC_P_X_LT] = (double)cint[1 * stride + c] / S;
  o[CLV_PPC_P_X_EQ] = (double)cint[2 * stride + c] / S;
  o[CLV_PPC_P_ZERO] = (double)cint[3 * stride + c] / S;
  o[CLV_PPC_TX_REP_MEAN] = s / S;
  o[CLV_PPC_P_TX_LE] = (double)cint[4 * stride + c] / S;
  o[CLV_PPC_P_ALIVE_REP] = (double)cint[5 * stride + c] / S;
}

// part[d][b0 + bl] = the 256-tree over block bl of the batch's t_x_rep of draw d: one wavefront per
// (draw, block).  s[e] += s[e + off] for off = 128 ... 1: the first two levels in registers, the rest
// by shuffles (lane e takes lane e + off's value; lanes e >= off hold values nobody reads).
__global__ __launch_bounds__(PPC_BLOCK) void ppc_block_sum_kernel(int64_t n_draws, int64_t b0, int64_t nblk, int64_t nb,
                                                                  int64_t stride, const double* tmp, double* part) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int64_t total = n_draws * nblk;
  for (int64_t wi = (int64_t)blockIdx.x * 4 + w; wi < total; wi += (int64_t)gridDim.x * 4) {
    const int64_t d = wi / nblk, bl = wi - d * nblk;
    const double* p = tmp + d * stride + bl * PPC_BLOCK;
    double a = (p[l] + p[l + 128]) + (p[l + 64] + p[l + 192]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a = a + __shfl_down(a, off, 64);
    if (l == 0) part[d * nb + b0 + bl] = a;
  }
}

// out_f[d] = the fixed-order sum of the nb block partials (ltv.hip's ltv_final_kernel: lane t takes
// partials t, t + 256, ... in turn, then the 256-tree).
__global__ __launch_bounds__(PPC_BLOCK) void ppc_final_kernel(const double* part, int64_t n_draws, int64_t nb,
                                                              double* out_f) {
  __shared__ double red[PPC_BLOCK];
  for (int64_t d = blockIdx.x; d < n_draws; d += gridDim.x) {
    const double* p = part + d * nb;
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += PPC_BLOCK) acc += p[b];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = PPC_BLOCK / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) out_f[d * CLV_N_PPC_DRAW_FLOATS + CLV_PPC_DRAW_SUM_TX] = red[0];
    __syncthreads();
  }
}

struct PpcOut {
  double* customers;
  int64_t* draws_int;
  double* draws_f;
  int64_t* x_rep;
  double* tx_rep;
};

// What needs no data, before any device call.
int check_args(int32_t level, int32_t width, int32_t D, int32_t K, bool has_cov, int64_t n_draws, int64_t n,
               int32_t k_hist, int64_t customer_offset) {
  if (level != 0 && level != 1) return fail(CLV_EINVAL, "level must be 0 (customer) or 1 (population)");
  if (n_draws < 1 || n < 1) return fail(CLV_EINVAL, "bad shape: no draw or no customer");
  if (n_draws > PPC_MAX_DRAWS || n > 0x7fffffffLL)
    return fail(CLV_EINVAL, "bad shape: more than 2^31 - 1 stacked draws or customers");
  if (level == 0 && width != 4 && width != 5) return fail(CLV_EINVAL, "bad level-1 width");
  if (level == 1) {
    if (D != 2 && D != 3) return fail(CLV_EINVAL, "D must be 2 or 3");
    if (K < 1 || K > CLV_MAX_K) return fail(CLV_EINVAL, "K must be 1 .. 9");
    if ((K > 1) != has_cov) return fail(CLV_EINVAL, "covariates do not match K (K - 1 rows of n, none for K = 1)");
  }
  if (k_hist < 1 || k_hist > PPC_MAX_K) return fail(CLV_EINVAL, "k_hist must be in [1, 4096]");
  if (customer_offset < 0 || customer_offset > (int64_t)0xFFFFFFFFLL || n > (int64_t)0x100000000LL - customer_offset)
    return fail(CLV_EINVAL, "customer_offset + n must fit in 32 bits");
  return CLV_OK;
}

// Every pointer of A on the device; the outputs on the host.  batch_customers / grid 0: the defaults.
int ppc_dev(PpcArgs A, int32_t level, uint64_t seed, int64_t batch_customers, int32_t grid, const PpcOut& o,
            hipStream_t st) {
  const int64_t n = A.n, nd = A.n_draws;
  const int64_t W = (int64_t)A.k_hist + 1 + CLV_N_PPC_DRAW_INTS;
  const int64_t nb = (n + PPC_BLOCK - 1) / PPC_BLOCK;
  const int64_t want = batch_customers > 0 ? (batch_customers + PPC_BLOCK - 1) / PPC_BLOCK
                                           : std::max<int64_t>(1, PPC_BATCH_DOUBLES / nd / PPC_BLOCK);
  const int64_t per_batch = std::min(want, nb) * PPC_BLOCK;
  const int64_t max_grid = grid > 0 ? grid : PPC_MAX_GRID;
  A.k0 = (uint32_t)seed;
  A.k1 = (uint32_t)(seed >> 32);
  DevBuf btmp, bcint, bdint, bpart, bf, bo, bx, btx;
  CLV_HIP(hipMalloc(&btmp.p, sizeof(double) * (size_t)per_batch * nd));
  CLV_HIP(hipMalloc(&bcint.p, sizeof(u64) * (size_t)per_batch * PPC_N_CUST_INTS));
  CLV_HIP(hipMalloc(&bdint.p, sizeof(u64) * (size_t)nd * W));
  CLV_HIP(hipMalloc(&bpart.p, sizeof(double) * (size_t)nd * nb));
  CLV_HIP(hipMalloc(&bf.p, sizeof(double) * (size_t)nd * CLV_N_PPC_DRAW_FLOATS));
  CLV_HIP(hipMalloc(&bo.p, sizeof(double) * (size_t)n * CLV_N_PPC_STATS));
  if (o.x_rep) CLV_HIP(hipMalloc(&bx.p, sizeof(int64_t) * (size_t)nd * n));
  if (o.tx_rep) CLV_HIP(hipMalloc(&btx.p, sizeof(double) * (size_t)nd * n));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  CLV_HIP(hipEventCreate(&e0));
  hipError_t err = hipEventCreate(&e1);
  if (err == hipSuccess) err = hipMemsetAsync(bdint.p, 0, sizeof(u64) * (size_t)nd * W, st);
  if (err == hipSuccess) err = hipEventRecord(e0, st);
  const int64_t nch = (nd + PPC_CHUNK - 1) / PPC_CHUNK;
  int64_t item_chunks = 1;  // CLV_PPC_ITEM_DRAWS: draws per work item, in whole chunks (the profile's knob)
  if (const char* e = std::getenv("CLV_PPC_ITEM_DRAWS")) {
    const long long v = std::atoll(e);
    if (v > 0) item_chunks = std::min<int64_t>(nch, ((int64_t)v + PPC_CHUNK - 1) / PPC_CHUNK);
  }
  const int64_t nit = (nch + item_chunks - 1) / item_chunks;
  for (int64_t i0 = 0; i0 < n && err == hipSuccess; i0 += per_batch) {
    const int64_t nc = std::min<int64_t>(per_batch, n - i0);
    const int64_t nblk = (nc + PPC_BLOCK - 1) / PPC_BLOCK;
    err = hipMemsetAsync(bcint.p, 0, sizeof(u64) * (size_t)per_batch * PPC_N_CUST_INTS, st);
    if (err != hipSuccess) break;
    const dim3 g((unsigned)std::min<int64_t>(nblk * nit, max_grid));
    if (level == 0)
      hipLaunchKernelGGL(ppc_rep_kernel<0>, g, dim3(PPC_BLOCK), 0, st, A, i0, nc, per_batch, item_chunks,
                         btmp.as<double>(),
                         bcint.as<u64>(), bdint.as<u64>(), bx.as<int64_t>(), btx.as<double>());
    else
      hipLaunchKernelGGL(ppc_rep_kernel<1>, g, dim3(PPC_BLOCK), 0, st, A, i0, nc, per_batch, item_chunks,
                         btmp.as<double>(),
                         bcint.as<u64>(), bdint.as<u64>(), bx.as<int64_t>(), btx.as<double>());
    hipLaunchKernelGGL(ppc_cust_kernel, dim3((unsigned)nblk), dim3(PPC_BLOCK), 0, st, nd, i0, nc, per_batch,
                       btmp.as<double>(), bcint.as<u64>(), bo.as<double>());
    hipLaunchKernelGGL(ppc_block_sum_kernel, dim3((unsigned)std::min<int64_t>((nd * nblk + 3) / 4, max_grid)),
                       dim3(PPC_BLOCK), 0, st, nd, i0 / PPC_BLOCK, nblk, nb, per_batch, btmp.as<double>(),
                       bpart.as<double>());
    err = hipGetLastError();
  }
  if (err == hipSuccess) {
    hipLaunchKernelGGL(ppc_final_kernel, dim3((unsigned)std::min<int64_t>(nd, max_grid)), dim3(PPC_BLOCK), 0, st,
                       bpart.as<double>(), nd, nb, bf.as<double>());
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipEventRecord(e1, st);
  auto d2h = [&](void* dst, const void* src, size_t bytes) {  // an optional output: dst null
    if (err == hipSuccess && dst) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  };
  d2h(o.customers, bo.p, sizeof(double) * (size_t)n * CLV_N_PPC_STATS);
  d2h(o.draws_int, bdint.p, sizeof(u64) * (size_t)nd * W);
  d2h(o.draws_f, bf.p, sizeof(double) * (size_t)nd * CLV_N_PPC_DRAW_FLOATS);
  d2h(o.x_rep, bx.p, sizeof(int64_t) * (size_t)nd * n);
  d2h(o.tx_rep, btx.p, sizeof(double) * (size_t)nd * n);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  float ms = 0.0f;
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (err != hipSuccess) return fail(CLV_EHIP, std::string("ppc: ") + hipGetErrorString(err));
  hipFuncAttributes fa{};
  CLV_HIP(hipFuncGetAttributes(&fa, level == 0 ? reinterpret_cast<const void*>(ppc_rep_kernel<0>)
                                               : reinterpret_cast<const void*>(ppc_rep_kernel<1>)));
  last_info[0] = fa.numRegs;
  last_info[1] = (int64_t)fa.localSizeBytes;
  last_info[2] = (int64_t)std::llround((double)ms * 1e6);
  return CLV_OK;
}

int ppc_host(int32_t device, int32_t level, const double* level1, int32_t width, const double* level2, int32_t D,
             int32_t K, const double* cov, int64_t n_draws, int64_t n, const int32_t* x, const double* t_x,
             const double* T_cal, int32_t k_hist, uint64_t seed, int64_t customer_offset, int64_t batch_customers,
             int32_t grid, const PpcOut& o) {
  int rc = check_args(level, width, D, K, cov != nullptr, n_draws, n, k_hist, customer_offset);
  if (rc) return rc;
  if (!x || !t_x || !T_cal || !o.customers || !o.draws_int || !o.draws_f || (level == 0 ? !level1 : !level2))
    return fail(CLV_EINVAL, "null argument");
  if (batch_customers < 0 || grid < 0) return fail(CLV_EINVAL, "batch_customers and grid must be >= 0");
  DeviceScope ds(device);
  PpcArgs A{};
  A.n_draws = n_draws;
  A.n = n;
  A.offset = customer_offset;
  A.width = width;
  A.D = level == 1 ? D : 2;
  A.K = level == 1 ? K : 1;
  A.k_hist = k_hist;
  DevBuf b1, b2, bc, bx, btx, bT;
  if (level == 0) {
    if ((rc = upload(b1, level1, (size_t)n_draws * n * width, nullptr))) return rc;
  } else {
    if ((rc = upload(b2, level2, (size_t)n_draws * (D * K + D * (D + 1) / 2), nullptr)) ||
        (rc = upload(bc, cov, (size_t)(K - 1) * n, nullptr)))
      return rc;
  }
  if ((rc = upload(bx, x, (size_t)n, nullptr)) || (rc = upload(btx, t_x, (size_t)n, nullptr)) ||
      (rc = upload(bT, T_cal, (size_t)n, nullptr)))
    return rc;
  A.level1 = b1.as<double>();
  A.level2 = b2.as<double>();
  A.cov = bc.as<double>();
  A.x = bx.as<int32_t>();
  A.tx = btx.as<double>();
  A.T = bT.as<double>();
  return ppc_dev(A, level, seed, batch_customers, grid, o, nullptr);
}

}  // namespace

extern "C" {

int clv_ppc_info(int64_t* out) {
  if (!out) return fail(CLV_EINVAL, "null argument");
  out[0] = PPC_BLOCK;
  out[1] = PPC_MAX_K;
  out[2] = PPC_BATCH_DOUBLES;
  out[3] = last_info[0];
  out[4] = last_info[1];
  out[5] = last_info[2];
  return CLV_OK;
}

int clv_ppc(int32_t device, int32_t level, const double* level1, int32_t width, const double* level2, int32_t D,
            int32_t K, const double* cov, int64_t n_draws, int64_t n, const int32_t* x, const double* t_x,
            const double* T_cal, int32_t k_hist, uint64_t seed, int64_t customer_offset, double* out_customers,
            int64_t* out_draws_int, double* out_draws_f, int64_t* out_x_rep, double* out_tx_rep) {
  return ppc_host(device, level, level1, width, level2, D, K, cov, n_draws, n, x, t_x, T_cal, k_hist, seed,
                  customer_offset, 0, 0, PpcOut{out_customers, out_draws_int, out_draws_f, out_x_rep, out_tx_rep});
}

int clv_debug_ppc(int32_t device, int32_t level, const double* level1, int32_t width, const double* level2, int32_t D,
                  int32_t K, const double* cov, int64_t n_draws, int64_t n, const int32_t* x, const double* t_x,
                  const double* T_cal, int32_t k_hist, uint64_t seed, int64_t customer_offset, double* out_customers,
                  int64_t* out_draws_int, double* out_draws_f, int64_t* out_x_rep, double* out_tx_rep,
                  int64_t batch_customers, int32_t grid) {
  return ppc_host(device, level, level1, width, level2, D, K, cov, n_draws, n, x, t_x, T_cal, k_hist, seed,
                  customer_offset, batch_customers, grid,
                  PpcOut{out_customers, out_draws_int, out_draws_f, out_x_rep, out_tx_rep});
}

int clv_ppc_sampler(clv_sampler* s, int32_t level, int32_t k_hist, uint64_t seed, double* out_customers,
                    int64_t* out_draws_int, double* out_draws_f, int64_t* out_x_rep, double* out_tx_rep) {
  if (!s || !out_customers || !out_draws_int || !out_draws_f) return fail(CLV_EINVAL, "null argument");
  const Geometry& g = s->g;
  // what needs no draws, before any device call
  int rc = check_args(level, 4, g.D, g.K, g.K > 1, 1, 1, k_hist, 0);
  if (rc) return rc;
  PpcArgs A{};
  A.n = g.n;
  A.offset = g.shard_begin;
  A.D = 2;
  A.K = 1;
  A.k_hist = k_hist;
  if (level == 0) {
    int32_t w;
    if ((rc = sampler_l1(s, &A.level1, &A.n_draws, &w))) return rc;
    A.width = w;
  } else {
    if ((rc = sampler_l2(s, &A.level2, "the run has not stored all of its level-2 records yet"))) return rc;
    A.n_draws = (int64_t)g.n_chains * g.n_draws;
    A.D = g.D;
    A.K = g.K;
    A.cov = s->d_cov;
  }
  rc = check_args(level, A.width, g.D, g.K, g.K > 1, A.n_draws, g.n, k_hist, g.shard_begin);
  if (rc) return rc;
  A.x = s->d_x;
  A.tx = s->d_tx;
  A.T = s->d_T;
  return ppc_dev(A, level, seed, 0, 0, PpcOut{out_customers, out_draws_int, out_draws_f, out_x_rep, out_tx_rep},
                 s->stream);
}

}  // extern "C"
