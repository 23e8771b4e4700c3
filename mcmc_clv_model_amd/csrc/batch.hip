// Many small fits in one launch: host side of clv_batch_fit / clv_batch_plan /
// clv_batch_info.  The kernel lives in kernels.hip (batch_fit_kernel) beside the per-customer and
// level-2 device functions it shares with the sweep.  Replaces a host loop of whole
// mcmc_draw_parameters calls (bi:346-431 / tri:465-574 once per fit) by one upload, one launch and
// one read-back; no handle outlives the call.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "internal.h"

using namespace clv;

namespace {

constexpr int PRIOR_DOUBLES = 81 + 81 + 27 + 9;  // V, cholV, A0B0, S0B (as clv_create's d_prior)
constexpr int MAX_TILES = 512;                   // one block per unit up to here (clv_default_blocks_per_unit)

// Segment offsets (customers before fit j), tiles per fit and the workgroup map: (fit, chain) pairs,
// the fits with the most tiles first (a stable sort: equal fits in call order, a fit's chains together).
void batch_plan(int64_t n_fits, const int64_t* n, int32_t n_chains, int64_t* seg, int32_t* tiles, int32_t* wg_map) {
  seg[0] = 0;
  for (int64_t j = 0; j < n_fits; ++j) {
    seg[j + 1] = seg[j] + n[j];
    tiles[j] = (int32_t)((n[j] + BLOCK - 1) / BLOCK);
  }
  std::vector<int64_t> order((size_t)n_fits);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t p, int64_t q) { return tiles[p] > tiles[q]; });
  int64_t w = 0;
  for (int64_t j : order)
    for (int32_t c = 0; c < n_chains; ++c, ++w) {
      wg_map[2 * w] = (int32_t)j;
      wg_map[2 * w + 1] = c;
    }
}

int plan_check(int64_t n_fits, const int64_t* n, int32_t n_chains) {
  if (n_fits < 1 || n_fits > (int64_t)0x7fffffff || !n) return fail(CLV_EINVAL, "n_fits must be >= 1");
  if (n_chains < 1) return fail(CLV_EINVAL, "n_chains must be >= 1");
  if (n_fits * (int64_t)n_chains > (int64_t)0x7fffffff) return fail(CLV_EINVAL, "n_fits * n_chains must fit in 31 bits");
  for (int64_t j = 0; j < n_fits; ++j) {
    if (n[j] < 1) return fail(CLV_EINVAL, "fit " + std::to_string(j) + ": n must be >= 1");
    if (n[j] > (int64_t)MAX_TILES * BLOCK)
      return fail(CLV_EINVAL, "fit " + std::to_string(j) + ": more than " + std::to_string(MAX_TILES) +
                                  " tiles of " + std::to_string(BLOCK) + " customers; fit it on its own");
  }
  return CLV_OK;
}

}  // namespace

extern "C" {

int clv_batch_plan(int64_t n_fits, const int64_t* n, int32_t n_chains, int64_t* seg_offsets, int32_t* tiles,
                   int32_t* wg_map) {
  if (!seg_offsets || !tiles || !wg_map) return fail(CLV_EINVAL, "null argument");
  int rc = plan_check(n_fits, n, n_chains);
  if (rc) return rc;
  batch_plan(n_fits, n, n_chains, seg_offsets, tiles, wg_map);
  return CLV_OK;
}

int clv_batch_info(int32_t D, int32_t K, int64_t* out) {
  if (!out) return fail(CLV_EINVAL, "null argument");
  if ((D != 2 && D != 3) || K < 1 || K > CLV_MAX_K) return fail(CLV_EINVAL, "D must be 2 or 3 and K 1 .. 9");
  int vg = 0, bpc = 0, dev = 0;
  size_t scratch = 0;
  CLV_HIP(batch_fit_resources(D, K, &vg, &scratch, &bpc));
  hipDeviceProp_t prop{};
  CLV_HIP(hipGetDevice(&dev));
  CLV_HIP(hipGetDeviceProperties(&prop, dev));
  out[0] = vg;
  out[1] = (int64_t)scratch;
  out[2] = bpc;
  out[3] = (int64_t)prop.multiProcessorCount * bpc;
  out[4] = prop.multiProcessorCount;
  return CLV_OK;
}

int clv_batch_fit(int32_t device, int32_t D, int32_t K, int32_t n_mh_steps, int32_t n_chains, int32_t burnin,
                  int32_t mcmc, int32_t thin, int32_t draw_sink, int64_t n_fits, const clv_batch_item* fits,
                  double* kernel_ms) {
  if (!fits) return fail(CLV_EINVAL, "null argument");
  if (D != 2 && D != 3) return fail(CLV_EINVAL, "D must be 2 or 3");
  if (K < 1 || K > CLV_MAX_K) return fail(CLV_EINVAL, "K must be in 1..9");
  if (n_mh_steps < 0) return fail(CLV_EINVAL, "n_mh_steps must be >= 0");
  if (thin < 1) return fail(CLV_EINVAL, "thin must be >= 1");
  if (burnin < 0 || mcmc < 0) return fail(CLV_EINVAL, "burnin/mcmc must be >= 0");
  if (draw_sink != CLV_SINK_FULL && draw_sink != CLV_SINK_SUMMARY && draw_sink != CLV_SINK_NONE)
    return fail(CLV_EINVAL, "draw_sink must be CLV_SINK_FULL, CLV_SINK_SUMMARY or CLV_SINK_NONE");
  if (n_fits < 1 || n_fits > (int64_t)0x7fffffff) return fail(CLV_EINVAL, "n_fits must be >= 1");
  std::vector<int64_t> ns((size_t)n_fits);
  for (int64_t j = 0; j < n_fits; ++j) ns[j] = fits[j].n;
  int rc = plan_check(n_fits, ns.data(), n_chains);
  if (rc) return rc;
  const int64_t n_draws = mcmc >= 1 ? (mcmc - 1) / thin + 1 : 0;
  const int stride = K * D + D * (D + 1) / 2 + 1, l2w = D * K + D * (D + 1) / 2;
  const int64_t C = n_chains;
  for (int64_t j = 0; j < n_fits; ++j) {
    const clv_batch_item& q = fits[j];
    const std::string who = "fit " + std::to_string(j) + ": ";
    if (!q.x || !q.t_x || !q.T_cal || !q.prior) return fail(CLV_EINVAL, who + "missing CBS column or prior");
    if ((K > 1) != (q.covariates != nullptr)) return fail(CLV_EINVAL, who + "covariates do not match K");
    if ((D == 3) != (q.log_s != nullptr)) return fail(CLV_EINVAL, who + "log_s does not match D");
    if (n_draws > 0 && (!q.level2 || !q.loglik)) return fail(CLV_EINVAL, who + "level2 / loglik outputs missing");
    if (draw_sink == CLV_SINK_FULL && n_draws > 0 && !q.level1) return fail(CLV_EINVAL, who + "the full sink needs level1");
    if (draw_sink == CLV_SINK_SUMMARY && !q.sums) return fail(CLV_EINVAL, who + "the summary sink needs sums");
  }

  std::vector<int64_t> seg((size_t)n_fits + 1);
  std::vector<int32_t> tiles((size_t)n_fits), map((size_t)(2 * n_fits * C));
  batch_plan(n_fits, ns.data(), n_chains, seg.data(), tiles.data(), map.data());
  const int64_t N = seg[n_fits];
  std::vector<int64_t> tseg((size_t)n_fits + 1, 0);  // tiles before fit j
  for (int64_t j = 0; j < n_fits; ++j) tseg[j + 1] = tseg[j] + tiles[j];
  const int64_t TT = tseg[n_fits];
  const bool full = draw_sink == CLV_SINK_FULL && n_draws > 0, summary = draw_sink == CLV_SINK_SUMMARY;

  DeviceScope ds(device);
  const size_t l1_doubles = full ? (size_t)C * n_draws * N * (D + 2) : 0;
  const size_t sum_doubles = summary ? (size_t)C * CLV_N_SUM_STATS * N : 0;
  {  // what the sink needs against what the device has, before anything is allocated
    size_t free_b = 0, total_b = 0;
    CLV_HIP(hipMemGetInfo(&free_b, &total_b));
    const double need = 8.0 * ((double)l1_doubles + (double)sum_doubles + (2.0 * C + 3.0 + K) * (double)N +
                               (double)C * stride * TT + (double)n_fits * (C * (HS + n_draws * (l2w + 1.0)) + PRIOR_DOUBLES + 40)) +
                        (double)n_fits * sizeof(SweepArgs);
    if (need > (double)free_b)
      return fail(CLV_EINVAL, "the batch needs " + std::to_string((uint64_t)need) + " bytes of device memory (" +
                                  std::to_string((uint64_t)free_b) + " free)" +
                                  (full ? "; use draw_sink=\"summary\" (CLV_SINK_SUMMARY) or fewer fits per call"
                                        : "; use fewer fits per call"));
  }

  // inputs, concatenated per column: fit j's segment starts at seg[j] (covariates: (K - 1) seg[j])
  std::vector<int32_t> hx((size_t)N);
  std::vector<double> htx((size_t)N), hT((size_t)N), hcov((size_t)(K - 1) * N), hls(D == 3 ? (size_t)N : 0);
  std::vector<double> hprior((size_t)n_fits * PRIOR_DOUBLES, 0.0), hbs((size_t)n_fits * (K * D + D * D), 0.0);
  for (int64_t j = 0; j < n_fits; ++j) {
    const clv_batch_item& q = fits[j];
    const size_t n = (size_t)q.n, o = (size_t)seg[j];
    std::copy(q.x, q.x + n, hx.begin() + o);
    std::copy(q.t_x, q.t_x + n, htx.begin() + o);
    std::copy(q.T_cal, q.T_cal + n, hT.begin() + o);
    if (K > 1) std::copy(q.covariates, q.covariates + (size_t)(K - 1) * n, hcov.begin() + (size_t)(K - 1) * o);
    if (D == 3) std::copy(q.log_s, q.log_s + n, hls.begin() + o);
    double* pr = hprior.data() + (size_t)j * PRIOR_DOUBLES;
    for (int i = 0; i < K * K; ++i) {
      pr[i] = q.prior->V[i];
      pr[81 + i] = q.prior->chol_V[i];
    }
    for (int i = 0; i < K * D; ++i) pr[162 + i] = q.prior->A0B0[i];
    for (int i = 0; i < D * D; ++i) pr[189 + i] = q.prior->S0_B0A0B0[i];
    double* bs = hbs.data() + (size_t)j * (K * D + D * D);
    for (int i = 0; i < K * D; ++i) bs[i] = q.prior->beta_init[i];
    for (int i = 0; i < D * D; ++i) bs[K * D + i] = q.prior->sigma_init[i];
  }

  hipStream_t st = nullptr;
  DevBuf bx, btx, bT, bcov, bls, bprior, bbs, blam, bmu, bhyper, bpart, bl1, bl2, bll, bsums, bargs, bmap;
  auto up = [&](DevBuf& b, const void* src, size_t bytes) -> int {
    if (!bytes) return CLV_OK;
    CLV_HIP(hipMalloc(&b.p, bytes));
    CLV_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
    return CLV_OK;
  };
  auto zeros = [&](DevBuf& b, size_t doubles) -> int {
    if (!doubles) return CLV_OK;
    CLV_HIP(hipMalloc(&b.p, sizeof(double) * doubles));
    CLV_HIP(hipMemsetAsync(b.p, 0, sizeof(double) * doubles, st));
    return CLV_OK;
  };
  if ((rc = up(bx, hx.data(), sizeof(int32_t) * hx.size())) || (rc = up(btx, htx.data(), 8 * htx.size())) ||
      (rc = up(bT, hT.data(), 8 * hT.size())) || (rc = up(bcov, hcov.data(), 8 * hcov.size())) ||
      (rc = up(bls, hls.data(), 8 * hls.size())) || (rc = up(bprior, hprior.data(), 8 * hprior.size())) ||
      (rc = up(bbs, hbs.data(), 8 * hbs.size())) || (rc = up(bmap, map.data(), sizeof(int32_t) * map.size())) ||
      (rc = zeros(blam, (size_t)C * N)) || (rc = zeros(bmu, (size_t)C * N)) || (rc = zeros(bhyper, (size_t)n_fits * C * HS)) ||
      (rc = zeros(bpart, (size_t)C * stride * TT)) || (rc = zeros(bl1, l1_doubles)) ||
      (rc = zeros(bl2, (size_t)n_fits * C * n_draws * l2w)) || (rc = zeros(bll, (size_t)n_fits * C * n_draws)) ||
      (rc = zeros(bsums, sum_doubles)))
    return rc;

  // one SweepArgs per fit, its pointers into the fit's own segments ([chain]-leading arrays: C seg[j])
  std::vector<SweepArgs> args((size_t)n_fits);
  for (int64_t j = 0; j < n_fits; ++j) {
    const clv_batch_item& q = fits[j];
    SweepArgs& a = args[j];
    a = SweepArgs{};
    Geometry& g = a.g;
    g.D = D;
    g.K = K;
    g.S = n_mh_steps;
    g.n_chains = n_chains;
    g.n = g.n_global = q.n;
    g.shard_begin = 0;
    g.nb_local = g.blocks_per_rank = g.units_per_rank = tiles[j];
    g.blocks_per_unit = 1;
    g.n_units_global = tiles[j];
    g.world_size = 1;
    g.stride = stride;
    g.burnin = burnin;
    g.mcmc = mcmc;
    g.thin = thin;
    g.n_draws = (int)n_draws;
    g.l2w = l2w;
    a.r.seed = q.seed;
    a.r.chain_first = 0;
    const int64_t o = seg[j];
    a.x = bx.as<int32_t>() + o;
    a.tx = btx.as<double>() + o;
    a.T = bT.as<double>() + o;
    a.cov = K > 1 ? bcov.as<double>() + (int64_t)(K - 1) * o : nullptr;
    a.log_s = D == 3 ? bls.as<double>() + o : nullptr;
    a.lam = blam.as<double>() + C * o;
    a.mu = bmu.as<double>() + C * o;
    double* hyper = bhyper.as<double>() + j * C * HS;
    a.hyper = hyper;
    a.blockpart = bpart.as<double>() + C * stride * tseg[j];
    a.level1 = full ? bl1.as<double>() + C * n_draws * o * (D + 2) : nullptr;
    a.sums = summary ? bsums.as<double>() + C * CLV_N_SUM_STATS * o : nullptr;
    a.lam_init = q.prior->lam_init;
    a.rank = 0;
    HyperArgs& h = a.h;
    h.g = g;
    h.r = a.r;
    h.units = a.blockpart;
    h.hyper = hyper;
    h.level2 = n_draws ? bl2.as<double>() + j * C * n_draws * l2w : nullptr;
    h.loglik = n_draws ? bll.as<double>() + j * C * n_draws : nullptr;
    const double* pr = bprior.as<double>() + j * PRIOR_DOUBLES;
    h.V = pr;
    h.cholV = pr + 81;
    h.A0B0 = pr + 162;
    h.S0B = pr + 189;
    h.nu_n = q.prior->nu_n;
    h.omega2 = q.prior->omega2;
    h.mode = 2;
    h.hvar = nullptr;  // the draw computes its own variates
  }
  if ((rc = up(bargs, args.data(), sizeof(SweepArgs) * args.size()))) return rc;

  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t err = hipEventCreate(&e0);
  if (err == hipSuccess) err = hipEventCreate(&e1);
  if (err == hipSuccess)
    err = launch_batch_fit(D, K, bargs.as<SweepArgs>(), bmap.as<int2>(), bbs.as<double>(), n_fits * C,
                           (int64_t)burnin + mcmc, st, e0, e1);
  auto down = [&](double* dst, const double* src, size_t doubles) {
    if (err == hipSuccess && dst && doubles) err = hipMemcpyAsync(dst, src, sizeof(double) * doubles, hipMemcpyDeviceToHost, st);
  };
  for (int64_t j = 0; j < n_fits && err == hipSuccess; ++j) {
    const clv_batch_item& q = fits[j];
    const SweepArgs& a = args[j];
    const size_t n = (size_t)q.n;
    if (full) down(q.level1, a.level1, (size_t)C * n_draws * n * (D + 2));
    down(q.level2, a.h.level2, (size_t)C * n_draws * l2w);
    down(q.loglik, a.h.loglik, (size_t)C * n_draws);
    if (summary) down(q.sums, a.sums, (size_t)C * CLV_N_SUM_STATS * n);
    down(q.state_lam, a.lam, (size_t)C * n);
    down(q.state_mu, a.mu, (size_t)C * n);
  }
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  float ms = 0.0f;
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (err != hipSuccess) return fail(CLV_EHIP, std::string("batch fit: ") + hipGetErrorString(err));
  if (kernel_ms) *kernel_ms = (double)ms;
  return CLV_OK;
}

}  // extern "C"
