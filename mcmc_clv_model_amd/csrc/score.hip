// Scoring customers outside the fit from its level-2 draws: host side of
// clv_score_customers / clv_score_customers_sampler / clv_score_info.  The kernels live in
// kernels.hip (score_prepare_kernel, score_kernel) beside the per-customer device functions they
// share with the sweep.
#include <algorithm>
#include <cmath>
#include <string>

#include "analysis_host.h"

using namespace clv;

namespace {

// What the last clv_score_customers* call of this thread launched (clv_score_info).
thread_local int64_t last_info[6] = {-1, -1, -1, -1, -1, -1};  // D, K, sink, VGPRs, scratch bytes, kernel ns

struct ScoreCall {
  int32_t D, K, n_chains;
  int64_t n_draws, n;
  const int32_t* x;
  const double *t_x, *T_cal, *cov, *log_s;
  double omega2;
  int32_t n_mh_steps, warmup, inner;
  uint64_t seed;
  int32_t chain_first;
  int64_t customer_offset, sweep_first;
  const double *init_lam, *init_mu;
  int32_t sink;
  double *level1_out, *sums_out, *state_lam_out, *state_mu_out;
};

bool all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// Every argument error, before any device call (level2: host records, or null when they are a
// sampler's own).
int score_check(const ScoreCall& q, const double* level2) {
  if (q.D != 2 && q.D != 3) return fail(CLV_EINVAL, "D must be 2 or 3");
  if (q.K < 1 || q.K > CLV_MAX_K) return fail(CLV_EINVAL, "K must be 1 .. 9");
  if (q.n_chains < 1 || q.n_draws < 1) return fail(CLV_EINVAL, "n_chains and n_draws must be >= 1");
  if (q.n <= 0) return fail(CLV_EINVAL, "n must be > 0");
  if (!q.x || !q.t_x || !q.T_cal || !q.init_lam || !q.init_mu || !q.state_lam_out || !q.state_mu_out)
    return fail(CLV_EINVAL, "null argument");
  if ((q.K > 1) != (q.cov != nullptr)) return fail(CLV_EINVAL, "covariates do not match K (K - 1 rows of n, none for K = 1)");
  if ((q.D == 3) != (q.log_s != nullptr)) return fail(CLV_EINVAL, "log_s does not match D (needed for D = 3 only)");
  if (q.D == 3 && !(q.omega2 > 0.0 && std::isfinite(q.omega2))) return fail(CLV_EINVAL, "omega2 must be finite and > 0");
  if (q.n_mh_steps < 0) return fail(CLV_EINVAL, "n_mh_steps must be >= 0");
  if (q.inner < 1) return fail(CLV_EINVAL, "inner_sweeps must be >= 1");
  if (q.warmup < 0) return fail(CLV_EINVAL, "warmup must be >= 0");
  if (q.sink != CLV_SINK_FULL && q.sink != CLV_SINK_SUMMARY) return fail(CLV_EINVAL, "sink must be CLV_SINK_FULL or CLV_SINK_SUMMARY");
  if (q.sink == CLV_SINK_FULL && !q.level1_out) return fail(CLV_EINVAL, "the full sink needs level1_out");
  if (q.sink == CLV_SINK_SUMMARY && !q.sums_out) return fail(CLV_EINVAL, "the summary sink needs sums_out");
  if (q.chain_first < 0) return fail(CLV_EINVAL, "chain_first must be >= 0");
  // the Philox counter holds the global customer index and the inner-sweep number in 32 bits each
  if (q.customer_offset < 0 || q.customer_offset > (int64_t)0xFFFFFFFFLL || q.n > (int64_t)0x100000000LL - q.customer_offset)
    return fail(CLV_EINVAL, "customer_offset + n must fit in 32 bits");
  if (q.sweep_first < 1 || q.sweep_first > (int64_t)0xFFFFFFFFLL) return fail(CLV_EINVAL, "sweep_first must be 1 .. 2^32 - 1");
  const int64_t room = (int64_t)0xFFFFFFFFLL - q.sweep_first + 1 - q.warmup;  // sweeps left for the records
  if (room < 1 || q.n_draws > room / q.inner)
    return fail(CLV_EINVAL, "the last inner-sweep number does not fit in 32 bits");
  const size_t n = (size_t)q.n, cn = (size_t)q.n_chains * n;
  for (size_t i = 0; i < n; ++i) {
    if (q.x[i] < 0) return fail(CLV_EINVAL, "x must be >= 0");
    if (!std::isfinite(q.t_x[i]) || !std::isfinite(q.T_cal[i])) return fail(CLV_EINVAL, "non-finite t_x or T_cal");
    if (q.t_x[i] < 0.0 || q.t_x[i] > q.T_cal[i]) return fail(CLV_EINVAL, "t_x must be in [0, T_cal]");
  }
  if (q.cov && !all_finite(q.cov, (size_t)(q.K - 1) * n)) return fail(CLV_EINVAL, "non-finite covariate");
  if (q.log_s && !all_finite(q.log_s, n)) return fail(CLV_EINVAL, "non-finite log_s");
  for (size_t i = 0; i < cn; ++i)
    // the sweep takes the state's logs (bi:286-287; log_fast is defined for positive normal numbers)
    if (!(std::isfinite(q.init_lam[i]) && q.init_lam[i] >= 2.2250738585072014e-308 && std::isfinite(q.init_mu[i]) &&
          q.init_mu[i] >= 2.2250738585072014e-308))
      return fail(CLV_EINVAL, "init must be finite and > 0");
  if (level2) {
    const int w = q.D * q.K + q.D * (q.D + 1) / 2;
    if (!all_finite(level2, (size_t)q.n_chains * q.n_draws * w)) return fail(CLV_EINVAL, "non-finite level-2 record");
    for (int64_t r = 0; r < (int64_t)q.n_chains * q.n_draws; ++r) {
      const double* sg = level2 + r * w + q.D * q.K;  // upper triangle: the diagonal at 0, D, 2 D - 1
      for (int p = 0, at = 0; p < q.D; at += q.D - p, ++p)
        if (!(sg[at] > 0.0)) return fail(CLV_EINVAL, "a level-2 record's Sigma has a non-positive variance");
    }
  }
  return CLV_OK;
}

// d_level2: the records on the device, [chain][n_draws][D K + D (D + 1) / 2].
int score_run(const ScoreCall& q, const double* d_level2, hipStream_t st) {
  const size_t n = (size_t)q.n, C = (size_t)q.n_chains, cn = C * n;
  const bool summary = q.sink == CLV_SINK_SUMMARY;
  const size_t out_doubles = summary ? C * CLV_N_SUM_STATS * n : C * (size_t)q.n_draws * n * (q.D + 2);
  const size_t hyper_doubles = C * (size_t)q.n_draws * HS;
  {  // a full sink larger than the device: say so before anything is allocated
    size_t free_b = 0, total_b = 0;
    CLV_HIP(hipMemGetInfo(&free_b, &total_b));
    const double need = 8.0 * ((double)out_doubles + (double)hyper_doubles + 4.0 * cn + (3.0 + q.K) * n);
    if (need > (double)free_b)
      return fail(CLV_ENOMEM, summary ? std::string("the scoring buffers do not fit in device memory")
                                      : std::string("the full sink's level-1 draws do not fit in device memory; use "
                                                    "sink=\"summary\" (CLV_SINK_SUMMARY) or score fewer customers per call"));
  }
  DevBuf bx, btx, bT, bcov, blogs, blam, bmu, blam_o, bmu_o, bhyper, bout;
  int rc;
  if ((rc = upload(bx, q.x, n, st)) || (rc = upload(btx, q.t_x, n, st)) || (rc = upload(bT, q.T_cal, n, st)) ||
      (rc = upload(bcov, q.cov, (size_t)(q.K - 1) * n, st)) || (rc = upload(blogs, q.log_s, n, st)) ||
      (rc = upload(blam, q.init_lam, cn, st)) || (rc = upload(bmu, q.init_mu, cn, st)))
    return rc;
  CLV_HIP(hipMalloc(&blam_o.p, sizeof(double) * cn));
  CLV_HIP(hipMalloc(&bmu_o.p, sizeof(double) * cn));
  CLV_HIP(hipMalloc(&bhyper.p, sizeof(double) * hyper_doubles));
  CLV_HIP(hipMalloc(&bout.p, sizeof(double) * out_doubles));
  CLV_HIP(hipMemsetAsync(bhyper.p, 0, sizeof(double) * hyper_doubles, st));
  CLV_HIP(launch_score_prepare(q.D, q.K, d_level2, (int64_t)C * q.n_draws, q.D == 3 ? q.omega2 : 1.0,
                               bhyper.as<double>(), st));

  SweepArgs a{};
  a.g.D = q.D;
  a.g.K = q.K;
  a.g.S = q.n_mh_steps;
  a.g.n_chains = q.n_chains;
  a.g.n = a.g.n_global = q.n;
  a.g.shard_begin = q.customer_offset;
  a.g.world_size = 1;
  a.r.seed = q.seed;
  a.r.chain_first = q.chain_first;
  a.x = bx.as<int32_t>();
  a.tx = btx.as<double>();
  a.T = bT.as<double>();
  a.cov = bcov.as<double>();
  a.log_s = blogs.as<double>();
  a.lam = blam.as<double>();
  a.mu = bmu.as<double>();
  ScoreArgs e{};
  e.hyper = bhyper.as<double>();
  e.n_draws = q.n_draws;
  e.s_first = q.sweep_first;
  e.warmup = q.warmup;
  e.inner = q.inner;
  e.level1 = summary ? nullptr : bout.as<double>();
  e.sums = summary ? bout.as<double>() : nullptr;
  e.lam_out = blam_o.as<double>();
  e.mu_out = bmu_o.as<double>();

  hipEvent_t e0 = nullptr, e1 = nullptr;
  CLV_HIP(hipEventCreate(&e0));
  hipError_t err = hipEventCreate(&e1);
  if (err == hipSuccess) err = launch_score(a, e, summary, st, e0, e1);
  if (err == hipSuccess) err = hipMemcpyAsync(summary ? q.sums_out : q.level1_out, bout.p, sizeof(double) * out_doubles, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(q.state_lam_out, blam_o.p, sizeof(double) * cn, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(q.state_mu_out, bmu_o.p, sizeof(double) * cn, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  float ms = 0.0f;
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (err != hipSuccess) return fail(CLV_EHIP, std::string("score: ") + hipGetErrorString(err));
  int vg = 0;
  size_t scratch = 0;
  CLV_HIP(score_resources(q.D, q.K, summary, &vg, &scratch));
  last_info[0] = q.D;
  last_info[1] = q.K;
  last_info[2] = q.sink;
  last_info[3] = vg;
  last_info[4] = (int64_t)scratch;
  last_info[5] = (int64_t)std::llround((double)ms * 1e6);
  return CLV_OK;
}

}  // namespace

extern "C" {

int clv_score_info(int64_t* out) {
  if (!out) return fail(CLV_EINVAL, "null argument");
  out[0] = BLOCK;
  out[1] = CLV_N_SUM_STATS;
  for (int k = 0; k < 6; ++k) out[2 + k] = last_info[k];
  return CLV_OK;
}

int clv_debug_score_hyper(int32_t device, int32_t D, int32_t K, int64_t n_rec, const double* level2, double omega2,
                          double* out) {
  if ((D != 2 && D != 3) || K < 1 || K > CLV_MAX_K || n_rec < 1 || !level2 || !out) return fail(CLV_EINVAL, "bad arguments");
  if (D == 3 && !(omega2 > 0.0 && std::isfinite(omega2))) return fail(CLV_EINVAL, "omega2 must be finite and > 0");
  DeviceScope ds(device);
  DevBuf bl2, bh;
  const size_t out_bytes = sizeof(double) * (size_t)n_rec * HS;
  int rc = upload(bl2, level2, (size_t)n_rec * (D * K + D * (D + 1) / 2), nullptr);
  if (rc) return rc;
  CLV_HIP(hipMalloc(&bh.p, out_bytes));
  CLV_HIP(hipMemsetAsync(bh.p, 0, out_bytes, nullptr));
  CLV_HIP(launch_score_prepare(D, K, bl2.as<double>(), n_rec, D == 3 ? omega2 : 1.0, bh.as<double>(), nullptr));
  CLV_HIP(hipMemcpyAsync(out, bh.p, out_bytes, hipMemcpyDeviceToHost, nullptr));
  CLV_HIP(hipStreamSynchronize(nullptr));
  return CLV_OK;
}

int clv_score_customers(int32_t device, int32_t D, int32_t K, int32_t n_chains, int64_t n_draws, const double* level2,
                        int64_t n, const int32_t* x, const double* t_x, const double* T_cal, const double* cov,
                        const double* log_s, double omega2, int32_t n_mh_steps, int32_t warmup, int32_t inner_sweeps,
                        uint64_t seed, int32_t chain_first, int64_t customer_offset, int64_t sweep_first,
                        const double* init_lam, const double* init_mu, int32_t sink, double* level1_out,
                        double* sums_out, double* state_lam_out, double* state_mu_out) {
  if (!level2) return fail(CLV_EINVAL, "null argument");
  const ScoreCall q{D, K, n_chains, n_draws, n, x, t_x, T_cal, cov, log_s, omega2, n_mh_steps, warmup, inner_sweeps,
                    seed, chain_first, customer_offset, sweep_first, init_lam, init_mu, sink, level1_out, sums_out,
                    state_lam_out, state_mu_out};
  int rc = score_check(q, level2);
  if (rc) return rc;
  DeviceScope ds(device);
  DevBuf bl2;
  if ((rc = upload(bl2, level2, (size_t)n_chains * n_draws * (D * K + D * (D + 1) / 2), nullptr))) return rc;
  return score_run(q, bl2.as<double>(), nullptr);
}

int clv_score_customers_sampler(clv_sampler* s, int64_t n, const int32_t* x, const double* t_x, const double* T_cal,
                                const double* cov, const double* log_s, int32_t n_mh_steps, int32_t warmup,
                                int32_t inner_sweeps, uint64_t seed, int64_t customer_offset, int64_t sweep_first,
                                const double* init_lam, const double* init_mu, int32_t sink, double* level1_out,
                                double* sums_out, double* state_lam_out, double* state_mu_out) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  const Geometry& g = s->g;
  const ScoreCall q{g.D, g.K, g.n_chains, g.n_draws, n, x, t_x, T_cal, cov, log_s, s->prior.omega2, n_mh_steps,
                    warmup, inner_sweeps, seed, s->cfg.chain_first, customer_offset, sweep_first, init_lam, init_mu,
                    sink, level1_out, sums_out, state_lam_out, state_mu_out};
  int rc = score_check(q, nullptr);
  if (rc) return rc;
  if (s->replay) return fail(CLV_ESTATE, "scoring draws Philox variates: not for a replay-mode sampler");
  const double* l2;
  if ((rc = sampler_l2(s, &l2, "the run has not stored all of its level-2 records yet"))) return rc;
  return score_run(q, l2, s->stream);
}

}  // extern "C"
