// C ABI of libclvmcmc.so (declared in include/clvmcmc.h): device memory, the sweep pipeline,
// hipGraph capture of sweep chunks, and outputs.  Host-side replacement of _run_chain /
// mcmc_draw_parameters (src/models/bivariate/mcmc.py:346-504, trivariate/mcmc.py:465-657).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "internal.h"
#include "kernels.h"
#include "philox.h"

using namespace clv;

namespace {

thread_local std::string g_err;

// The prior as the device holds it: V, cholV (9 x 9 each), A0B0 (9 x 3), S0B (3 x 3)
constexpr int PRIOR_V = 0, PRIOR_CHOLV = 81, PRIOR_A0B0 = 162, PRIOR_S0B = 189, PRIOR_DOUBLES = 198;
constexpr int GRAPH_CHUNK = 64;                  // sweeps per captured graph
constexpr int TIMING_EVENTS = 256;               // sweep launches timed per harvest

}  // namespace

int clv::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {

HyperArgs hyper_args(clv_sampler* s, const double* units, int mode);

Rng rng_args(const clv_sampler* s) {  // (seed, chain_first, tape, tape_sweep_stride, tape_sweeps)
  return Rng{s->cfg.seed, s->cfg.chain_first, s->d_tape, clv_replay_sweep_stride(s), s->tape_sweeps};
}

std::vector<double> pack_prior(const clv_prior* prior, int D, int K) {
  std::vector<double> pr(PRIOR_DOUBLES, 0.0);
  for (int i = 0; i < K * K; ++i) {
    pr[PRIOR_V + i] = prior->V[i];
    pr[PRIOR_CHOLV + i] = prior->chol_V[i];
  }
  for (int i = 0; i < K * D; ++i) pr[PRIOR_A0B0 + i] = prior->A0B0[i];
  for (int i = 0; i < D * D; ++i) pr[PRIOR_S0B + i] = prior->S0_B0A0B0[i];
  return pr;
}

SweepArgs sweep_args(clv_sampler* s, int init, int fuse = 0) {
  SweepArgs a{};
  a.g = s->g;
  a.r = rng_args(s);
  a.x = s->d_x;
  a.tx = s->d_tx;
  a.T = s->d_T;
  a.cov = s->d_cov;
  a.log_s = s->d_logs;
  a.lam = s->d_lam;
  a.mu = s->d_mu;
  a.hyper = s->d_hyper;
  a.blockpart = s->d_block;
  a.pblock = s->d_pblock;
  a.ctrl = s->d_ctrl;
  a.level1 = s->d_level1;
  a.sums = s->d_sums;
  a.qstore = s->d_qstore;
  a.n_stored = nullptr;
  a.lam_init = s->prior.lam_init;
  a.init = init;
  a.fuse = fuse;
  a.chain_arrive = s->d_arrive;
  a.unit_arrive = s->d_arrive + s->g.n_chains;
  a.ctrl_rw = s->d_ctrl;
  a.hyp2 = s->d_hyp2;
  a.unitpart = s->d_unit;
  a.hvar_out = s->d_hvar;
  a.stamps = s->d_stamps;
  a.mail = s->d_mail;
  a.peers = s->d_peers;
  a.wg_map = s->d_wgmap;
  a.rank = s->cfg.rank;
  a.lam_out = s->d_lam_alt ? s->d_lam_alt : s->d_lam;
  a.mu_out = s->d_mu_alt ? s->d_mu_alt : s->d_mu;
  a.hyper_out = s->d_hyper_alt ? s->d_hyper_alt : s->d_hyper;
  a.wait_ticks = s->wait_ticks;
  a.abort_host = s->d_h_abort;
  a.diag = s->d_diag;
  a.clk = s->d_clk;
  a.h = hyper_args(s, nullptr, 0);
  if (fuse) a.h.hvar = (s->replay || s->g.nb_local == 0) ? nullptr : s->d_hvar;  // (as hyper_args: no workgroup, no precomputed variates)
  return a;
}

HyperArgs hyper_args(clv_sampler* s, const double* units, int mode) {
  HyperArgs a{};
  a.g = s->g;
  a.r = rng_args(s);
  a.units = units ? units : s->d_unit;
  a.hyper = s->d_hyper;
  a.ctrl = s->d_ctrl;
  a.level2 = s->d_level2;
  a.loglik = s->d_loglik;
  a.V = s->d_prior + PRIOR_V;
  a.cholV = s->d_prior + PRIOR_CHOLV;
  a.A0B0 = s->d_prior + PRIOR_A0B0;
  a.S0B = s->d_prior + PRIOR_S0B;
  a.nu_n = s->prior.nu_n;
  a.omega2 = s->prior.omega2;
  a.mode = mode;
  a.stamps = s->d_stamps;
  // mode 0 follows a sweep kernel, which precomputed the draw's variates (if it had workgroups)
  a.hvar = (mode == 0 && !s->replay && s->g.nb_local > 0) ? s->d_hvar : nullptr;
  return a;
}

// The block partials of the sweep just enqueued summed into unit partials (blocks_per_unit > 1).
int enqueue_group(clv_sampler* s) {
  if (s->g.blocks_per_unit == 1) return CLV_OK;
  GroupArgs ga{};
  ga.g = s->g;
  ga.blockpart = s->d_block;
  ga.unitpart = s->d_unit;
  CLV_HIP(launch_group(ga, s->stream));
  return CLV_OK;
}

int enqueue_sweep(clv_sampler* s, hipEvent_t e0, hipEvent_t e1) {
  s->last_persist_n = 0;
  CLV_HIP(launch_sweep(sweep_args(s, 0), s->replay, s->stream, e0, e1));
  return enqueue_group(s);
}

// world_size == 1: one launch per sweep (the level-2 draw runs in the sweep kernel's tail)
int enqueue_fused(clv_sampler* s, hipEvent_t e0, hipEvent_t e1) {
  s->last_persist_n = 0;
  CLV_HIP(launch_sweep(sweep_args(s, 0, 1), s->replay, s->stream, e0, e1));
  return CLV_OK;
}

int enqueue_hyper(clv_sampler* s, const double* units, int mode, hipEvent_t e0, hipEvent_t e1) {
  s->last_persist_n = 0;
  if (e0) CLV_HIP(hipEventRecord(e0, s->stream));
  CLV_HIP(launch_hyper(hyper_args(s, units, mode), s->replay, s->stream));
  if (e1) CLV_HIP(hipEventRecord(e1, s->stream));
  return CLV_OK;
}

int check_replay_range(clv_sampler* s, int64_t n_more) {
  if (!s->replay) return CLV_OK;
  const int64_t need = s->sweeps_done + n_more + (s->g.D == 2 ? 1 : 0);
  if (!s->d_tape || need > s->tape_sweeps)
    return fail(CLV_ESTATE, "replay tape too short: need " + std::to_string(need) + " sweeps, have " +
                                std::to_string(s->tape_sweeps));
  return CLV_OK;
}

int harvest_timing(clv_sampler* s) {
  if (s->ev_used == 0) return CLV_OK;
  CLV_HIP(hipEventSynchronize(s->ev[4 * (s->ev_used - 1) + 1]));
  for (int k = 0; k < s->ev_used; ++k) {
    float ms = 0.f;
    CLV_HIP(hipEventElapsedTime(&ms, s->ev[4 * k], s->ev[4 * k + 1]));
    s->t_sweep_ms += ms;  // fused: the level-2 draw is inside the timed launch
    s->n_sweep_timed += s->ev_sweeps.empty() ? 1 : s->ev_sweeps[k];  // persistent: many sweeps
  }
  s->ev_used = 0;
  return CLV_OK;
}

int ensure_events(clv_sampler* s) {
  if (s->ev.empty()) {
    s->ev.resize(4 * TIMING_EVENTS);
    for (auto& e : s->ev) CLV_HIP(hipEventCreate(&e));
  }
  return CLV_OK;
}

// The captured graph holds state pointers, the tape, the wait bound and its stream: dropped when one changes.
int drop_graph(clv_sampler* s) {
  if (s->graph_exec) {
    CLV_HIP(hipGraphExecDestroy(s->graph_exec));
    s->graph_exec = nullptr;
  }
  return CLV_OK;
}

int build_graph(clv_sampler* s, int n) {
  if (s->graph_exec && s->graph_sweeps == n) return CLV_OK;
  if (int rc = drop_graph(s)) return rc;
  hipGraph_t graph;
  CLV_HIP(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
  for (int k = 0; k < n; ++k) {
    int rc = enqueue_fused(s, nullptr, nullptr);
    if (rc != CLV_OK) {
      hipGraph_t dummy;
      (void)hipStreamEndCapture(s->stream, &dummy);
      return rc;
    }
  }
  CLV_HIP(hipStreamEndCapture(s->stream, &graph));
  CLV_HIP(hipGraphInstantiate(&s->graph_exec, graph, nullptr, nullptr, 0));
  CLV_HIP(hipGraphDestroy(graph));
  s->graph_sweeps = n;
  return CLV_OK;
}

bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// Hand the level-1 draws completed since the last call to the copy pool (clv_stream_draws).
void stream_enqueue(clv_sampler* s) {
  if (!s->ds_dest || !s->d_level1) return;
  const Geometry& g = s->g;
  const int64_t k = stored_draws(s);
  if (k <= s->ds_next) return;
  const int64_t row = g.n * (g.D + 2);  // doubles per draw and chain
  for (int c = 0; c < g.n_chains; ++c) {
    const int64_t off = ((int64_t)c * g.n_draws + s->ds_next) * row;
    stream_copy(s->ds, s->device, s->d_level1 + off, s->ds_dest + off, sizeof(double) * (size_t)((k - s->ds_next) * row));
  }
  s->ds_next = k;
}

// Before the draws already streamed may be rewritten (the state is set back): wait for the copies in
// flight and stream again from the first draw the new sweep count has not stored.
void stream_rewind(clv_sampler* s) {
  if (!s->ds_dest) return;
  stream_wait(s->ds);
  s->ds_next = std::min(s->ds_next, stored_draws(s));
}

// The wait-timeout record of the last failed launch (kernels.hip report_wait) as text, and cleared
// for the next one; "" if no wave recorded one.
std::string take_wait_diag(clv_sampler* s) {
  if (!s->d_diag) return "";
  unsigned long long d[DIAG_WORDS] = {};
  if (hipMemcpy(d, s->d_diag, sizeof(d), hipMemcpyDeviceToHost) != hipSuccess) return "";
  (void)hipMemset(s->d_diag, 0, sizeof(d));
  if (!d[0]) return "";
  const Geometry& g = s->g;
  const char* what = d[1] == WAIT_HYPER ? "(beta, Sigma) hand-off slot"
                     : d[1] == WAIT_BLOCKS ? "block partial"
                     : d[1] == WAIT_RELAY ? "split layout's relay flag of workgroup"
                     : d[1] == WAIT_P2P_MAIL ? "peer unit partial (persistent)" : "peer unit partial (fused)";
  std::string m = std::string(" [wait record: sweep ") + std::to_string((long long)d[2]) + ", chain " +
                  std::to_string(d[3]) + ", rank " + std::to_string(d[4]) + ": " + what + " ";
  const long long unit = (long long)d[5];
  if ((d[1] == WAIT_P2P_MAIL || d[1] == WAIT_FX_MAIL) && g.units_per_rank > 0 && unit >= 0)
    m += "unit " + std::to_string(unit) + " (rank " + std::to_string(unit / g.units_per_rank) + ", local unit " +
         std::to_string(unit % g.units_per_rank) + ")";
  else
    m += (d[1] == WAIT_HYPER ? "of block " : "") + std::to_string(unit);
  if (d[1] == WAIT_RELAY) m += " (statistic: the wave row, bits: the flag's tag)";
  char bits[32];
  std::snprintf(bits, sizeof(bits), "%016llx", d[7]);
  m += " statistic " + std::to_string((long long)d[6]) + " still empty (bits " + bits + ") after " +
       std::to_string(d[8]) + " polls, " + std::to_string(d[9] / 100000.0) + " ms; " + std::to_string(d[10]) +
       " lanes of the wave missing";
  if (d[1] == WAIT_P2P_MAIL || d[1] == WAIT_FX_MAIL) {
    m += "; progress (sweep each rank's level-2 side last polled for):";
    for (int q = 0; q < std::min(g.world_size, 5); ++q)
      m += " " + std::to_string(q) + ":" + (d[11 + q] == ~0ull ? std::string("none") : std::to_string((long long)d[11 + q]));
  }
  return m + "]";
}

// CLV_WAIT_TIMEOUT_MS: a finite decimal number (surrounding blanks allowed; no hex, inf or nan),
// clamped to the range clv_set_wait_timeout accepts, [1 ms, 1 h].  distributed.run_wait_ms applies
// the same rule in Python.
bool parse_wait_ms(const char* txt, double* ms) {
  for (const char* c = txt; *c; ++c)
    if (*c == 'x' || *c == 'X' || *c == 'n' || *c == 'N' || *c == 'i' || *c == 'I') return false;
  char* end = nullptr;
  const double v = std::strtod(txt, &end);
  if (end == txt) return false;
  while (*end == ' ' || *end == '\t' || *end == '\n') ++end;
  if (*end || !(v == v) || v > 1e300 || v < -1e300) return false;
  *ms = std::min(3.6e6, std::max(1.0, v));
  return true;
}

}  // namespace

extern "C" {

int32_t clv_abi_version(void) { return CLV_ABI_VERSION; }

int32_t clv_default_blocks_per_unit(int64_t n_global) {
  // Keep the number of exchanged/reduced units <= 512 (one hyper workgroup sums them).
  const int64_t nb = (n_global + BLOCK - 1) / BLOCK;
  int32_t g = 1;
  while ((nb + g - 1) / g > 512) g *= 2;
  return g;
}

const char* clv_last_error(void) { return g_err.c_str(); }

int64_t clv_sizeof(int32_t which) {
  switch (which) {
    case 0: return (int64_t)sizeof(clv_config);
    case 1: return (int64_t)sizeof(clv_data);
    case 2: return (int64_t)sizeof(clv_prior);
    default: return -1;
  }
}

int clv_device_count(int32_t* count) {
  int n = 0;
  CLV_HIP(hipGetDeviceCount(&n));
  *count = n;
  return CLV_OK;
}

int64_t clv_replay_sweep_stride(const clv_sampler* s) {
  const int64_t n = s->g.n;
  return n * (2 + 3 * (int64_t)s->g.S + (s->g.D == 3 ? 1 : 0)) + TAPE_HYPER;
}

}  // extern "C"

// The persistent kernels spin on other workgroups of their grid, so every workgroup must be
// resident at once.  Admitted 256-thread blocks per CU (MI355X guide, "Residency and cooperative
// launch") = min(occupancy API, 8, floor(800 / (ceil(sgpr/16)*16 + 16))); the API answer is one
// high only where the SGPR term binds.  The persistent instances are VGPR-bound at 2 blocks per CU
// (129-256 VGPRs: 2 waves per SIMD) and their SGPR term is >= 6 even at the architectural maximum
// of 102 SGPRs, so it is applied at that maximum (never binding here) and a margin of one slot per
// 32 CUs guards against another kernel of the process holding slots.  c2 / c3: 376 of 512 slots;
// c4 at 8 ranks: 497 of 512 (504 allowed).  Every wait is bounded regardless.
bool clv::persist_grid_fits(int64_t grid_wgs, int blocks_per_cu, int n_cu) {
  constexpr int SGPR_MAX = 102;
  const int sgpr_term = 800 / (((SGPR_MAX + 15) / 16) * 16 + 16);
  const int64_t per_cu = std::min({blocks_per_cu, 8, sgpr_term});
  const int64_t slots = per_cu * n_cu;
  const int64_t margin = std::max(1, n_cu / 32);
  return grid_wgs > 0 && slots > 0 && grid_wgs <= slots - margin;
}

// Whether the persistent kernel is worth running a resident grid of grid_wgs workgroups (world size
// 1 and the peer exchange).  Round 4 measured it losing to the launch-per-sweep kernel once most CUs
// held two of its workgroups (c4's 8-rank shard, 1 chain x 497 workgroups: 43.8 vs 22.4 us per sweep)
// and capped it by density.  The cause was not the doubled SIMDs: the level-2 workgroup emptied its
// chain's hand-off slots lane-per-block (one double of a different line per lane and instruction), and
// at ~500 blocks those ~7k partial-line write-throughs queued ahead of its draw (the draw measured 9.2
// us of a 20 us sweep, profiles/r06_c4shard8_stamps_*.txt).  With coalesced resets (round 6) the
// persistent kernel wins at every measured point (tools/persist_crossover.py,
// profiles/r06_persist_crossover*.jsonl; us per sweep persistent / launch-per-sweep, workgroups per CU):
//   bivariate, 4 chains  K=2: 1.25 10.1 / 17.1, 1.61 9.8 / 18.2, 1.73 9.9 / 18.3, 1.86 10.3 / 19.0
//                        K=5: 1.25 10.4 / 18.5, 1.61 10.1 / 19.5
//   bivariate, 1-2 chains K=2: 0.92 7.2 / 15.2, 1.38 10.1 / 17.6, 1.68 10.3 / 18.3, 2 chains 1.84
//                        10.6 / 19.0; K=5: 0.92 9.2 / 16.6, 1.38 12.6 / 18.7, 1.68 13.8 / 19.6,
//                        1.91 14.1 / 20.3 (c4 at 8 ranks); K=9: 0.92 12.8 / 18.4, 1.38 16.9 / 22.5
//   trivariate, 4 chains K=3: 1.25 10.8 / 19.7, 1.61 11.5 / 20.7; 1 chain K=3: 1.38 14.6 / 19.6,
//                        1.68 15.6 / 20.6; K=9 (its persistent instance spills): 0.92 20.1 / 20.8
// So: wherever the grid fits (persist_grid_fits).  Kept as a function: the CPU test pins the choice.
// Instances whose private segment (spills) exceeds this many bytes per lane are never run
// persistently: the trivariate K = 9 peer instance (768 B per lane) at world 2 on one card left 39 of
// a chain's 40 customer workgroups undispatched until its 10 s wait bound (round 6) — the runtime
// provisions scratch for a limited number of waves, and a persistent grid must be resident whole.
// Every instance a BASELINE configuration selects is at or below it: world size 1 0 B (bivariate K <=
// 8, trivariate K <= 4), peer c2-tiled <2,2> 0 B, c4 at 8 ranks <2,5> 56 B, <3,3> 48 B (the tests'
// world-3 trivariate run).  (llvm-readelf --notes: .private_segment_fixed_size.)
constexpr size_t PERSIST_SCRATCH_MAX = 64;
// The split layout's relay instance with CLV_SPLIT_RELAY unset (the measurement
// that decides it).
#ifndef CLV_SPLIT_RELAY_DEFAULT
#define CLV_SPLIT_RELAY_DEFAULT 1
#endif
constexpr bool SPLIT_RELAY_DEFAULT = CLV_SPLIT_RELAY_DEFAULT != 0;

namespace {

bool persist_worth(int D, int K, int n_chains, int64_t grid_wgs, int n_cu) {
  (void)D, (void)K, (void)n_chains;
  return n_cu > 0 && grid_wgs > 0;
}

// The split layout's residency rule.  Its 512-thread workgroups fill a CU each (8 waves of up to 256
// VGPRs, ~95 KB of LDS), so the grid of chains x (split_wgs(nb) + 1) workgroups needs that many CUs
// free at once, and the dispatcher has nowhere else to put a workgroup: one slot per CU, less a
// margin of one CU per 64 (4 of 256; c2 and c3 take 252).  The block rule's margin is one slot per 32
// CUs of two-slot CUs; here a slot is a whole CU, so the same share of the card would leave c2 out.
// Every wait stays bounded, and a handle whose split launch aborts goes back to the block layout.
bool persist_split_fits(int n_chains, int nb, int blocks_per_cu, int n_cu) {
  if (n_chains < 1 || nb < 1 || nb > SPLIT_MAX_NB || blocks_per_cu < 1 || n_cu < 1) return false;
  const int64_t grid = (int64_t)n_chains * (split_wgs(nb) + 1);
  const int64_t margin = std::max(1, n_cu / 64);
  return grid <= n_cu - margin;
}

// Worth choosing only where the block layout doubles up: with one block workgroup per CU no SIMD
// holds two customer waves and there is nothing to balance.
bool persist_split_pays(int n_chains, int nb, int n_cu) { return (int64_t)n_chains * (nb + 1) > n_cu; }

// Per physical workgroup chain << 16 | p, chain by chain, each chain's workgroups in order (workgroup p hosts
// wave rows 6p .. 6p + 5), its level-2 workgroup (p = split_wgs(nb)) last: consecutive dispatch positions go round the XCDs, so every chain spreads
// over all of them.
std::vector<int32_t> persist_split_layout(int n_chains, int nb) {
  const int per = split_wgs(nb) + 1;
  std::vector<int32_t> map((size_t)n_chains * per);
  for (int c = 0; c < n_chains; ++c)
    for (int p = 0; p < per; ++p) map[(size_t)c * per + p] = (c << 16) | p;
  return map;
}

// Persistent grid: which (chain, block) each dispatched workgroup runs.  The grid has more
// workgroups (T = chains x (blocks + 1)) than CUs, and the dispatcher fills every CU once before
// doubling up: linear workgroup i < T - n_cu shares its CU with workgroup i + n_cu (measured,
// tools/placement.py).  A SIMD holding two customer waves runs each at ~0.68 of its solo speed,
// and the hardware favours the older wave; pairing two waves of DIFFERENT chains lets the older
// chain run ahead while the younger one crawls, and the run lasts until the slowest chain ends.
// So shared CUs pair workgroups of the SAME chain (every chain then paces at its pairs' rate), each
// chain's level-2 workgroup (asleep most of the time) shares a CU with one of its own customer
// workgroups, and the pairs are spread evenly over the chains.  Pure placement: every workgroup
// still runs one logical (chain, block), so results do not depend on it.
// Chains of at least CLV_L2_ALONE_MIN_NB blocks (the level-2 workgroup's lanes then poll two blocks
// each) place their level-2 workgroup on a CU of its own: c4's 8-rank shard (496 blocks, 1 chain)
// 13.54 -> 12.88 us per sweep; c2 (93 blocks per chain) 9.86 -> 9.80, within the noise, so it keeps
// the pairing (profiles/r06_ab_l2alone.txt).
#ifndef CLV_L2_ALONE_MIN_NB
#define CLV_L2_ALONE_MIN_NB 256
#endif
std::vector<int32_t> persist_wg_map(int C, int nb, int n_cu) {
  const int per = nb + 1;  // workgroups per chain (block nb = the level-2 workgroup)
  const int T = C * per;
  std::vector<int32_t> map(T);
  for (int c = 0; c < C; ++c)  // identity: blockIdx = (b, c)
    for (int b = 0; b < per; ++b) map[c * per + b] = (c << 16) | b;
  const int P = T - n_cu;  // shared CUs
  if (P <= 0 || T > 2 * n_cu) return map;
  std::vector<std::vector<int>> todo(C);  // customer blocks of each chain still to place
  for (int c = 0; c < C; ++c)
    for (int b = nb - 1; b >= 0; --b) todo[c].push_back(b);
  std::vector<int32_t> first, second, single;
  int p = 0;
  const bool l2_alone = nb >= CLV_L2_ALONE_MIN_NB;
  for (int c = 0; !l2_alone && c < C && p < P; ++c, ++p) {  // level-2 workgroup + one own customer workgroup
    first.push_back((c << 16) | nb);
    if (todo[c].empty()) return map;
    second.push_back((c << 16) | todo[c].back());
    todo[c].pop_back();
  }
  const int n_l2_paired = (int)first.size();
  const bool l2_paired = n_l2_paired == C;
  for (int c = 0; p < P; c = (c + 1) % C) {  // same-chain customer pairs, round robin over chains
    bool any = false;
    for (int k = 0; k < C && !any; ++k) any = todo[(c + k) % C].size() >= 2;
    if (!any) return map;  // cannot pair within chains: keep the identity
    if (todo[c].size() < 2) continue;
    first.push_back((c << 16) | todo[c].back());
    todo[c].pop_back();
    second.push_back((c << 16) | todo[c].back());
    todo[c].pop_back();
    ++p;
  }
  for (int c = 0; c < C; ++c) {
    if (!l2_paired && c >= n_l2_paired) single.push_back((c << 16) | nb);
    while (!todo[c].empty()) {
      single.push_back((c << 16) | todo[c].back());
      todo[c].pop_back();
    }
  }
  // interleave the chains over the single slots (so that each chain spreads over all XCDs)
  std::vector<int32_t> sorted_single;
  for (size_t k = 0; sorted_single.size() < single.size(); ++k)
    for (int c = 0; c < C; ++c) {
      size_t seen = 0;
      for (int32_t v : single)
        if ((v >> 16) == c && seen++ == k) sorted_single.push_back(v);
    }
  if ((int)first.size() != P || (int)sorted_single.size() != n_cu - P) return map;
  for (int i = 0; i < P; ++i) {
    map[i] = first[i];
    map[n_cu + i] = second[i];
  }
  for (int i = 0; i < n_cu - P; ++i) map[P + i] = sorted_single[i];
  return map;
}

// ---- The sweep path of a handle, decided once at create: plan_sweep, a function of numbers (no HIP
// call, no environment), so that it can be read and tested (clv_debug_sweep_plan) without a GPU. ----

// The environment's knobs, read in one place.
struct SweepEnv {
  int persistent = -1;  // CLV_PERSISTENT: 0 never, 1 whenever the grid fits (tests, A/B), else -1: where it pays
  int layout = 0;       // CLV_PERSIST_LAYOUT: 0 unset, LAYOUT_BLOCK, LAYOUT_SPLIT (tests, A/B), -1 anything else
  int relay = -1;       // CLV_SPLIT_RELAY: -1 unset, 0 the helpers, 1 the relay (tests, A/B), 2 anything else
  bool defer = true;    // CLV_DEFER=0: every launch draws its last level-2 draw
  int mail_first = 0;   // CLV_MAIL_ALLOC = uncached | fine | default: the first memory kind tried for the mail
  double wait_ms = 0.0;  // CLV_WAIT_TIMEOUT_MS (clamped to [1 ms, 1 h]); 0 unset, -1 not a finite decimal number
};

SweepEnv read_sweep_env() {
  const auto is = [](const char* v, const char* text) { return v && !std::strcmp(v, text); };
  SweepEnv e;
  const char* v = std::getenv("CLV_PERSISTENT");
  e.persistent = is(v, "0") ? 0 : is(v, "1") ? 1 : -1;
  v = std::getenv("CLV_PERSIST_LAYOUT");
  e.layout = !v ? 0 : is(v, "block") ? LAYOUT_BLOCK : is(v, "split") ? LAYOUT_SPLIT : -1;
  v = std::getenv("CLV_SPLIT_RELAY");
  e.relay = !v ? -1 : is(v, "0") ? 0 : is(v, "1") ? 1 : 2;
  e.defer = !is(std::getenv("CLV_DEFER"), "0");
  v = std::getenv("CLV_MAIL_ALLOC");
  e.mail_first = is(v, "fine") ? 1 : is(v, "default") ? 2 : 0;
  v = std::getenv("CLV_WAIT_TIMEOUT_MS");
  if (v && !parse_wait_ms(v, &e.wait_ms)) e.wait_ms = -1.0;
  return e;
}

// What the runtime reports of a kernel instance: workgroups per CU and scratch (spill) bytes per lane;
// scratch < 0: not asked yet (plan_sweep says when it needs it), or the query failed (never capable).
constexpr int64_t NOT_QUERIED = -2, QUERY_FAILED = -1;
struct Instance { int bpc = 0; int64_t scratch = NOT_QUERIED; };
struct SweepResources {
  int n_cu = 0;                  // 0: a query of the block instance failed
  Instance block, split, relay;  // persist_kernel (peer variant at world size > 1); persist_kernel_split: helpers, relay
};
struct SweepPlan {
  bool persistent = false, split = false, p2p_capable = false, p2p_persist_fits = false, fx_capable = false, defer = false;
  int relay_steps = 0;
  bool need_split = false, need_relay = false;  // undecided until this instance's resources are known
  const char* error = nullptr;                  // a rejected knob on a path that reads it (CLV_EINVAL)
};

// A shard whose persistent grid the kernels can run at all (every workgroup resident at once: the chain
// hand-off spins on the others); with peers also the exchange's bounds: ranks, units, this rank's partials in UMAIL.
bool persist_shape(const Geometry& g, bool replay) {
  if (replay || g.nb_local <= 0 || g.nb_local > 2 * BLOCK) return false;
  if (g.world_size == 1) return g.blocks_per_unit == 1;
  const int bpu = g.blocks_per_unit;
  return g.world_size <= MAX_WORLD && g.n_units_global <= 2 * BLOCK && bpu <= 64 &&
         (int64_t)g.stride * ((g.nb_local + bpu - 1) / bpu) <= UMAIL;
}

// A world whose last rank (and maybe more) has no customers: shard r is [r * blocks_per_rank * BLOCK, ...)
// of n_global, so distributed.plan gives one whenever the ranks' blocks overshoot by a rank or more
// (2,357 customers on 8 ranks: ranks 5-7).  An empty shard has no resident grid; it takes the fused
// exchange, and so does every rank of its world — each decides from the plan alone, so all decide alike.
bool world_has_empty_shard(int64_t n_global, int world, int blocks_per_rank) {
  return world > 1 && (int64_t)(world - 1) * blocks_per_rank * BLOCK >= n_global;
}

// The two rules the CPU tests pin through clv_debug_persist_choice / clv_debug_split_choice.
bool persist_grid_chosen(int D, int K, int n_chains, int64_t grid_wgs, int blocks_per_cu, int n_cu, bool force) {
  return persist_grid_fits(grid_wgs, blocks_per_cu, n_cu) && (force || persist_worth(D, K, n_chains, grid_wgs, n_cu));
}
bool split_chosen(int n_chains, int nb, int blocks_per_cu, int n_cu, bool force) {
  return persist_split_fits(n_chains, nb, blocks_per_cu, n_cu) && (force || persist_split_pays(n_chains, nb, n_cu));
}

SweepPlan plan_sweep(const Geometry& g, bool replay, const SweepResources& r, const SweepEnv& e) {
  SweepPlan p;
  const int C = g.n_chains, nb = g.nb_local;
  // Persistent sweeps (one launch runs many sweeps) where the grid fits at once, here and (peers: the caller
  // checks) on every rank; an instance spilling more than PERSIST_SCRATCH_MAX bytes per lane only when forced.
  const bool force = e.persistent == 1;
  const bool resident = persist_shape(g, replay) && e.persistent != 0 &&
                        (force || (r.block.scratch >= 0 && r.block.scratch <= (int64_t)PERSIST_SCRATCH_MAX)) &&
                        persist_grid_chosen(g.D, g.K, C, (int64_t)(nb + 1) * C, r.block.bpc, r.n_cu, force);
  if (g.world_size == 1) p.persistent = resident;
  else p.p2p_capable = p.p2p_persist_fits = resident;
  // Any other shard with peers: the sweep kernel's fused level-2 tail exchanges through the same mail
  // (one launch per sweep, no host collective; n_units_global <= 2 CLV_BLOCK as its readers assume)
  p.fx_capable = !replay && g.world_size > 1 && g.world_size <= MAX_WORLD && g.n_units_global <= 2 * BLOCK;
  p.defer = p.persistent && e.defer;
  // Layout: split (persist_kernel_split: 6 customer + 2 helper wavefronts per CU) for bivariate models whose
  // sweep's variates fit the pool, where its grid is resident whole with 0 B of scratch and the block layout
  // would double up; forced, still only where it can run.  The layout knobs are read on this branch only.
  if (!(p.persistent && g.D == 2 && g.S <= PRE_STEPS && nb <= SPLIT_MAX_NB)) return p;
  if (e.layout < 0) p.error = "CLV_PERSIST_LAYOUT must be block or split";
  else if (e.relay > 1) p.error = "CLV_SPLIT_RELAY must be 0 or 1";
  if (p.error || e.layout == LAYOUT_BLOCK) return p;
  if (r.split.scratch == NOT_QUERIED) {
    p.need_split = true;
    return p;
  }
  p.split = r.split.scratch == 0 && split_chosen(C, nb, r.split.bpc, r.n_cu, e.layout == LAYOUT_SPLIT);
  // The relay instance (wavefronts 6 and 7 finish rows 4 and 5 from MH step SPLIT_RELAY_STEPS on) where the
  // sweep has more steps than that and the instance has 0 B of scratch and fits; forced, only where it can run.
  if (p.split && SPLIT_RELAY_STEPS > 0 && g.S > SPLIT_RELAY_STEPS && (e.relay < 0 ? SPLIT_RELAY_DEFAULT : e.relay == 1)) {
    if (r.relay.scratch == NOT_QUERIED) p.need_relay = true;
    else if (r.relay.scratch == 0 && persist_split_fits(C, nb, r.relay.bpc, r.n_cu)) p.relay_steps = SPLIT_RELAY_STEPS;
  }
  return p;
}

// ---- clv_create's steps.  Each returns its code; clv_create destroys the half-built handle. ----

int validate_and_derive(const clv_config* cfg, const clv_data* data, const clv_prior* prior, clv_sampler** out) {
  if (cfg->abi_version != CLV_ABI_VERSION) return fail(CLV_EINVAL, "ABI version mismatch");
  if (cfg->D != 2 && cfg->D != 3) return fail(CLV_EINVAL, "D must be 2 or 3");
  if (cfg->K < 1 || cfg->K > CLV_MAX_K) return fail(CLV_EINVAL, "K must be in 1..9");
  if (cfg->n_mh_steps < 0) return fail(CLV_EINVAL, "n_mh_steps must be >= 0");
  if (cfg->thin < 1) return fail(CLV_EINVAL, "thin must be >= 1");
  if (cfg->burnin < 0 || cfg->mcmc < 0) return fail(CLV_EINVAL, "burnin/mcmc must be >= 0");
  if (cfg->n_chains < 1) return fail(CLV_EINVAL, "n_chains must be >= 1");
  if (cfg->rng_mode != CLV_RNG_PHILOX && cfg->rng_mode != CLV_RNG_REPLAY) return fail(CLV_EINVAL, "bad rng_mode");
  if (cfg->draw_sink < CLV_SINK_FULL || cfg->draw_sink > CLV_SINK_SUMMARY_PCT) return fail(CLV_EINVAL, "bad draw_sink");
  if (data->n < 0) return fail(CLV_EINVAL, "n must be >= 0");
  if (cfg->n_global > 0xffffffffLL) return fail(CLV_EINVAL, "n_global must fit the 32-bit Philox customer counter");
  if (cfg->n_global < data->n || cfg->n_global < 1) return fail(CLV_EINVAL, "n_global must be >= n >= 0 and > 0");
  if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) return fail(CLV_EINVAL, "bad rank/world_size");
  if (cfg->D == 3 && data->n > 0 && !data->log_s) return fail(CLV_EINVAL, "D == 3 needs log_s");
  if (cfg->K > 1 && data->n > 0 && !data->covariates) return fail(CLV_EINVAL, "K > 1 needs covariates");
  if (data->n > 0 && (!data->x || !data->t_x || !data->T_cal)) return fail(CLV_EINVAL, "missing CBS column");
  if (cfg->rng_mode == CLV_RNG_REPLAY && cfg->world_size != 1) return fail(CLV_EINVAL, "replay needs world_size 1");

  const int32_t bpu = cfg->blocks_per_unit ? cfg->blocks_per_unit : clv_default_blocks_per_unit(cfg->n_global);
  if (!is_pow2(bpu)) return fail(CLV_EINVAL, "blocks_per_unit must be a power of two");
  const int nb_local = (int)((data->n + BLOCK - 1) / BLOCK);
  int32_t bpr = cfg->blocks_per_rank;
  if (bpr == 0) {
    if (cfg->world_size != 1) return fail(CLV_EINVAL, "blocks_per_rank required when sharded");
    bpr = ((std::max(nb_local, 1) + bpu - 1) / bpu) * bpu;
  }
  if (bpr % bpu) return fail(CLV_EINVAL, "blocks_per_rank must be a multiple of blocks_per_unit");
  if (nb_local > bpr) return fail(CLV_EINVAL, "shard larger than blocks_per_rank * CLV_BLOCK");
  if (cfg->shard_begin != (int64_t)cfg->rank * bpr * BLOCK) return fail(CLV_EINVAL, "shard_begin != rank * blocks_per_rank * CLV_BLOCK");
  const int64_t nb_global = (cfg->n_global + BLOCK - 1) / BLOCK;
  if ((int64_t)bpr * cfg->world_size < nb_global) return fail(CLV_EINVAL, "shards do not cover n_global");

  auto* s = new clv_sampler();
  s->cfg = *cfg;
  s->cfg.blocks_per_rank = bpr;
  s->cfg.blocks_per_unit = bpu;
  s->prior = *prior;
  s->replay = cfg->rng_mode == CLV_RNG_REPLAY;

  Geometry& g = s->g;
  g.D = cfg->D;
  g.K = cfg->K;
  g.S = cfg->n_mh_steps;
  g.n_chains = cfg->n_chains;
  g.n = data->n;
  g.n_global = cfg->n_global;
  g.shard_begin = cfg->shard_begin;
  g.nb_local = nb_local;
  g.blocks_per_rank = bpr;
  g.blocks_per_unit = bpu;
  g.units_per_rank = bpr / bpu;
  g.n_units_global = (nb_global + bpu - 1) / bpu;
  g.world_size = cfg->world_size;
  g.stride = cfg->K * cfg->D + cfg->D * (cfg->D + 1) / 2 + 1;
  g.burnin = cfg->burnin;
  g.mcmc = cfg->mcmc;
  g.thin = cfg->thin;
  g.n_draws = cfg->mcmc >= 1 ? (cfg->mcmc - 1) / cfg->thin + 1 : 0;
  g.l2w = cfg->D * cfg->K + cfg->D * (cfg->D + 1) / 2;
  *out = s;
  return CLV_OK;
}

int open_device_and_stream(clv_sampler* s) {
  if (s->cfg.device >= 0) CLV_HIP(hipSetDevice(s->cfg.device));
  CLV_HIP(hipGetDevice(&s->device));
  if (s->cfg.stream) {
    s->stream = (hipStream_t)(uintptr_t)s->cfg.stream;
  } else {
    CLV_HIP(hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking));
    s->stream = s->own;
  }
  return CLV_OK;
}

// One instance's resources for plan_sweep.  A failed query is "never capable", not an error.
Instance query_split_instance(const Geometry& g, bool relay) {
  Instance in;
  size_t scratch = 0;
  const bool ok = persist_split_resources(g.D, g.K, &in.bpc, &scratch, relay) == hipSuccess;
  if (!ok) (void)hipGetLastError();
  in.scratch = ok ? (int64_t)scratch : QUERY_FAILED;
  return in;
}

// Ask the runtime for the resources the plan depends on — each instance only where plan_sweep reaches
// the question — and record the plan in the handle.
int decide_sweep_path(clv_sampler* s, const SweepEnv& env) {
  const Geometry& g = s->g;
  SweepResources r;
  if (persist_shape(g, s->replay)) {
    hipDeviceProp_t prop{};
    size_t scratch = 0;
    r.block.scratch = QUERY_FAILED;
    if (persist_occupancy(g.D, g.K, g.world_size > 1, &r.block.bpc) == hipSuccess &&
        persist_scratch_bytes(g.D, g.K, g.world_size > 1, &scratch) == hipSuccess &&
        hipGetDeviceProperties(&prop, s->device) == hipSuccess) {
      r.block.scratch = (int64_t)scratch;
      r.n_cu = prop.multiProcessorCount;
    }
    s->persist_bpc = r.block.bpc;
    s->n_cu = r.n_cu;
  }
  SweepPlan p = plan_sweep(g, s->replay, r, env);
  if (p.need_split) {
    r.split = query_split_instance(g, false);
    p = plan_sweep(g, s->replay, r, env);
  }
  if (p.need_relay) {  // (the relay question follows the split answer)
    r.relay = query_split_instance(g, true);
    p = plan_sweep(g, s->replay, r, env);
  }
  if (p.error) return fail(CLV_EINVAL, p.error);
  if (world_has_empty_shard(g.n_global, g.world_size, g.blocks_per_rank)) p.p2p_capable = p.p2p_persist_fits = false;
  s->persistent = p.persistent;
  s->split = p.split;
  s->relay_steps = p.relay_steps;
  s->p2p_capable = p.p2p_capable;
  s->p2p_persist_fits = p.p2p_persist_fits;
  s->fx_capable = p.fx_capable;
  s->defer = p.defer;
  if (s->persistent || s->p2p_capable || s->fx_capable) {
    // every wait of the persistent kernel is bounded: 2 s at world size 1 (all workgroups are resident, so a wait
    // that long means a fault), 10 s with peers (host-side launch skew between ranks); CLV_WAIT_TIMEOUT_MS overrides
    if (env.wait_ms < 0) return fail(CLV_EINVAL, "CLV_WAIT_TIMEOUT_MS must be a finite decimal number of ms");
    const double ms = env.wait_ms > 0 ? env.wait_ms : g.world_size > 1 ? 10000.0 : 2000.0;
    s->wait_ticks = (uint64_t)(ms * 1e5);  // s_memrealtime: 100 MHz
  }
  return CLV_OK;
}

void forget_peers(clv_sampler* s) {  // not connected; the peers' IPC mappings closed
  s->p2p_ready = false;
  for (void* p : s->ipc_opened) (void)hipIpcCloseMemHandle(p);
  s->ipc_opened.clear();
}

// every slot of the peer mail empty (all-ones bytes: the sentinel NaN)
hipError_t fill_mail(clv_sampler* s) {
  return hipMemsetAsync(s->d_mail, 0xFF, sizeof(double) * mail_count(s->g), s->stream);
}

// Every buffer of the handle, the clears queued on the stream (before the uploads and the initial
// sweep: stream order).  The order among the clears is incidental.
int allocate_and_clear(clv_sampler* s, const SweepEnv& env) {
  const Geometry& g = s->g;
  const hipStream_t st = s->stream;
  const size_t C = g.n_chains, n1 = std::max<int64_t>(g.n, 1);  // (no empty allocation for an empty shard)
  const bool summary = (s->cfg.draw_sink == CLV_SINK_SUMMARY || s->cfg.draw_sink == CLV_SINK_SUMMARY_PCT) && g.n > 0;
  CLV_HIP(s->d_x.alloc(n1));
  for (auto* b : {&s->d_tx, &s->d_T}) CLV_HIP(b->alloc(n1));
  if (g.K > 1) CLV_HIP(s->d_cov.alloc((g.K - 1) * n1));
  if (g.D == 3) CLV_HIP(s->d_logs.alloc(n1));
  CLV_HIP(s->d_clk.alloc(2 * CLK_RING, 0, st));
  for (auto* b : {&s->d_lam, &s->d_mu}) CLV_HIP(b->alloc(state_count(g)));
  CLV_HIP(s->d_hyper.alloc(hyper_count(g), 0, st));
  CLV_HIP(s->d_block.alloc(C * g.blocks_per_rank * g.stride, 0, st));
  if (g.blocks_per_unit > 1) CLV_HIP(s->d_unit_own.alloc(unit_count(g), 0, st));
  s->d_unit = g.blocks_per_unit > 1 ? s->d_unit_own : s->d_block;
  CLV_HIP(s->d_prior.alloc(PRIOR_DOUBLES));
  CLV_HIP(s->d_ctrl.alloc(1, 0, st));
  CLV_HIP(s->d_arrive.alloc(arrive_count(g), 0, st));
  CLV_HIP(s->d_hvar.alloc(2 * C * HV, 0, st));
  CLV_HIP(s->d_hyp2.alloc(handoff_count(g)));
  if (s->p2p_capable || s->fx_capable) {
    // The mail is written by OTHER GPUs (system-scope write-through stores over xGMI) while this GPU polls it.
    // Uncached device memory (MTYPE UC: every access of every agent goes to memory, no L2 line of this GPU can
    // hold a stale copy of a peer's store); fine-grained, then plain device memory if the allocator refuses
    const unsigned flags[3] = {hipDeviceMallocUncached, hipDeviceMallocFinegrained, hipDeviceMallocDefault};
    for (int k = env.mail_first; k < 3 && !s->d_mail; ++k) {
      void* p = nullptr;
      if (hipExtMallocWithFlags(&p, sizeof(double) * mail_count(g), flags[k]) == hipSuccess && p) {
        s->d_mail.reset((double*)p);
        s->mail_kind = k;
      } else {
        (void)hipGetLastError();
      }
    }
    if (!s->d_mail) return fail(CLV_ENOMEM, "peer mail buffer");
    CLV_HIP(fill_mail(s));
    CLV_HIP(s->d_peers.alloc(g.world_size));
  }
  if (s->persistent || s->p2p_capable || s->fx_capable) {  // (fused exchange: the snapshot buffers)
    CLV_HIP(s->d_pblock.alloc(pblock_count(g)));
    if (s->defer) CLV_HIP(s->d_pend.alloc(2 * C * g.stride));
    for (auto* b : {&s->d_lam_alt, &s->d_mu_alt}) CLV_HIP(b->alloc(state_count(g)));
    CLV_HIP(s->d_hyper_alt.alloc(hyper_count(g)));
    if (summary) CLV_HIP(s->d_sums_prev.alloc(sums_count(g)));
    CLV_HIP(s->d_diag.alloc(DIAG_WORDS, 0, st));
    CLV_HIP(hipHostMalloc((void**)&s->h_abort, sizeof(uint32_t), hipHostMallocMapped));
    *s->h_abort = 0;
    CLV_HIP(hipHostGetDevicePointer((void**)&s->d_h_abort, s->h_abort, 0));
  }
  if ((s->persistent || s->p2p_capable) && s->n_cu > 0) {
    // same-chain pairs on shared CUs, bivariate and trivariate: with the MH-phase wave priority
    // (kernels.hip persist_kernel) measured c2 10.70 -> 9.58 us per sweep against no map, c3 11.45 ->
    // 11.1 (chain pairs c / c + 2 instead: c2 10.16, c3 11.1; profiles/r05_ab_priority.txt)
    const std::vector<int32_t> map = persist_wg_map((int)C, g.nb_local, s->n_cu);
    CLV_HIP(s->d_wgmap.upload(map.data(), map.size()));
    if (s->split) {
      const std::vector<int32_t> smap = persist_split_layout((int)C, g.nb_local);
      CLV_HIP(s->d_wgmap_split.upload(smap.data(), smap.size()));
    }
  }
#ifdef CLV_STAMPS
  {
    // (+ 16 words per workgroup: the split layout's relay stamps and SIMD ids, clv_debug_split_stamps)
    std::vector<unsigned long long> stamps(1024 * 8 + (12 + 16) * C * (std::max(g.nb_local, 1) + 1), 0ull);
    for (int i = 0; i < 1024; ++i) stamps[i * 8 + 0] = stamps[i * 8 + 4] = ~0ull;
    CLV_HIP(s->d_stamps.upload(stamps.data(), stamps.size()));
  }
#endif
  CLV_HIP(s->d_bs.alloc(C * (CLV_MAX_K * CLV_MAX_D + CLV_MAX_D * CLV_MAX_D)));
  if (g.n_draws > 0) {
    CLV_HIP(s->d_level2.alloc(loglik_count(g) * g.l2w, 0, st));
    CLV_HIP(s->d_loglik.alloc(loglik_count(g), 0, st));
    if (s->cfg.draw_sink == CLV_SINK_FULL) CLV_HIP(s->d_level1.alloc(level1_count(g), 0, st));
  }
  if (summary) CLV_HIP(s->d_sums.alloc(sums_count(g), 0, st));
  if (s->cfg.draw_sink == CLV_SINK_SUMMARY_PCT) {
    const size_t nq = loglik_count(g) * g.n;  // a (lambda, mu) pair per stored draw and customer
    if (s->d_qstore.alloc(nq) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CLV_ENOMEM, "percentile store: " + std::to_string(sizeof(float2) * nq) +
                                  " bytes of device memory not available");
    }
    if (nq) CLV_HIP(hipMemsetAsync(s->d_qstore, 0, sizeof(float2) * nq, st));
  }
  return CLV_OK;
}

int upload_data_and_prior(clv_sampler* s, const clv_data* data, const clv_prior* prior) {
  const Geometry& g = s->g;
  const hipStream_t st = s->stream;
  const size_t n = g.n;
  if (n > 0) {
    CLV_HIP(hipMemcpyAsync(s->d_x, data->x, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    CLV_HIP(hipMemcpyAsync(s->d_tx, data->t_x, sizeof(double) * n, hipMemcpyHostToDevice, st));
    CLV_HIP(hipMemcpyAsync(s->d_T, data->T_cal, sizeof(double) * n, hipMemcpyHostToDevice, st));
    if (g.K > 1) CLV_HIP(hipMemcpyAsync(s->d_cov, data->covariates, sizeof(double) * (g.K - 1) * n, hipMemcpyHostToDevice, st));
    if (g.D == 3) CLV_HIP(hipMemcpyAsync(s->d_logs, data->log_s, sizeof(double) * n, hipMemcpyHostToDevice, st));
  }
  const std::vector<double> pr = pack_prior(prior, g.D, g.K);
  CLV_HIP(hipMemcpyAsync(s->d_prior, pr.data(), sizeof(double) * pr.size(), hipMemcpyHostToDevice, st));
  // needed: the copies read pageable host memory (pr, the caller's arrays) that must outlive them
  CLV_HIP(hipStreamSynchronize(st));
  return CLV_OK;
}

// Initial state (bi:367-379, tri:488-504) and, for D == 2, the statistics of the first draw.  In
// stream order behind the clears and the uploads; the group kernel reads the sweep's block partials.
int initial_state(clv_sampler* s) {
  const Geometry& g = s->g;
  if (g.n > 0) {
    CLV_HIP(launch_sweep(sweep_args(s, 1), false, s->stream));
    if (int rc = enqueue_group(s)) return rc;
  }
  std::vector<double> bs;
  if (g.D == 3) {
    const int w = g.K * g.D + g.D * g.D;
    bs.resize((size_t)g.n_chains * w);
    for (int c = 0; c < g.n_chains; ++c) {
      double* o = bs.data() + (size_t)c * w;
      for (int i = 0; i < g.K * g.D; ++i) o[i] = s->prior.beta_init[i];
      for (int i = 0; i < g.D * g.D; ++i) o[g.K * g.D + i] = s->prior.sigma_init[i];
    }
    CLV_HIP(hipMemcpyAsync(s->d_bs, bs.data(), sizeof(double) * bs.size(), hipMemcpyHostToDevice, s->stream));
    CLV_HIP(launch_set_hyper(g.D, g.K, g.n_chains, s->d_hyper, s->d_bs, s->prior.omega2, s->replay, s->stream));
  } else {
    s->pending_init_hyper = true;
  }
  // needed: bs must outlive its copy, and the caller may use the handle from another stream at once
  CLV_HIP(hipStreamSynchronize(s->stream));
  return CLV_OK;
}

}  // namespace

extern "C" {

int clv_create(const clv_config* cfg, const clv_data* data, const clv_prior* prior, clv_sampler** out) {
  if (!cfg || !data || !prior || !out) return fail(CLV_EINVAL, "null argument");
  *out = nullptr;
  clv_sampler* s = nullptr;
  int rc = validate_and_derive(cfg, data, prior, &s);
  if (rc) return rc;
  const SweepEnv env = read_sweep_env();
  rc = open_device_and_stream(s);
  if (!rc) rc = decide_sweep_path(s, env);
  if (!rc) rc = allocate_and_clear(s, env);
  if (!rc) rc = upload_data_and_prior(s, data, prior);
  if (!rc) rc = initial_state(s);
  if (rc) {
    clv_destroy(s);  // (owning members: whatever the steps had allocated)
    return rc;
  }
  *out = s;
  return CLV_OK;
}

void clv_destroy(clv_sampler* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);  // current while the members below free their memory
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->ds) {  // no copy may still read the draws freed below
    stream_wait(s->ds);
    delete s->ds;
  }
  if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
  for (auto e : s->ev) (void)hipEventDestroy(e);
  if (s->done_ev) (void)hipEventDestroy(s->done_ev);
  if (s->poll_stream) (void)hipStreamDestroy(s->poll_stream);
  if (s->h_abort) (void)hipHostFree(s->h_abort);
  forget_peers(s);  // before this rank's mail goes
  const hipStream_t own = s->own;
  delete s;  // every device buffer (the DevPtr members)
  if (own) (void)hipStreamDestroy(own);  // last
}

int clv_set_replay_tape(clv_sampler* s, const double* tape, int64_t n_sweeps) {
  if (!s || !tape || n_sweeps < 1) return fail(CLV_EINVAL, "bad replay tape arguments");
  if (!s->replay) return fail(CLV_ESTATE, "sampler not created in replay mode");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(s->d_tape.upload(tape, (size_t)s->g.n_chains * n_sweeps * clv_replay_sweep_stride(s)));
  s->tape_sweeps = n_sweeps;
  return drop_graph(s);
}

int clv_hyper(clv_sampler* s, const double* gathered) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (s->g.world_size > 1 && !gathered) return fail(CLV_EINVAL, "sharded hyper needs the gathered buffer");
  CLV_HIP(hipSetDevice(s->device));
  {
    int rc = persist_flush(s);
    if (rc) return rc;
  }
  if (s->pending_init_hyper) {
    int rc = check_replay_range(s, 0);
    if (rc) return rc;
    rc = enqueue_hyper(s, gathered, 1, nullptr, nullptr);
    if (rc) return rc;
    s->pending_init_hyper = false;
    return CLV_OK;
  }
  return enqueue_hyper(s, gathered, 0, nullptr, nullptr);
}

int clv_sweep(clv_sampler* s) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (s->pending_init_hyper) return fail(CLV_ESTATE, "bivariate: call clv_hyper once before the first sweep");
  CLV_HIP(hipSetDevice(s->device));
  int rc = persist_flush(s);
  if (rc) return rc;
  rc = check_replay_range(s, 1);
  if (rc) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (s->timing) {
    rc = ensure_events(s);
    if (rc) return rc;
    e0 = s->ev[4 * s->ev_used];
    e1 = s->ev[4 * s->ev_used + 1];
  }
  rc = enqueue_sweep(s, e0, e1);
  if (rc) return rc;
  if (s->timing && ++s->ev_used == TIMING_EVENTS) {
    rc = harvest_timing(s);
    if (rc) return rc;
  }
  s->sweeps_done++;
  return CLV_OK;
}

int clv_partials(clv_sampler* s, double** ptr, int64_t* n_doubles, int32_t* stride) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (ptr) *ptr = s->d_unit;
  if (n_doubles) *n_doubles = (int64_t)unit_count(s->g);
  if (stride) *stride = s->g.stride;
  return CLV_OK;
}

int clv_copy_partials(clv_sampler* s, void* dst) {
  if (!s || !dst) return fail(CLV_EINVAL, "null argument");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipMemcpyAsync(dst, s->d_unit, sizeof(double) * unit_count(s->g), hipMemcpyDeviceToDevice, s->stream));
  return CLV_OK;
}

int clv_synchronize(clv_sampler* s) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  return CLV_OK;
}

int64_t clv_sweeps_done(const clv_sampler* s) { return s ? s->sweeps_done : -1; }

int clv_clock_ghz(clv_sampler* s, double* ghz) {
  if (!s || !ghz) return fail(CLV_EINVAL, "null argument");
  *ghz = 0.0;
  // the last clv_run's sweeps [first, end]: each slot is one workgroup's (delta s_memtime, delta
  // s_memrealtime) up to that sweep's publish; the last sweep's draw may be deferred (persistent
  // kernel), so it is left out; at most the last CLK_RING sweeps are kept
  const int64_t end = s->sweeps_done - 1;
  const int64_t first = std::max<int64_t>(s->clk_first, end - (CLK_RING - 1));
  if (!s->d_clk || s->clk_first < 1 || end < first) return CLV_OK;
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  std::vector<unsigned long long> ring(2 * CLK_RING);
  CLV_HIP(hipMemcpy(ring.data(), s->d_clk, sizeof(unsigned long long) * ring.size(), hipMemcpyDeviceToHost));
  double dm = 0.0, dr = 0.0;
  for (int64_t q = first; q <= end; ++q) {
    dm += (double)ring[2 * (q % CLK_RING)];
    dr += (double)ring[2 * (q % CLK_RING) + 1];
  }
  if (dr > 0.0) *ghz = 0.1 * dm / dr;  // s_memrealtime: 100 MHz
  return CLV_OK;
}

int clv_launch_info(const clv_sampler* s, int64_t* out) {
  if (!s || !out) return fail(CLV_EINVAL, "null argument");
  out[0] = s->persistent ? 1 : 0;
  out[1] = s->persist_bpc;
  out[2] = s->n_cu;
  out[3] = (int64_t)(s->g.nb_local + (s->persistent ? 1 : 0)) * s->g.n_chains;
  // out[3] counts logical workgroups (one per block, + the level-2 one) in either layout; the
  // workgroups actually dispatched and the layout (LAYOUT_*; -LAYOUT_BLOCK: block after a split
  // launch aborted)
  out[4] = s->split ? (int64_t)(split_wgs(s->g.nb_local) + 1) * s->g.n_chains : out[3];
  out[5] = !s->persistent ? LAYOUT_NONE : s->split ? LAYOUT_SPLIT : s->split_reverted ? -LAYOUT_BLOCK : LAYOUT_BLOCK;
  return CLV_OK;
}

int clv_split_relay_steps(const clv_sampler* s, int32_t* out) {
  if (!s || !out) return fail(CLV_EINVAL, "null argument");
  *out = s->split ? s->relay_steps : 0;
  return CLV_OK;
}

int clv_p2p_info(const clv_sampler* s, int64_t* out) {
  if (!s || !out) return fail(CLV_EINVAL, "null argument");
  out[0] = (s->p2p_capable || s->fx_capable) ? 1 : 0;
  out[4] = s->p2p_capable ? 1 : 0;
  out[1] = s->p2p_ready ? 1 : 0;
  out[2] = s->d_mail ? (int64_t)sizeof(double) * 2 * s->g.world_size * s->g.n_chains * s->g.stride * s->g.units_per_rank : 0;
  out[3] = (int64_t)(uintptr_t)s->d_mail.p;
  out[5] = s->d_mail ? s->mail_kind : -1;
  return CLV_OK;
}

int clv_p2p_export(clv_sampler* s, void* handle) {
  if (!s || !handle) return fail(CLV_EINVAL, "null argument");
  if (!s->p2p_capable && !s->fx_capable) return fail(CLV_ESTATE, "no peer exchange for this sampler (world size 1 or replay mode)");
  CLV_HIP(hipSetDevice(s->device));
  hipIpcMemHandle_t h;
  CLV_HIP(hipIpcGetMemHandle(&h, s->d_mail));
  std::memcpy(handle, &h, sizeof(h));
  return CLV_OK;
}

int clv_p2p_connect(clv_sampler* s, const void* handles, const uint64_t* ptrs) {
  if (!s || (!handles && !ptrs)) return fail(CLV_EINVAL, "null argument");
  if (!s->p2p_capable && !s->fx_capable) return fail(CLV_ESTATE, "no peer exchange for this sampler (world size 1 or replay mode)");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  forget_peers(s);  // reconnect (after a failed step): drop the old mappings
  // every slot of this rank's mail empty (a failed step may have left units of any rank there);
  // the caller synchronises the ranks after connecting, before any rank runs
  CLV_HIP(fill_mail(s));
  const int W = s->g.world_size, r = s->cfg.rank;
  std::vector<double*> peers(W, nullptr);
  for (int q = 0; q < W; ++q) {
    if (q == r) {
      peers[q] = s->d_mail;
    } else if (handles) {
      hipIpcMemHandle_t h;
      std::memcpy(&h, (const char*)handles + (size_t)q * sizeof(h), sizeof(h));
      void* p = nullptr;
      CLV_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
      s->ipc_opened.push_back(p);
      peers[q] = (double*)p;
    } else {
      peers[q] = (double*)(uintptr_t)ptrs[q];
    }
    if (!peers[q]) return fail(CLV_EINVAL, "null peer mail pointer");
  }
  CLV_HIP(hipMemcpy(s->d_peers, peers.data(), sizeof(double*) * W, hipMemcpyHostToDevice));
  CLV_HIP(hipStreamSynchronize(s->stream));  // the mail's sentinel fill has landed
  s->p2p_ready = true;
  s->fx_epoch = s->sweeps_done;
  return CLV_OK;
}

int clv_p2p_set_persistent(clv_sampler* s, int32_t on) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (on && !s->p2p_persist_fits) return fail(CLV_ESTATE, "the persistent peer exchange does not fit this shard's grid");
  if (!on && !s->fx_capable) return fail(CLV_ESTATE, "no fused peer exchange for this sampler");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  s->p2p_capable = on != 0;
  s->last_persist_n = 0;  // (a rollback undoes a call of the path that ran it)
  return CLV_OK;
}

int clv_p2p_disconnect(clv_sampler* s) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  forget_peers(s);
  if (s->d_peers) CLV_HIP(hipMemset(s->d_peers, 0, sizeof(double*) * s->g.world_size));
  return CLV_OK;
}

int clv_set_wait_timeout(clv_sampler* s, double ms) {
  if (!s || !(ms >= 1.0) || ms > 3.6e6) return fail(CLV_EINVAL, "wait timeout must be in [1 ms, 1 h]");
  s->wait_ticks = (uint64_t)(ms * 1e5);  // s_memrealtime: 100 MHz
  return drop_graph(s);  // captured with the previous bound (kernel arguments)
}

int clv_set_stream(clv_sampler* s, uint64_t stream) {
  if (!s || !stream) return fail(CLV_EINVAL, "bad arguments");
  if (int rc = drop_graph(s)) return rc;  // captured on the previous stream
  s->stream = (hipStream_t)(uintptr_t)stream;  // caller-owned from now on
  return CLV_OK;
}

int clv_note_sweeps(clv_sampler* s, int64_t n) {
  if (!s || s->sweeps_done + n < 0) return fail(CLV_EINVAL, "bad arguments");
  s->sweeps_done += n;
  s->last_persist_n = 0;
  return CLV_OK;
}

}  // extern "C"

// What an aborted persistent launch, an aborted fused exchange and clv_rollback share of "back to before
// the launch" (lam / mu / hyper come back untouched, copied, swapped): Ctrl at s->sweeps_done, the saved sums.
static int rewind_ctrl_and_sums(clv_sampler* s) {
  Ctrl c{};
  c.cur = s->sweeps_done;
  CLV_HIP(hipMemcpy(s->d_ctrl, &c, sizeof(Ctrl), hipMemcpyHostToDevice));
  if (s->d_sums_prev)
    CLV_HIP(hipMemcpy(s->d_sums, s->d_sums_prev, sizeof(double) * sums_count(s->g), hipMemcpyDeviceToDevice));
  return CLV_OK;
}

// The sweep count is set back (clv_set_state, clv_rollback) with every rank's launches complete, so every mail
// slot is empty: wait_for_empty_ranks starts over from here, and the progress words of the sweeps now undone
// are cleared so that they cannot pass for the sweeps to come.  (The peers post again only after the caller
// has brought the ranks back in step, as after clv_p2p_connect.)
static int restart_fx_epoch(clv_sampler* s) {
  s->fx_epoch = s->sweeps_done;
  if (s->d_mail)
    CLV_HIP(hipMemset(s->d_mail + mail_slots(s->g.world_size, s->g.n_chains, s->g.stride, s->g.units_per_rank), 0xFF,
                      sizeof(double) * MAIL_TAIL));
  return CLV_OK;
}

// Persistent path: one launch of persist_kernel for all n sweeps (see kernels.hip), in two halves
// so that a group of shards in one process (group.hip) can have every shard's launch in flight
// before waiting for any.
static inline int64_t host_now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

int clv::persist_launch(clv_sampler* s, int64_t n_sweeps) {
  const Geometry& g = s->g;
  s->last_persist_n = 0;
  s->inflight_n = 0;
  if (n_sweeps == 0) return CLV_OK;
  if (s->slots_dirty) {  // a completed launch leaves every hand-off slot empty; else fill them
    // every hand-off slot empty (all-ones bytes: the sentinel NaN)
    CLV_HIP(hipMemsetAsync(s->d_hyp2, 0xFF, sizeof(double) * handoff_count(g), s->stream));
    CLV_HIP(hipMemsetAsync(s->d_pblock, 0xFF, sizeof(double) * pblock_count(g), s->stream));
    s->slots_dirty = false;
  }
  if (s->d_sums_prev)  // an aborted (or rolled-back) launch restores the running sums from here
    CLV_HIP(hipMemcpyAsync(s->d_sums_prev, s->d_sums, sizeof(double) * sums_count(g), hipMemcpyDeviceToDevice, s->stream));
  SweepArgs a = sweep_args(s, 0, 1);
  const int64_t stride_c = (int64_t)g.n_chains * g.stride;
  a.pend_in = s->pend ? s->d_pend + s->pend_buf * stride_c : nullptr;
  a.pend_out = s->defer ? s->d_pend + (s->pend_buf ^ 1) * stride_c : nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (s->timing) {
    int rc = ensure_events(s);
    if (rc) return rc;
    e0 = s->ev[4 * s->ev_used];
    e1 = s->ev[4 * s->ev_used + 1];
    if (s->ev_sweeps.size() < TIMING_EVENTS) s->ev_sweeps.assign(TIMING_EVENTS, 1);
    s->ev_sweeps[s->ev_used] = n_sweeps;
  }
  // timed launches: events recorded around the launch (measured 0.4-0.7 us per step less host cost
  // on the driver's 20-sweep run than the dispatch's own timestamps, same duration to 0.2%)
  if (e0) CLV_HIP(hipEventRecord(e0, s->stream));
  s->host_ns[2] = host_now_ns();
  if (s->split) {
    a.wg_map = s->d_wgmap_split;
    CLV_HIP(launch_persist_split(a, s->sweeps_done + 1, n_sweeps, s->stream, s->relay_steps > 0));
  } else {
    CLV_HIP(launch_persist(a, s->sweeps_done + 1, n_sweeps, s->stream, nullptr, nullptr));
  }
  s->host_ns[3] = host_now_ns();
  if (e1) CLV_HIP(hipEventRecord(e1, s->stream));
  // the launch's end event; timed launches are harvested later (clv_kernel_time or a full slot set)
  s->inflight_done = e1;
  if (s->timing) {
    if (++s->ev_used == TIMING_EVENTS) {
      int rc = harvest_timing(s);
      if (rc) return rc;
    }
  } else {
    if (!s->done_ev) CLV_HIP(hipEventCreateWithFlags(&s->done_ev, hipEventDisableTiming));
    CLV_HIP(hipEventRecord(s->done_ev, s->stream));
    s->inflight_done = s->done_ev;
  }
  s->inflight_n = n_sweeps;
  s->host_ns[4] = host_now_ns();
  return CLV_OK;
}

int clv::persist_wait(clv_sampler* s) {
  const int64_t n_sweeps = s->inflight_n;
  if (n_sweeps == 0) return CLV_OK;
  s->inflight_n = 0;
  const Geometry& g = s->g;
  // the host polls the launch's end event (stream synchronize / event synchronize measured within
  // 0.3 us per step of it, profiles/r04_host_variants.jsonl)
  const hipEvent_t done = s->inflight_done;
  if (!done) {
    CLV_HIP(hipStreamSynchronize(s->stream));
  } else {
    hipError_t q;
    while ((q = hipEventQuery(done)) == hipErrorNotReady) {
    }
    CLV_HIP(q);
  }
  s->host_ns[5] = host_now_ns();
  if (__atomic_load_n(s->h_abort, __ATOMIC_ACQUIRE)) {
    // the carried state was written to the *_alt buffers only: lam / mu / hyper still hold the
    // state this launch started from; restore the counters, flags and running sums
    *s->h_abort = 0;
    if (int rc = rewind_ctrl_and_sums(s)) return rc;
    s->slots_dirty = true;
    if (g.world_size > 1) s->p2p_ready = false;  // mail slots are in an unknown state now
    std::string diag = take_wait_diag(s);
    if (s->split) {  // its one-workgroup-per-CU grid was not resident whole (or a fault): the block
                     // layout, with its wider margin, for the rest of the handle's life
      s->split = false;
      s->relay_steps = 0;
      s->split_reverted = true;
      diag += "; the split layout's launch aborted: this handle uses the block layout from now on";
    }
    return fail(CLV_EHIP, std::string(g.world_size > 1
                                          ? "persistent sweep kernel: a wait timed out (a peer rank not running, or not all "
                                            "resident?); state unchanged"
                                          : "persistent sweep kernel: a workgroup timed out waiting for its chain (not all "
                                            "resident?); state unchanged") + diag);
  }
  s->d_lam.swap(s->d_lam_alt);
  s->d_mu.swap(s->d_mu_alt);
  s->rb_pend = s->pend;  // (rollback: the hyper state this launch started from)
  s->rb_pend_buf = s->pend_buf;
  s->rb_hyper_swaps = 0;
  if (s->defer) {  // the launch's last draw is pending in the other buffer; hyper untouched
    s->pend = true;
    s->pend_buf ^= 1;
  } else {
    s->d_hyper.swap(s->d_hyper_alt);
    s->rb_hyper_swaps = 1;
    s->pend = false;
  }
  if (int rc = drop_graph(s)) return rc;  // captured with the previous state pointers
  s->sweeps_done += n_sweeps;
  s->last_persist_n = n_sweeps;
  return CLV_OK;
}

// The pending level-2 draw of the last launch's last sweep (CLV_DEFER), into hyper (and the
// level-2 record it belongs to): before anything reads the hyper state or the level-2 records, or
// runs a sweep that is not a persistent launch.  The same draw (statistics, variates, order) the
// next launch would make first, so results do not depend on where a run is cut into clv_run calls.
int clv::persist_flush(clv_sampler* s) {
  if (!s->pend) return CLV_OK;
  CLV_HIP(hipSetDevice(s->device));
  SweepArgs a = sweep_args(s, 0, 1);
  a.pend_in = s->d_pend + s->pend_buf * (int64_t)s->g.n_chains * s->g.stride;
  a.pend_out = nullptr;
  CLV_HIP(launch_persist_flush(a, s->sweeps_done + 1, s->stream));
  CLV_HIP(hipStreamSynchronize(s->stream));
  s->d_hyper.swap(s->d_hyper_alt);
  s->rb_hyper_swaps++;
  s->pend = false;
  return drop_graph(s);
}

namespace {
int run_persistent(clv_sampler* s, int64_t n_sweeps) {
  int rc = persist_launch(s, n_sweeps);
  if (rc) return rc;
  return persist_wait(s);
}

// n launches of the fused sweep kernel (world size 1, or sharded with the fused peer exchange):
// hipGraph chunks, or (timing) one event pair per launch.  Not waited for.
int enqueue_fused_sweeps(clv_sampler* s, int64_t n_sweeps) {
  int rc = CLV_OK;
  int64_t left = n_sweeps;
  if (s->timing) {
    rc = ensure_events(s);
    if (rc) return rc;
    while (left > 0) {
      const int k = s->ev_used;
      rc = enqueue_fused(s, s->ev[4 * k], s->ev[4 * k + 1]);
      if (rc) return rc;
      s->ev_used++;
      s->sweeps_done++;
      left--;
      if (s->ev_used == TIMING_EVENTS) {
        rc = harvest_timing(s);
        if (rc) return rc;
      }
    }
    return harvest_timing(s);
  }
  if (left >= GRAPH_CHUNK) {
    rc = build_graph(s, GRAPH_CHUNK);
    if (rc) return rc;
    while (left >= GRAPH_CHUNK) {
      CLV_HIP(hipGraphLaunch(s->graph_exec, s->stream));
      s->sweeps_done += GRAPH_CHUNK;
      left -= GRAPH_CHUNK;
    }
  }
  while (left > 0) {
    rc = enqueue_fused(s, nullptr, nullptr);
    if (rc) return rc;
    s->sweeps_done++;
    left--;
  }
  return CLV_OK;
}

// A world with an empty shard, on a rank that has customers.  The mail's slots of one parity are reused two
// sweeps later, and what makes that safe is that the ranks wait for each other: a rank stores its units of
// sweep s + 2 after its draw of s + 1, which waited for every peer's units of s + 1, stored after that
// peer's draw of s had read and emptied its slots.  Nobody waits for an empty rank (it has no unit below
// n_units_global), so nothing would keep the others from running ahead of it and storing sweep s + 2 over
// the units of sweep s it has not read yet.  The host holds them back instead: sweep s is launched only once
// every empty rank's progress word in this rank's mail (kernels.hip post_progress) shows that it has started
// sweep s - 1, so its launch of s - 2, slot resets included, has ended.  The first two sweeps after fx_epoch
// find every slot empty.  Bounded like the in-kernel waits; such worlds are small (at most about world_size^2
// blocks), so one host round trip per sweep is their whole cost.
int wait_for_empty_ranks(clv_sampler* s, int64_t sweep) {
  const Geometry& g = s->g;
  if (sweep <= s->fx_epoch + 2) return CLV_OK;
  const int64_t per_rank = (int64_t)g.blocks_per_rank * BLOCK;
  const int first = (int)((g.n_global + per_rank - 1) / per_rank);  // ranks first .. world_size - 1 are empty
  std::vector<int64_t> prog((size_t)(g.world_size - first), -1);
  const double* words = s->d_mail + mail_slots(g.world_size, g.n_chains, g.stride, g.units_per_rank) + first;
  if (!s->poll_stream) CLV_HIP(hipStreamCreateWithFlags(&s->poll_stream, hipStreamNonBlocking));
  const int64_t t0 = host_now_ns(), bound_ns = (int64_t)s->wait_ticks * 10;  // (ticks of 100 MHz)
  for (;;) {
    CLV_HIP(hipMemcpyAsync(prog.data(), words, sizeof(int64_t) * prog.size(), hipMemcpyDeviceToHost, s->poll_stream));
    CLV_HIP(hipStreamSynchronize(s->poll_stream));
    size_t behind = 0;
    while (behind < prog.size() && prog[behind] >= sweep - 1) ++behind;  // (-1: that rank has not polled yet)
    if (behind == prog.size()) return CLV_OK;
    if (host_now_ns() - t0 > bound_ns)
      return fail(CLV_EHIP, "fused peer exchange: a wait timed out (a peer rank not running?); state unchanged [host wait: sweep " +
                                std::to_string(sweep) + ", empty rank " + std::to_string(first + (int)behind) +
                                " last polled for sweep " + (prog[behind] < 0 ? std::string("none") : std::to_string(prog[behind])) + "]");
  }
}

// World size > 1 without a resident grid: n launches of the sweep kernel whose fused tail
// exchanges unit partials through the peers' mail (kernels.hip sweep_body, FX).  The state before
// the call is kept in the persistent path's *_alt buffers, so that a call in which a wait times out
// (a peer not running; the call's later launches then return at once) leaves it unchanged, and a
// completed call can be undone by clv_rollback (a step that failed on another rank).
int run_fused_exchange(clv_sampler* s, int64_t n_sweeps) {
  s->last_persist_n = 0;
  if (n_sweeps == 0) return CLV_OK;
  const Geometry& g = s->g;
  const size_t nl = sizeof(double) * state_count(g), nh = sizeof(double) * hyper_count(g);
  CLV_HIP(hipMemcpyAsync(s->d_lam_alt, s->d_lam, nl, hipMemcpyDeviceToDevice, s->stream));
  CLV_HIP(hipMemcpyAsync(s->d_mu_alt, s->d_mu, nl, hipMemcpyDeviceToDevice, s->stream));
  CLV_HIP(hipMemcpyAsync(s->d_hyper_alt, s->d_hyper, nh, hipMemcpyDeviceToDevice, s->stream));
  if (s->d_sums_prev)
    CLV_HIP(hipMemcpyAsync(s->d_sums_prev, s->d_sums, sizeof(double) * sums_count(g), hipMemcpyDeviceToDevice, s->stream));
  const int64_t before = s->sweeps_done;
  int rc = CLV_OK;
  if (g.nb_local > 0 && world_has_empty_shard(g.n_global, g.world_size, g.blocks_per_rank)) {
    for (int64_t k = 0; k < n_sweeps && rc == CLV_OK; ++k) {  // (an empty rank itself waits in its kernel, as every rank does)
      rc = wait_for_empty_ranks(s, s->sweeps_done + 1);
      if (rc == CLV_OK) rc = enqueue_fused_sweeps(s, 1);
    }
  } else {
    rc = enqueue_fused_sweeps(s, n_sweeps);
  }
  CLV_HIP(hipStreamSynchronize(s->stream));
  const bool aborted = __atomic_load_n(s->h_abort, __ATOMIC_ACQUIRE) != 0;
  if (rc == CLV_OK && !aborted) {
    s->last_persist_n = n_sweeps;
    s->rb_pend = false;      // (rollback: the hyper state before the call is the copy in hyper_alt)
    s->rb_hyper_swaps = 1;
    return CLV_OK;
  }
  // back to the state before the call (copies: a captured graph keeps the buffer addresses)
  CLV_HIP(hipMemcpy(s->d_lam, s->d_lam_alt, nl, hipMemcpyDeviceToDevice));
  CLV_HIP(hipMemcpy(s->d_mu, s->d_mu_alt, nl, hipMemcpyDeviceToDevice));
  CLV_HIP(hipMemcpy(s->d_hyper, s->d_hyper_alt, nh, hipMemcpyDeviceToDevice));
  *s->h_abort = 0;
  s->sweeps_done = before;
  if (int rc2 = rewind_ctrl_and_sums(s)) return rc2;
  CLV_HIP(hipMemset(s->d_arrive, 0, sizeof(uint32_t) * arrive_count(g)));
  s->p2p_ready = false;  // mail slots in an unknown state: clv_p2p_connect refills them
  if (rc) return rc;
  return fail(CLV_EHIP, "fused peer exchange: a wait timed out (a peer rank not running?); state unchanged" +
                            take_wait_diag(s));
}

// World size 1 with the draws streamed to the host (clv_stream_draws): the burn-in in one go, the
// stored sweeps in sub-runs of >= 256 sweeps and ~64 MB of draws, each sub-run's draws handed to the
// copy pool while the next one runs (the same launches' sweeps in the same order: the same bits).
int run_streaming(clv_sampler* s, int64_t n_sweeps) {
  const Geometry& g = s->g;
  const int64_t per_draw = (int64_t)g.n_chains * g.n * (g.D + 2) * (int64_t)sizeof(double);
  const int64_t chunk = std::max<int64_t>(256, std::max<int64_t>(1, (64LL << 20) / std::max<int64_t>(per_draw, 1)) * g.thin);
  int64_t left = n_sweeps;
  while (left > 0) {
    const int64_t k = s->sweeps_done < g.burnin ? std::min<int64_t>(left, g.burnin - s->sweeps_done)
                                                : std::min<int64_t>(left, chunk);
    int rc;
    if (s->persistent) {
      rc = run_persistent(s, k);
    } else {
      rc = enqueue_fused_sweeps(s, k);
      if (rc == CLV_OK && hipStreamSynchronize(s->stream) != hipSuccess) rc = fail(CLV_EHIP, "hipStreamSynchronize");
    }
    if (rc) return rc;
    stream_enqueue(s);
    left -= k;
  }
  return CLV_OK;
}
}  // namespace

extern "C" {

int clv_run(clv_sampler* s, int64_t n_sweeps) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  s->clk_first = s->sweeps_done + 1;
  if (s->g.world_size != 1) {
    if (!s->p2p_ready) return fail(CLV_ESTATE, "sharded clv_run needs clv_p2p_connect; else use clv_sweep/clv_hyper");
    if (s->pending_init_hyper) return fail(CLV_ESTATE, "bivariate: call clv_hyper once before the first sweep");
    if (n_sweeps < 0) return fail(CLV_EINVAL, "n_sweeps < 0");
    CLV_HIP(hipSetDevice(s->device));
    if (s->p2p_capable) return run_persistent(s, n_sweeps);
    return run_fused_exchange(s, n_sweeps);
  }
  if (n_sweeps < 0) return fail(CLV_EINVAL, "n_sweeps < 0");
  s->host_ns[0] = host_now_ns();
  CLV_HIP(hipSetDevice(s->device));
  s->host_ns[1] = host_now_ns();
  int rc = check_replay_range(s, n_sweeps);
  if (rc) return rc;
  if (s->pending_init_hyper) {
    rc = enqueue_hyper(s, nullptr, 1, nullptr, nullptr);
    if (rc) return rc;
    s->pending_init_hyper = false;
  }
  if (s->ds_dest) return run_streaming(s, n_sweeps);
  if (s->persistent) {
    rc = run_persistent(s, n_sweeps);
    s->host_ns[6] = host_now_ns();
    return rc;
  }
  rc = enqueue_fused_sweeps(s, n_sweeps);
  if (rc) return rc;
  CLV_HIP(hipStreamSynchronize(s->stream));
  return CLV_OK;
}

int clv_stream_draws(clv_sampler* s, double* level1) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (s->ds) {
    stream_wait(s->ds);
    // the old registration ends here; a new one streams every draw again from the first
    // (ds_next = 0), so a failure of the old pieces has nothing left to repair
    stream_clear_failed(s->ds);
  }
  if (!level1) {
    s->ds_dest = nullptr;
    return CLV_OK;
  }
  if (s->g.world_size != 1) return fail(CLV_ESTATE, "draw streaming needs world_size 1");
  if (!s->d_level1) return fail(CLV_ESTATE, "draw streaming needs draw_sink == CLV_SINK_FULL with draws to store");
  CLV_HIP(hipSetDevice(s->device));
  if (!s->ds) s->ds = new DrawStreamState();
  s->ds_dest = level1;
  s->ds_next = 0;
  const Geometry& g = s->g;
  stream_prefault(s->ds, s->device, level1, sizeof(double) * level1_count(g));
  // draws of sweeps already run: the pool copies on the null stream, which does not order against
  // the sampler's non-blocking stream, so the sweeps enqueued there must have completed
  CLV_HIP(hipStreamSynchronize(s->stream));
  stream_enqueue(s);
  return CLV_OK;
}

int clv_rollback(clv_sampler* s) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  if (s->ds_dest) return fail(CLV_ESTATE, "clv_rollback while the draws are streamed (clv_stream_draws)");
  if (s->last_persist_n <= 0) return fail(CLV_ESTATE, "nothing to roll back (the last call was not a completed persistent clv_run)");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  s->d_lam.swap(s->d_lam_alt);
  s->d_mu.swap(s->d_mu_alt);
  // the hyper state the launch started from: pending statistics (still in their buffer), or the
  // hyper buffer that was current then (in hyper_alt after an odd number of swaps since)
  if (s->rb_hyper_swaps & 1) s->d_hyper.swap(s->d_hyper_alt);
  s->pend = s->rb_pend;
  s->pend_buf = s->rb_pend_buf;
  s->rb_hyper_swaps = 0;
  s->sweeps_done -= s->last_persist_n;
  s->last_persist_n = 0;
  if (int rc = restart_fx_epoch(s)) return rc;
  if (int rc = rewind_ctrl_and_sums(s)) return rc;
  return drop_graph(s);
}

int clv_read_draws(clv_sampler* s, double* level1, double* level2, double* loglik) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  if (level2) {
    int rc = persist_flush(s);  // the last level-2 record may still be pending
    if (rc) return rc;
  }
  const Geometry& g = s->g;
  const size_t C = g.n_chains;
  if (level1) {
    if (!s->d_level1 && g.n_draws > 0 && g.n > 0) return fail(CLV_ESTATE, "level-1 draws need draw_sink == CLV_SINK_FULL");
    bool done = false;
    if (s->ds_dest == level1) {  // streamed: the rest of the stored draws, then wait for every copy
      stream_enqueue(s);
      done = stream_wait(s->ds);
      // (draws beyond the stored ones are never written: zeros, as the device buffer holds)
      const int64_t k = stored_draws(s);
      if (done && k < g.n_draws)
        for (size_t c = 0; c < C; ++c)
          std::memset(level1 + ((int64_t)c * g.n_draws + k) * g.n * (g.D + 2), 0,
                      sizeof(double) * (size_t)((g.n_draws - k) * g.n * (g.D + 2)));
    } else if (s->ds) {
      stream_wait(s->ds);
    }
    if (s->d_level1 && !done) {
      CLV_HIP(s->d_level1.download(level1, level1_count(g)));
      if (s->ds && s->ds_dest == level1) stream_clear_failed(s->ds);  // the full copy repaired it
    }
  }
  if (level2 && s->d_level2)
    CLV_HIP(s->d_level2.download(level2, loglik_count(g) * g.l2w));
  if (loglik && s->d_loglik)
    CLV_HIP(s->d_loglik.download(loglik, loglik_count(g)));
  return CLV_OK;
}

int clv_read_summary(clv_sampler* s, double* sums, int64_t* n_stored) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  const Geometry& g = s->g;
  if (n_stored) *n_stored = stored_draws(s);
  const bool summary_sink = s->cfg.draw_sink == CLV_SINK_SUMMARY || s->cfg.draw_sink == CLV_SINK_SUMMARY_PCT;
  if (sums && !(summary_sink && g.n == 0)) {  // (an empty shard's sums have no columns: nothing to copy)
    if (!s->d_sums) return fail(CLV_ESTATE, "summaries need draw_sink == CLV_SINK_SUMMARY (or _PCT)");
    CLV_HIP(s->d_sums.download(sums, sums_count(g)));
  }
  return CLV_OK;
}

int clv_get_state(clv_sampler* s, double* lambdas, double* mus, double* hyper) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  CLV_HIP(hipSetDevice(s->device));
  CLV_HIP(hipStreamSynchronize(s->stream));
  if (hyper) {
    int rc = persist_flush(s);
    if (rc) return rc;
  }
  const Geometry& g = s->g;
  if (lambdas && g.n) CLV_HIP(hipMemcpy(lambdas, s->d_lam, sizeof(double) * g.n_chains * g.n, hipMemcpyDeviceToHost));
  if (mus && g.n) CLV_HIP(hipMemcpy(mus, s->d_mu, sizeof(double) * g.n_chains * g.n, hipMemcpyDeviceToHost));
  if (hyper) {
    std::vector<double> h((size_t)g.n_chains * HS);
    CLV_HIP(hipMemcpy(h.data(), s->d_hyper, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    const int w = g.K * g.D + g.D * g.D;
    for (int c = 0; c < g.n_chains; ++c) {
      for (int i = 0; i < g.K * g.D; ++i) hyper[c * w + i] = h[c * HS + H_BETA + i];
      for (int p = 0; p < g.D; ++p)
        for (int q = 0; q < g.D; ++q) hyper[c * w + g.K * g.D + p * g.D + q] = h[c * HS + H_SIGMA + p * 3 + q];
    }
  }
  return CLV_OK;
}

int clv_set_state(clv_sampler* s, const double* lambdas, const double* mus, const double* hyper, int64_t sweeps_done) {
  if (!s || sweeps_done < 0) return fail(CLV_EINVAL, "bad arguments");
  const Geometry& g = s->g;
  // the sampler takes logs of the state (bi:286-287; Philox mode: log_fast, defined for positive
  // normal doubles): reject what exp() of a log-scale state can never be
  for (const double* v : {lambdas, mus})
    if (v)
      for (int64_t i = 0; i < (int64_t)g.n_chains * g.n; ++i)
        if (!(v[i] >= 2.2250738585072014e-308 && v[i] <= 1.7976931348623157e308))
          return fail(CLV_EINVAL, "lambdas and mus must be positive, normal and finite");
  CLV_HIP(hipSetDevice(s->device));
  {  // a pending draw belongs to the state being replaced (its level-2 record too)
    int rc = persist_flush(s);
    if (rc) return rc;
  }
  if (lambdas && g.n) CLV_HIP(hipMemcpy(s->d_lam, lambdas, sizeof(double) * g.n_chains * g.n, hipMemcpyHostToDevice));
  if (mus && g.n) CLV_HIP(hipMemcpy(s->d_mu, mus, sizeof(double) * g.n_chains * g.n, hipMemcpyHostToDevice));
  if (hyper) {
    CLV_HIP(hipMemcpy(s->d_bs, hyper, sizeof(double) * g.n_chains * (g.K * g.D + g.D * g.D), hipMemcpyHostToDevice));
    CLV_HIP(launch_set_hyper(g.D, g.K, g.n_chains, s->d_hyper, s->d_bs, s->prior.omega2, s->replay, s->stream));
    s->pending_init_hyper = false;
  }
  Ctrl c{};
  c.cur = sweeps_done;
  CLV_HIP(hipMemcpyAsync(s->d_ctrl, &c, sizeof(Ctrl), hipMemcpyHostToDevice, s->stream));
  CLV_HIP(hipStreamSynchronize(s->stream));
  s->sweeps_done = sweeps_done;
  s->last_persist_n = 0;
  if (int rc = restart_fx_epoch(s)) return rc;
  stream_rewind(s);
  return CLV_OK;
}

int clv_set_timing(clv_sampler* s, int32_t enable) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  int rc = harvest_timing(s);  // never drop pending timed launches
  if (rc) return rc;
  s->timing = enable != 0;
  if (s->timing) {  // created here, not inside the first timed clv_run
    CLV_HIP(hipSetDevice(s->device));
    rc = ensure_events(s);
    if (rc) return rc;
  }
  s->t_sweep_ms = s->t_hyper_ms = 0.0;
  s->n_sweep_timed = s->n_hyper_timed = 0;
  return CLV_OK;
}

int clv_kernel_time(clv_sampler* s, double* sweep_ms, int64_t* n_sweep, double* hyper_ms, int64_t* n_hyper) {
  if (!s) return fail(CLV_EINVAL, "null sampler");
  int rc = harvest_timing(s);
  if (rc) return rc;
  if (sweep_ms) *sweep_ms = s->t_sweep_ms;
  if (n_sweep) *n_sweep = s->n_sweep_timed;
  if (hyper_ms) *hyper_ms = s->t_hyper_ms;
  if (n_hyper) *n_hyper = s->n_hyper_timed;
  return CLV_OK;
}

// ---- test hooks ----
int clv_debug_stamps(clv_sampler* s, uint64_t* out) {
  if (!s || !out) return fail(CLV_EINVAL, "null argument");
  if (!s->d_stamps) return fail(CLV_ESTATE, "library not built with CLV_STAMPS (make STAMPS=1)");
  CLV_HIP(hipStreamSynchronize(s->stream));
  CLV_HIP(hipMemcpy(out, s->d_stamps, sizeof(uint64_t) * 1024 * 8, hipMemcpyDeviceToHost));
  return CLV_OK;
}

int clv_debug_wg_stamps(clv_sampler* s, uint64_t* out) {
  if (!s || !out) return fail(CLV_EINVAL, "null argument");
  if (!s->d_stamps) return fail(CLV_ESTATE, "library not built with CLV_STAMPS (make STAMPS=1)");
  CLV_HIP(hipStreamSynchronize(s->stream));
  CLV_HIP(hipMemcpy(out, s->d_stamps + 1024 * 8, sizeof(uint64_t) * 12 * s->g.n_chains * (s->g.nb_local + 1),
                    hipMemcpyDeviceToHost));
  return CLV_OK;
}

int clv_debug_split_stamps(clv_sampler* s, uint64_t* out) {
  if (!s || !out) return fail(CLV_EINVAL, "null argument");
  if (!s->d_stamps) return fail(CLV_ESTATE, "library not built with CLV_STAMPS (make STAMPS=1)");
  CLV_HIP(hipStreamSynchronize(s->stream));
  const size_t wgs = (size_t)s->g.n_chains * (s->g.nb_local + 1);
  CLV_HIP(hipMemcpy(out, s->d_stamps + 1024 * 8 + 12 * wgs, sizeof(uint64_t) * 16 * wgs, hipMemcpyDeviceToHost));
  return CLV_OK;
}

int clv_debug_host_times(const clv_sampler* s, int64_t* out) {
  if (!s || !out) return fail(CLV_EINVAL, "bad arguments");
  for (int k = 0; k < 8; ++k) out[k] = s->host_ns[k];
  return CLV_OK;
}

int clv_debug_philox(uint32_t k0, uint32_t k1, const uint32_t* ctr, int64_t n, uint32_t* out) {
  if (!ctr || !out || n < 0) return fail(CLV_EINVAL, "bad arguments");
  DevPtr<uint32_t> dc, dout;
  const size_t words = 4 * std::max<int64_t>(n, 1);
  CLV_HIP(dc.alloc(words));
  CLV_HIP(dout.alloc(words));
  CLV_HIP(hipMemcpy(dc, ctr, 16 * n, hipMemcpyHostToDevice));
  CLV_HIP(launch_debug_philox(k0, k1, dc, n, dout, nullptr));
  CLV_HIP(dout.download(out, 4 * n));
  return CLV_OK;
}

int clv_debug_variates(uint64_t seed, int32_t chain, uint32_t sweep, int64_t n, int32_t S, float* tl, float* tm,
                       float* ua, double* uz, double* ut, double* ea, double* ez, float* l2u) {
  if (n < 1 || S < 0) return fail(CLV_EINVAL, "bad arguments");
  const int64_t nS = std::max<int64_t>(n * S, 1);
  DevPtr<float> dtl, dtm, dua, dl2u;
  DevPtr<double> duz, dut, dea, dez;
  for (DevPtr<float>* b : {&dtl, &dtm, &dua, &dl2u}) CLV_HIP(b->alloc(nS));
  for (DevPtr<double>* b : {&duz, &dut, &dea, &dez}) CLV_HIP(b->alloc(n));
  CLV_HIP(launch_debug_variates(seed, chain, sweep, n, S, dtl, dtm, dua, dl2u, duz, dut, dea, dez, nullptr));
  if (S > 0) {
    CLV_HIP(dtl.download(tl, n * S));
    CLV_HIP(dtm.download(tm, n * S));
    CLV_HIP(dua.download(ua, n * S));
    if (l2u) CLV_HIP(dl2u.download(l2u, n * S));
  }
  CLV_HIP(duz.download(uz, n));
  CLV_HIP(dut.download(ut, n));
  CLV_HIP(dea.download(ea, n));
  CLV_HIP(dez.download(ez, n));
  return CLV_OK;
}

int clv_debug_log2u_scan(uint64_t w_begin, uint64_t w_end, double* out) {
  if (!out || w_end > (1ull << 32) || w_begin >= w_end) return fail(CLV_EINVAL, "bad arguments");
  constexpr int NB = 4096;
  std::vector<double> r(4 * NB);
  DevPtr<double> dres;
  CLV_HIP(dres.alloc(r.size()));
  CLV_HIP(launch_debug_log2u_scan(w_begin, w_end, NB, dres, nullptr));
  CLV_HIP(dres.download(r.data(), r.size()));
  double mu = 0.0, ma = 0.0, wu = 0.0, mu_far = 0.0;
  for (int b = 0; b < NB; ++b) {
    if (r[4 * b] > mu) {
      mu = r[4 * b];
      wu = r[4 * b + 2];
    }
    ma = std::max(ma, r[4 * b + 1]);
    mu_far = std::max(mu_far, r[4 * b + 3]);
  }
  out[0] = mu;      // max error in fp32 ulps of the exact log2
  out[1] = ma;      // max absolute error
  out[2] = wu;      // the word where the ulp error is largest
  out[3] = mu_far;  // max ulp error where U <= 1/2 (|log2 U| >= 1)
  return CLV_OK;
}

int clv_debug_t3(const uint32_t* words, int64_t n, int32_t packed, float* tl, float* tm) {
  if (!words || !tl || !tm || n < 1 || (packed != 0 && packed != 1)) return fail(CLV_EINVAL, "bad arguments");
  DevPtr<uint32_t> dw;
  DevPtr<float> dl, dm;
  CLV_HIP(dw.upload(words, 3 * n));
  CLV_HIP(dl.alloc(n));
  CLV_HIP(dm.alloc(n));
  CLV_HIP(launch_debug_t3(dw, n, packed, dl, dm, nullptr));
  CLV_HIP(dl.download(tl, n));
  CLV_HIP(dm.download(tm, n));
  return CLV_OK;
}

int clv_debug_level2(int32_t D, int32_t K, const clv_prior* prior, const double* xty, const double* yty,
                     const double* iwn, const double* chi2, const double* z, double* beta, double* sigma) {
  if ((D != 2 && D != 3) || K < 1 || K > CLV_MAX_K || !prior) return fail(CLV_EINVAL, "bad arguments");
  const std::vector<double> pr = pack_prior(prior, D, K);
  std::vector<double> in(K * D + D * D + 6 + D * K, 0.0);
  for (int i = 0; i < K * D; ++i) in[i] = xty[i];
  for (int i = 0; i < D * D; ++i) in[K * D + i] = yty[i];
  for (int i = 0; i < D * (D - 1) / 2; ++i) in[K * D + D * D + i] = iwn[i];
  for (int i = 0; i < D; ++i) in[K * D + D * D + 3 + i] = chi2[i];
  for (int i = 0; i < D * K; ++i) in[K * D + D * D + 6 + i] = z[i];
  std::vector<double> o(K * D + D * D);
  DevPtr<double> dpr, din, dout;
  CLV_HIP(dpr.upload(pr.data(), pr.size()));
  CLV_HIP(din.upload(in.data(), in.size()));
  CLV_HIP(dout.alloc(o.size()));
  CLV_HIP(launch_debug_level2(D, K, dpr, din, dout, nullptr));
  CLV_HIP(dout.download(o.data(), o.size()));
  for (int i = 0; i < K * D; ++i) beta[i] = o[i];
  for (int i = 0; i < D * D; ++i) sigma[i] = o[K * D + i];
  return CLV_OK;
}

int clv_debug_hyper_variates(uint64_t seed, int32_t chain, uint32_t sweep, double df, int64_t n, double* chi2,
                             double* normals) {
  if (n < 1 || df < 2.0) return fail(CLV_EINVAL, "bad arguments");
  DevPtr<double> dc, dn;
  CLV_HIP(dc.alloc(n));
  CLV_HIP(dn.alloc(n));
  CLV_HIP(launch_debug_hyper_variates(seed, chain, sweep, df, n, dc, dn, nullptr));
  CLV_HIP(dc.download(chi2, n));
  CLV_HIP(dn.download(normals, n));
  return CLV_OK;
}

int clv_debug_persist_choice(int32_t D, int32_t K, int32_t n_chains, int64_t grid_wgs, int32_t blocks_per_cu,
                             int32_t n_cu) {
  return persist_grid_chosen(D, K, n_chains, grid_wgs, blocks_per_cu, n_cu, false) ? 1 : 0;
}

int clv_debug_persist_fits(int64_t grid_wgs, int32_t blocks_per_cu, int32_t n_cu) {
  return persist_grid_fits(grid_wgs, blocks_per_cu, n_cu) ? 1 : 0;
}

int clv_debug_split_fits(int32_t n_chains, int32_t nb, int32_t blocks_per_cu, int32_t n_cu) {
  return persist_split_fits(n_chains, nb, blocks_per_cu, n_cu) ? 1 : 0;
}

int clv_debug_split_choice(int32_t n_chains, int32_t nb, int32_t blocks_per_cu, int32_t n_cu) {
  return split_chosen(n_chains, nb, blocks_per_cu, n_cu, false) ? 1 : 0;
}

int clv_debug_world_has_empty_shard(int64_t n_global, int32_t world, int32_t blocks_per_rank) {
  return world_has_empty_shard(n_global, world, blocks_per_rank) ? 1 : 0;
}

int clv_debug_sweep_plan(const int64_t* in, int32_t* out) {
  if (!in || !out) return fail(CLV_EINVAL, "null argument");
  Geometry g{};
  g.D = (int)in[0];
  g.K = (int)in[1];
  g.S = (int)in[2];
  g.n_chains = (int)in[3];
  g.nb_local = (int)in[4];
  g.blocks_per_unit = (int)in[5];
  g.n_units_global = in[6];
  g.world_size = (int)in[7];
  g.stride = g.K * g.D + g.D * (g.D + 1) / 2 + 1;
  SweepResources r;
  r.n_cu = (int)in[9];
  r.block = Instance{(int)in[10], in[11]};
  r.split = Instance{(int)in[12], in[13]};
  r.relay = Instance{(int)in[14], in[15]};
  SweepEnv e;
  e.persistent = (int)in[16];
  e.layout = (int)in[17];
  e.relay = (int)in[18];
  e.defer = in[19] != 0;
  const SweepPlan p = plan_sweep(g, in[8] != 0, r, e);
  const int32_t o[8] = {p.persistent, p.split, p.relay_steps, p.p2p_capable, p.p2p_persist_fits, p.fx_capable,
                        p.defer, (p.need_split ? 1 : 0) | (p.need_relay ? 2 : 0)};
  std::copy(o, o + 8, out);
  return p.error ? fail(CLV_EINVAL, p.error) : CLV_OK;
}

int clv_debug_split_relay_plan(int32_t S, int32_t R, int32_t* out) {
  if (!out || S < 0 || S > PRE_STEPS || !(R == 0 || R == 8 || R == 12)) return fail(CLV_EINVAL, "bad arguments");
  const SplitRelayPlan pl = split_relay_plan(S, R);
  // the steps each wavefront runs, then the steps whose variates each draws (the same by construction:
  // the kernel takes both from this one plan)
  const int32_t o[8] = {pl.own_begin, pl.own_end, pl.relay_begin, pl.relay_end,
                        pl.own_begin, pl.own_end, pl.relay_begin, pl.relay_end};
  std::copy(o, o + 8, out);
  return CLV_OK;
}

int clv_debug_split_draw_plan(int32_t R, int32_t share, int32_t* out) {
  if (!out || !(R == 8 || R == 12) || share < -1 || share >= SPLIT_DRAW_SHARES) return fail(CLV_EINVAL, "bad arguments");
  if (share < 0) {  // the share this library's relay instance was built with
    out[0] = SPLIT_RELAY_DRAW;
    return CLV_OK;
  }
  constexpr int NQ = PRE_STEPS / 4;
  for (int row = 0; row < SPLIT_CW; ++row) {
    for (int q = 0; q < NQ; ++q) {
      const SplitDrawSlot d = split_draw_plan(R, share, row, q);
      const int32_t o[4] = {d.wave, d.slot, d.staged, d.reader};
      std::copy(o, o + 4, out + (row * NQ + q) * 4);
    }
  }
  return CLV_OK;
}

int clv_debug_split_layout(int32_t n_chains, int32_t nb, int32_t* out) {
  if (!out || n_chains < 1 || nb < 1 || nb > SPLIT_MAX_NB || n_chains >= (1 << 15)) return fail(CLV_EINVAL, "bad arguments");
  const std::vector<int32_t> m = persist_split_layout(n_chains, nb);
  const int nwg = split_wgs(nb);
  for (size_t i = 0; i < m.size(); ++i) {
    int32_t* o = out + 8 * i;
    const int p = m[i] & 0xFFFF;
    o[0] = m[i] >> 16;
    for (int k = 1; k < 8; ++k) o[k] = -1;
    if (p == nwg) continue;  // the chain's level-2 workgroup
    const int r0 = SPLIT_CW * p;
    o[1] = r0;
    o[2] = std::min(SPLIT_CW, 4 * nb - r0);
    // the two records (persist_kernel_split): wavefront 0 writes the first, wavefront 1 the second
    const int b0 = (p & 1) ? (r0 - 2) / 4 : r0 / 4, b1 = (p & 1) ? (r0 + 2) / 4 : r0 / 4 + 1;
    o[3] = (p & 1) ? 3 : 1;  // 3: rows 2, 3 into extension records 2 (b / 3), + 1;  1: a whole block's slot
    o[4] = b0;
    if (b1 < nb) {
      o[5] = (p & 1) ? 1 : 2;  // 2: the prefix r0 + r1 into the block's slot
      o[6] = b1;
    }
    o[7] = (p & 1) ? nb + 2 * (b0 / 3) : -1;  // first extension record
  }
  return CLV_OK;
}

int clv_debug_wg_map(int32_t n_chains, int32_t nb, int32_t n_cu, int32_t* out) {
  if (!out || n_chains < 1 || nb < 0 || n_cu < 1 || n_chains >= (1 << 15) || nb >= (1 << 16))
    return fail(CLV_EINVAL, "bad arguments");
  const std::vector<int32_t> m = persist_wg_map(n_chains, nb, n_cu);
  std::copy(m.begin(), m.end(), out);
  return CLV_OK;
}

int clv_debug_mh_step(int64_t n, const int32_t* x, const uint8_t* z, const double* T_cal, const double* tau,
                      const double* mean, const double* prec3, const double* cur_pt, const float* t3,
                      const double* scale2, const float* log_u, double* out) {
  if (!x || !z || !T_cal || !tau || !mean || !prec3 || !cur_pt || !t3 || !scale2 || !log_u || !out || n < 1)
    return fail(CLV_EINVAL, "bad arguments");
  DevPtr<int32_t> dx;
  DevPtr<uint8_t> dz;
  DevPtr<double> dT, dtau, dm, dp, dc, ds, dout;
  DevPtr<float> dt3, dlu;
  CLV_HIP(dx.upload(x, n));
  CLV_HIP(dz.upload(z, n));
  CLV_HIP(dT.upload(T_cal, n));
  CLV_HIP(dtau.upload(tau, n));
  CLV_HIP(dm.upload(mean, 2 * n));
  CLV_HIP(dp.upload(prec3, 3));
  CLV_HIP(dc.upload(cur_pt, 2 * n));
  CLV_HIP(ds.upload(scale2, 2));
  CLV_HIP(dt3.upload(t3, 2 * n));
  CLV_HIP(dlu.upload(log_u, n));
  CLV_HIP(dout.alloc(7 * n));
  CLV_HIP(launch_debug_mh(dx, dz, dT, dtau, dm, dp, dc, dt3, ds, dlu, n, dout, nullptr));
  CLV_HIP(dout.download(out, 7 * n));
  return CLV_OK;
}

}  // extern "C"
static int debug_fast_fn(const double* x, int64_t n, double* out, bool log_fn) {
  if (!x || !out || n < 1) return fail(CLV_EINVAL, "bad arguments");
  DevPtr<double> dx, dout;
  CLV_HIP(dx.upload(x, n));
  CLV_HIP(dout.alloc(n));
  CLV_HIP(launch_debug_exp(dx, n, dout, nullptr, log_fn));
  CLV_HIP(dout.download(out, n));
  return CLV_OK;
}
extern "C" {
int clv_debug_exp(const double* x, int64_t n, double* out) { return debug_fast_fn(x, n, out, false); }

int clv_debug_log(const double* x, int64_t n, double* out) { return debug_fast_fn(x, n, out, true); }

}  // extern "C"
