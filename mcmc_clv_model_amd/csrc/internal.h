// Internal declarations shared by the library's translation units (every .hip file):
// the sampler handle's layout and the error/allocation helpers.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"

namespace clv {

// Records msg as the calling thread's clv_last_error() and returns code.
int fail(int code, const std::string& msg);

// Persistent path in two halves (capi.hip): enqueue one launch of n sweeps; wait for it and adopt
// its carried state (or restore the state it started from, if a wait in it timed out).
int persist_launch(clv_sampler* s, int64_t n_sweeps);
int persist_wait(clv_sampler* s);
int persist_flush(clv_sampler* s);  // the deferred level-2 draw, if one is pending (synchronous)
// A persistent grid of grid_wgs workgroups fits at once (with a residency margin) on n_cu CUs
// admitting blocks_per_cu of its workgroups each (capi.hip).
bool persist_grid_fits(int64_t grid_wgs, int blocks_per_cu, int n_cu);

// Level-1 draws streamed to a host buffer during the run (drawstream.hip): the pieces a sampler has
// in flight in the process-wide copy pool, and whether any failed.
struct DrawStreamState {
  std::mutex m;
  std::condition_variable cv;
  int64_t pending = 0;
  std::atomic<int> failed{0};
};
void stream_prefault(DrawStreamState* st, int device, void* dst, size_t bytes);  // touch dst's pages
void stream_copy(DrawStreamState* st, int device, const void* src, void* dst, size_t bytes);
bool stream_wait(DrawStreamState* st);  // every piece done; false if one failed since the last clear
void stream_clear_failed(DrawStreamState* st);  // after a full copy has repaired the destination

// The level-1 draws a CLV_SINK_FULL sampler holds in HBM after its run (analysis.hip): *l1 =
// [chain * draw][n][width], *n_draws = chains x stored draws; CLV_ESTATE without them.
int sampler_l1(clv_sampler* s, const double** l1, int64_t* n_draws, int32_t* width);
// The level-2 records [chain][draw][l2w] of a run that has stored them all, the deferred last one
// flushed (analysis.hip); CLV_ESTATE with the caller's message without them.
int sampler_l2(clv_sampler* s, const double** l2, const char* not_stored);

// Scoring customers outside the fit (kernels.hip; host side in score.hip).  launch_score_prepare:
// level2 [n_rec][D K + D (D + 1) / 2] -> hyper [n_rec][HS] (cleared by the caller).  launch_score:
// grid (ceil(a.g.n / BLOCK), a.g.n_chains), optional events around the kernel.  score_resources:
// VGPRs and scratch bytes per lane of the (D, K, sink) instance.
hipError_t launch_score_prepare(int D, int K, const double* level2, int64_t n_rec, double omega2, double* hyper,
                                hipStream_t st);
hipError_t launch_score(const SweepArgs& a, const ScoreArgs& e, bool summary, hipStream_t st,
                        hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
hipError_t score_resources(int D, int K, bool summary, int* vgprs, size_t* scratch_bytes);

// Many small fits in one launch (kernels.hip batch_fit_kernel; host side in batch.hip).
// launch_batch_fit: one workgroup per entry of wg_map [(fit, chain)], fits / wg_map / init_bs on the
// device, sweeps 1 .. n_sweeps, optional events around the kernel.  batch_fit_resources: VGPRs and
// scratch bytes per lane and workgroups per CU of the (D, K) instance.
hipError_t launch_batch_fit(int D, int K, const SweepArgs* fits, const int2* wg_map, const double* init_bs,
                            int64_t n_wgs, int64_t n_sweeps, hipStream_t st, hipEvent_t e0 = nullptr,
                            hipEvent_t e1 = nullptr);
hipError_t batch_fit_resources(int D, int K, int* vgprs, size_t* scratch_bytes, int* blocks_per_cu);

// Owning device allocation, freed by hipFree on the device current at destruction: the sampler handle's
// members, the test hooks' locals and (DevBuf, untyped) the analysis entry points' buffers.  Reads as its T*
// (A.x = s->d_x, if (s->d_level1), s->d_arrive + k).  A buffer's element count is written once, at its alloc / upload.
template <class T>
struct DevPtr {
  T* p = nullptr;
  DevPtr() = default;
  DevPtr(const DevPtr&) = delete;
  DevPtr& operator=(const DevPtr&) = delete;
  ~DevPtr() { reset(); }
  operator T*() const { return p; }
  template <class U> U* as() const { return (U*)p; }
  void reset(T* adopt = nullptr) {  // adopt: memory of another allocator that hipFree releases
    if (p) (void)hipFree(p);
    p = adopt;
  }
  void swap(DevPtr& o) { std::swap(p, o.p); }
  hipError_t alloc(size_t count) {  // (count 0: null)
    reset();
    return count ? hipMalloc((void**)&p, count * sizeof(T)) : hipSuccess;
  }
  hipError_t alloc(size_t count, int byte, hipStream_t st) {  // ... every byte set to `byte`, queued on st
    const hipError_t e = alloc(count);
    return e != hipSuccess || !count ? e : hipMemsetAsync(p, byte, count * sizeof(T), st);
  }
  hipError_t upload(const T* host, size_t count) {  // a device copy of host[count] (synchronous)
    const hipError_t e = alloc(count);
    return e != hipSuccess || !count ? e : hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice);
  }
  hipError_t download(T* host, size_t count) const { return hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost); }
};
using DevBuf = DevPtr<void>;  // untyped: only p, as<U>() and reset() apply (the counted members need sizeof(T))

// A scoped device switch, for the host-side orchestration of the analysis / data-preparation entry points.
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int dev) {
    (void)hipGetDevice(&prev);
    if (dev >= 0) (void)hipSetDevice(dev);
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace clv

#define CLV_HIP(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return ::clv::fail(CLV_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
  } while (0)

namespace clv {

// buf <- a device copy of host[count], queued on st.  A null host (an optional array) leaves buf
// null.
template <class T>
int upload(DevBuf& buf, const T* host, size_t count, hipStream_t st) {
  if (!host) return CLV_OK;
  CLV_HIP(hipMalloc(&buf.p, sizeof(T) * count));
  CLV_HIP(hipMemcpyAsync(buf.p, host, sizeof(T) * count, hipMemcpyHostToDevice, st));
  return CLV_OK;
}

}  // namespace clv

struct clv_sampler {
  clv_config cfg{};
  clv_prior prior{};
  clv::Geometry g{};
  bool replay = false;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own = nullptr;  // stream created by the sampler (destroyed with it)

  // Every device allocation of the handle is a DevPtr member: destroying the handle frees it.
  clv::DevPtr<int32_t> d_x;
  clv::DevPtr<double> d_tx, d_T, d_cov, d_logs;
  clv::DevPtr<double> d_lam, d_mu, d_hyper;
  clv::DevPtr<double> d_block, d_unit_own;
  double* d_unit = nullptr;         // the unit partials (a view): d_unit_own, or d_block when blocks_per_unit == 1
  clv::DevPtr<double> d_prior;
  clv::DevPtr<clv::Ctrl> d_ctrl;
  clv::DevPtr<uint32_t> d_arrive;   // fused-tail arrival counters: [chain], then [chain][units_per_rank]
  clv::DevPtr<double> d_hyp2;       // persistent kernel: [2][chain][HS] hand-off slots
  clv::DevPtr<double> d_pblock;     // persistent kernel: [chain][nb_local][stride] block-partial slots
  // persistent kernel: the launch writes its carried state into the *_alt buffers; clv_run swaps
  // them in only when no wave aborted (an aborted launch leaves the state untouched), and
  // clv_rollback swaps them back (a sharded step that failed on another rank)
  clv::DevPtr<double> d_lam_alt, d_mu_alt, d_hyper_alt;
  clv::DevPtr<double> d_sums_prev;  // summary sink: the running sums before the last persistent launch
  uint32_t* h_abort = nullptr;      // host-mapped copy of ctrl->abort (the kernel stores it on a timeout;
                                    // hipHostMalloc: freed in clv_destroy)
  uint32_t* d_h_abort = nullptr;    // its device address
  clv::DevPtr<unsigned long long> d_diag;  // wait-timeout record (kernels.hip report_wait), DIAG_WORDS
  clv::DevPtr<unsigned long long> d_clk;   // shader-clock record [CLK_RING][2] (SweepArgs::clk)
  int64_t clk_first = 0;            // first sweep of the last clv_run (clv_clock_ghz)
  uint64_t wait_ticks = 0;          // bound on every persistent-kernel wait (s_memrealtime ticks)
  bool slots_dirty = true;          // persistent hand-off slots need the sentinel fill (a completed
                                    // launch leaves them empty; only an aborted one does not)
  int64_t last_persist_n = 0;       // sweeps of the last persistent launch (rollback), 0 = none
  // Deferred level-2 draw (world size 1, persistent, CLV_DEFER != "0"): a launch leaves the draw
  // that follows its last sweep to the next launch, which draws it first while its customer
  // workgroups load (kernels.hip persist_level2, iteration -1), or to persist_flush before anything
  // reads the hyper state or the level-2 records.  The pending statistics live in d_pend[pend_buf]
  // ([2][chain][stride]: a launch reads one buffer and writes the other, so an aborted launch or a
  // rollback finds the state it started from intact).
  bool defer = false;
  bool pend = false;                // the hyper state is the draw of d_pend[pend_buf], not d_hyper
  int pend_buf = 0;
  clv::DevPtr<double> d_pend;
  bool rb_pend = false;             // rollback: the pending state before the last persistent launch
  int rb_pend_buf = 0;
  int rb_hyper_swaps = 0;           // hyper / hyper_alt swaps since it (its hyper is in hyper_alt if odd)
  bool persistent = false;          // clv_run uses persist_kernel (all workgroups resident)
  int persist_bpc = 0, n_cu = 0;    // persist_kernel occupancy (workgroups per CU), CUs
  bool split = false;               // the persistent launch uses the split layout (persist_kernel_split)
  int relay_steps = 0;              // split layout: the relay instance's hand-over step (0: helper instance)
  bool split_reverted = false;      // a split launch aborted: block layout for the handle's lifetime
  clv::DevPtr<int32_t> d_wgmap_split;  // split grid: linear workgroup -> (chain << 16 | chain's workgroup)
  // world size > 1: persistent kernel with the peer (xGMI) exchange
  bool p2p_capable = false;         // the grid fits at once and the unit partials fit UMAIL
  bool p2p_persist_fits = false;    // (p2p_capable as chosen at create; clv_p2p_set_persistent may clear p2p_capable)
  bool fx_capable = false;          // fused peer exchange (launch-per-sweep, any shard size)
  bool p2p_ready = false;           // clv_p2p_connect done: clv_run runs persist_kernel
  // A world with an empty shard (fused exchange only): nobody waits for an empty rank's units, so the
  // other ranks' hosts hold each sweep launch until every empty rank has started the sweep before it
  // (capi.hip wait_for_empty_ranks).  fx_epoch: the sweep count when the mail was last known empty on
  // every rank (connect, set_state, rollback); poll_stream: the stream the progress words are read on.
  int64_t fx_epoch = 0;
  hipStream_t poll_stream = nullptr;
  clv::DevPtr<double> d_mail;       // [2][world][chain][units_per_rank][stride]
  int mail_kind = -1;               // the mail's memory: 0 uncached, 1 fine-grained, 2 plain device memory
  clv::DevPtr<double*> d_peers;     // [world] mail pointers (peers' opened IPC mappings, own d_mail)
  clv::DevPtr<int32_t> d_wgmap;     // persistent grid: linear workgroup -> (chain << 16 | block)
  std::vector<void*> ipc_opened;    // hipIpcOpenMemHandle mappings to close
  clv::DevPtr<double> d_hvar;       // [chain][HV] precomputed hyper variates
  clv::DevPtr<unsigned long long> d_stamps;  // CLV_STAMPS diagnostic build only
  clv::DevPtr<double> d_level1, d_level2, d_loglik, d_sums;
  clv::DevPtr<float2> d_qstore;     // CLV_SINK_SUMMARY_PCT: [chain][draw][n] (lambda, mu) float32
  clv::DevPtr<double> d_tape;
  clv::DevPtr<double> d_bs;  // staging for set_hyper
  int64_t tape_sweeps = 0;

  bool pending_init_hyper = false;  // bivariate: the draw for sweep 1 is still due
  int64_t sweeps_done = 0;

  hipGraphExec_t graph_exec = nullptr;
  int graph_sweeps = 0;

  // clv_run waits for a persistent launch by polling its end event
  hipEvent_t done_ev = nullptr;     // recorded after each untimed persistent launch (timing: e1)
  int64_t inflight_n = 0;           // sweeps of the persistent launch in flight (persist_launch)
  hipEvent_t inflight_done = nullptr;  // its end event (null: wait with hipStreamSynchronize)

  // host clock (steady_clock, ns) at the steps of the last persistent clv_run: entry, after
  // hipSetDevice, before the launch call, after it, after the end-event record, wait done, return
  int64_t host_ns[8] = {0, 0, 0, 0, 0, 0, 0, 0};

  // clv_stream_draws: the caller's level-1 buffer and the draws (per chain) handed to the copy pool
  clv::DrawStreamState* ds = nullptr;
  double* ds_dest = nullptr;
  int64_t ds_next = 0;

  bool timing = false;
  std::vector<hipEvent_t> ev;  // 4 per slot: sweep start/end, hyper start/end
  std::vector<int64_t> ev_sweeps;  // sweeps per timed launch (persistent launches time many)
  int ev_used = 0;
  double t_sweep_ms = 0.0, t_hyper_ms = 0.0;
  int64_t n_sweep_timed = 0, n_hyper_timed = 0;
};

namespace clv {

// Element counts of the handle's buffers, each used at the allocation, the fill and the copies.
inline size_t state_count(const Geometry& g) { return (size_t)g.n_chains * std::max<int64_t>(g.n, 1); }  // lam, mu: each
inline size_t hyper_count(const Geometry& g) { return (size_t)g.n_chains * HS; }
inline size_t sums_count(const Geometry& g) { return (size_t)g.n_chains * CLV_N_SUM_STATS * g.n; }  // running sums
inline size_t arrive_count(const Geometry& g) { return (size_t)g.n_chains * (1 + g.units_per_rank); }  // arrival counters
inline size_t handoff_count(const Geometry& g) { return 2 * hyper_count(g); }                          // hand-off slots
inline size_t pblock_count(const Geometry& g) { return (size_t)g.n_chains * split_records(std::max(g.nb_local, 1)) * g.stride; }
inline size_t unit_count(const Geometry& g) { return (size_t)g.n_chains * g.units_per_rank * g.stride; }
inline size_t mail_count(const Geometry& g) { return mail_slots(g.world_size, g.n_chains, g.stride, g.units_per_rank) + MAIL_TAIL; }
inline size_t loglik_count(const Geometry& g) { return (size_t)g.n_chains * g.n_draws; }
inline size_t level1_count(const Geometry& g) { return loglik_count(g) * g.n * (g.D + 2); }

// Draws per chain the run has stored so far: at most n_draws.
inline int64_t stored_draws(const clv_sampler* s) {
  if (s->sweeps_done <= s->g.burnin) return 0;
  const int64_t k = (s->sweeps_done - 1 - s->g.burnin) / s->g.thin + 1;
  return k < s->g.n_draws ? k : (int64_t)s->g.n_draws;
}

}  // namespace clv

