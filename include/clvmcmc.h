/*
 * clvmcmc.h — C ABI of the MI355X-native Gibbs/MH sampler for the Abe (2009/2015)
 * hierarchical Pareto/NBD model (libclvmcmc.so, built from mcmc_clv_model_amd/csrc/).
 *
 * The reference (lucagem29/mcmc_clv_model) is pure Python and has no FFI of its own;
 * its drop-in boundary is the Python function pair
 *     src/models/bivariate/mcmc.py:437   mcmc_draw_parameters(...)
 *     src/models/trivariate/mcmc.py:580  mcmc_draw_parameters_rfm_m(...)
 * The Python host (mcmc_clv_model_amd/bivariate.py, trivariate.py) keeps those
 * signatures and binds the entry points below with ctypes.
 * Each entry point names the reference code it replaces.
 *
 * Conventions
 *  - Every function returns 0 on success or a negative CLV_E* code; the message of the
 *    last failure on the calling thread is available from clv_last_error().
 *  - Inputs are copied to device memory by clv_create(); outputs are written into
 *    caller-owned, contiguous, preallocated host buffers (float64, C order).
 *  - A sampler handle belongs to one host thread and one HIP device.
 *  - Customer data is struct-of-arrays: one contiguous array per CBS column.
 *  - State, log posteriors and the level-2 draw are float64, like the reference.  In Philox mode
 *    the MH proposal noise t3 is generated in float32 (fp32 hardware transcendentals), and the
 *    accept test compares in float64 against cur + ln2 * log2(U) with log2(U) an fp32 v_log_f32
 *    (DESIGN.md §5); replay mode (tests) takes the reference's own float64 variates.
 */
#ifndef CLVMCMC_H
#define CLVMCMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLV_ABI_VERSION 2

/* Customers per workgroup == the sufficient-statistic block size. Shards must begin on a
 * multiple of it so block partial sums are identical for every GPU count. */
#define CLV_BLOCK 256
#define CLV_MAX_K 9
#define CLV_MAX_D 3

enum { CLV_OK = 0, CLV_EINVAL = -1, CLV_EHIP = -2, CLV_ESTATE = -3, CLV_ENOMEM = -4 };
enum { CLV_RNG_PHILOX = 0, CLV_RNG_REPLAY = 1 };
/* CLV_SINK_SUMMARY_PCT: the summary sums plus every stored (lambda, mu) as a float32 pair,
 * [chain][draw][n] (8 B per customer and stored sweep instead of the full sink's 8 (D+2)), from
 * which clv_level1_summary_sampler forms the per-customer 2.5 / 97.5 percentiles of Table 4
 * (analysis_bi_helpers.py:95-96, 116-117): exact order statistics of the float32-rounded draws. */
enum { CLV_SINK_FULL = 0, CLV_SINK_SUMMARY = 1, CLV_SINK_NONE = 2, CLV_SINK_SUMMARY_PCT = 3 };

/* Per-customer running sums kept on device by CLV_SINK_SUMMARY / _PCT, accumulated over stored
 * draws. Layout of clv_read_summary(): [chain][stat][n].  CLV_SUM_MU_CAPPED sums
 * min(mu, CLV_SUMMARY_MU_CAP): Table 4's capped posterior mean of mu (analysis_bi_helpers.py:88-93). */
#define CLV_SUMMARY_MU_CAP 0.05
enum {
  CLV_SUM_LAMBDA = 0, CLV_SUM_MU, CLV_SUM_Z, CLV_SUM_LOG_LAMBDA, CLV_SUM_LOG_MU,
  CLV_SUM_LAMBDA2, CLV_SUM_MU2, CLV_SUM_ETA, CLV_SUM_LOG_ETA, CLV_SUM_MU_CAPPED, CLV_SUM_TAU,
  CLV_N_SUM_STATS
};

typedef struct clv_config {
  int32_t abi_version;   /* must equal CLV_ABI_VERSION */
  int32_t D;             /* 2 = bivariate (bivariate/mcmc.py), 3 = trivariate (trivariate/mcmc.py) */
  int32_t K;             /* design-matrix columns incl. the intercept, 1..CLV_MAX_K (bi:467-470) */
  int32_t n_mh_steps;    /* MH steps per sweep (bi:278, default 20) */
  int32_t burnin, mcmc, thin;          /* bi:437-447 semantics */
  int32_t n_chains;      /* chains batched into one launch (reference: sequential, bi:485) */
  int32_t chain_first;   /* global index of chain 0 of this handle: Philox key = seed + chain */
  int32_t rng_mode;      /* CLV_RNG_PHILOX or CLV_RNG_REPLAY (test mode, clv_set_replay_tape) */
  int32_t draw_sink;     /* CLV_SINK_* */
  int32_t device;        /* HIP device ordinal, -1 = current device */
  uint64_t seed;         /* Philox key base (reference: default_rng(seed + chain), bi:486) */
  int64_t n_global;      /* customers in the whole problem (nu_n and the log-lik mean use it) */
  int64_t shard_begin;   /* global index of this shard's first customer, multiple of CLV_BLOCK */
  int32_t world_size;    /* shards (one process per GPU); 1 = unsharded */
  int32_t rank;          /* this shard */
  int32_t blocks_per_rank; /* blocks of CLV_BLOCK customers per shard (last shard may be short);
                              0 = derive (unsharded only) */
  int32_t blocks_per_unit; /* blocks whose partials are summed into one exchanged unit (power of
                              two, a function of n_global only so every world size sums alike);
                              0 = derive with clv_default_blocks_per_unit(n_global) */
  uint64_t stream;       /* hipStream_t to launch on; 0 = a stream owned by the sampler */
} clv_config;

typedef struct clv_data {
  int64_t n;                 /* customers in this shard */
  const int32_t* x;          /* repeat transactions (bi:280) */
  const double* t_x;         /* recency (bi:194) */
  const double* T_cal;       /* calibration length (bi:194) */
  const double* covariates;  /* (K-1) arrays of n doubles, one per non-intercept column; NULL if K==1 */
  const double* log_s;       /* log average spend, D==3 only (tri:329) */
} clv_data;

/* Host-computed constants; the reference computes the same quantities on the host. */
typedef struct clv_prior {
  double lam_init;           /* bi:368 */
  double V[CLV_MAX_K * CLV_MAX_K];       /* inv(X'X + A0), K x K row-major (bi:248-249; constant) */
  double chol_V[CLV_MAX_K * CLV_MAX_K];  /* lower Cholesky factor of V */
  double A0B0[CLV_MAX_K * CLV_MAX_D];    /* A0 @ B0, K x D row-major (bi:250) */
  double S0_B0A0B0[CLV_MAX_D * CLV_MAX_D]; /* S0 + B0' A0 B0, D x D (bi:255 after expansion) */
  double nu_n;               /* nu0 + n_global (bi:256) */
  double beta_init[CLV_MAX_K * CLV_MAX_D]; /* tri: beta used by sweep 1 = beta_0 (tri:504) */
  double sigma_init[CLV_MAX_D * CLV_MAX_D];/* tri: Sigma used by sweep 1 = gamma_00 (tri:504) */
  double omega2;             /* tri: var(log_s, ddof=1) (tri:494) */
} clv_prior;

typedef struct clv_sampler clv_sampler;

int32_t clv_abi_version(void);
int32_t clv_default_blocks_per_unit(int64_t n_global);
/* sizeof(clv_config), sizeof(clv_data), sizeof(clv_prior) for which = 0, 1, 2 (binding checks). */
int64_t clv_sizeof(int32_t which);
const char* clv_last_error(void);
int clv_device_count(int32_t* count);

/* Allocate device state, upload the shard, initialise lambda/mu (bi:367-379, tri:488-504) and,
 * for D==2, the block partial sums the first level-2 draw needs. Replaces the setup half of
 * _run_chain (bi:346-382, tri:465-507). */
int clv_create(const clv_config* cfg, const clv_data* data, const clv_prior* prior,
               clv_sampler** out);
void clv_destroy(clv_sampler* s);

/* Test mode (CLV_RNG_REPLAY): variates recorded from the reference's numpy Generator.
 * Per chain, per sweep: [u_z n][v_tau n][S x (t_l n, t_m n, u_acc n)][eta_z n if D==3]
 * [hyper 40: iw_normal(3) iw_chi2(3) mvn_noise(<=27) pad]; chains back to back. */
int clv_set_replay_tape(clv_sampler* s, const double* tape, int64_t n_sweeps);
int64_t clv_replay_sweep_stride(const clv_sampler* s);

/* Run n sweeps (world_size == 1, or sharded after clv_p2p_connect). One sweep = a6's loop body: z (bi:388),
 * tau (bi:390), level-2 (bi:393), level-1 MH (bi:396), eta (tri:524-526), storage (bi:402-428).
 * Synchronous; chunks of sweeps are replayed from a captured hipGraph.  The persistent path at
 * world size 1 leaves the level-2 draw that follows its last sweep pending (CLV_DEFER, default on):
 * the next clv_run draws it first, and clv_get_state / clv_set_state / clv_read_draws (level 2) /
 * clv_sweep / clv_hyper draw it before they read or replace the state — the same draw either way,
 * so results never depend on how a run is cut into clv_run calls. */
int clv_run(clv_sampler* s, int64_t n_sweeps);
/* Persistent path only: undo the last completed clv_run (state, sweep count, summary sums) — a
 * sharded step whose persistent launch failed on another rank is redone by every rank from the
 * same point.  A clv_run that fails (a wait timed out) already leaves the state unchanged. */
int clv_rollback(clv_sampler* s);

/* Sharded stepping (one process per GPU; the caller exchanges the unit partials over RCCL):
 *   after clv_create, bivariate only: [exchange] clv_hyper   (initial draw, bi:393 of sweep 1)
 *   per sweep:                        clv_sweep, [exchange] clv_hyper
 * (bivariate: the hyper after sweep s is bi:393 of sweep s+1; trivariate: tri:529 of sweep s).
 * clv_partials() exposes this shard's unit partials, [chain][stride][units_per_rank] doubles;
 * clv_hyper() reads the gathered buffer [world][chain][stride][units_per_rank]
 * (NULL = the local buffer, world_size == 1) and sums it in global unit order. */
int clv_sweep(clv_sampler* s);
int clv_hyper(clv_sampler* s, const double* gathered_device_ptr);
int clv_partials(clv_sampler* s, double** device_ptr, int64_t* n_doubles, int32_t* stride);
/* Device-to-device copy of this shard's unit partials into dst (on the sampler's stream). */
int clv_copy_partials(clv_sampler* s, void* dst_device_ptr);
int clv_synchronize(clv_sampler* s);
int64_t clv_sweeps_done(const clv_sampler* s);

/* Average shader clock (GHz) of the device over the last clv_run: s_memtime against s_memrealtime
 * (100 MHz) over its sweeps but the last (at most the last 1024), each sweep's interval measured on
 * one CU by chain 0's level-2 workgroup of the persistent kernel (s_memtime counts per XCD).  *ghz = 0
 * when the run had fewer than 2 sweeps or ran without the persistent kernel (the launch-per-sweep
 * kernel keeps no record: it measured 1-1.5% slower with one).  Measurement
 * only — the reference has no counterpart; bench.py reports it beside every timed line, because
 * MI355X boxes of one pool were measured to run the same cycles at clocks ~13% apart (DESIGN.md §8
 * round 5).  Synchronizes the sampler's stream. */
int clv_clock_ghz(clv_sampler* s, double* ghz);
/* Shader clock (GHz) read by a probe kernel enqueued on the sampler's stream behind whatever it runs
 * (csrc/probe.hip): one 64-lane workgroup per CU busy for `us` microseconds (1..1e5) of s_memrealtime,
 * s_memtime against s_memrealtime on each CU.  For legs whose kernel keeps no record of its own (the
 * launch-per-sweep kernel): called right after the timed launches, it reads the clock they ran at
 * (the governor moves on a millisecond scale).  Measurement only.  Synchronizes the stream. */
int clv_clock_probe(clv_sampler* s, double us, double* ghz);
/* How clv_run launches: out[6] = (persistent 0/1, persistent-kernel workgroups per CU, CUs,
 * logical workgroups per sweep (one per customer block, + one level-2 workgroup per chain when
 * persistent), workgroups dispatched, layout of the persistent grid: 0 none, 1 block, 2 split,
 * -1 block after a split launch aborted).
 * Split layout (bivariate, world_size == 1, n_mh_steps <= 20, at most 256 blocks): 512-thread
 * workgroups of six customer and two helper wavefronts, one per CU, chosen where that grid is
 * resident whole (clv_debug_split_choice) and the block layout would put two workgroups on a CU;
 * CLV_PERSIST_LAYOUT = block | split forces one (split only where it can run).  Same results to
 * the bit.
 * The split layout has two instances.  Helpers: wavefronts 6 and 7 draw part of the next sweep's
 * variates for the rows that share a SIMD.  Relay (n_mh_steps > the compile-time relay point
 * CLV_SPLIT_RELAY_STEPS, 8 or 12; 0 B of scratch): wavefronts 6 and 7 instead take over rows 4 and 5
 * after that many MH steps, through one LDS record and flag per row and sweep, and finish and
 * reduce them.  CLV_SPLIT_RELAY = 0 | 1 forces the helpers / the relay (the relay only where it can
 * run; anything else is CLV_EINVAL); unset, the relay runs where it can (8 steps
 * measured faster than the helpers, 12 slower).  Same results to
 * the bit.  clv_split_relay_steps: *out = the relay point of a handle running the relay instance,
 * else 0 (clv_launch_info's array stays six words).
 * Persistent = one launch for all of a clv_run's sweeps with every customer block resident, chosen
 * at create when world_size == 1, Philox mode, every workgroup fits at once (with a residency
 * margin) and few enough CUs hold two of them for it to pay (clv_debug_persist_choice), unless
 * CLV_PERSISTENT is "0" ("1": wherever it fits).  Otherwise one launch of the sweep kernel per
 * sweep (fused level-2 tail), replayed from captured hipGraph chunks. */
int clv_launch_info(const clv_sampler* s, int64_t* out);
int clv_split_relay_steps(const clv_sampler* s, int32_t* out);
/* Sharded runs without a host collective per sweep (world_size > 1, Philox mode): the persistent
 * kernel's level-2 workgroup of each chain writes this rank's unit partials of sweep s straight into
 * EVERY rank's mail buffer (device stores over xGMI into IPC-mapped peer memory), waits until its
 * own mail holds all ranks' units, and sums them in the same global unit order as clv_hyper — so
 * results are bitwise those of clv_sweep/clv_hyper with an all-gather (and of world size 1).
 * Replaces, per sweep, the all-gather of bi:243-255's statistics.
 *   clv_p2p_info:    out[6] = (capable 0/1, connected 0/1, mail bytes, mail device pointer,
 *                    persistent 0/1, mail memory: 0 uncached / 1 fine-grained / 2 device default /
 *                    -1 none); persistent = every workgroup of the persistent grid fits at
 *                    once on this GPU.  Otherwise (any shard size) clv_run launches the sweep
 *                    kernel once per sweep and its fused level-2 tail exchanges the same way: the
 *                    chain's unit-last workgroups store this rank's unit partials into every rank's
 *                    mail, the chain's last one waits for all ranks' units in its own mail, sums
 *                    them in global order and draws — no host collective, no separate launches.
 *   clv_p2p_export:  this rank's mail buffer as a hipIpcMemHandle (CLV_IPC_HANDLE_BYTES bytes).
 *   clv_p2p_connect: every rank's mail: handles = [world][CLV_IPC_HANDLE_BYTES] (opened with
 *                    hipIpcOpenMemHandle; this rank's entry ignored) or ptrs = [world] device
 *                    pointers valid in this process (ranks sharing one process).  Collective in
 *                    effect: call it on every rank, then barrier, before the first clv_run.
 * After connecting, clv_run(n) runs n sweeps (bivariate: after the initial clv_hyper); every rank
 * must call it with the same n.  A rank that waits longer than the bound (10 s by default,
 * CLV_WAIT_TIMEOUT_MS) for its peers fails with CLV_EHIP and keeps its state from before the call;
 * ranks whose call completed undo it with clv_rollback, and clv_p2p_connect may be called again
 * (it refills this rank's mail) to resume the peer exchange.
 * A shard plan with an empty shard (no customers: clv_debug_world_has_empty_shard) takes the fused
 * exchange on every rank.  The empty rank launches one workgroup per chain that draws its level 2
 * from its mail; no rank waits for units of its, so the other ranks' hosts hold each sweep launch
 * until every empty rank has started the sweep before it (one host round trip per sweep, same bound).
 * clv_set_state and clv_rollback, which set the sweep count back, are called with every rank's
 * launches complete and the ranks brought back in step before the next clv_run, as after a connect. */
#define CLV_IPC_HANDLE_BYTES 64
int clv_p2p_info(const clv_sampler* s, int64_t* out);
int clv_p2p_export(clv_sampler* s, void* handle);
int clv_p2p_connect(clv_sampler* s, const void* handles, const uint64_t* ptrs);
/* Drop the peer connection (closes opened IPC mappings, forgets the peers' mail pointers): a sharded
 * clv_run then fails with CLV_ESTATE until clv_p2p_connect is called again.  Idempotent. */
int clv_p2p_disconnect(clv_sampler* s);
/* Which peer exchange clv_run takes on this shard: on = 1 the persistent kernel (only where its grid
 * fits: clv_p2p_info out[4] as created), 0 the fused exchange (one sweep launch per sweep).  Both
 * write the same mail with the same protocol and give the same bits; ShardedSampler falls back from
 * the first to the second (then to RCCL) when the verification against RCCL fails. */
int clv_p2p_set_persistent(clv_sampler* s, int32_t on);
/* Bound of every wait in the persistent / fused-exchange kernels, in ms (default 2000 at world size
 * 1, 10000 with peers; the CLV_WAIT_TIMEOUT_MS environment variable sets the default at create).
 * A short bound makes a failed peer-exchange check cheap (distributed.ShardedSampler's verification
 * runs under 500 ms). */
int clv_set_wait_timeout(clv_sampler* s, double ms);
/* Launch on another stream from now on (e.g. a stream under hipGraph capture by the caller,
 * who then replays the captured sweeps), and adjust the host's sweep count by n (+chunk per
 * replay; -chunk after a capture, which records launches without executing them). */
int clv_set_stream(clv_sampler* s, uint64_t stream);
int clv_note_sweeps(clv_sampler* s, int64_t n);

/* Outputs. level1: [chain][draw][n][D+2] (lambda, mu, tau, z, [eta]) — bi:407-410, tri:544-548;
 * level2: [chain][draw][D*K + D(D+1)/2] — bi:411-412, tri:549-554;
 * loglik: [chain][draw] per-draw mean of the likelihood term — bi:423-428.
 * Any pointer may be NULL. level1 requires draw_sink == CLV_SINK_FULL. */
int clv_read_draws(clv_sampler* s, double* level1, double* level2, double* loglik);
/* Stream the level-1 draws into the caller's host buffer while the sampler runs (world_size 1,
 * CLV_SINK_FULL) — the drop-in's end-to-end time, run_mcmc_abe.py:60-77 around bi:437-504, instead
 * of one pageable copy of every stored draw after the run.  level1: [chain][n_draws][n][D+2]
 * doubles, caller-owned, valid until clv_read_draws with the same pointer (or NULL here, or
 * clv_destroy).  Host threads of a process-wide copy pool first fault its pages in (madvise
 * MADV_POPULATE_WRITE), then each clv_run (its stored sweeps in sub-runs of >= 256 sweeps and ~64 MB
 * of draws) hands the draws it completed to the pool (pinned staging, DMA on the device's null
 * stream, which the sampler's non-blocking stream does not wait for) and goes on sampling;
 * clv_read_draws(s, level1, ...) waits for the copies in flight and copies what is left.  Same
 * launches, same sweeps, same bits.  NULL stops streaming (after the copies in flight). */
int clv_stream_draws(clv_sampler* s, double* level1);
/* [chain][CLV_N_SUM_STATS][n] running sums over stored draws, and the number of stored draws. */
int clv_read_summary(clv_sampler* s, double* sums, int64_t* n_stored);

/* Current state: lambda, mu [chain][n]; hyper [chain][beta K*D, Sigma D*D]. Setting the state
 * is exact resume (the Philox counter is the sweep index); lambdas and mus must be positive,
 * normal and finite (CLV_EINVAL otherwise: the sweep takes their logs, bi:286-287). */
int clv_get_state(clv_sampler* s, double* lambdas, double* mus, double* hyper);
int clv_set_state(clv_sampler* s, const double* lambdas, const double* mus, const double* hyper,
                  int64_t sweeps_done);

/* Per-launch timing of the sweep kernel with HIP events on the launch stream. */
int clv_set_timing(clv_sampler* s, int32_t enable);
int clv_kernel_time(clv_sampler* s, double* sweep_kernel_ms_total, int64_t* sweep_launches,
                    double* hyper_kernel_ms_total, int64_t* hyper_launches);

/* ---- test hooks (run the device code paths on caller data) ---- */
/* Host clock (steady_clock ns) at the steps of the last persistent clv_run at world size 1:
 * out[0] entry, [1] after hipSetDevice, [2] before the launch call, [3] after it, [4] launch
 * enqueued (end event recorded), [5] end seen, [6] return; 0 where not reached. */
int clv_debug_host_times(const clv_sampler* s, int64_t* out);
/* Philox4x32-10 on device: ctr/out are n x 4 words. */
int clv_debug_philox(uint32_t k0, uint32_t k1, const uint32_t* ctr, int64_t n, uint32_t* out);
/* The Philox-mode variates of one sweep for customers [0, n): t_l/t_m/u_acc are S x n;
 * log2_u_acc (S x n, may be NULL) is the accept threshold's log2 U exactly as the sweep kernels
 * form it (v_log_f32 of the fp32 uniform; bi:329-330 compares exp(lp' - lp) with U). */
int clv_debug_variates(uint64_t seed, int32_t chain, uint32_t sweep, int64_t n, int32_t n_steps,
                       float* t_l, float* t_m, float* u_acc, double* u_z, double* u_tau,
                       double* e_alive, double* eta_z, float* log2_u_acc);
/* The accept threshold's log2 U over the Philox words [w_begin, w_end) (<= 2^32), against float64
 * log2 of the same fp32 uniform: out[4] = max error in fp32 ulps of the exact value, max absolute
 * error, the word with the largest ulp error, max ulp error where U <= 1/2. */
int clv_debug_log2u_scan(uint64_t w_begin, uint64_t w_end, double* out);
/* The MH proposal's Student-t(3) transforms on caller words (n x 3 uint32: radius word of t_l,
 * radius word of t_m, angle word: t_l takes its high 16 bits, t_m its low 16 bits), as the sweep
 * kernels form them (packed 0: t3_f32, 1: the trivariate launch-per-sweep kernels' t3_pair).
 * Pins the proposal's symmetry (bi:316-317 draws Sigma[0,0] * standard_t(3)). */
int clv_debug_t3(const uint32_t* words, int64_t n, int32_t packed, float* t_l, float* t_m);
/* Level-2 draw from given sufficient statistics and variates (replaces bi:233-262 given rng):
 * xty K*D, yty D*D, iw_normal n_tril, iw_chi2 D, z D*K (standard normals) -> beta, Sigma. */
int clv_debug_level2(int32_t D, int32_t K, const clv_prior* prior, const double* xty,
                     const double* yty, const double* iw_normal, const double* iw_chi2,
                     const double* z, double* beta, double* sigma);
/* Diagnostic build only (make STAMPS=1 -> libclvmcmc_stamps.so): per-sweep s_memrealtime stamps
 * [1024][8] (slot = sweep % 1024); CLV_ESTATE in the shipped library. */
int clv_debug_stamps(clv_sampler* s, uint64_t* out);
/* Diagnostic build only: per workgroup of the latest sweep launch, [chain * n_blocks + 1 per chain]
 * records of 12 u64 (sweep kernel: start / end of customer work (s_memrealtime), HW_ID, XCC_ID,
 * s_memtime phase stamps; persistent kernel: s_memrealtime phase stamps of one sweep, see
 * kernels.hip CLV_P_STAMP); out must hold 12 * n_chains * (n_blocks + 1) values; CLV_ESTATE in
 * the shipped library. */
int clv_debug_wg_stamps(clv_sampler* s, uint64_t* out);
/* Philox-mode chi-square and normal draws of the hyper stream (n of each). */
int clv_debug_hyper_variates(uint64_t seed, int32_t chain, uint32_t sweep, double df, int64_t n,
                             double* chi2, double* normals);
/* The Philox-mode MH step's fp64 exp (csrc/fastmath.h, |x| <= 700) on n values. */
int clv_debug_exp(const double* x, int64_t n, double* out);
/* The Philox-mode fp64 log (csrc/fastmath.h log_fast, x > 0 normal) on n values: the z/tau
 * draw's logs (bi:200-225) and the eta normal's radius. */
int clv_debug_log(const double* x, int64_t n, double* out);
/* One Philox-mode MH step exactly as the sweep kernels run it (bi:291-335: log posterior with the
 * Q3 cap, fma + clip proposal, accept iff pm <= 5 and plp > cur + ln2 log2 U), on n independent
 * lanes.  Per lane: x, z, T_cal, tau, mean [n][2] (X @ beta), cur_pt [n][2] (log lambda, log mu),
 * t3 [n][2] (fp32 t3 noise), log_u = log2 U (fp32, as the sweeps draw it; +inf = a padded step);
 * shared prec3 = inv(Sigma)[0:2,0:2] as (p00, p01, p11) and scale2 = (Sigma00, Sigma11) (Q2).
 * out [n][7] = current log posterior (up to a per-customer constant), the proposal's (before the
 * Q3 cap), the proposal (pl, pm; pm clipped below only: one above 5 is rejected whatever it is),
 * the new log lambda, log mu and log posterior. */
int clv_debug_mh_step(int64_t n, const int32_t* x, const uint8_t* z, const double* T_cal, const double* tau,
                      const double* mean, const double* prec3, const double* cur_pt, const float* t3,
                      const double* scale2, const float* log_u, double* out);
/* Host only (no device): the persistent grid's placement map for n_chains chains of nb customer
 * workgroups (+1 level-2 workgroup each) on n_cu CUs — out[linear workgroup] = chain << 16 | block. */
int clv_debug_wg_map(int32_t n_chains, int32_t nb, int32_t n_cu, int32_t* out);
/* Host only: 1 if a persistent grid of grid_wgs workgroups is taken as resident at once on n_cu CUs
 * admitting blocks_per_cu of them each: min(blocks_per_cu, 8, the SGPR rule at 102 SGPRs) per CU,
 * less one slot per 32 CUs (MI355X guide, residency of 256-thread blocks), else 0. */
int clv_debug_persist_fits(int64_t grid_wgs, int32_t blocks_per_cu, int32_t n_cu);
/* Host only: 1 if clv_create runs a grid of grid_wgs persistent workgroups (n_chains chains of a
 * D / K model) on n_cu CUs: it fits (clv_debug_persist_fits) and few enough CUs hold two of its
 * workgroups for it to beat the launch-per-sweep kernel (capi.hip persist_worth, measured
 * crossover); CLV_PERSISTENT=1 forces it wherever it fits, =0 never. */
int clv_debug_persist_choice(int32_t D, int32_t K, int32_t n_chains, int64_t grid_wgs, int32_t blocks_per_cu,
                             int32_t n_cu);
/* Host only, the split layout of the persistent grid (n_chains chains of nb blocks of 256 customers,
 * 1 <= nb <= 256; a chain's 4 nb wave rows of 64 customers dealt six at a time to its workgroups).
 * clv_debug_split_fits: 1 if its n_chains x (ceil(2 nb / 3) + 1) one-per-CU workgroups are taken as
 * resident at once on n_cu CUs admitting blocks_per_cu (>= 1) each, less one CU per 64.
 * clv_debug_split_choice: fits, and the block layout would double up (n_chains x (nb + 1) > n_cu).
 * clv_debug_split_layout: out[physical workgroup][8] = chain, first wave row (-1: the chain's
 * level-2 workgroup), wave rows hosted, then the workgroup's two hand-off records as (kind, block):
 * kind 1 = four rows summed into the block's slot, 2 = rows 0, 1 summed into the block's slot (the
 * prefix of a split block), 3 = rows 2, 3 of a split block as two extension records, -1 = none;
 * out[.][7] = the first extension record's index in the chain's record table (kind 3), else -1.
 * clv_debug_split_relay_plan: the relay instance's division of a sweep's S (0..20) MH steps at relay
 * point R (0, 8 or 12) between a relayed row's owner and its relay wavefront, as [begin, end):
 * out[8] = steps run by the owner, by the relay wavefront, steps whose variates the owner draws, the
 * relay wavefront draws.  S <= R (or R = 0) is not relayed: the owner has all of it.
 * clv_debug_split_draw_plan: who draws the next sweep's variates in the relay instance at relay point R
 * (8 or 12) and draw share 0..5 (CLV_SPLIT_RELAY_DRAW: 0 nothing in the relay wavefronts' idle gaps,
 * 1 their own chunks after their row's reduction, 2 / 3 also one / two chunks of the rows on the
 * owner's SIMD before the flag, 4 / 5 those one / two chunks alone; 4 is built by default, DESIGN.md §8
 * round 9): out[row 0..5][chunk 0..4][4] = the wavefront that draws the chunk
 * first, its slot (0 the hand-off window, 1 gap 1 before the flag, 2 gap 2 after the row's reduction),
 * whether it is staged outside the pool, and the chunk's reader, which draws it in the window if the
 * gap ended first.  share = -1: out[0] = the share the library was built with.
 * clv_debug_split_stamps (CLV_STAMPS build): out[workgroup][16], the relay wavefronts' flag-seen and
 * row-done times of the stamped sweep (rows 4, 5), then HW_ID of wavefronts 0..7 (bits 5:4: SIMD),
 * then the end of the relay wavefronts' gap 1 (two words) and gap 2 (two words) in that sweep. */
int clv_debug_split_fits(int32_t n_chains, int32_t nb, int32_t blocks_per_cu, int32_t n_cu);
int clv_debug_split_choice(int32_t n_chains, int32_t nb, int32_t blocks_per_cu, int32_t n_cu);
int clv_debug_split_layout(int32_t n_chains, int32_t nb, int32_t* out);
int clv_debug_split_relay_plan(int32_t S, int32_t R, int32_t* out);
int clv_debug_split_draw_plan(int32_t R, int32_t share, int32_t* out);
int clv_debug_split_stamps(clv_sampler* s, uint64_t* out);
/* Host only: the sweep path clv_create decides on (the same function, no device and no environment),
 * from numbers.  in[20] = D, K, n_mh_steps, n_chains, local blocks, blocks_per_unit, n_units_global,
 * world_size, replay (0 / 1); the device's CUs (0: a query failed); workgroups per CU and scratch
 * bytes per lane of the block instance (the peer instance at world size > 1), of the split layout's
 * helper instance and of its relay instance (scratch -1: the query failed, -2: not queried yet);
 * CLV_PERSISTENT (-1 unset, 0, 1), CLV_PERSIST_LAYOUT (0 unset, 1 block, 2 split, -1 anything else),
 * CLV_SPLIT_RELAY (-1 unset, 0, 1, 2 anything else), CLV_DEFER (0: "0", else 1).
 * out[8] = persistent, split, relay_steps, p2p_capable, p2p_persist_fits, fx_capable, defer, and the
 * instances whose resources the decision still waits for (1 helper | 2 relay; their fields stay 0).
 * CLV_EINVAL with clv_create's message where clv_create rejects a knob. */
int clv_debug_sweep_plan(const int64_t* in, int32_t* out);
/* Host only: 1 if the shard plan (n_global, world_size, blocks_per_rank) leaves its last rank, and
 * maybe more, without customers.  clv_create then turns the persistent peer exchange off on every rank
 * of that world (the empty rank has no grid to keep resident): all of them take the fused exchange. */
int clv_debug_world_has_empty_shard(int64_t n_global, int32_t world_size, int32_t blocks_per_rank);

/* ---- In-process multi-device runs (SURVEY.md §8b devices=, §8e) ----
 * A group drives the n shards of one problem from one host thread: shards[r] = the sampler of rank
 * r of a world of n (clv_create with world_size n, blocks_per_rank / blocks_per_unit of the shard
 * plan, each on its own device or sharing one), all at the same sweep.  Per sweep the shards
 * exchange their unit partials (the all-gather of bi:243-255's statistics) either
 *   CLV_EXCHANGE_P2P:  every shard's persistent grid fits at once (on shared devices: together) and
 *                      distinct devices have peer access — clv_p2p_connect by device pointers, one
 *                      persistent launch per shard and call, all in flight before any is awaited;
 *   CLV_EXCHANGE_COPY: per sweep the sweep kernels, device-to-device copies of each shard's unit
 *                      partials into every shard's gathered buffer (stream-ordered by events), and
 *                      every shard's level-2 draw.
 * CLV_EXCHANGE_AUTO picks P2P where possible and no two shards share a device (their persistent
 * kernels would have to run concurrently from different streams, which HIP does not promise); the
 * group disconnects the shards it connected when destroyed.  Results are bitwise those of the unsharded run.  A
 * P2P call that times out on any shard is undone on the others and redone by copies (kept).
 * clv_group_run is synchronous; the bivariate initial draw (bi:393 of sweep 1) is its first
 * exchange.  The group does not own the shards (destroy the group first). */
enum { CLV_EXCHANGE_AUTO = 0, CLV_EXCHANGE_P2P = 1, CLV_EXCHANGE_COPY = 2 };
typedef struct clv_group clv_group;
int clv_group_create(clv_sampler* const* shards, int32_t n, int32_t exchange, clv_group** out);
int clv_group_run(clv_group* g, int64_t n_sweeps);
int32_t clv_group_exchange(const clv_group* g);
void clv_group_destroy(clv_group* g);

/* ---- Posterior analysis on device ----
 * Inputs are level-1 draws [n_draws][n][width] in the reference's layout, chains stacked
 * (np.vstack of draws["level_1"]); width 4 = (lambda, mu, tau, z), 5 = (+ eta).  The plain
 * variants take host arrays (uploaded, device = ordinal or -1 for the current one); the
 * *_sampler variants use the draws a CLV_SINK_FULL sampler holds in HBM after its run. */
enum {
  CLV_L1_MEAN_LAMBDA = 0, CLV_L1_LAMBDA_P025, CLV_L1_LAMBDA_P975, CLV_L1_MEAN_MU, CLV_L1_MEAN_MU_CAPPED,
  CLV_L1_MU_P025, CLV_L1_MU_P975, CLV_L1_MEAN_Z, CLV_L1_MEAN_TAU, CLV_L1_MEAN_ETA, CLV_N_L1_STATS
};
/* Posterior predictive future transactions: bivariate/mcmc.py:506-546 (draw_future_transactions)
 * and, with simulate_spend = 1 (width 5), the lognormal spend totals of trivariate/mcmc.py:660-749.
 * x_future int64 [n_draws][n]; spend_future float64 [n_draws][n] or NULL. */
int clv_predict(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                const double* T_cal, double T_star, uint64_t seed, int32_t simulate_spend, double sigma_s,
                int64_t* x_future, double* spend_future);
int clv_predict_sampler(clv_sampler* s, double T_star, uint64_t seed, int32_t simulate_spend,
                        double sigma_s, int64_t* x_future, double* spend_future);
/* Weekly tracking curve of bivariate/analysis_abe.py:444-464: for each week t of `times`
 * (ascending), the mean over draws of the posterior-predictive number of repeat transactions of
 * the customers active in that week (birth_week < t <= birth_week + tau).  inc_weekly [n_times]. */
int clv_track(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
              const double* birth_week, const double* times, int32_t n_times, uint64_t seed,
              double* inc_weekly);
int clv_track_sampler(clv_sampler* s, const double* birth_week, const double* times, int32_t n_times,
                      uint64_t seed, double* inc_weekly);
/* Per-customer posterior statistics (out [n][CLV_N_L1_STATS]): means as numpy's axis-0 mean,
 * capped-mu mean min(mu, mu_cap) and numpy-'linear' 2.5/97.5 percentiles of lambda and mu —
 * utils/analysis_bi_helpers.py:15-27 (post_mean_*) and :75-107 (compute_table4). */
int clv_level1_summary(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                       double mu_cap, double* out);
/* The _sampler variant also serves a CLV_SINK_SUMMARY_PCT sampler (no level-1 draws kept): means
 * from its running sums (pooled over chains), percentiles from its float32 (lambda, mu) store;
 * mu_cap must then be CLV_SUMMARY_MU_CAP. */
int clv_level1_summary_sampler(clv_sampler* s, double mu_cap, double* out);
/* Mean over draws of the total log-likelihood incl. -lgamma(x+1) (analysis_bi_helpers.py:52-72). */
int clv_chain_total_loglik(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                           const int32_t* x, const double* T_cal, double* mean_total);
int clv_chain_total_loglik_sampler(clv_sampler* s, double* mean_total);

/* ---- Posterior customer lifetime value and customer equity (csrc/ltv.hip) ----
 * What Abe (2015) derives from the level-1 draws.  Per stacked draw and customer, with
 * a = mu + delta (delta the continuous discount rate per time unit of the data), H the horizon in
 * that unit (infinity allowed) and m the value per transaction — eta * value_scale for width 5,
 * monetary[i] (1 when monetary is NULL: discounted expected transactions, "DERT") for width 4:
 *   value    = (lambda m) / a                      H infinite (multiply, divide: no other rounding)
 *            = ((lambda m) (-expm1(-(a H)))) / a   H finite
 *   residual = z value                             the value left after T_cal
 * out_customers [n][CLV_N_LTV_STATS], over the draws: mean (sum in draw order / n_draws), sd
 * (numpy's std, ddof 1: NaN at one draw) and numpy-'linear' 2.5 / 50 / 97.5 percentiles of value
 * and of residual; the means of z, of 1 / (periods_per_year mu) (expected lifetime in years) and of
 * exp(-periods_per_year mu) (one-year survival).
 * out_draws [n_draws][CLV_N_LTV_DRAW_STATS], over the customers: equity = sum residual,
 * value_total = sum value, n_alive = sum z, mu_share = (sum mu / a) / n — every sum in the fixed
 * order of clv_pnbd_eval (zero-padded 256-customer blocks by the 256-tree, the block partials by
 * the same scheme), so the bits do not depend on the launch geometry or the customer batch.
 * CLV_EINVAL before any device call: a bad level-1 shape (n_draws, n < 1, width not 4 or 5, more
 * than 2^22 stacked draws), delta negative or not finite, horizon <= 0 or NaN, value_scale or
 * periods_per_year not finite, monetary given with width 5, a null pointer.  The _sampler variant
 * uses the draws a CLV_SINK_FULL sampler holds in HBM (CLV_ESTATE as clv_predict_sampler). */
enum {
  CLV_LTV_VALUE_MEAN = 0, CLV_LTV_VALUE_SD, CLV_LTV_VALUE_P025, CLV_LTV_VALUE_P50, CLV_LTV_VALUE_P975,
  CLV_LTV_RESIDUAL_MEAN, CLV_LTV_RESIDUAL_SD, CLV_LTV_RESIDUAL_P025, CLV_LTV_RESIDUAL_P50, CLV_LTV_RESIDUAL_P975,
  CLV_LTV_P_ALIVE, CLV_LTV_LIFETIME_YRS, CLV_LTV_SURVIVAL_1YR, CLV_N_LTV_STATS
};
enum {
  CLV_LTV_DRAW_EQUITY = 0, CLV_LTV_DRAW_VALUE_TOTAL, CLV_LTV_DRAW_N_ALIVE, CLV_LTV_DRAW_MU_SHARE,
  CLV_N_LTV_DRAW_STATS
};
int clv_lifetime_value(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                       const double* monetary /* NULL or [n] */, double delta, double horizon /* inf allowed */,
                       double value_scale, double periods_per_year, double* out_customers, double* out_draws);
int clv_lifetime_value_sampler(clv_sampler* s, const double* monetary, double delta, double horizon,
                               double value_scale, double periods_per_year, double* out_customers,
                               double* out_draws);
/* The limits of csrc/ltv.hip: out[0] customers per reduction block (256), out[1] draws per LDS
 * tile of the transposing pass, out[2] keys per sort batch, out[3] the most stacked draws, out[4]
 * draws per LDS tile of the sd kernel.  The
 * environment variable CLV_LTV_BATCH (customers, rounded up to whole blocks) lowers the customer
 * batch: a test knob, the results do not depend on it.
 * CLV_DIAG_BATCH (series) likewise lowers the series batch of clv_diagnostics, clv_rank_diagnostics and clv_autocorr.
 * CLV_SUMMARY_BATCH (customers) likewise lowers the customer batch of clv_level1_summary's percentile sort. */
int clv_ltv_info(int64_t* out);

/* ---- Model comparison: pointwise log-likelihood, WAIC and PSIS-LOO (csrc/ic.hip) ----
 * The pointwise log-likelihood of customer i under stacked draw d is the Pareto/NBD individual
 * likelihood given (lambda, mu), marginal over z and tau, in the form that cannot overflow; with
 * ml = lambda + mu:
 *   l = ((x log(lambda) - log(ml)) - ml t_x) + log(mu + lambda exp(-(ml (T_cal - t_x))))
 * and, with log_s given (width 5 only; omega2 > 0), one observation of log_s ~ N(log eta, omega2):
 *       + (-log(2 pi omega2) / 2 - (log_s - log eta)^2 / (2 omega2)).
 * log_s NULL on a width-5 array compares the transaction part only.
 * Per customer over the S = n_draws values (out [n][CLV_N_IC_STATS]):
 *   lppd = logsumexp(l) - log S, p_waic = var(l) (ddof 0), elpd_waic = lppd - p_waic;
 *   PSIS (Vehtari, Gelman & Gabry 2017, as ArviZ): log ratios r = -l, x = r - max r,
 *   M = ceil(min(S / 5, 3 sqrt(S / reff))), cutoff = max((M + 1)-th largest x, log(DBL_MIN)), tail =
 *   every x > cutoff (tail_len of them, at most M); a tail of 5 or more is fitted with Zhang &
 *   Stephens' generalised Pareto estimator (pareto_k, shrunk towards 0.5 by a prior worth 10
 *   values) and replaced by the fit's quantiles, every log weight capped at 0 and normalised;
 *   a shorter tail or a non-finite fit keeps the raw weights and reports pareto_k = +infinity;
 *   elpd_loo = logsumexp(log weight + l), p_loo = lppd - elpd_loo.
 * A customer with a non-finite l has NaN in all its columns.  Every sum has a fixed order (ic.hip):
 * the results do not depend on the launch geometry or the customer batch; no atomics.
 * CLV_EINVAL before any device call: a null pointer, n_draws < 8 or > 2^20, n < 1, width not 4 or
 * 5, log_s with width 4, omega2 not in (0, inf) with log_s, reff not in (0, inf) or so small that M
 * exceeds 4096. */
enum {
  CLV_IC_LPPD = 0, CLV_IC_P_WAIC, CLV_IC_ELPD_WAIC, CLV_IC_ELPD_LOO, CLV_IC_P_LOO, CLV_IC_PARETO_K,
  CLV_IC_TAIL_LEN, CLV_N_IC_STATS
};
/* out [n_draws][n]. */
int clv_pointwise_loglik(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                         const int32_t* x, const double* t_x, const double* T_cal,
                         const double* log_s /* NULL: no spend term */, double omega2, double* out);
/* The statistics of any caller-supplied matrix loglik [n_draws][n]. */
int clv_psis_loo(int32_t device, const double* loglik, int64_t n_draws, int64_t n, double reff, double* out);
/* clv_pointwise_loglik and clv_psis_loo fused (the same bits): the matrix stays on the device. */
int clv_information_criteria(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                             const int32_t* x, const double* t_x, const double* T_cal, const double* log_s,
                             double omega2, double reff, double* out);
/* From the draws a CLV_SINK_FULL sampler holds in HBM and the data it was created with (spend != 0:
 * its log_s; CLV_ESTATE as clv_predict_sampler). */
int clv_information_criteria_sampler(clv_sampler* s, int32_t spend, double omega2, double reff, double* out);
/* The limits of csrc/ic.hip: out[0] customers per workgroup of the pass (256), out[1] draws per LDS
 * tile of its transpose, out[2] keys per sort batch, out[3] the fewest and out[4] the most stacked
 * draws, out[5] the longest tail, out[6] the shortest tail that is fitted. */
int clv_ic_info(int64_t* out);
/* clv_information_criteria with batch_keys (> 0: keys per sort batch, whole 256-customer blocks, at
 * least one) and grid (> 0: the most workgroups per launch) overridden: the tests' knobs, the
 * results do not depend on them. */
int clv_debug_information_criteria(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                                   const int32_t* x, const double* t_x, const double* T_cal, const double* log_s,
                                   double omega2, double reff, int64_t batch_keys, int32_t grid, double* out);

/* ---- Scoring customers outside the fit (csrc/score.hip, kernels.hip score_kernel) ----
 * Given (beta, Sigma) customers are conditionally independent, so a customer the fit never saw has
 *   p(theta_i | y_i, fit) = integral p(theta_i | y_i, beta, Sigma) p(beta, Sigma | fit) d(beta, Sigma):
 * the level-1 half of the sweep — draw_z, draw_tau (bi:193-227), the MH steps on (log lambda, log mu)
 * (bi:268-339) and draw_eta (tri:306-333) — run against the fit's stored level-2 records instead of a
 * live level-2 draw.  level2 is [n_chains][n_draws][D K + D (D + 1) / 2], a row being beta.T.ravel()
 * then Sigma's upper triangle (bi:411-412, tri:549-554: what clv_read_draws returns).  For chain c
 * and new customer i one shadow chain runs from init_*[c][i]: warmup inner sweeps against record 0
 * (nothing recorded), then inner_sweeps against every record d in turn, the state after the last
 * of them being draw d.  Inner sweep number t (1-based from sweep_first, warm-up counted) is the
 * production Philox-mode level-1 sweep with n_mh_steps MH steps, key chain_key(seed + chain_first +
 * c) and counter (customer_offset + i, t, slot, customer stream): the result is a function of
 * (seed, chain, global customer index, t) alone, whatever the batch or the grid.  A call with
 * init_* = an earlier call's state_*_out, warmup = 0 and sweep_first = that call's last t + 1
 * continues it exactly.
 * (beta, Sigma) is held fixed during a record's inner sweeps (a two-stage, "cut" analysis).  With
 * all of a chain's records equal the scheme is exactly invariant for any inner_sweeps; when they
 * vary, theta enters record d distributed for record d - 1, a bias that fades with inner_sweeps and
 * with the narrowness of the level-2 posterior (measured: DESIGN.md §4h).
 * Host pointers.  x [n] int32; t_x, T_cal [n]; cov [(K - 1)][n] (NULL for K = 1); log_s [n] and
 * omega2 > 0 for D = 3 (log_s NULL for D = 2); init_lam, init_mu, state_lam_out, state_mu_out
 * [n_chains][n] (the final state is always written).  sink = CLV_SINK_FULL: level1_out
 * [n_chains][n_draws][n][D + 2] = (lambda, mu, tau, z, [eta]), the layout of clv_read_draws;
 * CLV_SINK_SUMMARY: sums_out [n_chains][CLV_N_SUM_STATS][n], the CLV_SUM_* sums over the records in
 * record order from zero (the log sums are logs of the recorded natural-scale draws; eta sums zero
 * for D = 2) — nothing per record leaves the registers, so millions of customers x thousands of
 * records fit.  The other output may be NULL.
 * CLV_EINVAL before any device call: a null pointer, D not 2 or 3, K not 1 .. 9, n_chains or n_draws
 * < 1, n <= 0, cov / log_s that do not match (D, K), omega2 not in (0, inf) for D = 3, n_mh_steps or
 * warmup < 0, inner_sweeps < 1, a sink other than the two, the sink's output NULL, init not finite
 * and positive, x < 0, t_x outside [0, T_cal], non-finite data or records, a record with a
 * non-positive variance, customer_offset + n or the last inner-sweep number beyond 32 bits.
 * CLV_ENOMEM (before anything is allocated) when the sink does not fit in device memory. */
int clv_score_customers(int32_t device, int32_t D, int32_t K, int32_t n_chains, int64_t n_draws,
                        const double* level2, int64_t n, const int32_t* x, const double* t_x,
                        const double* T_cal, const double* cov, const double* log_s, double omega2,
                        int32_t n_mh_steps, int32_t warmup, int32_t inner_sweeps, uint64_t seed,
                        int32_t chain_first, int64_t customer_offset, int64_t sweep_first,
                        const double* init_lam, const double* init_mu, int32_t sink, double* level1_out,
                        double* sums_out, double* state_lam_out, double* state_mu_out);
/* The same from the level-2 records a sampler holds in HBM after its run (any draw sink; CLV_ESTATE
 * before every record is stored, and for a replay-mode sampler): D, K, n_chains, n_draws, omega2 and
 * the chain keys' chain_first are the sampler's. */
int clv_score_customers_sampler(clv_sampler* s, int64_t n, const int32_t* x, const double* t_x,
                                const double* T_cal, const double* cov, const double* log_s,
                                int32_t n_mh_steps, int32_t warmup, int32_t inner_sweeps, uint64_t seed,
                                int64_t customer_offset, int64_t sweep_first, const double* init_lam,
                                const double* init_mu, int32_t sink, double* level1_out, double* sums_out,
                                double* state_lam_out, double* state_mu_out);
/* out[0] customers per workgroup (256), out[1] CLV_N_SUM_STATS; of the instance the calling thread's
 * last clv_score_customers* call launched (-1 before one): out[2] D, out[3] K, out[4] sink, out[5]
 * VGPRs and out[6] scratch bytes per lane (hipFuncGetAttributes), out[7] the kernel's device time
 * in ns (events around the launch). */
int clv_score_info(int64_t* out);
/* The prepare kernel alone (tests): out [n_rec][64], the hyper block the score kernel reads for each
 * record of level2 [n_rec][D K + D (D + 1) / 2] — beta[k][d] at k D + d, Sigma 3 x 3 row-major at 27,
 * inv(Sigma)[0:2, 0:2] = (P00, P01, P11) at 36 .. 38, the proposal scales Sigma00, Sigma11 at 39, 40,
 * and for D = 3 Sigma22, post_var, sqrt(post_var), omega2, 1 / omega2, 1 / Sigma22 at 41 .. 46. */
int clv_debug_score_hyper(int32_t device, int32_t D, int32_t K, int64_t n_rec, const double* level2,
                          double omega2, double* out);

/* ---- Closed-form holdout predictive distribution and forecast scores (csrc/forecast.hip) ----
 * The number of purchases X* of customer i (x, t_x, T_cal) in (T_cal, T_cal + T_star] given stacked
 * draw d's (lambda, mu), marginal over z and tau (the conditioning of the pointwise likelihood
 * above).  With ml = lambda + mu, D = T_cal - t_x, E = exp(-(ml D)), t = T_star, y = ml t,
 * r = lambda / ml, w = mu / ml:
 *   p_alive(d, i) = (ml E) / (mu + lambda E)
 *   pmf_alive(k)  = exp(-y) (lambda t)^k / k!  +  w r^k P(k + 1, y)     (P: regularised lower incomplete gamma)
 *   pmf(d, i, k)  = p_alive pmf_alive(k) + (1 - p_alive) [k = 0],  k = 0 ... k_max - 1
 *   mean(d, i)    = p_alive (lambda / mu) (-expm1(-(mu t)))
 * A customer's posterior predictive is the mean over the draws: the draws are added in the order
 * d = 0, 1, ..., n_draws - 1, one plain float64 addition each, into an accumulator that starts at
 * zero, and the sum is divided by n_draws once.  One lane owns a customer and nothing else adds to
 * its accumulators: the order depends on n_draws only, not on the launch geometry or the customer
 * batch; no atomics.  Columns of out [n][CLV_N_FC_STATS], F the cumulative sum of the mean pmf in k
 * order: xstar_mean; p_alive; p_zero = pmf(0); q05, q50, q95 (the smallest k with F(k) >= p, k_max
 * if F never reaches p); tail_mass = max(0, 1 - F(k_max - 1)); and, NaN without x_star,
 * log_score = log pmf(x*), pit_lo = F(x* - 1), pit_hi = F(x*), rps = sum_k (F(k) - [k >= x*])^2.
 * out_pmf (or NULL) takes the mean pmf [n][k_max]; out has the same bits with and without it.
 * A draw whose lambda or mu is not in (0, inf), or whose lambda + mu overflows, marks the customer:
 * NaN in every column and in its pmf row.
 * CLV_EINVAL before any device call: a null pointer, n_draws < 1 or > 2^31 - 1, n < 1 or > 2^31 - 1,
 * width not 4 or 5, T_star not in (0, inf), k_max not in [1, 4096], an x_star[i] outside [0, k_max). */
enum {
  CLV_FC_XSTAR_MEAN = 0, CLV_FC_P_ALIVE, CLV_FC_P_ZERO, CLV_FC_Q05, CLV_FC_Q50, CLV_FC_Q95, CLV_FC_TAIL_MASS,
  CLV_FC_LOG_SCORE, CLV_FC_PIT_LO, CLV_FC_PIT_HI, CLV_FC_RPS, CLV_N_FC_STATS
};
int clv_forecast(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width, const int32_t* x,
                 const double* t_x, const double* T_cal, double T_star, int32_t k_max,
                 const int32_t* x_star /* NULL or [n] */, double* out, double* out_pmf /* NULL or [n][k_max] */);
/* From the draws a CLV_SINK_FULL sampler holds in HBM and the data it was created with (CLV_ESTATE
 * as clv_predict_sampler); x_star, out and out_pmf on the host. */
int clv_forecast_sampler(clv_sampler* s, double T_star, int32_t k_max, const int32_t* x_star, double* out,
                         double* out_pmf);
/* The limits of csrc/forecast.hip: out[0] customers per workgroup (256), out[1] the largest k_max
 * (4096), out[2] the most stacked draws, out[3] the cap on the terms of the series that starts the
 * recurrence at k_max - 1, out[4] the accumulator doubles of one customer batch by default. */
int clv_forecast_info(int64_t* out);
/* clv_forecast with batch_customers (> 0: customers per accumulator batch, rounded up to whole
 * 256-customer blocks) and grid (> 0: the most workgroups per launch) overridden: the tests' knobs,
 * the results do not depend on them. */
int clv_debug_forecast(int32_t device, const double* level1, int64_t n_draws, int64_t n, int32_t width,
                       const int32_t* x, const double* t_x, const double* T_cal, double T_star, int32_t k_max,
                       const int32_t* x_star, int64_t batch_customers, int32_t grid, double* out, double* out_pmf);

/* ---- Posterior predictive checks of the calibration data (csrc/ppc.hip) ----
 * One replicate (x_rep, t_x_rep) of every customer's calibration data (x, t_x) on (0, T_cal] per
 * stacked draw d (chains stacked chain-major).  Philox4x32-10 keyed by the seed (low word, high
 * word), counter (customer_offset + i, d, slot, 5):
 *   level 0 (customer):   lambda = level1[d][i][0], mu = level1[d][i][1].
 *   level 1 (population): (beta, Sigma) = record d of level2 [n_draws][D K + D (D + 1) / 2] (the layout
 *     of clv_score_customers; only beta's first two columns and Sigma's leading 2 x 2 block are read);
 *     m_j = sum_k X_ik beta_kj, k ascending, X_i0 = 1; l00 = sqrt(S00), l10 = S01 / l00,
 *     l11 = sqrt(S11 - l10^2); (n0, n1) = sqrt(-2 log(u53_open0(x, y))) (cos, sin)(2 pi u53(z, w)) of
 *     slot 1; lambda = exp(m0 + l00 n0), mu = exp((m1 + l10 n0) + l11 n1).
 *   slot 0: E = -log(u53_open0(x, y)), U = u53_open0(z, w); tau = E / mu (may be +inf);
 *     alive = tau > T_cal; L = alive ? T_cal : tau.
 *   x_rep = Poisson(lambda L) from slots 16 + attempt (0 for a mean <= 0 or NaN, inversion below 10,
 *     PTRS from 10, at most 2^16 steps or attempts);
 *   t_x_rep = x_rep > 0 ? L exp(log(U) / x_rep) : 0  (the largest of x_rep uniform times on (0, L]).
 * No multiply-add is contracted.  out_customers [n][CLV_N_PPC_STATS], over the S = n_draws draws:
 * x_rep_mean = (int64 sum) / S, p_x_lt = #(x_rep < x) / S, p_x_eq, p_zero = #(x_rep = 0) / S,
 * tx_rep_mean = (the sum of t_x_rep in draw order from zero) / S, p_tx_le = #(t_x_rep <= t_x) / S,
 * p_alive_rep = #(alive) / S.  out_draws_int [n_draws][k_hist + 1 + CLV_N_PPC_DRAW_INTS], over the
 * customers: the histogram of x_rep in bins 0 ... k_hist - 1 and a last bin for x_rep >= k_hist, then
 * sum x_rep, sum x_rep^2, max x_rep and the number alive (integer atomics: exact in any order).
 * out_draws_f [n_draws][CLV_N_PPC_DRAW_FLOATS]: sum t_x_rep in the fixed order of
 * clv_lifetime_value's per-draw sums (zero-padded 256-customer blocks by the 256-tree, the block
 * partials by the same scheme): its bits depend neither on the grid nor on the customer batch.
 * out_x_rep / out_tx_rep (either may be NULL) take the replicates [n_draws][n]; the other outputs have
 * the same bits with and without them.  Host pointers; cov [(K - 1)][n] (NULL for K = 1).
 * CLV_EINVAL before any device call: a null pointer, level not 0 or 1, n_draws or n < 1 or
 * > 2^31 - 1, width not 4 or 5 (level 0), D not 2 or 3, K not 1 .. 9 or cov not matching K (level 1),
 * k_hist not in [1, 4096], customer_offset < 0 or customer_offset + n beyond 32 bits. */
enum {
  CLV_PPC_X_REP_MEAN = 0, CLV_PPC_P_X_LT, CLV_PPC_P_X_EQ, CLV_PPC_P_ZERO, CLV_PPC_TX_REP_MEAN, CLV_PPC_P_TX_LE,
  CLV_PPC_P_ALIVE_REP, CLV_N_PPC_STATS
};
enum { CLV_PPC_DRAW_SUM_X = 0, CLV_PPC_DRAW_SUM_X2, CLV_PPC_DRAW_MAX_X, CLV_PPC_DRAW_N_ALIVE, CLV_N_PPC_DRAW_INTS };
enum { CLV_PPC_DRAW_SUM_TX = 0, CLV_N_PPC_DRAW_FLOATS };
int clv_ppc(int32_t device, int32_t level,
            const double* level1, int32_t width,          /* level 0; NULL at level 1 */
            const double* level2, int32_t D, int32_t K,   /* level 1; NULL at level 0 */
            const double* cov /* [K - 1][n] or NULL */,
            int64_t n_draws, int64_t n, const int32_t* x, const double* t_x, const double* T_cal,
            int32_t k_hist, uint64_t seed, int64_t customer_offset,
            double* out_customers, int64_t* out_draws_int, double* out_draws_f,
            int64_t* out_x_rep /* NULL or [n_draws][n] */, double* out_tx_rep /* NULL or [n_draws][n] */);
/* From the draws (level 0) or the level-2 records (level 1) a CLV_SINK_FULL sampler holds in HBM and
 * the data and covariates it was created with (CLV_ESTATE as clv_predict_sampler); the counter's
 * customer word starts at the sampler's shard_begin.  The outputs on the host. */
int clv_ppc_sampler(clv_sampler* s, int32_t level, int32_t k_hist, uint64_t seed, double* out_customers,
                    int64_t* out_draws_int, double* out_draws_f, int64_t* out_x_rep, double* out_tx_rep);
/* The limits of csrc/ppc.hip: out[0] customers per workgroup and per reduction block (256), out[1]
 * the largest k_hist (4096), out[2] the t_x_rep doubles of one customer batch by default; of the
 * replicate kernel the calling thread's last clv_ppc* call launched (-1 before one): out[3] VGPRs and
 * out[4] scratch bytes per lane (hipFuncGetAttributes), out[5] the device time of the call's kernels
 * in ns (events around them). */
int clv_ppc_info(int64_t* out);
/* clv_ppc with batch_customers (> 0: customers per batch, rounded up to whole 256-customer blocks)
 * and grid (> 0: the most workgroups per launch) overridden: the tests' knobs, the results do not
 * depend on them — nor on the environment variable CLV_PPC_ITEM_DRAWS (draws per work item of the
 * replicate kernel, whole 32-draw chunks, default 32: the profile's knob, every clv_ppc* call). */
int clv_debug_ppc(int32_t device, int32_t level, const double* level1, int32_t width, const double* level2,
                  int32_t D, int32_t K, const double* cov, int64_t n_draws, int64_t n, const int32_t* x,
                  const double* t_x, const double* T_cal, int32_t k_hist, uint64_t seed, int64_t customer_offset,
                  double* out_customers, int64_t* out_draws_int, double* out_draws_f, int64_t* out_x_rep,
                  double* out_tx_rep, int64_t batch_customers, int32_t grid);

/* ---- The marginal likelihood and marginal WAIC / PSIS-LOO (csrc/marginal.hip) ----
 * Nothing in the reference: it replaces az.loo / az.waic on a log-likelihood that is marginal over the
 * customer's own parameters (Merkle, Furr & Rabe-Hesketh 2019), which needs a quadrature per
 * (customer, level-2 record).  Per record r of level2 [n_records][D K + D (D + 1) / 2] (the layout of
 * clv_score_customers) and customer i:
 *   l_marg[r][i] = log int int L(x_i, t_x,i, T_i | lambda, mu) N2((log lambda, log mu); m_i, Sigma_12) dlog lambda dlog mu
 * m_ij = sum_k X_ik beta_kj, k ascending, X_i0 = 1; cov [(K - 1)][n] (NULL for K = 1).  With log_s
 * (D = 3 only) the integrand is multiplied by N(log_s_i; m_i3 + c (theta - m_i,12), v), c = Sigma_3,12
 * Sigma_12^-1, v = Sigma_33 - c Sigma_12,3 + omega2: one observation log_s ~ N(log eta, omega2) with eta
 * integrated out analytically.  With D = 3 and log_s NULL only beta's first two columns and Sigma's
 * leading 2 x 2 block are read.  The dropped-out and the alive component of L (both log-concave in
 * theta) are integrated separately and joined by logaddexp; each by CLV_MARGINAL_NEWTON damped Newton
 * steps from m_i to its mode and the adaptive Gauss-Hermite rule of `nodes` points per dimension
 * (8, 16, 24, 32; 0 = CLV_MARGINAL_DEFAULT_NODES) centred there and scaled by the Cholesky factor of
 * the inverse negative Hessian (csrc/marginal.hip's header has every operation in order; no
 * multiply-add is contracted).  out [n_records][n]: the (S, N) layout of clv_pointwise_loglik.  A
 * record whose Sigma_12 is not positive definite (or whose v is not positive), or a non-finite
 * input, gives NaN in that cell alone.  Each cell is a function of that customer and that record
 * only: the bits depend neither on the grid nor on how the customers are batched or sharded.
 * CLV_EINVAL before any device call: a null pointer, D not 2 or 3, K not 1 .. 9, cov not matching K,
 * log_s with D = 2, omega2 not finite and > 0 with log_s, nodes not 0, 8, 16, 24 or 32, n_records or
 * n < 1, n_records > 2^20, n > 2^31 - 1. */
#define CLV_MARGINAL_DEFAULT_NODES 32
#define CLV_MARGINAL_NEWTON 16
int clv_marginal_loglik(int32_t device, const double* level2, int32_t D, int32_t K,
                        const double* cov /* [K - 1][n] or NULL */, int64_t n_records, int64_t n, const int32_t* x,
                        const double* t_x, const double* T_cal, const double* log_s /* NULL: no spend term */,
                        double omega2, int32_t nodes, double* out);
/* clv_marginal_loglik and clv_psis_loo fused (the same bits): the matrix stays on the device.  out
 * [n][CLV_N_IC_STATS]; a customer with a NaN cell is NaN in all seven.  Also CLV_EINVAL: n_records
 * outside clv_psis_loo's range of draws, reff not finite and > 0 or giving too long a tail. */
int clv_marginal_information_criteria(int32_t device, const double* level2, int32_t D, int32_t K, const double* cov,
                                      int64_t n_records, int64_t n, const int32_t* x, const double* t_x,
                                      const double* T_cal, const double* log_s, double omega2, int32_t nodes,
                                      double reff, double* out);
/* From the level-2 records a sampler holds in HBM after its run and the data and covariates it was
 * created with (CLV_ESTATE as clv_ppc_sampler at level 1; spend != 0 needs a trivariate sampler). */
int clv_marginal_information_criteria_sampler(clv_sampler* s, int32_t spend, double omega2, double reff, int32_t nodes,
                                              double* out);
/* out[0 .. 3] the supported orders, out[4] the default, out[5] the Newton steps per component, out[6]
 * customers per workgroup (256), out[7] the most records; of the kernel the calling thread's last
 * clv_marginal* call launched (-1 before one): out[8] VGPRs and out[9] scratch bytes per lane
 * (hipFuncGetAttributes), out[10] the device time of the call's quadrature kernels in ns. */
int clv_marginal_info(int64_t* out);
/* clv_marginal_loglik with batch_customers (> 0: customers per launch, rounded up to whole
 * 256-customer blocks) and grid (> 0: the most workgroups per launch) overridden — the tests' knobs,
 * the results do not depend on them — and out_centre (NULL or [n_records][n][12]): per component,
 * the dropped-out one first, the centre (log lambda, log mu), the three entries L00, L10, L11 of the
 * scale and the first Newton step that moved neither coordinate by 1e-9 (CLV_MARGINAL_NEWTON if none). */
int clv_debug_marginal_loglik(int32_t device, const double* level2, int32_t D, int32_t K, const double* cov,
                              int64_t n_records, int64_t n, const int32_t* x, const double* t_x, const double* T_cal,
                              const double* log_s, double omega2, int32_t nodes, int64_t batch_customers, int32_t grid,
                              double* out, double* out_centre);

/* ---- The log-normal Pareto/NBD by maximum marginal likelihood (csrc/mml.hip) ----
 * The objective is sum_i w_i l_i with l_i = clv_marginal_loglik's cell of customer i under the one
 * record (beta [2][K], then Sigma_00, Sigma_01, Sigma_11: D = 2, 2K + 3 doubles), bit for bit, and its
 * score comes from the customer's posterior moments by Fisher's identity: with (da, db) = (log lambda,
 * log mu) - m_i and P = Sigma^-1, d l_i / d m_i = P E_i[(da, db)] and d l_i / d Sigma = P (S_i - Sigma) P / 2,
 * S_i = E_i[(da, db)(da, db)'].  The moments are sums over the nodes of the quadrature that forms l_i:
 * the score is the derivative of the quadrature value at fixed nodes.
 * clv_mml_create copies x, t_x, T, weights (NULL: all 1) and cov [K - 1][n] (NULL for K = 1) to the
 * device, where they stay until clv_mml_destroy.  cov is not checked for finiteness: a customer with a
 * non-finite covariate has a NaN row.
 * clv_mml_eval: sums[2K + 6] = sum w l, sum w, the customers whose l is not finite (also
 * *n_nonfinite, which may be NULL), sum w S_i (00, 01, 11), sum w d_ik E_i[da] for k < K, then sum w d_ik
 * E_i[db] for k < K (d_i0 = 1), in the fixed order of clv_pnbd_eval (zero-padded 256-customer blocks
 * by the 256-tree, the block partials by the final kernel): the same bits on every call and grid.  A
 * non-finite customer makes the sums NaN; none is dropped.
 * clv_mml_customers: out[n][8] = l_i, P(alive | data, record), E_i[da], E_i[db], E_i[da da], E_i[da db],
 * E_i[db db] and E[X*(t_star) | data, record], the expected purchases in (T, T + t_star].
 * clv_debug_mml_eval: clv_mml_eval with the most workgroups overridden (grid > 0), the tests' knob.
 * clv_mml_info: out[0] customers and out[1] lanes per workgroup; VGPRs and scratch bytes per lane of
 * the eval kernel (out[2], out[3]) and of the customers kernel (out[4], out[5]); out[6] the device time in
 * ns of the eval kernel of the calling thread's last clv_mml_eval (-1 before one).
 * CLV_EINVAL: a null handle or pointer, K not 1 .. 9, cov not matching K, x < 0, t_x outside [0, T], a
 * negative or non-finite weight, nodes not 0, 8, 16, 24 or 32, t_star negative or not finite. */
typedef struct clv_mml clv_mml;
int clv_mml_create(int32_t device, int64_t n, const int32_t* x, const double* t_x, const double* T,
                   const double* weights, int32_t K, const double* cov, clv_mml** out);
void clv_mml_destroy(clv_mml* h);
int clv_mml_eval(clv_mml* h, const double* record, int32_t nodes, double* sums, int64_t* n_nonfinite);
int clv_mml_customers(clv_mml* h, const double* record, int32_t nodes, double t_star, double* out);
int clv_debug_mml_eval(clv_mml* h, const double* record, int32_t nodes, int32_t grid, double* sums,
                       int64_t* n_nonfinite);
int clv_mml_info(int64_t* out);

/* ---- Convergence diagnostics on device (csrc/diag.hip) ----
 * The reference checks convergence with ArviZ on its level-2 draws (bivariate/analysis_abe.py:
 * 651-706: az.summary, az.plot_autocorr).  Here a series is m chains x n draws (n >= 8) of one
 * quantity, optionally logged first, and its statistics are six doubles: mean and sd (ddof 1) over
 * all m n values; the split-chain R-hat and the mean effective sample size of BDA3 / Stan / ArviZ
 * WITHOUT rank normalisation (each chain split into its first and last n / 2 draws, biased
 * autocovariances averaged over the 2 m split chains, Geyer's initial positive sequence truncated
 * at lag T and made monotone, tau floored at 1 / log10(2 m (n / 2))); mcse = sd / sqrt(ess); and
 * the truncation lag T (-1 when no pair was accepted).  All six are NaN for a series with a
 * non-finite value (after the log) or zero within-chain variance — a customer whose z never
 * changes.  az.summary reports the rank-normalised variants (bulk / tail ESS, rank R-hat): those
 * are clv_rank_diagnostics below; this estimator is meant for the scales the sampler works on —
 * log lambda, log mu and the level-2 parameters.
 *   series: [chain][draw][n_series] — level-2 draws [chain][draw][P] as they are, level-1 draws
 *           [chain][draw][n][D+2] with n_series = n (D+2);  out: [n_series][CLV_N_DIAG_STATS].
 *   Series s is logged when bit s % period of log_mask is set (period 1..32; level 1: D+2).
 * clv_diagnostics_sampler works on the draws a sampler holds in HBM after its run, without a host
 * copy: level1_out [n (D+2)][6] (CLV_SINK_FULL only, log_mask over the D+2 columns; CLV_ESTATE as
 * the other *_sampler entry points), level2_out [D K + D(D+1)/2][6] (never logged); either may be
 * NULL.  Same kernels and summation order as clv_diagnostics: the same bits.
 * clv_autocorr: acf_c(t) = A_c(t) / A_c(0) of every unsplit chain, A_c(t) = (1/n) sum_i c[i] c[i+t]
 * centred at the chain mean, t = 0..max_lag (< n_draws); out [chain][n_series][max_lag + 1].
 * CLV_EINVAL before any device call: null pointer, n_chains < 1, n_draws < 8, n_series < 1,
 * period outside 1..32, max_lag outside 0..n_draws-1. */
enum {
  CLV_DIAG_MEAN = 0, CLV_DIAG_SD, CLV_DIAG_MCSE, CLV_DIAG_ESS, CLV_DIAG_RHAT, CLV_DIAG_LAG, CLV_N_DIAG_STATS
};
int clv_diagnostics(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                    int32_t period, uint32_t log_mask, double* out);
int clv_diagnostics_sampler(clv_sampler* s, uint32_t log_mask, double* level1_out, double* level2_out);
int clv_autocorr(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                 int32_t max_lag, double* out);

/* ---- Rank-normalised diagnostics on device (csrc/diag.hip) ----
 * The remaining columns of az.summary (hdi, mcse_sd, ess_bulk, ess_tail, r_hat), after Vehtari,
 * Gelman, Simpson, Carpenter & Buerkner (2021) as ArviZ implements them; same input, logging and
 * limits as clv_diagnostics, thirteen doubles per series.  With y the (logged) m x n series,
 * h = n / 2, the 2 m split chains y[c][0..h) and y[c][n-h..n) (an odd n drops its middle draw),
 * S = 2 m h pooled split values, and ESS(.), Rhat(.), lag the estimator of clv_diagnostics applied
 * to split chains:
 *   z(s)         Phi^-1((r - 3/8) / (S + 1/4)), r the average 1-based rank of s in the pool (ties
 *                share the mean of their positions); Phi^-1 is Wichura's AS241 (PPND16)
 *   RHAT_BULK    Rhat(z(split y));  ESS_BULK = ESS(z(split y)), LAG_BULK its truncation lag
 *   RHAT_FOLDED  Rhat(z(|split y - med|)), med the median of the S split values
 *   RHAT         max(RHAT_BULK, RHAT_FOLDED): az.summary's r_hat
 *   ESS_Q05/Q95  ESS(split I(y <= q_p)), q_p numpy's default (linear) quantile of all m n values
 *   ESS_TAIL     min(ESS_Q05, ESS_Q95)
 *   ESS_SD       ESS(split (y - mean)^2);  MCSE_SD = sqrt(varvar / evar / 4) with evar = mean((y -
 *                mean)^2), varvar = (mean((y - mean)^4) - evar^2) / ESS_SD
 *   HDI_LO/HI    with the m n values sorted and k = floor(hdi_prob m n): (x[i], x[i+k]) for the
 *                first i < m n - k that minimises x[i+k] - x[i]
 *   MEDIAN       of all m n values
 * NaN: a series with a non-finite value (after the log) is NaN in all thirteen; otherwise a
 * statistic is NaN exactly when its own transformed split series has no within-chain variance
 * (MCSE_SD also when evar == 0), RHAT and ESS_TAIL when either of their two components is;
 * HDI_* and MEDIAN are always finite.  A binary series (z) has a finite ESS_BULK but usually a
 * NaN ESS_Q95: its indicator is all ones.
 * A series of up to CLV_RANK_LDS_ELEMS values (m n) is sorted and transformed in LDS (two buffers
 * of that many doubles and the workgroup's scalars: 64 KiB, two workgroups per CU); longer series
 * take the same code on global-memory scratch.  Every sum runs in an order fixed by (m, n): the
 * _sampler entry gives the same bits as the host-array one; CLV_ESTATE as clv_diagnostics_sampler.
 * clv_debug_zscale: ranks and z of the split values (folded: of |split y - med|), [n_series][2 m][h]
 * each in split-chain order (chain 0 first half, chain 0 second half, chain 1 first half, ...).
 * CLV_EINVAL before any device call: as clv_diagnostics, and hdi_prob outside (0, 1). */
#define CLV_RANK_LDS_ELEMS 4080
enum {
  CLV_RANK_RHAT = 0, CLV_RANK_RHAT_BULK, CLV_RANK_RHAT_FOLDED, CLV_RANK_ESS_BULK, CLV_RANK_ESS_TAIL,
  CLV_RANK_ESS_Q05, CLV_RANK_ESS_Q95, CLV_RANK_ESS_SD, CLV_RANK_MCSE_SD, CLV_RANK_HDI_LO, CLV_RANK_HDI_HI,
  CLV_RANK_MEDIAN, CLV_RANK_LAG_BULK, CLV_N_RANK_STATS
};
int clv_rank_diagnostics(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                         int32_t period, uint32_t log_mask, double hdi_prob, double* out);
int clv_rank_diagnostics_sampler(clv_sampler* s, uint32_t log_mask, double hdi_prob, double* level1_out,
                                 double* level2_out);
int clv_debug_zscale(int32_t device, const double* series, int32_t n_chains, int64_t n_draws, int64_t n_series,
                     int32_t folded, double* ranks_out, double* z_out);

/* ---- Data preparation on device ----
 * Event log -> CBS (utils/elog2cbs2param.py:33-94): events (cust, date in ns since the epoch,
 * sales or NULL = 1) -> one row per customer with calibration events, sorted by cust.  Output
 * buffers hold n_events rows (upper bound); *n_customers rows are written.  Hold-out columns
 * (T_star, x_star, sales_star) are meaningful when T_cal_ns < T_tot_ns. */
int clv_elog2cbs(int32_t device, int64_t n_events, const int64_t* cust, const int64_t* date_ns, const double* sales,
                 int64_t unit_ns, int64_t T_cal_ns, int64_t T_tot_ns, int64_t* n_customers, int64_t* cust_out,
                 int64_t* x, double* t_x, double* litt, double* sales_out, double* sales_x, int64_t* first_ns,
                 double* T_cal, double* T_star, int64_t* x_star, double* sales_star);
/* Synthetic Abe (2009) data (bivariate/mcmc.py:95-187): covariates [1, U(-1,1)...] (or the
 * caller's [n][K] incl. intercept), theta = exp(X beta + MVN(0, gamma)), tau ~ Exp(mu), purchases
 * as a Poisson process until min(T_cal + max T_star, tau); CBS of bi:75-89 and hold-out counts
 * x_star[n_star][n].  beta K x 2 row-major, gamma 2 x 2, T_cal[n].  n_events = elog rows per
 * customer; with elog_offsets (exclusive prefix sum of n_events from a first call) a second call
 * also writes the elog (cust 1-based, t). */
int clv_generate_pareto_abe(int32_t device, int64_t n, int32_t K, const double* beta, const double* gamma,
                            const double* covars, const double* T_cal, int32_t n_star, const double* T_star,
                            uint64_t seed, int64_t* x, double* t_x, double* lambda_true, double* mu_true,
                            double* tau_true, uint8_t* alive_true, int64_t* x_star, double* covars_out,
                            int64_t* n_events, const int64_t* elog_offsets, int64_t elog_rows, int64_t* elog_cust,
                            double* elog_t);

/* ---- Pareto/NBD maximum-likelihood baseline on device (csrc/pnbd.hip) ----
 * The classical Pareto/NBD the reference fits with lifetimes.ParetoNBDFitter and compares both HB
 * models against: bivariate/analysis_abe.py:205-217 (fit, conditional expected purchases for the
 * Table 2 rows) and :426-438 (the birth-aligned "Pareto/NBD (MLE)" curve of Figure 2);
 * full_analysis.py:245, :437.  params = (r, alpha, s, beta), all > 0 and finite (CLV_EINVAL
 * otherwise).  Per customer x (repeat count), t_x, T with 0 <= t_x <= T:
 *   L = Gamma(r+x) alpha^r beta^s / Gamma(r) { (alpha+T)^-(r+x) (beta+T)^-s + s I },
 *   I = int_{t_x}^{T} (alpha+y)^-(r+x) (beta+y)^-(s+1) dy,
 * evaluated through an Euler-transformed hypergeometric series of positive terms that stops when
 * its remainder bound is below 2^-53 of the sum, or after 2048 terms (z = |alpha - beta| /
 * (max(alpha, beta) + t) up to about 0.98).  A customer that reaches the cap is counted, and its
 * values are NaN: nothing is truncated silently.
 * A handle keeps x, t_x, T and the optional weights (NULL = 1) on the device for the evaluations
 * of a fit; creating one fails with CLV_EINVAL for n <= 0, a null column, a negative x or weight,
 * t_x outside [0, T] or a non-finite value.
 * The eval entry writes sums[6] = sum w log L, its derivatives with respect to (log r, log alpha,
 * log s, log beta), sum w; *n_unconverged (may be NULL) = customers at the term cap, sums[0] is NaN
 * then.  Sums are per-256-customer block partials added in a fixed order: the same bits on every
 * call.  The customers entry writes out[n][3] = log L, P(alive | x, t_x, T), E[Y(t_star) | x, t_x,
 * T] (t_star >= 0).  The track entry writes cum[j] = sum_i E[X(max(times[j] - birth_week[i], 0))],
 * E[X(t)] = r beta / alpha (1 - (beta / (beta + t))^(s-1)) / (s - 1), reduced in the same fixed
 * order for every time; n_times in 1..65535. */
typedef struct clv_pnbd clv_pnbd;
int clv_pnbd_create(int32_t device, int64_t n, const int32_t* x, const double* t_x, const double* T,
                    const double* weights, clv_pnbd** out);
void clv_pnbd_destroy(clv_pnbd* h);
int clv_pnbd_eval(clv_pnbd* h, const double* params, double* sums, int64_t* n_unconverged);
int clv_pnbd_customers(clv_pnbd* h, const double* params, double t_star, double* out);
int clv_pnbd_track(int32_t device, int64_t n, const double* birth_week, const double* times, int32_t n_times,
                   const double* params, double* cum);

/* ---- Pareto/NBD with time-invariant covariates (csrc/pnbd.hip) ----
 * Fader & Hardie (2007), "Incorporating time-invariant covariates into the Pareto/NBD and BG/NBD
 * models", equations (1) and (2): alpha_i = alpha0 exp(-gamma1' z1_i), beta_i = beta0
 * exp(-gamma2' z2_i); the likelihood of customer i is the Pareto/NBD L above at (r, alpha_i, s,
 * beta_i) (their equation 3).  params = (r, alpha0, s, beta0, gamma1[k1], gamma2[k2]): the first
 * four > 0 and finite, the coefficients finite (CLV_EINVAL otherwise).
 * clv_pnbd_set_covariates copies z1 [k1][n] and z2 [k2][n] (row k = covariate k of every customer,
 * the sampler's layout) into the handle; 0 <= k1, k2 <= 8, every value finite (CLV_EINVAL
 * otherwise, and the handle keeps what it had).  k1 = k2 = 0 is allowed.  The _cov entries are
 * CLV_EINVAL on a handle without covariates.
 * clv_pnbd_eval_cov: sums[6 + k1 + k2] = the six sums of clv_pnbd_eval, then sum_i w_i g_logalpha,i
 * (-z1[k][i]) for k < k1 and sum_i w_i g_logbeta,i (-z2[k][i]) for k < k2: d sum w log L / d gamma
 * by the chain rule, g the score with respect to log alpha_i and log beta_i.  Every sum in the fixed
 * order of clv_pnbd_eval; with every gamma = 0 (or k1 = k2 = 0) the first six are its bits.
 * clv_pnbd_customers_cov: out[n][7] = log L_i, P(alive), E[Y(t_star) | x, t_x, T, z_i] (the three
 * columns of clv_pnbd_customers at (r, alpha_i, s, beta_i)) and the score d log L_i / d log(r,
 * alpha_i, s, beta_i).
 * clv_pnbd_track_cov: cum[j] = sum_i E[X(max(times[j] - birth_week[i], 0)) | z_i], E[X(t) | z_i] =
 * r beta_i / alpha_i (1 - (beta_i / (beta_i + t))^(s-1)) / (s - 1) (Fader & Hardie 2007, the
 * Pareto/NBD expectation at alpha_i, beta_i), in the fixed order of clv_pnbd_track. */
int clv_pnbd_set_covariates(clv_pnbd* h, int32_t k1, const double* z1, int32_t k2, const double* z2);
int clv_pnbd_eval_cov(clv_pnbd* h, const double* params, double* sums, int64_t* n_unconverged);
int clv_pnbd_customers_cov(clv_pnbd* h, const double* params, double t_star, double* out);
int clv_pnbd_track_cov(int32_t device, int64_t n, const double* birth_week, const double* times, int32_t n_times,
                       const double* params, int32_t k1, const double* z1, int32_t k2, const double* z2, double* cum);

/* Discounted expected residual transactions (Fader, Hardie & Lee 2005, "RFM and CLV", equation 14,
 * with Psi(s, s; z) z^(s-1) written as e^z E_s(z) and a finite horizon):
 *   DERT_i = P(alive)_i (r + x_i) / (alpha_i + T_i) J_i,
 *   J_i = int_0^H exp(-delta t) (B_i / (B_i + t))^s dt,  B_i = beta_i + T_i,
 * at params as clv_pnbd_eval_cov takes them (a handle without covariates: four parameters).  J is
 * integrated itself, by 16-point Gauss-Legendre panels of a positive integrand (DESIGN.md section
 * 4m): no difference of two E_s, no series in s.  delta >= 0 and finite, horizon > 0 or +inf; an
 * infinite horizon needs delta > 0 (CLV_EINVAL otherwise).  out[n][2] = P(alive), DERT.
 * clv_dert_integral evaluates J alone for n rows of (s, B, delta, horizon): the kernel's device
 * function under test. */
int clv_pnbd_dert(clv_pnbd* h, const double* params, double delta, double horizon, double* out);
int clv_dert_integral(int32_t device, int64_t n, const double* s, const double* B, const double* delta,
                      const double* horizon, double* out);

/* ---- The integral I past the series' term cap (csrc/pnbd.hip) ----
 * The series of clv_pnbd_eval needs about 36.7 / (-ln z) terms, z = |alpha_i - beta_i| /
 * (max(alpha_i, beta_i) + t): 2,048 terms end at z of about 0.98, and a covariate that moves
 * alpha_i / beta_i by orders of magnitude passes that.  The second evaluation integrates I itself by
 * 16-point Gauss-Legendre panels of a positive integrand in d = log((m + y) / (m + t_x)), m =
 * min(alpha_i, beta_i), measured from the lower limit; the gradient is taken under the integral at the
 * same nodes.  It converges for every z < 1 and forms no difference of two series.
 * clv_pnbd_set_integral chooses, per handle, how clv_pnbd_eval, _eval_cov, _customers,
 * _customers_cov and clv_pnbd_dert evaluate I:
 *   CLV_PNBD_INTEGRAL_SERIES      the series for every customer: the default, and the behaviour of a
 *                                 handle that never called this entry, bit for bit (NaN and a count at
 *                                 the term cap);
 *   CLV_PNBD_INTEGRAL_AUTO        the series, with the same bits, for a customer with z(t_x) <= 0.9, the
 *                                 quadrature for every other customer with t_x < T;
 *   CLV_PNBD_INTEGRAL_QUADRATURE  the quadrature for every customer with t_x < T.
 * In the last two modes a customer is counted in *n_unconverged only when a result is not finite (an
 * alpha_i that underflowed to 0).  CLV_EINVAL for another mode or a null handle, before any device
 * call. */
enum {
  CLV_PNBD_INTEGRAL_SERIES = 0,
  CLV_PNBD_INTEGRAL_AUTO = 1,
  CLV_PNBD_INTEGRAL_QUADRATURE = 2
};
int clv_pnbd_set_integral(clv_pnbd* h, int32_t mode);

/* ---- Gamma-Gamma spend model by maximum likelihood (csrc/gg.hip) ----
 * Fader, Hardie & Lee (2005), "RFM and CLV", and Fader & Hardie (2013), "The Gamma-Gamma model of
 * monetary value", equation (1a): customer i with mean spend m_i > 0 over n_i >= 1 transactions,
 *   log L_i = lnGamma(p n + q) - lnGamma(p n) - lnGamma(q) + q ln gamma + (p n - 1) ln m + p n ln n
 *             - (p n + q) ln(gamma + n m),
 * params = (p, q, gamma), all > 0 and finite.  clv_gg_create is CLV_EINVAL on n_i < 1, m_i <= 0 or a
 * negative or non-finite weight.  clv_gg_eval: sums[5] = sum w log L, its derivatives with respect
 * to log(p, q, gamma), sum w, in the fixed order of clv_pnbd_eval.  clv_gg_customers: out[n][4] =
 * log L_i and d log L_i / d log(p, q, gamma).  lnGamma(p n + q) - lnGamma(p n) and psi(p n + q) -
 * psi(p n) are each one function (Stirling's series differenced term by term from 32 on), so a
 * heavy buyer loses no digits.  clv_digamma evaluates the device digamma (upward shift to 10, then
 * the asymptotic series) on n positive arguments: the kernel's device function under test. */
typedef struct clv_gg clv_gg;
int clv_gg_create(int32_t device, int64_t n, const int32_t* frequency, const double* monetary, const double* weights,
                  clv_gg** out);
void clv_gg_destroy(clv_gg* h);
int clv_gg_eval(clv_gg* h, const double* params, double* sums);
int clv_gg_customers(clv_gg* h, const double* params, double* out);
int clv_digamma(int32_t device, int64_t n, const double* x, double* out);

/* ---- Many small fits in one launch (csrc/batch.hip) ----
 * Replaces a host loop of whole runs, bi:346-431 / tri:465-574 once per fit and chain: n_fits
 * independent problems of one (D, K), each with its own customers, prior constants and seed, are
 * uploaded together, run by ONE kernel launch and read back; no handle outlives the call.  One
 * 256-thread workgroup per (fit, chain) runs that chain from the initial state (bi:367-379,
 * tri:488-504) through all burnin + mcmc sweeps: per sweep it walks the fit's tiles of CLV_BLOCK
 * customers in order (z bi:388, tau bi:390, level-1 MH bi:396, eta tri:524-526, storage
 * bi:402-428), writes each tile's block partial, and draws level 2 (bi:393, tri:529) from the
 * partials summed in the fixed order of every other path — so fit j's outputs are, bit for bit,
 * those of clv_create + clv_run + clv_read_draws / clv_read_summary on fit j alone with
 * chain_first = 0 (production Philox mode).  No workgroup waits for another.
 * Per fit (clv_batch_item, host pointers): n in [1, 512 CLV_BLOCK], seed, the CBS columns,
 * covariates [(K - 1)][n] (NULL for K = 1), log_s (D = 3 only), the prior; outputs level1
 * [chain][n_draws][n][D + 2] (CLV_SINK_FULL), level2 [chain][n_draws][D K + D (D + 1) / 2], loglik
 * [chain][n_draws], sums [chain][CLV_N_SUM_STATS][n] (CLV_SINK_SUMMARY; all n_draws stored draws
 * are in them), and, optional, the final state state_lam / state_mu [chain][n].
 * draw_sink: CLV_SINK_FULL, CLV_SINK_SUMMARY or CLV_SINK_NONE.  *kernel_ms (may be NULL): the
 * kernel's device time by hipEvents.  CLV_EINVAL before any allocation when the buffers of the
 * sink exceed the free device memory (hipMemGetInfo); the message names the bytes needed.
 * clv_batch_plan (host only): seg_offsets [n_fits + 1] customers before each fit in the
 * concatenated arrays, tiles [n_fits], wg_map [n_fits * n_chains][2] = (fit, chain) of every
 * workgroup, fits with the most tiles first (stable).
 * clv_batch_info: out[5] = VGPRs, scratch bytes per lane, workgroups per CU of the (D, K)
 * instance, slots = CUs x workgroups per CU, CUs (of the current device). */
typedef struct clv_batch_item {
  int64_t n;
  uint64_t seed;
  const int32_t* x;
  const double* t_x;
  const double* T_cal;
  const double* covariates;
  const double* log_s;
  const clv_prior* prior;
  double* level1;
  double* level2;
  double* loglik;
  double* sums;
  double* state_lam;
  double* state_mu;
} clv_batch_item;
int clv_batch_fit(int32_t device, int32_t D, int32_t K, int32_t n_mh_steps, int32_t n_chains, int32_t burnin,
                  int32_t mcmc, int32_t thin, int32_t draw_sink, int64_t n_fits, const clv_batch_item* fits,
                  double* kernel_ms);
int clv_batch_plan(int64_t n_fits, const int64_t* n, int32_t n_chains, int64_t* seg_offsets, int32_t* tiles,
                   int32_t* wg_map);
int clv_batch_info(int32_t D, int32_t K, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* CLVMCMC_H */
