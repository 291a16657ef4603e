/* hmcx.h — C ABI of the MI355X-native SG-HMC engine (libhmcx.so).
 *
 * The reference (sherna90/dropout_hamiltonian_montecarlo) has no FFI: its boundary is a
 * duck-typed Python protocol.  This header is the boundary the Python host
 * layer (dropout_hamiltonian_montecarlo_amd/hamiltonian/...) binds through ctypes; each
 * entry point names the reference interface it replaces.
 *
 * Conventions
 *  - All array pointers are DEVICE pointers (caller-owned, e.g. torch tensors), row-major
 *    and contiguous, unless the comment says "host".
 *  - C independent chains are stored chain-interleaved so the two gradient GEMMs see one
 *    [rows x C*K] matrix: weights W[D][C][K], bias b[C][K]  (C = 1 is exactly the
 *    reference's {'weights': [D,K], 'bias': [K]} layout).  The SGHMC / SGLD samplers
 *    (hmcx_sampler_args), the multi-chain full-batch HMC (hmcx_hmc_chains_args, the
 *    reference's hmc_multicore) and the random-walk Metropolis sampler (hmcx_mh_args, the
 *    reference's metropolis.py) use it; per-(step, chain) schedules and outputs are indexed
 *    s*C + c, Philox streams by chain id chain0 + c.
 *  - dtype: HMCX_F64 (the reference's float64) or HMCX_F32.
 *  - Return 0 on success or a negative hmcx_status; hmcx_last_error() has the message.
 *    No C++ exception crosses the ABI.  A context is bound to one device, owns its
 *    workspace and (unless hmcx_set_stream is used) its HIP stream; it is not thread-safe.
 *  - Every call is asynchronous on the context stream; results are ready after
 *    hmcx_synchronize() (or any stream-ordered consumer).
 */
#ifndef HMCX_H
#define HMCX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hmcx_ctx hmcx_ctx;

enum hmcx_dtype { HMCX_F32 = 0, HMCX_F64 = 1 };
enum hmcx_noise { HMCX_NOISE_BUFFER = 0, HMCX_NOISE_PHILOX = 1 };
enum hmcx_status {
  HMCX_OK = 0,
  HMCX_EINVAL = -1,       /* bad argument / shape */
  HMCX_EHIP = -2,         /* HIP runtime error */
  HMCX_ENOMEM = -3,       /* device allocation failed */
  HMCX_EUNSUPPORTED = -4  /* shape/dtype combination not built */
};

/* ------------------------------------------------------------------ context */
int hmcx_version(void);
int hmcx_create(int device, hmcx_ctx** out);
int hmcx_destroy(hmcx_ctx* ctx);
const char* hmcx_last_error(const hmcx_ctx* ctx);
/* Run on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the legacy
 * default stream.  A new context runs on its own non-blocking stream until this is called. */
int hmcx_set_stream(hmcx_ctx* ctx, void* hip_stream);
int hmcx_synchronize(hmcx_ctx* ctx);
/* Capture each hmcx_*_run call into a hipGraph and replay it (1) or launch eagerly (0). */
int hmcx_set_graph_mode(hmcx_ctx* ctx, int enabled);
/* SGHMC implementation: 0 = auto (persistent single-launch kernel when C == 1 and the shape
 * fits, else kernel-per-phase), 1 = kernel-per-phase, 2 = persistent only (error otherwise). */
int hmcx_set_sghmc_path(hmcx_ctx* ctx, int path);
/* Look-ahead of the persistent single-chain SGHMC launch: 0 = off, 1 = on, 2 = auto (the default).  With
 * look-ahead the launch carries two chain teams ("lanes") on disjoint halves of the device; step s + 1 runs
 * at the same time as step s under the assumption that s rejects, and is run again from the true state
 * when s accepted — every step that counts performs the same arithmetic in the same order, so results do
 * not depend on the mode.  It pays while most proposals are rejected.  A shape where the second lane does
 * not fit, and a call with out_trace, run without it.  Auto starts with look-ahead on and follows
 * hmcx_p2_ahead_rule over the accept flags reported through hmcx_sghmc_ahead_note: flags of calls that
 * have finished, handed over by the caller when it reads them, so nothing blocks (a caller that never
 * reports stays on).  The environment variable HMCX_P2_AHEAD=<0|1|2>, read per call, overrides the mode. */
int hmcx_set_sghmc_ahead(hmcx_ctx* ctx, int mode);
int hmcx_sghmc_ahead_note(hmcx_ctx* ctx, const int32_t* accepted /* host [n] */, int n);
/* The auto rule (host arithmetic only): the next launch's mode from the last launch's (`on`) and the
 * accept flags of the last `seen` resolved steps (at most 32), `accepted` of them set.  Fewer than 16
 * steps decide nothing; look-ahead goes off above an accept rate of 0.4 and on again below 0.3. */
int hmcx_p2_ahead_rule(int on, int seen, int accepted);
/* Look-ahead counters of the context's latest persistent SGHMC launch (waits for it): out[0] = speculative
 * runs that were voided and run again, out[1] = those of them that were stopped in flight, at a leapfrog
 * boundary, once the other lane's verdict had arrived, out[2] = leapfrog iterations so skipped.  All zero
 * before the first launch and after a launch without look-ahead.  Timing-dependent: results never are. */
int hmcx_sghmc_ahead_stats(hmcx_ctx* ctx, long long out[3]);
/* Parked steps of the same launch (look-ahead; HMCX_P2_RUNON=0, read per call, turns parking off): a lane
 * whose speculative run ends with the other lane's verdict still unknown, and leaves the state as it was,
 * starts its next step at once and resolves the verdict while that runs.  out[0] = steps so parked, out[1] =
 * those of them whose verdict came back "changed" (the step and the run started on it are run again).
 * Zero and timing-dependent as above. */
int hmcx_sghmc_run_on_stats(hmcx_ctx* ctx, long long out[2]);
/* Device timing of sampler runs: when enabled, HIP events on the launch stream bracket the
 * kernels of every hmcx_sghmc_run / hmcx_sgld_run call (for the persistent SGHMC path: exactly
 * its one kernel launch).  Enabling (or disabling) resets the totals; hmcx_get_timing waits
 * for the last bracketed run and returns the summed kernel time and the number of runs. */
int hmcx_set_timing(hmcx_ctx* ctx, int enabled);
int hmcx_get_timing(hmcx_ctx* ctx, double* kernel_ms, long long* launches);

/* Philox4x32-10 uniforms in [0,1), bit-identical to the device generator (host function). */
void hmcx_philox_uniforms(uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot,
                          uint32_t n, double* out /* host [n] */);
/* Philox standard normals for slot/element range (host function; used by tests): the float32
 * Box–Muller stream of the f32 chains. */
void hmcx_philox_normals(uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot,
                         uint32_t e0, uint32_t n, double* out /* host [n] */);
/* The float64 stream of the f64 chains (53-bit uniforms, double Box–Muller; host function).
 * Replaces the f64 draws of cpu/sghmc.py:21,31 and cpu/sgld.py:45 in noise='philox' mode. */
void hmcx_philox_normals_f64(uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot,
                             uint32_t e0, uint32_t n, double* out /* host [n] */);

/* ------------------------------------------------------------------ softmax model
 * Replaces hamiltonian/models/cpu/softmax.py:45-61 (grad) and gpu/softmax.py:53-69.
 * X [B][D], Y [B][K] one-hot (dtype), W [D][C*K], b [C*K]  ->  gW [D][C*K], gb [C*K]
 * grad = -(Xᵀ(Y - softmax(clip(XW+b))) - alpha*theta)                                  */
int hmcx_softmax_grad(hmcx_ctx* ctx, int dtype, const void* X, const void* Y, int B, int D, int K,
                      int C, const void* W, const void* b, double alpha, void* gW, void* gb);

/* Replaces softmax.py:63-72 (log_likelihood): ll[c] = Σ_rows Σ_k y·(z − logsumexp z), z = clip(XW+b).
 * ll: device double[C]. */
int hmcx_softmax_loglik(hmcx_ctx* ctx, int dtype, const void* X, const void* Y, int B, int D, int K,
                        int C, const void* W, const void* b, double* ll);

/* Replaces softmax.py:38-43,82-89 (net / predict(prob=True)): prob [B][C*K]. */
int hmcx_softmax_predict(hmcx_ctx* ctx, int dtype, const void* X, int B, int D, int K, int C,
                         const void* W, const void* b, void* prob);

/* ------------------------------------------------------------------ logistic model
 * Replaces hamiltonian/models/cpu/logistic.py:24-72 (K = 1; the GPU file models/gpu/logistic.py is
 * its CuPy twin).  X [B][D], y [B] (dtype, 0/1), W [D][C], b [C] (C independent parameter sets, C = 1
 * is the reference's {'weights': [D,1], 'bias': [1]}).
 * net = sigmoid(clip(XW + b)) = 1/(1 + exp(−z)) (:43-55);  grad = −(Xᵀ(y − net) − alpha·θ) (:24-41). */
int hmcx_logistic_grad(hmcx_ctx* ctx, int dtype, const void* X, const void* y, int B, int D, int C,
                       const void* W, const void* b, double alpha, void* gW, void* gb);
/* ll[c] = Σ_rows y·log(net) + (1 − y)·log(1 − net)  (:64-72), device double[C].  HMCX_F32 takes both
 * logarithms from the clipped logit z (log net = min(z, 0) − log1p(exp(−|z|)), log(1 − net) likewise at −z):
 * a float32 net is exactly 1 from z = 16.64 on, far inside the clip bound. */
int hmcx_logistic_loglik(hmcx_ctx* ctx, int dtype, const void* X, const void* y, int B, int D, int C,
                         const void* W, const void* b, double* ll);
/* prob [B][C] = net (predict(prob=True) of :75-87, before batching). */
int hmcx_logistic_predict(hmcx_ctx* ctx, int dtype, const void* X, int B, int D, int C, const void* W,
                          const void* b, void* prob);
/* out[0] = Σ x² (float64 accumulation, fixed order): the θ-dependent part of logistic.log_prior
 * (:15-21).  x device [n] (dtype), out device double[1]. */
int hmcx_sumsq(hmcx_ctx* ctx, int dtype, const void* x, int64_t n, double* out);

/* ------------------------------------------------------------------ momentum SGD (sgd.fit)
 * Replaces hamiltonian/inference/cpu/sgd.py:25-45 (fit) and :47-70 (fit_dropout) for the softmax
 * and logistic models: per minibatch s (rows row0[s] .. +B of X / Y)
 *   g = model.grad(θ, X_s, Y_s);  m = gamma·m − step_size·g;  θ += m      (sgd.py:38-41)
 * with X_s replaced by X_s ⊙ Z (Z ∈ {0,1}^{B×D}) when dropout is set (sgd.py:61-63).  Z comes from
 * keep (device uint8, B·D per step from keep_off[s]; BUFFER: the host's np.random.binomial draws)
 * or from Philox (PHILOX: Z = u < keep_p, u = Philox(seed, 0, step_base + s, 0xFFFFFFFC, element)). */
enum hmcx_model { HMCX_MODEL_SOFTMAX = 0, HMCX_MODEL_LOGISTIC = 1 };
typedef struct hmcx_sgd_args {
  int dtype;
  int model;               /* hmcx_model                                                  */
  int B, D, K, n_steps;    /* K = 1 for the logistic model                                */
  double alpha;            /* prior precision (hyper['alpha'])                            */
  double step_size;        /* sgd.py:14                                                   */
  double gamma;            /* momentum decay, sgd.py:25                                   */
  const void* X;           /* device [N][D]                                               */
  const void* Y;           /* device [N][K] (softmax one-hot) or [N] (logistic)           */
  const int64_t* row0;     /* host [n_steps]                                              */
  int dropout;             /* 0: fit, 1: fit_dropout                                      */
  double keep_p;           /* fit_dropout's p (PHILOX mode)                               */
  int mask_mode;           /* HMCX_NOISE_BUFFER or HMCX_NOISE_PHILOX                      */
  const uint8_t* keep;     /* device, BUFFER                                              */
  const int64_t* keep_off; /* host [n_steps], BUFFER                                      */
  uint64_t seed;           /* PHILOX                                                      */
  uint32_t step_base;      /* PHILOX                                                      */
  void* W; void* b;        /* device state [D][K], [K], updated in place                  */
  void* mW; void* mb;      /* device momentum (zero at fit start, sgd.py:35)              */
} hmcx_sgd_args;
int hmcx_sgd_run(hmcx_ctx* ctx, const hmcx_sgd_args* a);

/* ------------------------------------------------------------------ samplers
 * One call enqueues n_steps consecutive sampler steps for C chains that share each
 * minibatch; the minibatch of step s is rows [row0[s], row0[s]+B) of X / Y.
 * noise_mode BUFFER: `noise` (device double) holds standard normals; the block of
 * (step s, chain c) starts at noise_off[s*C+c] and is laid out exactly in the
 * reference's draw order, P = D*K + K values per draw: SGHMC = momentum then one
 * draw per leapfrog iteration (weights then bias each); SGLD = one draw per step.
 * noise_mode PHILOX: normals come from Philox(seed, chain0+c, step_base+s, slot, elem). */
typedef struct hmcx_sampler_args {
  int dtype;
  int B, D, K, C;          /* minibatch rows, features, classes, chains in this call   */
  int n_steps;
  double alpha;            /* Gaussian prior precision (hyper['alpha'])               */
  double log_prior;        /* constant log_prior (cpu softmax.py:22-30), host-computed */
  const void* X;           /* device [N][D] (dtype)                                    */
  const void* Y;           /* device [N][K] (dtype, one-hot)                           */
  const int64_t* row0;     /* host [n_steps]                                           */
  const double* eps;       /* host [n_steps]  step size used by step s                */
  const int32_t* n_iter;   /* host [n_steps*C] SGHMC leapfrog iterations max(0, L-1)   */
  const double* u_accept;  /* host [n_steps*C] accept uniforms (SGHMC); both NULL in    */
                           /* PHILOX mode: drawn by the call (path_length, out_L)       */
  const uint8_t* want_ll;  /* host [n_steps] or NULL: SGLD computes ll(q_new) after s  */
  int noise_mode;
  const double* noise;     /* device, BUFFER mode                                      */
  const int64_t* noise_off;/* host [n_steps*C], BUFFER mode                            */
  uint64_t seed;           /* PHILOX mode                                              */
  uint32_t chain0;         /* PHILOX: global id of chain 0 of this call               */
  uint32_t step_base;      /* PHILOX: global step id of step 0 of this call           */
  void* W;                 /* device [D][C*K] state, updated in place                  */
  void* b;                 /* device [C*K]                                              */
  double* out_A;           /* device [n_steps*C] accept probability (SGHMC)            */
  int32_t* out_accepted;   /* device [n_steps*C]                                       */
  double* out_ll;          /* device [n_steps*C] log_likelihood(q_after, batch)        */
  double* out_E;           /* device [n_steps*C*2] (E_current, E_new) or NULL          */
  void* pW;                /* SGLD only, or NULL: device [D][C*K] momentum carried     */
  void* pb;                /*   across steps; selects the CuPy file's update (A2g)     */
  void* out_trace;         /* device [n_steps][C][D*K+K] (dtype) or NULL: the state     */
                           /* after every step (weights row-major, then bias) — the rows */
                           /* of the HDF5 backend (sghmc_multicore.py:49-51)            */
  int32_t* out_abort;      /* device [1] or NULL (SGHMC): 0, or 1 when a persistent launch */
                           /* timed out in a hand-off (or followed one that did) and left */
                           /* W/b untouched — see hmcx_clear_abort.  NULL: the check is    */
                           /* deferred to the next call / hmcx_synchronize instead.       */
                           /* SGLD (wide path): 1 when a fused team round timed out; W/b  */
                           /* are then invalid (hmcx_set_sgld_fuse).  NULL: the call re-runs */
                           /* itself and waits for its stream.                            */
  double path_length;      /* SGHMC, PHILOX mode with n_iter == u_accept == NULL: the call */
  double* out_L;           /* draws its own schedule (hmcx_philox_schedule, this path     */
                           /* length); out_L (host [n_steps*C] or NULL) receives the L's  */
  void* out_mom;           /* SGHMC, C < 16, or NULL: device [C][D*K+K] (dtype), the       */
                           /* momentum the call's LAST step returns (sghmc.py:36-39): the */
                           /* final p_new if accepted, else the drawn p                   */
  void* out_host;          /* SGHMC or NULL: pinned host block that receives the call's     */
                           /* outputs once the launch has finished: [n_steps*C f64 A]      */
                           /* [.. f64 ll][2*n_steps*C f64 E][n_steps*C i32 accepted][i32   */
                           /* abort].  out_A/out_ll/out_E/out_accepted must then be that    */
                           /* layout in one device block; the call copies it behind its     */
                           /* kernels (one copy when out_abort is the i32 right after that  */
                           /* block, else two) and records an event: hmcx_host_wait.        */
} hmcx_sampler_args;

/* Replaces hamiltonian/inference/{cpu,gpu}/sghmc.py:19-39 (step, with the A1 completion:
 * momentum ~ N(0,1), MH accept min(1, exp(E_cur - E_new)) from cpu/hmc.py:67-87). */
int hmcx_sghmc_run(hmcx_ctx* ctx, const hmcx_sampler_args* a);

/* Blocks until the outputs of the latest hmcx_sghmc_run call that named this out_host block have
 * landed in it (an event recorded behind that call's copies; no stream-wide synchronisation, so
 * calls enqueued after it keep running).  A block no call has named returns at once. */
int hmcx_host_wait(hmcx_ctx* ctx, const void* out_host);

/* Persistent-kernel hand-off timeouts (single-chain SGHMC).  A launch whose workgroups time out
 * waiting for each other (they were not co-resident, or not placed on the XCDs the kernel assumes)
 * writes nothing to W/b and raises the context's abort word; every later persistent launch sees the
 * raised word and returns at once, also without touching W/b.  The caller re-runs those calls (in
 * order, e.g. on the kernel-per-phase path: hmcx_set_sghmc_path(ctx, 1)) after hmcx_clear_abort,
 * which lowers the word (stream-ordered) and drops the deferred checks still pending. */
int hmcx_clear_abort(hmcx_ctx* ctx);

/* Fallback bookkeeping.  Every path that re-runs work after a timed-out cross-workgroup exchange
 * is counted per context, so a test suite, smoke check or benchmark can require that none happened
 * (a re-run gives the right result, which is exactly why it must not go unnoticed):
 *   HMCX_RECOVERY_PERSISTENT  persistent SGHMC calls re-run after a timed-out launch (hmcx_clear_abort
 *                             itself counts nothing; the host code that re-runs records each call)
 *   HMCX_RECOVERY_MLP_FUSED   hmcx_mlp_sghmc_run calls re-run unfused after their out_abort verdict
 *                             (the host code that re-runs records it: hmcx_note_recovery)
 *   HMCX_RECOVERY_WIDE_FUSED  hmcx_sgld_run calls whose fused forward + softmax timed out and that
 *                             re-ran on the three-launch path inside the call
 * counts: host int64_t[HMCX_RECOVERY_KINDS], totals since hmcx_create. */
enum hmcx_recovery {
  HMCX_RECOVERY_PERSISTENT = 0,
  HMCX_RECOVERY_MLP_FUSED = 1,
  HMCX_RECOVERY_WIDE_FUSED = 2,
  HMCX_RECOVERY_KINDS = 3
};
int hmcx_get_recoveries(const hmcx_ctx* ctx, int64_t* counts);
int hmcx_note_recovery(hmcx_ctx* ctx, int kind);

/* Which forward ran.  hmcx_mlp_sghmc_run picks the forward kernels per step from the shape, dtype and
 * mask alignment of the call; the host counts the forward launches it enqueues, per context, so a test
 * can require the path it means to cover (totals since hmcx_create):
 *   counts[0]  k_fwdr launches (every forward of a batched leapfrog iteration in one launch; float32)
 *   counts[1]  batched fused layer-2/3 launches of the k_mm family (several sub-steps per launch)
 *   counts[2]  single forwards (one sub-step or one energy forward at a time)
 * counts: host int64_t[3]. */
int hmcx_get_mlp_forward_counts(const hmcx_ctx* ctx, int64_t counts[3]);

/* Host-side Philox schedule of noise='philox' SGHMC steps (sghmc.py:25 path length, :36 accept
 * uniform), bit-identical to the device generator: for step s < n_steps and chain c < C
 *   L[s*C+c] = ceil(2·u_path·path_length / eps[s]),  n_iter = max(0, L − 1),  u = u_accept
 * with u_path / u_accept = Philox(seed, chain0 + c, step_base + s, SLOT_PATH / SLOT_ACCEPT, 0).
 * All arrays host.  Returns HMCX_EINVAL for a non-finite or oversized path length. */
int hmcx_philox_schedule(uint64_t seed, uint32_t chain0, int C, uint32_t step_base, int n_steps,
                         double path_length, const double* eps, double* L, int32_t* n_iter, double* u);

/* Launch plan of the persistent single-chain SGHMC kernel for a call of this shape on a device of
 * num_cus CUs with lds_max bytes of LDS per CU (host arithmetic only, no device needed): tsize = 4 or 8,
 * pad as HMCX_P2_PAD, want as HMCX_P2_HELP.  out: host long long[31] —
 *   [0] plan found, [1..7] Gr, Gf, Br, Bf, BfP, Ro, Fo, [8] plan LDS bytes, [9] helper mode the launch
 *   runs in (2, or 0 when want is not 2 or 2·G workgroups at one per CU do not fit), [10] dynamic LDS of
 *   the launch,
 *   [11] workgroups launched, [12..29] offset and size in granules of the arena regions XA, XD, XB, XW, XS,
 *   XC, XAh, XQ, XP, [30] granules in the arena. */
int hmcx_p2_plan_query(int B, int D, int K, int tsize, int num_cus, long long lds_max, int pad, int want,
                       long long* out);
/* The same for look-ahead mode `want` (1 = on).  out: host long long[26] — [0] 1 when the launch carries
 * two lanes, [1] workgroups launched, [2] dynamic LDS of the launch, [3] plan LDS, [4..21] offset and size
 * in granules of XA, XD, XB, XW, XS, XC, XQ, L1 (lane 1's XA … XS) and XV (verdict records), in address
 * order, [22] granules in the arena, [23..25] Br, BFP, Ro. */
int hmcx_p2_ahead_query(int B, int D, int K, int tsize, int num_cus, long long lds_max, int pad, int want,
                        long long* out);

/* Launches of one leapfrog iteration of the chain-batched SGHMC path (hmcx_sghmc_run with C >= 16, K = 10,
 * even D) when c_act of the C chains are still moving, on a device of num_cus CUs (host arithmetic only, no
 * device needed; the launcher follows the same function).  tail32, bfwd8, tail_wg, bgw_min, bgw_tail: the
 * values of HMCX_BTAIL32, HMCX_BFWD8, HMCX_BTAIL_WG, HMCX_BGW_MIN, HMCX_BGW_TAIL, or < 0 for the defaults
 * (1, 1, num_cus, 2·num_cus, 1).  out: host long long[12] —
 *   [0] 1 when the chain-batched path serves the shape (else the rest is 0), [1] 64-row forward tiles at full
 *   occupancy (C >= 512; the E_current forward always takes them then), [2] log-likelihood / column-sum
 *   partial blocks of the call, [3] kinetic-energy partial blocks of the call,
 *   [4] rows per forward tile (32 or 64), [5] waves per forward workgroup (4 or 8), [6] 1 when the forward is
 *   a compaction-tail launch, [7] forward row tiles, [8] chain tiles,
 *   [9] gradient kernel: 1 the 64-feature k_bgradw, 0 the 32-feature k_bgrad, [10] 1 when k_bgradw dispatches
 *   its partial last feature tile last, [11] gradient feature tiles.
 * Returns HMCX_EINVAL unless 1 <= c_act <= C and B, D, num_cus >= 1. */
int hmcx_sghmc_batch_plan_query(int B, int D, int K, int C, int c_act, int num_cus, int tail32, int bfwd8,
                                int tail_wg, int bgw_min, int bgw_tail, long long* out);

/* Replaces hamiltonian/inference/cpu/sgld.py:31-46 (step): p = N(0,(2ε)²) − ½ε∇U; q += p.
 * With pW/pb set: hamiltonian/inference/gpu/sgld.py:11-20, p = ν⊙p_prev − ½ε∇U with
 * ν ~ N(0,(2ε)²), q += p, p written back to pW/pb. */
int hmcx_sgld_run(hmcx_ctx* ctx, const hmcx_sampler_args* a);

/* ------------------------------------------------------------------ full-batch HMC, MVN model
 * Replaces cpu/hmc.py:39-64 with models/cpu/mvn_gaussian.py (config 1).
 * x [C][dim] state; mu [dim]; prec [dim][dim] = inv(cov); nlp_const = dim·log2π + log det cov,
 * nlp(x) = 0.5·(nlp_const + (x−μ)ᵀ·prec·(x−μ))  (mvn_gaussian.py:27-30 op order).
 * momentum/accept randomness as in hmcx_sampler_args (BUFFER: noise_off per step/chain, dim
 * normals per step).  out_nlp = nlp(q after step). */
typedef struct hmcx_hmc_mvn_args {
  int dim, C, n_steps;
  const double* mu;        /* device [dim] */
  const double* prec;      /* device [dim][dim] */
  double nlp_const;
  const double* eps;       /* host [n_steps] */
  const int32_t* n_iter;   /* host [n_steps*C] */
  const double* u_accept;  /* host [n_steps*C] */
  int noise_mode;
  const double* noise;
  const int64_t* noise_off;
  uint64_t seed;
  uint32_t chain0, step_base;
  double* x;               /* device [C][dim] */
  double* out_A;
  int32_t* out_accepted;
  double* out_nlp;
  double* out_trace;       /* device [n_steps][C][dim] or NULL */
} hmcx_hmc_mvn_args;
int hmcx_hmc_mvn_run(hmcx_ctx* ctx, const hmcx_hmc_mvn_args* a);
/* Per-call MVN surface, mvn_gaussian.py:14-31: for C points x [C][dim], g = (x − μ)·prec (grad) and
 * nlp = 0.5·(nlp_const + (x−μ)ᵀ·prec·(x−μ)) (negative_log_posterior); g or nlp may be NULL. */
int hmcx_mvn_eval(hmcx_ctx* ctx, int dim, int C, const double* mu, const double* prec, double nlp_const,
                  const double* x, double* g, double* nlp);

/* ------------------------------------------------------------------ full-batch HMC, linear models
 * Replaces cpu/hmc.py:39-64 (step) with the softmax (models/cpu/softmax.py) or logistic
 * (models/cpu/logistic.py) model, one chain: per step, momentum p ~ N(0,1) (hmc.py:41, draw order
 * weights then bias), then for it < n_iter, per var v in (weights, bias):
 *   p_v −= (½ε)·g_v;  q_v += ε·p_v;  g = grad(q);  p_v −= ε·g_v          (hmc.py:49-54)
 * with g = grad(q0) before the loop (hmc.py:47), p ← −p, and the MH accept
 * A = min(1, exp(E_cur − E_new)), E = nlp + ½Σp² (hmc.py:56-79; nlp = −(ll + log_prior)/N).
 * The whole schedule runs on the device: per gradient one k_fwd + one k_grad launch with the
 * kick/drift fused into the gradient epilogue; energies, accept and commit in step kernels.
 * log_prior: softmax — the constant `log_prior` (softmax.py:22-30); logistic — Σ_var
 * (lp_const[var] − ½·alpha·Σθ_var²) with Σθ² on the device (logistic.py:15-21).
 * X [N][D] (full batch: B = N rows), Y [N][K] one-hot (softmax) or [N] 0/1 (logistic, K = 1).
 * Noise as hmcx_sampler_args (BUFFER: noise_off[s], P = D·K + K momentum normals per step).
 * hmcx_hmc_run is the C = 1 case of hmcx_hmc_chains_run below (chain0 = chain): one implementation,
 * the same validation, bit-identical results. */
typedef struct hmcx_hmc_args {
  int dtype;
  int model;               /* HMCX_MODEL_SOFTMAX or HMCX_MODEL_LOGISTIC                  */
  int B, D, K, n_steps;    /* B = N (full batch)                                        */
  double alpha;
  double log_prior;        /* softmax: constant log prior                               */
  double lp_const[2];      /* logistic: dim·½·log(alpha/2π) of weights, bias            */
  const void* X;
  const void* Y;
  const double* eps;       /* host [n_steps]                                            */
  const int32_t* n_iter;   /* host [n_steps]  max(0, L − 1)                            */
  const double* u_accept;  /* host [n_steps]                                            */
  int noise_mode;
  const double* noise;     /* device, BUFFER                                            */
  const int64_t* noise_off;/* host [n_steps], BUFFER                                    */
  uint64_t seed;
  uint32_t chain, step_base;
  void* W;                 /* device [D][K] state, updated in place                     */
  void* b;                 /* device [K]                                                */
  double* out_A;           /* device [n_steps]                                          */
  int32_t* out_accepted;   /* device [n_steps]                                          */
  double* out_nlp;         /* device [n_steps]: nlp of the state kept after step s     */
  double* out_E;           /* device [n_steps*2] (E_current, E_new) or NULL             */
  void* out_trace;         /* device [n_steps][D*K+K] (dtype) or NULL: state after s    */
  void* out_mom;           /* device [n_steps][D*K+K] (dtype) or NULL: momentum drawn   */
} hmcx_hmc_args;
int hmcx_hmc_run(hmcx_ctx* ctx, const hmcx_hmc_args* a);

/* C chains of the above in one call — the intent of hamiltonian/inference/cpu/hmc_multicore.py:22-38
 * (one hmc.sample per worker; the reference's Pool.map omits `self`).  Every chain follows the
 * semantics documented above hmcx_hmc_args; the chains share X, Y, eps and the launches.  State in the
 * chain-interleaved layout of hmcx_sampler_args: W [D][C*K], b [C*K].  Schedules are per (step, chain),
 * index s*C + c; a step launches max_c(1 + 2·n_iter[s][c]) gradient evaluations (k_fwd + k_grad over
 * all chains), and each chain derives the kicks/drifts that follow evaluation e from (e, its own
 * n_iter): a chain past its last evaluation (or with n_iter = 0: q kept, A = 1) writes nothing.
 * BUFFER noise: P = D·K + K momentum normals per (step, chain) at noise_off[s*C + c] (weights
 * row-major, then bias).  PHILOX: chain c draws Philox(seed, chain0 + c, step_base + s, slot 0, elem),
 * the stream of a one-chain hmcx_hmc_run with chain = chain0 + c.  C = 1 is what hmcx_hmc_run runs. */
typedef struct hmcx_hmc_chains_args {
  int dtype;
  int model;               /* HMCX_MODEL_SOFTMAX or HMCX_MODEL_LOGISTIC                  */
  int B, D, K, C, n_steps; /* B = N (full batch); C chains                              */
  double alpha;
  double log_prior;        /* softmax: constant log prior                               */
  double lp_const[2];      /* logistic: dim·½·log(alpha/2π) of weights, bias            */
  const void* X;
  const void* Y;
  const double* eps;       /* host [n_steps]                                            */
  const int32_t* n_iter;   /* host [n_steps*C]  max(0, L − 1)                          */
  const double* u_accept;  /* host [n_steps*C]                                          */
  int noise_mode;
  const double* noise;     /* device, BUFFER                                            */
  const int64_t* noise_off;/* host [n_steps*C], BUFFER                                  */
  uint64_t seed;
  uint32_t chain0, step_base;
  void* W;                 /* device [D][C*K] state, updated in place                   */
  void* b;                 /* device [C*K]                                              */
  double* out_A;           /* device [n_steps*C]                                        */
  int32_t* out_accepted;   /* device [n_steps*C]                                        */
  double* out_nlp;         /* device [n_steps*C]: nlp of the state kept after step s   */
  double* out_E;           /* device [n_steps*C*2] (E_current, E_new) or NULL           */
  void* out_trace;         /* device [n_steps][C][D*K+K] (dtype) or NULL: state after s */
  void* out_mom;           /* device [n_steps][C][D*K+K] (dtype) or NULL: momentum drawn*/
} hmcx_hmc_chains_args;
int hmcx_hmc_chains_run(hmcx_ctx* ctx, const hmcx_hmc_chains_args* a);

/* ------------------------------------------------------------------ random-walk Metropolis, linear models
 * Replaces cpu/metropolis.py:27-64 (step / accept / random_walk) with the softmax (CPU prior) or
 * logistic model, C chains and n_steps steps in one call.  Per step and chain, per variable v in
 * (weights, bias):  q_new_v = q_v + (T)mult_v·z_v  (metropolis.py:59, mult = factor·scale evaluated on the
 * host), on every coordinate when site_v = −1, else on the one flat coordinate site_v of that variable
 * (update_sequential=False, metropolis.py:61-62).  Then E = −(ll + lp) on the sum scale (no division
 * by N; metropolis.py:49-50 with logp = log_likelihood + log_prior), A = exp(E − E_new) and
 *   accepted = isfinite(A) && u < A                                        (metropolis.py:42-46)
 * — no min(1, ·): an overflowing ratio (A = inf) is REJECTED like NaN, unlike hmcx_hmc_run's accept.
 * log prior as in hmcx_hmc_args (softmax: the constant `log_prior`; logistic: Σ_var (lp_const[var] −
 * ½·alpha·Σθ_var²), logistic.py:15-21 order).  State in the layout of hmcx_hmc_chains_args, W [D][C*K],
 * b [C*K], updated in place; schedules per (step, chain), index s*C + c, two entries (weights, bias)
 * where marked [·2].  Noise: BUFFER — P = D·K + K normals per (step, chain) at noise_off[s*C + c]
 * (weights row-major, then bias; with site ≥ 0 only the element at `site` is read); PHILOX — element i
 * is Philox(seed, chain0 + c, step_base + s, slot 0, i), the momentum stream of hmcx_hmc_chains_run.
 * A step is three launches: k_mh_propose (commit of the previous step, its trace row, the new proposal
 * and its Σθ² partials in one elementwise pass), k_fwd in log-likelihood mode over all chains, and
 * k_mh_accept; the kept state's log-likelihood is carried on the device, never evaluated twice. */
typedef struct hmcx_mh_args {
  int dtype;
  int model;               /* HMCX_MODEL_SOFTMAX or HMCX_MODEL_LOGISTIC                  */
  int B, D, K, C, n_steps; /* B = N (full batch); C chains                              */
  double alpha;
  double log_prior;        /* softmax: constant log prior                               */
  double lp_const[2];      /* logistic: dim·½·log(alpha/2π) of weights, bias            */
  const void* X;
  const void* Y;
  const double* mult;      /* host [n_steps*C*2]  factor·scale of (weights, bias)       */
  const int32_t* site;     /* host [n_steps*C*2]  −1: all coordinates, else flat index  */
  const double* u_accept;  /* host [n_steps*C]                                          */
  int noise_mode;
  const double* noise;     /* device, BUFFER                                            */
  const int64_t* noise_off;/* host [n_steps*C], BUFFER                                  */
  uint64_t seed;
  uint32_t chain0, step_base;
  void* W;                 /* device [D][C*K] state, updated in place                   */
  void* b;                 /* device [C*K]                                              */
  double* out_A;           /* device [n_steps*C]: the raw ratio (may be inf / NaN)      */
  int32_t* out_accepted;   /* device [n_steps*C]                                        */
  double* out_logp;        /* device [n_steps*C]: ll + lp of the state kept after step s */
  double* out_E;           /* device [n_steps*C*2] (E_current, E_new) or NULL           */
  void* out_trace;         /* device [n_steps][C][D*K+K] (dtype) or NULL: state after s */
} hmcx_mh_args;
int hmcx_mh_run(hmcx_ctx* ctx, const hmcx_mh_args* a);

/* The same for the MVN model (mvn_gaussian.py:22-31): x [C][dim] state, one variable, E = nlp(x) with
 * mu / prec / nlp_const as in hmcx_hmc_mvn_args; mult, site [n_steps*C]; BUFFER noise: dim normals per
 * (step, chain).  One thread per chain, the whole phase in one launch.  out_logp = −nlp of the state
 * kept after step s. */
typedef struct hmcx_mh_mvn_args {
  int dim, C, n_steps;
  const double* mu;        /* device [dim] */
  const double* prec;      /* device [dim][dim] */
  double nlp_const;
  const double* mult;      /* host [n_steps*C] */
  const int32_t* site;     /* host [n_steps*C] */
  const double* u_accept;  /* host [n_steps*C] */
  int noise_mode;
  const double* noise;
  const int64_t* noise_off;
  uint64_t seed;
  uint32_t chain0, step_base;
  double* x;               /* device [C][dim] */
  double* out_A;
  int32_t* out_accepted;
  double* out_logp;
  double* out_E;           /* device [n_steps*C*2] (E_current, E_new) or NULL */
  double* out_trace;       /* device [n_steps][C][dim] or NULL */
} hmcx_mh_mvn_args;
int hmcx_mh_mvn_run(hmcx_ctx* ctx, const hmcx_mh_mvn_args* a);

/* Leapfrog arithmetic on device vectors of n elements (dtype), for hmc.step on models without a
 * fused entry (the MLP): mode 0  y −= a·x;  mode 1  y += a·x  (hmc.py:50-53, p −= ε·g, q += ε·p).
 * hmcx_sumsq gives the kinetic energy's Σp² (hmc.py:74-79). */
int hmcx_axpy(hmcx_ctx* ctx, int dtype, int mode, int64_t n, double a, const void* x, void* y);

/* ------------------------------------------------------------------ MLP model (config 3)
 * Replaces hamiltonian/models/gpu/mlp.py:19-31 (MyNetwork: l1 -> relu(dropout) -> l2 ->
 * relu(dropout) -> dropout -> l3) and :47-82 (grad / log_likelihood / negative_log_posterior)
 * without Chainer.  Parameters in Chainer's layout, L.Linear W = [out][in]:
 *   W1 [n_mid][n_in], b1 [n_mid], W2 [n_mid][n_mid], b2 [n_mid], W3 [n_out][n_mid], b3 [n_out].
 * Dropout (mlp.py:29-31, train mode): mask = (u >= ratio) / (1 − ratio) for the three [B][n_mid]
 * activations of every forward, ratio the context's (hmcx_set_mlp_dropout; 0.1 by default, the
 * reference's).  mask_mode BUFFER: masks[...] holds them (3·B·n_mid values per forward, dtype) and is
 * used as given, whatever the ratio; PHILOX: u = Philox(seed, chain, step, slot = forward index, element). */
typedef struct hmcx_mlp_params {
  void* p[6];              /* W1, b1, W2, b2, W3, b3 (device, dtype) */
} hmcx_mlp_params;

/* Philox dropout masks of one forward: out [3][B][n_mid] (dtype) = (u >= ratio) / (1 − ratio) with
 * u = Philox(seed, chain, step, slot, element) and the context's ratio (hmcx_set_mlp_dropout) — the masks
 * every PHILOX mode of the MLP entries below draws. */
int hmcx_mlp_masks(hmcx_ctx* ctx, int dtype, int B, int n_mid, uint64_t seed, uint32_t chain, uint32_t step,
                   uint32_t slot, void* out);

/* grad = ∇ mean softmax-CE(net(X), y) + ½·alpha·θ for all six parameters (mlp.py:47-64).
 * y: device int32 [B] labels.  masks: device [3][B][n_mid] or NULL (no dropout).
 * grads: output pointers, same shapes.  loss (device double[1] or NULL): the mean CE. */
int hmcx_mlp_grad(hmcx_ctx* ctx, int dtype, const void* X, const int32_t* y, int B, int n_in, int n_mid,
                  int n_out, const hmcx_mlp_params* par, const void* masks, double alpha,
                  hmcx_mlp_params* grads, double* loss);

/* loss = mean softmax-CE (mlp.py:66-78 returns the loss); logits [B][n_out] optional output
 * (predict, mlp.py:84-96). */
int hmcx_mlp_loss(hmcx_ctx* ctx, int dtype, const void* X, const int32_t* y, int B, int n_in, int n_mid,
                  int n_out, const hmcx_mlp_params* par, const void* masks, double* loss, void* logits);

/* SGHMC steps for the MLP (reference cpu/sghmc.py:19-39 with the A1 completion; energies from
 * mlp.py:80-82 nlp = loss + log_prior, log_prior = −Σ_var ½·alpha·Σθ²/dim).  Sub-steps follow
 * order[0..5] (canonical indices 0=W1 1=b1 2=W2 3=b2 4=W3 5=b3 in the caller's start_p order).
 * Noise BUFFER: per step, normals in the reference's draw order — momentum of every variable
 * in `order`, then per leapfrog iteration one draw per variable in `order` — from noise_off[s].
 * PHILOX: slot 0 momentum, slot it+1 iteration it, element = offset of the variable in `order`
 * + index.  Masks: forward f of step s (f = 0 .. 6·n_iter−1 for the gradient calls, then the
 * proposal's and the current state's energies) — BUFFER: masks + mask_off[s] + f·3·B·n_mid;
 * PHILOX: slot 0x80000000 + f.  out_loss[s] = mean CE loss (log_likelihood, mlp.py:66-78) and out_nlp[s] =
 * loss + log_prior (negative_log_posterior) of the state kept after step s, both under the masks
 * of that state's energy forward. */
typedef struct hmcx_mlp_sghmc_args {
  int dtype;
  int B, n_in, n_mid, n_out, n_steps;
  int order[6];
  double alpha;
  const void* X;           /* device [N][n_in] */
  const int32_t* y;        /* device [N] labels */
  const int64_t* row0;     /* host [n_steps] */
  const double* eps;       /* host [n_steps] */
  const int32_t* n_iter;   /* host [n_steps] */
  const double* u_accept;  /* host [n_steps] */
  int noise_mode;
  const double* noise;     /* device, BUFFER */
  const int64_t* noise_off;/* host [n_steps], BUFFER */
  int mask_mode;
  const void* masks;       /* device, BUFFER (dtype) */
  const int64_t* mask_off; /* host [n_steps], BUFFER */
  uint64_t seed;
  uint32_t chain, step_base;
  hmcx_mlp_params par;     /* state, updated in place */
  double* out_A;           /* device [n_steps] */
  int32_t* out_accepted;   /* device [n_steps] */
  double* out_loss;        /* device [n_steps] */
  double* out_nlp;         /* device [n_steps] or NULL */
  double* out_E;           /* device [n_steps*2] (E_current, E_new) or NULL */
  int32_t* out_abort;      /* device [1] or NULL: the call's verdict — 1 when an exchange of the fused
                              layer-2/3 launches timed out; the state and every output of the call are
                              then invalid: restore the state and re-run with hmcx_set_mlp_fuse(ctx, 0).
                              NULL: the call waits for its stream and returns an error instead. */
} hmcx_mlp_sghmc_args;
int hmcx_mlp_sghmc_run(hmcx_ctx* ctx, const hmcx_mlp_sghmc_args* a);

/* Full-batch HMC leapfrog trajectory of the MLP in one call: replaces the per-variable loop of
 * hamiltonian/inference/cpu/hmc.py:46-56 as the GPU hmc.step runs it on the MLP (the reference's
 * gpu/hmc.py step with models/gpu/mlp.py grad).  With g = grad(q) first, per iteration and per
 * variable v in order[0..5]:  p_v −= ε/2·g_v;  q_v += ε·p_v;  g = grad(q);  p_v −= ε·g_v  (hmc.py:50-53),
 * then p = −p (hmc.py:55-56, as p − 2·p).  grad is hmcx_mlp_grad (∇ mean CE + ½·alpha·θ, all six
 * variables, 1 + 6·n_iter calls; every call but the last computes only the one or two components the
 * next kicks read, the last one all six).  The kicks and drifts between two gradient calls run in one
 * launch of k_mlp_kicks, which mirrors k_axpy's (hmcx_axpy's) per-element arithmetic (ax = a·x; y ∓ ax),
 * and the sign flip in k_mlp_neg6 (p − 2·p): other kernels than the host loop's, the same roundings, so
 * the trajectory is bit-identical to it (test_hmc_mlp_device_leapfrog_equals_host_loop pins that).
 * Masks per gradient call:
 *   HMCX_MLP_MASKS_NONE    no dropout;
 *   HMCX_MLP_MASKS_FIXED   masks [3][B][n_mid] (dtype) for every call;
 *   HMCX_MLP_MASKS_PHILOX  call k draws hmcx_mlp_masks(seed, chain, step, slot0 + k) into masks (scratch).
 * q and p are advanced in place; g holds the gradient at the final position on return. */
#define HMCX_MLP_MASKS_NONE 0
#define HMCX_MLP_MASKS_FIXED 1
#define HMCX_MLP_MASKS_PHILOX 2
typedef struct hmcx_mlp_leapfrog_args {
  int dtype;
  int B, n_in, n_mid, n_out, n_iter;
  int order[6];            /* canonical variable indices 0=W1 .. 5=b3 in the caller's start order */
  double eps, alpha;
  const void* X;           /* device [B][n_in] */
  const int32_t* y;        /* device [B] labels */
  hmcx_mlp_params q, p, g; /* device: position, momentum (in/out), gradient (out) */
  int mask_mode;
  void* masks;             /* device [3][B][n_mid]: FIXED input / PHILOX scratch */
  uint64_t seed;
  uint32_t chain, step, slot0;
} hmcx_mlp_leapfrog_args;
int hmcx_mlp_hmc_leapfrog(hmcx_ctx* ctx, const hmcx_mlp_leapfrog_args* a);

/* Momentum SGD on the MLP, a whole fit in one call: replaces the loop of hamiltonian/inference/gpu/sgd.py:25-47
 * (cpu/sgd.py:36-42) over models/gpu/mlp.py:47-64.  Per step s on the minibatch rows row0[s] .. row0[s] + B:
 *   g = grad(θ) — the values hmcx_mlp_grad returns for the step's masks (∇ mean CE + ½·alpha·θ), then for every
 *   element of all six variables  m = gamma·m − step_size·g;  θ = θ + m  (sgd.py:40-41), in dtype.
 * out_loss[s] is the mean CE of that gradient forward (θ before the update).  Where want_eval[s] is set the
 * state after the update is evaluated on the same minibatch under fresh masks (sgd.py:42): the e-th set flag
 * (step order, n_evals flags in all) writes out_eval_loss[e] = the mean CE (hmcx_mlp_loss's value) and
 * out_eval_sumsq[e][v] = Σθ² (float64, fixed summation order) of canonical variable v (0=W1 .. 5=b3) — the
 * pieces of negative_log_posterior (mlp.py:80-82), which the caller composes in its own variable order.
 * Masks (the HMCX_MLP_MASKS_* values):
 *   NONE    no dropout;
 *   FIXED   the gradient forward of step s reads masks + mask_off[s], the evaluation after it
 *           masks + eval_mask_off[s] (3·B·n_mid values each, dtype);
 *   PHILOX  the gradient forward of step s uses what hmcx_mlp_masks(ctx, dtype, B, n_mid, seed, chain,
 *           step_base + s, 0x80000000, ·) writes, the evaluation after it slot 0x80000001 (SGHMC's
 *           "slot 0x80000000 + f", f the forward index within the step).
 * One call of n steps equals any split into calls that carry par / mom and advance step_base, bit for bit.
 * Every launch is the unfused one of hmcx_mlp_grad / hmcx_mlp_loss (no cross-workgroup exchange, nothing
 * that could time out: no out_abort), plus one element-wise launch per step (k_mlp_sgd: the update, the next
 * step's Philox masks, the Σθ² partials and the step's loss).  n_steps == 0 does nothing.  Stream-ordered;
 * returns once enqueued. */
typedef struct hmcx_mlp_sgd_args {
  int dtype;
  int B, n_in, n_mid, n_out, n_steps;
  double alpha, step_size, gamma;
  const void* X;              /* device [N][n_in] */
  const int32_t* y;           /* device [N] labels */
  const int64_t* row0;        /* host [n_steps]: minibatch of step s = rows row0[s] .. +B */
  const uint8_t* want_eval;   /* host [n_steps] or NULL: 1 = evaluate after step s */
  int mask_mode;              /* HMCX_MLP_MASKS_NONE / _FIXED / _PHILOX */
  const void* masks;          /* device (dtype), FIXED */
  const int64_t* mask_off;    /* host [n_steps], FIXED: masks of step s's gradient forward */
  const int64_t* eval_mask_off;/* host [n_steps], FIXED: masks of the evaluation after step s (read where want_eval) */
  uint64_t seed;
  uint32_t chain, step_base;
  hmcx_mlp_params par;        /* state, updated in place */
  hmcx_mlp_params mom;        /* momentum, updated in place (zeros at fit start, sgd.py:35) */
  double* out_loss;           /* device [n_steps] or NULL */
  double* out_eval_loss;      /* device [n_evals] */
  double* out_eval_sumsq;     /* device [n_evals][6] */
} hmcx_mlp_sgd_args;
int hmcx_mlp_sgd_run(hmcx_ctx* ctx, const hmcx_mlp_sgd_args* a);

/* SGLD on the MLP, an epoch of steps in one call: replaces the loop of hamiltonian/inference/{cpu,gpu}/sgmcmc.py
 * over sgld.step (cpu/sgld.py:31-46, gpu/sgld.py:11-26).  Per step s on the minibatch rows row0[s] .. row0[s] + B,
 * with ε = eps[s]:
 *   g = grad(θ) — the values hmcx_mlp_grad returns for the step's masks (∇ mean CE + ½·alpha·θ), z = P standard
 *   normals (P = all six variables' elements), then for every element, in dtype T, every product and sum rounded
 *   once as the NumPy expression rounds them:
 *     variant 0 (cpu/sgld.py:34-38, rng.normal(0, 2ε)):  p = (T)(2ε)·z;  p = p + (T)(−0.5·ε)·g;  θ = θ + p
 *     variant 1 (gpu/sgld.py:14-19):  p = ((T)(2ε)·z)·p_prev − (T)(0.5·ε)·g;  θ = θ + p;  p is stored in mom.
 * Noise: z is laid out variable after variable in `order` (the caller's start_p order, in which draw_momentum
 * draws), element e = the variable's offset in that layout + its index.
 *   HMCX_NOISE_BUFFER  step s reads z[e] = noise[noise_off[s] + e] (double, converted to T);
 *   HMCX_NOISE_PHILOX  z[e] = the Philox normal of (seed, chain, step_base + s, slot 0, e) in T — SGHMC's momentum
 *                      convention; hmcx_philox_normals (float) / hmcx_philox_normals_f64 (double) return the same
 *                      stream on the host.
 * out_loss[s] is the mean CE of the gradient forward (θ before the update).
 * Evaluations: want_eval[s] is a bit mask, each set bit one more forward on the step's minibatch at the updated θ
 * under fresh masks.  Bit 0: the outer loop's log line, log_likelihood(q) (sgmcmc.py:60-62,74-76); bit 1: the
 * epoch-end negative_log_posterior (sgmcmc.py:79).  The forwards of a step are numbered in call order: 0 the
 * gradient forward, then the bit-0 forward if set, then the bit-1 forward if set.  The e-th evaluation of the call
 * (step order, bit 0 before bit 1; n_evals set bits in all) writes out_eval_loss[e] = the mean CE (hmcx_mlp_loss's
 * value) and, where out_eval_sumsq is given, out_eval_sumsq[e][v] = Σθ² (float64, fixed summation order) of
 * canonical variable v (0=W1 .. 5=b3) — the pieces of negative_log_posterior (mlp.py:80-82), which the caller
 * composes in its own variable order.
 * Masks (the HMCX_MLP_MASKS_* values):
 *   NONE    no dropout;
 *   FIXED   forward 0 of step s reads masks + mask_off[s], forward f ≥ 1 masks + eval_mask_off[2·s + f − 1]
 *           (3·B·n_mid values each, dtype);
 *   PHILOX  forward f of step s uses what hmcx_mlp_masks(ctx, dtype, B, n_mid, seed, chain, step_base + s,
 *           0x80000000 + f, ·) writes.
 * Draws: where want_draw[s] is set, the updated θ of step s is also stored, the d-th flagged step of the call at
 * draws.p[v] + d·n_v (n_v the elements of canonical variable v): the [S][shape] stacked layout hmcx_mlp_predictive
 * reads.
 * One call of n steps equals any split into calls that carry par / mom and advance step_base (and the draw
 * pointers), bit for bit.  Every launch is the unfused one of hmcx_mlp_grad / hmcx_mlp_loss (no cross-workgroup
 * exchange, nothing that could time out: no out_abort), plus one element-wise launch per step (k_mlp_sgld: the
 * noise, the update, the draw store, the Σθ² partials, the step's loss and the next step's Philox masks).
 * n_steps == 0 does nothing.  Stream-ordered; returns once enqueued. */
typedef struct hmcx_mlp_sgld_args {
  int dtype;
  int B, n_in, n_mid, n_out, n_steps;
  int order[6];               /* canonical variable indices 0=W1 .. 5=b3 in the caller's start order */
  int variant;                /* 0: cpu/sgld.py, 1: gpu/sgld.py (carried momentum) */
  double alpha;
  const void* X;              /* device [N][n_in] */
  const int32_t* y;           /* device [N] labels */
  const int64_t* row0;        /* host [n_steps]: minibatch of step s = rows row0[s] .. +B */
  const double* eps;          /* host [n_steps]: step size of step s */
  const uint8_t* want_eval;   /* host [n_steps] or NULL: bit 0 = log-line forward, bit 1 = epoch-end forward */
  int noise_mode;             /* HMCX_NOISE_BUFFER or HMCX_NOISE_PHILOX */
  const double* noise;        /* device, BUFFER */
  const int64_t* noise_off;   /* host [n_steps], BUFFER: step s reads noise + noise_off[s] .. + P */
  int mask_mode;              /* HMCX_MLP_MASKS_NONE / _FIXED / _PHILOX */
  const void* masks;          /* device (dtype), FIXED */
  const int64_t* mask_off;    /* host [n_steps], FIXED: masks of step s's gradient forward */
  const int64_t* eval_mask_off;/* host [n_steps][2], FIXED: masks of forwards 1 and 2 of step s (read where set) */
  uint64_t seed;
  uint32_t chain, step_base;
  hmcx_mlp_params par;        /* state, updated in place */
  hmcx_mlp_params mom;        /* variant 1: momentum, updated in place (zeros at the start, gpu/sgmcmc.py:48);
                                 variant 0: all NULL */
  double* out_loss;           /* device [n_steps] or NULL */
  double* out_eval_loss;      /* device [n_evals] */
  double* out_eval_sumsq;     /* device [n_evals][6] or NULL */
  const uint8_t* want_draw;   /* host [n_steps] or NULL: 1 = store θ after step s */
  hmcx_mlp_params draws;      /* device, [n_draws][shape] per variable (read where want_draw is given) */
} hmcx_mlp_sgld_args;
int hmcx_mlp_sgld_run(hmcx_ctx* ctx, const hmcx_mlp_sgld_args* a);

/* C chains of hmcx_mlp_sgld_run in one call (extension; the reference runs one chain per process).  The chains
 * take the same steps on the same minibatches row0[s] with the same eps[s]; every field hmcx_mlp_sgld_args also
 * has means what it means there.
 * State: par.p[v] holds C stacked copies [C][shape_v], chain-major and contiguous (the [S][shape] layout
 * hmcx_mlp_predictive reads), updated in place; mom.p[v] the same for variant 1 (all NULL for variant 0).
 * Chains: with PHILOX noise and PHILOX masks chain c is bit for bit the one-chain hmcx_mlp_sgld_run with
 * chain = chain0 + c and the same seed, step_base and want_eval — state, momentum, out_loss, the evaluation
 * outputs and the draws, in float64 and float32, both variants — so the result of chain c depends neither on C
 * nor on how the chains are grouped into launches.  BUFFER noise and FIXED masks are shared by all chains
 * (noise_off[s], mask_off[s] and eval_mask_off[s][2] as in the one-chain call): the chains are replicas apart
 * from their start.
 * Outputs: out_loss [n_steps][C], out_eval_loss [n_evals][C], out_eval_sumsq [n_evals][C][6].  Draws: the d-th
 * flagged step of chain c is stored at draws.p[v] + (c·draw_stride + d)·n_v; draw_stride is the caller's draws
 * per chain, so one [C][T][shape] buffer serves a whole run with the pointers advanced from call to call.
 * One call of n steps equals any split into calls that carry par / mom and advance step_base and the draw
 * pointers, bit for bit.
 * Schedule: the chains are the problems of batched launches, in groups of at most 6 chains; per step and group
 * the one-chain schedule with every launch widened over the group's chains (layer 1, layer 2, layer 3 +
 * cross-entropy, layer-1 backward, the W1 and W2 gradients, the bias / W3 gradients, the update: 8 launches
 * with n_out ≤ 32; above, layer 3 runs chain by chain).  Only unfused launches: no cross-workgroup exchange, no
 * spin-wait, no abort word.
 * 1 ≤ C ≤ 64; chain0 + C and step_base + n_steps must not wrap 2^32; want_draw needs draw_stride ≥ the call's
 * flagged steps.  Invalid arguments return a negative code, set hmcx_last_error and launch nothing.
 * n_steps == 0 does nothing.  Stream-ordered; returns once enqueued. */
typedef struct hmcx_mlp_sgld_chains_args {
  int dtype;
  int B, n_in, n_mid, n_out, n_steps;
  int C;                      /* chains, 1 .. 64 */
  int order[6];
  int variant;
  double alpha;
  const void* X;
  const int32_t* y;
  const int64_t* row0;
  const double* eps;
  const uint8_t* want_eval;
  int noise_mode;
  const double* noise;        /* device, BUFFER: shared by the chains */
  const int64_t* noise_off;
  int mask_mode;
  const void* masks;          /* device (dtype), FIXED: shared by the chains */
  const int64_t* mask_off;
  const int64_t* eval_mask_off;
  uint64_t seed;
  uint32_t chain0, step_base; /* chain c draws under Philox chain chain0 + c */
  hmcx_mlp_params par;        /* [C][shape_v] per variable, updated in place */
  hmcx_mlp_params mom;        /* variant 1: [C][shape_v]; variant 0: all NULL */
  double* out_loss;           /* device [n_steps][C] or NULL */
  double* out_eval_loss;      /* device [n_evals][C] */
  double* out_eval_sumsq;     /* device [n_evals][C][6] or NULL */
  const uint8_t* want_draw;
  hmcx_mlp_params draws;      /* device, [C][draw_stride][shape_v] per variable (read where want_draw is given) */
  int64_t draw_stride;        /* draws per chain of the caller's buffer */
} hmcx_mlp_sgld_chains_args;
int hmcx_mlp_sgld_chains_run(hmcx_ctx* ctx, const hmcx_mlp_sgld_chains_args* a);

/* Full-batch HMC on the MLP, n_steps steps of C chains in one call (extension; the reference's hmc.sample drives
 * one chain step by step from the host): replaces hamiltonian/inference/cpu/hmc.py:39-64 (step, accept) over
 * models/gpu/mlp.py for every (step s, chain c), with ε = eps[s], n = n_iter[s·C + c], u = u_accept[s·C + c]:
 *   1. momentum: p = P standard normals laid out variable after variable in `order` (element e = the variable's
 *      offset in that layout + its index).  HMCX_NOISE_BUFFER: noise[noise_off[s·C + c] + e] (double, converted
 *      to dtype); HMCX_NOISE_PHILOX: the Philox normal of (seed, chain0 + c, step_base + s, slot 0, e) in dtype,
 *      the stream hmcx_philox_normals / hmcx_philox_normals_f64 return on the host.
 *   2. trajectory on copies (q', p'), exactly hmcx_mlp_hmc_leapfrog's: 1 + 6n gradient calls, kicks and drifts by
 *      k_mlp_kicks's per-element arithmetic, each call computing only the components the next kicks read, the
 *      layer-1 output reused until W1 moves.  The final p = −p is skipped: p is discarded after the step and the
 *      sign does not change the kinetic energy.
 *   3. the forwards of (s, c) are numbered in call order: f = 0 the gradient at q; f = 1 + 6·it + i the gradient
 *      after the drift of order[i] in iteration it; f = 6n + 1 the proposal's energy forward; f = 6n + 2 the
 *      current state's (hmc.py:68-69 evaluates the proposal first); f = 6n + 3 the record forward, only where
 *      want_eval[s] is set.  Masks of forward f: HMCX_MLP_MASKS_NONE no dropout; FIXED masks +
 *      mask_off[s·C + c] + f·3·B·n_mid (dtype; each chain its own block); PHILOX what hmcx_mlp_masks(seed,
 *      chain0 + c, step_base + s, 0x80000000 + f) writes.
 *   4. n = 0 keeps the numbering; its f = 0 gradient is never read and is not launched.  A still comes from the two
 *      energy forwards: under dropout it is not 1.
 *   5. energies: E = (loss + log_prior) + K, loss the mean CE of the forward (hmcx_mlp_loss's value up to the
 *      order of the row-block sum), log_prior = −Σ_v ½·alpha·Σθ_v²/dim_v and K = Σ_v ½·Σp_v², both over `order`, in
 *      float64 with a fixed summation order (hmcx_mlp_sghmc_run's composition).
 *   6. A = min(1, exp(E_cur − E_new)) as Python's min (NaN gives 1); accepted = isfinite(A) && u < A; an
 *      accepted step commits q' to par.
 * Outputs: out_A, out_accepted [n_steps·C] and out_E [n_steps·C][2] = (E_current, E_new) at index s·C + c.  Where
 * want_eval[s] is set, the e-th such step writes out_eval_loss[e][c] = the mean CE of the kept state under forward
 * 6n + 3 and out_eval_sumsq[e][c][v] = Σθ² of canonical variable v of the kept state — the pieces of
 * negative_log_posterior, as hmcx_mlp_sgd_run returns them.  Where want_draw[s] is set, the d-th such step of
 * chain c stores the kept state at draws.p[v] + (c·draw_stride + d)·n_v and, where out_mom.p[v] is given, the
 * momentum drawn in that step at the same offset of out_mom.p[v].
 * Guarantees:
 *   chains   with PHILOX noise and masks chain c is bit for bit the C = 1 call with chain0 + c — state, A, E,
 *            flags, evaluations, draws, float64 and float32: a chain's result depends neither on C, nor on how the
 *            chains are grouped into launches, nor on the other chains' path lengths.
 *   splits   one call of n steps equals any split into calls that carry par and advance step_base (and the
 *            host arrays and the draw pointers), bit for bit.
 *   errors   invalid arguments return a negative code, set hmcx_last_error, launch nothing and leave par
 *            untouched: C outside 1 .. 64, order not a permutation, n_iter < 0 or so large that
 *            0x80000000 + 6n + 3 wraps, chain0 + C or step_base + n_steps wrapping 2^32, want_draw with
 *            draw_stride below the call's flagged steps, a missing buffer for the chosen modes; NULL ctx or
 *            args: −1.
 *   n_steps == 0 does nothing.
 * Schedule: the chains are the problems of batched launches, in groups of at most 6; gradient evaluation e of a
 * step is launched for the chains of the group that still have one, so a step costs max_c(1 + 6·n_c) evaluations.
 * Only unfused launches: no cross-workgroup exchange, no spin-wait, no abort word.  Nothing is read back inside
 * the call.  Stream-ordered; returns once enqueued. */
typedef struct hmcx_mlp_hmc_chains_args {
  int dtype;
  int B, n_in, n_mid, n_out, n_steps;
  int C;                      /* chains, 1 .. 64 */
  int order[6];               /* canonical variable indices 0=W1 .. 5=b3 in the caller's start order */
  double alpha;
  const void* X;              /* device [B][n_in] */
  const int32_t* y;           /* device [B] labels */
  const double* eps;          /* host [n_steps] */
  const int32_t* n_iter;      /* host [n_steps*C] */
  const double* u_accept;     /* host [n_steps*C] */
  int noise_mode;             /* HMCX_NOISE_BUFFER or HMCX_NOISE_PHILOX */
  const double* noise;        /* device, BUFFER */
  const int64_t* noise_off;   /* host [n_steps*C], BUFFER */
  int mask_mode;              /* HMCX_MLP_MASKS_NONE / _FIXED / _PHILOX */
  const void* masks;          /* device (dtype), FIXED */
  const int64_t* mask_off;    /* host [n_steps*C], FIXED: forward f of (s, c) at + f·3·B·n_mid */
  uint64_t seed;
  uint32_t chain0, step_base; /* chain c draws under Philox chain chain0 + c */
  hmcx_mlp_params par;        /* [C][shape_v] per variable, updated in place */
  double* out_A;              /* device [n_steps*C] */
  int32_t* out_accepted;      /* device [n_steps*C] */
  double* out_E;              /* device [n_steps*C][2] or NULL */
  const uint8_t* want_eval;   /* host [n_steps] or NULL */
  double* out_eval_loss;      /* device [n_evals][C] */
  double* out_eval_sumsq;     /* device [n_evals][C][6] or NULL */
  const uint8_t* want_draw;   /* host [n_steps] or NULL */
  hmcx_mlp_params draws;      /* device, [C][draw_stride][shape_v] per variable (read where want_draw is given) */
  int64_t draw_stride;        /* draws per chain of the caller's buffers */
  hmcx_mlp_params out_mom;    /* device, the layout of draws; all NULL: the momentum is not stored */
} hmcx_mlp_hmc_chains_args;
int hmcx_mlp_hmc_chains_run(hmcx_ctx* ctx, const hmcx_mlp_hmc_chains_args* a);

/* SGHMC on the MLP, n_steps steps of C chains in one call (extension; the reference runs one chain per process):
 * replaces hamiltonian/inference/cpu/sghmc.py:19-39 with the A1 completion, exactly as hmcx_mlp_sghmc_run defines it,
 * for every (step s, chain c).  All chains share the minibatch rows row0[s] .. row0[s] + B and ε = eps[s]; n =
 * n_iter[s·C + c] and u = u_accept[s·C + c] are the chain's own:
 *   1. momentum: p = P standard normals laid out variable after variable in `order` (element e = the variable's
 *      offset in that layout + its index).  HMCX_NOISE_BUFFER: noise[noise_off[s·C + c] + e] (double, converted to
 *      dtype); HMCX_NOISE_PHILOX: the Philox normal of (seed, chain0 + c, step_base + s, slot 0, e) in dtype.  The
 *      trajectory works on a copy q' ← q.
 *   2. trajectory: for it = 0 .. n − 1 and i = 0 .. 5, v = order[i]:  q'_v += ε·p_v;  g_v = the v component of
 *      hmcx_mlp_grad at q' (∇ mean CE + ½·alpha·θ) under forward f = 6·it + i;  p_v = ((1 − ε)·p_v + ε·g_v) + (2ε)·z,
 *      each product and sum rounded once in dtype (the statements of the one-chain call's update).  z: BUFFER
 *      noise[noise_off[s·C + c] + P·(it + 1) + e], PHILOX slot it + 1, element e.  No momentum negation; the dead
 *      gradient of sghmc.py:26 is not executed.  Only component v of an evaluation is computed, the layer-1 output is
 *      reused until W1 moves.
 *   3. forward 6n is the proposal's energy forward, forward 6n + 1 the current state's (hmcx_mlp_sghmc_run's
 *      numbering).  n = 0 keeps the numbering and A still comes from the two forwards: under dropout it is not 1.
 *      Masks of forward f: HMCX_MLP_MASKS_NONE no dropout; FIXED masks + mask_off[s·C + c] + f·3·B·n_mid (dtype;
 *      each chain its own block); PHILOX what hmcx_mlp_masks(seed, chain0 + c, step_base + s, 0x80000000 + f) writes.
 *   4. energies: E = (loss + log_prior) + ½Σp², loss the mean CE of the forward, log_prior = −Σ_v ½·alpha·Σθ_v²/dim_v
 *      and the kinetic term both over `order`, in float64 with a fixed summation order.
 *   5. A = min(1, exp(E_cur − E_new)) as Python's min (NaN gives 1); accepted = isfinite(A) && u < A; an accepted
 *      step commits q' to par.
 * Outputs at index s·C + c: out_A, out_accepted, out_E [·][2] = (E_current, E_new), out_loss = the mean CE of the
 * kept state under that state's energy forward, out_nlp = loss + log_prior of the kept state.  Where want_draw[s] is
 * set, the d-th such step of chain c stores the kept state at draws.p[v] + (c·draw_stride + d)·n_v.
 * Guarantees:
 *   chains   with PHILOX noise and masks chain c is bit for bit the C = 1 call with chain0 + c — state, A, E, flags,
 *            loss, nlp, draws, float64 and float32: a chain's result depends neither on C, nor on how the chains
 *            are grouped into launches, nor on the other chains' path lengths.
 *   splits   one call of n steps equals any split into calls that carry par and advance step_base (and the host
 *            arrays and the draw pointers), bit for bit.
 *   errors   invalid arguments return a negative code, set hmcx_last_error, launch nothing and leave par
 *            untouched: C outside 1 .. 64, order not a permutation, n_iter < 0 or so large that the forward number
 *            0x80000000 + 6n + 1 wraps, chain0 + C or step_base + n_steps wrapping 2^32, want_draw with draw_stride
 *            below the call's flagged steps, a missing buffer for the chosen modes; NULL ctx or args: −1.
 *   n_steps == 0 does nothing.
 * Against hmcx_mlp_sghmc_run: the same values up to the summation order inside the forwards (other GEMM launches);
 * the one-chain call stays the fused, faster path for one chain.
 * Schedule: the chains are the problems of batched launches, in groups of at most 6; a group takes all steps of the
 * call before the next group starts.  Evaluation f of a step is launched for the chains of the group that still
 * have one, so a ragged step costs max_c(6·n_c) evaluations per group.  Only unfused launches: no cross-workgroup
 * exchange, no spin-wait, no abort word.  Nothing is read back inside the call.  Stream-ordered; returns once
 * enqueued. */
typedef struct hmcx_mlp_sghmc_chains_args {
  int dtype;
  int B, n_in, n_mid, n_out, n_steps;
  int C;                      /* chains, 1 .. 64 */
  int order[6];               /* canonical variable indices 0=W1 .. 5=b3 in the caller's start order */
  double alpha;
  const void* X;              /* device [N][n_in] */
  const int32_t* y;           /* device [N] labels */
  const int64_t* row0;        /* host [n_steps] */
  const double* eps;          /* host [n_steps] */
  const int32_t* n_iter;      /* host [n_steps*C] */
  const double* u_accept;     /* host [n_steps*C] */
  int noise_mode;             /* HMCX_NOISE_BUFFER or HMCX_NOISE_PHILOX */
  const double* noise;        /* device, BUFFER */
  const int64_t* noise_off;   /* host [n_steps*C], BUFFER: P·(n + 1) normals each */
  int mask_mode;              /* HMCX_MLP_MASKS_NONE / _FIXED / _PHILOX */
  const void* masks;          /* device (dtype), FIXED */
  const int64_t* mask_off;    /* host [n_steps*C], FIXED: forward f of (s, c) at + f·3·B·n_mid */
  uint64_t seed;
  uint32_t chain0, step_base; /* chain c draws under Philox chain chain0 + c */
  hmcx_mlp_params par;        /* [C][shape_v] per variable, updated in place */
  double* out_A;              /* device [n_steps*C] */
  int32_t* out_accepted;      /* device [n_steps*C] */
  double* out_loss;           /* device [n_steps*C] */
  double* out_nlp;            /* device [n_steps*C] or NULL */
  double* out_E;              /* device [n_steps*C][2] or NULL */
  const uint8_t* want_draw;   /* host [n_steps] or NULL */
  hmcx_mlp_params draws;      /* device, [C][draw_stride][shape_v] per variable (read where want_draw is given) */
  int64_t draw_stride;        /* draws per chain of the caller's buffers */
} hmcx_mlp_sghmc_chains_args;
int hmcx_mlp_sghmc_chains_run(hmcx_ctx* ctx, const hmcx_mlp_sghmc_chains_args* a);

/* Posterior predictive of the MLP on the device (extension; the reference's predict, mlp.py:84-96, is one
 * parameter set and one mask draw per call).  D = S·T draws, draw d = s·T + t: parameter set s (par.p[i]
 * holds S stacked copies, [S][shape_i], contiguous) under dropout draw t.  z_d = net(X; θ_s, masks_d) by the
 * arithmetic of hmcx_mlp_loss, p_d = softmax(z_d) (max-subtracted).  Masks of draw d:
 *   HMCX_MLP_MASKS_NONE    no dropout (T must be 1);
 *   HMCX_MLP_MASKS_FIXED   block d of masks [D][3][N][n_mid] (dtype);
 *   HMCX_MLP_MASKS_PHILOX  the values hmcx_mlp_masks(ctx, dtype, N, n_mid, seed, chain, step, slot0 + d)
 *                          writes (slot0 + D must not wrap 2^32), drawn where they are used.
 * path: 0 picks by shape, 1 the general path (one hmcx_mlp_loss forward per draw, then a reduce launch),
 * 2 the fused row-block kernel (an error when the shape is not eligible: n_mid a multiple of 32 up to 256,
 * n_out <= 16, n_in a multiple of 8, 16-byte aligned operands, and 16 rows of X, h1 and h2 within the
 * 160 KiB of LDS).  path 0 takes the fused kernel where it is eligible and D >= 2 (there it measured
 * faster at every point) and the general path elsewhere.
 * Outputs (device; each may be NULL; float64 unless noted), sums over draws and rows in float64 and in
 * a fixed order, so equal calls give equal bits:
 *   out_mean [N][n_out]      (1/D) Σ_d p_d
 *   out_pred int32 [N]       argmax_k of the mean, lowest index on ties
 *   out_entropy [N]          −Σ_k m·log m of the mean (0·log 0 = 0)
 *   out_exp_entropy [N]      (1/D) Σ_d H[p_d]
 * and, with labels y (device int32 [N]; asking for one of these without y is an error):
 *   out_lppd [N]             log((1/D) Σ_d p_d[n][y_n])
 *   out_draw_nll [D]         the mean cross-entropy of draw d (what hmcx_mlp_loss returns for it)
 *   out_draw_correct int32 [D]   #{n : argmax z_d[n] = y_n}
 * Stream-ordered; returns once enqueued. */
typedef struct hmcx_mlp_predictive_args {
  int dtype;
  int N, n_in, n_mid, n_out, S, T;
  int mask_mode, path;
  const void* X;           /* device [N][n_in] */
  const int32_t* y;        /* device [N] or NULL */
  hmcx_mlp_params par;     /* device, each [S][shape] */
  const void* masks;       /* device [D][3][N][n_mid], FIXED */
  uint64_t seed;
  uint32_t chain, step, slot0;
  double* out_mean;
  int32_t* out_pred;
  double* out_entropy;
  double* out_exp_entropy;
  double* out_lppd;
  double* out_draw_nll;
  int32_t* out_draw_correct;
} hmcx_mlp_predictive_args;
int hmcx_mlp_predictive(hmcx_ctx* ctx, const hmcx_mlp_predictive_args* a);

/* Posterior predictive of the softmax and logistic models on the device (extension; the reference's
 * predict / predict_stochastic, models/cpu/softmax.py:82-100 and logistic.py:75-87, score one parameter
 * set and one input-dropout mask per call).  S·T draws, draw d = s·T + t: parameter set s (W [S][D][K],
 * b [S][K], stacked as sample() returns them) under input-dropout mask t of that set,
 *   z_d = clip((X ⊙ Z_d)·W_s + b_s)   (the clip bounds of softmax.py:40-41 / logistic.py:48-49),
 *   softmax:  p_d = softmax(z_d), max-subtracted;   logistic (K = 1):  p_d = 1/(1 + exp(−z_d)), the class
 *   probabilities being (1 − p_d, p_d) — S = T = 1 without masks is predict(prob=True).
 * Masks Z_d (mask_mode, the HMCX_MLP_MASKS_* values):
 *   NONE    no input dropout (T must be 1);
 *   FIXED   block d of masks, uint8 [S·T][N][D] (non-zero keeps the element);
 *   PHILOX  Z_d[n][i] = philox_uniform(seed, chain, step0 + d, 0xFFFFFFFC, n·D + i) < keep_p, the draw
 *           hmcx_sgd_run makes for sgd.fit_dropout and hmcx_input_masks writes (an error when N·D >= 2^32
 *           or step0 + S·T wraps 2^32).
 * path: 0 picks by shape (the fused kernel only where it measured no slower), 1 the general path (draws in chunks: the existing forward kernel
 * in predict mode into a chunk buffer, then a reduce launch; every shape hmcx_softmax_predict accepts),
 * 2 the fused row-block kernel (an error when the shape is not eligible: K <= 16, and 16 rows of X plus
 * the kernel's scratch within the 160 KiB of LDS).
 * Outputs as hmcx_mlp_predictive's (device; each may be NULL; float64 unless noted; the softmax, sigmoid,
 * logarithms and every sum over draws or rows in float64 and in a fixed order, so equal calls give equal
 * bits; the general path takes p_d from the existing forward kernel, in dtype, and is float64 from there):
 *   out_mean [N][K]          (1/(S·T)) Σ_d p_d   (logistic: the mean of p_d, [N][1])
 *   out_pred int32 [N]       softmax: argmax_k of the mean, lowest index on ties; logistic: mean > 0.5
 *   out_entropy [N]          entropy of the mean over the K classes (logistic: over its two), 0·log 0 = 0
 *   out_exp_entropy [N]      (1/(S·T)) Σ_d H[p_d]
 * and, with labels y (device int32 [N], class indices, 0/1 for logistic; asking for one of these without
 * y is an error):
 *   out_lppd [N]             log((1/(S·T)) Σ_d p_d[n][y_n])
 *   out_draw_nll [S·T]       −ll_d / N, ll_d = hmcx_softmax_loglik / hmcx_logistic_loglik of X ⊙ Z_d
 *   out_draw_correct int32 [S·T]   rows whose decision under draw d (argmax z_d; p_d > 0.5) equals y_n
 * A NaN parameter set reaches the per-row outputs and its own draws' out_draw_nll / out_draw_correct only.
 * Stream-ordered; returns once enqueued.  Invalid arguments return a negative code and launch nothing. */
typedef struct hmcx_linear_predictive_args {
  int dtype;
  int model;               /* HMCX_MODEL_SOFTMAX or HMCX_MODEL_LOGISTIC (K = 1)           */
  int N, D, K, S, T;
  int mask_mode, path;
  const void* X;           /* device [N][D] */
  const int32_t* y;        /* device [N] or NULL */
  const void* W;           /* device [S][D][K] */
  const void* b;           /* device [S][K] */
  const uint8_t* masks;    /* device [S·T][N][D], FIXED */
  double keep_p;           /* PHILOX */
  uint64_t seed;
  uint32_t chain, step0;
  double* out_mean;
  int32_t* out_pred;
  double* out_entropy;
  double* out_exp_entropy;
  double* out_lppd;
  double* out_draw_nll;
  int32_t* out_draw_correct;
} hmcx_linear_predictive_args;
int hmcx_linear_predictive(hmcx_ctx* ctx, const hmcx_linear_predictive_args* a);
/* out[n·D + i] (device uint8 [N][D]) = the PHILOX mask of one draw: philox_uniform(seed, chain, step,
 * 0xFFFFFFFC, n·D + i) < keep_p.  N·D must be below 2^32. */
int hmcx_input_masks(hmcx_ctx* ctx, int N, int D, double keep_p, uint64_t seed, uint32_t chain, uint32_t step,
                     uint8_t* out);

/* on = 0: hmcx_mlp_sghmc_run stops fusing layer 2 and layer 3 into one launch (no cross-workgroup
 * exchange; one more launch per forward) — the recovery path after out_abort; on = 1 restores it. */
int hmcx_set_mlp_fuse(hmcx_ctx* ctx, int on);
/* The dropout ratio of every Philox mask the context draws from then on (default 0.1): hmcx_mlp_masks,
 * hmcx_mlp_hmc_leapfrog, hmcx_mlp_sghmc_run, hmcx_mlp_sgd_run, hmcx_mlp_sgld_run, the three *_chains_run entries
 * and hmcx_mlp_predictive in their PHILOX mask modes.  An element with 24-bit uniform x is kept iff
 * x >= ceil(ratio · 2^24) and then has the value (dtype)(1 / (1 − ratio)); at 0.1 that is x >= 0x19999A and
 * (dtype)(1 / 0.9).  Valid iff 0 <= ratio and ceil(ratio · 2^24) < 2^24; anything else (negative, NaN, 1 and above)
 * returns HMCX_EINVAL with a message and leaves the ratio as it was.  FIXED / BUFFER masks are the caller's values,
 * untouched; a context shared by models of different ratios sets it before each call. */
int hmcx_set_mlp_dropout(hmcx_ctx* ctx, double ratio);
int hmcx_get_mlp_dropout(const hmcx_ctx* ctx, double* ratio);
/* Wide SGLD (config 5, hmcx_sgld_run with K ≤ 64 or several chains): fused forward + softmax (1, the
 * default) or the three-launch form (0).  A fused call given out_abort stores its verdict there
 * (stream-ordered, no host wait): 1 means a team round timed out and W / b (pW / pb) are invalid —
 * restore the start state and re-run the call with hmcx_set_sgld_fuse(ctx, 0).  Without out_abort the
 * call restores and re-runs itself and waits for its stream (hmcx_get_recoveries counts either re-run
 * once the caller reports its own with hmcx_note_recovery). */
int hmcx_set_sgld_fuse(hmcx_ctx* ctx, int on);

/* ------------------------------------------------------------------ cross-rank gather (RCCL)
 * Replaces the reference's multi-chain result collection (hamiltonian/inference/cpu/
 * sghmc_multicore.py:86-94: Pool.map of per-worker posteriors, concatenated on the parent;
 * SURVEY §8(e)): one process per GPU samples its own chains with no communication, then ONE
 * all-gather over RCCL (xGMI) moves every rank's per-chain summaries (per-parameter Welford mean /
 * M2 and a thinned trace, packed by the caller) to every rank.  The communicator is created here
 * from a unique id that rank 0 makes (hmcx_comm_unique_id) and the launcher hands to every rank
 * (any out-of-band channel: the bench uses the torch.distributed gloo store).  Collectives run on
 * the context's stream and return once enqueued. */
typedef struct hmcx_comm hmcx_comm;
#define HMCX_COMM_ID_BYTES 128
int hmcx_comm_unique_id(void* id /* host [HMCX_COMM_ID_BYTES] */);
int hmcx_comm_init(hmcx_ctx* ctx, int nranks, int rank, const void* id /* host */, hmcx_comm** out);
int hmcx_comm_destroy(hmcx_comm* comm);
/* recv[r][0..count) = send of rank r (device doubles; recv holds nranks·count) */
int hmcx_allgather_chain_stats(hmcx_ctx* ctx, hmcx_comm* comm, const double* send, double* recv, uint64_t count);
/* recv = elementwise sum (op 0) or max (op 1) over the ranks of send (device doubles): the bench's
 * leapfrog total and max-over-ranks time */
int hmcx_allreduce_f64(hmcx_ctx* ctx, hmcx_comm* comm, const double* send, double* recv, uint64_t count, int op);

/* Cross-chain convergence diagnostics on the device (the reference has none — its
 * multi-chain layer concatenates posteriors, hamiltonian/inference/cpu/sghmc_multicore.py:86-94,
 * read back by hmc.py:132-138 backend_mean).  Per parameter p < P of C chains:
 *   out[p]       R̂ from per-chain moments (means / M2 [C][P] over n_moments draws; NaN when means
 *                is NULL),
 *   out[P + p]   split-R̂ of the traces (chains halved: 2C sequences of T/2 draws),
 *   out[2P + p]  bulk ESS (Geyer's initial monotone sequence on the split sequences),
 * with the definitions of dropout_hamiltonian_montecarlo_amd/diagnostics.py (BDA3 §11.4-11.5).
 * trace: device [C][T][P] float64 (T >= 4) — e.g. the buffer hmcx_allgather_chain_stats filled;
 * means, M2, out: device float64.  Stream-ordered; returns before the kernel completes. */
int hmcx_chain_diagnostics(hmcx_ctx* ctx, int C, int T, int P, const double* trace, const double* means,
                           const double* M2, int64_t n_moments, double* out);

#ifdef __cplusplus
}
#endif
#endif /* HMCX_H */
