// hmcx_persist2.hip — single-chain SGHMC for the softmax model as ONE persistent launch per call,
// built around tagged-granule hand-offs (no counters, no fences, no grid barrier per leapfrog).
//
// Mathematics and op order: cpu/sghmc.py:19-39 with the A1 completion, cpu/softmax.py:38-79, as in
// the kernel-per-phase path (hmcx_softmax.hip).  Layout (BASELINE config 2: B=500, D=784, K=10):
//
//  * G = Gr x Gf workgroups (256 threads, one per CU, co-resident).  Workgroup (r, f) keeps the
//    minibatch tile X[R_r, F_f] in LDS for a whole step (rows R_r = Br rows, features F_f = Bf).
//  * Inside the row team r, workgroup f OWNS the row slice rho(r,f) (Ro rows); inside the feature
//    team f, workgroup r OWNS the feature slice phi(r,f) (Fo features x K weights and momenta).
//  * One leapfrog iteration = four team-local hand-off rounds, each a reduce-scatter or an
//    all-gather of a few KB:
//      A-RS  partial logits X[R_r,F_f]·W[F_f]          → owner of rho sums the Gf partials,
//            runs both softmaxes of its rows (at b and at b' = b + ε·pb), builds diff rows;
//      A-AG  diff rows + colsum/ll partials            → every member has diff[R_r];
//      B-RS  partial gradient X[R_r,F_f]ᵀ·diff         → owner of phi sums the Gr partials and
//            updates its weights/momenta (friction noise from Philox); the bias sub-step is
//            replicated from the all-row colsum that travels with the partials;
//      B-AG  drifted weights of phi                    → every member has W[F_f] for the next X·W.
//    Per step one more all-gather (kinetic and log-likelihood partials) decides the MH accept in
//    every workgroup identically.
//  * When the device has room (2·G workgroups at one per CU; HMCX_P2_HELP, default on) the same launch
//    carries G helper workgroups: helper G + b computes the step-start log-likelihood (E_current) of
//    chain workgroup b's rows from the state the chain publishes after each accept, and draws the next
//    step's momentum for it, so neither sits on the chain's critical path.
//  * Look-ahead (HMCX_P2_AHEAD / hmcx_set_sghmc_ahead, default auto → on): instead of helpers the launch
//    carries a SECOND chain team on those G workgroups.  Lane 0 runs the even steps, lane 1 the odd ones, each
//    assuming that the step before it rejects (≈ 91 % do at the benchmark's settings); a step whose assumption
//    failed is run again from the true state, so every step that counts is computed exactly as without it.
//    A run whose assumption is known to have failed is left at the next leapfrog boundary the lane agrees on
//    (the verdict is polled once per iteration), not finished first.  A run that ends with the verdict still
//    unknown, and leaves the state as it was, is parked (HMCX_P2_RUNON, default on): the lane starts its next
//    step at once and the same poll resolves the verdict while that runs.
//  * The two GEMMs run on MFMA (v_mfma_f64_16x16x4 / f32_16x16x4) with operands from the LDS tile;
//    the class dimension (KC = 10 compiled in, 16 generic) pads to the 16-wide tile.  A VALU
//    variant with the classes in registers measured 1.7x slower (LDS-latency bound).
//  * Transport: every value travels as one 16-byte granule {lo32, epoch, hi32, epoch} written by
//    ONE `buffer_store_dwordx4 … sc1` and read by `buffer_load_dwordx4 … sc1`; a consumer re-reads
//    a granule until both epoch words match (cdna_hip_programming.md §6 G16, recipe R2: the data
//    is the flag).  Epochs count rounds over the arena's whole life (each launch reserves a fresh
//    range, sghmc_p2_t), so an epoch is never written twice and the arena is NOT cleared per launch.
//    Measured on MI355X (tools/microbench_handoff.hip): one team round of 8 x 80-130 granules
//    ≈ 1.4-1.6 µs, against 3-3.4 µs for payload + counter barrier.
// All reductions run in a fixed order, so the replicated state is bit-identical in every
// workgroup and runs are deterministic.
#include "hmcx_common.h"
#include "hmcx_internal.h"
#include "hmcx_persist.h"
#include "hmcx_p2x.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace hmcx {


struct Q2Args {
  int B, D, K, P, n_steps;
  int Gr, Gf, Br, Bf, BfP, BFP, Ro, Fo;
  double alpha, neg_inv_n, log_prior;
  const void* X; const void* Y;
  const double* eps; const double* u; const int64_t* row0; const int32_t* n_iter;
  int noise_mode; const double* noise; const int64_t* noff;
  uint64_t seed; uint32_t chain0, step_base;
  void* W; void* b;
  char* arena;                              // granule arena (the context's; epochs are unique over its life)
  // Region offsets in granules.  XA, XD, XB, XW and XS are double-buffered by the parity of a per-region
  // use counter, so a producer P overwrites the granule of its use u at its use u + 2.  The poll passes
  // (hmcx_p2x.h) carry nothing from one pass to the next, so a consumer C needs every granule of use u to
  // stay in place until C's pass that sees them all.  Every consume ends in a workgroup barrier (all_ok),
  // so "P consumed" below means all of P's threads did.  Per region, for teams of any size:
  //  XA (A-RS, row team): between P's uses u and u + 2 lies an A-AG consume of P (rounds run A, [A,] D, B,
  //     [W,] A …) or an accept round (across a step boundary), in which P polls the header or the partials
  //     of EVERY row-team member (a member that owns no softmax rows polls nothing in A-RS, but always
  //     those).  C publishes them only after its consume of A(u).
  //  XD (A-AG, row team): P reaches use u + 2 through its consume of D(u + 1), which polls C's block of
  //     D(u + 1); C published it after its consume of D(u).
  //  XB (B-RS / B all-reduce, feature team): the same through B(u + 1): with `bar` every member polls every
  //     producer's whole block; without it the header threads poll all Gr headers.
  //  XW (B-AG, `bar` off, feature team): a member may poll only the producers that own features, so W(u + 1)
  //     does not order P behind C; but between W(u) and W(u + 2) P consumes a B-RS round, whose header it
  //     polls from every member, and C publishes that B round only after its consume of W(u).
  //  XS (accept, all G): P's consume of S(u + 1) polls C's partials, published after C's consume of S(u).
  //  XC (commit, one use per launch): written once per launch with the launch's last epoch; the next
  //     write is by the next launch on the same stream, which starts after every workgroup of this one,
  //     workgroup 0 and its gather included, has ended.
  // Helper regions (help: workgroup G + b computes E_current and draws p0 for chain workgroup b).  Step s uses parity
  // s & 1 of each; E(s) is the chain's accept epoch of step s, which a helper derives from the schedule.
  //  ll0 slot (granule 2 of a chain workgroup's XS record, written by its helper with E(s)): every chain
  //     workgroup polls it in accept s.  Its helper P rewrites it for step s + 2, which it starts only with
  //     q(s+2) in hand; the chain publishes q(s+2) after its consume of accept s + 1, and no workgroup
  //     publishes its S(s + 1) partials before its consume of S(s).
  //  XQ (state q(s), feature team of chain → same team of helpers, epoch E(s − 1)): chain member P rewrites
  //     its block for q(s+2) after its consume of accept s + 1, which polled the ll0(s + 1) of EVERY helper;
  //     helper C publishes that only after its consume of XQ(s + 1), later than its consume of XQ(s).
  //  XAh (the helpers' A-RS, row team of helpers, epoch E(s)): helper P reaches step s + 2 only with
  //     q(s+2), published after an accept s + 1 that polled the ll0(s + 1) of every helper C — published
  //     after C's A-RS consume of step s + 1, later than that of step s.
  //  XP (momentum p0(s) of the slice, feature team of helpers → same team of chain, epoch
  //     E(s − 1); E(−1) is the launch's first epoch): helper P rewrites its block for p0(s + 2) after its
  //     ll0(s + 1), for which it consumed XQ(s + 1) from EVERY chain member C of its feature team; C
  //     publishes q(s+1) at the end of step s, after it consumed p0(s) at the start of step s.
  // So no chain workgroup passes accept s without every helper's ll0(s), no helper starts step s + 1
  // without the post-accept publish of q(s+1), and the skew between the two halves is at most one step.
  // Look-ahead regions (ahead: lane l = blocks [l·G, (l + 1)·G) runs the steps k ≡ l mod 2; each lane has
  // XA … XS regions and an epoch sequence of its own, for which the arguments above hold lane by lane — a
  // redone step is one more step of the lane's sequence).  Both cross-lane records carry the tag T(k) =
  // ep0 + k of the step, never a lane epoch, and live in the slot of parity k & 1, which is the lane.
  //  XV (verdict V(k): "step k is final and did / did not change the state", workgroup b of lane k & 1 →
  //     its twin b of the other lane): V(k + 2) is written when step k + 2 is final, after this workgroup
  //     read V(k + 1); its twin publishes V(k + 1) only after it read V(k).
  //  XQ (state q(k+1) after an accepted step k, feature team of lane k & 1 → same team of the other lane,
  //     written before V(k)): member P rewrites its block for step k + 2 after it read V(k + 1) from its
  //     twin, which published it after its accept round of the final run of step k + 1; that round polled
  //     the partials of EVERY workgroup of the twin's lane, each published after its gather of XQ(k) (a
  //     lane gathers XQ(k) before it redoes step k + 1, or, lane 0 at the end of the call, never rewrites).
  // The oldest unresolved step waits for nothing (V(k − 1) is published before its lane goes on), so the
  // lanes cannot wait for each other in a cycle.
  // Stopped runs (a speculative run of step k + 1 that the lane leaves at a leapfrog boundary once V(k) =
  // "changed" is known lane-wide; every workgroup of the lane leaves at the SAME boundary, so inside the
  // lane the sequence of rounds only gets shorter and the arguments for XA … XS hold as they stand: across
  // the stop the rounds run … A, D, B, [W,] | A (redo, it = −1), A, D, B …, and the D consume of the last
  // iteration lies between the A uses of equal parity as the accept round does across a step boundary):
  //  XV: a workgroup b that stops on the lane's flag may never have read V(k) from its own twin b'.  It no
  //     longer needs it: the redo reads no verdict, and b' overwrites the slot with V(k + 2) only after it
  //     read V(k + 1), which b publishes after the redo.  The slot's next poll by b is for the tag of
  //     V(k + 2); a V(k) still in place carries T(k) and does not match.
  //  XQ: b gathers XQ(k) by its tag T(k) whether or not it saw V(k) itself; the twin lane publishes it
  //     unconditionally (every one of its workgroups computed the same "changed"), before its V(k), so the
  //     gather waits for nothing that depends on b.  It still precedes the redo, whose accept round is what
  //     the XQ argument above rests on.
  //  A stopped run's granules stay in their slots with the run's epochs; the lane's epoch then jumps to the
  //     value the full run would have reached, so every later round polls for an epoch larger than any the
  //     stopped run wrote, and a slot the stopped run never reached holds an older one still.
  // Parked steps (runon: a speculative run of step p that ends with V(p − 1) unknown to the WHOLE lane and with
  // the own decision "state unchanged" is parked — nothing published but the step's outputs — and the lane
  // starts step p + 2 on the prefetched tile; V(p − 1) is then looked for by the poll of that run, at the latest
  // before its accept round.  Whether the lane parks is decided from item 3 of the accept records, in which
  // every workgroup reports what its own poll has read: the lane parks only when no workgroup has read
  // V(p − 1), so all of them park or none does, and every workgroup of a lane is in the same run at all times):
  //  XV, twin side: the twin overwrites the slot of V(p − 1) with V(p + 1) only after it read V(p) from THIS
  //     workgroup, and this workgroup publishes V(p) only after it read V(p − 1) itself (in flight or in the
  //     blocking wait), after the redo of p, or when it leaves the run of p + 2 on the lane's flag for V(p + 1) =
  //     "changed" (next entry).  Nobody acts on another workgroup's reading of an "unchanged" verdict.
  //  XV, stopped workgroup: the flag carries its reason.  Left on "V(p − 1) changed" (4096 per flag), a
  //     workgroup that has not read V(p − 1) never needs it: the redo of p reads no verdict.  Left on "V(p + 1)
  //     changed" (1 per flag), some twin published V(p + 1), which it does only after it read a V(p), and no
  //     V(p) exists before V(p − 1) = "unchanged" is read (a "changed" one makes the whole lane redo p first): the
  //     step p is final, the workgroup publishes V(p) = unchanged unread and never polls for T(p − 1) again.
  //     The two reasons exclude each other within a run, so the sum of the flags tells them apart.
  //  XQ, own side: a parked step publishes no XQ (only an unchanged state is parked; the redo publishes as ever).
  //  XQ, twin side: XQ(p − 1) is gathered before the redo of p; the twin rewrites that parity for step p + 1
  //     only after it read V(p), which is published after the redo.
  //  Tile: the buffer of tile p is loaded again (tile p + 4) only in the accept round of p + 2, behind the
  //     resolution of p.
  //  XA … XS: the lane's sequence of rounds is that of a lane that ran p, p + 2 [, p again, p + 2 again]; a run
  //     of p + 2 voided at its end is left behind its last B round like a stopped one, and only steps with
  //     leapfrogs are started on a parked one, so a D consume lies between the A uses of equal parity.
  //  Outputs: out_A … out_E of step p are written when it is parked and written again by a redo.  They are read
  //     by the host behind the launch only; a launch that aborts is re-run as a whole.
  //  Progress: a lane parks step p only with its step p − 2 resolved, i.e. with V(p − 2) published, so the twin's
  //     step p − 1, the oldest unresolved step, waits for nothing, also with both lanes parked at once.
  int oXA, oXD, oXB, oXW, oXS;
  int oXC;                                  // commit round: one granule per workgroup
  int oXAh, oXQ, oXP;
  int help;                                 // 2: helper workgroups G … 2G − 1 compute E_current and draw the
                                            // step's momentum (HMCX_P2_HELP); 0: none
  int arena_bytes;
  int pad;                                  // line-aligned producer blocks (HMCX_P2_PAD, default on)
  unsigned ep0;                             // first round epoch of this launch (unique in the arena's life)
  int zoff;                                 // noise off the A-RS pollers (HMCX_P2_ZOFF, default on)
  int spread;                               // rounds with spread gathers, bits A-RS, A-AG, B-RS, B-AG
                                            // (HMCX_P2_SPREAD=<mask>; default A-AG, where it measured faster)
  int xmap;                                 // 1: logical id (b % 8)·(G/8) + b/8 — row teams on one XCD
  int fl2;                                  // feature teams share an XCD: B-round stores plain (kept in L2)
  int al2;                                  // row teams share an XCD (xmap): A-round stores plain
  int prefetch;                             // 1: next step's tile/labels loaded during the accept round
  int acc1;                                 // 1: accept partials polled in one batch (HMCX_P2_ACC1)
  int bar;                                  // 1: round B is an all-reduce by redundant reads (every feature-
                                            // team member sums all Gr partials of the WHOLE slice and updates
                                            // it identically) — no B-AG round (HMCX_P2_BAR, default on)
  int* abort_flag;                          // the context's sticky abort word (hmcx_clear_abort)
  int force_abort;                          // HMCX_P2_FORCE_ABORT=<step>: the last workgroup raises the
                                            // abort word at that step (tests the recovery path); −1 off
  double* out_A; int32_t* out_acc; double* out_ll; double* out_E;
  void* out_trace;                          // [n_steps][P] state after every step, or null
  void* out_mom;                            // [P] momentum returned by the last step, or null
  unsigned long long* prof;                 // HMCX_PERSIST_PROF=1: per-segment s_memtime totals (workgroup 0)
  unsigned long long* trace;                // HMCX_P2_TRACE=1: [G][P2TR_IT][8] s_memrealtime stamps (step 0)
  int* verdict;                             // this launch's abort verdict (hmcx_sampler_args::out_abort), or
                                            // null: 0 stored by workgroup 0 on completion, 1 by every
                                            // workgroup that leaves early (no device-to-device copy)
  int ninl;                                 // > 0: the schedule of the call's ninl steps rides in inl (no
                                            // host-to-device upload); 0: eps / u / row0 / n_iter above
  struct { double eps, u; int64_t row0; int32_t n_iter, pad_; } inl[32];
  // look-ahead (declared last: the kernel-argument offsets of everything above are the parent's)
  int ahead;                                // 1: look-ahead (HMCX_P2_AHEAD): blocks [G, 2G) are a second chain team
                                            // ("lane 1") that runs the odd steps, each under the assumption
                                            // that the step before it rejects; help is 0 then
  int laneoff;                              // lane 1's XA, XD, XB, XW and XS: lane 0's offsets plus this
  int oXV;                                  // verdict records, 8 granules (one line) per workgroup and lane
  int* stats;                               // [12] look-ahead counters, 4 per lane (workgroup 0 of each): runs redone,
                                            // runs stopped in flight, leapfrog iterations skipped, steps parked;
                                            // [8 + lane]: parked steps whose verdict came back "changed"
  int runon;                                // 1: a lane whose verdict is pending parks the step and starts its next
                                            // one (HMCX_P2_RUNON, default on; look-ahead launches only)
};
constexpr int P2_NINL = 32;                 // calls of up to this many steps pass their schedule inline
// One schedule value of step s: the kernel-argument copy (inline calls) and the global array are both
// loaded and the value selected.  A conditional `inl ? a.inl[s].x : a.x[s]` became one load through a
// pointer that may be the kernarg segment or global memory — a flat load, which every later
// `s_waitcnt lgkmcnt` (LDS traffic) then also waited for.  Inline calls point the arrays at zeros.
__device__ inline int sched_k(int s) { return s < P2_NINL ? s : P2_NINL - 1; }
template <typename V>
__device__ inline V sched_at(bool inl, int s, V kv, const V* g) {
  const V gv = g[inl ? 0 : s];
  return inl ? kv : gv;
}

// Writes the launch's abort verdict when a workgroup leaves the kernel without committing (a timed-out
// hand-off, a sticky abort word, or a decided abort): 1.  The host zeroes the verdict before the launch
// and nothing stores 0, so the verdict is sticky — an abort is never overwritten (the commit decision
// makes "no workgroup stored 1" and "every workgroup committed" the same event).
struct P2Verdict {
  int* out;
  bool done;
  __device__ ~P2Verdict() {
    if (out && !done) out[0] = 1;
  }
};
constexpr int P2TR_IT = 16;                 // traced leapfrog iterations
// HMCX_P2_HELP when the environment does not set it, and the mode folded into the config-2 instantiation
#ifndef HMCX_P2_HELP_DEFAULT
#define HMCX_P2_HELP_DEFAULT 2
#endif

// Segment profiler (workgroup 0, thread 0): s_memtime deltas accumulate in LDS (a global
// read-modify-write per stamp would add a memory round trip to the critical path); flushed once.
struct P2Prof {
  unsigned long long* out;
  unsigned long long* acc;   // LDS [16]
  unsigned long long last;
  int cur;
  __device__ inline void stamp(int next) {
    if (!out) return;
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    if (last) acc[cur] += t - last;
    last = t;
    cur = next;
  }
  __device__ inline void flush() {
    if (!out) return;
    for (int i = 0; i < 16; ++i) out[i] = acc[i];
  }
};


// Noise value of flat element e for slot `slot` of step s: Philox block z4 (already generated for
// block e >> 2) or the host-drawn buffer (cpu/sghmc.py:21,31 draw order).
template <typename T>
__device__ inline T noise_at(const Q2Args& a, int s, uint32_t slot, uint32_t e, const T* z4) {
  if (a.noise_mode == HMCX_NOISE_BUFFER) return (T)a.noise[a.noff[s] + (int64_t)slot * a.P + e];
  return z4[e & 3];
}
template <typename T>
__device__ inline void philox4_if(const Q2Args& a, int s, uint32_t slot, uint32_t g, T z[4]) {
  if (a.noise_mode != HMCX_NOISE_BUFFER) philox_normal4(opaque_s64(a.seed), a.chain0, a.step_base + (uint32_t)s, slot, g, z);
}
// One element's noise (f32 chains: float Box–Muller; f64 chains: the double one, hmcx_common.h).
template <typename T>
__device__ inline T noise1(const Q2Args& a, int s, uint32_t slot, uint32_t e) {
  if (a.noise_mode == HMCX_NOISE_BUFFER) return (T)a.noise[a.noff[s] + (int64_t)slot * a.P + e];
  return philox_normal_t<T>(opaque_s64(a.seed), a.chain0, a.step_base + (uint32_t)s, slot, e);
}

// Minibatch tile X[row0:+nrow, feat0:+nfeat] → LDS [Br][BFP], zero padded to BfP columns;
// 16-byte loads, 8 in flight per thread when rows are 16-byte aligned.
template <typename T>
__device__ inline void load_tile(T* Xs, const T* Xg, int Br, int BfP, int BFP, int nrow, int nfeat, int row0,
                                 int feat0, int D) {
  constexpr int V = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int PR = BfP / V;                        // vectors per tile row
  const float inv = 1.0f / (float)PR;
  const int total = Br * PR;
  const bool vec_ok = (D % V) == 0 && (feat0 % V) == 0 &&
                      ((reinterpret_cast<uintptr_t>(Xg) & 15) == 0);
  for (int base = threadIdx.x; base < total; base += 8 * QTH) {
    vec_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * QTH;
      const int i = qdiv(e, inv), j = (e - i * PR) * V;
      const T* src = Xg + (size_t)(row0 + i) * D + feat0 + j;
      if (e < total && i < nrow && j + V <= nfeat && vec_ok) {
        v[u] = *reinterpret_cast<const vec_t*>(src);
      } else {
#pragma unroll
        for (int q = 0; q < V; ++q) v[u][q] = (e < total && i < nrow && j + q < nfeat) ? src[q] : T(0);
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * QTH;
      if (e < total) {
        const int i = qdiv(e, inv), j = (e - i * PR) * V;
#pragma unroll
        for (int q = 0; q < V; ++q) Xs[i * BFP + j + q] = v[u][q];
      }
    }
  }
}

// One step's minibatch rows: the X tile of this workgroup and the labels of its softmax rows
// (label loads issued first so they travel with the tile's).
template <typename T>
__device__ inline void load_step_rows(T* Xs, T* Yo, const T* Xg, const T* Yg, int Br, int BfP, int BFP, int nrow,
                                      int nfeat, int row0, int feat0, int D, int K, int Ro, int nro, int ro0) {
  const int tid = threadIdx.x;
  T y = T(0);
  if (tid < Ro * 16) {                       // Ro·16 ≤ QTH (plan_p2: Ro·KC + KC + 1 ≤ QTH, KC ≥ 10)
    const int ii = tid >> 4, k = tid & 15;
    if (ii < nro && k < K) y = Yg[(size_t)(row0 + ro0 + ii) * K + k];
  }
  for (int e = tid + QTH; e < Ro * 16; e += QTH) {
    const int ii = e >> 4, k = e & 15;
    Yo[e] = (ii < nro && k < K) ? Yg[(size_t)(row0 + ro0 + ii) * K + k] : T(0);
  }
  load_tile<T>(Xs, Xg, Br, BfP, BFP, nrow, nfeat, row0, feat0, D);
  if (tid < Ro * 16) Yo[tid] = y;
}

// C[16 x 16] += A[16 x 4·nk] · B[4·nk x 16] on one wave (v_mfma_*_16x16x4).  Lane group lg of k-step kk
// holds A(i, ·) = a[i·as_i + lg·a_lg + kk·a_kk] and B(·, j) = b[lg·b_lg + kk·b_kk + j]: (a_lg, a_kk) =
// (as_k, 4·as_k) walks k in order, (a_lg, a_kk) = (nk·as_k, as_k) lets the four lane groups of one
// k-step read k values nk apart (the same 4·nk terms, summed in another grouping).  Operands of 8
// k-steps are loaded before their MFMAs, two accumulators alternate.  Returns the D fragment (rows
// M::row(lane, q), column lane & 15).
template <typename T>
__device__ inline typename mfma16<T>::acc_t mfma_tile(const T* a, int as_i, int a_lg, int a_kk, const T* b, int b_lg,
                                                      int b_kk, int nk) {
  using M = mfma16<T>;
  const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
  const T* pa = a + lr * as_i + lg * a_lg;
  const T* pb = b + lg * b_lg + lr;
  typename M::acc_t c0 = M::zero(), c1 = M::zero();
  int kk = 0;
  for (; kk + 8 <= nk; kk += 8) {
    T av[8], bv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      av[u] = pa[(kk + u) * a_kk];
      bv[u] = pb[(kk + u) * b_kk];
    }
#pragma unroll
    for (int u = 0; u < 8; u += 2) {
      c0 = M::fma(av[u], bv[u], c0);
      c1 = M::fma(av[u + 1], bv[u + 1], c1);
    }
  }
  // tail: the two accumulators still alternate (two dependent MFMA chains, not one)
  for (; kk + 2 <= nk; kk += 2) {
    c0 = M::fma(pa[kk * a_kk], pb[kk * b_kk], c0);
    c1 = M::fma(pa[(kk + 1) * a_kk], pb[(kk + 1) * b_kk], c1);
  }
  if (kk < nk) c0 = M::fma(pa[kk * a_kk], pb[kk * b_kk], c0);
  return c0 + c1;
}

template <typename T, int KC, int SPEC = 0>
__global__ __launch_bounds__(QTH) void k_sghmc_p2(Q2Args a) {
  using M = mfma16<T>;
  // SPEC = 1: the plan of BASELINE config 2 (f64, B=500, D=784, K=10: 8 x 16 teams, 64-row x 49-feature
  // tiles) with every knob at its default, folded into constants — fewer live scalars (the generic
  // kernel spills SGPRs into VGPR lanes) and no runtime branches on the knobs
  constexpr bool SP = SPEC != 0;
  const int spread = SP ? 2 : a.spread, pad = SP ? 1 : a.pad, xmap = SP ? 0 : a.xmap, fl2 = SP ? 1 : a.fl2,
            al2 = SP ? 0 : a.al2, prefetch = SP ? 1 : a.prefetch, acc1 = SP ? 1 : a.acc1,
            zoffa = SP ? 1 : a.zoff, bara = SP ? 1 : a.bar;
  // E_current and the step's momentum p0 come from helper workgroups
  // SPEC = 4 (5 with the segment profiler): config 2 folded with look-ahead, two chain lanes and no helpers
  const bool ah = SP ? SPEC >= 4 : a.ahead != 0;
  const bool hp = !ah && (SP ? HMCX_P2_HELP_DEFAULT : a.help) != 0;
  extern __shared__ __align__(16) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15;
  const int Gr = SP ? 8 : a.Gr, Gf = SP ? 16 : a.Gf, G = Gr * Gf;
  // workgroups are dealt to the 8 XCDs round-robin by blockIdx: with the identity map feature team
  // f (blocks f, f+Gf, …) shares an XCD when Gf % 8 == 0; xmap = 1 puts each row team on one XCD
  // helper G + b is the twin of chain workgroup b: same (r, f) and tile, and the same XCD whenever a team
  // region is kept in an XCD's L2 (fl2 / al2 need G % 8 == 0, so blockIdx % 8 is equal)
  const bool helper = hp && (int)blockIdx.x >= G;
  const int lanei = (ah && (int)blockIdx.x >= G) ? 1 : 0;              // look-ahead: the lane of this workgroup
  const int pbid = (helper || lanei) ? (int)blockIdx.x - G : (int)blockIdx.x;
  const int bid = xmap ? (pbid & 7) * (G >> 3) + (pbid >> 3) : pbid;
  const int r = bid / Gf, f = bid - (bid / Gf) * Gf;
  const int Br = SP ? 64 : a.Br, Bf = SP ? 49 : a.Bf, BfP = SP ? 64 : a.BfP, BFP = SP ? 65 : a.BFP, Ro = SP ? 4 : a.Ro,
            Fo = SP ? 7 : a.Fo;
  const int K = SP ? 10 : a.K, D = SP ? 784 : a.D, B = SP ? 500 : a.B;
  const int row0 = r * Br, feat0 = f * Bf;
  const int nrow = max(0, min(Br, B - row0));
  const int nfeat = max(0, min(Bf, D - feat0));
  const int ro0 = f * Ro, nro = max(0, min(Ro, nrow - ro0));            // my softmax rows
  const int fo0 = r * Fo, nfo = max(0, min(Fo, nfeat - fo0));           // my owned features
  const T hi = (T)CLIP_HI, lo = (T)CLIP_LO;
  const T alpha = (T)a.alpha;
  const __amdgpu_buffer_rsrc_t rs = arena_rsrc(a.arena, a.arena_bytes);
  // MFMA work split: phase A m-tiles = Br/16 rows (k over BfP features), phase B m-tiles = BfP/16
  // features (k over Br rows); split-K parts when the tiles are fewer than the waves
  const int MTA = Br / 16, WPA = max(1, QNW / MTA);
  const int MTB = BfP / 16, WPB = max(1, QNW / MTB);
  const int HA = KC + 1;                              // payload header: colsum[KC], ll
  // payload blocks per producer, rounded to whole 128-byte lines (8 granules) when pad is set
  const int NXA0 = HA + Ro * KC;                      // A-AG payload per producer
  const int NXA = p2_pad(NXA0, pad);                // ... and its block stride
  const int NXB = p2_pad(HA + Bf * KC, pad);        // B-RS payload per producer
  const int NXS = pad ? 8 : 4;                      // accept partials per workgroup

  // ---- LDS carve-up (mirrored by p2_lds)
  T* Xs = reinterpret_cast<T*>(smem);                 // [Br][BFP]
  T* Wf = Xs + (size_t)Br * BFP;                      // [BfP][16] weights of F_f
  T* Wf0 = Wf + BfP * 16;                             // [BfP][16] step-start copy
  T* Ds = Wf0 + BfP * 16;                             // [Gf·Ro][16] diff of the row tile
  T* Zp = Ds + Gf * Ro * 16;                          // split-K partials: [WPA][Br][16] | [WPB][BfP][16]
  const int ZPN = max(WPA * Br, WPB * BfP) * 16;
  T* Zo = Zp + ZPN;                                   // [Ro][16] logits of my rows
  T* Yo = Zo + Ro * 16;                               // [Ro][16] labels of my rows
  T* Dme = Yo + Ro * 16;                              // [Ro][16] diff of my rows
  T* Csr = Dme + Ro * 16;                             // [Ro][16] y − ŷ' of my rows
  T* bsh = Csr + Ro * 16;                             // [16] b
  T* pbsh = bsh + 16;                                 // [16] pb
  T* b0sh = pbsh + 16;                                // [16] b at step start
  T* bpsh = b0sh + 16;                                // [16] b'
  T* pb0sh = bpsh + 16;                               // [16] pb drawn at step start
  size_t off = ((size_t)(reinterpret_cast<char*>(pb0sh + 16) - smem) + 15) & ~(size_t)15;
  double* rowll = reinterpret_cast<double*>(smem + off);  // [Ro] ll of my rows
  double* hdr = rowll + Ro;                               // [16] all-row colsum, ll
  double* dsh = hdr + 16;                                 // [16] reductions
  int* ish = reinterpret_cast<int*>(dsh + 16);            // [4] flags
  unsigned long long* profacc = reinterpret_cast<unsigned long long*>(ish + 4);   // [16]
  double* stg = reinterpret_cast<double*>(profacc + 16);                             // [QSTAGE] spread gathers
  T* zbuf = reinterpret_cast<T*>(stg + QSTAGE);                                      // [Fo·KC + 16] noise
  T* pWs = zbuf + Fo * 16 + 16;                       // [BfP][16] momentum of the whole slice (bar)
  T* Xs2 = pWs + BfP * 16;                            // look-ahead: second tile [Br][BFP] and labels [Ro][16];
  T* Yo2 = Xs2 + (size_t)Br * BFP;                    // a step's tile stays until the step is final
  T* Xc = Xs;                                         // tile and labels of the current step
  T* Yc = Yo;
  // friction noise by the waves that do not poll A-RS (threads from NZ0 on), when they fit.  NZ0 comes
  // from the plan's Ro, not this member's nro: zoff decides `bar`, the protocol of round B, which every
  // workgroup must agree on — with a per-member nro, a member owning no rows (B = 40, D = 32: plan 2x2,
  // rows 32-39 in row team 1) chose the all-reduce while its team ran RS + AG, and the launch waited out
  // its 4 s timeout before the recovery re-ran it
  const int NZ0 = ((Ro * KC + 63) / 64) * 64;
  const bool zoff = zoffa && !(spread & 1) && NZ0 + Fo * KC + K <= QTH;
  // B all-reduce (bara) needs the owners' noise in LDS (zoff) to fold it into their partials
  const bool bar = bara && zoff;
  const auto all_items = [](int, int) { return true; };

  // owned weight of this thread: feature fo0 + od, class ok (thread t = od·KC + ok)
  const int od = tid / KC, okc = tid - (tid / KC) * KC;
  const bool own = od < nfo && okc < K;
  const int e_own = (feat0 + fo0 + od) * K + okc;     // flat index (W is [D][K])
  const int wl = (fo0 + od) * 16 + okc;               // index in Wf
  T pw = T(0), wv = T(0), w0 = T(0), zn = T(0);

  P2Verdict verdict{threadIdx.x == 0 ? a.verdict : nullptr, false};
  const bool inl = a.ninl > 0;
  // a launch behind a timed-out one (sticky abort word) leaves everything untouched
  if (__hip_atomic_load(a.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  if (tid == 0) ish[0] = 0;
  if (tid < 16) profacc[tid] = 0ull;
  for (int e = tid; e < BfP * 16; e += QTH) {
    const int i = e >> 4, k = e & 15;
    Wf[e] = (i < nfeat && k < K) ? reinterpret_cast<const T*>(a.W)[(size_t)(feat0 + i) * K + k] : T(0);
  }
  for (int e = tid; e < Gf * Ro * 16; e += QTH) Ds[e] = T(0);
  for (int e = tid; e < Ro * 16; e += QTH) { Dme[e] = T(0); Csr[e] = T(0); }
  if (tid < 16) bsh[tid] = tid < K ? reinterpret_cast<const T*>(a.b)[tid] : T(0);
  __syncthreads();
  if (own) wv = Wf[wl];

  // segment profiler: compiled out of the config-2 instantiation (SPEC = 1); SPEC = 3 is that
  // instantiation with it (HMCX_PERSIST_PROF=1 at the config-2 shape)
  P2Prof prof{((!SP || SPEC == 3 || SPEC == 5) && bid == 0 && tid == 0 && !helper && a.prof) ? a.prof + 16 * lanei : nullptr,
              profacc, 0ull, 0};
  // round trace: slot 2·round = payload published, 2·round + 1 = consumed (rounds A, D, B, W)
  unsigned long long* trb = (!SP && a.trace && !helper) ? a.trace + (size_t)bid * P2TR_IT * 8 : nullptr;
  auto tstamp = [&](int s_, int it_, int slot) {
    if (trb && tid == 0 && s_ == 0 && it_ >= 0 && it_ < P2TR_IT) trb[it_ * 8 + slot] = __builtin_amdgcn_s_memrealtime();
  };
  // round epoch (same sequence in every workgroup); with helpers the launch's first epoch is E(-1), the
  // "accept epoch" before step 0
  unsigned ep = a.ep0 - 1 + (hp ? 1u : 0u);
  unsigned uA = 0, uD = 0, uB = 0, uW = 0, uS = 0;    // per-region use counters (buffer parity)

  // ---- phase A: partial logits X[R_r,F_f]·W[F_f] → XA(par, r, f) [nrow][KC], then A-RS consume:
  //      Zo[ii][k] = Σ_f' partials of my rows (f' order)
  // Two A rounds may be in flight (the step-start round of E_current and iteration 0's): each is
  // published into region parity `par` with its own epoch (epA[par]), and consumed from the same.
  unsigned epA[2] = {0u, 0u};
  const int lno = lanei ? a.laneoff : 0;              // look-ahead: lane 1's copies of the five round regions
  const int oXA = helper ? a.oXAh : a.oXA + lno;      // the helpers' A-RS rounds have a region of their own
  const int oXD = a.oXD + lno, oXB = a.oXB + lno, oXW = a.oXW + lno, oXS = a.oXS + lno;
  auto roundA = [&](int par) -> bool {
    const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6, lr = lane & 15;   // not hoisted (registers)
    epA[par] = ++ep;
    const int reg = oXA + ((par * Gr + r) * Gf + f) * Br * KC;
    // zero-padded tail skipped; config 2: 49 features in every feature team → 13 k-steps (a constant:
    // the k loop unrolls completely)
    const int nkp = SP ? 13 : WPA == 1 ? (nfeat + 3) / 4 : (BfP / 4) / WPA;
    for (int item = wave; item < MTA * WPA; item += QNW) {
      const int mt = item % MTA, part = item / MTA;
      const typename M::acc_t c = mfma_tile<T>(Xc + mt * 16 * BFP + part * nkp * 4, BFP, 1, 4,
                                               Wf + part * nkp * 4 * 16, 16, 64, nkp);
      if (WPA == 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = mt * 16 + M::row(lane, q);
          if (row < nrow && lr < KC) put_t(al2, rs, reg + row * KC + lr, (double)c[q], epA[par]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) Zp[(part * Br + mt * 16 + M::row(lane, q)) * 16 + lr] = c[q];
      }
    }
    if (WPA > 1) {
      __syncthreads();
      for (int e = tid; e < nrow * KC; e += QTH) {
        const int i = e / KC, k = e - (e / KC) * KC;
        T v = Zp[i * 16 + k];
        for (int p = 1; p < WPA; ++p) v += Zp[(p * Br + i) * 16 + k];
        put_t(al2, rs, reg + e, (double)v, epA[par]);
      }
    }
    return true;
  };
  auto consumeA = [&](int par) -> bool {
    const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6, lr = lane & 15;   // not hoisted (registers)
    const int base0 = oXA + (par * Gr + r) * Gf * Br * KC;
    const unsigned ep = epA[par];
    ++uA;
    if (spread & 1) {
      const int ni = nro * KC;
      const bool ok = gather(rs, base0, Br * KC, Gf, ni, [&](int i) { return ro0 * KC + i; }, all_items, ep,
                             a.abort_flag, stg);
      if (!all_ok(ok, ish)) return false;
      if (tid < ni) {
        double z = stg[tid];
        for (int p = 1; p < Gf; ++p) z += stg[p * ni + tid];
        Zo[(tid / KC) * 16 + (tid % KC)] = (T)z;
      }
      __syncthreads();
      return true;
    }
    double z = 0.0;
    const bool ok = poll<true>(rs, base0, Br * KC, Gf, -1, ro0 * KC + tid, tid < nro * KC, ep, nullptr, 0, &z,
                               a.abort_flag);
    if (tid < nro * KC) Zo[(tid / KC) * 16 + (tid % KC)] = (T)z;
    return all_ok(ok, ish);
  };

  // ---- helpers on: the slice's momentum p0(s) arrives from the helpers (XP).  Item j < nfeat·KC is class
  //      j % KC of slice feature j / KC (from the member that owns it), then KC bias items from member 0;
  //      two items per thread and chunk.  The loads of a step's first chunk are issued before the previous
  //      accept poll (p0 does not depend on the accept) and tested at the step start.
  const int nXPi = nfeat * KC + KC;
  gran_t xpv[2];
  int xpo[2];
  const auto xp_issue = [&](int s_, int c) {
    const int tid = opaque((int)threadIdx.x);
    const int perQ = p2_pad(Fo * KC + KC, pad);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      int j = c * 2 * QTH + u * QTH + tid;
      if (j >= nXPi) j = nXPi - 1;                    // nothing wanted: an alias that matches with the rest
      int p = 0, i = Fo * KC + j - nfeat * KC;
      if (j < nfeat * KC) {
        const int d = j / KC;
        p = d / Fo;
        i = (d - p * Fo) * KC + (j - d * KC);
      }
      xpo[u] = (a.oXP + (((s_ & 1) * Gf + f) * Gr + p) * perQ + i) * 16;
      xpv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, xpo[u], 0, 16 /* sc1 */);
    }
  };
  // tests the chunk (re-reading it until it is complete) and stores it: pWs, and pbsh / pb0sh for the bias
  const auto xp_finish = [&](int c, unsigned e) -> bool {
    const int tid = opaque((int)threadIdx.x);
    unsigned long long t0 = 0;
    for (int spins = 0;; ++spins) {
      if (pass_complete(gran_miss(xpv[0], e) | gran_miss(xpv[1], e))) break;
      if (p2_pass_missed(spins, t0, a.abort_flag, a.oXP, e)) return false;
#pragma unroll
      for (int u = 0; u < 2; ++u) xpv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, xpo[u], 0, 16 /* sc1 */);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = c * 2 * QTH + u * QTH + tid;
      if (j >= nXPi) continue;
      const T v = (T)decode(xpv[u]);
      if (j < nfeat * KC) {
        pWs[(j / KC) * 16 + (j - (j / KC) * KC)] = v;
      } else {
        pbsh[j - nfeat * KC] = v;
        pb0sh[j - nfeat * KC] = v;
      }
    }
    return true;
  };

  // ---- helper workgroups (help): E_current of every step, off the chain's workgroups.  ll0 = ll(q_s;
  //      batch s) is first used in the accept at the END of step s, so the helper of (r, f) computes it
  //      while the chain runs the step's leapfrogs: the same A-gemm, A-RS exchange (region XAh), log-softmax
  //      and row order as the chain's own it = -1 round, from the state the chain's feature team published
  //      after the previous accept (XQ), into slot 2 of its twin's accept record.  Helpers store nothing to
  //      W or b and take no part in the commit round; they leave after the last step's publish, or from a
  //      poll that timed out or saw the abort word (the chain then sees the word in its accept poll).
  if (helper) {
    const int perQ = p2_pad(Fo * KC + KC, pad);
    unsigned eacc = a.ep0;                            // E(s - 1): the chain's accept epoch of the previous step
    // p0(sn) of the team's slice, 1/Gr per member (its owned features; member 0 the bias too), drawn as
    // the chain draws its owned elements
    const auto pubP = [&](int sn, unsigned e) {
      const int tid = opaque((int)threadIdx.x);
      const int reg = a.oXP + ((((sn & 1) * Gf + f) * Gr + r) * perQ);
      if (tid < Fo * KC) {
        put_t(fl2, rs, reg + tid, own ? (double)noise1<T>(a, sn, 0u, (uint32_t)e_own) : 0.0, e);
      } else if (r == 0 && tid < Fo * KC + KC) {
        const int k = tid - Fo * KC;
        put_t(fl2, rs, reg + tid, k < K ? (double)noise1<T>(a, sn, 0u, (uint32_t)(D * K + k)) : 0.0, e);
      }
    };
    pubP(0, eacc);
    for (int s = 0; s < a.n_steps; ++s) {
      const int tid = opaque((int)threadIdx.x), lane = tid & 63;
      const int n = sched_at(inl, s, a.inl[sched_k(s)].n_iter, a.n_iter);
      if (s == 0) {
        const int64_t rw = sched_at(inl, s, a.inl[sched_k(s)].row0, a.row0);
        load_step_rows<T>(Xs, Yo, reinterpret_cast<const T*>(a.X) + (size_t)rw * D,
                          reinterpret_cast<const T*>(a.Y) + (size_t)rw * K, Br, BfP, BFP, nrow, nfeat, row0, feat0, D, K,
                          Ro, nro, ro0);
        if (tid < 16) b0sh[tid] = bsh[tid];           // q_0 came from W and b, as in the chain
        __syncthreads();
      } else {
        // q_s: the owned slices of the feature team's Gr chain members (+ the bias, from member 0)
        const int ni = Fo * KC + KC;
        const int base0 = a.oXQ + ((s & 1) * Gf + f) * Gr * perQ;
        // a helper idles for most of a step: until the chain's step ends, ONE thread polls ONE granule
        // (member 0's first, always published) with long naps, so that 2·G·QTH spinning threads do not load
        // the fabric under the chain's rounds; after a timeout or the abort word the gather below leaves
        if (tid == 0) {
          unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
          for (int spins = 0;; ++spins) {
            const gran_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, base0 * 16, 0, 16 /* sc1 */);
            if (pass_complete(gran_miss(v, eacc))) break;
            if ((spins & 63) == 63 && p2_spin_over(t0, a.abort_flag, base0, eacc)) break;
            __builtin_amdgcn_s_sleep(32);
          }
        }
        __syncthreads();
        const bool ok = gather_ws(rs, base0, perQ, Gr, ni, [](int i) { return i; },
                                  [&](int p, int i) { return i < Fo * KC ? p * Fo + i / KC < nfeat : p == 0; }, eacc,
                                  a.abort_flag, [&](int q, double v) {
          const int p = q / ni, i = q - p * ni;
          if (i < Fo * KC) Wf[(p * Fo + i / KC) * 16 + i % KC] = (T)v;
          else b0sh[i - Fo * KC] = (T)v;
        });
        if (!all_ok(ok, ish)) return;
      }
      // the chain's epochs of step s: 3 rounds per leapfrog with the B all-reduce, 4 (none after the last
      // B-RS) without, then the accept round; the chain runs no it = -1 round when helpers do
      eacc += (n > 0 ? (bar ? 3u * (unsigned)n : 4u * (unsigned)n - 1u) : 0u) + 1u;
      ep = eacc - 1;
      const int par = s & 1;
      roundA(par);                                    // epoch E(s)
      if (!consumeA(par)) return;
      {
        const int k = lane & 15, grp = tid >> 4;
        const bool kv = k < K;
        for (int ii = grp; ii < nro; ii += QTH / 16) {
          const T z = kv ? clipz(Zo[ii * 16 + k] + b0sh[k], hi, lo) : (T)-__builtin_inf();
          const T m = g16_max2(z);
          const T e = kv ? exp(z - m) : T(0);
          const T sm = g16_sum2(e);
          const T lse = log(sm) + m;                                          // softmax.py:18
          const double t = kv ? (double)(Yo[ii * 16 + k] * (z - lse)) : 0.0;  // softmax.py:19-20
          const double rsum = g16_sum2(t);
          if (k == 0) rowll[ii] = rsum;
        }
        __syncthreads();
        if (tid == 0) {
          double v = 0.0;
          for (int ii = 0; ii < nro; ++ii) v += rowll[ii];
          put(rs, a.oXS + ((s & 1) * G + bid) * NXS + 2, v, eacc);
        }
      }
      if (s + 1 < a.n_steps) pubP(s + 1, eacc);
      // the next step's tile and labels: Xs and Yo have no reader left behind the barrier above, and the
      // next reader comes after the barrier that ends the XQ gather
      if (s + 1 < a.n_steps) {
        const int64_t rn = sched_at(inl, s + 1, a.inl[sched_k(s + 1)].row0, a.row0);
        load_step_rows<T>(Xs, Yo, reinterpret_cast<const T*>(a.X) + (size_t)rn * D,
                          reinterpret_cast<const T*>(a.Y) + (size_t)rn * K, Br, BfP, BFP, nrow, nfeat, row0, feat0, D, K,
                          Ro, nro, ro0);
      }
    }
    verdict.done = true;                              // nothing to report: the chain workgroups decide
    return;
  }

  // ---- look-ahead (ah): lane l runs the steps l, l + 2, …, each at first SPECULATIVELY from its own last
  //      state, i.e. assuming that the twin lane's step before it leaves the state unchanged (MCMC
  //      pre-fetching with one level).  After its accept round the lane reads the twin's verdict V(s − 1):
  //      "unchanged" makes the run final — decision applied, outputs written, V(s) (and the new state)
  //      published; "changed" voids it — the lane gathers the true q_s from the twin's XQ publish and runs
  //      the step again (`redo`: not speculative, same tile, the momentum drawn again from the same
  //      counters).  Every final run performs today's help = 0 arithmetic in today's order.
  const int s_first = lanei, s_inc = ah ? 2 : 1;
  bool redo = false;                                  // this run starts from the true state
  bool pf_done = false;                               // the lane's next tile already sits in the other buffer
  int tb = 0;                                         // tile buffer of the current step
  const int perV = p2_pad(Fo * KC + KC, pad);         // XQ block of a feature-team member: slice + bias
  // q after step k: the owned slices of the twin lane's feature-team members (the bias from member 0) → Wf, bsh
  const auto gatherQ = [&](int k) -> bool {
    const int ni = Fo * KC + KC;
    const int base0 = a.oXQ + ((k & 1) * Gf + f) * Gr * perV;
    const bool ok = gather_ws(rs, base0, perV, Gr, ni, [](int i) { return i; },
                              [&](int p, int i) { return i < Fo * KC ? p * Fo + i / KC < nfeat : p == 0; },
                              a.ep0 + (unsigned)k, a.abort_flag, [&](int q, double v) {
      const int p = q / ni, i = q - p * ni;
      if (i < Fo * KC) Wf[(p * Fo + i / KC) * 16 + i % KC] = (T)v;
      else bsh[i - Fo * KC] = (T)v;
    });
    return all_ok(ok, ish);
  };
  // V(k) of the twin workgroup: one thread polls one granule with naps (a lane that waits stays off the
  // fabric); 0 / 1 = the state was kept / changed, −1 = timed out or the abort word is up
  // `known` (thread 0's): the verdict when the run's own poll has already read it (0 / 1), else −1
  const auto waitV = [&](int k, int known) -> int {
    if (threadIdx.x == 0) {
      const int g = (a.oXV + ((k & 1) * G + pbid) * 8) * 16;
      const unsigned tg = a.ep0 + (unsigned)k;
      unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      int res = known;
      for (int spins = 0; known < 0; ++spins) {
        const gran_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, g, 0, 16 /* sc1 */);
        if (pass_complete(gran_miss(v, tg))) { res = decode(v) != 0.0 ? 1 : 0; break; }
        if ((spins & 63) == 63 && p2_spin_over(t0, a.abort_flag, a.oXV, tg)) break;
        __builtin_amdgcn_s_sleep(4);
      }
      ish[2] = res;
    }
    __syncthreads();
    const int res = ish[2];
    __syncthreads();
    return res;
  };

  // ---- stopping a voided run in flight (look-ahead, a speculative run with leapfrogs).  Thread 0 looks for the
  //      twin's V(s − 1) once per leapfrog iteration: one load issued at the top of the iteration and tested
  //      behind the A publish, while the partials travel.  "Unchanged" ends the looking, and the wait after
  //      the accept round; "changed" raises the workgroup's flag ish[3].  Every poller of the kernel takes a
  //      missing partner for a timeout, so the lane has to leave the run as one: the flag rides in the A-AG
  //      header's ll item, which carries nothing before the last iteration (row team: every f of one r),
  //      and the sum of those in the B round's header (feature team: every r of one f).  Both sums run in
  //      producer order, so after the B round of iteration i every workgroup of the lane holds the same
  //      count of flags raised before their A-AG publish of iteration i, and all of them leave there when it
  //      is not zero.  The item reaches no output: hdr[KC] is read as ll only in the last iteration, whose
  //      item is the ll.  A flag raised in the last iteration travels nowhere; that run ends in the accept
  //      round, the verdict (known by then) and the redo, as before.
  int c_redo = 0, c_stop = 0, c_skip = 0;              // thread 0 of a lane's workgroup 0: the call's counters
  const bool cnt0 = ah && bid == 0 && threadIdx.x == 0;
  // ---- parked steps (runon).  A speculative run of step p that ends with V(p − 1) unknown to the whole lane
  //      (item 3 of the accept records: what each workgroup's poll has read) and with the own decision "state
  //      unchanged" is parked: q restored, the outputs written, nothing published, and the lane starts step
  //      p + 2 on the prefetched tile (pk).  The poll of that run then looks for V(p − 1) first: "unchanged"
  //      makes p final (thread 0 publishes V(p), and goes on to look for V(p + 1)); "changed" raises the stop
  //      flag with the reason "p is void", the lane leaves at the agreed boundary, gathers q_p, goes back to
  //      tile p and redoes p, then runs p + 2 again.  A run of p + 2 that ends with p still parked waits for
  //      V(p − 1) before its accept round (one pending step per lane, and tile p's buffer is the prefetch's).
  const bool runon = ah && a.runon != 0;
  bool pk = false;                                    // step s − 2 is parked (the same in every workgroup of the lane)
  int pres = -1;                                      // thread 0: V(s − 3) of a parked step as read, −1 not yet
  int c_ron = 0, c_void = 0;
  // V(k) = unchanged, unread by anyone but the twin (thread 0)
  const auto pubV0 = [&](int k) { put(rs, a.oXV + ((k & 1) * G + pbid) * 8, 0.0, a.ep0 + (unsigned)k); };
  // the parked step s − 2 is void: q_{s−2}, its tile (the tile of s stays loaded in the other buffer), and again
  const auto unpark = [&](int s_) -> bool {
    if (!gatherQ(s_ - 3)) return false;
    wv = own ? Wf[wl] : T(0);
    tb ^= 1;
    Xc = tb ? Xs2 : Xs;
    Yc = tb ? Yo2 : Yo;
    pf_done = true;
    pk = false;
    redo = true;
    return true;
  };
  for (int s = s_first; s < a.n_steps;) {
    const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6, lr = lane & 15;   // not hoisted (registers)
    const double epsd = sched_at(inl, s, a.inl[sched_k(s)].eps, a.eps);
    const T eps = (T)epsd, ome = (T)(1.0 - epsd), nsc = (T)(2.0 * epsd);
    const int n = sched_at(inl, s, a.inl[sched_k(s)].n_iter, a.n_iter);
    const int64_t rw = sched_at(inl, s, a.inl[sched_k(s)].row0, a.row0);
    const T* Xg = reinterpret_cast<const T*>(a.X) + (size_t)rw * D;
    const T* Yg = reinterpret_cast<const T*>(a.Y) + (size_t)rw * K;
    const bool specrun = ah && s > 0 && !redo && n > 0;
    int vst = -1;                                       // thread 0: V(s − 1) as this run's poll read it, −1 not yet
    int stopj = 0;                                      // > 0: the lane left this run after that many iterations
    int stopk = 0;                                      // ... 1: V(s − 1) changed, 2: the parked step is void
    if (specrun && tid == 0) { ish[1] = 0; ish[3] = 0; }   // barriers lie between this and every reader
    prof.stamp(0);
    if (s == a.force_abort && bid == G - 1) {                             // test knob: a "timed-out" member
      if (tid == 0) __hip_atomic_store(a.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }

    // ---- step start: tile, labels of my rows (step 0 only: later steps' were loaded while the
    //      previous accept round travelled), momentum (hmc.py:82-87), step-start copies
    if ((s == s_first || !prefetch) && !redo) load_step_rows<T>(Xc, Yc, Xg, Yg, Br, BfP, BFP, nrow, nfeat, row0, feat0, D, K, Ro, nro, ro0);
    for (int e = tid; e < BfP * 16; e += QTH) Wf0[e] = Wf[e];
    if (hp) {
      // momentum (hmc.py:82-87) from the helpers: the whole slice's p0 into pWs, the bias's into pbsh / pb0sh; then the owned
      // element from pWs and iteration 0's drift of the slice (sghmc.py:32) — behind the barrier that
      // ends the chunk, so the step-start copy above has read Wf
      if (tid >= QTH - 16) b0sh[tid - (QTH - 16)] = bsh[tid - (QTH - 16)];
      if (s == 0) xp_issue(0, 0);
      for (int c = 0; c * 2 * QTH < nXPi; ++c) {
        if (c > 0) xp_issue(s, c);
        if (!all_ok(xp_finish(c, ep), ish)) return;
      }
      pw = own ? pWs[wl] : T(0);
      if (n > 0)
        for (int j = tid; j < nfeat * KC; j += QTH) {
          const int l = (j / KC) * 16 + (j - (j / KC) * KC);
          Wf[l] = Wf[l] + eps * pWs[l];
        }
    } else {
      // momentum (hmc.py:82-87): the owned elements' by their threads, the bias's by the last 16 threads
      // (not the owners of elements 0..15: one Box–Muller latency per thread, not two)
      pw = own ? noise1<T>(a, s, 0u, (uint32_t)e_own) : T(0);
      if (tid >= QTH - 16) {
        const int k = tid - (QTH - 16);
        pbsh[k] = k < K ? noise1<T>(a, s, 0u, (uint32_t)(D * K + k)) : T(0);
        pb0sh[k] = pbsh[k];
        b0sh[k] = bsh[k];
      }
    }
    const T pw0 = pw;
    w0 = wv;
    const double kin0 = wsum((double)pw * (double)pw, dsh);
    double kb0 = 0.0;
    for (int k = 0; k < K; ++k) kb0 += (double)pbsh[k] * (double)pbsh[k];

    // ---- it = -1: log-likelihood of my rows at the step-start state (E_current).  (Round 5 measured
    //      issuing iteration 0's A round before consuming this one, both rounds in flight: 1.724 vs
    //      1.701 ms per driver-shape launch, 3 A/B pairs — slower, not kept.)
    //      With helpers (hp) the round is theirs, and the drift was done above.
    double ll0 = 0.0, ll_last = 0.0;
    if (!hp) prof.stamp(11);
    const int parm1 = (int)(uA & 1);
    if (!hp) roundA(parm1);
    if (n > 0 && !hp) {
      // iteration 0's drift of the whole F_f slice by p0 (every member computes it identically;
      // sghmc.py:32), by the waves that do not poll this A-RS round, while the partials travel —
      // after a barrier: every wave's A-gemm has read Wf
      __syncthreads();
      const int nzp = (spread & 1) ? 0 : ((nro * KC + 63) / 64) * 64;   // the polling threads
      const int ge0 = (feat0 * K) >> 2, ge1 = ((feat0 + nfeat) * K + 3) >> 2;
      for (int g = ge0 + tid - nzp; tid >= nzp && g < ge1; g += QTH - nzp) {
        T z4[4];
        philox4_if(a, s, 0u, (uint32_t)g, z4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = 4 * g + q;
          if (e < feat0 * K || e >= (feat0 + nfeat) * K) continue;
          const int i = e / K - feat0, k = e - (e / K) * K;
          const T p0 = noise_at<T>(a, s, 0u, (uint32_t)e, z4);
          Wf[i * 16 + k] = Wf[i * 16 + k] + eps * p0;
          if (bar) pWs[i * 16 + k] = p0;
        }
      }
    }
    if (!hp) {
      if (!consumeA(parm1)) return;
      const int k = lane & 15, grp = tid >> 4;
      const bool kv = k < K;
      for (int ii = grp; ii < nro; ii += QTH / 16) {
        const T z = kv ? clipz(Zo[ii * 16 + k] + b0sh[k], hi, lo) : (T)-__builtin_inf();
        const T m = g16_max2(z);
        const T e = kv ? exp(z - m) : T(0);
        const T sm = g16_sum2(e);
        const T lse = log(sm) + m;                                          // softmax.py:18
        const double t = kv ? (double)(Yc[ii * 16 + k] * (z - lse)) : 0.0;  // softmax.py:19-20
        const double rsum = g16_sum2(t);
        if (k == 0) rowll[ii] = rsum;
      }
      __syncthreads();
      if (tid == 0) {
        double v = 0.0;
        for (int ii = 0; ii < nro; ++ii) v += rowll[ii];
        dsh[4] = v;
      }
      __syncthreads();
      ll0 = dsh[4];
    }

    double kin1 = 0.0;
    T zb_prev = T(0);                                   // bias friction noise of the previous iteration
    for (int it = 0; it < n; ++it) {
      const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6, lr = lane & 15;   // not hoisted (registers)
      const bool last = it == n - 1;
      if (it == 0 && own) wv = wv + eps * pw;          // the slice drifted during the it = -1 round

      // ===== A-RS: partial logits → owners of the row slices
      prof.stamp(1);
      const int parA = (int)(uA & 1);
      const bool vlook = specrun && tid == 0 && vst < 0;
      gran_t vq = {0u, 0u, 0u, 0u};
      if (vlook) vq = __builtin_amdgcn_raw_buffer_load_b128(rs, (a.oXV + (((s - 1) & 1) * G + pbid) * 8) * 16, 0, 16 /* sc1 */);
      roundA(parA);
      tstamp(s, it, 0);
      // (a parked step's V(s − 3) comes first, in the same slot: V(s − 1) cannot be there before V(s − 2) is read)
      const bool vpk = runon && pk && pres < 0;
      if (vlook && pass_complete(gran_miss(vq, a.ep0 + (unsigned)(s - 1) - (vpk ? 2u : 0u)))) {
        const int ch = decode(vq) != 0.0 ? 1 : 0;
        if (vpk) {
          pres = ch;
          if (ch) ish[3] = 2;
          else pubV0(s - 2);
        } else {
          vst = ch;
          if (vst) ish[3] = 1;
        }
      }
      // B-AR: the previous iteration's bias sub-step runs here, after this workgroup's A partials went
      // out (it only has to be done before the softmax), then b' of this iteration
      if (bar && it > 0 && tid < K) {
        const T gr = -((T)hdr[tid] - alpha * bpsh[tid]);
        pbsh[tid] = (ome * pbsh[tid] + eps * gr) + nsc * zb_prev;
        bsh[tid] = bpsh[tid];
      }
      if (tid < 16) bpsh[tid] = bsh[tid] + eps * pbsh[tid];                // b' (bias sub-step)
      prof.stamp(2);
      // friction noise of this iteration (sghmc.py:31), generated while the partials travel
      T zb = T(0);
      if (zoff) {
        // by the waves that do not poll the A-RS round, into LDS; the owners pick it up below
        const int zi = tid - NZ0;
        if (zi >= 0 && zi < nfo * KC + K) {
          bool v = true;
          uint32_t e;
          if (zi < nfo * KC) {
            const int od_ = zi / KC, ok_ = zi - (zi / KC) * KC;
            v = ok_ < K;
            e = (uint32_t)((feat0 + fo0 + od_) * K + ok_);
          } else {
            e = (uint32_t)(D * K + zi - nfo * KC);
          }
          zbuf[zi] = v ? noise1<T>(a, s, (uint32_t)(it + 1), e) : T(0);
        }
      } else {
        zn = own ? noise1<T>(a, s, (uint32_t)(it + 1), (uint32_t)e_own) : T(0);
        if (tid < K) zb = noise1<T>(a, s, (uint32_t)(it + 1), (uint32_t)(D * K + tid));
      }
      prof.stamp(3);
      if (!consumeA(parA)) return;
      if (zoff) {                                       // consumeA ended in a barrier
        zn = own ? zbuf[tid] : T(0);
        zb = tid < K ? zbuf[nfo * KC + tid] : T(0);
      }
      tstamp(s, it, 1);
      prof.stamp(4);

      // ===== softmaxes of my rows: diff at b (weights sub-step), y − ŷ' at b' (bias sub-step)
      {
        const int k = lane & 15, grp = tid >> 4;
        const bool kv = k < K;
        for (int item = grp; item < 2 * nro; item += QTH / 16) {
          const bool v1 = item >= nro;
          const int ii = v1 ? item - nro : item;
          const T bias = kv ? (v1 ? bpsh[k] : bsh[k]) : T(0);
          const T y = Yc[ii * 16 + k];
          const T z = kv ? clipz(Zo[ii * 16 + k] + bias, hi, lo) : (T)-__builtin_inf();   // softmax.py:39-41
          const T m = g16_max2(z);
          const T e = kv ? exp(z - m) : T(0);                                                // softmax.py:34
          const T sm = g16_sum2(e);
          const T dd = kv ? y - e / sm : T(0);                                                // softmax.py:52
          if (!v1) {
            Dme[ii * 16 + k] = dd;
          } else {
            Csr[ii * 16 + k] = dd;
            if (last) {
              const T lse = log(sm) + m;
              const double t = kv ? (double)(y * (z - lse)) : 0.0;
              const double rsum = g16_sum2(t);
              if (k == 0) rowll[ii] = rsum;
            }
          }
        }
        __syncthreads();
      }
      // ===== A-AG: [colsum part (KC), ll part, diff rows (Ro·KC)] → every row-team member
      prof.stamp(5);
      double hv = 0.0;                                  // t < KC: team colsum; t == KC: team ll
      {
        ++ep;
        const int reg = oXD + (((int)(uD & 1) * Gr + r) * Gf + f) * NXA;
        for (int t = tid; t < NXA0; t += QTH) {
          double v;
          if (t < KC) {
            T c = T(0);
            for (int ii = 0; ii < nro; ++ii) c += Csr[ii * 16 + t];
            v = (double)c;
          } else if (t == KC) {
            // not the last iteration: the stop flag, 1 for "V(s − 1) changed", 4096 for "the parked step is void"
            // (one reason per run, at most G ≤ 256 flags: the sum tells which)
            v = (specrun && ish[3]) ? ((runon && ish[3] == 2) ? 4096.0 : 1.0) : 0.0;
            if (last) { v = 0.0; for (int ii = 0; ii < nro; ++ii) v += rowll[ii]; }
          } else {
            const int m = t - HA;
            v = (double)Dme[(m / KC) * 16 + (m % KC)];
          }
          put_t(al2, rs, reg + t, v, ep);
        }
        tstamp(s, it, 2);
        const int base0 = oXD + ((int)(uD & 1) * Gr + r) * Gf * NXA;
        ++uD;
        bool ok;
        if (spread & 2) {
          // diff rows straight into Ds, headers into stg (no staging copy, no second barrier)
          ok = gather_st(rs, base0, NXA, Gf, NXA0, [](int i) { return i; }, ep, a.abort_flag, [&](int q, double v) {
            const int p = q / NXA0, t = q - p * NXA0;
            if (t < HA) stg[q] = v;
            else Ds[(p * Ro + (t - HA) / KC) * 16 + (t - HA) % KC] = (T)v;
          });
          if (!all_ok(ok, ish)) return;
          if (tid < HA) {                           // producer order; the loads issued together
            double hvs[QNPM];
#pragma unroll
            for (int p = 0; p < QNPM; ++p) hvs[p] = stg[min(p, Gf - 1) * NXA0 + tid];
            hv = hvs[0];
#pragma unroll
            for (int p = 1; p < QNPM; ++p)
              if (p < Gf) hv += hvs[p];
          }
        } else if (tid < HA) {
          ok = poll<true>(rs, base0, NXA, Gf, -1, tid, true, ep, nullptr, 0, &hv, a.abort_flag);
        } else {
          const int m = tid - HA;
          ok = poll<false>(rs, base0, NXA, Gf, -1, tid, tid < NXA0, ep, nullptr, 0, nullptr, a.abort_flag,
                           Ds + (m / KC) * 16 + (m % KC), Ro * 16);
        }
        if (!(spread & 2) && !all_ok(ok, ish)) return;
        tstamp(s, it, 3);
      }

      // ===== B-RS: partial gradient X[R_r,F_f]ᵀ·diff → owners of the feature slices
      prof.stamp(6);
      {
        ++ep;
        const int reg = oXB + (((int)(uB & 1) * Gf + f) * Gr + r) * NXB;
        if (tid < HA) put_t(fl2, rs, reg + tid, hv, ep);
        // bar: the owner of an element folds its friction noise into its partial — Σ partials − 2z, so
        // ε·(−(Σ − 2z − αw)) = ε·g + 2ε·z (sghmc.py:31,34) arrives with the all-reduce and no other
        // member has to draw that noise
        const auto bpart = [&](int d, int k, double v) -> double {
          return (bar && d >= fo0 && d < fo0 + nfo && k < K) ? v - 2.0 * (double)zbuf[(d - fo0) * KC + k] : v;
        };
        const int nkp = (Br / 4) / WPB;
        for (int item = wave; item < MTB * WPB; item += QNW) {
          const int mt = item % MTB, part = item / MTB;
          const typename M::acc_t c = mfma_tile<T>(Xc + part * nkp * 4 * BFP + mt * 16, 1, nkp * BFP, BFP,
                                                   Ds + part * nkp * 4 * 16, nkp * 16, 16, nkp);
          if (WPB == 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int d = mt * 16 + M::row(lane, q);
              if (d < nfeat && lr < KC) put_t(fl2, rs, reg + HA + d * KC + lr, bpart(d, lr, (double)c[q]), ep);
            }
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) Zp[(part * BfP + mt * 16 + M::row(lane, q)) * 16 + lr] = c[q];
          }
        }
        if (WPB > 1) {
          __syncthreads();
          for (int e = tid; e < nfeat * KC; e += QTH) {
            const int i = e / KC, k = e - (e / KC) * KC;
            T v = Zp[i * 16 + k];
            for (int q = 1; q < WPB; ++q) v += Zp[(q * BfP + i) * 16 + k];
            put_t(fl2, rs, reg + HA + e, bpart(i, k, (double)v), ep);
          }
        }
        const int base0 = oXB + ((int)(uB & 1) * Gf + f) * Gr * NXB;
        ++uB;
        tstamp(s, it, 4);
        prof.stamp(7);
        if (bar) {
          // all-reduce by redundant reads: items [0, HA) header, [HA, HA + nfeat·KC) the slice's gradient
          // (noise folded in by the owners); every member sums the Gr partials of every item in producer
          // order and applies the same update to the whole slice (momentum pWs, position Wf), so no B-AG
          // round is needed
          const int ni = HA + nfeat * KC;
          bool ok = true;
          double kl = 0.0;
          for (int i0 = tid; i0 < ni; i0 += 2 * QTH) {
            int off[2] = {i0, i0 + QTH};
            const unsigned vm = 1u | (off[1] < ni ? 2u : 0u);
            double sm[2];
            ok = polln<2>(rs, base0, NXB, Gr, off, vm, ep, sm, a.abort_flag, []() {});
            if (!ok) break;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int i = off[j];
              if (i >= ni) continue;
              if (i < HA) {
                hdr[i] = sm[j];
                if (specrun && !last && i == KC && sm[j] != 0.0) ish[1] = (runon && sm[j] >= 4096.0) ? 2 : 1;   // flags raised in the lane
                continue;
              }
              const int m = i - HA, d = m / KC, k = m - (m / KC) * KC;
              if (k >= K) continue;
              const int l = d * 16 + k;
              const T w = Wf[l];
              const T gz = -((T)sm[j] - alpha * w);                   // softmax.py:57-58 gradient + 2z
              const T p = ome * pWs[l] + eps * gz;                     // sghmc.py:31,34
              pWs[l] = p;
              if (!last) Wf[l] = w + eps * p;                          // sghmc.py:32
              else if (d >= fo0 && d < fo0 + nfo) kl += (double)p * (double)p;
            }
          }
          const int q = specrun ? all_okq(ok, ish) : all_ok(ok, ish) ? 0 : -1;
          if (q < 0) return;
          tstamp(s, it, 5);
          prof.stamp(8);
          if (q > 0 && !last) { stopj = it + 1; stopk = q; break; }
          if (last) {
            if (tid < K) {                                                    // bias sub-step, replicated
              const T gr = -((T)hdr[tid] - alpha * bpsh[tid]);
              pbsh[tid] = (ome * pbsh[tid] + eps * gr) + nsc * zb;
              bsh[tid] = bpsh[tid];
            }
            ll_last = hdr[KC];                                                // ll(q_new) on this batch
            kin1 = kl;
            break;
          }
          zb_prev = zb;                               // its bias sub-step: after the next A publish
          continue;
        }
        // threads [0, nfo·KC): owned gradient element; threads [nfo·KC, nfo·KC + HA): header
        const int ng = nfo * KC;
        double sum = 0.0;
        const bool isg = tid < ng, ish_ = tid >= ng && tid < ng + HA;
        const int offB = isg ? HA + fo0 * KC + tid : tid - ng;
        if (spread & 4) {
          const int ni = ng + HA;
          const bool ok = gather(rs, base0, NXB, Gr, ni, [&](int i) { return i < ng ? HA + fo0 * KC + i : i - ng; },
                                 all_items, ep, a.abort_flag, stg);
          if (!all_ok(ok, ish)) return;
          if (tid < ni) {
            sum = stg[tid];
            for (int p = 1; p < Gr; ++p) sum += stg[p * ni + tid];
          }
          if (ish_) hdr[tid - ng] = sum;
          __syncthreads();
        } else {
          const bool ok = fl2 ? poll<true, double, 16>(rs, base0, NXB, Gr, -1, offB, isg || ish_, ep, nullptr, 0, &sum,
                                                        a.abort_flag)
                                : poll<true>(rs, base0, NXB, Gr, -1, offB, isg || ish_, ep, nullptr, 0, &sum, a.abort_flag);
          if (ish_) hdr[tid - ng] = sum;
          if (!all_ok(ok, ish)) return;
        }
        tstamp(s, it, 5);
        prof.stamp(8);
        // (both branches ended in a barrier behind the header's store)
        if (specrun && !last && hdr[KC] != 0.0) { stopj = it + 1; stopk = (runon && hdr[KC] >= 4096.0) ? 2 : 1; break; }
        // owned weight: gradient (softmax.py:57-58), momentum (sghmc.py:31,34), drift (:32)
        if (own) {
          const T gr = -((T)sum - alpha * wv);
          const T p = (ome * pw + eps * gr) + nsc * zn;
          pw = p;
          if (!last) wv = wv + eps * p;
          else kin1 = (double)p * (double)p;
        }
        if (tid < K) {                                                      // bias sub-step, replicated
          const T gr = -((T)hdr[tid] - alpha * bpsh[tid]);
          pbsh[tid] = (ome * pbsh[tid] + eps * gr) + nsc * zb;
          bsh[tid] = bpsh[tid];
        }
        if (last) ll_last = hdr[KC];                                        // ll(q_new) on this batch
      }
      if (last) break;
      // ===== B-AG: drifted owned weights → every member of the feature team
      prof.stamp(9);
      {
        ++ep;
        const int per = p2_pad(Fo * KC, pad);
        const int reg = oXW + (((int)(uW & 1) * Gf + f) * Gr + r) * per;
        if (tid < nfo * KC) put_t(fl2, rs, reg + tid, own ? (double)wv : 0.0, ep);
        tstamp(s, it, 6);
        if (own) Wf[wl] = wv;
        const int base0 = oXW + ((int)(uW & 1) * Gf + f) * Gr * per;
        ++uW;
        if (spread & 8) {
          const int ni = Fo * KC;
          const auto want = [&](int p, int i) { return p != r && p < min(Gr, (nfeat - i / KC + Fo - 1) / Fo); };
          const bool ok = gather(rs, base0, per, Gr, ni, [](int i) { return i; }, want, ep, a.abort_flag, stg);
          if (!all_ok(ok, ish)) return;
          for (int q = tid; q < Gr * ni; q += QTH) {
            const int p = q / ni, i = q - p * ni;
            if (want(p, i)) Wf[(p * Fo + i / KC) * 16 + i % KC] = (T)stg[q];
          }
          __syncthreads();
          tstamp(s, it, 7);
          continue;
        }
        const int dloc = tid / KC, kk = tid - (tid / KC) * KC;
        const int npd = tid < Fo * KC ? min(Gr, (nfeat - dloc + Fo - 1) / Fo) : 0;   // producers owning feature dloc
        const bool ok = fl2 ? poll<false, T, 16>(rs, base0, per, npd, r, tid, tid < Fo * KC, ep, nullptr, 0, nullptr,
                                                  a.abort_flag, Wf + dloc * 16 + kk, Fo * 16)
                              : poll<false>(rs, base0, per, npd, r, tid, tid < Fo * KC, ep, nullptr, 0, nullptr,
                                            a.abort_flag, Wf + dloc * 16 + kk, Fo * 16);
        if (!all_ok(ok, ish)) return;
        tstamp(s, it, 7);
      }
    }

    if (specrun && stopj) {                              // (specrun: the block folds away where look-ahead does)
      // the lane left the run at a boundary: the epoch the full run would have ended on (the remaining
      // iterations' rounds — without the B all-reduce iteration stopj − 1 had its B-AG still to come — and
      // the accept round), then the voided run's path: the true q_s, and step s again on the tile it holds
      // (the redo's accept round loads the next tile: pf_done is still false)
      prof.stamp(14);
      ep += (bar ? 3u : 4u) * (unsigned)(n - stopj) + 1u;
      if (cnt0) { ++c_redo; ++c_stop; c_skip += n - stopj; }
      if (runon && pk && stopk == 2) {                  // the parked step and this run are void
        if (cnt0) ++c_void;
        if (!unpark(s)) return;
        s -= 2;
        continue;
      }
      if (runon && pk) {                                // V(s − 1) exists: the parked step is final (Q2Args, XV)
        if (tid == 0 && pres < 0) pubV0(s - 2);
        pk = false;
      }
      if (!gatherQ(s - 1)) return;
      wv = own ? Wf[wl] : T(0);
      redo = true;
      continue;
    }
    if (runon && pk) {
      // one pending step per lane: the parked step is resolved before this run's accept round, whose prefetch
      // loads into the parked step's tile buffer.  (Also the end of a run whose flag was raised in its last
      // iteration and travelled nowhere.)
      prof.stamp(12);
      const int vp = waitV(s - 3, pres);
      if (vp < 0) return;
      if (vp) {
        prof.stamp(13);
        ++ep;                                           // this run's accept round, not held
        if (cnt0) { ++c_redo; ++c_void; }
        if (!unpark(s)) return;
        s -= 2;
        continue;
      }
      if (tid == 0 && pres < 0) pubV0(s - 2);
      pk = false;
    }
    if (bar && n > 0 && own) wv = Wf[wl];            // the slice lives in LDS (last write: barrier-ed)
    // ===== accept (hmc.py:67-71): all-gather of the kinetic / log-likelihood partials
    prof.stamp(10);
    const double kin1w = wsum(kin1, dsh);
    double kb1 = 0.0;
    for (int k = 0; k < K; ++k) kb1 += (double)pbsh[k] * (double)pbsh[k];
    ++ep;
    {
      const int reg = oXS + ((int)(uS & 1) * G + bid) * NXS;
      if (tid == 0) put(rs, reg + 0, kin0, ep);
      if (tid == 1) put(rs, reg + 1, kin1w, ep);
      if (tid == 2 && !hp) put(rs, reg + 2, ll0, ep);   // hp: this workgroup's helper wrote it
      // runon, item 3: what this workgroup's poll has read of V(s − 1) — 0 nothing, 1 unchanged, 1024 changed
      if (runon && tid == 0) put(rs, reg + 3, (s > 0 && !redo && vst >= 0) ? (vst ? 1024.0 : 1.0) : 0.0, ep);
    }
    if (hp && s + 1 < a.n_steps) xp_issue(s + 1, 0);   // p0 of the next step: tested at its start
    // next step's tile and labels while the partials travel: Xs and Yo have no reader left in this
    // step (the last B-gemm and softmax ended before a barrier)
    // (measured: loading it with only the half of the workgroup that does not poll the accept round
    // is slower — 9.68 vs 9.44 µs per leapfrog: two load batches instead of one)
    // (look-ahead: the lane's next step is s + 2, and its tile goes into the OTHER buffer — this step may
    // have to be run again from the tile it holds; a redone step finds the next tile already loaded)
    if (prefetch && s + s_inc < a.n_steps && !pf_done) {
      const int sn = s + s_inc;
      const int64_t rn = sched_at(inl, sn, a.inl[sched_k(sn)].row0, a.row0);
      const T* Xn = reinterpret_cast<const T*>(a.X) + (size_t)rn * D;
      const T* Yn = reinterpret_cast<const T*>(a.Y) + (size_t)rn * K;
      load_step_rows<T>(ah ? (tb ? Xs : Xs2) : Xs, ah ? (tb ? Yo : Yo2) : Yo, Xn, Yn, Br, BfP, BFP, nrow, nfeat, row0, feat0,
                        D, K, Ro, nro, ro0);
      pf_done = ah;
    }
    const int sbase = oXS + (int)(uS & 1) * G * NXS;
    ++uS;
    double v3[3] = {0.0, 0.0, 0.0};
    double v4 = 0.0;                                    // runon: item 3 of workgroup tid's record
    if (acc1) {
      // the three partials of workgroup tid in one batch of loads (one round trip, not three); runon: four
      const int nv = runon ? 4 : 3;
      const bool ok = poll_nb<1, false, double>(rs, sbase + tid * NXS, 1, nv, -1, 0, tid < G, ep, nullptr,
                                                a.abort_flag, stg + nv * tid, 1);
      if (!all_ok(ok, ish)) return;
      if (tid < G) { v3[0] = stg[nv * tid]; v3[1] = stg[nv * tid + 1]; v3[2] = stg[nv * tid + 2]; }
      if (runon && tid < G) v4 = stg[nv * tid + 3];
    } else {
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        ok = ok && poll<true>(rs, sbase + j, NXS, 1, -1, tid * NXS, tid < G, ep, nullptr, 0, &v3[j], a.abort_flag);
      if (runon) ok = ok && poll<true>(rs, sbase + 3, NXS, 1, -1, tid * NXS, tid < G, ep, nullptr, 0, &v4, a.abort_flag);
      if (!all_ok(ok, ish)) return;
    }
    const double S0 = wsum(v3[0], dsh), S1 = wsum(v3[1], dsh), L0 = wsum(v3[2], dsh);
    const double K0 = (0.0 + 0.5 * S0) + 0.5 * kb0;
    const double Ecur = a.neg_inv_n * (L0 + a.log_prior) + K0;
    double A, Enew, llq;
    int acc;
    if (n <= 0) {
      A = 1.0; Enew = Ecur; llq = L0;
      acc = sched_at(inl, s, a.inl[sched_k(s)].u, a.u) < A;
    } else {
      const double K1 = (0.0 + 0.5 * S1) + 0.5 * kb1;
      Enew = a.neg_inv_n * (ll_last + a.log_prior) + K1;
      const double x = exp(Ecur - Enew);
      A = (x < 1.0) ? x : 1.0;                                             // Python min(1, x)
      acc = sched_at(inl, s, a.inl[sched_k(s)].u, a.u) < A;
      llq = acc ? ll_last : L0;
    }
    if (ah && s > 0 && !redo) {
      // the twin's verdict on step s − 1 (this run assumed "state unchanged")
      prof.stamp(12);
      if (runon) {
        // no workgroup of the lane has read V(s − 1) (the same sum in all of them), this run leaves the state as
        // it was, and a step with leapfrogs follows on a tile that is loaded: park the step
        const double seen = wsum(v4, dsh);
        const int s2 = s + 2 < a.n_steps ? s + 2 : s;
        const int n2 = sched_at(inl, s2, a.inl[sched_k(s2)].n_iter, a.n_iter);
        if (seen == 0.0 && (!acc || n <= 0) && s + 2 < a.n_steps && pf_done && n2 > 0) {
          for (int e = tid; e < BfP * 16; e += QTH) Wf[e] = Wf0[e];         // keep q (sghmc.py:36-38)
          wv = w0;
          if (tid < 16) bsh[tid] = b0sh[tid];
          if (bid == 0 && tid == 0) {                                       // written again if the step is redone
            a.out_A[s] = A;
            a.out_acc[s] = acc;
            a.out_ll[s] = llq;
            if (a.out_E) { a.out_E[2 * s] = Ecur; a.out_E[2 * s + 1] = Enew; }
          }
          if (cnt0) ++c_ron;
          __syncthreads();
          tb ^= 1;
          Xc = tb ? Xs2 : Xs;
          Yc = tb ? Yo2 : Yo;
          pf_done = false;
          pk = true;
          pres = -1;
          s += 2;
          continue;
        }
      }
      const int vprev = waitV(s - 1, vst);
      if (vprev < 0) return;
      if (vprev) {
        prof.stamp(13);
        if (cnt0) ++c_redo;
        if (!gatherQ(s - 1)) return;
        wv = own ? Wf[wl] : T(0);
        redo = true;
        continue;                                                          // step s again, from q_s
      }
    }
    if (!acc || n <= 0) {                                                  // keep q (sghmc.py:36-38)
      for (int e = tid; e < BfP * 16; e += QTH) Wf[e] = Wf0[e];
      wv = w0;
      if (tid < 16) bsh[tid] = b0sh[tid];
    }
    if (a.out_mom && s == a.n_steps - 1) {                                 // sghmc.py:36-39 returned p
      T* mo = reinterpret_cast<T*>(a.out_mom);
      const bool keep_new = acc && n > 0;
      if (own) mo[e_own] = keep_new ? (bar ? pWs[wl] : pw) : pw0;
      if (bid == 0 && tid < K) mo[D * K + tid] = keep_new ? pbsh[tid] : pb0sh[tid];
    }
    if (a.out_trace) {                                                     // sghmc_multicore.py:49-51 row
      T* tr = reinterpret_cast<T*>(a.out_trace) + (size_t)s * (D * K + K);
      if (own) tr[e_own] = wv;
      if (bid == 0 && tid < K) tr[D * K + tid] = bsh[tid];
    }
    if (bid == 0 && tid == 0) {
      a.out_A[s] = A;
      a.out_acc[s] = acc;
      a.out_ll[s] = llq;
      if (a.out_E) { a.out_E[2 * s] = Ecur; a.out_E[2 * s + 1] = Enew; }
    }
    __syncthreads();
    // q_{s+1} for the helpers of this feature team: the owned slice (the bias too from member 0), one
    // store per thread, with the accept's epoch
    if (hp && s + 1 < a.n_steps) {
      const int reg = a.oXQ + ((((s + 1) & 1) * Gf + f) * Gr + r) * p2_pad(Fo * KC + KC, pad);
      if (tid < Fo * KC) put_t(fl2, rs, reg + tid, own ? (double)wv : 0.0, ep);
      else if (r == 0 && tid < Fo * KC + KC) put_t(fl2, rs, reg + tid, (double)bsh[tid - Fo * KC], ep);
    }
    if (ah) {
      // step s is final: the new state for the twin lane when the step changed it (also lane 1's last step,
      // which lane 0 commits), then the verdict V(s), both tagged with the step
      const bool changed = acc && n > 0;
      const unsigned tg = a.ep0 + (unsigned)s;
      if (changed && (s + 1 < a.n_steps || lanei)) {
        const int reg = a.oXQ + (((s & 1) * Gf + f) * Gr + r) * perV;
        if (tid < Fo * KC) put_t(fl2, rs, reg + tid, own ? (double)wv : 0.0, tg);
        else if (r == 0 && tid < Fo * KC + KC) put_t(fl2, rs, reg + tid, (double)bsh[tid - Fo * KC], tg);
      }
      if (tid == 0) put(rs, a.oXV + ((s & 1) * G + pbid) * 8, changed ? 1.0 : 0.0, tg);
      if (pf_done) {                                                       // the prefetched tile is the next step's
        tb ^= 1;
        Xc = tb ? Xs2 : Xs;
        Yc = tb ? Yo2 : Yo;
        pf_done = false;
      }
      redo = false;
    }
    s += s_inc;
  }
  prof.stamp(0);
  prof.flush();
  if (cnt0 && a.stats) {
    int* st = a.stats + 4 * lanei;
    st[0] = c_redo; st[1] = c_stop; st[2] = c_skip; st[3] = c_ron;
    a.stats[8 + lanei] = c_void;
  }
  if (ah) {
    if (lanei) {                                      // lane 1 takes no part in the commit round
      verdict.done = true;
      return;
    }
    // the call's last step was lane 1's: its verdict, and the final state when it moved
    if (a.n_steps >= 2 && !(a.n_steps & 1)) {
      const int vlast = waitV(a.n_steps - 1, -1);
      if (vlast < 0) return;
      if (vlast) {
        if (!gatherQ(a.n_steps - 1)) return;
        wv = own ? Wf[wl] : T(0);
      }
    }
  }
  // ---- commit round: every workgroup publishes a 'done' granule; workgroup 0 gathers all G and
  //      proposes commit (or abort, when its gather times out or sees the abort word) on the launch's
  //      decision word; the others wait for the decision (bounded: on timeout they propose abort).
  //      The first compare-and-swap decides and everyone follows it, so either every workgroup
  //      writes its slice of W/b or none does — independent timeouts (each measured from its own
  //      publish) cannot split the launch, and a decided abort leaves W/b untouched for the re-run.
  //      A member that timed out anywhere earlier never publishes, so workgroup 0 cannot commit.
  ++ep;
  if (tid == 0) put(rs, a.oXC + bid, 1.0, ep);
  {
    unsigned long long* dword = reinterpret_cast<unsigned long long*>(a.arena + (size_t)(a.oXC + G) * 16);
    if (bid == 0) {
      const bool ok = gather_st(rs, a.oXC, 1, G, 1, [](int) { return 0; }, ep, a.abort_flag, [](int, double) {});
      const bool all = all_ok(ok, ish);
      if (tid == 0) ish[1] = p2_decide(dword, ep, all ? P2_COMMIT : P2_ABORT);
    } else if (tid == 0) {
      ish[1] = p2_wait_decision(dword, ep, a.abort_flag);
    }
    __syncthreads();
    if (ish[1] != P2_COMMIT) return;
  }
  // ---- committed state: owners write their weights, workgroup 0 the bias
  verdict.done = true;
  if (own) reinterpret_cast<T*>(a.W)[e_own] = wv;
  if (bid == 0 && tid < K) reinterpret_cast<T*>(a.b)[tid] = bsh[tid];
}

// ---------------------------------------------------------------- plan + launch
static int kc_of(int K) { return K == 10 ? 10 : 16; }

static size_t p2_lds(const PersistPlan2& p, int K, size_t ts) {
  const int WPA = std::max(1, QNW / (p.Br / 16)), WPB = std::max(1, QNW / (p.BfP / 16));
  const int ZPN = std::max(WPA * p.Br, WPB * p.BfP) * 16;
  size_t t = ts * ((size_t)p.Br * p.BFP + 2 * (size_t)p.BfP * 16 + (size_t)p.Gf * p.Ro * 16 + ZPN +
                   4 * (size_t)p.Ro * 16 + 64);
  t += ts * 16;                                                              // pb0sh
  t = (t + 15) & ~(size_t)15;
  t += 8 * ((size_t)p.Ro + 32) + 16 + 16 * 8 + 8 * (size_t)QSTAGE + ts * ((size_t)p.Fo * 16 + 16);
  t += ts * ((size_t)p.BfP * 16);                                            // pWs (bar)
  (void)K;
  return t;
}

PersistPlan2 plan_p2(int B, int D, int K, size_t ts, int num_cus, size_t lds_max) {
  PersistPlan2 best{};
  best.ok = false;
  if (K > 16 || K < 1 || B < 1 || D < 1) return best;
  const int KC = kc_of(K);
  int fGr = 0, fGf = 0;
  if (const char* env = getenv("HMCX_P2_GRID")) sscanf(env, "%dx%d", &fGr, &fGf);
  const int cand[] = {1, 2, 4, 8, 16};
  for (int Gr : cand)
    for (int Gf : cand) {
      if (fGr && (Gr != fGr || Gf != fGf)) continue;
      const int G = Gr * Gf;
      if (G > num_cus) continue;
      PersistPlan2 p{};
      p.Gr = Gr; p.Gf = Gf;
      const int rows = (B + Gr - 1) / Gr;
      p.Br = 16;
      while (p.Br < rows) p.Br <<= 1;                                         // power of two (GEMM split)
      if (p.Br > QTH) continue;
      p.Bf = (D + Gf - 1) / Gf;
      p.BfP = (p.Bf + 15) / 16 * 16;
      // odd row pitch: the A-gemm's column reads (16 rows per ds_read2_b64 group) hit 16 distinct bank
      // pairs; the B-gemm reads its k values Br/4 rows apart per lane group (mfma_tile), 2·BFP·16 ≡ 32
      // dwords mod 64, so the two half-waves of its ds_read_b64 land on disjoint banks
      p.BFP = p.BfP + 1;
      p.Ro = (p.Br + Gf - 1) / Gf;
      p.Fo = (p.Bf + Gr - 1) / Gr;
      if ((long)(Gr - 1) * rows >= B || (long)(Gf - 1) * p.Bf >= D) continue;  // no empty teams
      // thread ↔ element mappings of the rounds (one granule per producer per thread)
      if (KC + 1 + p.Ro * KC > QTH || p.Fo * KC + KC + 1 > QTH || G > QTH) continue;
      p.lds = p2_lds(p, K, ts);
      if (p.lds > lds_max) continue;
      // cost model (calibrated on MI355X at B=500, D=784, K=10: 8x16 15.6, 16x8 16.3, 8x8 16.7,
      // 16x16 16.8, 4x16 27 µs per leapfrog): f64 MFMAs per wave of the two GEMMs, plus a price per
      // member of the row teams (A rounds, softmax skew) and of the feature teams
      const int WPA = std::max(1, QNW / (p.Br / 16)), WPB = std::max(1, QNW / (p.BfP / 16));
      const double mfma = (double)(p.Br / 16) * (p.BfP / 4) / QNW + (double)(p.BfP / 16) * (p.Br / 4) / QNW;
      const double cost = 300.0 * mfma + 700.0 * Gr + 400.0 * Gf + 0.0 * (WPA + WPB);
      p.cost = cost;
      p.ok = true;
      if (!best.ok || cost < best.cost) best = p;
    }
  return best;
}

int p2_help_mode(const PersistPlan2& p, int K, int num_cus, size_t lds_max, int want, size_t* lds) {
  const int G = p.Gr * p.Gf, KC = kc_of(K);
  const size_t half = lds_max / 2 + 1024;        // two such workgroups do not fit one CU
  const size_t need = std::max(p.lds, half);
  // the helpers gather q_s with at most 4 granules per thread (gather_ws)
  const bool ok = want == 2 && 2L * G <= num_cus && need <= lds_max && p.Gr * (p.Fo * KC + KC) <= 4 * QTH;
  if (lds) *lds = ok ? need : p.lds;
  return ok ? 2 : 0;
}

// Look-ahead (HMCX_P2_AHEAD, hmcx_set_sghmc_ahead): 1 when a launch of plan p can carry a second chain
// lane — 2·G workgroups at one per CU, the second X tile and label block in LDS, and the state gather of
// at most 4 granules per thread — else 0 (the helper launch, or today's plain one); *lds as p2_help_mode.
int p2_ahead_mode(const PersistPlan2& p, int K, size_t ts, int num_cus, size_t lds_max, int want, size_t* lds) {
  const int G = p.Gr * p.Gf, KC = kc_of(K);
  const size_t half = lds_max / 2 + 1024;
  const size_t need = std::max(p.lds + ts * ((size_t)p.Br * p.BFP + (size_t)p.Ro * 16), half);
  const bool ok = want == 1 && 2L * G <= num_cus && need <= lds_max && p.Gr * (p.Fo * KC + KC) <= 4 * QTH;
  if (ok && lds) *lds = need;
  return ok ? 1 : 0;
}

P2Layout p2_layout(const PersistPlan2& p, int K, int pad, int help, int ahead) {
  const long G = (long)p.Gr * p.Gf;
  const int KC = kc_of(K);
  P2Layout l{};
  // XA, XD, XB, XW, XS (double-buffered), the commit round ('done' granules + the launch's decision word,
  // one spare granule), then the helpers' regions (empty without helpers)
  l.nXA = 2 * G * p.Br * KC;
  l.nXD = 2 * G * p2_pad(KC + 1 + p.Ro * KC, pad);
  l.nXB = 2 * G * p2_pad(KC + 1 + p.Bf * KC, pad);
  l.nXW = 2 * G * p2_pad(p.Fo * KC, pad);
  l.nXS = 2 * G * (pad ? 8 : 4);
  l.nXC = G + 2;
  l.nXAh = help ? l.nXA : 0;
  l.nXQ = help ? 2 * G * p2_pad(p.Fo * KC + KC, pad) : 0;
  l.oXA = 0;
  l.oXD = l.oXA + l.nXA;
  l.oXB = l.oXD + l.nXD;
  l.oXW = l.oXB + l.nXB;
  l.oXS = l.oXW + l.nXW;
  l.oXC = l.oXS + l.nXS;
  l.oXAh = l.oXC + l.nXC;
  l.oXQ = l.oXAh + l.nXAh;
  l.nXP = l.nXQ;
  l.oXP = l.oXQ + l.nXQ;
  l.oL1 = l.oXV = l.ngran = l.oXP + l.nXP;
  if (ahead) {
    // no helpers: XQ carries the accepted states between the lanes; then lane 1's copy of XA … XS (same
    // order and sizes, so one offset serves all five) and the verdict records, a line per workgroup and lane
    l.nXAh = l.nXP = 0;
    l.nXQ = 2 * G * p2_pad(p.Fo * KC + KC, pad);
    l.oXQ = l.oXAh;
    l.oXP = l.oXQ + l.nXQ;
    l.oL1 = l.oXP;
    l.nL1 = l.oXC - l.oXA;
    l.oXV = l.oL1 + l.nL1;
    l.nXV = 2 * G * 8;
    l.ngran = l.oXV + l.nXV;
  }
  return l;
}

template <typename T>
int sghmc_p2_t(hmcx_ctx* ctx, const hmcx_sampler_args* s, const PersistPlan2& pl) {
  const int G = pl.Gr * pl.Gf, K = s->K, KC = kc_of(K);
  const size_t n = (size_t)s->n_steps;
  static const int pad = !(getenv("HMCX_P2_PAD") && getenv("HMCX_P2_PAD")[0] == '0');
  // HMCX_P2_HELP (read per call): 0 = E_current and the momentum draw on the chain's workgroups, 2 = on G
  // helper workgroups (1, E_current alone, measured no gain at the 20-step shape and is not built)
  const char* help_env = getenv("HMCX_P2_HELP");
  size_t lds = pl.lds;
  // HMCX_P2_AHEAD (read per call; else the context's hmcx_set_sghmc_ahead mode): 0 off, 1 on, 2 auto — the
  // rule below on the accept flags the caller has reported (hmcx_sghmc_ahead_note); speed only, never
  // results.  HMCX_P2_HELP alone in the environment asks for the launch it names, without look-ahead.
  // Calls that record the state of every step, or stamp the rounds, run without it.
  static const bool trace_on = getenv("HMCX_P2_TRACE") && getenv("HMCX_P2_TRACE")[0] == '1';
  const char* ahead_env = getenv("HMCX_P2_AHEAD");
  int ahead_want = ahead_env ? atoi(ahead_env) : help_env ? 0 : ctx->sghmc_ahead;
  if (ahead_want == 2) {
    int acc = 0;
    const int seen = std::min(ctx->ahead_seen, P2_AHEAD_WINDOW);
    for (int i = 0; i < seen; ++i) acc += (int)((ctx->ahead_flags >> i) & 1ull);
    ahead_want = ctx->ahead_on = hmcx_p2_ahead_rule(ctx->ahead_on, seen, acc);
  }
  if (s->out_trace || trace_on) ahead_want = 0;
  const int ahead = p2_ahead_mode(pl, K, sizeof(T), ctx->num_cus, ctx->lds_max, ahead_want, &lds);
  const int help = ahead ? 0 : p2_help_mode(pl, K, ctx->num_cus, ctx->lds_max,
                                            help_env ? atoi(help_env) : HMCX_P2_HELP_DEFAULT, &lds);
  const P2Layout lay = p2_layout(pl, K, pad, help, ahead);
  const long ngran = lay.ngran;
  if (ngran * 16 > 0x7fffffffL) return set_error(ctx, HMCX_EUNSUPPORTED, "persistent SGHMC: arena too large");
  int rc = abort_precheck(ctx);                  // an earlier launch's timeout, before enqueueing more
  if (rc) return rc;
  // the call's schedule travels in one packed host-to-device copy
  const bool buf = s->noise_mode == HMCX_NOISE_BUFFER;
  const void* hsrc[5] = {s->eps, s->u_accept, s->row0, s->n_iter, buf ? (const void*)s->noise_off : nullptr};
  const size_t hbytes[5] = {n * sizeof(double), n * sizeof(double), n * sizeof(int64_t), n * sizeof(int32_t),
                            buf ? n * sizeof(int64_t) : 0};
  for (int i = 0; i < 5; ++i)
    if (hbytes[i] && !hsrc[i]) return set_error(ctx, HMCX_EINVAL, "sghmc: null host schedule array");
  const size_t sched_bytes = packed_bytes(5, hbytes);
  // the exchange arena is the context's granule arena: every launch polls for epochs of its own,
  // never written before, so it is not cleared per call
  if ((rc = gx_reserve(ctx, (size_t)ngran * 16))) return rc;
  char* arena = ctx->gx_arena;
  unsigned rounds = 0;                           // ≤ 5 epochs per leapfrog iteration (it = -1 … L-1, accept)
  for (size_t i = 0; i < n; ++i) rounds += 5u * (unsigned)(std::max(s->n_iter[i], 0) + 2);
  rounds += 1 + (help ? 1 : 0);                  // the commit round; with helpers E(-1), the launch's first epoch
  // look-ahead: each lane counts its own rounds from ep0 (in regions of its own) and may run each of its
  // steps three times (as the run started on a parked step and voided with it, as a speculative run voided by
  // its own verdict, and as the redo); the step tags ep0 + k of the verdicts lie in the same range (n_steps ≤
  // rounds)
  if (ahead) rounds = 3 * rounds + 2;
  unsigned ep0 = 1;
  if ((rc = gx_epochs(ctx, rounds, &ep0))) return rc;
  Q2Args a{};
  // a short call's schedule (the driver's 20-step call) rides in the kernel arguments: no staging
  // copy, no upload, no staging event ahead of the launch
  char* dp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (!buf && n <= (size_t)P2_NINL) {
    a.ninl = (int)n;
    for (size_t i = 0; i < n; ++i) {
      a.inl[i].eps = s->eps[i];
      a.inl[i].u = s->u_accept[i];
      a.inl[i].row0 = s->row0[i];
      a.inl[i].n_iter = s->n_iter[i];
    }
  } else {
    Workspace ws(ctx);
    char* sched;
    do {
      ws.reset();
      sched = ws.take<char>(sched_bytes);
    } while (ws.retry());
    if (ws.failed) return HMCX_ENOMEM;
    begin_call(ctx);
    if ((rc = upload_packed(ctx, sched, 5, hsrc, hbytes, dp))) return rc;
  }
  double* d_eps = reinterpret_cast<double*>(dp[0]);
  double* d_u = reinterpret_cast<double*>(dp[1]);
  int64_t* d_row0 = reinterpret_cast<int64_t*>(dp[2]);
  int32_t* d_n = reinterpret_cast<int32_t*>(dp[3]);
  int64_t* d_noff = reinterpret_cast<int64_t*>(dp[4]);

  a.B = s->B; a.D = s->D; a.K = K; a.P = s->D * K + K; a.n_steps = s->n_steps;
  a.Gr = pl.Gr; a.Gf = pl.Gf; a.Br = pl.Br; a.Bf = pl.Bf; a.BfP = pl.BfP; a.BFP = pl.BFP; a.Ro = pl.Ro; a.Fo = pl.Fo;
  a.alpha = s->alpha; a.neg_inv_n = -1.0 / (double)s->B; a.log_prior = s->log_prior;
  a.X = s->X; a.Y = s->Y;
  a.eps = d_eps; a.u = d_u; a.row0 = d_row0; a.n_iter = d_n;
  if (a.ninl > 0) {              // the kernel loads both sources and selects the value (sched_at)
    a.eps = a.u = reinterpret_cast<double*>(ctx->zeros_dev);
    a.row0 = reinterpret_cast<int64_t*>(ctx->zeros_dev);
    a.n_iter = reinterpret_cast<int32_t*>(ctx->zeros_dev);
  }
  a.noise_mode = s->noise_mode; a.noise = s->noise; a.noff = d_noff;
  a.seed = s->seed; a.chain0 = s->chain0; a.step_base = s->step_base;
  a.W = s->W; a.b = s->b;
  a.arena = arena;
  a.oXA = (int)lay.oXA; a.oXD = (int)lay.oXD; a.oXB = (int)lay.oXB; a.oXW = (int)lay.oXW;
  a.oXS = (int)lay.oXS; a.oXC = (int)lay.oXC; a.oXAh = (int)lay.oXAh; a.oXQ = (int)lay.oXQ;
  a.oXP = (int)lay.oXP;
  a.help = help;
  a.ahead = ahead;
  a.laneoff = (int)(lay.oL1 - lay.oXA);
  a.oXV = (int)lay.oXV;
  if (!ctx->ahead_stats_dev) {
    HMCX_HIP(ctx, hipMalloc((void**)&ctx->ahead_stats_dev, 12 * sizeof(int)));
    HMCX_HIP(ctx, hipMemsetAsync(ctx->ahead_stats_dev, 0, 12 * sizeof(int), ctx->stream));
  }
  a.stats = ctx->ahead_stats_dev;
  // HMCX_P2_RUNON (read per call, default 1): 0 = a lane waits for the verdict at the end of every speculative run
  {
    const char* runon_env = getenv("HMCX_P2_RUNON");
    a.runon = (ahead && !(runon_env && runon_env[0] == '0')) ? 1 : 0;
  }
  ctx->ahead_stats_on = ahead;                   // a launch without look-ahead leaves the record alone: all zero then
  a.arena_bytes = (int)(ngran * 16);
  a.ep0 = ep0;
  a.pad = pad;
  static const bool dbg = getenv("HMCX_P2_DEBUG") && getenv("HMCX_P2_DEBUG")[0] == '1';
  if (dbg)
    fprintf(stderr, "[hmcx p2] B=%d D=%d K=%d plan %dx%d Br=%d Bf=%d BfP=%d Ro=%d Fo=%d; granule bases XA %d XD %d XB %d "
            "XW %d XS %d XC %d; help %d XAh %d XQ %d XP %d; ahead %d lane-1 offset %d XV %d; epochs %u..%u\n", s->B, s->D, K,
            pl.Gr, pl.Gf, pl.Br, pl.Bf, pl.BfP, pl.Ro, pl.Fo, a.oXA, a.oXD, a.oXB, a.oXW, a.oXS, a.oXC, a.help, a.oXAh, a.oXQ,
            a.oXP, a.ahead, a.laneoff, a.oXV, ep0, ep0 + rounds - 1);
  {
    const int HA = KC + 1;
    const bool fits = pl.Gf * pl.Ro * KC <= QSTAGE && pl.Gf * (HA + pl.Ro * KC) <= QSTAGE &&
                      pl.Gr * (pl.Fo * KC + HA) <= QSTAGE && pl.Gr * pl.Fo * KC <= QSTAGE;
    static const int spread_env = getenv("HMCX_P2_SPREAD") ? atoi(getenv("HMCX_P2_SPREAD")) : 2;
    a.spread = fits ? spread_env : 0;
    a.zoff = !(getenv("HMCX_P2_ZOFF") && getenv("HMCX_P2_ZOFF")[0] == '0');
    static const int bar_env = getenv("HMCX_P2_BAR") ? atoi(getenv("HMCX_P2_BAR")) : 1;
    a.bar = bar_env == 1 ? 1 : 0;
    // HMCX_P2_XMAP: which team shares an XCD (workgroups are dealt to the XCDs round-robin).  0 = identity
    // map: each FEATURE team on one XCD, its B rounds kept in that XCD's L2 (default with the B all-
    // reduce: its redundant reads, 8x the bytes of the other rounds, then stay off the fabric — same
    // speed, 11.1 -> 4.5 MB of fabric traffic per leapfrog); 1 = each ROW team on one XCD (default
    // without it); 2 = deliberately MISPLACED (test knob, read per call): identity map with the row-team
    // rounds published into one XCD's L2, so members on other XCDs never see them — the launch times
    // out (4 s) and aborts
    const int xmap_env = getenv("HMCX_P2_XMAP") ? atoi(getenv("HMCX_P2_XMAP")) : (a.bar ? 0 : 1);
    a.xmap = (xmap_env == 1 && (pl.Gr * pl.Gf) % 8 == 0) ? 1 : 0;
    static const int fl2_env = getenv("HMCX_P2_FL2") ? atoi(getenv("HMCX_P2_FL2")) : 1;
    a.fl2 = (fl2_env == 1 && !a.xmap && pl.Gf % 8 == 0 && xmap_env != 2) ? 1 : 0;
    a.al2 = (fl2_env == 1 && a.xmap && ((pl.Gr * pl.Gf) / 8) % pl.Gf == 0) ? 1 : 0;
    if (xmap_env == 2) a.al2 = 1;
    static const int pf_env = getenv("HMCX_P2_PREFETCH") ? atoi(getenv("HMCX_P2_PREFETCH")) : 1;
    a.prefetch = pf_env == 1 ? 1 : 0;
    static const int acc1_env = getenv("HMCX_P2_ACC1") ? atoi(getenv("HMCX_P2_ACC1")) : 1;
    a.acc1 = acc1_env == 1 ? 1 : 0;
  }
  a.abort_flag = ctx->abort_dev;
  a.force_abort = getenv("HMCX_P2_FORCE_ABORT") ? atoi(getenv("HMCX_P2_FORCE_ABORT")) : -1;
  a.out_A = s->out_A; a.out_acc = s->out_accepted; a.out_ll = s->out_ll; a.out_E = s->out_E;
  a.out_trace = s->out_trace;
  a.out_mom = s->out_mom;
  a.verdict = s->out_abort;
  // out_host in the packed layout (include/hmcx.h): the kernel stores the per-step outputs and its
  // verdict straight into the pinned host block (a handful of values per step) — no copy behind the
  // launch, so the host's wait ends when the kernel does
  const bool direct_host = s->out_host && s->out_E && s->out_abort && s->out_ll == s->out_A + n &&
                           s->out_E == s->out_A + 2 * n &&
                           reinterpret_cast<char*>(s->out_accepted) == reinterpret_cast<char*>(s->out_A) + 32 * n &&
                           reinterpret_cast<char*>(s->out_abort) == reinterpret_cast<char*>(s->out_A) + 36 * n;
  if (direct_host) {
    char* h = reinterpret_cast<char*>(s->out_host);
    a.out_A = reinterpret_cast<double*>(h);
    a.out_ll = a.out_A + n;
    a.out_E = a.out_A + 2 * n;
    a.out_acc = reinterpret_cast<int32_t*>(h + 32 * n);
    a.verdict = reinterpret_cast<int*>(h + 36 * n);
  }
  static const bool prof_on = getenv("HMCX_PERSIST_PROF") && getenv("HMCX_PERSIST_PROF")[0] == '1';
  unsigned long long* dprof = nullptr;
  if (prof_on) {                                 // one block of 16 per lane (look-ahead: workgroups 0 and G)
    HMCX_HIP(ctx, hipMalloc((void**)&dprof, 32 * sizeof(unsigned long long)));
    HMCX_HIP(ctx, hipMemsetAsync(dprof, 0, 32 * sizeof(unsigned long long), ctx->stream));
  }
  a.prof = dprof;
  unsigned long long* dtrace = nullptr;
  const size_t ntr = (size_t)G * P2TR_IT * 8;
  if (trace_on) {
    HMCX_HIP(ctx, hipMalloc((void**)&dtrace, ntr * sizeof(unsigned long long)));
    HMCX_HIP(ctx, hipMemsetAsync(dtrace, 0, ntr * sizeof(unsigned long long), ctx->stream));
  }
  a.trace = dtrace;
  // the folded instantiation when the call is exactly BASELINE config 2's plan with default knobs
  const bool spec = sizeof(T) == 8 && KC == 10 && s->B == 500 && s->D == 784 && K == 10 && pl.Gr == 8 && pl.Gf == 16 &&
                    pl.Br == 64 && pl.Bf == 49 && pl.BfP == 64 && pl.BFP == 65 && pl.Ro == 4 && pl.Fo == 7 &&
                    a.spread == 2 && a.pad == 1 && a.xmap == 0 && a.fl2 == 1 && a.al2 == 0 && a.prefetch == 1 &&
                    a.acc1 == 1 && a.zoff == 1 && a.bar == 1 && !a.trace && (ahead || a.help == HMCX_P2_HELP_DEFAULT);
  static const bool no_spec = getenv("HMCX_P2_SPEC") && getenv("HMCX_P2_SPEC")[0] == '0';
  const void* kfn = KC == 10 ? (const void*)k_sghmc_p2<T, 10> : (const void*)k_sghmc_p2<T, 16>;
  if constexpr (sizeof(T) == 8) {                // config 2 is f64: no folded f32 kernel is built
    if (spec && !no_spec && !ahead) kfn = a.prof ? (const void*)k_sghmc_p2<T, 10, 3> : (const void*)k_sghmc_p2<T, 10, 1>;
    if (spec && !no_spec && ahead) kfn = a.prof ? (const void*)k_sghmc_p2<T, 10, 5> : (const void*)k_sghmc_p2<T, 10, 4>;
  }
  void* kargs[] = {&a};
  // co-residency of all workgroups (G, or 2·G at one per CU with helpers) is checked here (occupancy
  // query × CUs, cached per kernel); a plain launch then has the same residency as a cooperative one
  // without its per-launch host cost
  const int nwg = (help || ahead) ? 2 * G : G;
  int per_cu = 0;
  if ((rc = kernel_occupancy(ctx, kfn, QTH, (int)lds, &per_cu))) return rc;
  if ((long)per_cu * ctx->num_cus < nwg || ((help || ahead) && per_cu != 1))
    return set_error(ctx, HMCX_EUNSUPPORTED, "persistent SGHMC: workgroups cannot be co-resident");
  // the verdict is sticky (P2Verdict): zeroed here, only a workgroup that leaves without committing
  // stores 1.  The call's output slot is idle at enqueue time (the caller collected its previous use).
  if (direct_host)
    *reinterpret_cast<volatile int*>(a.verdict) = 0;
  else if (a.verdict)
    HMCX_HIP(ctx, hipMemsetAsync(a.verdict, 0, sizeof(int), ctx->stream));
  if ((rc = timing_begin(ctx, ctx->stream))) return rc;
  HMCX_HIP(ctx, hipLaunchKernel(kfn, dim3(nwg), dim3(QTH), kargs, (unsigned)lds, ctx->stream));
  if ((rc = timing_end(ctx, ctx->stream))) return rc;
  if (s->out_host && direct_host) {
    if (!dprof && !dtrace) return HMCX_OK;
  } else if (s->out_host) {                      // outputs and this launch's verdict
    char* h = reinterpret_cast<char*>(s->out_host);
    const bool packed = s->out_abort == reinterpret_cast<int32_t*>(reinterpret_cast<char*>(s->out_A) + 36 * n);
    HMCX_HIP(ctx, hipMemcpyAsync(h, s->out_A, 36 * n + (packed ? sizeof(int) : 0), hipMemcpyDeviceToHost,
                                 ctx->stream));
    if (!packed)
      HMCX_HIP(ctx, hipMemcpyAsync(h + 36 * n, s->out_abort ? (const void*)s->out_abort : ctx->abort_dev,
                                   sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (!dprof && !dtrace) return HMCX_OK;
  }
  if (s->out_abort) {                            // the kernel stored this launch's verdict there itself
    if (!dprof && !dtrace) return HMCX_OK;
  } else if (!dprof && !dtrace) {                // no per-call sync: checked once the launch is done
    return abort_defer(ctx, a.abort_flag, ctx->stream);
  }
  int flag = 0;
  HMCX_HIP(ctx, hipMemcpyAsync(&flag, a.abort_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HMCX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (dprof) {
    unsigned long long hh[32];
    HMCX_HIP(ctx, hipMemcpy(hh, dprof, sizeof(hh), hipMemcpyDeviceToHost));
    (void)hipFree(dprof);
    static const char* names[15] = {"step-start", "A-gemm+publish", "noise", "A-RS wait", "softmax", "A-AG",
                                    "B-gemm+publish", "B-RS wait", "update", "B-AG", "accept", "it=-1",
                                    "verdict wait+apply", "state gather", "stopped run"};
    for (int ln = 0; ln < (ahead ? 2 : 1); ++ln) {
      const unsigned long long* h = hh + 16 * ln;
      unsigned long long tot = 0;
      for (int i = 0; i < 15; ++i) tot += h[i];
      fprintf(stderr, "[hmcx p2 prof] G=%dx%d Br=%d Bf=%d Ro=%d Fo=%d lane %d total %llu ticks:", pl.Gr, pl.Gf, pl.Br,
              pl.Bf, pl.Ro, pl.Fo, ln, tot);
      for (int i = 0; i < 15; ++i) fprintf(stderr, " %s %.1f%% (%llu)", names[i], tot ? 100.0 * h[i] / tot : 0.0, h[i]);
      fprintf(stderr, "\n");
    }
  }
  if (dtrace) {
    std::vector<unsigned long long> h(ntr);
    HMCX_HIP(ctx, hipMemcpy(h.data(), dtrace, ntr * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    (void)hipFree(dtrace);
    // per round: latency = consumed(b) − last publish of b's team; skew = last team publish − publish(b)
    static const char* rn[4] = {"A-RS", "A-AG", "B-RS", "B-AG"};
    for (int rd = 0; rd < 4; ++rd) {
      double lat = 0, skew = 0, lmax = 0;
      long cnt = 0;
      for (int it = 1; it < P2TR_IT; ++it)
        for (int b = 0; b < G; ++b) {
          const int r = b / pl.Gf, f = b % pl.Gf;
          const unsigned long long pub = h[((size_t)b * P2TR_IT + it) * 8 + 2 * rd];
          const unsigned long long done = h[((size_t)b * P2TR_IT + it) * 8 + 2 * rd + 1];
          if (!pub || !done) continue;
          unsigned long long mx = 0;
          const bool rowteam = rd < 2;
          const int nm = rowteam ? pl.Gf : pl.Gr;
          bool okm = true;
          for (int m = 0; m < nm; ++m) {
            const int pb = rowteam ? r * pl.Gf + m : m * pl.Gf + f;
            const unsigned long long v = h[((size_t)pb * P2TR_IT + it) * 8 + 2 * rd];
            if (!v) okm = false;
            mx = v > mx ? v : mx;
          }
          if (!okm) continue;
          const double l = (double)(long long)(done - mx) * 10.0 / 1000.0;   // µs (100 MHz ticks)
          lat += l; lmax = l > lmax ? l : lmax;
          skew += (double)(long long)(mx - pub) * 10.0 / 1000.0;
          ++cnt;
        }
      if (cnt) fprintf(stderr, "[hmcx p2 trace] %s: latency after last team publish %.2f us (max %.2f), own wait for "
                       "slowest member %.2f us (n=%ld)\n", rn[rd], lat / cnt, lmax, skew / cnt, cnt);
    }
    // iteration period from block 0
    const unsigned long long t1 = h[1 * 8 + 0], t2 = h[(P2TR_IT - 1) * 8 + 0];
    if (t1 && t2) fprintf(stderr, "[hmcx p2 trace] leapfrog period %.2f us\n", (double)(t2 - t1) * 10.0 / 1000.0 / (P2TR_IT - 2));
  }
  if (flag) return set_error(ctx, HMCX_EHIP, "persistent SGHMC: hand-off timed out (workgroups not co-resident?)");
  return HMCX_OK;
}

}  // namespace hmcx

// Plan, helper mode and arena layout a call of this shape would get on a device of num_cus CUs (host
// arithmetic only; the tests of the plan read it).  out[0..10]: ok, Gr, Gf, Br, Bf, BfP, Ro, Fo, plan LDS,
// helper mode, launch LDS; out[11]: workgroups launched; out[12..30]: P2Layout in declaration order.
extern "C" int hmcx_p2_plan_query(int B, int D, int K, int tsize, int num_cus, long long lds_max, int pad, int want,
                                  long long* out) {
  using namespace hmcx;
  const PersistPlan2 p = plan_p2(B, D, K, (size_t)tsize, num_cus, (size_t)lds_max);
  for (int i = 0; i < 31; ++i) out[i] = 0;
  out[0] = p.ok;
  if (!p.ok) return 0;
  size_t lds = p.lds;
  const int help = p2_help_mode(p, K, num_cus, (size_t)lds_max, want, &lds);
  const P2Layout l = p2_layout(p, K, pad, help);
  const long long v[] = {p.Gr, p.Gf, p.Br, p.Bf, p.BfP, p.Ro, p.Fo, (long long)p.lds, help, (long long)lds,
                         (long long)(help ? 2 : 1) * p.Gr * p.Gf,
                         l.oXA, l.nXA, l.oXD, l.nXD, l.oXB, l.nXB, l.oXW, l.nXW, l.oXS, l.nXS, l.oXC, l.nXC, l.oXAh, l.nXAh,
                         l.oXQ, l.nXQ, l.oXP, l.nXP, l.ngran};
  for (int i = 0; i < 30; ++i) out[1 + i] = v[i];
  return 0;
}

// Look-ahead of the same call (hmcx_set_sghmc_ahead mode `want`, 1 = on): out[0..3] = mode (1 when the
// launch carries two lanes), workgroups launched, launch LDS, plan LDS; out[4..25]: offset and size of XA,
// XD, XB, XW, XS, XC, XQ, L1 (lane 1's XA … XS), XV in address order, then ngran, Br, BFP, Ro.
extern "C" int hmcx_p2_ahead_query(int B, int D, int K, int tsize, int num_cus, long long lds_max, int pad, int want,
                                   long long* out) {
  using namespace hmcx;
  const PersistPlan2 p = plan_p2(B, D, K, (size_t)tsize, num_cus, (size_t)lds_max);
  for (int i = 0; i < 26; ++i) out[i] = 0;
  if (!p.ok) return 0;
  size_t lds = p.lds;
  const int ahead = p2_ahead_mode(p, K, (size_t)tsize, num_cus, (size_t)lds_max, want, &lds);
  const P2Layout l = p2_layout(p, K, pad, 0, ahead);
  const long long v[] = {ahead, (long long)(ahead ? 2 : 1) * p.Gr * p.Gf, (long long)lds, (long long)p.lds,
                         l.oXA, l.nXA, l.oXD, l.nXD, l.oXB, l.nXB, l.oXW, l.nXW, l.oXS, l.nXS, l.oXC, l.nXC,
                         l.oXQ, l.nXQ, l.oL1, l.nL1, l.oXV, l.nXV, l.ngran, p.Br, p.BFP, p.Ro};
  for (int i = 0; i < 26; ++i) out[i] = v[i];
  return 0;
}

// The auto rule of hmcx_set_sghmc_ahead(ctx, 2): the mode of the next launch from the mode `on` of the
// last one and the accept flags of the context's last `seen` resolved steps, `accepted` of them set.
// Fewer than P2_AHEAD_MIN steps decide nothing.  Look-ahead wins while most proposals are rejected (a
// rejected step's successor was already running); above the break-even accept rate every accepted step
// costs a redone one.  Two thresholds (hysteresis), derived in DESIGN §5.1 round 9.
// The look-ahead counters of the context's latest persistent SGHMC launch (include/hmcx.h): both lanes'
// records added, read behind the stream.
extern "C" int hmcx_sghmc_ahead_stats(hmcx_ctx* ctx, long long out[3]) {
  if (!ctx) return HMCX_EINVAL;
  if (!out) return hmcx::set_error(ctx, HMCX_EINVAL, "ahead_stats: null output");
  out[0] = out[1] = out[2] = 0;
  if (!ctx->ahead_stats_dev || !ctx->ahead_stats_on) return HMCX_OK;
  int h[8];
  HMCX_HIP(ctx, hipMemcpyAsync(h, ctx->ahead_stats_dev, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  HMCX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 3; ++i) out[i] = (long long)h[i] + h[4 + i];
  return HMCX_OK;
}

// The parked-step counters of the same launch (include/hmcx.h): out[0] = steps parked, out[1] = parked steps
// whose verdict came back "changed", both lanes added.
extern "C" int hmcx_sghmc_run_on_stats(hmcx_ctx* ctx, long long out[2]) {
  if (!ctx) return HMCX_EINVAL;
  if (!out) return hmcx::set_error(ctx, HMCX_EINVAL, "run_on_stats: null output");
  out[0] = out[1] = 0;
  if (!ctx->ahead_stats_dev || !ctx->ahead_stats_on) return HMCX_OK;
  int h[12];
  HMCX_HIP(ctx, hipMemcpyAsync(h, ctx->ahead_stats_dev, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  HMCX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out[0] = (long long)h[3] + h[7];
  out[1] = (long long)h[8] + h[9];
  return HMCX_OK;
}

extern "C" int hmcx_p2_ahead_rule(int on, int seen, int accepted) {
  if (seen < hmcx::P2_AHEAD_MIN) return on ? 1 : 0;
  const double rate = (double)accepted / (double)seen;
  if (on && rate > hmcx::P2_AHEAD_OFF_ABOVE) return 0;
  if (!on && rate < hmcx::P2_AHEAD_ON_BELOW) return 1;
  return on ? 1 : 0;
}

namespace hmcx {

template int sghmc_p2_t<float>(hmcx_ctx*, const hmcx_sampler_args*, const PersistPlan2&);
template int sghmc_p2_t<double>(hmcx_ctx*, const hmcx_sampler_args*, const PersistPlan2&);

}  // namespace hmcx
