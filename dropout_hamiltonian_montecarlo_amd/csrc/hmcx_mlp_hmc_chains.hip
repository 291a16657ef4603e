// hmcx_mlp_hmc_chains.hip — full-batch HMC on the dropout MLP, a phase of steps of C chains in one call
// (hmcx_mlp_hmc_chains_run): the step around mlp_leapfrog_t's trajectory — momentum draw, energies, accept, commit,
// trace — on the device, and the chains as the problems of batched launches.  The same step shell carries SGHMC on
// minibatches (hmcx_mlp_sghmc_chains_run, mlp_sghmc_chains_t at the end of the file): its trajectory schedule and its
// element-wise kernel k_sghmc_upd are its own, the start / ends / accept / commit kernels are shared.
// A unit of its own, once per dtype.  The GEMM launches go through helpers seen here as prototypes only
// (hmcx_mlp_shared.h: mlp_chains_forward / mlp_chains_backward of hmcx_mlp_chains.hip, which reach mlp_layer1_batch
// and mlp_forward of hmcx_mlp.hip), so this unit's code object holds its own element-wise kernels and nothing else:
// k_hmc_start, k_hmc_kicks, k_hmc_ends, k_hmc_accept, k_hmc_commit, k_hmc_eval.  The launch group's nets, mask sizes,
// workspaces, noise layout and mask sources are ChainGroup's (hmcx_mlp_shared.h); the arguments are checked in
// hmcx_mlp_checks.h before this unit is reached.
#include "hmcx_mlp_kernels.h"
#include "hmcx_mlp_shared.h"
#include <algorithm>

namespace hmcx {
// A launch group holds up to MAXPROB chains; chain ci of the group keeps its working buffers at fixed strides in
// the call's workspace (proposal q', momentum p, gradient g: [ci][n_v] per variable; energy partials
// [ci][4][6][NPART]: Σp², Σθ² of the current state, then of the proposal; mask scratches [ci][mstride]) and its
// state in the caller's par at [c0 + ci][n_v].  Variables are indexed canonically (0 = W1 .. 5 = b3) everywhere;
// the caller's order enters through e0 (the noise layout), the trajectory's schedule and the energy sums.
template <typename T> struct HmcGroup {
  T* q[6]; T* qn[6]; T* p[6]; T* g[6];
  int n[6], e0[6];
  double* part;
  T* mA; T* mB; int64_t mstride; int n3;
  uint64_t seed; uint32_t chain, step;   // chain: Philox chain of the group's first chain
  DropLaw<T> law;                        // of the group's Philox masks
};

// Step start, every chain of the group (grid NPART × (6 + mask rows) × chains): row v < 6 draws the momentum of
// variable v (BUFFER: the chain's block of the caller's normals; PHILOX: philox_normal_t of (seed, chain, step,
// slot 0, e), the stream of hmcx_philox_normals), stores it in the out_mom slot where one is given, copies q' ← q
// and writes the block's float64 partials of Σp² and Σθ² (k_mlp_init's partition and sums).  The rows behind them
// draw the Philox masks of the chain's first gradient forward (slot 0x80000000) where the chain has a trajectory.
template <typename T> struct HmcStart {
  HmcGroup<T> gr;
  int noise_mode; const double* noise; int64_t noff[MAXPROB];
  T* mom[6]; int64_t mom_stride;      // out_mom slot of the group's first chain, elements per chain = stride·n_v
  int draw_masks[MAXPROB];
};
template <typename T>
__global__ __launch_bounds__(256) void k_hmc_start(HmcStart<T> a) {
  const int ci = blockIdx.z;
  if (blockIdx.y >= 6) {
    if (!a.draw_masks[ci]) return;
    const size_t g = ((size_t)(blockIdx.y - 6) * NPART + blockIdx.x) * 256 + threadIdx.x;
    if (g * 64 < (size_t)a.gr.n3)
      mlp_masks_group<T>(a.gr.law, a.gr.mA + ci * a.gr.mstride, a.gr.n3, a.gr.seed, a.gr.chain + (uint32_t)ci, a.gr.step,
                         MASK_SLOT0, (int)g);
    return;
  }
  const int v = blockIdx.y, n = a.gr.n[v], bx = blockIdx.x;
  double* const part = a.gr.part + (size_t)ci * 24 * NPART;
  const int nb = var_blocks(n);
  if (bx >= nb) {                                              // block-uniform
    if (threadIdx.x == 0) { part[v * NPART + bx] = 0.0; part[(6 + v) * NPART + bx] = 0.0; }
    return;
  }
  const size_t off = (size_t)ci * (size_t)n;
  const T* q = a.gr.q[v] + off;
  T* qn = a.gr.qn[v] + off;
  T* p = a.gr.p[v] + off;
  T* mom = a.mom[v] ? a.mom[v] + (size_t)ci * (size_t)a.mom_stride * (size_t)n : nullptr;
  const double* noise = a.noise_mode == HMCX_NOISE_BUFFER ? a.noise + a.noff[ci] : nullptr;
  const uint32_t chain = a.gr.chain + (uint32_t)ci;
  double sp = 0.0, sq = 0.0;
  for (int i = bx * 256 + threadIdx.x; i < n; i += nb * 256) {
    const uint32_t e = (uint32_t)(a.gr.e0[v] + i);
    const T z = noise ? (T)noise[e] : philox_normal_t<T>(a.gr.seed, chain, a.gr.step, 0u, e);
    const T qv = q[i];
    qn[i] = qv;
    p[i] = z;
    if (mom) mom[i] = z;
    sp += (double)z * (double)z;
    sq += (double)qv * (double)qv;
  }
  block_sum2(sp, sq, part + v * NPART + bx, part + (6 + v) * NPART + bx);
}

// The kicks and the drift between two gradient evaluations, k_mlp_kicks's three rows for every active chain
// (grid x × 3 × active chains; slot j of the table is chain idx[j] of the group): row 0 the second kick of variable
// pu (−1: none), row 1 the first kick and the drift of variable nv where the chain goes on (has_nv), row 2 the
// chain's Philox masks of the next evaluation.  Per element k_mlp_kicks's statements, so the bits are its bits.
// A bias / W3 gradient the kick reads is still the chain's row-block partials: the row computes it first, element
// by element (k_pending's arithmetic, as k_mlp_kicks does): the partials added one after the other in row-block order,
// then apply_upd's v + ½α·θ — with 8 loads in flight per batch as in k_pending_chains (pending_elem's 16 clamped
// row offsets spilled 90 SGPRs here; the value does not depend on the batch size).
template <typename T>
__device__ inline T pend_grad(const T* part, int nparts, int n, int i, T half_alpha, T w) {
  constexpr int PB = 8;
  T s = T(0);
  for (int b0 = 0; b0 < nparts; b0 += PB) {
    T v[PB];
#pragma unroll
    for (int q = 0; q < PB; ++q) v[q] = part[(size_t)min(b0 + q, nparts - 1) * n + i];   // clamped, unconditional
#pragma unroll
    for (int q = 0; q < PB; ++q)
      if (b0 + q < nparts) s = (b0 + q == 0) ? v[q] : s + v[q];
  }
  return s + half_alpha * w;
}
template <typename T> struct HmcKicks {
  int idx[MAXPROB], has_nv[MAXPROB];
  // the group's first chain: momentum, gradient and q' of variable pu (n_u = 0: none) and of variable nv
  T* p_u; T* g_u; const T* q_u; int n_u;
  T* p_v; T* g_v; T* q_v; int n_v;
  T eu, hv, ev, half_alpha;
  const T* part_u; const T* part_v;   // pending partials of pu / nv of the group's first chain, or null
  int64_t pstride; int nparts;
  T* masks; int64_t mstride; int n3;  // masks null: no draw; else where has_nv, the next evaluation's slot
  uint64_t seed; uint32_t chain, step, slot;
  DropLaw<T> law;
};
template <typename T>
__global__ __launch_bounds__(256) void k_hmc_kicks(HmcKicks<T> k) {
  const int ci = k.idx[blockIdx.z];
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, st = (int64_t)gridDim.x * 256;
  if (blockIdx.y == 0) {
    const int n = k.n_u;
    const size_t off = (size_t)ci * (size_t)n;
    T* const pu = k.p_u + off;
    T* const gu = k.g_u + off;
    const T* const part = k.part_u ? k.part_u + (size_t)ci * k.pstride : nullptr;
    const T* const qu = k.q_u + off;
    for (int64_t i = i0; i < n; i += st) {
      if (part) gu[i] = pend_grad<T>(part, k.nparts, n, (int)i, k.half_alpha, qu[i]);
      const T ax = k.eu * gu[i];
      pu[i] = pu[i] - ax;
    }
  } else if (blockIdx.y == 1) {
    if (!k.has_nv[blockIdx.z]) return;
    const int n = k.n_v;
    const size_t off = (size_t)ci * (size_t)n;
    T* const pv = k.p_v + off;
    T* const gv = k.g_v + off;
    T* const qv = k.q_v + off;
    const T* const part = k.part_v ? k.part_v + (size_t)ci * k.pstride : nullptr;
    for (int64_t i = i0; i < n; i += st) {
      if (part) gv[i] = pend_grad<T>(part, k.nparts, n, (int)i, k.half_alpha, qv[i]);
      const T ax = k.hv * gv[i];
      const T p = pv[i] - ax;
      pv[i] = p;
      const T aq = k.ev * p;
      qv[i] = qv[i] + aq;
    }
  } else if (k.masks && k.has_nv[blockIdx.z]) {
    T* const m = k.masks + ci * k.mstride;
    for (int64_t g = i0; 64 * g < k.n3; g += st)
      mlp_masks_group<T>(k.law, m, k.n3, k.seed, k.chain + (uint32_t)ci, k.step, k.slot, (int)g);
  }
}

// After the trajectories, every chain of the group (grid NPART × (6 + mask rows) × chains): rows v < 6 the
// partials of Σp'² and Σθ'² of the proposal (k_sumsq12's sums), the rows behind them the Philox masks of the chain's
// two energy forwards: slot0[ci] (forward 6n + 1, the proposal) into mA, slot0[ci] + 1 (the current state) into mB.
template <typename T> struct HmcEnds {
  HmcGroup<T> gr;
  uint32_t slot0[MAXPROB];
  int draw_masks, ngroups;            // ngroups: mask groups of one forward
};
template <typename T>
__global__ __launch_bounds__(256) void k_hmc_ends(HmcEnds<T> a) {
  const int ci = blockIdx.z;
  if (blockIdx.y >= 6) {
    if (!a.draw_masks) return;
    size_t g = ((size_t)(blockIdx.y - 6) * NPART + blockIdx.x) * 256 + threadIdx.x;
    const int second = g >= (size_t)a.ngroups;
    if (second) g -= (size_t)a.ngroups;
    if (g >= (size_t)a.ngroups) return;
    mlp_masks_group<T>(a.gr.law, (second ? a.gr.mB : a.gr.mA) + ci * a.gr.mstride, a.gr.n3, a.gr.seed,
                       a.gr.chain + (uint32_t)ci, a.gr.step, a.slot0[ci] + (uint32_t)second, (int)g);
    return;
  }
  const int v = blockIdx.y, n = a.gr.n[v], bx = blockIdx.x;
  double* const part = a.gr.part + ((size_t)ci * 24 + 12) * NPART;
  const int nb = var_blocks(n);
  if (bx >= nb) {
    if (threadIdx.x == 0) { part[v * NPART + bx] = 0.0; part[(6 + v) * NPART + bx] = 0.0; }
    return;
  }
  const T* q = a.gr.qn[v] + (size_t)ci * (size_t)n;
  const T* p = a.gr.p[v] + (size_t)ci * (size_t)n;
  double sp = 0.0, sq = 0.0;
  for (int i = bx * 256 + threadIdx.x; i < n; i += nb * 256) {
    const double pv = (double)p[i], qv = (double)q[i];
    sp += pv * pv;
    sq += qv * qv;
  }
  block_sum2(sp, sq, part + v * NPART + bx, part + (6 + v) * NPART + bx);
}

// Energies and accept, one workgroup per chain: k_mlp_accept's sums (each lane a fixed-order strided sum, then a
// fixed-order tree) and composition, E = (loss + log_prior) + K with log_prior = −Σ_v ½α·Σθ_v²/dim_v and
// K = Σ_v ½·Σp_v² over the caller's order; A = min(1, exp(E_cur − E_new)) as Python's min; accepted =
// isfinite(A) && u < A.  Writes A, the flag, E, the group's flag word for the commit and, on an evaluation step,
// Σθ² of the kept state per canonical variable.  The SGHMC schedule also takes, where out_loss / out_nlp are given,
// the mean CE and loss + log_prior of the kept state under that state's energy forward (k_mlp_accept's outputs).
struct HmcAccept {
  const double* part;                 // [chains][4][6][NPART]
  const double* lp_cur; const double* lp_new; int64_t lstride; int nlb, B;
  int order[6], dim[6];
  double alpha, u[MAXPROB];
  double* out_A; int32_t* out_acc; double* out_E; double* out_sumsq;   // at the group's first chain
  double* out_loss; double* out_nlp;  // at the group's first chain, or null
  int32_t* acc;                       // [chains]
};
template <typename T>
__global__ __launch_bounds__(1024) void k_hmc_accept(HmcAccept a) {
  __shared__ double sh[26][32];
  const int ci = blockIdx.x;
  const int t = threadIdx.x, g = t >> 5, j = t & 31;
  double x = 0.0;
  if (g < 24) {
    const double* pp = a.part + ((size_t)ci * 24 + g) * NPART;
    for (int q = 0; q < NPART / 32; ++q) x += pp[q * 32 + j];
  } else if (g < 26) {
    const double* lp = (g == 24 ? a.lp_cur : a.lp_new) + (size_t)ci * a.lstride;
    for (int b = j; b < a.nlb; b += 32) x += lp[b];
  }
  if (g < 26) sh[g][j] = x;
  __syncthreads();
  for (int w = 16; w > 0; w >>= 1) {
    if (g < 26 && j < w) sh[g][j] += sh[g][j + w];
    __syncthreads();
  }
  if (t != 0) return;
  const double lc = sh[24][0] / (double)a.B, ln = sh[25][0] / (double)a.B;
  double pri_c = 0.0, pri_n = 0.0, kc = 0.0, kn = 0.0;
  for (int i = 0; i < 6; ++i) {                                // variables in the caller's order
    const int v = a.order[i];
    pri_c -= 0.5 * a.alpha * sh[6 + v][0] / (double)a.dim[v];
    pri_n -= 0.5 * a.alpha * sh[18 + v][0] / (double)a.dim[v];
    kc += 0.5 * sh[v][0];
    kn += 0.5 * sh[12 + v][0];
  }
  const double Enew = (ln + pri_n) + kn;
  const double Ecur = (lc + pri_c) + kc;
  const double e = exp(Ecur - Enew);
  const double A = (e < 1.0) ? e : 1.0;                       // Python min(1, x)
  const int acc = (A == A) && (A - A == 0.0) && a.u[ci] < A;  // isfinite(A) and u < A
  a.out_A[ci] = A;
  a.out_acc[ci] = acc;
  if (a.out_E) { a.out_E[2 * ci] = Ecur; a.out_E[2 * ci + 1] = Enew; }
  if (a.out_sumsq)
    for (int v = 0; v < 6; ++v) a.out_sumsq[6 * ci + v] = acc ? sh[18 + v][0] : sh[6 + v][0];
  if (a.out_loss) a.out_loss[ci] = acc ? ln : lc;
  if (a.out_nlp) a.out_nlp[ci] = acc ? (ln + pri_n) : (lc + pri_c);
  a.acc[ci] = acc;
}

// Commit and trace, every chain of the group (grid NPART × (6 + mask rows) × chains): q ← q' where the chain's
// flag is set, the kept state into the draw slot where one is given, and in the rows behind them the Philox masks
// of the record forward (slot[ci], forward 6n + 3) into mA.
template <typename T> struct HmcCommit {
  HmcGroup<T> gr;
  const int32_t* acc;
  T* draw[6]; int64_t draw_stride;    // draw slot of the group's first chain, or null
  uint32_t slot[MAXPROB];
  int draw_masks;
};
template <typename T>
__global__ __launch_bounds__(256) void k_hmc_commit(HmcCommit<T> a) {
  const int ci = blockIdx.z;
  if (blockIdx.y >= 6) {
    if (!a.draw_masks) return;
    const size_t g = ((size_t)(blockIdx.y - 6) * NPART + blockIdx.x) * 256 + threadIdx.x;
    if (g * 64 < (size_t)a.gr.n3)
      mlp_masks_group<T>(a.gr.law, a.gr.mA + ci * a.gr.mstride, a.gr.n3, a.gr.seed, a.gr.chain + (uint32_t)ci, a.gr.step,
                         a.slot[ci], (int)g);
    return;
  }
  const int v = blockIdx.y, n = a.gr.n[v];
  const bool take = a.acc[ci] != 0;                            // uniform
  T* const draw = a.draw[v] ? a.draw[v] + (size_t)ci * (size_t)a.draw_stride * (size_t)n : nullptr;
  if (!take && !draw) return;
  T* const q = a.gr.q[v] + (size_t)ci * (size_t)n;
  const T* const qn = a.gr.qn[v] + (size_t)ci * (size_t)n;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const T x = take ? qn[i] : q[i];
    if (take) q[i] = x;
    if (draw) draw[i] = x;
  }
}

// The record's loss, one thread per chain: the mean CE of the record forward (k_loss_final's arithmetic).
template <typename T>
__global__ void k_hmc_eval(const double* lpart, int64_t lstride, int nlb, int B, int np, double* out_loss) {
  const int ci = threadIdx.x;
  if (ci >= np) return;
  const double* lp = lpart + (size_t)ci * lstride;
  double s = 0.0;
  for (int b = 0; b < nlb; ++b) s += lp[b];
  out_loss[ci] = s / (double)B;
}

// The schedule.  Chains are independent, so they run group after group (≤ MAXPROB chains each), a group taking all
// n steps before the next starts: the workspace holds one group.  Per step and group:
//   k_hmc_start                                   momentum, q' ← q, Σp² / Σθ², the masks of forward 0
//   evaluation e = 0 .. max_c(1 + 6·n_c) − 1, for the chains that still have one (n_c > 0 and e < 1 + 6·n_c):
//     layer 1 (only after W1 moved), layer 2, layer 3 + CE, layer-1 backward, W1 / W2 gradient — of these the ones
//     the two wanted components need (mlp_grad_launch's choice) — and k_hmc_kicks
//   k_hmc_ends                                    Σp'² / Σθ'², the masks of the two energy forwards
//   forward at q' (6n + 1), forward at q (6n + 2) all chains; 3 launches each
//   k_hmc_accept, k_hmc_commit
//   on an evaluation step: forward at the kept state (6n + 3), k_hmc_eval
// Every evaluation computes the component of the variable just drifted and of the next one in the order, whether or
// not the chain goes on: what is launched for a chain depends on (e, n_c) alone, never on the other chains.
template <typename T>
int mlp_hmc_chains_t(hmcx_ctx* ctx, const hmcx_mlp_hmc_chains_args* s) {
  const int B = s->B, n_mid = s->n_mid, C = s->C;
  const bool philox = s->mask_mode == HMCX_MLP_MASKS_PHILOX;
  ChainGroup<T> grp(C, B, s->n_in, n_mid, s->n_out, ctx->stream);
  MlpNet<T>* const cn = grp.cn;
  MlpNet<T>& net = cn[0];
  const int G = grp.G, n3 = grp.n3, ng = grp.ng, nlb = net.nlb;
  const size_t mstride = grp.mstride;
  for (int c = 0; c < G; ++c) { cn[c].X = (const T*)s->X; cn[c].y = s->y; }
  Workspace ws(ctx);
  T *g[6], *qn[6], *p[6], *mA = nullptr, *mB = nullptr;
  double *lpA, *lpB, *part;
  int32_t* acc;
  do {
    ws.reset();
    grp.take(ws);
    lpA = ws.take<double>((size_t)G * nlb);
    lpB = ws.take<double>((size_t)G * nlb);
    for (int v = 0; v < 6; ++v) {
      g[v] = ws.take<T>((size_t)G * net.nvar(v));
      qn[v] = ws.take<T>((size_t)G * net.nvar(v));
      p[v] = ws.take<T>((size_t)G * net.nvar(v));
    }
    part = ws.take<double>((size_t)G * 24 * NPART);
    acc = ws.take<int32_t>(MAXPROB);
    if (philox) { mA = ws.take<T>(G * mstride); mB = ws.take<T>(G * mstride); }
  } while (ws.retry());
  if (ws.failed) return set_error(ctx, HMCX_ENOMEM, "mlp hmc chains: the workspace of one launch group does not fit in device memory");
  if (int rc = grp.spacing(ctx, "mlp hmc chains: ")) return rc;
  const int64_t pstride = grp.pstride;
  if (int rc = timing_begin(ctx, ctx->stream)) return rc;
  const int* o = s->order;
  const unsigned mrows1 = grp.mask_rows(1), mrows2 = grp.mask_rows(2);
  for (int c0 = 0; c0 < C; c0 += MAXPROB) {
    const int np = std::min(MAXPROB, C - c0);
    T *qc[MAXPROB][6], *qnc[MAXPROB][6], *gc[MAXPROB][6];
    HmcGroup<T> gr{};
    for (int v = 0; v < 6; ++v) {
      gr.q[v] = (T*)s->par.p[v] + (size_t)c0 * (size_t)net.nvar(v);
      gr.qn[v] = qn[v]; gr.p[v] = p[v]; gr.g[v] = g[v]; gr.n[v] = net.nvar(v);
      for (int c = 0; c < np; ++c) {
        qc[c][v] = gr.q[v] + (size_t)c * net.nvar(v);
        qnc[c][v] = qn[v] + (size_t)c * net.nvar(v);
        gc[c][v] = g[v] + (size_t)c * net.nvar(v);
      }
    }
    grp.noise_layout(o, gr.e0);
    gr.part = part; gr.mA = mA; gr.mB = mB; gr.mstride = (int64_t)mstride; gr.n3 = n3;
    gr.seed = s->seed; gr.chain = s->chain0 + (uint32_t)c0; gr.law = drop_law<T>(ctx);
    // a forward of the listed chains (group indices) at q' or q under forward number f[ci] of the step
    ChainList<T> L{};
    auto list = [&](const int* idx, int n, bool proposal, const int64_t* f, const T* scr, double* lp, size_t sc) {
      L = ChainList<T>{};
      L.n = n;
      for (int j = 0; j < n; ++j) {
        const int ci = idx[j];
        const T* fm = s->mask_mode == HMCX_MLP_MASKS_FIXED
                          ? (const T*)s->masks + s->mask_off[sc + ci] + f[ci] * (int64_t)n3 : nullptr;
        L.net[j] = &cn[ci]; L.q[j] = proposal ? qnc[ci] : qc[ci]; L.g[j] = gc[ci];
        L.ms[j] = grp.mask_src(ci, s->mask_mode, fm, scr);
        L.lpart[j] = lp + (size_t)ci * nlb;
      }
    };
    int n_eval = 0, n_draw = 0;
    for (int si = 0; si < s->n_steps; ++si) {
      const size_t sc = (size_t)si * C + c0;                   // index of the group's first chain in the step's rows
      const double eps = s->eps[si];
      const bool ev = s->want_eval && s->want_eval[si], keep = s->want_draw && s->want_draw[si];
      gr.step = s->step_base + (uint32_t)si;
      int64_t nev[MAXPROB] = {}, maxe = 0, fnum[MAXPROB] = {};
      int all[MAXPROB];
      HmcStart<T> st{};
      for (int c = 0; c < np; ++c) {
        const int64_t n = s->n_iter[sc + c];
        nev[c] = n > 0 ? 1 + 6 * n : 0;
        maxe = std::max(maxe, nev[c]);
        all[c] = c;
        st.noff[c] = s->noise_mode == HMCX_NOISE_BUFFER ? s->noise_off[sc + c] : 0;
        st.draw_masks[c] = philox && n > 0;
      }
      st.gr = gr; st.noise_mode = s->noise_mode; st.noise = s->noise;
      for (int v = 0; v < 6; ++v)
        st.mom[v] = keep && s->out_mom.p[v]
                        ? (T*)s->out_mom.p[v] + ((size_t)c0 * (size_t)s->draw_stride + (size_t)n_draw) * (size_t)net.nvar(v)
                        : nullptr;
      st.mom_stride = s->draw_stride;
      hipLaunchKernelGGL(k_hmc_start<T>, dim3(NPART, 6 + (philox && maxe > 0 ? mrows1 : 0u), (unsigned)np), dim3(256), 0,
                         ctx->stream, st);
      HMCX_HIP(ctx, hipGetLastError());
      bool xw_valid = false;
      for (int64_t e = 0; e < maxe; ++e) {
        HmcKicks<T> k{};
        int na = 0;
        const int i = e > 0 ? (int)((e - 1) % 6) : -1;
        const int vu = e > 0 ? o[i] : -1, vn = e > 0 ? o[(i + 1) % 6] : o[0];
        bool any_nv = false;
        for (int c = 0; c < np; ++c)
          if (e < nev[c]) {
            k.idx[na] = c;
            k.has_nv[na] = e + 1 < nev[c];
            any_nv = any_nv || k.has_nv[na];
            fnum[c] = e;
            ++na;
          }
        const unsigned want = (vu >= 0 ? 1u << vu : 0u) | (1u << vn);
        list(k.idx, na, true, fnum, mA, lpA, sc);
        if (int rc = mlp_chains_forward<T>(ctx, L, want, !xw_valid)) return rc;
        xw_valid = true;
        if (int rc = mlp_chains_backward<T>(ctx, L, want, s->alpha)) return rc;
        if (vu >= 0) { k.p_u = p[vu]; k.g_u = g[vu]; k.q_u = qn[vu]; k.n_u = net.nvar(vu); }
        if (any_nv) { k.p_v = p[vn]; k.g_v = g[vn]; k.q_v = qn[vn]; k.n_v = net.nvar(vn); }
        k.eu = (T)eps; k.hv = (T)(0.5 * eps); k.ev = (T)eps; k.half_alpha = (T)(0.5 * s->alpha);
        k.part_u = vu >= 0 ? grp.part_of(cn[0], vu) : nullptr;
        k.part_v = any_nv ? grp.part_of(cn[0], vn) : nullptr;
        k.pstride = pstride; k.nparts = nlb;
        const bool kmasks = philox && any_nv;
        k.masks = kmasks ? mA : nullptr; k.law = gr.law; k.mstride = (int64_t)mstride; k.n3 = n3;
        k.seed = s->seed; k.chain = gr.chain; k.step = gr.step;
        k.slot = MASK_SLOT0 + (uint32_t)(e + 1);
        int64_t n = 0;
        if (vu >= 0) n = std::max<int64_t>(n, net.nvar(vu));
        if (any_nv) n = std::max<int64_t>(n, net.nvar(vn));
        if (kmasks) n = std::max<int64_t>(n, ng);
        const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(k_hmc_kicks<T>, dim3(nb, 3, (unsigned)na), dim3(256), 0, ctx->stream, k);
        HMCX_HIP(ctx, hipGetLastError());
        if (any_nv && vn == 0) xw_valid = false;
      }
      HmcEnds<T> en{};
      en.gr = gr; en.draw_masks = philox; en.ngroups = ng;
      for (int c = 0; c < np; ++c) {
        fnum[c] = nev[c] > 0 ? nev[c] : 1;                     // 6n + 1
        en.slot0[c] = MASK_SLOT0 + (uint32_t)fnum[c];
      }
      hipLaunchKernelGGL(k_hmc_ends<T>, dim3(NPART, 6 + (philox ? mrows2 : 0u), (unsigned)np), dim3(256), 0, ctx->stream,
                         en);
      HMCX_HIP(ctx, hipGetLastError());
      list(all, np, true, fnum, mA, lpA, sc);                  // the proposal's energy forward
      if (int rc = mlp_chains_forward<T>(ctx, L, 0u, true)) return rc;
      for (int c = 0; c < np; ++c) ++fnum[c];                  // 6n + 2
      list(all, np, false, fnum, mB, lpB, sc);                 // the current state's
      if (int rc = mlp_chains_forward<T>(ctx, L, 0u, true)) return rc;
      HmcAccept ac{};
      ac.part = part; ac.lp_cur = lpB; ac.lp_new = lpA; ac.lstride = nlb; ac.nlb = nlb; ac.B = B;
      for (int v = 0; v < 6; ++v) { ac.order[v] = o[v]; ac.dim[v] = net.nvar(v); }
      ac.alpha = s->alpha;
      for (int c = 0; c < np; ++c) ac.u[c] = s->u_accept[sc + c];
      ac.out_A = s->out_A + sc; ac.out_acc = s->out_accepted + sc;
      ac.out_E = s->out_E ? s->out_E + 2 * sc : nullptr;
      ac.out_sumsq = ev && s->out_eval_sumsq ? s->out_eval_sumsq + 6 * ((size_t)n_eval * C + c0) : nullptr;
      ac.acc = acc;
      hipLaunchKernelGGL(k_hmc_accept<T>, dim3((unsigned)np), dim3(1024), 0, ctx->stream, ac);
      HMCX_HIP(ctx, hipGetLastError());
      HmcCommit<T> cm{};
      cm.gr = gr; cm.acc = acc; cm.draw_stride = s->draw_stride; cm.draw_masks = philox && ev;
      for (int v = 0; v < 6; ++v)
        cm.draw[v] = keep ? (T*)s->draws.p[v] + ((size_t)c0 * (size_t)s->draw_stride + (size_t)n_draw) * (size_t)net.nvar(v)
                          : nullptr;
      for (int c = 0; c < np; ++c) {
        ++fnum[c];                                             // 6n + 3
        cm.slot[c] = MASK_SLOT0 + (uint32_t)fnum[c];
      }
      hipLaunchKernelGGL(k_hmc_commit<T>, dim3(NPART, 6 + (cm.draw_masks ? mrows1 : 0u), (unsigned)np), dim3(256), 0,
                         ctx->stream, cm);
      HMCX_HIP(ctx, hipGetLastError());
      n_draw += keep ? 1 : 0;
      if (ev) {
        list(all, np, false, fnum, mA, lpA, sc);               // the record forward at the kept state
        if (int rc = mlp_chains_forward<T>(ctx, L, 0u, true)) return rc;
        hipLaunchKernelGGL(k_hmc_eval<T>, dim3(1), dim3(64), 0, ctx->stream, (const double*)lpA, (int64_t)nlb, nlb, B, np,
                           s->out_eval_loss + (size_t)n_eval * C + c0);
        HMCX_HIP(ctx, hipGetLastError());
        ++n_eval;
      }
    }
  }
  return timing_end(ctx, ctx->stream);
}

// ------------------------------------------------------------------ hmcx_mlp_sghmc_chains_run
// What follows gradient evaluation f = 6·it + i of the SGHMC trajectory, k_hmc_kicks's three rows for every active
// chain (grid x × rows × active chains; slot j of the table is chain idx[j] of the group): row 0 the SGHMC update of
// the variable just evaluated, pu = order[i] (n_u = 0: none, the launch ahead of a step's first evaluation) —
// apply_upd's statements, g = v + ½α·θ, z, p = ((1 − ε)·p + ε·g) + 2ε·z, with v the W1 / W2 gradient the GEMM left
// (g_u holds v + ½α·θ already, apply_upd's UPD_GRAD) or the bias / W3 row-block partials summed here first
// (pend_grad); z the chain's normal of iteration it: BUFFER noise[noff[ci] + zoff + i], PHILOX (seed, chain,
// step, zslot, e0_u + i).  Row 1 the drift of the next variable, q' += ε·p, where the chain goes on (has_nv); row 2
// the chain's Philox masks of the next evaluation.  pu ≠ nv, so the rows touch different arrays.
template <typename T> struct SghmcUpd {
  int idx[MAXPROB], has_nv[MAXPROB];
  int64_t noff[MAXPROB];              // BUFFER: where the step's noise of chain ci of the group starts
  // the group's first chain: momentum, gradient and q' of variable pu; momentum and q' of variable nv
  T* p_u; const T* g_u; const T* q_u; int n_u;
  const T* p_v; T* q_v; int n_v;
  T eps, one_minus_eps, noise_scale, half_alpha;
  const T* part_u;                    // pending partials of pu of the group's first chain, or null
  int64_t pstride; int nparts;
  int noise_mode; const double* noise; int64_t zoff;
  uint32_t zslot, e0_u;
  T* masks; int64_t mstride; int n3;  // masks null: no draw; else where has_nv, the next evaluation's slot
  uint64_t seed; uint32_t chain, step, slot;
  DropLaw<T> law;
};
template <typename T>
__global__ __launch_bounds__(256) void k_sghmc_upd(SghmcUpd<T> k) {
  const int ci = k.idx[blockIdx.z];
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, st = (int64_t)gridDim.x * 256;
  if (blockIdx.y == 0) {
    const int n = k.n_u;
    if (n == 0) return;
    const size_t off = (size_t)ci * (size_t)n;
    T* const pu = k.p_u + off;
    const T* const gu = k.g_u + off;
    const T* const qu = k.q_u + off;
    const T* const part = k.part_u ? k.part_u + (size_t)ci * k.pstride : nullptr;
    const double* const nz = k.noise_mode == HMCX_NOISE_BUFFER ? k.noise + k.noff[ci] + k.zoff : nullptr;
    const uint32_t chain = k.chain + (uint32_t)ci;
    // two passes over the thread's elements, so that the partials' row offsets and the Philox key are not live
    // together (in one loop they spilled 12 SGPRs): the gradient into the momentum's update term, then the noise
    for (int64_t i = i0; i < n; i += st) {
      const T g = part ? pend_grad<T>(part, k.nparts, n, (int)i, k.half_alpha, qu[i]) : gu[i];
      pu[i] = k.one_minus_eps * pu[i] + k.eps * g;
    }
    for (int64_t i = i0; i < n; i += st) {
      const T z = nz ? (T)nz[i] : philox_normal_t<T>(k.seed, chain, k.step, k.zslot, k.e0_u + (uint32_t)i);
      pu[i] = pu[i] + k.noise_scale * z;
    }
  } else if (blockIdx.y == 1) {
    if (!k.has_nv[blockIdx.z]) return;
    const int n = k.n_v;
    const size_t off = (size_t)ci * (size_t)n;
    const T* const pv = k.p_v + off;
    T* const qv = k.q_v + off;
    for (int64_t i = i0; i < n; i += st) qv[i] = qv[i] + k.eps * pv[i];
  } else if (k.masks && k.has_nv[blockIdx.z]) {
    T* const m = k.masks + ci * k.mstride;
    for (int64_t g = i0; 64 * g < k.n3; g += st)
      mlp_masks_group<T>(k.law, m, k.n3, k.seed, k.chain + (uint32_t)ci, k.step, k.slot, (int)g);
  }
}

// The SGHMC schedule over a group of chains: cpu/sghmc.py:19-39 with the A1 completion as hmcx_mlp_sghmc_run defines
// it, on the step shell of mlp_hmc_chains_t.  Per step and group (≤ MAXPROB chains, a group taking all steps of the
// call before the next starts):
//   k_hmc_start                                   momentum, q' ← q, Σp² / Σθ², the masks of forward 0
//   k_sghmc_upd (no update row)                   the first drift, q'_{order[0]} += ε·p, of the chains with n_c > 0
//   evaluation f = 0 .. max_c(6·n_c) − 1, for the chains that still have one (f < 6·n_c), v = order[f % 6]:
//     layer 1 (only after W1 moved), layer 2, layer 3 + CE, layer-1 backward (v = W1, b1), the W1 / W2 gradient
//     (v = W1, W2) — mlp_grad_launch's choice for the one component v — and k_sghmc_upd: v's momentum update of
//     iteration f / 6, the drift of order[(f + 1) % 6] and the masks of forward f + 1 where the chain goes on
//   k_hmc_ends                                    Σp'² / Σθ'², the masks of the two energy forwards
//   forward at q' (6n), forward at q (6n + 1)     all chains; 3 launches each
//   k_hmc_accept (with out_loss / out_nlp), k_hmc_commit
// What is launched for a chain depends on (f, n_c) alone, never on the other chains.
template <typename T>
int mlp_sghmc_chains_t(hmcx_ctx* ctx, const hmcx_mlp_sghmc_chains_args* s) {
  const int B = s->B, n_mid = s->n_mid, C = s->C;
  const bool philox = s->mask_mode == HMCX_MLP_MASKS_PHILOX;
  ChainGroup<T> grp(C, B, s->n_in, n_mid, s->n_out, ctx->stream);
  MlpNet<T>* const cn = grp.cn;
  MlpNet<T>& net = cn[0];
  const int G = grp.G, n3 = grp.n3, ng = grp.ng, nlb = net.nlb;
  const size_t mstride = grp.mstride;
  Workspace ws(ctx);
  T *g[6], *qn[6], *p[6], *mA = nullptr, *mB = nullptr;
  double *lpA, *lpB, *part;
  int32_t* acc;
  do {
    ws.reset();
    grp.take(ws);
    lpA = ws.take<double>((size_t)G * nlb);
    lpB = ws.take<double>((size_t)G * nlb);
    for (int v = 0; v < 6; ++v) {
      g[v] = ws.take<T>((size_t)G * net.nvar(v));
      qn[v] = ws.take<T>((size_t)G * net.nvar(v));
      p[v] = ws.take<T>((size_t)G * net.nvar(v));
    }
    part = ws.take<double>((size_t)G * 24 * NPART);
    acc = ws.take<int32_t>(MAXPROB);
    if (philox) { mA = ws.take<T>(G * mstride); mB = ws.take<T>(G * mstride); }
  } while (ws.retry());
  if (ws.failed) return set_error(ctx, HMCX_ENOMEM, "mlp sghmc chains: the workspace of one launch group does not fit in device memory");
  if (int rc = grp.spacing(ctx, "mlp sghmc chains: ")) return rc;
  const int64_t pstride = grp.pstride;
  if (int rc = timing_begin(ctx, ctx->stream)) return rc;
  const int* o = s->order;
  const unsigned mrows1 = grp.mask_rows(1), mrows2 = grp.mask_rows(2);
  int64_t P = 0;
  for (int v = 0; v < 6; ++v) P += net.nvar(v);
  for (int c0 = 0; c0 < C; c0 += MAXPROB) {
    const int np = std::min(MAXPROB, C - c0);
    T *qc[MAXPROB][6], *qnc[MAXPROB][6], *gc[MAXPROB][6];
    HmcGroup<T> gr{};
    for (int v = 0; v < 6; ++v) {
      gr.q[v] = (T*)s->par.p[v] + (size_t)c0 * (size_t)net.nvar(v);
      gr.qn[v] = qn[v]; gr.p[v] = p[v]; gr.g[v] = g[v]; gr.n[v] = net.nvar(v);
      for (int c = 0; c < np; ++c) {
        qc[c][v] = gr.q[v] + (size_t)c * net.nvar(v);
        qnc[c][v] = qn[v] + (size_t)c * net.nvar(v);
        gc[c][v] = g[v] + (size_t)c * net.nvar(v);
      }
    }
    grp.noise_layout(o, gr.e0);
    gr.part = part; gr.mA = mA; gr.mB = mB; gr.mstride = (int64_t)mstride; gr.n3 = n3;
    gr.seed = s->seed; gr.chain = s->chain0 + (uint32_t)c0; gr.law = drop_law<T>(ctx);
    // a forward of the listed chains (group indices) at q' or q under forward number f[ci] of the step
    ChainList<T> L{};
    auto list = [&](const int* idx, int n, bool proposal, const int64_t* f, const T* scr, double* lp, size_t sc) {
      L = ChainList<T>{};
      L.n = n;
      for (int j = 0; j < n; ++j) {
        const int ci = idx[j];
        const T* fm = s->mask_mode == HMCX_MLP_MASKS_FIXED
                          ? (const T*)s->masks + s->mask_off[sc + ci] + f[ci] * (int64_t)n3 : nullptr;
        L.net[j] = &cn[ci]; L.q[j] = proposal ? qnc[ci] : qc[ci]; L.g[j] = gc[ci];
        L.ms[j] = grp.mask_src(ci, s->mask_mode, fm, scr);
        L.lpart[j] = lp + (size_t)ci * nlb;
      }
    };
    int n_draw = 0;
    for (int si = 0; si < s->n_steps; ++si) {
      const size_t sc = (size_t)si * C + c0;                   // index of the group's first chain in the step's rows
      const double eps = s->eps[si];
      const bool keep = s->want_draw && s->want_draw[si];
      gr.step = s->step_base + (uint32_t)si;
      for (int c = 0; c < G; ++c) {                            // the step's minibatch
        cn[c].X = (const T*)s->X + (size_t)s->row0[si] * s->n_in;
        cn[c].y = s->y + s->row0[si];
      }
      int64_t nev[MAXPROB] = {}, maxe = 0, fnum[MAXPROB] = {};
      int all[MAXPROB];
      HmcStart<T> st{};
      SghmcUpd<T> k{};                                         // what every launch of the step shares
      for (int c = 0; c < np; ++c) {
        nev[c] = 6 * (int64_t)s->n_iter[sc + c];
        maxe = std::max(maxe, nev[c]);
        all[c] = c;
        st.noff[c] = k.noff[c] = s->noise_mode == HMCX_NOISE_BUFFER ? s->noise_off[sc + c] : 0;
        st.draw_masks[c] = philox && nev[c] > 0;
      }
      st.gr = gr; st.noise_mode = s->noise_mode; st.noise = s->noise;
      hipLaunchKernelGGL(k_hmc_start<T>, dim3(NPART, 6 + (philox && maxe > 0 ? mrows1 : 0u), (unsigned)np), dim3(256), 0,
                         ctx->stream, st);
      HMCX_HIP(ctx, hipGetLastError());
      k.eps = (T)eps; k.one_minus_eps = (T)(1.0 - eps); k.noise_scale = (T)(2.0 * eps); k.half_alpha = (T)(0.5 * s->alpha);
      k.pstride = pstride; k.nparts = nlb;
      k.noise_mode = s->noise_mode; k.noise = s->noise;
      k.mstride = (int64_t)mstride; k.n3 = n3;
      k.seed = s->seed; k.chain = gr.chain; k.step = gr.step;
      bool xw_valid = false;
      for (int64_t e = maxe > 0 ? -1 : 0; e < maxe; ++e) {     // e = −1: the first drift alone
        int na = 0;
        const int vu = e >= 0 ? o[e % 6] : -1, vn = o[(e + 1) % 6];
        const int64_t it = e >= 0 ? e / 6 : 0;
        bool any_nv = false;
        for (int c = 0; c < np; ++c)
          if (nev[c] > 0 && e < nev[c]) {
            k.idx[na] = c;
            k.has_nv[na] = e + 1 < nev[c];
            any_nv = any_nv || k.has_nv[na];
            fnum[c] = e;
            ++na;
          }
        if (e >= 0) {
          const unsigned want = 1u << vu;
          list(k.idx, na, true, fnum, mA, lpA, sc);
          if (int rc = mlp_chains_forward<T>(ctx, L, want, !xw_valid)) return rc;
          xw_valid = true;
          if (int rc = mlp_chains_backward<T>(ctx, L, want, s->alpha)) return rc;
        }
        k.p_u = nullptr; k.g_u = nullptr; k.q_u = nullptr; k.n_u = 0; k.part_u = nullptr;
        k.p_v = nullptr; k.q_v = nullptr; k.n_v = 0;
        if (vu >= 0) {
          k.p_u = p[vu]; k.g_u = g[vu]; k.q_u = qn[vu]; k.n_u = net.nvar(vu);
          k.part_u = grp.part_of(cn[0], vu);
          k.zoff = P * (it + 1) + gr.e0[vu];
          k.zslot = (uint32_t)(it + 1); k.e0_u = (uint32_t)gr.e0[vu];
        }
        if (any_nv) { k.p_v = p[vn]; k.q_v = qn[vn]; k.n_v = net.nvar(vn); }
        const bool kmasks = philox && any_nv && e >= 0;        // forward 0's masks are the start launch's
        k.masks = kmasks ? mA : nullptr; k.law = gr.law;
        k.slot = MASK_SLOT0 + (uint32_t)(e + 1);
        int64_t n = 1;
        if (vu >= 0) n = std::max<int64_t>(n, net.nvar(vu));
        if (any_nv) n = std::max<int64_t>(n, net.nvar(vn));
        if (kmasks) n = std::max<int64_t>(n, ng);
        const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(k_sghmc_upd<T>, dim3(nb, kmasks ? 3u : 2u, (unsigned)na), dim3(256), 0, ctx->stream, k);
        HMCX_HIP(ctx, hipGetLastError());
        if (any_nv && vn == 0) xw_valid = false;
      }
      HmcEnds<T> en{};
      en.gr = gr; en.draw_masks = philox; en.ngroups = ng;
      for (int c = 0; c < np; ++c) {
        fnum[c] = nev[c];                                      // 6n
        en.slot0[c] = MASK_SLOT0 + (uint32_t)fnum[c];
      }
      hipLaunchKernelGGL(k_hmc_ends<T>, dim3(NPART, 6 + (philox ? mrows2 : 0u), (unsigned)np), dim3(256), 0, ctx->stream,
                         en);
      HMCX_HIP(ctx, hipGetLastError());
      list(all, np, true, fnum, mA, lpA, sc);                  // the proposal's energy forward
      if (int rc = mlp_chains_forward<T>(ctx, L, 0u, true)) return rc;
      for (int c = 0; c < np; ++c) ++fnum[c];                  // 6n + 1
      list(all, np, false, fnum, mB, lpB, sc);                 // the current state's
      if (int rc = mlp_chains_forward<T>(ctx, L, 0u, true)) return rc;
      HmcAccept ac{};
      ac.part = part; ac.lp_cur = lpB; ac.lp_new = lpA; ac.lstride = nlb; ac.nlb = nlb; ac.B = B;
      for (int v = 0; v < 6; ++v) { ac.order[v] = o[v]; ac.dim[v] = net.nvar(v); }
      ac.alpha = s->alpha;
      for (int c = 0; c < np; ++c) ac.u[c] = s->u_accept[sc + c];
      ac.out_A = s->out_A + sc; ac.out_acc = s->out_accepted + sc;
      ac.out_E = s->out_E ? s->out_E + 2 * sc : nullptr;
      ac.out_loss = s->out_loss + sc;
      ac.out_nlp = s->out_nlp ? s->out_nlp + sc : nullptr;
      ac.acc = acc;
      hipLaunchKernelGGL(k_hmc_accept<T>, dim3((unsigned)np), dim3(1024), 0, ctx->stream, ac);
      HMCX_HIP(ctx, hipGetLastError());
      HmcCommit<T> cm{};
      cm.gr = gr; cm.acc = acc; cm.draw_stride = s->draw_stride; cm.draw_masks = 0;
      for (int v = 0; v < 6; ++v)
        cm.draw[v] = keep ? (T*)s->draws.p[v] + ((size_t)c0 * (size_t)s->draw_stride + (size_t)n_draw) * (size_t)net.nvar(v)
                          : nullptr;
      hipLaunchKernelGGL(k_hmc_commit<T>, dim3(NPART, 6, (unsigned)np), dim3(256), 0, ctx->stream, cm);
      HMCX_HIP(ctx, hipGetLastError());
      n_draw += keep ? 1 : 0;
    }
  }
  return timing_end(ctx, ctx->stream);
}

#if !defined(HMCX_MLP_DTYPES) || (HMCX_MLP_DTYPES & 1)   // bit 0 float, bit 1 double, as hmcx_mlp.hip
template int mlp_hmc_chains_t<float>(hmcx_ctx*, const hmcx_mlp_hmc_chains_args*);
template int mlp_sghmc_chains_t<float>(hmcx_ctx*, const hmcx_mlp_sghmc_chains_args*);
#endif
#if !defined(HMCX_MLP_DTYPES) || (HMCX_MLP_DTYPES & 2)
template int mlp_hmc_chains_t<double>(hmcx_ctx*, const hmcx_mlp_hmc_chains_args*);
template int mlp_sghmc_chains_t<double>(hmcx_ctx*, const hmcx_mlp_sghmc_chains_args*);
#endif
}  // namespace hmcx
