// hmcx_mlp_kernels.h — the device side of the dropout MLP (hmcx_mlp.hip): argument blocks and kernels.
// Included by hmcx_mlp.hip and hmcx_mlp_chains.hip; a unit's code object holds the template kernels its host code
// launches.  Kernels only one unit launches live in that unit (k_mlp_keep, k_mlp_accept, k_loss_final — static, so
// every unit that saw them would emit them; k_mmc, k_pending_chains, k_mlp_sgld_chains); the SGD / SGLD update
// kernels are in hmcx_mlp_shared.h.
//
// Names: xw = X·W1ᵀ, a1 = xw + b1, h1 = max(a1·m0, 0), h2 = max((h1·W2ᵀ + b2)·m1, 0), d3 = h2·m2,
// z = d3·W3ᵀ + b3; m0, m1, m2 are the three dropout masks of one forward ([B][n_mid] each).
// xw is stored without the bias, so a move of b1 never re-runs the 784-deep layer-1 GEMM: every
// consumer forms a1 = xw + b1 on the fly (the same rounding as the reference's X·W1ᵀ + b1).
//
// Kernels:
//  * k_mm<T, EPI, AOP, BOP, ...>: C = op(A)·op(B) on v_mfma_*_16x16x4, 32x32 output tile per
//    workgroup, K split over its 8 waves (three k chunks in flight per wave, 16-byte vector loads
//    along k for k-contiguous operands, fixed-order LDS combine).  OP_H1 builds h1 from xw, b1 and
//    m0 on the fly (h1 is never stored).  Epilogues: layer 2 (bias, dropout, relu, next dropout →
//    h2, d3); layer 3 + softmax cross-entropy, which in the same workgroup also forms ga2 (the
//    layer-2 backward) and the row-block partials of the b2 / b3 / W3 gradients; the layer-1
//    backward ga1 (+ b1 partials); the weight gradients with the gradient + prior or the SGHMC
//    epilogue (sghmc.py:31-34), which also writes the NEXT iteration's drifted position into the
//    other half of a double buffer (no drift launch).
//  * Deferred updates: the gradient of a bias (or of W3) is a sum of per-row-block partials; its
//    gradient / SGHMC update runs in the prologue of whatever kernel is launched next (none of them
//    reads the momentum or the next-position buffer it writes) — no reduction launch.
//  * k_mlp_start (k_mlp_init + keep_flags) / k_sumsq12 / k_mlp_accept / k_mlp_commit: momentum draw,
//    first drift and energy partials together with the keep flags of every dropout mask of the step
//    (Philox), end-of-trajectory energy partials, MH accept (hmc.py:67-79), commit on accept.
#pragma once
#include "hmcx_common.h"
#include "hmcx_internal.h"
#include "hmcx_granule.h"
#include "hmcx_mlp_mask.h"
#include <type_traits>

namespace hmcx {

constexpr int NPART = 256;    // blocks per variable (grid.x) and energy partials per variable
constexpr int MM_NW = 8;      // waves per k_mm workgroup; the K range is split over them
constexpr int MM_NT = MM_NW * 64;

// Gradient + prior (mlp.py:63) or the SGHMC momentum update (sghmc.py:31,34) of one variable.
template <typename T> struct Upd {
  const T* W; T* P; T* Qn; T* G;     // θ, momentum, next drifted θ (or null), gradient output (GRAD)
  T half_alpha, eps, one_minus_eps, noise_scale;
  int noise_mode; const double* noise;
  uint64_t seed; uint32_t chain, step, slot, e0;
};
enum UpdMode { UPD_NONE = 0, UPD_GRAD = 1, UPD_SGHMC = 2 };

template <typename T>
__device__ inline void apply_upd(const Upd<T>& u, int mode, size_t i, T v) {
  if (mode == UPD_GRAD) {
    u.G[i] = v + u.half_alpha * u.W[i];
  } else {
    const T g = v + u.half_alpha * u.W[i];
    const T z = u.noise_mode == HMCX_NOISE_BUFFER ? (T)u.noise[i]
                                                  : philox_normal_t<T>(u.seed, u.chain, u.step, u.slot, u.e0 + (uint32_t)i);
    const T p = (u.one_minus_eps * u.P[i] + u.eps * g) + u.noise_scale * z;
    u.P[i] = p;
    if (u.Qn) u.Qn[i] = u.W[i] + u.eps * p;                   // sghmc.py:32 of the next iteration
  }
}

// A gradient given as nparts row-block partials [nparts][n], applied by the next kernel's prologue.
template <typename T> struct Pending {
  int mode, n, nparts;
  const T* part;
  Upd<T> u;
};
// the update of element i: the sum of its partials in fixed order (in-order sum of batches of 16 loads
// that all go out before it: one memory round trip per 16 partials instead of one per partial)
template <typename T>
__device__ inline void pending_elem(const Pending<T>& pd, int i) {
  constexpr int PB = 16;                                       // partials loaded per batch
  T s = T(0);
  if (pd.nparts == 4) {                                        // a split-K weight gradient (W2): 4 partials
    T v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = pd.part[(size_t)q * pd.n + i];
    s = ((v[0] + v[1]) + v[2]) + v[3];
    apply_upd(pd.u, pd.mode, i, s);
    return;
  }
  for (int b0 = 0; b0 < pd.nparts; b0 += PB) {
    T v[PB];
#pragma unroll
    for (int q = 0; q < PB; ++q) v[q] = pd.part[(size_t)min(b0 + q, pd.nparts - 1) * pd.n + i];   // clamped, unconditional
#pragma unroll
    for (int q = 0; q < PB; ++q)
      if (b0 + q < pd.nparts) s = (b0 + q == 0) ? v[q] : s + v[q];
  }
  apply_upd(pd.u, pd.mode, i, s);
}
// bid / nb: this workgroup's index among the nb workgroups that share the work (pending_elem's arithmetic,
// written out: routed through pending_elem, the sampler's pending planes measured 0.4 % slower)
template <typename T>
__device__ inline void run_pending(const Pending<T>& pd, int bid, int nb) {
  if (pd.mode == UPD_NONE) return;
  const int nthr = nb * blockDim.x;
  constexpr int PB = 16;                                       // partials loaded per batch
  for (int i = bid * blockDim.x + threadIdx.x; i < pd.n; i += nthr) {
    // all loads of a batch go out before the (in-order) sum: one memory round trip per 16
    // partials instead of one per partial
    T s = T(0);
    if (pd.nparts == 4) {                                      // a split-K weight gradient (W2): 4 partials
      T v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = pd.part[(size_t)q * pd.n + i];
      s = ((v[0] + v[1]) + v[2]) + v[3];
      apply_upd(pd.u, pd.mode, i, s);
      continue;
    }
    for (int b0 = 0; b0 < pd.nparts; b0 += PB) {
      T v[PB];
#pragma unroll
      for (int q = 0; q < PB; ++q) v[q] = pd.part[(size_t)min(b0 + q, pd.nparts - 1) * pd.n + i];   // clamped, unconditional
#pragma unroll
      for (int q = 0; q < PB; ++q)
        if (b0 + q < pd.nparts) s = (b0 + q == 0) ? v[q] : s + v[q];
    }
    apply_upd(pd.u, pd.mode, i, s);
  }
}
// The pending updates a launch applies first (up to four: the bias / W3 sub-steps of one batched
// iteration).  A batched launch (blockIdx.z = problem) runs them in an extra plane of workgroups of
// their own, z = number of problems, beside the problems.
constexpr int MAXPEND = 4;
template <typename T> struct PendSet {
  Pending<T> p[MAXPEND];
  int n;
};
// With at least one workgroup per update, update j gets its own share of the workgroups (they run side
// by side: each is a short chain of partial loads, a Philox draw and stores); otherwise every
// workgroup runs them in turn.
template <typename T>
__device__ inline void run_pendset(const PendSet<T>& ps, int bid, int nb) {
  if (ps.n == 0) return;
  const bool split = nb >= ps.n;
  const int per = split ? nb / ps.n : nb;
#pragma unroll
  for (int j = 0; j < MAXPEND; ++j)
    if (j < ps.n) {
      if (!split) {
        run_pending(ps.p[j], bid, nb);
      } else {
        const int lo = j * per, hi = j == ps.n - 1 ? nb : lo + per;
        if (bid >= lo && bid < hi) run_pending(ps.p[j], bid - lo, hi - lo);
      }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_pending(PendSet<T> ps) {
  run_pendset(ps, (int)(blockIdx.y * gridDim.x + blockIdx.x), (int)(gridDim.x * gridDim.y));
}

enum MMEpi { MM_STORE = 0, MM_L2 = 1, MM_L3CE = 2, MM_GA1 = 3, MM_UPD = 4, MM_L23 = 5 };
enum MMOp { OP_PLAIN = 0, OP_H1 = 1 };

template <typename T> struct MMArgs {
  int M, N, K;
  const T* A; int lda, ta;           // A(m,k) = ta ? A[k·lda + m] : A[m·lda + k]
  const T* B; int ldb, tb;           // B(k,n) = tb ? B[n·ldb + k] : B[k·ldb + n]
  T* C; int ldc;                     // output [M][ldc]
  const T* bias;                     // L2: b2, L3CE: b3
  const T* b1;                       // OP_H1 / GA1: layer-1 bias
  MaskSrc<T> ms;
  const T* H;                        // GA1: xw (the relu gate is (xw + b1)·m0 > 0)
  T* C2;                             // L2: d3
  T* colpart;                        // GA1: b1 partials [gridDim.x][ldc]
  // L3CE extras (per 32-row block): loss, ga2 and the b2 / b3 / W3 gradient partials
  double* lpart; const int32_t* y;
  const T* W3; const T* h2; const T* d3; int n_mid;
  T* ga2; T* pb2; T* pb3; T* pw3;
  int upd_mode; Upd<T> u;            // MM_UPD
  PendSet<T> pend;                   // run first, by the whole grid
  // MM_L23 (layer 2 + layer 3 in one launch): the 32 × n_out logit partials of the column-slice
  // workgroups of one row block meet in a tagged-granule arena (see k_mm)
  char* gx; int gx_bytes; unsigned ep; int* abort_flag;
  int N3; const T* bias3; T* gz;     // n_out, b3 and the gz output of the fused layer 3
  int force_abort;                   // test knob (HMCX_MLP_FORCE_ABORT): raise the abort word, skip the publish
  unsigned long long* prof;          // HMCX_MLP_PROF: per-workgroup s_memrealtime stamps of the MM_L23 phases
  int xmap, xbx, xby;                // GEMM plane placement over the XCDs (xcd_place): 0 dispatch order, 1 y-major
                                     // chunks, 2 xbx × xby tile blocks, one per XCD
};
constexpr int L23_NPH = 12;          // stamps per workgroup and launch (prof)

// Batched launches: several independent problems of one kernel in one grid, problem = blockIdx.z.
// The sub-steps of one leapfrog iteration are independent of each other (see mlp_sghmc_t), so their
// fused forwards (MM_L23) and layer-1 backwards (MM_GA1) go out as one launch each; a problem
// overrides the operands, masks and outputs of the shared MMArgs (dimensions, X, labels, xw shared).
constexpr int MAXPROB = 6;
template <typename T> struct MMProb {
  const T* A; const T* B; T* C;
  const T* b1; const T* bias; const T* W3; const T* bias3;
  MaskSrc<T> ms;
  T* ga2; T* pb2; T* pb3; T* pw3; T* gz; double* lpart; T* colpart;
  char* gx;                          // MM_L23: the problem's own region of the granule arena
};
template <typename T, int NP> struct MMProbsN {
  MMProb<T> p[NP];
  int n;                             // 0: a plain launch
};
template <typename T> using MMProbs = MMProbsN<T, MAXPROB>;
template <typename T> using MMProbs3 = MMProbsN<T, 4>;   // the sub-grids of a dual launch (up to 4 problems)
// Chains as problems (hmcx_mlp_sgld_chains_run, k_mmc): a chain owns every buffer of its step, so its problem
// also overrides what the sub-steps of one SGHMC iteration share or never use in a batched launch — d3 (MM_L2),
// xw (MM_GA1), h2 / d3 (MM_L3CE's layer-3 backward) and θ / gradient of the weight-gradient epilogue (MM_UPD).
template <typename T> struct MMProbC : MMProb<T> {
  T* C2; const T* H; const T* h2; const T* d3;
  const T* uW; T* uG;
};
template <typename T> struct MMChains {
  MMProbC<T> p[MAXPROB];
  int n;
};
template <typename T, typename PR> constexpr bool is_chains_v = std::is_same<PR, MMChains<T>>::value;

template <typename T, int OP>
__device__ inline T op_apply(T x, T mask, T bias) {
  if constexpr (OP == OP_H1) {
    const T t = (x + bias) * mask;                             // h1 = max((xw + b1)·m0, 0)
    return t > T(0) ? t : T(0);
  }
  return x;
}

// k offset, inside a 16-wide k chunk, of MFMA step u (0..3) for lane group lg: each lane's k values
// are contiguous (4 floats / 2+2 doubles), so a k-contiguous operand is one or two 16-byte loads.
template <typename T> __device__ inline int kmap(int u, int lg);
template <> __device__ inline int kmap<float>(int u, int lg) { return 4 * lg + u; }
template <> __device__ inline int kmap<double>(int u, int lg) { return ((u >> 1) << 3) + 2 * lg + (u & 1); }

// Operand values of one 16-k chunk for rows (A) / columns (B) r0 + 16·i + lr, i = 0, 1:
// x[u][i] = Op(r, k0 + kmap(u, lg)).  TR: element (r, k) at P[k·ld + r], else P[r·ld + k].
// VEC (requires !TR, ld % (16/sizeof T) == 0 and a 16-byte aligned P): 16-byte vector loads along k.
// OP_H1 masks index the stored matrix (element idx); its bias column is TR ? r : k.
template <typename T, int OP, int TR, int VEC, int MK>
__device__ inline void load_chunk(T (&x)[4][2], const T* P, int ld, int r0, int R, int k0, int ke, int lr, int lg,
                                  const MaskSrc<T>& ms, const T* b1) {
  if constexpr (!VEC) {
    // scalar path: all 8 operand loads (+ masks and b1 for OP_H1) of the chunk go out first
    T pv[2][4], bv[2][4];
    MRaw<T> mr[2][4];
    bool okv[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = r0 + 16 * i + lr;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + kmap<T>(u, lg);
        const bool ok = r < R && k < ke;
        const size_t idx = ok ? (TR ? (size_t)k * ld + r : (size_t)r * ld + k) : 0;
        okv[i][u] = ok;
        pv[i][u] = P[idx];
        if constexpr (OP == OP_H1) {
          mr[i][u] = mraw<T, MK>(ms, 0, idx);
          bv[i][u] = b1[ok ? (TR ? r : k) : 0];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if constexpr (OP == OP_H1) mpin<T, MK>(mr[i][u]);
        const T mv = OP == OP_H1 ? mfin<T, MK>(ms, mr[i][u]) : T(1);
        const T bb = OP == OP_H1 ? bv[i][u] : T(0);
        x[u][i] = okv[i][u] ? op_apply<T, OP>(pv[i][u], mv, bb) : T(0);
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = r0 + 16 * i + lr;
    const bool rok = r < R;
    if constexpr (VEC) {
      // VEC also requires K % V == 0 (host), so a vector lies entirely inside [k0, ke) or entirely
      // outside it.  Every load is unconditional (clamped address, zeroed afterwards): a load under
      // a branch makes hipcc wait for it before the next one, which serialises the k chunks.
      constexpr int V = 16 / sizeof(T);
#pragma unroll
      for (int h = 0; h < 4 / V; ++h) {                        // f32: one float4; f64: two double2
        const int kv = k0 + (sizeof(T) == 8 ? 8 * h + 2 * lg : 4 * lg);
        const bool ok = rok && kv < ke;
        const size_t base = ok ? (size_t)r * ld + kv : 0;
        T v[V], m[V], bb[V];
        if constexpr (V == 4) {
          const float4 w = *reinterpret_cast<const float4*>(P + base);
          v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
        } else {
          const double2 w = *reinterpret_cast<const double2*>(P + base);
          v[0] = w.x; v[1] = w.y;
        }
        if constexpr (OP == OP_H1) {
          mvals<T, V, MK>(ms, 0, base, m);
#pragma unroll
          for (int q = 0; q < V; ++q) bb[q] = b1[ok ? kv + q : q];
        }
#pragma unroll
        for (int q = 0; q < V; ++q) x[h * V + q][i] = ok ? op_apply<T, OP>(v[q], m[q], bb[q]) : T(0);
      }
    }
  }
}

// Softmax cross-entropy of the rows of one 32-row block held in LDS zt[32][zs] (F.softmax_cross_entropy,
// mean): gz = (softmax − onehot)/M replaces z in LDS and goes to gz[m][ldg]; lpart[blk] = Σ −log p[y].
template <typename T>
__device__ inline void ce_rows(T* zt, int zs, double* rowl, int m0, int M, int N, const int32_t* y, T* gz, int ldg,
                               double* lpart, int blk, bool writer = true) {
  const int t = threadIdx.x;
  if (t < 32) {
    T* zr = zt + t * zs;
    const int m = m0 + t;
    double l = 0.0;
    if (m < M) {
      T mx = zr[0];
      for (int k = 1; k < N; ++k) mx = zr[k] > mx ? zr[k] : mx;
      T s = T(0);
      for (int k = 0; k < N; ++k) s += exp(zr[k] - mx);
      const T ls = log(s);
      const int lab = y[m];
      l = -(double)((zr[lab] - mx) - ls);
      for (int k = 0; k < N; ++k) {
        T g = exp((zr[k] - mx) - ls);
        if (k == lab) g -= T(1);
        g = g / (T)M;
        zr[k] = g;
        if (writer) gz[(size_t)m * ldg + k] = g;
      }
    } else {
      for (int k = 0; k < N; ++k) zr[k] = T(0);
    }
    rowl[t] = l;
  }
  __syncthreads();
  if (t == 0 && writer) {
    double s = 0.0;
    for (int r = 0; r < 32; ++r) s += rowl[r];
    lpart[blk] = s;
  }
}

// ce_rows with the classes of a row spread over LPR lanes (LPR ≥ N; 16 or 32): max, Σexp and the
// label's log-probability by lane butterflies instead of serial loops over LDS, the row's label
// already in a register (yv[pass], loaded at kernel start).  Same formula as ce_rows (F.softmax_
// cross_entropy, mean): gz = (exp((z − max) − log Σ) − onehot)/M; lpart[blk] = Σ_rows −log p[y].
template <typename T, int LPR>
__device__ inline void ce_rows_lanes(T* zt, int zs, double* rowl, int m0, int M, int N, const int32_t (&yv)[2],
                                     T* gz, int ldg, double* lpart, int blk, bool writer) {
  constexpr int RPP = MM_NT / LPR;                               // rows per pass
  const int t = threadIdx.x, k = t % LPR;
#pragma unroll
  for (int pass = 0; pass < 32 / RPP; ++pass) {
    const int r = pass * RPP + t / LPR, m = m0 + r;
    const bool kin = k < N;
    const T z = kin ? zt[r * zs + k] : T(0);
    T mx = kin ? z : -INFINITY;
#pragma unroll
    for (int w = LPR / 2; w >= 1; w >>= 1) {                      // NaN propagates as in np.max
      const T o = __shfl_xor(mx, w, LPR);
      mx = (o > mx || o != o) ? o : mx;
    }
    T e = kin ? exp(z - mx) : T(0);
#pragma unroll
    for (int w = LPR / 2; w >= 1; w >>= 1) e += __shfl_xor(e, w, LPR);
    const T ls = log(e);
    const int lab = yv[pass];
    double l = (kin && k == lab && m < M) ? -(double)((z - mx) - ls) : 0.0;
    if (kin) {
      T g = T(0);
      if (m < M) {
        g = exp((z - mx) - ls);
        if (k == lab) g -= T(1);
        g = g / (T)M;
        if (writer) gz[(size_t)m * ldg + k] = g;
      }
      zt[r * zs + k] = g;
    }
#pragma unroll
    for (int w = LPR / 2; w >= 1; w >>= 1) l += __shfl_xor(l, w, LPR);
    if (k == 0) rowl[r] = l;
  }
  __syncthreads();
  if (t == 0 && writer) {
    double s = 0.0;
    for (int r = 0; r < 32; ++r) s += rowl[r];
    lpart[blk] = s;
  }
}

// Layer-3 backward of one 32-row block from gz in LDS (zt[32][zs], N = n_out columns; rows past M
// hold zeros):  ga2 = ((gz·W3)·m2)·[h2>0]·m1 and its column sums (b2 partial), column sums of gz
// (b3 partial), and gzᵀ·d3 over the block's rows (W3 partial).  Threads own a column j and a row
// group (rows ≡ g mod R, R = blockDim / n_mid); W3 is staged in LDS scratch `scr` when it fits.
// Columns [jlo, jhi) of n_mid only (the workgroup's slice: the layer-3 kernel runs one workgroup per
// (row block, column slice)); `first` marks the slice that also writes the b3 partial.
// `a`: the launch's MMArgs, or the fields below of a chain's problem (L3Args, k_mmc).
template <typename T> struct L3Args {
  int M, N, n_mid;
  const T* W3; const T* h2; const T* d3;
  MaskSrc<T> ms;
  T* ga2; T* pb2; T* pb3; T* pw3;
};
template <typename T, int MK, typename AR>
__device__ inline void l3_backward(const AR& a, const T* zt, int zs, int m0, int blk, T* scr, int scr_n,
                                   int jlo, int jhi, bool first, int n_out = -1) {
  const int N = n_out >= 0 ? n_out : a.N, nm = a.n_mid, nj = jhi - jlo;
  const int rows = min(32, a.M - m0);
  const int tid = threadIdx.x, nt = blockDim.x;
  if (a.ga2 && nj > 0) {
    const bool wl = N * nm + nt <= scr_n;                      // W3 in LDS (+ nt values for the combine)
    T* w3 = scr + nt;
    if (wl) {                                                  // the slice's columns, 8 loads in flight
      const int nw = N * nj;
      for (int e0 = tid; e0 < nw; e0 += 8 * nt) {
        T v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int e = min(e0 + q * nt, nw - 1), o = e / nj;
          v[q] = a.W3[(size_t)o * nm + jlo + (e - o * nj)];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (e0 + q * nt < nw) {
            const int e = e0 + q * nt, o = e / nj;
            w3[o * nm + jlo + (e - o * nj)] = v[q];
          }
      }
      __syncthreads();
    }
    const int R = max(1, nt / nj), cols = nt / R;
#pragma unroll 1
    for (int jb = jlo; jb < jhi; jb += cols) {
      const int j = jb + tid % cols, g = tid / cols;
      const bool act = g < R && j < jhi;
      T cs = T(0);
      // RB rows per pass (rows g, g + R, …): their h2 / mask loads go out first, then RB independent
      // dot products; RB = 32 / R so that one pass covers the 32-row block
      auto rows_pass = [&](auto rbc) {
        constexpr int RB = decltype(rbc)::value;
#pragma unroll 1
        for (int r0 = g; r0 < rows; r0 += RB * R) {
          T hv[RB], m1v[RB], m2v[RB], acc8[RB];
#pragma unroll
          for (int c = 0; c < RB; ++c) {
            const int r = min(r0 + c * R, rows - 1);
            const size_t i = (size_t)(m0 + r) * nm + j;
            hv[c] = a.h2[i];
            m1v[c] = mval<T, MK>(a.ms, 1, i);
            m2v[c] = mval<T, MK>(a.ms, 2, i);
            acc8[c] = T(0);
          }
#pragma unroll 1
          for (int o = 0; o < N; ++o) {
            const T w = wl ? w3[o * nm + j] : a.W3[(size_t)o * nm + j];
#pragma unroll
            for (int c = 0; c < RB; ++c) acc8[c] += zt[min(r0 + c * R, 31) * zs + o] * w;
          }
#pragma unroll
          for (int c = 0; c < RB; ++c) {
            const int r = r0 + c * R;
            T t = acc8[c] * m2v[c];
            t = t * (hv[c] > T(0) ? T(1) : T(0));
            t = t * m1v[c];
            if (r < rows) {
              a.ga2[(size_t)(m0 + r) * nm + j] = t;
              cs += t;
            }
          }
        }
      };
      if (act) {
        if (R <= 2) rows_pass(std::integral_constant<int, 16>{});
        else if (R <= 4) rows_pass(std::integral_constant<int, 8>{});
        else if (R <= 8) rows_pass(std::integral_constant<int, 4>{});
        else rows_pass(std::integral_constant<int, 2>{});
      }
      if (a.pb2) {
        scr[tid] = cs;
        __syncthreads();
        if (act && g == 0) {
          T t = scr[tid];
          for (int q = 1; q < R; ++q) t += scr[q * cols + tid];
          a.pb2[(size_t)blk * nm + j] = t;
        }
        __syncthreads();
      }
    }
  }
  if (a.pb3 && first) {
    for (int j = tid; j < N; j += nt) {
      T cs = T(0);
      for (int r = 0; r < rows; ++r) cs += zt[r * zs + j];
      a.pb3[(size_t)blk * N + j] = cs;
    }
  }
  if (a.pw3) {
#pragma unroll 1
    for (int j = jlo + tid; j < jhi; j += nt) {                // one column of d3 per thread, all rows
      T dv[32];
#pragma unroll
      for (int r = 0; r < 32; ++r) dv[r] = a.d3[(size_t)(m0 + min(r, rows - 1)) * nm + j];
#pragma unroll 1
      for (int o = 0; o < N; ++o) {
        T sacc = T(0);
#pragma unroll
        for (int r = 0; r < 32; ++r) sacc += zt[r * zs + o] * dv[r];   // rows past M: gz = 0
        a.pw3[(size_t)blk * N * nm + (size_t)o * nm + j] = sacc;
      }
    }
  }
}

template <typename T, int EPI, int MK>
__device__ inline void mm_epilogue(const MMArgs<T>& a, int m, int n, T v) {
  const size_t i = (size_t)m * a.ldc + n;
  if constexpr (EPI == MM_STORE) {
    a.C[i] = v;
  } else if constexpr (EPI == MM_L2) {                          // mlp.py:30-31
    const T t = (v + a.bias[n]) * mval<T, MK>(a.ms, 1, i);
    const T h = t > T(0) ? t : T(0);
    a.C[i] = h;
    a.C2[i] = h * mval<T, MK>(a.ms, 2, i);
  } else if constexpr (EPI == MM_UPD) {
    apply_upd(a.u, a.upd_mode, i, v);
  }
}

// The workgroup's place in its (sub-)grid: a dual launch (k_mm2) runs two grids in one.
struct Blk { int x, y, z, gx, gy; };

template <typename T, int EPI, int AOP, int BOP, int TA, int TB, int AV, int BV, int MK, typename PR>
__device__ __forceinline__ void mm_body(const MMArgs<T>& a, const PR& pr, const Blk bk,
                                        T (&red)[MM_NW][32][33], double* rowl) {
  using M = mfma16<T>;
  const int pbid0 = bk.y * bk.gx + bk.x, nb0 = bk.gx * bk.gy;
  // The pending updates run in an extra plane of workgroups of their own (z = number of problems, 1
  // for a plain launch), beside the GEMM: nothing in this launch reads what they write (the momentum
  // and the NEXT iteration's position buffer of other variables), and no GEMM workgroup waits for them.
  if ((int)bk.z == (pr.n > 0 ? pr.n : 1)) {
    run_pendset(a.pend, pbid0, nb0);
    return;
  }
  // batched launch (pr.n > 0): the problem of this workgroup (bk.z) supplies the operands, masks
  // and outputs; the kernel argument block itself is never copied (a local MMArgs would live in scratch)
  const MMProb<T>* pp = pr.n > 0 ? &pr.p[bk.z] : nullptr;
  const T* const oA = pp ? pp->A : a.A;
  const T* const oB = pp ? pp->B : a.B;
  T* const oC = pp ? pp->C : a.C;
  const T* const ob1 = pp ? pp->b1 : a.b1;
  const T* const obias = pp ? pp->bias : a.bias;
  const T* const oW3 = pp ? pp->W3 : a.W3;
  const T* const obias3 = pp ? pp->bias3 : a.bias3;
  const MaskSrc<T> oms = pp ? pp->ms : a.ms;
  T* const oga2 = pp ? pp->ga2 : a.ga2;
  T* const opb2 = pp ? pp->pb2 : a.pb2;
  T* const opb3 = pp ? pp->pb3 : a.pb3;
  T* const opw3 = pp ? pp->pw3 : a.pw3;
  T* const ogz = pp ? pp->gz : a.gz;
  double* const olpart = pp ? pp->lpart : a.lpart;
  T* const ocolpart = pp ? pp->colpart : a.colpart;
  char* const ogx = pp ? pp->gx : a.gx;
  // a chain's problem (k_mmc: always batched) also supplies xw of MM_GA1; every other launch shares it
  constexpr bool CH = is_chains_v<T, PR>;
  const T* const oH = [&] {
    if constexpr (CH) return pr.p[bk.z].H;
    else return a.H;
  }();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  // MM_L3CE: bk.y is the n_mid column slice of the layer-3 backward (N = n_out ≤ 32: one tile)
  const int m0 = bk.x * 32, n0 = EPI == MM_L3CE ? 0 : bk.y * 32;
  const int pbid = bk.y * bk.gx + bk.x;
  auto stamp = [&](int ph) {
    if constexpr (EPI == MM_L23)
      if (a.prof && tid == 0) a.prof[(size_t)pbid * L23_NPH + ph] = __builtin_amdgcn_s_memrealtime();
  };
  stamp(0);
  // MM_L23: every operand of the epilogue and of layer 3 that does not depend on the GEMM (dropout
  // masks m1 / m2 and b2 of the two tile elements a thread finishes, the slice's W3 columns, b3) is
  // loaded before the GEMM's own operands, so the epilogue never waits on memory
  MRaw<T> pm1[2], pm2[2];
  T pb2v[2], pw3v[2], pb3v = T(0);
  int32_t yv[2] = {0, 0};
  if constexpr (EPI == MM_L23) {
    // labels of the rows this thread handles in the cross-entropy (ce_rows_lanes)
    const int lpr = a.N3 <= 16 ? 16 : 32, rpp = MM_NT / lpr;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) yv[pass] = a.y[min(m0 + pass * rpp + tid / lpr, a.M - 1)];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + MM_NT * u, mm = e >> 5, nn = e & 31, m = m0 + mm, n = n0 + nn;
      const bool ok = m < a.M && n < a.N;
      const size_t i = ok ? (size_t)m * a.ldc + n : 0;
      pm1[u] = mraw<T, MK>(oms, 1, i);
      pm2[u] = mraw<T, MK>(oms, 2, i);
      pb2v[u] = obias[ok ? n : 0];
      const int o = e >> 5, c = e & 31;
      const bool okw = o < a.N3 && n0 + c < a.N;
      pw3v[u] = oW3[okw ? (size_t)o * a.n_mid + n0 + c : 0];
    }
    pb3v = obias3[tid < a.N3 ? tid : 0];
  }
  stamp(7);
  const int Kq = ((a.K + 16 * MM_NW - 1) / (16 * MM_NW)) * 16;   // k range per wave (multiple of 16)
  const int kb = wave * Kq, ke = min(a.K, kb + Kq);
  typename M::acc_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = M::zero();
  // three chunks in flight (register ring), then one MFMA batch per chunk
  T av[3][4][2], bv[3][4][2];
  auto load = [&](int s, int k0) {
    load_chunk<T, AOP, TA, AV, MK>(av[s], oA, a.lda, m0, a.M, k0, ke, lr, lg, oms, ob1);
    load_chunk<T, BOP, !TB, BV, MK>(bv[s], oB, a.ldb, n0, a.N, k0, ke, lr, lg, oms, ob1);
  };
  auto mfma = [&](int s, int k0) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = M::fma(av[s][u][i], bv[s][u][j], acc[i][j]);
    if (s == 0) stamp(8);
  };
  if (kb < ke) load(0, kb);
  if (kb + 16 < ke) load(1, kb + 16);
  if (kb + 32 < ke) load(2, kb + 32);
  for (int k0 = kb; k0 < ke; k0 += 48) {
    mfma(0, k0);
    if (k0 + 48 < ke) load(0, k0 + 48);
    if (k0 + 16 < ke) {
      mfma(1, k0 + 16);
      if (k0 + 64 < ke) load(1, k0 + 64);
    }
    if (k0 + 32 < ke) {
      mfma(2, k0 + 32);
      if (k0 + 80 < ke) load(2, k0 + 80);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[wave][16 * i + M::row(lane, q)][16 * j + lr] = acc[i][j][q];
  stamp(9);
  __syncthreads();
  stamp(10);
#pragma unroll
  for (int u = 0; u < 1024 / MM_NT; ++u) {
    const int e = tid + MM_NT * u, mm = e >> 5, nn = e & 31;
    const int m = m0 + mm, n = n0 + nn;
    T v = red[0][mm][nn];
#pragma unroll
    for (int w = 1; w < MM_NW; ++w) v += red[w][mm][nn];
    if constexpr (EPI == MM_L3CE) {
      red[0][mm][nn] = (n < a.N) ? v + obias[n] : T(0);     // logits of the block (one writer each)
    } else if constexpr (EPI == MM_GA1) {                      // (ga2·W2)·[(xw + b1)·m0 > 0]·m0
      T g = T(0);
      if (m < a.M && n < a.N) {
        const size_t i = (size_t)m * a.ldc + n;
        const T m0v = mval<T, MK>(oms, 0, i);
        g = (v * ((oH[i] + ob1[n]) * m0v > T(0) ? T(1) : T(0))) * m0v;
        oC[i] = g;
      }
      red[0][mm][nn] = g;
    } else if constexpr (EPI == MM_L23) {                      // mlp.py:30-31; the tile stays in LDS
      T d = T(0), h = T(0), m1 = T(0), m2 = T(0);
      mpin<T, MK>(pm1[u]);
      mpin<T, MK>(pm2[u]);
      if (m < a.M && n < a.N) {
        m1 = mfin<T, MK>(oms, pm1[u]);
        m2 = mfin<T, MK>(oms, pm2[u]);
        const T t = (v + pb2v[u]) * m1;
        h = t > T(0) ? t : T(0);
        d = h * m2;
        if (oC) {                                              // h2 / d3 are dead in the fused sampler
          const size_t i = (size_t)m * a.ldc + n;
          oC[i] = h;
          a.C2[i] = d;
        }
      }
      // planes of this element only (each (mm, nn) has one thread): d3, h2, m1, m2 of the tile
      red[0][mm][nn] = d;
      red[3][mm][nn] = h;
      red[4][mm][nn] = m1;
      red[5][mm][nn] = m2;
    } else if constexpr (EPI == MM_STORE) {
      if (m < a.M && n < a.N) oC[(size_t)m * a.ldc + n] = v;
    } else if constexpr (CH) {                                 // mm_epilogue's arithmetic on the chain's own buffers
      if (m < a.M && n < a.N) {
        const MMProbC<T>& pc = pr.p[bk.z];
        const size_t i = (size_t)m * a.ldc + n;
        if constexpr (EPI == MM_L2) {
          const T t = (v + obias[n]) * mval<T, MK>(oms, 1, i);
          const T h = t > T(0) ? t : T(0);
          oC[i] = h;
          pc.C2[i] = h * mval<T, MK>(oms, 2, i);
        } else {                                               // MM_UPD, UPD_GRAD (apply_upd)
          static_assert(EPI == MM_UPD, "k_mmc: MM_L2, MM_L3CE, MM_GA1 and MM_UPD");
          pc.uG[i] = v + a.u.half_alpha * pc.uW[i];
        }
      }
    } else {
      if (m < a.M && n < a.N) mm_epilogue<T, EPI, MK>(a, m, n, v);
    }
  }
  if constexpr (EPI == MM_L3CE) {
    __syncthreads();
    const bool first = bk.y == 0;
    ce_rows<T>(&red[0][0][0], 33, rowl, m0, a.M, a.N, a.y, oC, a.ldc, olpart, bk.x, first);
    __syncthreads();
    const int cw = (a.n_mid + bk.gy - 1) / bk.gy;
    const int jlo = min(a.n_mid, (int)bk.y * cw), jhi = min(a.n_mid, jlo + cw);
    if constexpr (CH) {
      const MMProbC<T>& pc = pr.p[bk.z];
      const L3Args<T> la{a.M, a.N, a.n_mid, oW3, pc.h2, pc.d3, oms, oga2, opb2, opb3, opw3};
      l3_backward<T, MK>(la, &red[0][0][0], 33, m0, bk.x, &red[1][0][0], (MM_NW - 1) * 32 * 33, jlo, jhi, first);
    } else {
      l3_backward<T, MK>(a, &red[0][0][0], 33, m0, bk.x, &red[1][0][0], (MM_NW - 1) * 32 * 33, jlo, jhi, first);
    }
  }
  if constexpr (EPI == MM_L23) {
    // Layer 3 of this row block, in the same launch: z = d3·W3ᵀ + b3 (mlp.py:31) needs all n_mid
    // columns, which the S = bk.gy column-slice workgroups of the block hold.  Each publishes
    // its 32 × n_out partial (own 32 columns, k order within the slice) as 16-byte granules
    // {lo32, ep, hi32, ep} with write-through (sc1) stores; every member reads all S partials of
    // every (row, class) and sums them in slice order — the all-reduce by redundant reads of
    // hmcx_persist2.hip — then runs the cross-entropy of the block (slice 0 writes loss and gz) and
    // the layer-3 backward of its own columns.  The epoch is new per launch and the arena only ever
    // holds granules of earlier launches, so no stale value can match.
    const int No = a.N3, S = bk.gy, s = bk.y, rb = bk.x;
    T* d3t = &red[0][0][0];                                      // [32][33] d3 of the tile
    T* w3s = &red[1][0][0];                                      // [n_out][32] W3 columns of the slice
    T* zt = &red[2][0][0];                                       // [32][33] logits, then gz
    T* b3s = &red[7][0][0];                                      // [n_out] b3
    __syncthreads();                                             // the reduction has read every red[w]
    stamp(1);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + MM_NT * u;
      if (e < No * 32) w3s[e] = n0 + (e & 31) < a.N ? pw3v[u] : T(0);  // prefetched; zero past n_mid
    }
    if (tid < No) b3s[tid] = pb3v;
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs = gx_rsrc(ogx, a.gx_bytes);
    const int items = 32 * No;
    const int base_rb = rb * S * items;
    if (a.force_abort && pbid == 0 && tid == 0)                  // test knob: this launch never completes
      __hip_atomic_store(a.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // items reaches 1024 at n_out = 32, twice the workgroup: two passes, and every put of a thread goes out
    // before its first poll (the other slices of the row block wait for them)
#pragma unroll
    for (int u = 0; u < 1024 / MM_NT; ++u) {
      const int e = tid + MM_NT * u;
      if (e < items && !(a.force_abort && pbid == 0)) {
        const int r = e / No, o = e - r * No;
        T zp = T(0);
#pragma unroll 8
        for (int c = 0; c < 32; ++c) zp += d3t[r * 33 + c] * w3s[o * 32 + c];
        gx_put(rs, base_rb + s * items + e, (double)zp, a.ep);
      }
    }
    stamp(2);
    stamp(3);
#pragma unroll 1
    for (int u = 0; u < 1024 / MM_NT; ++u) {
      const int e = tid + MM_NT * u;
      if (e < items) {
        const int r = e / No, o = e - r * No;
        double sum = 0.0;
        (void)gx_poll_sum(rs, base_rb + e, items, S, a.ep, a.abort_flag, &sum);   // a timeout raises the
        zt[r * 33 + o] = (m0 + r < a.M) ? (T)sum + b3s[o] : T(0);                 // MLP abort word
      }
    }
    __syncthreads();
    stamp(4);
    const bool first = s == 0;
    if (No <= 16) ce_rows_lanes<T, 16>(zt, 33, rowl, m0, a.M, No, yv, ogz, No, olpart, rb, first);
    else ce_rows_lanes<T, 32>(zt, 33, rowl, m0, a.M, No, yv, ogz, No, olpart, rb, first);
    __syncthreads();
    stamp(5);
    // layer-3 backward of the slice's columns, all operands in LDS (gz in zt, W3 slice in w3s, the
    // tile's h2 / d3 / masks): ga2 = ((gz·W3)·m2)·[h2 > 0]·m1 and its column sums (b2 partial),
    // gzᵀ·d3 (W3 partial), column sums of gz (b3 partial, slice 0)
    const int rows = min(32, a.M - m0), nm = a.n_mid;
    T* gat = &red[6][0][0];                                      // [32][33] ga2 of the tile
    for (int e = tid; e < 1024; e += MM_NT) {
      const int r = e >> 5, c = e & 31;
      T g = T(0);
      for (int o = 0; o < No; ++o) g += zt[r * 33 + o] * w3s[o * 32 + c];
      T t = g * red[5][r][c];
      t = t * (red[3][r][c] > T(0) ? T(1) : T(0));
      t = t * red[4][r][c];
      const bool ok2 = r < rows && n0 + c < nm;
      gat[r * 33 + c] = ok2 ? t : T(0);
      if (ok2 && oga2) oga2[(size_t)(m0 + r) * nm + n0 + c] = t;
    }
    __syncthreads();
    if (opb2 && tid < 32 && n0 + tid < nm) {
      T cs = T(0);
      for (int r = 0; r < rows; ++r) cs += gat[r * 33 + tid];
      opb2[(size_t)rb * nm + n0 + tid] = cs;
    }
    if (opw3)
      for (int e = tid; e < No * 32; e += MM_NT) {
        const int o = e >> 5, c = e & 31;
        if (n0 + c >= nm) continue;
        T acc = T(0);
        for (int r = 0; r < 32; ++r) acc += zt[r * 33 + o] * d3t[r * 33 + c];   // rows past M: gz = 0
        opw3[(size_t)rb * No * nm + (size_t)o * nm + n0 + c] = acc;
      }
    if (opb3 && first && tid < No) {
      T cs = T(0);
      for (int r = 0; r < rows; ++r) cs += zt[r * 33 + tid];
      opb3[(size_t)rb * No + tid] = cs;
    }
    stamp(6);
  }
  if constexpr (EPI == MM_GA1) {
    if (ocolpart) {
      __syncthreads();
      if (tid < 32 && n0 + tid < a.N) {
        T s = T(0);
        for (int r = 0; r < 32; ++r) s += red[0][r][tid];
        ocolpart[(size_t)bk.x * a.ldc + n0 + tid] = s;
      }
    }
  }
}

// amdgpu_waves_per_eu(4): two 8-wave workgroups per CU (≤ 128 registers): a batched fused launch
// (MM_L23) needs all its problems' workgroups co-resident, and at 136 registers only one fit per CU.
// Workgroups are dealt round-robin over the 8 XCDs in dispatch order (position lin of a launch plane
// whose size is a multiple of 8: XCD = lin % 8), and every XCD pulls its tiles' operands into its own
// L2.  xcd_place maps position (x, y) of a GX-wide plane to the tile it computes, or to none: xmap 1
// gives XCD k the tiles [k·P/8, (k+1)·P/8) of the gx × gy tiles in y-major order, xmap 2 the k-th
// xbx × xby block; both keep the tiles an XCD needs to few row tiles of A and few column slices of B
// (A and B tiles are both 32 × K).  xmap 0: the dispatch order itself.
template <typename T>
__device__ inline bool xcd_place(const MMArgs<T>& a, int GX, int gx, int gy, int& x, int& y) {
  if (!a.xmap) return x < gx && y < gy;
  const int lin = y * GX + x, k = lin & 7, s = lin >> 3;
  if (a.xmap == 1) {
    const int P = gx * gy, q = P >> 3, rem = P & 7;
    if (s >= q + (k < rem ? 1 : 0)) return false;
    const int t = k * q + min(k, rem) + s;
    x = t % gx;
    y = t / gx;
    return true;
  }
  if (s >= a.xbx * a.xby) return false;
  const int nbx = gx / a.xbx;
  x = (k % nbx) * a.xbx + s % a.xbx;
  y = (k / nbx) * a.xby + s / a.xbx;
  return true;
}

// A plain launch (k_mm) and a batched one (k_mmb, blockIdx.z = problem): the plain kernel keeps the
// small argument block (no problem table).
template <typename T, int EPI, int AOP, int BOP, int TA, int TB, int AV, int BV, int MK>
__global__ __launch_bounds__(MM_NT) __attribute__((amdgpu_waves_per_eu(4))) void k_mm(MMArgs<T> a) {
  __shared__ T red[MM_NW][32][33];
  __shared__ double rowl[32];
  MMProbsN<T, 1> none;
  none.n = 0;
  int x = blockIdx.x, y = blockIdx.y;
  if (a.xmap && blockIdx.z == 0 && !xcd_place(a, (int)gridDim.x, (int)gridDim.x, (int)gridDim.y, x, y)) return;
  mm_body<T, EPI, AOP, BOP, TA, TB, AV, BV, MK>(
      a, none, Blk{x, y, (int)blockIdx.z, (int)gridDim.x, (int)gridDim.y}, red, rowl);
}
template <typename T, int EPI, int AOP, int BOP, int TA, int TB, int AV, int BV, int MK>
__global__ __launch_bounds__(MM_NT) __attribute__((amdgpu_waves_per_eu(4))) void k_mmb(MMArgs<T> a, MMProbs<T> pr) {
  __shared__ T red[MM_NW][32][33];
  __shared__ double rowl[32];
  mm_body<T, EPI, AOP, BOP, TA, TB, AV, BV, MK>(
      a, pr, Blk{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, (int)gridDim.x, (int)gridDim.y}, red, rowl);
}

// Two independent launches as one: planes z < g1.z run grid 1 (g1.x × g1.y workgroups per plane, a
// batched launch with its problems), the planes after it grid 2 (a plain launch, g2.x × g2.y).  The
// launch grid is the larger of the two in x and y; workgroups outside their grid leave at once.
template <typename T, int E1, int A1, int B1, int TA1, int TB1, int AV1, int BV1,
          int E2, int A2, int B2, int TA2, int TB2, int AV2, int BV2, int MK>
__global__ __launch_bounds__(MM_NT) __attribute__((amdgpu_waves_per_eu(4)))
void k_mm2(MMArgs<T> a1, MMProbs3<T> p1, MMArgs<T> a2, int3 g1, int2 g2) {
  __shared__ T red[MM_NW][32][33];
  __shared__ double rowl[32];
  int x = blockIdx.x, y = blockIdx.y;
  const int z = blockIdx.z, GX = gridDim.x;
  if (z < g1.z) {
    // GEMM planes of grid 1 (not its pending plane) and grid 2's GEMM plane follow the XCD placement
    const bool gemm = z < (p1.n > 0 ? p1.n : 1);
    if (gemm ? xcd_place(a1, GX, g1.x, g1.y, x, y) : (x < g1.x && y < g1.y))
      mm_body<T, E1, A1, B1, TA1, TB1, AV1, BV1, MK>(a1, p1, Blk{x, y, z, g1.x, g1.y}, red, rowl);
  } else if (z == g1.z ? xcd_place(a2, GX, g2.x, g2.y, x, y) : (x < g2.x && y < g2.y)) {
    MMProbsN<T, 1> none;
    none.n = 0;
    mm_body<T, E2, A2, B2, TA2, TB2, AV2, BV2, MK>(a2, none, Blk{x, y, z - g1.z, g2.x, g2.y}, red, rowl);
  }
}

// Two batched launches as one: planes z < g1.z run batched grid 1, the next g2.z planes batched grid 2.
template <typename T, int E1, int A1, int B1, int TA1, int TB1, int AV1, int BV1,
          int E2, int A2, int B2, int TA2, int TB2, int AV2, int BV2, int MK>
__global__ __launch_bounds__(MM_NT) __attribute__((amdgpu_waves_per_eu(4)))
void k_mm2b(MMArgs<T> a1, MMProbs3<T> p1, MMArgs<T> a2, MMProbs3<T> p2, int3 g1, int3 g2) {
  __shared__ T red[MM_NW][32][33];
  __shared__ double rowl[32];
  const int x = blockIdx.x, y = blockIdx.y, z = blockIdx.z;
  if (z < g1.z) {
    if (x < g1.x && y < g1.y) mm_body<T, E1, A1, B1, TA1, TB1, AV1, BV1, MK>(a1, p1, Blk{x, y, z, g1.x, g1.y}, red, rowl);
  } else if (x < g2.x && y < g2.y) {
    mm_body<T, E2, A2, B2, TA2, TB2, AV2, BV2, MK>(a2, p2, Blk{x, y, z - g1.z, g2.x, g2.y}, red, rowl);
  }
}

// Layer 3 for n_out > 32: xw-free logits d3·W3ᵀ already stored in z; one 32-row block per
// workgroup, rows (+ b3) staged in dynamic LDS, then the same cross-entropy and layer-3 backward.
template <typename T, int MK>
__global__ __launch_bounds__(MM_NT) void k_l3_wide(MMArgs<T> a, const T* z) {
  extern __shared__ unsigned char dsm[];
  double* rowl = reinterpret_cast<double*>(dsm);
  T* scr = reinterpret_cast<T*>(dsm + 32 * sizeof(double));
  T* zt = scr + MM_NT;
  const int N = a.N, zs = N + 1, m0 = blockIdx.x * 32;
  run_pendset(a.pend, (int)blockIdx.x, (int)gridDim.x);
  for (int e = threadIdx.x; e < 32 * N; e += blockDim.x) {
    const int r = e / N, k = e - r * N;
    zt[r * zs + k] = (m0 + r < a.M) ? z[(size_t)(m0 + r) * N + k] + a.bias[k] : T(0);
  }
  __syncthreads();
  ce_rows<T>(zt, zs, rowl, m0, a.M, N, a.y, a.C, a.ldc, a.lpart, blockIdx.x);
  __syncthreads();
  l3_backward<T, MK>(a, zt, zs, m0, blockIdx.x, scr, MM_NT, 0, a.n_mid, true);
}

// ------------------------------------------------------------------ forwards by row block (k_fwdr)
// The forwards of a batched iteration (mlp.py:30-31 + the loss of :52 and its layer-3 backward), one
// workgroup per (16-row block, problem), holding ALL n_mid columns of its rows: layer 3 contracts over
// those columns, so the logits, the cross-entropy and the layer-3 backward of the block need no other
// workgroup — no cross-workgroup exchange, no co-residency requirement, and all six forwards of an
// iteration (plus the energy forwards that ride along) fit one launch.  Measured on the layer-2 GEMM
// alone (tools/microbench_fwdr.hip): 9.5 µs for six problems, flat in the problem count, against
// 8.3 µs for k_mm's 32 × 32 tiles before their exchange.
//   * h1 = max((xw + b1)·m0, 0) of the 16 rows is built once into LDS (A);
//   * wave w computes h2ᵀ for the columns n ∈ [32w, 32w + 32) over all of K = n_mid: A = W2 rows
//     (16-byte loads along k, three chunks in flight), B = h1ᵀ from LDS.  The accumulator layout (rows
//     n, columns r = lane & 15) is the B-operand layout of the layer-3 MFMA, so d3 never leaves the
//     registers: zᵀ[o][r] = Σ_n W3[o][n]·d3[r][n] is 8 more MFMAs per wave, then a fixed-order sum over
//     the waves in LDS;
//   * cross-entropy with 16 lanes per row (ce_rows_lanes' formula), then the layer-3 backward as MFMAs
//     in the same layout: ga2ᵀ = W3ᵀ·gzᵀ, the W3 partial (gzᵀ·d3)ᵀ from the d3 tile in LDS, the b2 / b3
//     partials as fixed-order sums over the block's rows.
// Partials are per 16-row block (nparts = ⌈B/16⌉).  Float32 results differ from the k_mm path by
// summation order only (K in one MFMA chain instead of split over the waves; slice partials of the
// logits summed in T instead of double).
constexpr int FR_ROWS = 16;
constexpr int FR_NW = 8;                 // waves per workgroup: n_mid ≤ 32·FR_NW
constexpr int FR_NMAX = 32 * FR_NW;
constexpr int FR_MAXP = 8;               // problems per launch: six sub-steps + E_new + E_current
template <typename T> struct RbFwdProb {
  const T* xw; const T* xw2;             // layer 1 as split-K planes: xw + xw2 (xw2 null: one plane)
  T* xwout;                              // the summed xw of the block's rows is stored here (null: not)
  const T* b1; const T* W2; const T* b2; const T* W3; const T* b3;
  MaskSrc<T> ms;
  T* ga2; T* pb2; T* pb3; T* pw3;        // outputs, null when not wanted; partials [⌈B/16⌉][…]
  double* lpart;                         // loss partial of each 16-row block (null: none)
};
template <typename T> struct RbFwdArgs {
  int M, n_mid, n_out, np;
  const int32_t* y;
  RbFwdProb<T> p[FR_MAXP];
  PendSet<T> pend;                       // pending updates: run by the extra plane blockIdx.y == np
  unsigned long long* prof;              // HMCX_FWDR_PROF: FR_NPH s_memrealtime stamps per workgroup
  // the NEXT iteration's keep flags under the default dropout ratio, drawn by the rows after the problems and the
  // pending plane (kr.nf == 0: none): they land on the CUs the problems leave free (192 + 32 workgroups on 256 CUs)
  uint32_t* keep; int n3; KeepRange kr; uint64_t seed; uint32_t chain, step;
};
constexpr int FR_NPH = 8;

template <typename T, int MK>
__global__ __launch_bounds__(FR_NW * 64) void k_fwdr(RbFwdArgs<T> a) {
  using Mf = mfma16<T>;
  constexpr int AP = FR_NMAX + 16 / (int)sizeof(T);               // pitch ≡ 4 dwords (mod 64): conflict-free
  __shared__ T At[FR_ROWS][AP];                                   // h1 tile, then the d3 tile
  __shared__ T w3s[16][FR_NMAX];                                  // W3 (rows ≥ n_out zero)
  __shared__ T zr[FR_NW][16][17];                                 // per-wave logit partials zᵀ[o][r]
  __shared__ T gzs[16][17];                                       // gz[r][o]
  __shared__ double rowl[FR_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  if ((int)blockIdx.y >= a.np + (a.pend.n > 0 ? 1 : 0)) {         // the next iteration's keep flags
    const int y0 = a.np + (a.pend.n > 0 ? 1 : 0);
    // the default ratio's law as constants: a law in scalar registers cost this kernel four more spilled SGPRs, so
    // under any other ratio the host leaves these rows out (kr.nf == 0) and draws the flags with k_mlp_keep
    keep_flags(KeepLawDefault{}, a.keep, a.n3, a.kr, a.seed, a.chain, a.step,
               ((size_t)((int)blockIdx.y - y0) * gridDim.x + blockIdx.x) * blockDim.x + tid);
    return;
  }
  if ((int)blockIdx.y == a.np) {                                  // the pending updates' plane
    run_pendset(a.pend, (int)blockIdx.x, (int)gridDim.x);
    return;
  }
  // this workgroup's problem, read through the kernel-argument segment pointer (address space 4) at a
  // uniform offset: scalar loads of ITS fields only (a.p[blockIdx.y] on the by-value argument made the
  // compiler load every problem's fields and select among them — 500+ spilled SGPRs)
  typedef __attribute__((address_space(4))) const RbFwdArgs<T> KArgs;
  KArgs* ka = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const int pb = (int)blockIdx.y;
  struct {
    const T *xw, *xw2; T *xwout; const T *b1, *W2, *b2, *W3, *b3;
    const uint32_t* keep; const T* vals; T scale; int mn;
    T *ga2, *pb2, *pb3, *pw3; double* lpart;
  } P = {ka->p[pb].xw, ka->p[pb].xw2, ka->p[pb].xwout, ka->p[pb].b1, ka->p[pb].W2, ka->p[pb].b2,
         ka->p[pb].W3, ka->p[pb].b3, ka->p[pb].ms.keep, ka->p[pb].ms.vals, ka->p[pb].ms.scale, ka->p[pb].ms.mn,
         ka->p[pb].ga2, ka->p[pb].pb2, ka->p[pb].pb3, ka->p[pb].pw3, ka->p[pb].lpart};
  const MaskSrc<T> nomask{};
  const int rb = blockIdx.x, m0 = rb * FR_ROWS, nm = a.n_mid, No = a.n_out, M = a.M;
  auto stamp = [&](int ph) {
    if (a.prof && tid == 0) a.prof[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * FR_NPH + ph] = __builtin_amdgcn_s_memrealtime();
  };
  stamp(0);
  static_assert(sizeof(T) == 4, "k_fwdr is the float32 kernel (fwdr_ok)");
  const int nwv = (nm + 31) / 32;                                  // waves with columns
  const int n0 = 32 * wave;
  const bool wact = wave < nwv;
  const int r = lr, m = m0 + r;
  const bool rok = m < M;
  const int mn = P.mn;
  // Every load of the prologue goes out before the first use (one memory round trip, not four):
  // 1. the first three 16-k chunks of this wave's W2 rows — the operand the launch waits on longest
  T bv[3][4][2];
  auto load = [&](int s, int k0) {
    load_chunk<T, OP_PLAIN, 0, 1, MK_NONE>(bv[s], P.W2, nm, n0, nm, k0, nm, lr, lg, nomask, nullptr);
  };
  load(0, 0);
  if (16 < nm) load(1, 16);
  if (32 < nm) load(2, 32);
  // 2. h1's inputs, two 4-element pieces per thread of the 16 × n_mid tile: xw, b1, the m0 mask
  constexpr int HP = FR_ROWS * FR_NMAX / 4 / (FR_NW * 64);
  float4 hx[HP], hx2[HP], hb[HP], hv4[HP];
  uint32_t hk[HP];
  size_t hbase[HP];
#pragma unroll
  for (int h = 0; h < HP; ++h) {
    const int e = tid + h * FR_NW * 64, rr = e / (nm / 4), c = (e % (nm / 4)) * 4, mm = m0 + rr;
    const bool ok = e < FR_ROWS * nm / 4 && mm < M;
    const size_t base = ok ? (size_t)mm * nm + c : 0;
    hbase[h] = base;
    hx[h] = *reinterpret_cast<const float4*>(P.xw + base);
    hx2[h] = *reinterpret_cast<const float4*>((P.xw2 ? P.xw2 : P.xw) + base);
    hb[h] = *reinterpret_cast<const float4*>(P.b1 + (ok ? c : 0));
    if constexpr (MK == MK_KEEP) hk[h] = P.keep[base >> 5];
    if constexpr (MK == MK_VALS) hv4[h] = *reinterpret_cast<const float4*>(P.vals + base);
  }
  // 3. W3, two 4-column pieces per thread (rows o ≥ n_out: zero)
  float4 w3v[HP];
#pragma unroll
  for (int h = 0; h < HP; ++h) {
    const int e = tid + h * FR_NW * 64, o = e / (FR_NMAX / 4), c = (e % (FR_NMAX / 4)) * 4;
    const bool ok = o < No && c < nm;
    w3v[h] = *reinterpret_cast<const float4*>(P.W3 + (ok ? (size_t)o * nm + c : 0));
  }
  // 4. the epilogue's operands for this lane's 8 elements (r = lr, n = n0 + 16j + 4·lg + q): b2, the
  //    m1 / m2 masks (one keep word or one 16-byte vector each); the labels and b3 of the cross-entropy
  float4 b2v[2], m1v4[2], m2v4[2];
  uint32_t k1[2], k2[2];
  size_t ebase[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + 16 * j + 4 * lg;
    const bool ok = rok && n < nm;
    const size_t e = ok ? (size_t)m * nm + n : 0;
    ebase[j] = e;
    b2v[j] = *reinterpret_cast<const float4*>(P.b2 + (ok ? n : 0));
    if constexpr (MK == MK_KEEP) {
      k1[j] = P.keep[((size_t)mn + e) >> 5];
      k2[j] = P.keep[((size_t)2 * mn + e) >> 5];
    }
    if constexpr (MK == MK_VALS) {
      m1v4[j] = *reinterpret_cast<const float4*>(P.vals + (size_t)mn + e);
      m2v4[j] = *reinterpret_cast<const float4*>(P.vals + (size_t)2 * mn + e);
    }
  }
  const int32_t yv = a.y[min(m0 + (tid >> 4), M - 1)];
  const T b3v = P.b3[min(tid & 15, No - 1)];
  // h1 = max((xw + b1)·m0, 0) (mlp.py:30) and W3 into LDS
  // the mask value of flag q of a 4-element piece at element e: one bit of a keep word (bit e % 32 + q)
  auto mbit = [&](uint32_t w, size_t e, int q) {
    return ((w >> (uint32_t)((e & 31) + q)) & 1u) ? P.scale : T(0);
  };
#pragma unroll
  for (int h = 0; h < HP; ++h) {
    const int e = tid + h * FR_NW * 64, rr = e / (nm / 4), c = (e % (nm / 4)) * 4;
    if (e < FR_ROWS * nm / 4) {
      const bool ok = m0 + rr < M;
      if (P.xw2) {                                             // the two split-K planes, in plane order
        hx[h].x += hx2[h].x; hx[h].y += hx2[h].y; hx[h].z += hx2[h].z; hx[h].w += hx2[h].w;
        if (P.xwout && ok) *reinterpret_cast<float4*>(P.xwout + hbase[h]) = hx[h];
      }
      const T x[4] = {hx[h].x, hx[h].y, hx[h].z, hx[h].w}, bb[4] = {hb[h].x, hb[h].y, hb[h].z, hb[h].w};
      const T vv[4] = {hv4[h].x, hv4[h].y, hv4[h].z, hv4[h].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        T mk = T(1);
        if constexpr (MK == MK_KEEP) mk = mbit(hk[h], hbase[h], q);
        if constexpr (MK == MK_VALS) mk = vv[q];
        At[rr][c + q] = ok ? op_apply<T, OP_H1>(x[q], mk, bb[q]) : T(0);
      }
    }
    const int o = e / (FR_NMAX / 4), c3 = (e % (FR_NMAX / 4)) * 4;
    const bool ok3 = o < No && c3 < nm;
    *reinterpret_cast<float4*>(&w3s[o][c3]) = ok3 ? w3v[h] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  stamp(1);
  __syncthreads();
  stamp(2);
  // layer 2, transposed: acc[j] = h2ᵀ[n0 + 16j + row][r] over all of K = n_mid; A = W2 rows (the ring),
  // B = h1ᵀ from LDS (16-byte reads)
  typename Mf::acc_t acc[2] = {Mf::zero(), Mf::zero()};
  if (wact) {
    auto mf = [&](int s, int k0) {
      const float4 w = *reinterpret_cast<const float4*>(&At[lr][k0 + 4 * lg]);
      const T hv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = Mf::fma(bv[s][u][j], hv[u], acc[j]);
    };
    for (int k0 = 0; k0 < nm; k0 += 48) {
      mf(0, k0);
      if (k0 + 48 < nm) load(0, k0 + 48);
      if (k0 + 16 < nm) {
        mf(1, k0 + 16);
        if (k0 + 64 < nm) load(1, k0 + 64);
      }
      if (k0 + 32 < nm) {
        mf(2, k0 + 32);
        if (k0 + 80 < nm) load(2, k0 + 80);
      }
    }
  }
  stamp(3);
  // h2 = max((z2 + b2)·m1, 0), d3 = h2·m2 (mlp.py:30-31), kept in registers
  T dv[2][4], hp[2][4], m1v[2][4], m2v[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const T b2q[4] = {b2v[j].x, b2v[j].y, b2v[j].z, b2v[j].w};
    const T v1[4] = {m1v4[j].x, m1v4[j].y, m1v4[j].z, m1v4[j].w}, v2[4] = {m2v4[j].x, m2v4[j].y, m2v4[j].z, m2v4[j].w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + 16 * j + Mf::row(lane, q);
      const bool ok = rok && n < nm;
      m1v[j][q] = m2v[j][q] = T(1);
      if constexpr (MK == MK_KEEP) {
        m1v[j][q] = mbit(k1[j], (size_t)mn + ebase[j], q);
        m2v[j][q] = mbit(k2[j], (size_t)2 * mn + ebase[j], q);
      }
      if constexpr (MK == MK_VALS) {
        m1v[j][q] = v1[q];
        m2v[j][q] = v2[q];
      }
      const T t = (acc[j][q] + b2q[q]) * m1v[j][q];
      const T h = t > T(0) ? t : T(0);
      hp[j][q] = h > T(0) ? T(1) : T(0);
      dv[j][q] = ok ? h * m2v[j][q] : T(0);
    }
  }
  __syncthreads();                                                 // every wave is done with the h1 tile
  stamp(4);
  // layer 3: zᵀ[o][r] = Σ_n W3[o][n]·d3[r][n] over this wave's columns (k index n = n0 + 16j + row(u))
  {
    typename Mf::acc_t za = Mf::zero();
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = n0 + 16 * j + Mf::row(lane, u);
        za = Mf::fma(w3s[lr][min(n, FR_NMAX - 1)], dv[j][u], za);
        At[r][min(n, FR_NMAX - 1)] = dv[j][u];                     // the d3 tile, for the W3 partial
      }
#pragma unroll
    for (int q = 0; q < 4; ++q) zr[wave][Mf::row(lane, q)][lr] = za[q];
  }
  __syncthreads();
  stamp(5);
  // cross-entropy of the block's rows, 16 lanes per row (F.softmax_cross_entropy, mean over M)
  if (tid < 256) {
    const int rr = tid >> 4, k = tid & 15, mm = m0 + rr;
    const bool kin = k < No;
    T z = zr[0][k][rr];
    for (int w = 1; w < nwv; ++w) z += zr[w][k][rr];
    z = kin ? z + b3v : T(0);
    T mx = kin ? z : -INFINITY;
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1) {                               // NaN propagates as in np.max
      const T o = __shfl_xor(mx, w, 16);
      mx = (o > mx || o != o) ? o : mx;
    }
    T e = kin ? exp(z - mx) : T(0);
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1) e += __shfl_xor(e, w, 16);
    const T ls = log(e);
    double l = (kin && k == yv && mm < M) ? -(double)((z - mx) - ls) : 0.0;
    T g = T(0);
    if (kin && mm < M) {
      g = exp((z - mx) - ls);
      if (k == yv) g -= T(1);
      g = g / (T)M;
    }
    gzs[rr][k] = g;
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1) l += __shfl_xor(l, w, 16);
    if (k == 0) rowl[rr] = l;
  }
  __syncthreads();
  stamp(6);
  if (tid == 0 && P.lpart) {
    double s = 0.0;
    for (int q = 0; q < FR_ROWS; ++q) s += rowl[q];
    P.lpart[rb] = s;
  }
  if (P.pb3 && tid < No) {                                           // b3 partial: Σ_rows gz
    T cs = T(0);
    for (int q = 0; q < FR_ROWS; ++q) cs += gzs[q][tid];
    P.pb3[(size_t)rb * No + tid] = cs;
  }
  if (!wact) return;
  // layer-3 backward (k index o = 4·lg + u < 16): ga2ᵀ[n][r] = Σ_o W3[o][n]·gz[r][o], then
  // ga2 = ((·)·m2)·[h2 > 0]·m1 in the layer-2 accumulator layout
  if (P.ga2 || P.pb2) {
    typename Mf::acc_t ga[2] = {Mf::zero(), Mf::zero()};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = 4 * lg + u;
      const T gzv = gzs[lr][o];
#pragma unroll
      for (int j = 0; j < 2; ++j) ga[j] = Mf::fma(w3s[o][min(n0 + 16 * j + lr, FR_NMAX - 1)], gzv, ga[j]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      T gv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        T t = ga[j][q] * m2v[j][q];
        t = t * hp[j][q];
        t = t * m1v[j][q];
        const int n = n0 + 16 * j + Mf::row(lane, q);
        gv[q] = (rok && n < nm) ? t : T(0);
      }
      if (P.ga2 && rok) {
        if constexpr (sizeof(T) == 4) {                              // rows 4·lg … 4·lg + 3: one float4
          const int n = n0 + 16 * j + 4 * lg;
          if (n < nm) *reinterpret_cast<float4*>(P.ga2 + (size_t)m * nm + n) = make_float4(gv[0], gv[1], gv[2], gv[3]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int n = n0 + 16 * j + Mf::row(lane, q);
            if (n < nm) P.ga2[(size_t)m * nm + n] = gv[q];
          }
        }
      }
      if (P.pb2) {                                                   // b2 partial: Σ over the block's rows
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          T s = gv[q];
#pragma unroll
          for (int w = 1; w < 16; w <<= 1) s += __shfl_xor(s, w, 16);
          const int n = n0 + 16 * j + Mf::row(lane, q);
          if (lr == 0 && n < nm) P.pb2[(size_t)rb * nm + n] = s;
        }
      }
    }
  }
  // W3 partial: pw3ᵀ[n][o] = Σ_r d3[r][n]·gz[r][o] over the block's rows (k index r = 4·lg + u)
  if (P.pw3) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      typename Mf::acc_t pw = Mf::zero();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rk = 4 * lg + u;
        pw = Mf::fma(At[rk][min(n0 + 16 * j + lr, FR_NMAX - 1)], gzs[rk][lr], pw);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + 16 * j + Mf::row(lane, q);
        if (lr < No && n < nm) P.pw3[(size_t)rb * No * nm + (size_t)lr * nm + n] = pw[q];
      }
    }
  }
  stamp(7);
}

// Mask values of one forward (the API twin of the sampler's keep flags: same groups, value = keep·law.scale).
// Thread g: group g (64 elements), written as 16-byte vectors.
template <typename T>
__device__ inline void mlp_masks_group(const DropLaw<T>& law, T* masks, int n3, uint64_t seed, uint32_t chain, uint32_t step,
                                       uint32_t slot, int g) {
  if (64 * g >= n3) return;
  const KeepGroup k = keep_group(law.keep, seed, (uint32_t)g, slot, step, chain);
  const T scale = law.scale;
  constexpr int V = 16 / sizeof(T);
  typedef T tv __attribute__((ext_vector_type(V)));
  const int e0 = 64 * g, n = min(64, n3 - e0);
  for (int p = 0; p < 64; p += V) {
    tv v;
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = (((p + q < 32 ? k.lo >> (p + q) : k.hi >> (p + q - 32)) & 1u) ? scale : T(0));
    if (p + V <= n && (reinterpret_cast<uintptr_t>(masks + e0 + p) & 15) == 0) {
      *reinterpret_cast<tv*>(masks + e0 + p) = v;
    } else {
#pragma unroll
      for (int q = 0; q < V; ++q)
        if (p + q < n) masks[e0 + p + q] = v[q];
    }
  }
}
template <typename T>
__global__ void k_mlp_masks(DropLaw<T> law, T* masks, int n3, uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot) {
  mlp_masks_group<T>(law, masks, n3, seed, chain, step, slot, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

// The kicks and the drift between two gradient calls of the full-batch trajectory in one launch
// (mlp_leapfrog_t; each row the per-element arithmetic of k_axpy, hmc.py:50-53): row 0 the previous
// sub-step's second kick p_u −= ε·g_u, row 1 the next sub-step's first kick and drift p_v −= (ε/2)·g_v,
// q_v += ε·p_v, row 2 the next gradient call's dropout masks (hmcx_mlp_masks).  u ≠ v always (consecutive
// variables of the order), so the rows touch disjoint memory.  A bias / W3 gradient the kick reads may still
// be pending (its row-block partials, UPD_GRAD): the row computes it element by element first (k_pending's
// arithmetic, the same thread reads back g[i]) — no k_pending launch of its own.
template <typename T> struct MlpKicks {
  T* pu; const T* gu; int64_t nu; T eu;
  T* pv; const T* gv; T* qv; int64_t nv; T hv, ev;
  T* masks; int n3; uint64_t seed; uint32_t chain, step, slot;   // masks null: no draw
  DropLaw<T> law;
  PendSet<T> ps;
};
template <typename T> __device__ inline int pend_of(const PendSet<T>& ps, const T* g) {
  int pj = -1;
#pragma unroll
  for (int j = 0; j < MAXPEND; ++j)
    if (j < ps.n && ps.p[j].mode == UPD_GRAD && ps.p[j].u.G == g) pj = j;
  return pj;
}
template <typename T>
__global__ __launch_bounds__(256) void k_mlp_kicks(MlpKicks<T> k) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, st = (int64_t)gridDim.x * 256;
  if (blockIdx.y == 0) {
    const int pj = pend_of(k.ps, k.gu);
    for (int64_t i = i0; i < k.nu; i += st) {
      if (pj >= 0) pending_elem(k.ps.p[pj], (int)i);
      const T ax = k.eu * k.gu[i];
      k.pu[i] = k.pu[i] - ax;
    }
  } else if (blockIdx.y == 1) {
    const int pj = pend_of(k.ps, k.gv);
    for (int64_t i = i0; i < k.nv; i += st) {
      if (pj >= 0) pending_elem(k.ps.p[pj], (int)i);
      const T ax = k.hv * k.gv[i];
      const T p = k.pv[i] - ax;
      k.pv[i] = p;
      const T aq = k.ev * p;
      k.qv[i] = k.qv[i] + aq;
    }
  } else if (k.masks) {
    for (int64_t g = i0; 64 * g < k.n3; g += st) mlp_masks_group<T>(k.law, k.masks, k.n3, k.seed, k.chain, k.step, k.slot, (int)g);
  }
}
// p = −p of the six variables (hmc.py:55-56, k_axpy's p − 2·p), one launch (row = variable)
template <typename T> struct Neg6 { T* p[6]; int64_t n[6]; };
template <typename T>
__global__ __launch_bounds__(256) void k_mlp_neg6(Neg6<T> a) {
  T* p = a.p[blockIdx.y];
  const T two = T(2);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n[blockIdx.y]; i += (int64_t)gridDim.x * 256) {
    const T ax = two * p[i];
    p[i] = p[i] - ax;
  }
}

template <typename T>
__global__ void k_bias_into_z(T* z, const T* b, int n, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = z[i] + b[i % N];
}

// Six variables in the caller's order (position i of `order`).
struct VarTab {
  void* q[6]; void* qn[6]; void* p[6];
  void* qc[6];                 // step start: the previous step's proposal, committed here if accepted
  int n[6], e0[6];
};

__device__ inline void block_sum2(double a, double b, double* out_a, double* out_b) {
  __shared__ double sa[256], sb[256];
  const int t = threadIdx.x;
  sa[t] = a;
  sb[t] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) { sa[t] += sa[t + w]; sb[t] += sb[t + w]; }
    __syncthreads();
  }
  if (t == 0) { *out_a = sa[0]; if (out_b) *out_b = sb[0]; }
}

// Blocks of grid.x that work on a variable of n elements (≈ 4 per thread): W1 (200,704 at config 3)
// gets 196 blocks instead of a fixed 32, so no thread walks a long serial chain of loads and Philox
// draws (k_mlp_init: 12.9 → 7.1 µs per step).  The other blocks only write zero partials.
__device__ inline int var_blocks(int n) { return min(NPART, max(1, (n + 1023) / 1024)); }

// Momentum draw (hmc.py:82-87) + first drift q' = q + ε·p + partials of Σp², Σq² (part [2][6][NPART]).
// With prev_acc set, the previous step's commit happens here first (state ← proposal where it was
// accepted, hmc.py:75-79): one launch less per step.
template <typename T>
__device__ inline void init_block(const VarTab& vt, T eps, int drift, int noise_mode, const double* noise,
                                  uint64_t seed, uint32_t chain, uint32_t step, double* part, int v, int bx,
                                  const int32_t* prev_acc) {
  const int n = vt.n[v];
  T* const qw = (T*)vt.q[v];
  const bool take = prev_acc != nullptr && vt.qc[v] != nullptr && *prev_acc != 0;   // uniform
  const T* q = take ? (const T*)vt.qc[v] : qw;
  T* qn = (T*)vt.qn[v];
  T* p = (T*)vt.p[v];
  const int nb = var_blocks(n);
  if (bx >= nb) {                                              // block-uniform
    if (threadIdx.x == 0) { part[v * NPART + bx] = 0.0; part[(6 + v) * NPART + bx] = 0.0; }
    return;
  }
  double sp = 0.0, sq = 0.0;
  for (int i = bx * 256 + threadIdx.x; i < n; i += nb * 256) {
    const uint32_t e = (uint32_t)(vt.e0[v] + i);
    const T z = noise_mode == HMCX_NOISE_BUFFER ? (T)noise[e] : philox_normal_t<T>(seed, chain, step, 0u, e);
    const T qv = q[i];
    if (take) qw[i] = qv;
    p[i] = z;
    if (drift) qn[i] = qv + eps * z;
    sp += (double)z * (double)z;
    sq += (double)qv * (double)qv;
  }
  block_sum2(sp, sq, part + v * NPART + bx, part + (6 + v) * NPART + bx);
}
template <typename T>
__global__ __launch_bounds__(256) void k_mlp_init(VarTab vt, T eps, int drift, int noise_mode, const double* noise,
                                                  uint64_t seed, uint32_t chain, uint32_t step, double* part,
                                                  const int32_t* prev_acc) {
  init_block<T>(vt, eps, drift, noise_mode, noise, seed, chain, step, part, (int)blockIdx.y, (int)blockIdx.x, prev_acc);
}
// Step start in one launch: rows y < 6 draw the momentum of variable y and the first drift (k_mlp_init),
// rows y ≥ 6 the keep flags of the step's nf forwards (keep_flags; work item (y − 6, x, thread) in
// row-major order) — independent work, one launch less per step.  grid.x = NPART.
template <typename T>
__global__ __launch_bounds__(256) void k_mlp_start(VarTab vt, T eps, int drift, int noise_mode, const double* noise,
                                                   uint64_t seed, uint32_t chain, uint32_t step, double* part,
                                                   const int32_t* prev_acc, uint32_t* keep, int n3, KeepRange kr,
                                                   KeepLaw law) {
  if (blockIdx.y < 6) {
    init_block<T>(vt, eps, drift, noise_mode, noise, seed, chain, step, part, (int)blockIdx.y, (int)blockIdx.x,
                  prev_acc);
  } else {
    keep_flags(law, keep, n3, kr, seed, chain, step, ((size_t)(blockIdx.y - 6) * NPART + blockIdx.x) * 256 + threadIdx.x);
  }
}

// End-of-trajectory partials: part[0][i] = Σp², part[1][i] = Σq² per variable (same layout as init).
template <typename T>
__global__ __launch_bounds__(256) void k_sumsq12(VarTab vt, double* part) {
  const int v = blockIdx.y, n = vt.n[v];
  const T* q = (const T*)vt.q[v];
  const T* p = (const T*)vt.p[v];
  const int nb = var_blocks(n);
  if ((int)blockIdx.x >= nb) {
    if (threadIdx.x == 0) { part[v * NPART + blockIdx.x] = 0.0; part[(6 + v) * NPART + blockIdx.x] = 0.0; }
    return;
  }
  double sp = 0.0, sq = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += nb * 256) {
    const double pv = (double)p[i], qv = (double)q[i];
    sp += pv * pv;
    sq += qv * qv;
  }
  block_sum2(sp, sq, part + v * NPART + blockIdx.x, part + (6 + v) * NPART + blockIdx.x);
}


// state ← proposal where accepted
template <typename T>
__global__ void k_mlp_commit(VarTab vt, const int32_t* acc) {
  const int v = blockIdx.y, n = vt.n[v];
  if (!*acc || vt.q[v] == vt.qn[v]) return;
  const T* src = (const T*)vt.q[v];
  T* dst = (T*)vt.qn[v];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = src[i];
}

}  // namespace hmcx
