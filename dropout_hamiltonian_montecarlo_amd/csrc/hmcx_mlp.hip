// hmcx_mlp.hip — the reference's dropout MLP (config 3) on gfx950: gradient, loss and fused SGHMC.
//
// Reference: hamiltonian/models/gpu/mlp.py:19-31 (MyNetwork: relu(dropout(l1 x)) → relu(dropout(l2 ·))
// → l3(dropout(·)), dropout ratio 0.1 in train mode) and :47-82 (grad = ∇ mean softmax-CE + ½αθ,
// log_likelihood returns the mean CE, nlp = loss + log_prior).  Chainer/CuPy are not available, so
// the arithmetic follows the NumPy restatement in oracle/models.py::mlp (parity with injected masks).
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
//  * Batched iterations (mlp_sghmc_t): the six sub-steps of a leapfrog iteration only depend on the
//    previous iteration, so their kernels go out as multi-problem launches (k_mmb, blockIdx.z = sub-step)
//    and one dual launch (k_mm2: layer-1 backwards + W2 gradient); ≈1.0 GFLOP per iteration at
//    784-256-256-10, B = 500 (layer 1 runs once, after W1 moved), 5 launches per iteration (11 one
//    sub-step at a time).
//  * Chains as problems (mlp_sgld_chains_t): several SGLD chains on shared minibatches run the one-chain
//    schedule with every launch widened over a group of up to MAXPROB chains — k_mmc (k_mmb with a problem
//    table that also carries the buffers a chain owns), k_pending_chains, k_mlp_sgld_chains; compiled in
//    units of their own (HMCX_MLP_CHAINS_UNIT).
#include "hmcx_common.h"
#include "hmcx_internal.h"
#include "hmcx_granule.h"
#include "hmcx_mlp_mask.h"
#include <type_traits>
#include <algorithm>
#include <vector>
#include <cstring>

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
// Chains as problems (blockIdx.z = chain of the launch group): k_mmb with the chain problem table.  The same
// mm_body — tiles, K split over the waves, combine order — as the one-chain launch of the same EPI, so a chain's
// result is the one-chain result bit for bit.
template <typename T, int EPI, int AOP, int BOP, int TA, int TB, int AV, int BV, int MK>
__global__ __launch_bounds__(MM_NT) __attribute__((amdgpu_waves_per_eu(4))) void k_mmc(MMArgs<T> a, MMChains<T> pr) {
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
  // the NEXT iteration's keep flags, drawn by the rows after the problems and the pending plane (kr.nf == 0:
  // none): they land on the CUs the problems leave free (192 + 32 workgroups on 256 CUs)
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
    keep_flags(a.keep, a.n3, a.kr, a.seed, a.chain, a.step,
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

// Mask values of one forward (the API twin of the sampler's keep flags: same groups, value = keep·(1/0.9)).
// Thread g: group g (64 elements), written as 16-byte vectors.
template <typename T>
__device__ inline void mlp_masks_group(T* masks, int n3, uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot,
                                       int g) {
  if (64 * g >= n3) return;
  const KeepGroup k = keep_group(seed, (uint32_t)g, slot, step, chain);
  const T scale = (T)(1.0 / 0.9);
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
__global__ void k_mlp_masks(T* masks, int n3, uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot) {
  mlp_masks_group<T>(masks, n3, seed, chain, step, slot, (int)(blockIdx.x * blockDim.x + threadIdx.x));
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
    for (int64_t g = i0; 64 * g < k.n3; g += st) mlp_masks_group<T>(k.masks, k.n3, k.seed, k.chain, k.step, k.slot, (int)g);
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
                                                   const int32_t* prev_acc, uint32_t* keep, int n3, KeepRange kr) {
  if (blockIdx.y < 6) {
    init_block<T>(vt, eps, drift, noise_mode, noise, seed, chain, step, part, (int)blockIdx.y, (int)blockIdx.x,
                  prev_acc);
  } else {
    keep_flags(keep, n3, kr, seed, chain, step, ((size_t)(blockIdx.y - 6) * NPART + blockIdx.x) * 256 + threadIdx.x);
  }
}
// The keep flags alone (the forwards a k_fwdr step left undrawn when it falls back to the k_mm forwards).
static __global__ __launch_bounds__(256) void k_mlp_keep(uint32_t* keep, int n3, KeepRange kr, uint64_t seed, uint32_t chain,
                                                  uint32_t step) {
  keep_flags(keep, n3, kr, seed, chain, step, (size_t)blockIdx.x * 256 + threadIdx.x);
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

// MH accept (hmc.py:67-79): E = nlp + ½Σp², nlp = loss + log_prior, log_prior = −Σ_v ½α·Σθ²/dim.
struct MlpAccept {
  const double* part_cur; const double* part_new;   // [2][6][NPART]
  const double* lp_cur; const double* lp_new;       // loss partials [nlb_cur] / [nlb_new]
  int nlb_cur, nlb_new, B;
  int dim[6];
  double alpha, u;
  double* out_A; int32_t* out_acc; double* out_loss; double* out_nlp; double* out_E;
  int32_t* acc_flag;
};
// One workgroup of 26 × 32 threads: group g < 24 sums the NPART partials of (state g/12, kind, variable),
// groups 24/25 the loss partials of the current / proposed state — each lane a fixed-order strided
// sum, then a fixed-order tree.
static __global__ __launch_bounds__(1024) void k_mlp_accept(MlpAccept a) {
  __shared__ double sh[26][32];
  const int t = threadIdx.x, g = t >> 5, j = t & 31;
  double x = 0.0;
  if (g < 24) {
    const double* pp = (g < 12 ? a.part_cur : a.part_new) + (g % 12) * NPART;
    for (int q = 0; q < NPART / 32; ++q) x += pp[q * 32 + j];
  } else if (g < 26) {
    const double* lp = g == 24 ? a.lp_cur : a.lp_new;
    const int nb = g == 24 ? a.nlb_cur : a.nlb_new;
    for (int b = j; b < nb; b += 32) x += lp[b];
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
  for (int v = 0; v < 6; ++v) {                                // variables in the caller's order
    pri_c -= 0.5 * a.alpha * sh[6 + v][0] / (double)a.dim[v];
    pri_n -= 0.5 * a.alpha * sh[18 + v][0] / (double)a.dim[v];
    kc += 0.5 * sh[v][0];
    kn += 0.5 * sh[12 + v][0];
  }
  const double Enew = (ln + pri_n) + kn;
  const double Ecur = (lc + pri_c) + kc;
  const double e = exp(Ecur - Enew);
  const double A = (e < 1.0) ? e : 1.0;                       // Python min(1, x)
  const int acc = (A == A) && (A - A == 0.0) && a.u < A;      // isfinite(A) and u < A
  *a.out_A = A;
  *a.out_acc = acc;
  *a.out_loss = acc ? ln : lc;
  if (a.out_nlp) *a.out_nlp = acc ? (ln + pri_n) : (lc + pri_c);
  if (a.out_E) { a.out_E[0] = Ecur; a.out_E[1] = Enew; }
  *a.acc_flag = acc;
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

static __global__ void k_loss_final(const double* lpart, int nlb, int B, double* out) {
  double s = 0.0;
  for (int b = 0; b < nlb; ++b) s += lpart[b];
  *out = s / (double)B;
}

// One momentum-SGD step on all six variables (sgd.py:40-41; hmcx_mlp_sgd_run), grid (NPART, 6 + extra rows):
// row v < 6, with k_mlp_init's var_blocks partition: m = γ·m − η·g, θ = θ + m (each product and sum rounded
// once, the NumPy expression), and the block's float64 partial of Σθ² of the updated θ (part [6][NPART],
// zeros from the idle blocks).  The rows after them hold independent work on the CUs the update leaves free, as
// k_mlp_start's keep-flag rows do: their first workgroup finalises the step's loss from the gradient forward's
// row-block partials (k_loss_final's arithmetic), every later one draws 256 groups of the NEXT step's dropout
// masks (hmcx_mlp_masks's values) into the scratch the step just finished reading.
template <typename T> struct MlpSgd {
  VarTab vt;                          // q: θ, p: momentum, qn: the step's gradient; canonical order
  T gamma, lr;
  double* part;
  const double* lpart; int nlb, B; double* out_loss;               // out_loss null: no loss
  T* masks; int n3; uint64_t seed; uint32_t chain, step, slot;     // masks null: no draw
};
template <typename T>
__global__ __launch_bounds__(256) void k_mlp_sgd(MlpSgd<T> a) {
  if (blockIdx.y >= 6) {
    const size_t lb = (size_t)(blockIdx.y - 6) * NPART + blockIdx.x;
    if (lb == 0) {
      if (a.out_loss && threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < a.nlb; ++b) s += a.lpart[b];
        *a.out_loss = s / (double)a.B;
      }
    } else if (a.masks) {
      const size_t g = (lb - 1) * 256 + threadIdx.x;
      if (g * 64 < (size_t)a.n3) mlp_masks_group<T>(a.masks, a.n3, a.seed, a.chain, a.step, a.slot, (int)g);
    }
    return;
  }
  const int v = blockIdx.y, n = a.vt.n[v], bx = blockIdx.x;
  const int nb = var_blocks(n);
  if (bx >= nb) {                                              // block-uniform
    if (threadIdx.x == 0) a.part[v * NPART + bx] = 0.0;
    return;
  }
  T* q = (T*)a.vt.q[v];
  T* p = (T*)a.vt.p[v];
  const T* g = (const T*)a.vt.qn[v];
  double sq = 0.0;
  for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < n; i += (int64_t)nb * 256) {
    const T ax = a.lr * g[i];
    const T m = a.gamma * p[i] - ax;
    p[i] = m;
    const T qv = q[i] + m;
    q[i] = qv;
    sq += (double)qv * (double)qv;
  }
  block_sum2(sq, 0.0, a.part + v * NPART + bx, nullptr);
}
// The evaluation after a marked step: thread 0 the mean CE of the evaluation forward (k_loss_final's
// arithmetic), threads 1..6 Σθ² of variable t − 1 from k_mlp_sgd's partials, in block order.
static __global__ void k_mlp_sgd_eval(const double* lpart, int nlb, int B, const double* part, double* out_loss,
                                      double* out_sumsq) {
  const int t = threadIdx.x;
  if (t == 0) {
    double s = 0.0;
    for (int b = 0; b < nlb; ++b) s += lpart[b];
    *out_loss = s / (double)B;
  } else if (t <= 6 && out_sumsq) {
    double s = 0.0;
    for (int b = 0; b < NPART; ++b) s += part[(t - 1) * NPART + b];
    out_sumsq[t - 1] = s;
  }
}

// One SGLD step on all six variables (cpu/sgld.py:31-46, gpu/sgld.py:11-26; hmcx_mlp_sgld_run), grid
// (NPART, 6 + extra rows) laid out as k_mlp_sgd's: row v < 6 (canonical variable v, var_blocks partition)
// draws or reads the element's standard normal z and applies the variant's update, every product and sum
// rounded once in T:
//   variant 0:  p = (2ε)·z;  p = p + (−½ε)·g;  θ = θ + p
//   variant 1:  p = ((2ε)·z)·p_prev − (½ε)·g;  θ = θ + p;  p stored
// then stores θ into the step's draw slot (vt.qc[v], null: not a kept step) and writes the block's float64
// partial of Σθ² (part [6][NPART], zeros from the idle blocks).  The noise is indexed by e = e0[v] + i, the
// variable's offset in the caller's order plus the index.  A thread takes whole Philox blocks — the four
// consecutive e of one float block (philox_normal4), the two of one double block (philox_pair_d): one Philox
// call per block, the values philox_normal_t<T> gives each e — so a variable's first and last block may be
// shared with its neighbours in the layout: the elements outside [0, n) are skipped.  BUFFER noise walks the
// same groups.  The spare rows are k_mlp_sgd's: the step's loss and the NEXT step's dropout masks.
__device__ inline void sgld_normals(uint64_t seed, uint32_t chain, uint32_t step, uint32_t blk, float (&z)[4]) {
  philox_normal4(seed, chain, step, 0u, blk, z);
}
__device__ inline void sgld_normals(uint64_t seed, uint32_t chain, uint32_t step, uint32_t blk, double (&z)[2]) {
  philox_pair_d(seed, chain, step, 0u, blk, z[0], z[1]);
}
template <typename T> struct MlpSgld {
  VarTab vt;                          // q: θ, p: momentum (variant 1), qn: gradient, qc: draw slot; canonical order
  T two_eps, half_eps;                // (T)(2ε); variant 0: (T)(−½ε), variant 1: (T)(½ε)
  int variant, noise_mode;
  const double* noise;                // BUFFER: the step's P normals
  uint64_t seed; uint32_t chain, step;
  double* part;
  const double* lpart; int nlb, B; double* out_loss;               // out_loss null: no loss
  T* masks; int n3; uint32_t mstep, slot;                          // masks null: no draw
};
// Several chains (k_mlp_sgld_chains, blockIdx.z = chain c of the launch group): `a` describes the group's first
// chain and chain c lies at fixed strides behind it — θ, momentum and gradient [c][n_v], the draw slot
// [c·draw][n_v] (draw = the caller's draws per chain), the Σθ² partials [c][6][NPART], the loss partials [c][nlb],
// out_loss [c] and the mask scratch [c][masks] — under Philox chain a.chain + c.
struct SgldStrides { int64_t draw, masks; };
template <typename T>
__global__ __launch_bounds__(256) void k_mlp_sgld_chains(MlpSgld<T> a, SgldStrides cs) {
  const int c = blockIdx.z;
  const uint32_t chain = a.chain + (uint32_t)c;
  double* const part = a.part + (size_t)c * 6 * NPART;
  if (blockIdx.y >= 6) {
    const size_t lb = (size_t)(blockIdx.y - 6) * NPART + blockIdx.x;
    if (lb == 0) {
      if (a.out_loss && threadIdx.x == 0) {
        const double* lpart = a.lpart + (size_t)c * a.nlb;
        double s = 0.0;
        for (int b = 0; b < a.nlb; ++b) s += lpart[b];
        a.out_loss[c] = s / (double)a.B;
      }
    } else if (a.masks) {
      const size_t g = (lb - 1) * 256 + threadIdx.x;
      T* const masks = a.masks + (size_t)c * cs.masks;
      if (g * 64 < (size_t)a.n3) mlp_masks_group<T>(masks, a.n3, a.seed, chain, a.mstep, a.slot, (int)g);
    }
    return;
  }
  const int v = blockIdx.y, n = a.vt.n[v], bx = blockIdx.x;
  const int nb = var_blocks(n);
  if (bx >= nb) {                                              // block-uniform
    if (threadIdx.x == 0) part[v * NPART + bx] = 0.0;
    return;
  }
  T* q = (T*)a.vt.q[v];
  T* p = (T*)a.vt.p[v];
  T* draw = (T*)a.vt.qc[v];
  const T* g = (const T*)a.vt.qn[v];
  const size_t off = (size_t)c * (size_t)n;
  q += off;
  if (p) p += off;
  g += off;
  if (draw) draw += (size_t)c * (size_t)cs.draw * (size_t)n;
  const int e0 = a.vt.e0[v];                                   // e0 + n ≤ P < 2^31 (the host's int offsets)
  constexpr int G = sizeof(T) == 4 ? 4 : 2;                    // normals per Philox block
  const int blk0 = e0 / G, nblk = (int)(((int64_t)e0 + n + G - 1) / G) - blk0;   // blocks holding an element of v
  const bool philox = a.noise_mode == HMCX_NOISE_PHILOX;
  double sq = 0.0;
  for (int b = bx * 256 + (int)threadIdx.x; b < nblk; b += nb * 256) {
    T z[G] = {};
    if (philox) sgld_normals(a.seed, chain, a.step, (uint32_t)(blk0 + b), z);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int64_t e = G * (int64_t)(blk0 + b) + j, i = e - e0;
      if (i < 0 || i >= n) continue;
      const T zi = philox ? z[j] : (T)a.noise[e];
      const T nu = a.two_eps * zi;
      const T hg = a.half_eps * g[i];
      T m;
      if (a.variant == 0) {
        m = nu + hg;
      } else {
        const T np = nu * p[i];
        m = np - hg;
        p[i] = m;
      }
      const T qv = q[i] + m;
      q[i] = qv;
      if (draw) draw[i] = qv;
      sq += (double)qv * (double)qv;
    }
  }
  block_sum2(sq, 0.0, part + v * NPART + bx, nullptr);
}
// The one-chain kernel: the same statements without the chain offsets (sharing one body cost it 2 – 3 SGPRs);
// keep the two in step.
template <typename T>
__global__ __launch_bounds__(256) void k_mlp_sgld(MlpSgld<T> a) {
  if (blockIdx.y >= 6) {
    const size_t lb = (size_t)(blockIdx.y - 6) * NPART + blockIdx.x;
    if (lb == 0) {
      if (a.out_loss && threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < a.nlb; ++b) s += a.lpart[b];
        *a.out_loss = s / (double)a.B;
      }
    } else if (a.masks) {
      const size_t g = (lb - 1) * 256 + threadIdx.x;
      if (g * 64 < (size_t)a.n3) mlp_masks_group<T>(a.masks, a.n3, a.seed, a.chain, a.mstep, a.slot, (int)g);
    }
    return;
  }
  const int v = blockIdx.y, n = a.vt.n[v], bx = blockIdx.x;
  const int nb = var_blocks(n);
  if (bx >= nb) {                                              // block-uniform
    if (threadIdx.x == 0) a.part[v * NPART + bx] = 0.0;
    return;
  }
  T* q = (T*)a.vt.q[v];
  T* p = (T*)a.vt.p[v];
  T* draw = (T*)a.vt.qc[v];
  const T* g = (const T*)a.vt.qn[v];
  const int e0 = a.vt.e0[v];                                   // e0 + n ≤ P < 2^31 (the host's int offsets)
  constexpr int G = sizeof(T) == 4 ? 4 : 2;                    // normals per Philox block
  const int blk0 = e0 / G, nblk = (int)(((int64_t)e0 + n + G - 1) / G) - blk0;   // blocks holding an element of v
  const bool philox = a.noise_mode == HMCX_NOISE_PHILOX;
  double sq = 0.0;
  for (int b = bx * 256 + (int)threadIdx.x; b < nblk; b += nb * 256) {
    T z[G] = {};
    if (philox) sgld_normals(a.seed, a.chain, a.step, (uint32_t)(blk0 + b), z);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int64_t e = G * (int64_t)(blk0 + b) + j, i = e - e0;
      if (i < 0 || i >= n) continue;
      const T zi = philox ? z[j] : (T)a.noise[e];
      const T nu = a.two_eps * zi;
      const T hg = a.half_eps * g[i];
      T m;
      if (a.variant == 0) {
        m = nu + hg;
      } else {
        const T np = nu * p[i];
        m = np - hg;
        p[i] = m;
      }
      const T qv = q[i] + m;
      q[i] = qv;
      if (draw) draw[i] = qv;
      sq += (double)qv * (double)qv;
    }
  }
  block_sum2(sq, 0.0, a.part + v * NPART + bx, nullptr);
}

// The deferred bias / W3 gradients of a launch group's chains in one launch (k_pending's arithmetic per chain,
// on the chain's 32-row-block partials): blockIdx.z = chain, blockIdx.y = variable j of b1, b2, W3,
// b3, the x blocks share its elements.  One launch per group whatever its size, so no pending set ever fills.
// The argument block describes the group's first chain; chain c lies at fixed strides behind it, as in
// k_mlp_sgld_chains: θ and gradient [c][n_j], the partials at pstride elements per chain (the chains' workspaces
// are equal chunks taken one after the other; the host checks it).
template <typename T> struct PendChains {
  const T* part[4]; const T* W[4]; T* G[4];
  int n[4], nparts;
  T half_alpha;
  int64_t pstride;
};
// The sum is run_pending's — the partials added one after the other in row-block order, then apply_upd's
// v + ½α·θ — with PB = 8 loads in flight per batch instead of 16: the 16 clamped row offsets of run_pending's batch
// are what spills SGPRs there (inlined here: 32 spilled in float64), and the value does not depend on the batch size.
template <typename T>
__global__ __launch_bounds__(256) void k_pending_chains(PendChains<T> a) {
  constexpr int PB = 8;                                        // partials loaded per batch
  const size_t c = blockIdx.z;
  const int j = blockIdx.y;
  // the variable's record by compares on the block-uniform j: no indexed read of the argument block
  const int n = j == 0 ? a.n[0] : j == 1 ? a.n[1] : j == 2 ? a.n[2] : a.n[3];
  const T* const part = (j == 0 ? a.part[0] : j == 1 ? a.part[1] : j == 2 ? a.part[2] : a.part[3]) + c * a.pstride;
  const T* const W = (j == 0 ? a.W[0] : j == 1 ? a.W[1] : j == 2 ? a.W[2] : a.W[3]) + c * n;
  T* const G = (j == 0 ? a.G[0] : j == 1 ? a.G[1] : j == 2 ? a.G[2] : a.G[3]) + c * n;
  const int nparts = a.nparts;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    T s = T(0);
    for (int b0 = 0; b0 < nparts; b0 += PB) {
      T v[PB];
#pragma unroll
      for (int q = 0; q < PB; ++q) v[q] = part[(size_t)min(b0 + q, nparts - 1) * n + i];   // clamped, unconditional
#pragma unroll
      for (int q = 0; q < PB; ++q)
        if (b0 + q < nparts) s = (b0 + q == 0) ? v[q] : s + v[q];
    }
    G[i] = s + a.half_alpha * W[i];
  }
}

// ------------------------------------------------------------------ host side
namespace {

inline bool vec_ok(const void* p, int ld, int elt) {
  return ((uintptr_t)p % 16 == 0) && ((size_t)ld * elt) % 16 == 0;
}

template <typename T>
struct MlpNet {
  int B, n_in, n_mid, n_out, nlb;
  const T* X; const int32_t* y;
  T *xw, *h2, *d3, *z, *gz, *ga2, *ga1;
  T *pb1, *pb2, *pb3, *pw3;              // gradient partials of b1, b2, b3, W3 ([nlb][...])
  T *fpb2 = nullptr, *fpb3 = nullptr, *fpw3 = nullptr;   // the same partials per 16-row block (k_fwdr, [nrb][...])
  unsigned long long* fr_prof = nullptr;  // HMCX_FWDR_PROF: stamps of the call's k_fwdr launches
  int fr_prof_cap = 0, fr_prof_n = 0;
  std::vector<int> fr_prof_np;
  int nrb = 0;                           // 16-row blocks: ⌈B/16⌉
  hipStream_t st;
  bool xw_valid = false;
  bool vec_masks = true;                 // masks may be read as 4-/2-element vectors
  PendSet<T> pend{};                     // consumed by the next launch
  // fused layer 2 + layer 3 (MM_L23): granule arena and epoch counter of the context
  char* gx = nullptr; int gx_bytes = 0; hmcx_ctx* ctx = nullptr; int* abort_flag = nullptr; bool fuse = false;
  double* lpart_scr = nullptr;           // batched sampler: the sub-step's loss partials (unused output)
  int force_abort = -1, l23_count = 0;   // HMCX_MLP_FORCE_ABORT: the fused launch (0-based, per call) that aborts
  int l23_fit = 0;                       // fused grids that fit on the chip at once (occupancy × CUs / grid)
  int64_t* fwd_counts = nullptr;         // the sampler's forward-launch counters (hmcx_get_mlp_forward_counts)
  unsigned long long* prof = nullptr;    // HMCX_MLP_PROF: stamps of every fused launch of the call
  int prof_cap = 0;
  int nvar(int v) const {
    switch (v) {
      case 0: return n_mid * n_in;  case 1: return n_mid;
      case 2: return n_mid * n_mid; case 3: return n_mid;
      case 4: return n_out * n_mid; default: return n_out;
    }
  }
};

template <typename T>
void net_init(MlpNet<T>& net, int B, int n_in, int n_mid, int n_out, hipStream_t st) {
  net.B = B; net.n_in = n_in; net.n_mid = n_mid; net.n_out = n_out; net.nlb = (B + 31) / 32; net.st = st;
  net.nrb = (B + FR_ROWS - 1) / FR_ROWS;
  net.vec_masks = n_mid % 4 == 0;
}

// an environment switch set to 0 (every HMCX_MLP_* switch is on unless its value starts with '0')
inline bool env_off(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '0';
}

// mask kind of a launch (one per launch: every sub-grid reads the same kind)
template <typename T> inline int mask_kind(const MaskSrc<T>& ms) {
  return ms.keep ? MK_KEEP : ms.vals ? MK_VALS : MK_NONE;
}
// f(std::integral_constant<int, MK>): a launch site instantiates its kernel once per mask kind it can meet
template <typename F> void with_mask_kind(int mk, F&& f) {
  if (mk == MK_KEEP) f(std::integral_constant<int, MK_KEEP>{});
  else if (mk == MK_VALS) f(std::integral_constant<int, MK_VALS>{});
  else f(std::integral_constant<int, MK_NONE>{});
}
// the float32-only launches: fwdr_ok / quad_ok admit keep-flag and buffer masks only
template <typename F> void with_mask_kind2(int mk, F&& f) {
  if (mk == MK_KEEP) f(std::integral_constant<int, MK_KEEP>{});
  else f(std::integral_constant<int, MK_VALS>{});
}

// The grids of a dual launch (k_mm2 / k_mm2b: two GEMM sub-grids side by side, z planes each): the tile
// grid of one, and the launch grid that covers both.
template <typename T> inline int3 tile_grid(const MMArgs<T>& a, int z) {
  return make_int3((a.M + 31) / 32, (a.N + 31) / 32, z);
}
inline dim3 dual_grid(const int3& g1, const int3& g2) {
  return dim3((unsigned)std::max(g1.x, g2.x), (unsigned)std::max(g1.y, g2.y), (unsigned)(g1.z + g2.z));
}
inline int2 xy(const int3& g) { return make_int2(g.x, g.y); }

// Launch k_mm for a call site with compile-time operand layouts (TA: A stored [K][M], TB: B stored
// [N][K]); k-contiguous operands take the 16-byte vector path when aligned.  Takes the pending update.
// BAT: the call site passes a problem table (k_mmb); plain call sites instantiate k_mm only.
// XCD placement of one GEMM plane (xcd_place): the candidate that leaves each XCD the fewest distinct
// operand tiles (A row tiles + B column slices) — the dispatch order, y-major chunks, or one block of
// tiles per XCD.  f32 only: config 3's W1 gradient (8 × 25 tiles; chunks: 8 + 4 tiles per XCD instead
// of 1 + 25) went from 63 to 78 % L2 hits and 14.91 k to 15.04 k leapfrog/s, f64 measured 5.92 k → 5.90 k
// (DESIGN §5.3 Round 5).  HMCX_MLP_XMAP=0 keeps the dispatch order everywhere.
template <typename T>
void xcd_choose(MMArgs<T>& a, int GX, int GY, int gx, int gy) {
  static const bool off = env_off("HMCX_MLP_XMAP");
  a.xmap = 0;
  if (off || sizeof(T) != 4 || gx * gy < 16 || (GX * GY) % 8) return;
  const int per = GX * GY / 8;                                   // positions per XCD in the plane
  int best = GX % 8 == 0 ? (gx + 7) / 8 + gy : gx + gy;          // dispatch order
  const int P = gx * gy, q = P / 8 + (P % 8 ? 1 : 0);
  if (q <= per) {
    const int c = std::min(gx, q) + (q + gx - 1) / gx + 1;
    if (c < best) { best = c; a.xmap = 1; }
  }
  for (int bx = 1; bx <= gx; ++bx) {
    if (gx % bx) continue;
    for (int by = 1; by <= gy; ++by) {
      if (gy % by || (gx / bx) * (gy / by) != 8 || bx * by > per) continue;
      if (bx + by < best) { best = bx + by; a.xmap = 2; a.xbx = bx; a.xby = by; }
    }
  }
}

template <typename T, int EPI, int TA, int TB, int AOP = OP_PLAIN, int BOP = OP_PLAIN, bool BAT = false>
hipError_t mm(MlpNet<T>& net, MMArgs<T>& a, const MMProbs<T>* prp = nullptr) {
  if (a.ta != TA || a.tb != TB || (prp && !BAT)) return hipErrorInvalidValue;
  a.pend = net.pend;
  net.pend.n = 0;
  MMProbs<T> pr{};
  if (prp) pr = *prp;
  // a batched launch: one plane per problem, plus one for the pending updates
  dim3 grid((a.M + 31) / 32, (a.N + 31) / 32, (pr.n > 0 ? pr.n : 1) + (a.pend.n > 0 ? 1 : 0)), blk(MM_NT);
  if (EPI == MM_L3CE) grid.y = (unsigned)std::max(1, std::min(8, a.n_mid / 32));   // n_mid column slices
  if (pr.n == 0 && (EPI == MM_UPD || EPI == MM_STORE)) xcd_choose<T>(a, (int)grid.x, (int)grid.y, (int)grid.x, (int)grid.y);
  const bool h1ok = AOP != OP_H1 || net.vec_masks;
  const bool kvec = a.K % (int)(16 / sizeof(T)) == 0;       // vectors never straddle the K end
  bool aal = vec_ok(a.A, a.lda, sizeof(T)), bal = vec_ok(a.B, a.ldb, sizeof(T));
  for (int p = 0; p < pr.n; ++p) {                            // every problem's operands
    aal = aal && vec_ok(pr.p[p].A, a.lda, sizeof(T));
    bal = bal && vec_ok(pr.p[p].B, a.ldb, sizeof(T));
  }
  const bool av = !TA && h1ok && kvec && aal;
  const bool bv = TB && kvec && bal;
  hipStream_t st = net.st;
  auto go = [&](auto mkc) {
    constexpr int MK = decltype(mkc)::value;
    if constexpr (BAT) {
      if (pr.n > 0) {
        if (av && bv) hipLaunchKernelGGL((k_mmb<T, EPI, AOP, BOP, TA, TB, !TA, TB, MK>), grid, blk, 0, st, a, pr);
        else if (av) hipLaunchKernelGGL((k_mmb<T, EPI, AOP, BOP, TA, TB, !TA, 0, MK>), grid, blk, 0, st, a, pr);
        else if (bv) hipLaunchKernelGGL((k_mmb<T, EPI, AOP, BOP, TA, TB, 0, TB, MK>), grid, blk, 0, st, a, pr);
        else hipLaunchKernelGGL((k_mmb<T, EPI, AOP, BOP, TA, TB, 0, 0, MK>), grid, blk, 0, st, a, pr);
        return;
      }
    }
    if (av && bv) hipLaunchKernelGGL((k_mm<T, EPI, AOP, BOP, TA, TB, !TA, TB, MK>), grid, blk, 0, st, a);
    else if (av) hipLaunchKernelGGL((k_mm<T, EPI, AOP, BOP, TA, TB, !TA, 0, MK>), grid, blk, 0, st, a);
    else if (bv) hipLaunchKernelGGL((k_mm<T, EPI, AOP, BOP, TA, TB, 0, TB, MK>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_mm<T, EPI, AOP, BOP, TA, TB, 0, 0, MK>), grid, blk, 0, st, a);
  };
  constexpr bool masked = AOP == OP_H1 || BOP == OP_H1 || EPI == MM_L2 || EPI == MM_L3CE || EPI == MM_GA1 ||
                          EPI == MM_L23;
  if constexpr (!masked) go(std::integral_constant<int, MK_NONE>{});
  else with_mask_kind(mask_kind(a.ms), go);
  return hipGetLastError();
}

template <typename T>
void mm_set(MMArgs<T>& a, int M, int N, int K, const T* A, int lda, int ta, const T* B, int ldb, int tb, T* C, int ldc) {
  a.M = M; a.N = N; a.K = K; a.A = A; a.lda = lda; a.ta = ta; a.B = B; a.ldb = ldb; a.tb = tb; a.C = C; a.ldc = ldc;
}

// What the layer-3 kernel produces besides the loss
struct L3Want { bool ga2, pb2, pb3, pw3; };

// Forward with masks `ms` at parameters q (+ the requested layer-3 backward pieces); loss partials
// into lpart (null: no loss); logits (optional) stored without b3.  Layer 1 only when xw is stale.
template <typename T>
hipError_t mlp_forward(MlpNet<T>& net, T* const* q, const MaskSrc<T>& ms, double* lpart, L3Want w,
                       T* logits = nullptr) {
  const int B = net.B, nm = net.n_mid;
  hipError_t e;
  if (net.fwd_counts) ++net.fwd_counts[2];
  if (!net.xw_valid) {                                        // xw = X·W1ᵀ
    MMArgs<T> a{};
    mm_set<T>(a, B, nm, net.n_in, net.X, net.n_in, 0, q[0], net.n_in, 1, net.xw, nm);
    if ((e = mm<T, MM_STORE, 0, 1>(net, a))) return e;
    net.xw_valid = true;
  }
  if (net.fuse && lpart && !logits && net.n_out <= 32) {
    // h2, d3 and layer 3 (cross-entropy, layer-3 backward) in one launch (MM_L23)
    MMArgs<T> a{};
    mm_set<T>(a, B, nm, nm, net.xw, nm, 0, q[2], nm, 1, net.h2, nm);
    a.bias = q[3]; a.b1 = q[1]; a.ms = ms; a.C2 = net.d3;
    a.N3 = net.n_out; a.bias3 = q[5]; a.gz = net.gz; a.y = net.y; a.lpart = lpart;
    a.W3 = q[4]; a.h2 = net.h2; a.d3 = net.d3; a.n_mid = nm;
    a.ga2 = w.ga2 ? net.ga2 : nullptr;
    a.pb2 = w.pb2 ? net.pb2 : nullptr;
    a.pb3 = w.pb3 ? net.pb3 : nullptr;
    a.pw3 = w.pw3 ? net.pw3 : nullptr;
    a.C = nullptr; a.C2 = nullptr;                             // h2 / d3 stay in LDS
    a.gx = net.gx; a.gx_bytes = net.gx_bytes; a.ep = gx_next_epoch(net.ctx); a.abort_flag = net.abort_flag;
    a.force_abort = net.l23_count == net.force_abort;
    if (net.prof && net.l23_count < net.prof_cap)
      a.prof = net.prof + (size_t)net.l23_count * net.nlb * ((nm + 31) / 32) * L23_NPH;
    ++net.l23_count;
    return mm<T, MM_L23, 0, 1, OP_H1>(net, a);
  }
  {                                                           // h2, d3 from h1 = max((xw + b1)·m0, 0)
    MMArgs<T> a{};
    mm_set<T>(a, B, nm, nm, net.xw, nm, 0, q[2], nm, 1, net.h2, nm);
    a.bias = q[3]; a.b1 = q[1]; a.ms = ms; a.C2 = net.d3;
    if ((e = mm<T, MM_L2, 0, 1, OP_H1>(net, a))) return e;
  }
  if (logits) {
    MMArgs<T> a{};
    mm_set<T>(a, B, net.n_out, nm, net.d3, nm, 0, q[4], nm, 1, logits, net.n_out);
    if ((e = mm<T, MM_STORE, 0, 1>(net, a))) return e;
  }
  if (!lpart) return hipSuccess;
  MMArgs<T> a{};
  a.bias = q[5]; a.y = net.y; a.lpart = lpart; a.ms = ms;
  a.W3 = q[4]; a.h2 = net.h2; a.d3 = net.d3; a.n_mid = nm;
  a.ga2 = w.ga2 ? net.ga2 : nullptr;
  a.pb2 = w.pb2 ? net.pb2 : nullptr;
  a.pb3 = w.pb3 ? net.pb3 : nullptr;
  a.pw3 = w.pw3 ? net.pw3 : nullptr;
  if (net.n_out <= 32) {                                      // z, cross-entropy, layer-3 backward
    mm_set<T>(a, B, net.n_out, nm, net.d3, nm, 0, q[4], nm, 1, net.gz, net.n_out);
    return mm<T, MM_L3CE, 0, 1>(net, a);
  }
  {
    MMArgs<T> az{};
    mm_set<T>(az, B, net.n_out, nm, net.d3, nm, 0, q[4], nm, 1, net.z, net.n_out);
    if ((e = mm<T, MM_STORE, 0, 1>(net, az))) return e;       // d3·W3ᵀ; b3 is added in k_l3_wide
  }
  a.M = B; a.N = net.n_out; a.C = net.gz; a.ldc = net.n_out;
  a.pend = net.pend;
  net.pend.n = 0;
  const size_t lds = 32 * sizeof(double) + ((size_t)MM_NT + (size_t)32 * (net.n_out + 1)) * sizeof(T);
  with_mask_kind(mask_kind(a.ms), [&](auto mkc) {
    hipLaunchKernelGGL((k_l3_wide<T, decltype(mkc)::value>), dim3(net.nlb), dim3(MM_NT), lds, net.st, a, (const T*)net.z);
  });
  return hipGetLastError();
}

template <typename T>
hipError_t mlp_ga1(MlpNet<T>& net, T* const* q, const MaskSrc<T>& ms, bool want_pb1) {
  MMArgs<T> a{};
  mm_set<T>(a, net.B, net.n_mid, net.n_mid, net.ga2, net.n_mid, 0, q[2], net.n_mid, 0, net.ga1, net.n_mid);
  a.ms = ms; a.H = net.xw; a.b1 = q[1];
  a.colpart = want_pb1 ? net.pb1 : nullptr;
  return mm<T, MM_GA1, 0, 0>(net, a);
}

// Weight gradient of W1 (v = 0: ga1ᵀ·X) or W2 (v = 2: ga2ᵀ·h1, h1 from net's xw, b1 and the m0 mask) with the
// update `mode` in the k_mm epilogue (biases and W3 come from partials): the launch arguments, and the launch.
template <typename T>
void wgrad_build(MlpNet<T>& net, const MaskSrc<T>& ms, const T* b1, int v, int mode, const Upd<T>& u, MMArgs<T>& a) {
  const int B = net.B, nm = net.n_mid;
  a = MMArgs<T>{};
  a.upd_mode = mode; a.u = u;
  if (v == 2) {
    mm_set<T>(a, nm, nm, B, net.ga2, nm, 1, net.xw, nm, 0, nullptr, nm);
    a.ms = ms; a.b1 = b1;
  } else {
    mm_set<T>(a, nm, net.n_in, B, net.ga1, nm, 1, net.X, net.n_in, 0, nullptr, net.n_in);
  }
}
template <typename T>
hipError_t mlp_wgrad(MlpNet<T>& net, T* const* q, const MaskSrc<T>& ms, int v, int mode, const Upd<T>& u) {
  MMArgs<T> a;
  wgrad_build(net, ms, (const T*)q[1], v, mode, u, a);
  return v == 2 ? mm<T, MM_UPD, 1, 0, OP_PLAIN, OP_H1>(net, a) : mm<T, MM_UPD, 1, 0>(net, a);
}

// xw = X·W1ᵀ into net.xw
template <typename T>
hipError_t mlp_layer1(MlpNet<T>& net, const T* W1) {
  MMArgs<T> a{};
  mm_set<T>(a, net.B, net.n_mid, net.n_in, net.X, net.n_in, 0, W1, net.n_in, 1, net.xw, net.n_mid);
  net.xw_valid = true;
  return mm<T, MM_STORE, 0, 1>(net, a);
}

// xw = X·W1ᵀ for np (W1, out) pairs in one launch
template <typename T>
hipError_t mlp_layer1_batch(MlpNet<T>& net, const T* const* W1, T* const* out, int np) {
  MMArgs<T> a{};
  MMProbs<T> pr{};
  pr.n = np;
  for (int p = 0; p < np; ++p) {
    pr.p[p].A = net.X; pr.p[p].B = W1[p]; pr.p[p].C = out[p];
  }
  mm_set<T>(a, net.B, net.n_mid, net.n_in, net.X, net.n_in, 0, W1[0], net.n_in, 1, out[0], net.n_mid);
  return mm<T, MM_STORE, 0, 1, OP_PLAIN, OP_PLAIN, true>(net, a, &pr);
}

// One sub-step's share of a batched launch: its positions, masks, scratch net (ga2, ga1, gz and the
// gradient partials), loss partials and what its layer-3 backward must produce.
template <typename T> struct SubStep {
  const T* xw;                       // layer-1 output of its W1 (null: net's)
  const T* xw2 = nullptr;            // k_fwdr: the second split-K plane of layer 1 (xw = xw + xw2)
  T* xwout = nullptr;                // k_fwdr: store the summed xw here
  T* q[6];
  MaskSrc<T> ms;
  MlpNet<T>* scr;
  double* lpart;
  L3Want w;
  int v;
};

// Batched-launch argument builders: the shared MMArgs (problem 0's operands) and the problem table.
// Fused forwards (MM_L23) at net's xw (or the sub-step's own): problem p uses arena region p0 + p and
// writes into its own scratch.
template <typename T, typename PR>
void l23_build(MlpNet<T>& net, const SubStep<T>* const* ss, int np, int p0, MMArgs<T>& a, PR& pr) {
  const int nm = net.n_mid;
  a = MMArgs<T>{};
  pr.n = np;
  for (int p = 0; p < np; ++p) {
    const SubStep<T>& s = *ss[p];
    const MlpNet<T>& sc = *s.scr;
    MMProb<T>& q = pr.p[p];
    q = MMProb<T>{};
    q.A = s.xw ? s.xw : net.xw; q.B = s.q[2]; q.C = nullptr;
    q.b1 = s.q[1]; q.bias = s.q[3]; q.W3 = s.q[4]; q.bias3 = s.q[5];
    q.ms = s.ms;
    q.ga2 = s.w.ga2 ? sc.ga2 : nullptr;
    q.pb2 = s.w.pb2 ? sc.pb2 : nullptr;
    q.pb3 = s.w.pb3 ? sc.pb3 : nullptr;
    q.pw3 = s.w.pw3 ? sc.pw3 : nullptr;
    q.gz = sc.gz; q.lpart = s.lpart; q.colpart = nullptr;
    q.gx = net.gx + (size_t)(p0 + p) * net.gx_bytes;
  }
  const MMProb<T>& q0 = pr.p[0];
  mm_set<T>(a, net.B, nm, nm, q0.A, nm, 0, q0.B, nm, 1, nullptr, nm);
  a.bias = q0.bias; a.b1 = q0.b1; a.ms = q0.ms; a.C2 = nullptr;
  a.N3 = net.n_out; a.bias3 = q0.bias3; a.gz = q0.gz; a.y = net.y; a.lpart = q0.lpart;
  a.W3 = q0.W3; a.n_mid = nm;
  a.ga2 = q0.ga2; a.pb2 = q0.pb2; a.pb3 = q0.pb3; a.pw3 = q0.pw3;
  a.gx = q0.gx; a.gx_bytes = net.gx_bytes; a.ep = gx_next_epoch(net.ctx); a.abort_flag = net.abort_flag;
  a.force_abort = net.l23_count == net.force_abort;
  ++net.l23_count;
}

// Layer-1 backwards (MM_GA1: ga1 = (ga2·W2)·gate, + b1 partials for the b1 sub-step), each from its
// own ga2 into its own ga1.
template <typename T, typename PR>
void ga1_build(MlpNet<T>& net, const SubStep<T>* const* ss, int np, MMArgs<T>& a, PR& pr) {
  const int nm = net.n_mid;
  a = MMArgs<T>{};
  pr.n = np;
  for (int p = 0; p < np; ++p) {
    const SubStep<T>& s = *ss[p];
    MMProb<T>& q = pr.p[p];
    q = MMProb<T>{};
    q.A = s.scr->ga2; q.B = s.q[2]; q.C = s.scr->ga1;
    q.b1 = s.q[1]; q.ms = s.ms;
    q.colpart = s.v == 1 ? s.scr->pb1 : nullptr;
  }
  const MMProb<T>& q0 = pr.p[0];
  mm_set<T>(a, net.B, nm, nm, q0.A, nm, 0, q0.B, nm, 0, q0.C, nm);
  a.ms = q0.ms; a.H = net.xw; a.b1 = q0.b1; a.colpart = q0.colpart;
}

// The same arguments for sub-step s on its scratch net `sn`, with the SGHMC epilogue.
template <typename T>
void wgrad_build(MlpNet<T>& sn, const SubStep<T>& s, int v, const Upd<T>& u, MMArgs<T>& a) {
  wgrad_build(sn, s.ms, (const T*)s.q[1], v, UPD_SGHMC, u, a);
}

template <typename T>
hipError_t mlp_forward_batch(MlpNet<T>& net, const SubStep<T>* ss, int np) {
  const SubStep<T>* sp[MAXPROB];
  for (int p = 0; p < np; ++p) sp[p] = ss + p;
  MMArgs<T> a;
  MMProbs<T> pr{};
  l23_build(net, sp, np, 0, a, pr);
  if (net.fwd_counts) ++net.fwd_counts[1];
  return mm<T, MM_L23, 0, 1, OP_H1, OP_PLAIN, true>(net, a, &pr);
}

// The layer-1 backwards of np sub-steps and the W2 gradient of sub-step net `w2n` in ONE launch
// (k_mm2): neither reads what the other writes.  net's pending updates run in the first grid's extra
// plane.
template <typename T>
hipError_t mlp_ga1_w2(MlpNet<T>& net, const SubStep<T>* const* ss, int np, MlpNet<T>& w2n, const SubStep<T>& s2,
                      const Upd<T>& u2) {
  const int nm = net.n_mid;
  MMArgs<T> a1, a2;
  MMProbs3<T> pr{};
  ga1_build(net, ss, np, a1, pr);
  a1.pend = net.pend;
  net.pend.n = 0;
  wgrad_build(w2n, s2, 2, u2, a2);
  a2.pend = w2n.pend;
  w2n.pend.n = 0;
  if (mask_kind(a1.ms) != mask_kind(a2.ms)) return hipErrorInvalidValue;
  const int3 g1 = tile_grid(a1, np + (a1.pend.n > 0 ? 1 : 0)), g2 = tile_grid(a2, 1);
  const dim3 grid = dual_grid(g1, g2);
  bool aal = nm % (int)(16 / sizeof(T)) == 0;
  for (int p = 0; p < np; ++p) aal = aal && vec_ok(pr.p[p].A, nm, sizeof(T));
  hipStream_t st = net.st;
  auto go = [&](auto mkc, auto avc) {
    constexpr int MK = decltype(mkc)::value, AV = decltype(avc)::value;
    hipLaunchKernelGGL((k_mm2<T, MM_GA1, OP_PLAIN, OP_PLAIN, 0, 0, AV, 0, MM_UPD, OP_PLAIN, OP_H1, 1, 0, 0, 0, MK>),
                       grid, dim3(MM_NT), 0, st, a1, pr, a2, g1, xy(g2));
  };
  with_mask_kind(mask_kind(a1.ms), [&](auto mkc) {
    if (aal) go(mkc, std::integral_constant<int, 1>{});
    else go(mkc, std::integral_constant<int, 0>{});
  });
  return hipGetLastError();
}

// The quad schedule (iter_quad), four launches per iteration (float32, fit ≥ 4 fused grids co-resident,
// keep-flag or buffer masks, aligned operands): the fused forwards of 4 sub-steps (those of W1, b1, W2 and
// one more), then ONE launch of the other 2 fused forwards beside the layer-1 backwards of W1 / b1
// (mlp_l23_ga1, k_mm2b), then the W1 gradient (mlp_wgrad, the pending bias / W3 updates in its extra
// plane), then ONE launch of the next iteration's layer 1 beside the W2 gradient (mlp_l1_w2, k_mm2).
template <typename T>
bool quad_ok(const MlpNet<T>& net, const SubStep<T>* ss) {
  if (sizeof(T) != 4) return false;                            // float64: two fused grids fit, not four
  const int mk = mask_kind(ss[0].ms);
  if (mk != MK_KEEP && mk != MK_VALS) return false;
  if (net.l23_fit < 4 || net.n_mid % (int)(16 / sizeof(T)) || net.n_in % (int)(16 / sizeof(T))) return false;
  if (!net.vec_masks || !vec_ok(net.xw, net.n_mid, sizeof(T))) return false;
  for (int i = 0; i < 6; ++i)
    if (!vec_ok(ss[i].q[2], net.n_mid, sizeof(T)) || !vec_ok(ss[i].scr->ga2, net.n_mid, sizeof(T))) return false;
  return true;
}

template <typename T>
hipError_t mlp_l23_ga1(MlpNet<T>& net, const SubStep<T>* const* fw, int nf, const SubStep<T>* const* ga, int nga) {
  MMArgs<T> a1, a2;
  MMProbs3<T> p1{}, p2{};
  l23_build(net, fw, nf, 0, a1, p1);
  ga1_build(net, ga, nga, a2, p2);
  a1.pend.n = 0;
  a2.pend.n = 0;
  const int3 g1 = tile_grid(a1, nf), g2 = tile_grid(a2, nga);
  const dim3 grid = dual_grid(g1, g2);
  hipStream_t st = net.st;
  if constexpr (sizeof(T) == 4) {                              // float32 only (quad_ok)
    with_mask_kind2(mask_kind(a1.ms), [&](auto mkc) {
      constexpr int MK = decltype(mkc)::value;
      hipLaunchKernelGGL((k_mm2b<T, MM_L23, OP_H1, OP_PLAIN, 0, 1, 1, 1, MM_GA1, OP_PLAIN, OP_PLAIN, 0, 0, 1, 0, MK>),
                         grid, dim3(MM_NT), 0, st, a1, p1, a2, p2, g1, g2);
    });
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

// k_fwdr in the batched sampler: float32 (the bench's dtype; float64 keeps the k_mm forwards), n_mid a
// multiple of 32 up to 256, n_out ≤ 16, keep-flag or buffer masks, 16-byte aligned xw / W2 rows and
// masks.  on: the call's HMCX_MLP_FWDR switch; 0 keeps the k_mm fused forwards (MM_L23) — whose results
// the one-sub-step-at-a-time order reproduces bit for bit.
template <typename T>
bool fwdr_ok(const MlpNet<T>& net, const SubStep<T>* ss, int n, bool on) {
  if (!on || sizeof(T) != 4) return false;
  if (net.n_mid % 32 || net.n_mid > FR_NMAX || net.n_out > 16 || !net.vec_masks || !net.fpb2) return false;
  // layer 1 in two 16-byte-aligned split-K halves; the W2 gradient in 4 row quarters whose m0 masks start
  // on a keep word
  if (net.n_in % 8 || net.B % 4 || ((size_t)(net.B / 4) * net.n_mid) % 32) return false;
  const int mk = mask_kind(ss[0].ms);
  if (mk != MK_KEEP && mk != MK_VALS) return false;
  for (int i = 0; i < n; ++i) {
    const T* xw = ss[i].xw ? ss[i].xw : net.xw;
    if (!vec_ok(xw, net.n_mid, sizeof(T)) || !vec_ok(ss[i].q[2], net.n_mid, sizeof(T)) || mask_kind(ss[i].ms) != mk)
      return false;
    if (!vec_ok(ss[i].q[1], 4, 4) || !vec_ok(ss[i].q[3], 4, 4) || !vec_ok(ss[i].q[4], net.n_mid, sizeof(T))) return false;
    if (mk == MK_VALS && !vec_ok(ss[i].ms.vals, 4, 4)) return false;
  }
  return true;
}

// The forwards of np problems (sub-steps and energy forwards) in one k_fwdr launch: sub-step v writes
// ga2 when a backward reads it (W1, b1: the layer-1 backward; W2: its gradient) and the 16-row-block
// partials of its own bias / W3 gradient into its net's fpb2 / fpw3 / fpb3; energy forwards (v < 0)
// only their loss partials.  net's pending updates run in the extra plane.
template <typename T>
hipError_t mlp_fwdr(MlpNet<T>& net, const SubStep<T>* const* ss, int np, const RbFwdArgs<T>* flags = nullptr) {
  if (np < 1 || np > FR_MAXP) return hipErrorInvalidValue;
  if (net.fwd_counts) ++net.fwd_counts[0];
  RbFwdArgs<T> a{};
  if (flags) {                                                   // keep-flag rows: keep, n3, kr, seed, chain, step
    a.keep = flags->keep; a.n3 = flags->n3; a.kr = flags->kr; a.seed = flags->seed; a.chain = flags->chain;
    a.step = flags->step;
  }
  if (net.fr_prof && net.fr_prof_n < net.fr_prof_cap) {          // HMCX_FWDR_PROF: this launch's stamps
    a.prof = net.fr_prof + (size_t)net.fr_prof_n * net.nrb * FR_MAXP * FR_NPH;
    net.fr_prof_np[net.fr_prof_n++] = np;
  }
  a.M = net.B; a.n_mid = net.n_mid; a.n_out = net.n_out; a.np = np; a.y = net.y;
  for (int p = 0; p < np; ++p) {
    const SubStep<T>& x = *ss[p];
    RbFwdProb<T>& q = a.p[p];
    q.xw = x.xw ? x.xw : net.xw;
    q.xw2 = x.xw2;
    q.xwout = x.xwout;
    q.b1 = x.q[1]; q.W2 = x.q[2]; q.b2 = x.q[3]; q.W3 = x.q[4]; q.b3 = x.q[5];
    q.ms = x.ms;
    q.ga2 = (x.v >= 0 && x.v <= 2) ? x.scr->ga2 : nullptr;
    q.pb2 = x.w.pb2 ? x.scr->fpb2 : nullptr;
    q.pw3 = x.w.pw3 ? x.scr->fpw3 : nullptr;
    q.pb3 = x.w.pb3 ? x.scr->fpb3 : nullptr;
    q.lpart = x.v < 0 ? x.lpart : nullptr;
  }
  a.pend = net.pend;
  net.pend.n = 0;
  const size_t kitems = (size_t)a.kr.nf * ((a.n3 + 63) / 64), per_row = (size_t)net.nrb * FR_NW * 64;
  const unsigned krows = (unsigned)((kitems + per_row - 1) / per_row);
  const dim3 grid((unsigned)net.nrb, (unsigned)(np + (a.pend.n > 0 ? 1 : 0)) + krows);
  if constexpr (sizeof(T) == 4) {                              // float32 only (fwdr_ok)
    with_mask_kind2(mask_kind(a.p[0].ms), [&](auto mkc) {
      hipLaunchKernelGGL((k_fwdr<T, decltype(mkc)::value>), grid, dim3(FR_NW * 64), 0, net.st, a);
    });
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

// Layer 1 as two split-K planes (k_fwdr sums them, plane 0 + plane 1): out[w][h] = X[:, K_h]·W1_w[:, K_h]ᵀ
// over the h-th half of n_in, for nw W1s in one batched launch — twice the workgroups of the plain
// layer 1 (config 3: 256 instead of 128, each half the 784-deep dot products); net's pending updates run
// in the extra plane.  Needs n_in % 8 == 0 (16-byte vectors in both halves).
template <typename T>
hipError_t mlp_layer1_split(MlpNet<T>& net, const T* const* W1, T* const (*out)[2], int nw) {
  const int Kh = net.n_in / 2;
  MMArgs<T> a{};
  MMProbs<T> pr{};
  pr.n = 2 * nw;
  for (int w = 0; w < nw; ++w)
    for (int h = 0; h < 2; ++h) {
      MMProb<T>& q = pr.p[2 * w + h];
      q.A = net.X + (size_t)h * Kh; q.B = W1[w] + (size_t)h * Kh; q.C = out[w][h];
    }
  mm_set<T>(a, net.B, net.n_mid, Kh, pr.p[0].A, net.n_in, 0, pr.p[0].B, net.n_in, 1, pr.p[0].C, net.n_mid);
  return mm<T, MM_STORE, 0, 1, OP_PLAIN, OP_PLAIN, true>(net, a, &pr);
}

// The W1 gradient (SGHMC epilogue; pn's pending bias / W3 updates in its extra plane) and the W2 gradient
// of sub-step net `w2n` as 4 split-K partial planes wp[4][n_mid][n_mid] over the minibatch rows, in ONE
// launch (k_mm2b): the W2 update itself runs as a pending update (4 partials, summed in plane order) in
// the NEXT launch.  200 + 256 workgroups at config 3 instead of 200 and a separate 64-workgroup W2 launch.
template <typename T>
hipError_t mlp_w1_w2split(MlpNet<T>& pn0, const SubStep<T>& s1, const Upd<T>& u1, MlpNet<T>& w2n, const SubStep<T>& s2,
                          T* wp) {
  MMArgs<T> a1, a2;
  MMProbs3<T> p1{}, p2{};
  wgrad_build(pn0, s1, 0, u1, a1);
  a1.pend = pn0.pend;
  pn0.pend.n = 0;
  wgrad_build(w2n, s2, 2, Upd<T>{}, a2);
  a2.upd_mode = UPD_NONE;
  a2.pend.n = 0;
  const int nm = w2n.n_mid, Kq = w2n.B / 4;
  a2.K = Kq;
  p2.n = 4;
  for (int q = 0; q < 4; ++q) {
    MMProb<T>& x = p2.p[q];
    const size_t r0 = (size_t)q * Kq * nm;                       // rows q·Kq … of ga2 and xw (and the m0 mask)
    x.A = a2.A + r0; x.B = a2.B + r0; x.C = wp + (size_t)q * nm * nm; x.b1 = a2.b1;
    x.ms = a2.ms;
    if (x.ms.keep) x.ms.keep += r0 / 32;
    if (x.ms.vals) x.ms.vals += r0;
  }
  a2.C = p2.p[0].C; a2.ldc = nm;
  const int3 g1 = tile_grid(a1, 1 + (a1.pend.n > 0 ? 1 : 0)), g2 = tile_grid(a2, 4);   // a2: n_mid × n_mid
  const dim3 grid = dual_grid(g1, g2);
  if constexpr (sizeof(T) == 4) {                              // float32 only (the k_fwdr path)
    with_mask_kind2(mask_kind(a2.ms), [&](auto mkc) {
      constexpr int MK = decltype(mkc)::value;                 // the W1 gradient reads no masks
      hipLaunchKernelGGL((k_mm2b<T, MM_UPD, OP_PLAIN, OP_PLAIN, 1, 0, 0, 0, MM_STORE, OP_PLAIN, OP_H1, 1, 0, 0, 0, MK>),
                         grid, dim3(MM_NT), 0, pn0.st, a1, p1, a2, p2, g1, g2);
    });
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

// The layer-1 backwards of np sub-steps (W1, b1) in one batched launch.
template <typename T>
hipError_t mlp_ga1_batch(MlpNet<T>& net, const SubStep<T>* const* ss, int np) {
  MMArgs<T> a;
  MMProbs<T> pr{};
  ga1_build(net, ss, np, a, pr);
  return mm<T, MM_GA1, 0, 0, OP_PLAIN, OP_PLAIN, true>(net, a, &pr);
}

// Layer 1 of the next iteration (xw = X·W1ᵀ into `out`, net's X) and the W2 gradient of sub-step net
// `w2n` in one launch (k_mm2): the W2 gradient reads the CURRENT iteration's xw (another buffer) and
// writes only W2's momentum and next position; layer 1 reads only X and W1.  False: the operands are
// not all 16-byte aligned (the caller launches them one by one).
template <typename T>
hipError_t mlp_l1_w2(MlpNet<T>& net, const T* W1, T* out, MlpNet<T>& w2n, const SubStep<T>& s2, const Upd<T>& u2,
                     bool* done) {
  *done = false;
  MMArgs<T> a1{}, a2;
  MMProbs3<T> p1{};
  mm_set<T>(a1, net.B, net.n_mid, net.n_in, net.X, net.n_in, 0, W1, net.n_in, 1, out, net.n_mid);
  wgrad_build(w2n, s2, 2, u2, a2);
  a1.pend.n = 0;
  a2.pend.n = 0;
  const int mk = mask_kind(a2.ms);
  if (sizeof(T) != 4 || (mk != MK_KEEP && mk != MK_VALS) || net.n_in % 4 || !vec_ok(net.X, net.n_in, sizeof(T)) ||
      !vec_ok(W1, net.n_in, sizeof(T)))
    return hipSuccess;
  const int3 g1 = tile_grid(a1, 1), g2 = tile_grid(a2, 1);
  const dim3 grid = dual_grid(g1, g2);
  xcd_choose<T>(a1, (int)grid.x, (int)grid.y, g1.x, g1.y);     // layer 1: 4 × 4 tile blocks per XCD
  xcd_choose<T>(a2, (int)grid.x, (int)grid.y, g2.x, g2.y);     // W2 gradient: 2 × 4
  hipStream_t st = net.st;
  if constexpr (sizeof(T) == 4) {
    with_mask_kind2(mk, [&](auto mkc) {
      constexpr int MK = decltype(mkc)::value;   // layer 1 reads no masks: any kind is its plain code
      hipLaunchKernelGGL((k_mm2<T, MM_STORE, OP_PLAIN, OP_PLAIN, 0, 1, 1, 1, MM_UPD, OP_PLAIN, OP_H1, 1, 0, 0, 0, MK>),
                         grid, dim3(MM_NT), 0, st, a1, p1, a2, g1, xy(g2));
    });
    *done = true;
  }
  return hipGetLastError();
}

// Queue the update of variable v from the partials [nparts][n] on net's next launch.  False: the launch's
// MAXPEND slots are taken (the caller reports pend_full).
template <typename T>
bool set_pending_part(MlpNet<T>& net, int v, int mode, const Upd<T>& u, const T* part, int nparts) {
  if (net.pend.n == MAXPEND) return false;
  Pending<T>& p = net.pend.p[net.pend.n++];
  p.mode = mode; p.u = u; p.nparts = nparts; p.part = part;
  p.n = net.nvar(v);
  return true;
}

// The same for a bias or W3 (v = 1, 3, 4, 5) from the 32-row-block partials of `src` (default: net's own).
template <typename T>
bool set_pending(MlpNet<T>& net, int v, int mode, const Upd<T>& u, const MlpNet<T>* src = nullptr) {
  if (!src) src = &net;
  return set_pending_part(net, v, mode, u, v == 1 ? src->pb1 : v == 3 ? src->pb2 : v == 4 ? src->pw3 : src->pb3, net.nlb);
}

inline int pend_full(hmcx_ctx* ctx) {
  return set_error(ctx, HMCX_EINVAL, "mlp: more than 4 pending updates queued on one launch");
}

template <typename T>
hipError_t flush_pending(MlpNet<T>& net) {
  if (net.pend.n == 0) return hipSuccess;
  int n = 0;
  for (int j = 0; j < net.pend.n; ++j) n = std::max(n, net.pend.p[j].n);
  hipLaunchKernelGGL(k_pending<T>, dim3((n + 255) / 256), dim3(256), 0, net.st, net.pend);
  net.pend.n = 0;
  return hipGetLastError();
}

// Fused layer 2 + layer 3 (MM_L23) in the sampler when n_out ≤ 32, at most 16 column slices, and the
// whole grid fits on the chip at once (its slice workgroups wait for each other); HMCX_MLP_FUSE=0 or
// hmcx_set_mlp_fuse(ctx, 0) turns it off.  A timed-out exchange raises the MLP's own abort word
// (ctx->mlp_abort_dev, never the persistent SGHMC kernels' word) and the call reports it (out_abort).
// The arena holds `regions` equal parts: a batched fused launch gives problem p region p.
template <typename T>
int net_fuse(hmcx_ctx* ctx, MlpNet<T>& net, int regions = 1) {
  static const bool off = env_off("HMCX_MLP_FUSE");
  const int S = (net.n_mid + 31) / 32;
  if (off || ctx->mlp_nofuse || net.n_out > 32 || S > 16) return HMCX_OK;
  int per_cu = 0;
  const void* kfn = (const void*)k_mm<T, MM_L23, OP_H1, OP_PLAIN, 0, 1, 1, 1, MK_KEEP>;
  HMCX_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, MM_NT, 0));
  if ((long)per_cu * ctx->num_cus < (long)net.nlb * S) return HMCX_OK;
  const size_t need = (size_t)net.nlb * S * 32 * net.n_out * 16;
  if (need > 0x7fffffff) return HMCX_OK;
  if (int rc = gx_reserve(ctx, need * regions)) return rc;
  // batched fused launches: the fewest workgroups per CU of the batched variants that can run
  int per_b = per_cu;
  for (const void* f : {(const void*)k_mmb<T, MM_L23, OP_H1, OP_PLAIN, 0, 1, 1, 1, MK_KEEP>,
                        (const void*)k_mmb<T, MM_L23, OP_H1, OP_PLAIN, 0, 1, 0, 0, MK_KEEP>,
                        (const void*)k_mmb<T, MM_L23, OP_H1, OP_PLAIN, 0, 1, 1, 1, MK_VALS>,
                        (const void*)k_mmb<T, MM_L23, OP_H1, OP_PLAIN, 0, 1, 0, 0, MK_VALS>}) {
    int pc = 0;
    if (int rc = kernel_occupancy(ctx, f, MM_NT, 0, &pc)) return rc;
    per_b = std::min(per_b, pc);
  }
  net.l23_fit = std::min(regions, (int)((long)per_b * ctx->num_cus / ((long)net.nlb * S)));
  if (!ctx->mlp_abort_dev) {
    HMCX_HIP(ctx, hipMalloc((void**)&ctx->mlp_abort_dev, sizeof(int)));
    HMCX_HIP(ctx, hipMemsetAsync(ctx->mlp_abort_dev, 0, sizeof(int), ctx->stream));
  }
  net.gx = ctx->gx_arena;
  net.gx_bytes = (int)need;
  net.ctx = ctx;
  net.abort_flag = ctx->mlp_abort_dev;
  net.fuse = true;
  const char* fa = getenv("HMCX_MLP_FORCE_ABORT");
  net.force_abort = fa ? atoi(fa) : -1;
  return HMCX_OK;
}

template <typename T>
void mlp_workspace(Workspace& ws, MlpNet<T>& net) {
  const size_t mn = (size_t)net.B * net.n_mid;
  net.xw = ws.take<T>(mn); net.h2 = ws.take<T>(mn); net.d3 = ws.take<T>(mn);
  net.ga2 = ws.take<T>(mn); net.ga1 = ws.take<T>(mn);
  net.z = ws.take<T>((size_t)net.B * net.n_out); net.gz = ws.take<T>((size_t)net.B * net.n_out);
  net.pb1 = ws.take<T>((size_t)net.nlb * net.n_mid);
  net.pb2 = ws.take<T>((size_t)net.nlb * net.n_mid);
  net.pb3 = ws.take<T>((size_t)net.nlb * net.n_out);
  net.pw3 = ws.take<T>((size_t)net.nlb * net.n_out * net.n_mid);
}

// The net of a one-off call (gradient, loss, HMC trajectory): unfused — no exchange that could time out —
// with its workspace, loss partials and the caller's mask buffer (null: no masks).
template <typename T>
int oneoff_net(hmcx_ctx* ctx, Workspace& ws, MlpNet<T>& net, const void* X, const int32_t* y, int B, int n_in, int n_mid,
               int n_out, const void* masks, double** lpart, MaskSrc<T>* ms) {
  net_init(net, B, n_in, n_mid, n_out, ctx->stream);
  net.X = (const T*)X; net.y = y;
  do { ws.reset(); mlp_workspace<T>(ws, net); *lpart = ws.take<double>(net.nlb); } while (ws.retry());
  if (ws.failed) return HMCX_ENOMEM;
  *ms = MaskSrc<T>{(const T*)masks, nullptr, T(1), B * n_mid};
  if (masks && (uintptr_t)masks % 16) net.vec_masks = false;
  return HMCX_OK;
}

// Profiling dumps (HMCX_MLP_PROF, HMCX_FWDR_PROF): wait for the call, copy its n stamps from the device and
// let `records` append them to the file as records of an int header followed by stamps.
inline void prof_record(FILE* f, std::initializer_list<int> hdr, const unsigned long long* stamps, size_t n) {
  fwrite(hdr.begin(), sizeof(int), hdr.size(), f);
  fwrite(stamps, sizeof(unsigned long long), n, f);
}
template <typename F>
int prof_append(hmcx_ctx* ctx, hipStream_t st, const char* path, const unsigned long long* dev, size_t n, F&& records) {
  HMCX_HIP(ctx, hipStreamSynchronize(st));
  std::vector<unsigned long long> h(n);
  HMCX_HIP(ctx, hipMemcpy(h.data(), dev, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (FILE* f = fopen(path, "ab")) {
    records(f, (const unsigned long long*)h.data());
    fclose(f);
  }
  return HMCX_OK;
}

}  // namespace

template <typename T>
int mlp_masks_t(hmcx_ctx* ctx, int B, int n_mid, uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot,
                void* out) {
  const int n3 = 3 * B * n_mid;
  hipLaunchKernelGGL(k_mlp_masks<T>, dim3((unsigned)(((n3 + 63) / 64 + 255) / 256)), dim3(256), 0, ctx->stream,
                     (T*)out, n3, seed, chain, step, slot);
  HMCX_HIP(ctx, hipGetLastError());
  return HMCX_OK;
}

template <typename T>
int mlp_grad_t(hmcx_ctx* ctx, const void* X, const int32_t* y, int B, int n_in, int n_mid, int n_out,
               const hmcx_mlp_params* par, const void* masks, double alpha, hmcx_mlp_params* grads, double* loss) {
  MlpNet<T> net{};
  Workspace ws(ctx);
  double* lpart;
  MaskSrc<T> ms;
  if (int rc = oneoff_net<T>(ctx, ws, net, X, y, B, n_in, n_mid, n_out, masks, &lpart, &ms)) return rc;
  T* q[6];
  for (int v = 0; v < 6; ++v) q[v] = (T*)par->p[v];
  HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, lpart, L3Want{true, true, true, true}));
  HMCX_HIP(ctx, mlp_ga1<T>(net, q, ms, true));
  Upd<T> u{};
  u.half_alpha = (T)(0.5 * alpha);
  for (int v : {0, 2}) {
    u.W = q[v]; u.G = (T*)grads->p[v];
    HMCX_HIP(ctx, mlp_wgrad<T>(net, q, ms, v, UPD_GRAD, u));
  }
  for (int v : {1, 3, 4, 5}) {
    u.W = q[v]; u.G = (T*)grads->p[v];
    if (!set_pending(net, v, UPD_GRAD, u)) return pend_full(ctx);
    HMCX_HIP(ctx, flush_pending(net));
  }
  if (loss) {
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(1), 0, ctx->stream, lpart, net.nlb, B, loss);
    HMCX_HIP(ctx, hipGetLastError());
  }
  return HMCX_OK;
}

// The full-batch HMC trajectory of hmcx_mlp_hmc_leapfrog (hmc.py:46-56): g = grad(q); per iteration and
// variable v = order[i]: p_v −= ε/2·g_v, q_v += ε·p_v, g = grad(q), p_v −= ε·g_v; then p = −p.  Of each
// gradient only two components are ever read — g_v (this sub-step's second kick) and g_v' of the next
// variable (its first kick) — so each call computes just those, with mlp_grad_t's kernels and flags
// for them (identical bits), and the layer-1 output xw is reused until W1 itself moves.
template <typename T>
int mlp_leapfrog_t(hmcx_ctx* ctx, const hmcx_mlp_leapfrog_args* s) {
  MlpNet<T> net{};
  Workspace ws(ctx);
  double* lpart;
  MaskSrc<T> ms;
  const void* mptr = s->mask_mode == HMCX_MLP_MASKS_NONE ? nullptr : s->masks;
  if (int rc = oneoff_net<T>(ctx, ws, net, s->X, s->y, s->B, s->n_in, s->n_mid, s->n_out, mptr, &lpart, &ms)) return rc;
  T *q[6], *p[6], *g[6];
  int64_t dim[6];
  for (int v = 0; v < 6; ++v) {
    q[v] = (T*)s->q.p[v]; p[v] = (T*)s->p.p[v]; g[v] = (T*)s->g.p[v];
    dim[v] = net.nvar(v);
  }
  uint32_t slot = s->slot0;
  const bool pmasks = s->mask_mode == HMCX_MLP_MASKS_PHILOX;
  // the gradient components `want` (bit v) at q, in mlp_grad_t's order: forward (+ the layer-3 backward
  // pieces the wanted components use), layer-1 backward, W1 / W2 gradients, then the bias / W3 updates (one
  // k_pending launch for all of them: independent element-wise updates).  The call's masks are drawn by the
  // kicks launch before it (draw = false), except for the first call.
  auto grad = [&](unsigned want, bool draw, bool defer) -> int {
    if (pmasks && draw)
      if (int rc = mlp_masks_t<T>(ctx, s->B, s->n_mid, s->seed, s->chain, s->step, slot++, s->masks)) return rc;
    const bool l1 = want & 3u;
    HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, lpart,
                                 L3Want{(want & 15u) != 0, (want & 8u) != 0, (want & 32u) != 0, (want & 16u) != 0}));
    if (l1) HMCX_HIP(ctx, mlp_ga1<T>(net, q, ms, true));
    Upd<T> u{};
    u.half_alpha = (T)(0.5 * s->alpha);
    for (int v : {0, 2})
      if (want & (1u << v)) {
        u.W = q[v]; u.G = g[v];
        HMCX_HIP(ctx, mlp_wgrad<T>(net, q, ms, v, UPD_GRAD, u));
      }
    for (int v : {1, 3, 4, 5})
      if (want & (1u << v)) {
        u.W = q[v]; u.G = g[v];
        if (!set_pending(net, v, UPD_GRAD, u)) return pend_full(ctx);
      }
    if (!defer) HMCX_HIP(ctx, flush_pending(net));            // else: the next kicks launch applies them
    return HMCX_OK;
  };
  // one launch between two gradient calls: the second kick of variable pu (−1: none, hmc.py:53), the first
  // kick and the drift of variable nv (−1: none, :50-51), and the next call's masks
  auto kicks = [&](int pu, int nv, bool masks) -> int {
    MlpKicks<T> k{};
    int64_t n = 0;
    if (pu >= 0) { k.pu = p[pu]; k.gu = g[pu]; k.nu = dim[pu]; k.eu = (T)s->eps; n = std::max(n, k.nu); }
    if (nv >= 0) {
      k.pv = p[nv]; k.gv = g[nv]; k.qv = q[nv]; k.nv = dim[nv]; k.hv = (T)(0.5 * s->eps); k.ev = (T)s->eps;
      n = std::max(n, k.nv);
    }
    if (masks && pmasks) {
      k.masks = (T*)s->masks; k.n3 = 3 * s->B * s->n_mid; k.seed = s->seed; k.chain = s->chain; k.step = s->step;
      k.slot = slot++;
      n = std::max(n, (int64_t)(k.n3 + 63) / 64);
    }
    // the previous call's deferred bias / W3 gradients: the launch applies those its kicks read (g of pu or
    // nv); any other would be dropped, so it is applied first, in a launch of its own
    bool read_here = true;
    for (int j = 0; j < net.pend.n; ++j) {
      const Pending<T>& pd = net.pend.p[j];
      read_here = read_here && pd.mode == UPD_GRAD && (pd.u.G == k.gu || pd.u.G == k.gv);
    }
    if (!read_here) HMCX_HIP(ctx, flush_pending(net));
    k.ps = net.pend;
    net.pend.n = 0;
    if (n == 0) return HMCX_OK;
    const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_mlp_kicks<T>, dim3(nb, 3), dim3(256), 0, ctx->stream, k);
    HMCX_HIP(ctx, hipGetLastError());
    return HMCX_OK;
  };
  const int* o = s->order;
  // the last gradient call computes all six components, so g is the full gradient at the final
  // position (as the header promises); every earlier call only the two the next kicks read
  if (int rc = grad(s->n_iter > 0 ? 1u << o[0] : 63u, true, s->n_iter > 0)) return rc;
  for (int it = 0; it < s->n_iter; ++it)
    for (int i = 0; i < 6; ++i) {
      const int v = o[i];
      const bool tail = it == s->n_iter - 1 && i == 5;        // no next kick follows
      // :53 of the previous sub-step (none before the first), :50-51 of this one, this call's masks
      int rc = kicks(it == 0 && i == 0 ? -1 : o[(i + 5) % 6], v, true);
      if (v == 0) net.xw_valid = false;
      if (!rc) rc = grad(tail ? 63u : (1u << v) | (1u << o[(i + 1) % 6]), false, !tail);   // :52
      if (rc) return rc;
    }
  if (s->n_iter > 0)
    if (int rc = kicks(o[5], -1, false)) return rc;                                   // :53 of the last sub-step
  Neg6<T> ng{};                                                                         // :55-56
  int64_t nmax = 0;
  for (int v = 0; v < 6; ++v) { ng.p[v] = p[v]; ng.n[v] = dim[v]; nmax = std::max(nmax, dim[v]); }
  hipLaunchKernelGGL(k_mlp_neg6<T>, dim3((unsigned)std::min<int64_t>((nmax + 255) / 256, 4096), 6), dim3(256), 0,
                     ctx->stream, ng);
  HMCX_HIP(ctx, hipGetLastError());
  return HMCX_OK;
}

// Momentum SGD of hmcx_mlp_sgd_run (sgd.py:36-42): per step mlp_grad_t's own launches on the step's minibatch
// (forward, layer-1 backward, W1 / W2 gradients, the bias / W3 gradients in ONE k_pending launch — independent
// element-wise updates, the same bits as one launch each) into a gradient workspace, then k_mlp_sgd.  With
// n_out ≤ 32 that is 8 launches per step: layer 1, layer 2, layer 3 + CE, layer-1 backward, two weight
// gradients, k_pending, k_mlp_sgd (n_out > 32: 9, layer 3 takes two).  A marked step adds the evaluation: its
// masks (PHILOX: hmcx_mlp_masks's launch), mlp_loss_t's forward at the updated θ and k_mlp_sgd_eval.
// lpart is written by the gradient forward, read by the k_mlp_sgd behind it (out_loss[s]) and only then
// rewritten by the evaluation forward or the next step: stream order keeps the three apart.
template <typename T>
int mlp_sgd_t(hmcx_ctx* ctx, const hmcx_mlp_sgd_args* s) {
  MlpNet<T> net{};
  Workspace ws(ctx);
  double* lpart;
  MaskSrc<T> ms;
  const int B = s->B, n_mid = s->n_mid;
  if (int rc = oneoff_net<T>(ctx, ws, net, s->X, s->y, B, s->n_in, n_mid, s->n_out, nullptr, &lpart, &ms)) return rc;
  const bool philox = s->mask_mode == HMCX_MLP_MASKS_PHILOX, fixed = s->mask_mode == HMCX_MLP_MASKS_FIXED;
  const int n3 = 3 * B * n_mid;
  T *g[6], *mscr = nullptr, *escr = nullptr;
  double* part;
  do {                                                         // oneoff_net's takes again, then this call's own
    ws.reset();
    mlp_workspace<T>(ws, net);
    lpart = ws.take<double>(net.nlb);
    for (int v = 0; v < 6; ++v) g[v] = ws.take<T>((size_t)net.nvar(v));
    part = ws.take<double>(6 * NPART);
    if (philox) { mscr = ws.take<T>((size_t)n3); escr = ws.take<T>((size_t)n3); }
  } while (ws.retry());
  if (ws.failed) return HMCX_ENOMEM;
  if (int rc = timing_begin(ctx, ctx->stream)) return rc;
  T* q[6];
  MlpSgd<T> k{};
  for (int v = 0; v < 6; ++v) {
    q[v] = (T*)s->par.p[v];
    k.vt.q[v] = q[v]; k.vt.p[v] = s->mom.p[v]; k.vt.qn[v] = g[v]; k.vt.n[v] = net.nvar(v);
  }
  k.gamma = (T)s->gamma; k.lr = (T)s->step_size;
  k.part = part; k.lpart = lpart; k.nlb = net.nlb; k.B = B;
  k.n3 = n3; k.seed = s->seed; k.chain = s->chain; k.slot = MASK_SLOT0;
  const T* const X0 = (const T*)s->X;
  // the masks of a forward: FIXED at `off` of the caller's buffer, PHILOX in `scr`, NONE nothing
  auto masks_of = [&](const int64_t* off, int si, const T* scr) {
    const T* m = fixed ? (const T*)s->masks + off[si] : philox ? scr : nullptr;
    ms.vals = m;
    net.vec_masks = n_mid % 4 == 0 && !(m && (uintptr_t)m % 16);
  };
  const int ng = (n3 + 63) / 64;                               // mask groups: one thread each
  const unsigned xrows = (unsigned)(((size_t)(ng + 255) / 256 + 1 + NPART - 1) / NPART);
  if (philox)
    if (int rc = mlp_masks_t<T>(ctx, B, n_mid, s->seed, s->chain, s->step_base, MASK_SLOT0, mscr)) return rc;
  int n_eval = 0;
  for (int si = 0; si < s->n_steps; ++si) {
    net.X = X0 + (size_t)s->row0[si] * s->n_in;
    net.y = s->y + s->row0[si];
    net.xw_valid = false;
    masks_of(s->mask_off, si, mscr);
    HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, lpart, L3Want{true, true, true, true}));
    HMCX_HIP(ctx, mlp_ga1<T>(net, q, ms, true));
    Upd<T> u{};
    u.half_alpha = (T)(0.5 * s->alpha);
    for (int v : {0, 2}) {
      u.W = q[v]; u.G = g[v];
      HMCX_HIP(ctx, mlp_wgrad<T>(net, q, ms, v, UPD_GRAD, u));
    }
    for (int v : {1, 3, 4, 5}) {
      u.W = q[v]; u.G = g[v];
      if (!set_pending(net, v, UPD_GRAD, u)) return pend_full(ctx);
    }
    HMCX_HIP(ctx, flush_pending(net));
    const bool next_masks = philox && si + 1 < s->n_steps;
    k.out_loss = s->out_loss ? s->out_loss + si : nullptr;
    k.masks = next_masks ? mscr : nullptr;
    k.step = s->step_base + (uint32_t)(si + 1);
    const unsigned rows = next_masks ? xrows : k.out_loss ? 1u : 0u;
    hipLaunchKernelGGL(k_mlp_sgd<T>, dim3(NPART, 6 + rows), dim3(256), 0, ctx->stream, k);
    HMCX_HIP(ctx, hipGetLastError());
    if (!(s->want_eval && s->want_eval[si])) continue;
    // sgd.py:42: the state after the update on the same minibatch, fresh masks (forward 1 of the step)
    if (philox)
      if (int rc = mlp_masks_t<T>(ctx, B, n_mid, s->seed, s->chain, s->step_base + (uint32_t)si, MASK_SLOT0 + 1u, escr))
        return rc;
    masks_of(s->eval_mask_off, si, escr);
    net.xw_valid = false;                                      // W1 moved
    HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, lpart, L3Want{false, false, false, false}));
    hipLaunchKernelGGL(k_mlp_sgd_eval, dim3(1), dim3(64), 0, ctx->stream, lpart, net.nlb, B, part,
                       s->out_eval_loss + n_eval, s->out_eval_sumsq ? s->out_eval_sumsq + 6 * (size_t)n_eval : nullptr);
    HMCX_HIP(ctx, hipGetLastError());
    ++n_eval;
  }
  return timing_end(ctx, ctx->stream);
}

// SGLD of hmcx_mlp_sgld_run (sgld.py step inside sgmcmc.py's minibatch loop): mlp_sgd_t's schedule with another
// last kernel.  Per step the unfused launches of mlp_grad_t on the step's minibatch into a gradient workspace
// (forward, layer-1 backward, W1 / W2 gradients, the bias / W3 gradients in ONE k_pending launch), then
// k_mlp_sgld: noise, update, draw store, Σθ² partials, the step's loss and the next step's Philox masks — 8
// launches per ordinary step with n_out ≤ 32 (9 above: layer 3 takes two).  Each set bit of want_eval[s] adds
// an evaluation at the updated θ: its masks (PHILOX: hmcx_mlp_masks's launch, slot 0x80000000 + f), mlp_loss_t's
// forward and k_mlp_sgd_eval.  lpart is written by the gradient forward, read by the k_mlp_sgld behind it and
// only then rewritten by an evaluation forward (read by its k_mlp_sgd_eval) or the next step: stream order
// keeps them apart.
template <typename T>
int mlp_sgld_t(hmcx_ctx* ctx, const hmcx_mlp_sgld_args* s) {
  MlpNet<T> net{};
  Workspace ws(ctx);
  double* lpart;
  MaskSrc<T> ms;
  const int B = s->B, n_mid = s->n_mid;
  if (int rc = oneoff_net<T>(ctx, ws, net, s->X, s->y, B, s->n_in, n_mid, s->n_out, nullptr, &lpart, &ms)) return rc;
  const bool philox = s->mask_mode == HMCX_MLP_MASKS_PHILOX, fixed = s->mask_mode == HMCX_MLP_MASKS_FIXED;
  const int n3 = 3 * B * n_mid;
  T *g[6], *mscr = nullptr, *escr = nullptr;
  double* part;
  do {                                                         // oneoff_net's takes again, then this call's own
    ws.reset();
    mlp_workspace<T>(ws, net);
    lpart = ws.take<double>(net.nlb);
    for (int v = 0; v < 6; ++v) g[v] = ws.take<T>((size_t)net.nvar(v));
    part = ws.take<double>(6 * NPART);
    if (philox) { mscr = ws.take<T>((size_t)n3); escr = ws.take<T>((size_t)n3); }
  } while (ws.retry());
  if (ws.failed) return HMCX_ENOMEM;
  if (int rc = timing_begin(ctx, ctx->stream)) return rc;
  T* q[6];
  MlpSgld<T> k{};
  for (int v = 0; v < 6; ++v) {
    q[v] = (T*)s->par.p[v];
    k.vt.q[v] = q[v]; k.vt.p[v] = s->variant == 1 ? s->mom.p[v] : nullptr; k.vt.qn[v] = g[v]; k.vt.n[v] = net.nvar(v);
  }
  for (int i = 0, off = 0; i < 6; ++i) {                       // the noise layout: variable after variable in `order`
    k.vt.e0[s->order[i]] = off;
    off += net.nvar(s->order[i]);
  }
  k.variant = s->variant; k.noise_mode = s->noise_mode;
  k.seed = s->seed; k.chain = s->chain;
  k.part = part; k.lpart = lpart; k.nlb = net.nlb; k.B = B;
  k.n3 = n3; k.slot = MASK_SLOT0;
  const T* const X0 = (const T*)s->X;
  // the masks of a forward: FIXED at `off` of the caller's buffer, PHILOX in `scr`, NONE nothing
  auto masks_of = [&](int64_t off, const T* scr) {
    const T* m = fixed ? (const T*)s->masks + off : philox ? scr : nullptr;
    ms.vals = m;
    net.vec_masks = n_mid % 4 == 0 && !(m && (uintptr_t)m % 16);
  };
  const int ng = (n3 + 63) / 64;                               // mask groups: one thread each
  const unsigned xrows = (unsigned)(((size_t)(ng + 255) / 256 + 1 + NPART - 1) / NPART);
  if (philox)
    if (int rc = mlp_masks_t<T>(ctx, B, n_mid, s->seed, s->chain, s->step_base, MASK_SLOT0, mscr)) return rc;
  int n_eval = 0, n_draw = 0;
  for (int si = 0; si < s->n_steps; ++si) {
    net.X = X0 + (size_t)s->row0[si] * s->n_in;
    net.y = s->y + s->row0[si];
    net.xw_valid = false;
    masks_of(fixed ? s->mask_off[si] : 0, mscr);
    HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, lpart, L3Want{true, true, true, true}));
    HMCX_HIP(ctx, mlp_ga1<T>(net, q, ms, true));
    Upd<T> u{};
    u.half_alpha = (T)(0.5 * s->alpha);
    for (int v : {0, 2}) {
      u.W = q[v]; u.G = g[v];
      HMCX_HIP(ctx, mlp_wgrad<T>(net, q, ms, v, UPD_GRAD, u));
    }
    for (int v : {1, 3, 4, 5}) {
      u.W = q[v]; u.G = g[v];
      if (!set_pending(net, v, UPD_GRAD, u)) return pend_full(ctx);
    }
    HMCX_HIP(ctx, flush_pending(net));
    const double eps = s->eps[si];
    k.two_eps = (T)(2.0 * eps);
    k.half_eps = s->variant == 0 ? (T)(-0.5 * eps) : (T)(0.5 * eps);
    k.noise = s->noise_mode == HMCX_NOISE_BUFFER ? s->noise + s->noise_off[si] : nullptr;
    k.step = s->step_base + (uint32_t)si;
    const bool keep = s->want_draw && s->want_draw[si];
    for (int v = 0; v < 6; ++v)
      k.vt.qc[v] = keep ? (void*)((T*)s->draws.p[v] + (size_t)n_draw * (size_t)net.nvar(v)) : nullptr;
    n_draw += keep ? 1 : 0;
    const bool next_masks = philox && si + 1 < s->n_steps;
    k.out_loss = s->out_loss ? s->out_loss + si : nullptr;
    k.masks = next_masks ? mscr : nullptr;
    k.mstep = s->step_base + (uint32_t)(si + 1);
    const unsigned rows = next_masks ? xrows : k.out_loss ? 1u : 0u;
    hipLaunchKernelGGL(k_mlp_sgld<T>, dim3(NPART, 6 + rows), dim3(256), 0, ctx->stream, k);
    HMCX_HIP(ctx, hipGetLastError());
    const int want = s->want_eval ? s->want_eval[si] : 0;
    // the state after the update on the same minibatch, fresh masks: forward 1, then 2, of the step in call
    // order (sgmcmc.py:60-62 / 74-76 the log line, :79 the epoch-end negative_log_posterior)
    for (int bit = 0, f = 1; bit < 2; ++bit) {
      if (!((want >> bit) & 1)) continue;
      if (philox)
        if (int rc = mlp_masks_t<T>(ctx, B, n_mid, s->seed, s->chain, s->step_base + (uint32_t)si,
                                    MASK_SLOT0 + (uint32_t)f, escr))
          return rc;
      masks_of(fixed ? s->eval_mask_off[2 * (size_t)si + (size_t)(f - 1)] : 0, escr);
      net.xw_valid = false;                                    // W1 moved
      HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, lpart, L3Want{false, false, false, false}));
      hipLaunchKernelGGL(k_mlp_sgd_eval, dim3(1), dim3(64), 0, ctx->stream, lpart, net.nlb, B, part,
                         s->out_eval_loss + n_eval, s->out_eval_sumsq ? s->out_eval_sumsq + 6 * (size_t)n_eval : nullptr);
      HMCX_HIP(ctx, hipGetLastError());
      ++n_eval;
      ++f;
    }
  }
  return timing_end(ctx, ctx->stream);
}

// Launch k_mmc for a group of chains: mm()'s choices — tile grid, vector paths (over every chain's operands), mask
// kind (explicit values or none: the chains never read keep flags) — with one plane per chain and no pending plane.
namespace {
template <typename T, int EPI, int TA, int TB, int AOP = OP_PLAIN, int BOP = OP_PLAIN>
hipError_t mmc(MlpNet<T>& net, MMArgs<T>& a, const MMChains<T>& pr) {
  if (a.ta != TA || a.tb != TB || pr.n < 1 || pr.n > MAXPROB || a.ms.keep) return hipErrorInvalidValue;
  a.pend.n = 0;
  dim3 grid((a.M + 31) / 32, (a.N + 31) / 32, pr.n), blk(MM_NT);
  if (EPI == MM_L3CE) grid.y = (unsigned)std::max(1, std::min(8, a.n_mid / 32));   // n_mid column slices
  const bool h1ok = AOP != OP_H1 || net.vec_masks;
  const bool kvec = a.K % (int)(16 / sizeof(T)) == 0;
  bool aal = true, bal = true;
  for (int p = 0; p < pr.n; ++p) {
    aal = aal && vec_ok(pr.p[p].A, a.lda, sizeof(T));
    bal = bal && vec_ok(pr.p[p].B, a.ldb, sizeof(T));
  }
  const bool av = !TA && h1ok && kvec && aal;
  const bool bv = TB && kvec && bal;
  hipStream_t st = net.st;
  auto go = [&](auto mkc) {
    constexpr int MK = decltype(mkc)::value;
    if (av && bv) hipLaunchKernelGGL((k_mmc<T, EPI, AOP, BOP, TA, TB, !TA, TB, MK>), grid, blk, 0, st, a, pr);
    else if (av) hipLaunchKernelGGL((k_mmc<T, EPI, AOP, BOP, TA, TB, !TA, 0, MK>), grid, blk, 0, st, a, pr);
    else if (bv) hipLaunchKernelGGL((k_mmc<T, EPI, AOP, BOP, TA, TB, 0, TB, MK>), grid, blk, 0, st, a, pr);
    else hipLaunchKernelGGL((k_mmc<T, EPI, AOP, BOP, TA, TB, 0, 0, MK>), grid, blk, 0, st, a, pr);
  };
  constexpr bool masked = AOP == OP_H1 || BOP == OP_H1 || EPI == MM_L2 || EPI == MM_L3CE || EPI == MM_GA1;
  if constexpr (masked) {
    if (a.ms.vals) go(std::integral_constant<int, MK_VALS>{});
    else go(std::integral_constant<int, MK_NONE>{});
  } else {
    go(std::integral_constant<int, MK_NONE>{});
  }
  return hipGetLastError();
}
}  // namespace

// SGLD of hmcx_mlp_sgld_chains_run: mlp_sgld_t's schedule with the chains as the problems of batched launches.
// The chains are independent, so they run group after group (≤ MAXPROB chains each), a group taking all n steps
// before the next starts: the workspace holds one group.  Per step and group, n_out ≤ 32: layer 1 (k_mmb), layer 2,
// layer 3 + CE, layer-1 backward, W1 gradient, W2 gradient (k_mmc), the bias / W3 gradients (k_pending_chains) and
// the update (k_mlp_sgld_chains) — 8 launches for up to six chains.  n_out > 32: layers 2 and 3 chain by chain
// (mlp_forward's launches on the chain's net, k_l3_wide).  An evaluation adds the chains' masks (PHILOX: one
// hmcx_mlp_masks launch per chain), the batched forward and one k_mlp_sgd_eval per chain.  Every GEMM runs
// mm_body with the one-chain call's tiles and K split, the update keeps k_mlp_sgld's arithmetic: chain c equals
// the one-chain call under Philox chain chain0 + c bit for bit.  Each chain has its own xw, h2, d3, z, gz, ga2, ga1,
// gradient partials (its net), loss partials, gradient buffers, Σθ² partials and mask scratches.
template <typename T>
int mlp_sgld_chains_t(hmcx_ctx* ctx, const hmcx_mlp_sgld_chains_args* s) {
  const int B = s->B, n_mid = s->n_mid, C = s->C, G = std::min(C, MAXPROB);
  const bool philox = s->mask_mode == HMCX_MLP_MASKS_PHILOX, fixed = s->mask_mode == HMCX_MLP_MASKS_FIXED;
  const int n3 = 3 * B * n_mid;
  const size_t mstride = ((size_t)n3 + 63) / 64 * 64;          // a chain's mask scratch: 16-byte aligned like the first
  MlpNet<T> cn[MAXPROB];
  for (int c = 0; c < G; ++c) net_init(cn[c], B, s->n_in, n_mid, s->n_out, ctx->stream);
  MlpNet<T>& net = cn[0];                                      // the group's shared dimensions, minibatch and stream
  const int nlb = net.nlb;
  Workspace ws(ctx);
  T *g[6], *mscr = nullptr, *escr = nullptr;
  double *lpart, *part;
  do {
    ws.reset();
    for (int c = 0; c < G; ++c) mlp_workspace<T>(ws, cn[c]);
    lpart = ws.take<double>((size_t)G * nlb);
    for (int v = 0; v < 6; ++v) g[v] = ws.take<T>((size_t)G * net.nvar(v));
    part = ws.take<double>((size_t)G * 6 * NPART);
    if (philox) { mscr = ws.take<T>(G * mstride); escr = ws.take<T>(G * mstride); }
  } while (ws.retry());
  if (ws.failed) return HMCX_ENOMEM;
  // k_pending_chains reaches chain c's gradient partials at c·pstride behind the first chain's: the chains'
  // workspaces are equal chunks taken one after the other
  auto part_of = [](const MlpNet<T>& n, int v) -> const T* {
    return v == 1 ? n.pb1 : v == 3 ? n.pb2 : v == 4 ? n.pw3 : n.pb3;
  };
  const int64_t pstride = G > 1 ? (int64_t)(cn[1].pb1 - cn[0].pb1) : 0;
  for (int c = 0; c < G; ++c)
    for (int v : {1, 3, 4, 5})
      if (part_of(cn[c], v) != part_of(cn[0], v) + (int64_t)c * pstride)
        return set_error(ctx, HMCX_EINVAL, "mlp sgld chains: the chains' workspaces are not equally spaced");
  if (int rc = timing_begin(ctx, ctx->stream)) return rc;
  const T* const X0 = (const T*)s->X;
  const int nm = n_mid, n_out = s->n_out;
  const int ng = (n3 + 63) / 64;                               // mask groups: one thread each
  const unsigned xrows = (unsigned)(((size_t)(ng + 255) / 256 + 1 + NPART - 1) / NPART);
  int nmax_pend = 0;
  for (int v : {1, 3, 4, 5}) nmax_pend = std::max(nmax_pend, net.nvar(v));
  for (int c0 = 0; c0 < C; c0 += MAXPROB) {
    const int np = std::min(MAXPROB, C - c0);
    T* q[MAXPROB][6];
    const T* W1[MAXPROB];
    T* xw[MAXPROB];
    for (int c = 0; c < np; ++c) {
      for (int v = 0; v < 6; ++v) q[c][v] = (T*)s->par.p[v] + (size_t)(c0 + c) * (size_t)net.nvar(v);
      W1[c] = q[c][0];
      xw[c] = cn[c].xw;
    }
    MlpSgld<T> k{};
    for (int v = 0; v < 6; ++v) {
      k.vt.q[v] = q[0][v];
      k.vt.p[v] = s->variant == 1 ? (void*)((T*)s->mom.p[v] + (size_t)c0 * (size_t)net.nvar(v)) : nullptr;
      k.vt.qn[v] = g[v]; k.vt.n[v] = net.nvar(v);
    }
    for (int i = 0, off = 0; i < 6; ++i) {                     // the noise layout: variable after variable in `order`
      k.vt.e0[s->order[i]] = off;
      off += net.nvar(s->order[i]);
    }
    k.variant = s->variant; k.noise_mode = s->noise_mode;
    k.seed = s->seed; k.chain = s->chain0 + (uint32_t)c0;
    k.part = part; k.lpart = lpart; k.nlb = nlb; k.B = B;
    k.n3 = n3; k.slot = MASK_SLOT0;
    const SgldStrides cs{s->draw_stride, (int64_t)mstride};
    // the masks of a forward: FIXED at `off` of the caller's buffer (every chain's), PHILOX the chain's part of
    // `scr`, NONE nothing
    MaskSrc<T> ms[MAXPROB];
    auto masks_of = [&](int64_t off, const T* scr) {
      for (int c = 0; c < np; ++c) {
        const T* m = fixed ? (const T*)s->masks + off : philox ? scr + c * mstride : nullptr;
        ms[c] = MaskSrc<T>{m, nullptr, T(1), B * n_mid};
        cn[c].vec_masks = n_mid % 4 == 0 && !(m && (uintptr_t)m % 16);
      }
    };
    // the group's forward at its chains' θ: layer 1 as one batched launch, then layers 2 and 3
    auto forward = [&](bool want) -> int {
      HMCX_HIP(ctx, mlp_layer1_batch<T>(net, W1, xw, np));
      if (n_out > 32) {
        for (int c = 0; c < np; ++c) {
          cn[c].xw_valid = true;
          HMCX_HIP(ctx, mlp_forward<T>(cn[c], q[c], ms[c], lpart + (size_t)c * nlb, L3Want{want, want, want, want}));
        }
        return HMCX_OK;
      }
      MMChains<T> pr{};
      pr.n = np;
      for (int c = 0; c < np; ++c) {
        MMProbC<T>& p = pr.p[c];
        p.A = cn[c].xw; p.B = q[c][2]; p.C = cn[c].h2; p.C2 = cn[c].d3;
        p.b1 = q[c][1]; p.bias = q[c][3]; p.ms = ms[c];
      }
      MMArgs<T> a{};
      mm_set<T>(a, B, nm, nm, cn[0].xw, nm, 0, q[0][2], nm, 1, cn[0].h2, nm);
      a.ms = ms[0];
      HMCX_HIP(ctx, (mmc<T, MM_L2, 0, 1, OP_H1>(net, a, pr)));
      pr = MMChains<T>{};
      pr.n = np;
      for (int c = 0; c < np; ++c) {
        MMProbC<T>& p = pr.p[c];
        p.A = cn[c].d3; p.B = q[c][4]; p.C = cn[c].gz; p.bias = q[c][5]; p.ms = ms[c];
        p.lpart = lpart + (size_t)c * nlb;
        p.W3 = q[c][4]; p.h2 = cn[c].h2; p.d3 = cn[c].d3;
        p.ga2 = want ? cn[c].ga2 : nullptr;
        p.pb2 = want ? cn[c].pb2 : nullptr;
        p.pb3 = want ? cn[c].pb3 : nullptr;
        p.pw3 = want ? cn[c].pw3 : nullptr;
      }
      a = MMArgs<T>{};
      mm_set<T>(a, B, n_out, nm, cn[0].d3, nm, 0, q[0][4], nm, 1, cn[0].gz, n_out);
      a.y = net.y; a.n_mid = nm; a.ms = ms[0];
      HMCX_HIP(ctx, (mmc<T, MM_L3CE, 0, 1>(net, a, pr)));
      return HMCX_OK;
    };
    if (philox)
      for (int c = 0; c < np; ++c)
        if (int rc = mlp_masks_t<T>(ctx, B, n_mid, s->seed, s->chain0 + (uint32_t)(c0 + c), s->step_base, MASK_SLOT0,
                                    mscr + c * mstride))
          return rc;
    int n_eval = 0, n_draw = 0;
    for (int si = 0; si < s->n_steps; ++si) {
      for (int c = 0; c < np; ++c) {
        cn[c].X = X0 + (size_t)s->row0[si] * s->n_in;
        cn[c].y = s->y + s->row0[si];
      }
      masks_of(fixed ? s->mask_off[si] : 0, mscr);
      if (int rc = forward(true)) return rc;
      MMChains<T> pr{};
      MMArgs<T> a{};
      pr.n = np;
      for (int c = 0; c < np; ++c) {                           // layer-1 backward (+ b1 partials)
        MMProbC<T>& p = pr.p[c];
        p.A = cn[c].ga2; p.B = q[c][2]; p.C = cn[c].ga1; p.b1 = q[c][1]; p.ms = ms[c];
        p.colpart = cn[c].pb1; p.H = cn[c].xw;
      }
      mm_set<T>(a, B, nm, nm, cn[0].ga2, nm, 0, q[0][2], nm, 0, cn[0].ga1, nm);
      a.ms = ms[0];
      HMCX_HIP(ctx, (mmc<T, MM_GA1, 0, 0>(net, a, pr)));
      pr = MMChains<T>{};
      pr.n = np;
      for (int c = 0; c < np; ++c) {                           // W1 gradient: ga1ᵀ·X
        MMProbC<T>& p = pr.p[c];
        p.A = cn[c].ga1; p.B = net.X; p.uW = q[c][0]; p.uG = g[0] + (size_t)c * net.nvar(0);
      }
      a = MMArgs<T>{};
      mm_set<T>(a, nm, s->n_in, B, cn[0].ga1, nm, 1, net.X, s->n_in, 0, nullptr, s->n_in);
      a.upd_mode = UPD_GRAD; a.u.half_alpha = (T)(0.5 * s->alpha);
      HMCX_HIP(ctx, (mmc<T, MM_UPD, 1, 0>(net, a, pr)));
      pr = MMChains<T>{};
      pr.n = np;
      for (int c = 0; c < np; ++c) {                           // W2 gradient: ga2ᵀ·h1, h1 from xw, b1 and m0
        MMProbC<T>& p = pr.p[c];
        p.A = cn[c].ga2; p.B = cn[c].xw; p.b1 = q[c][1]; p.ms = ms[c];
        p.uW = q[c][2]; p.uG = g[2] + (size_t)c * net.nvar(2);
      }
      a = MMArgs<T>{};
      mm_set<T>(a, nm, nm, B, cn[0].ga2, nm, 1, cn[0].xw, nm, 0, nullptr, nm);
      a.ms = ms[0];
      a.upd_mode = UPD_GRAD; a.u.half_alpha = (T)(0.5 * s->alpha);
      HMCX_HIP(ctx, (mmc<T, MM_UPD, 1, 0, OP_PLAIN, OP_H1>(net, a, pr)));
      PendChains<T> pc{};                                      // the bias / W3 gradients from the row-block partials
      pc.nparts = nlb; pc.half_alpha = (T)(0.5 * s->alpha); pc.pstride = pstride;
      {
        int j = 0;
        for (int v : {1, 3, 4, 5}) {
          pc.n[j] = net.nvar(v);
          pc.part[j] = part_of(cn[0], v);
          pc.W[j] = q[0][v];
          pc.G[j] = g[v];
          ++j;
        }
      }
      hipLaunchKernelGGL(k_pending_chains<T>, dim3((unsigned)((nmax_pend + 255) / 256), 4, (unsigned)np), dim3(256), 0,
                         ctx->stream, pc);
      HMCX_HIP(ctx, hipGetLastError());
      const double eps = s->eps[si];
      k.two_eps = (T)(2.0 * eps);
      k.half_eps = s->variant == 0 ? (T)(-0.5 * eps) : (T)(0.5 * eps);
      k.noise = s->noise_mode == HMCX_NOISE_BUFFER ? s->noise + s->noise_off[si] : nullptr;
      k.step = s->step_base + (uint32_t)si;
      const bool keep = s->want_draw && s->want_draw[si];
      for (int v = 0; v < 6; ++v)
        k.vt.qc[v] = keep ? (void*)((T*)s->draws.p[v] +
                                    ((size_t)c0 * (size_t)s->draw_stride + (size_t)n_draw) * (size_t)net.nvar(v))
                          : nullptr;
      n_draw += keep ? 1 : 0;
      const bool next_masks = philox && si + 1 < s->n_steps;
      k.out_loss = s->out_loss ? s->out_loss + (size_t)si * C + c0 : nullptr;
      k.masks = next_masks ? mscr : nullptr;
      k.mstep = s->step_base + (uint32_t)(si + 1);
      const unsigned rows = next_masks ? xrows : k.out_loss ? 1u : 0u;
      hipLaunchKernelGGL(k_mlp_sgld_chains<T>, dim3(NPART, 6 + rows, (unsigned)np), dim3(256), 0, ctx->stream, k, cs);
      HMCX_HIP(ctx, hipGetLastError());
      const int want = s->want_eval ? s->want_eval[si] : 0;
      for (int bit = 0, f = 1; bit < 2; ++bit) {               // forward 1, then 2, of the step (mlp_sgld_t)
        if (!((want >> bit) & 1)) continue;
        if (philox)
          for (int c = 0; c < np; ++c)
            if (int rc = mlp_masks_t<T>(ctx, B, n_mid, s->seed, s->chain0 + (uint32_t)(c0 + c),
                                        s->step_base + (uint32_t)si, MASK_SLOT0 + (uint32_t)f, escr + c * mstride))
              return rc;
        masks_of(fixed ? s->eval_mask_off[2 * (size_t)si + (size_t)(f - 1)] : 0, escr);
        if (int rc = forward(false)) return rc;
        for (int c = 0; c < np; ++c) {
          const size_t e = (size_t)n_eval * C + c0 + c;
          hipLaunchKernelGGL(k_mlp_sgd_eval, dim3(1), dim3(64), 0, ctx->stream, lpart + (size_t)c * nlb, nlb, B,
                             part + (size_t)c * 6 * NPART, s->out_eval_loss + e,
                             s->out_eval_sumsq ? s->out_eval_sumsq + 6 * e : nullptr);
          HMCX_HIP(ctx, hipGetLastError());
        }
        ++n_eval;
        ++f;
      }
    }
  }
  return timing_end(ctx, ctx->stream);
}

template <typename T>
int mlp_loss_t(hmcx_ctx* ctx, const void* X, const int32_t* y, int B, int n_in, int n_mid, int n_out,
               const hmcx_mlp_params* par, const void* masks, double* loss, void* logits) {
  MlpNet<T> net{};
  Workspace ws(ctx);
  double* lpart;
  MaskSrc<T> ms;
  if (int rc = oneoff_net<T>(ctx, ws, net, X, y, B, n_in, n_mid, n_out, masks, &lpart, &ms)) return rc;
  T* q[6];
  for (int v = 0; v < 6; ++v) q[v] = (T*)par->p[v];
  HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, y ? lpart : nullptr, L3Want{false, false, false, false}, (T*)logits));
  if (logits) {
    const int n = B * n_out;
    hipLaunchKernelGGL(k_bias_into_z<T>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (T*)logits, q[5], n, n_out);
    HMCX_HIP(ctx, hipGetLastError());
  }
  if (y && loss) {
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(1), 0, ctx->stream, lpart, net.nlb, B, loss);
    HMCX_HIP(ctx, hipGetLastError());
  }
  return HMCX_OK;
}

// ------------------------------------------------------------------ hmcx_mlp_sghmc_run
// The pieces of mlp_sghmc_t (below): validate, plan, then per step the start launch, the leapfrog iterations
// on ONE of four host schedules (iter_fwdr / iter_quad / iter_chunked / iter_single; DESIGN §5.3 "Host
// schedules" has their eligibility and launches), the energy forwards and the accept test.  The object is
// the call context: the net and its scratch nets, the layout of the variables, the switches (each read once
// per call, in validate) and every workspace pointer (plan).
namespace {
template <typename T>
struct MlpSghmc {
  hmcx_ctx* ctx;
  const hmcx_mlp_sghmc_args* s;
  hipStream_t stream = nullptr;
  MlpNet<T> net{}, pn[6]{}, en[2]{};                         // pn: one per sub-step; en: gz of E_new / E_current
  int off_v[6], dim[6], P = 0;                               // element offset of each variable in `order`
  int mn = 0, n3 = 0, kw = 0, maxF = 2;                      // B·n_mid; mask elements, keep words per forward
  bool philox_masks = false, batch = false, keep_split_on = true, fwdr_on = true;
  T *par[6], *pv[6], *qa[6], *qb[6], *qc[6];
  T *xw_own = nullptr, *xw_b1 = nullptr, *xw_par = nullptr; // xw of even / odd iterations, of the start state
  T *xwp[2] = {}, *xpar[2] = {}, *w2part = nullptr;         // k_fwdr path: layer-1 split-K planes, W2 partials
  double *part_cur, *part_new, *lp_cur, *lp_new, *lp_scr;
  uint32_t* keep = nullptr;                                  // keep flags of the step: one bit per element
  int32_t* accf = nullptr;
  const char *prof_path = nullptr, *fr_prof_path = nullptr;
  bool commit_pending = false;                               // the previous step's proposal awaits its commit
  T* prev_prop[6] = {};
  // Batched: positions of iteration it (−1: the start state) in the (it % 3)-th of three sets: its sub-steps
  // read iterations it and it − 1 and write it + 1, so three sets never alias within an iteration (the pending
  // bias / W3 updates then run beside readers of it − 1).  Its xw in one of two: the next iteration's layer 1
  // may run beside this iteration's W2 gradient, which reads this iteration's xw.
  T* const* pos(int it) const { return it < 0 ? par : it % 3 == 0 ? qa : it % 3 == 1 ? qb : qc; }
  T* xwb(int it) const { return (it & 1) ? xw_b1 : xw_own; }
  // One leapfrog iteration: its positions and, on the batched schedules, its six sub-steps.
  struct Iter {
    int it;
    bool last;                                                 // no iteration follows in this step
    T* const* Xit; T* const* Xpr; T* const* Xnx;               // positions of iterations it, it − 1, it + 1
    SubStep<T> ss[6];
    const SubStep<T>* ga[6];                                   // the sub-steps with a layer-1 backward (W1, b1)
    int nga = 0, i2 = 0;                                       // i2: position of the W2 sub-step
    T* next(int v) const { return last ? nullptr : Xnx[v]; }  // where v's next position goes (none after the last)
  };
  // Fixed for a step, and the state that evolves through it.
  struct Step {
    const MlpSghmc* c;
    int si, n, F;                                              // F: forwards of the step, 6n + 2
    double eps;
    uint32_t step_id;
    const double* nz;                                          // BUFFER noise of the step (null: Philox)
    bool batched = false, fr_step = false, keep_split = false;
    T* cur[6];                                                 // the proposal's positions so far
    int fwd = 0;                                               // one at a time: forwards run so far
    bool l1_done = false;                                      // quad: the last launch carried the next layer 1
    // batched: the E_new / E_current forwards (step_begin), which rode along, which by k_fwdr
    SubStep<T> es[2];
    bool e_done[2] = {false, false}, e_fr[2] = {false, false};
    // masks of forward f of the step: its stored keep flags (Philox), or the caller's values
    MaskSrc<T> masks_for(int f) const {
      const T scale = (T)(1.0 / 0.9);
      if (c->philox_masks) return MaskSrc<T>{nullptr, c->keep + (size_t)f * c->kw, scale, c->mn};
      return MaskSrc<T>{(const T*)c->s->masks + c->s->mask_off[si] + (size_t)f * c->n3, nullptr, scale, c->mn};
    }
    // the SGHMC update of variable v in iteration x
    Upd<T> upd_for(const Iter& x, int v) const {
      const hmcx_mlp_sghmc_args* s = c->s;
      Upd<T> u{};
      u.W = x.Xit[v]; u.P = c->pv[v]; u.Qn = x.next(v);
      u.half_alpha = (T)(0.5 * s->alpha); u.eps = (T)eps; u.one_minus_eps = (T)(1.0 - eps);
      u.noise_scale = (T)(2.0 * eps);
      u.noise_mode = s->noise_mode;
      u.noise = nz ? nz + (size_t)c->P * (x.it + 1) + c->off_v[v] : nullptr;   // BUFFER: one block of P per iteration
      u.seed = s->seed; u.chain = s->chain; u.step = step_id; u.slot = (uint32_t)(x.it + 1);
      u.e0 = (uint32_t)c->off_v[v];
      return u;
    }
  };
  using IterFn = int (MlpSghmc::*)(Step&, Iter&);

  int validate() {
    net_init(net, s->B, s->n_in, s->n_mid, s->n_out, ctx->stream);
    if (int rc = net_fuse<T>(ctx, net, MAXPROB)) return rc;
    net.fwd_counts = ctx->mlp_fwd_counts;
    mn = s->B * s->n_mid; n3 = 3 * mn; kw = (n3 + 31) / 32;
    for (int i = 0, seen = 0; i < 6; ++i) {
      const int v = s->order[i];
      if (v < 0 || v > 5 || ((seen >> v) & 1))
        return set_error(ctx, HMCX_EINVAL, "mlp sghmc: order must be a permutation of 0..5");
      seen |= 1 << v;
      off_v[v] = P; dim[v] = net.nvar(v); P += dim[v];
      par[v] = (T*)s->par.p[v];
    }
    for (int si = 0; si < s->n_steps; ++si) {
      if (s->n_iter[si] < 0) return set_error(ctx, HMCX_EINVAL, "mlp sghmc: n_iter < 0");
      // the step-start launch has one grid row per forward of the step (gridDim.y = 6 + 6·n_iter + 2,
      // capped at 65535 by the hardware)
      if (s->n_iter[si] > (65535 - 8) / 6)
        return set_error(ctx, HMCX_EINVAL, "mlp sghmc: n_iter above 10921 leapfrog iterations per step");
      maxF = std::max(maxF, 6 * s->n_iter[si] + 2);
    }
    // A step's masks come from one of two sources: the caller's buffer (MK_VALS), or — Philox masks — the
    // step's keep flags, drawn once (k_mlp_start / k_mlp_keep / k_fwdr's free rows) and loaded by every
    // kernel that reads them (MK_KEEP).  No kernel here draws its own flags: the draws would sit on the
    // layer-2 GEMM's critical path.
    philox_masks = s->mask_mode == HMCX_NOISE_PHILOX;
    if (philox_masks) {
      if (n3 % 4) net.vec_masks = false;
    } else {
      if ((uintptr_t)s->masks % 16 || ((size_t)n3 * sizeof(T)) % 16) net.vec_masks = false;
      for (int si = 0; si < s->n_steps; ++si)
        if ((s->mask_off[si] * sizeof(T)) % 16) net.vec_masks = false;
    }
    // The switches, read per call (tests switch them).  Batched iterations: sub-step i of iteration it
    // (variable v = order[i]) evaluates the gradient at q_u(it) for the variables at order positions u ≤ i and
    // q_u(it − 1) for the others (sghmc.py:29-34: each variable is drifted just before its own gradient call)
    // and moves only v's momentum and v's NEXT position — it needs iteration it − 1 complete and nothing of
    // iteration it, so the six sub-steps of an iteration are independent and, with W1 first (one xw per
    // iteration), share launches: same arithmetic, operands, masks and noise as one at a time, identical results.
    batch = !env_off("HMCX_MLP_BATCH") && net.fuse && s->order[0] == 0 && net.l23_fit >= 1;
    fwdr_on = !env_off("HMCX_MLP_FWDR");
    keep_split_on = !env_off("HMCX_MLP_KEEP_SPLIT");
    return HMCX_OK;
  }

  int plan(Workspace& ws) {
    static const char* const paths[2] = {getenv("HMCX_MLP_PROF"), getenv("HMCX_FWDR_PROF")};   // read once
    prof_path = paths[0]; fr_prof_path = paths[1];
    net.prof_cap = prof_path && net.fuse ? 8192 : 0;
    net.fr_prof_cap = fr_prof_path ? 512 : 0;
    net.fr_prof_np.assign(net.fr_prof_cap, 0);
    do {
      ws.reset();
      mlp_workspace<T>(ws, net);
      for (int i = 0; i < 6 && batch; ++i) {
        net_init(pn[i], s->B, s->n_in, s->n_mid, s->n_out, ctx->stream);
        mlp_workspace<T>(ws, pn[i]);
        pn[i].lpart_scr = ws.take<double>(net.nlb);
        pn[i].fpb2 = ws.take<T>((size_t)net.nrb * s->n_mid);     // k_fwdr's 16-row-block partials
        pn[i].fpw3 = ws.take<T>((size_t)net.nrb * s->n_out * s->n_mid);
        pn[i].fpb3 = ws.take<T>((size_t)net.nrb * s->n_out);
      }
      net.fpb2 = batch ? pn[0].fpb2 : nullptr;                   // marks the buffers as present (fwdr_ok)
      const size_t nprof = (size_t)net.prof_cap * net.nlb * ((net.n_mid + 31) / 32) * L23_NPH;
      net.prof = nprof ? ws.take<unsigned long long>(nprof) : nullptr;
      net.fr_prof = fr_prof_path ? ws.take<unsigned long long>((size_t)512 * net.nrb * FR_MAXP * FR_NPH) : nullptr;
      for (int v = 0; v < 6; ++v) {
        pv[v] = ws.take<T>(dim[v]); qa[v] = ws.take<T>(dim[v]); qb[v] = ws.take<T>(dim[v]);
        qc[v] = batch ? ws.take<T>(dim[v]) : nullptr;
      }
      if (batch) {
        xw_par = ws.take<T>((size_t)mn);
        xw_b1 = ws.take<T>((size_t)mn);
        for (int h = 0; h < 2; ++h) { xwp[h] = ws.take<T>((size_t)mn); xpar[h] = ws.take<T>((size_t)mn); }
        w2part = ws.take<T>((size_t)4 * s->n_mid * s->n_mid);
        for (auto& e : en) e.gz = ws.take<T>((size_t)s->B * s->n_out);
      }
      part_cur = ws.take<double>(12 * NPART);
      part_new = ws.take<double>(12 * NPART);
      lp_cur = ws.take<double>(std::max(net.nlb, net.nrb));      // 32-row (k_mm) or 16-row (k_fwdr) partials
      lp_new = ws.take<double>(std::max(net.nlb, net.nrb));
      lp_scr = ws.take<double>(net.nlb);
      if (philox_masks) keep = ws.take<uint32_t>((size_t)maxF * kw);
      accf = ws.take<int32_t>(1);
    } while (ws.retry());
    xw_own = net.xw;
    return ws.failed ? HMCX_ENOMEM : HMCX_OK;
  }

  void step_begin(int si, Step& st) {
    net.X = (const T*)s->X + (size_t)s->row0[si] * s->n_in;
    net.y = s->y + s->row0[si];
    net.xw_valid = false;
    st.c = this; st.si = si; st.eps = s->eps[si];
    st.n = s->n_iter[si]; st.F = 6 * st.n + 2;
    st.step_id = s->step_base + (uint32_t)si;
    st.nz = s->noise_mode == HMCX_NOISE_BUFFER ? s->noise + s->noise_off[si] : nullptr;
    st.batched = batch && st.n > 0;
    for (int v = 0; v < 6; ++v) st.cur[v] = par[v];
    if (!st.batched) return;
    // the k_fwdr path for this step's iterations, on iteration 0's positions with the start state's xw and
    // forward 0's masks (decided before the start launch, which draws fewer keep flags when k_fwdr draws the
    // later iterations': only iteration 0's and the two energy forwards'; HMCX_MLP_KEEP_SPLIT=0: all of them)
    Iter x0;
    iter_begin(st, 0, x0);
    for (SubStep<T>& y : x0.ss) { y.xw = xw_par; y.ms = st.masks_for(0); }
    st.fr_step = fwdr_ok(net, x0.ss, 6, fwdr_on);
    st.keep_split = philox_masks && st.fr_step && st.n > 1 && keep_split_on;
    for (int i = 0; i < 6; ++i) { pn[i].X = net.X; pn[i].y = net.y; pn[i].vec_masks = net.vec_masks; }
    // The energy forwards (hmc.py:67-71): E_new at the last iteration's positions with forward 6n's masks,
    // E_current at the start state with forward 6n + 1's.  Both only need what is known when the last
    // (first) iteration starts, so a schedule with room lets them ride in that iteration's forward launch
    // (energy_ride); energies_rest runs the others after the iterations.
    for (int e = 0; e < 2; ++e) {
      SubStep<T>& x = st.es[e];
      x.xw = e == 0 ? xwb(st.n - 1) : xw_par;
      for (int v = 0; v < 6; ++v) x.q[v] = e == 0 ? pos(st.n - 1)[v] : par[v];
      x.ms = st.masks_for(6 * st.n + e);
      x.scr = &en[e];
      x.lpart = e == 0 ? lp_new : lp_cur;
      x.w = L3Want{false, false, false, false};
      x.v = -1;
    }
  }
  // planes: k_fwdr sums its layer 1 from these two split-K planes and leaves 16-row loss partials
  const SubStep<T>* energy_ride(Step& st, int e, T* const* planes = nullptr) {
    if (planes) { st.es[e].xw = planes[0]; st.es[e].xw2 = planes[1]; st.e_fr[e] = true; }
    st.e_done[e] = true;
    return &st.es[e];
  }
  int energies_rest(Step& st) {
    for (int v = 0; v < 6; ++v) st.cur[v] = pos(st.n - 1)[v];
    SubStep<T> rest[2];                                        // each names its xw; one launch when both fit
    int nr = 0;
    for (int e = 0; e < 2; ++e)
      if (!st.e_done[e]) rest[nr++] = st.es[e];
    const int fit = std::min(MAXPROB, net.l23_fit);
    for (int e0 = 0; e0 < nr; e0 += fit) HMCX_HIP(ctx, mlp_forward_batch<T>(net, rest + e0, std::min(fit, nr - e0)));
    net.xw = xw_own;                                       // the net's own buffer again
    return HMCX_OK;
  }

  // The step-start launch: momentum (hmc.py:82-87), first drift into qa, Σp², Σθ² of the current state, the
  // previous step's commit folded in, and — Philox masks — the keep flags of the step's forwards (compute-bound
  // Philox draws: drawn instead beside each iteration's last launch, in an extra plane, they lengthened that
  // launch by as much as they took off this one — 21.46 k vs 22.2 k leapfrog/s at config 3).
  void step_start(Step& st) {
    VarTab vt{};
    for (int i = 0; i < 6; ++i) {
      const int v = s->order[i];
      vt.q[i] = par[v]; vt.qn[i] = qa[v]; vt.p[i] = pv[v]; vt.n[i] = dim[v]; vt.e0[i] = off_v[v];
      vt.qc[i] = commit_pending ? prev_prop[v] : nullptr;
    }
    const int32_t* prev_acc = commit_pending ? accf : nullptr;   // the previous step's commit, folded in
    commit_pending = false;
    const int n = st.n, drift = n > 0 ? 1 : 0;
    if (philox_masks) {
      // forwards 0 … 5 and the energies 6n, 6n + 1 when split, else all F
      const KeepRange kr = st.keep_split ? KeepRange{8, 0, 6, 6 * n} : KeepRange{st.F, 0, st.F, 0};
      const size_t items = (size_t)kr.nf * ((n3 + 63) / 64);      // one keep group per thread
      const unsigned rows = (unsigned)((items + (size_t)NPART * 256 - 1) / ((size_t)NPART * 256));
      hipLaunchKernelGGL(k_mlp_start<T>, dim3(NPART, 6 + rows), dim3(256), 0, stream, vt, (T)st.eps, drift, s->noise_mode,
                         st.nz, s->seed, s->chain, st.step_id, part_cur, prev_acc, keep, n3, kr);
    } else {
      hipLaunchKernelGGL(k_mlp_init<T>, dim3(NPART, 6), dim3(256), 0, stream, vt, (T)st.eps, drift, s->noise_mode, st.nz,
                         s->seed, s->chain, st.step_id, part_cur, prev_acc);
    }
  }

  // Iteration it of a step: its positions and, batched, its six sub-steps (sub-step i: the variables at order
  // positions ≤ i at iteration it, the others at it − 1) on this iteration's xw.
  void iter_begin(Step& st, int it, Iter& x) {
    const int* order = s->order;
    x.it = it; x.last = it + 1 == st.n;
    if (!st.batched) {                                         // one at a time: two sets in turn
      x.Xit = (it & 1) ? qb : qa; x.Xnx = (it & 1) ? qa : qb; x.Xpr = nullptr;
      return;
    }
    x.Xit = pos(it); x.Xpr = pos(it - 1); x.Xnx = pos(it + 1);
    net.xw = xwb(it);
    for (int i = 0; i < 6; ++i) {
      const int v = order[i];
      SubStep<T>& y = x.ss[i];
      pn[i].xw = net.xw;
      y.xw = nullptr;
      for (int j = 0; j < 6; ++j) y.q[order[j]] = j <= i ? x.Xit[order[j]] : x.Xpr[order[j]];
      y.ms = st.masks_for(6 * it + i);
      y.scr = &pn[i];
      y.lpart = pn[i].lpart_scr;
      y.w = L3Want{v <= 3, v == 3, v == 5, v == 4};
      y.v = v;
      if (v <= 1) x.ga[x.nga++] = &y;
      if (v == 2) x.i2 = i;
    }
  }

  // Queue the SGHMC updates of the four small variables (b1, b2, W3, b3) of iteration x from their gradient
  // partials: b1 — the layer-1 backward's 32-row partials — on t1's next launch, the others on t's, from
  // k_fwdr's 16-row-block partials (fr) or the fused k_mm forwards' 32-row ones.
  int queue_small(Step& st, Iter& x, MlpNet<T>& t1, MlpNet<T>& t, bool fr) {
    for (int i = 0; i < 6; ++i) {
      const int v = s->order[i];
      if (v == 0 || v == 2) continue;
      const MlpNet<T>& src = pn[i];
      const Upd<T> u = st.upd_for(x, v);
      const bool ok = v == 1 || !fr ? set_pending(v == 1 ? t1 : t, v, UPD_SGHMC, u, &src)
                                    : set_pending_part(t, v, UPD_SGHMC, u, v == 3 ? src.fpb2 : v == 4 ? src.fpw3 : src.fpb3,
                                                       net.nrb);
      if (!ok) return pend_full(ctx);
    }
    return HMCX_OK;
  }

  // Schedule fwdr, 4 launches, the layer-1 GEMM and the W2 gradient as split-K partials: k_fwdr (every forward
  // of the iteration and the energy forwards due; h1 from the two layer-1 planes, whose sum problem 0 stores as
  // the iteration's xw; the next iteration's keep flags) | the W1 / b1 layer-1 backwards | the W1 gradient + the
  // W2 gradient as 4 row-quarter partials, the pending bias / W3 updates in the extra plane | the next layer 1
  // with the W2 update from its partials in the extra plane (after the last: flushed before the kinetic energies)
  int iter_fwdr(Step& st, Iter& x) {
    if (x.it == 0) {                                           // layer 1 of iteration 0 and of the start state
      const T* w1[2] = {qa[0], par[0]};
      T* const out[2][2] = {{xwp[0], xwp[1]}, {xpar[0], xpar[1]}};
      HMCX_HIP(ctx, mlp_layer1_split<T>(net, w1, out, 2));
    }
    const SubStep<T>* fa[FR_MAXP];
    int na = 0;
    for (int i = 0; i < 6; ++i) {
      x.ss[i].xw = xwp[0];
      x.ss[i].xw2 = xwp[1];
      fa[na++] = &x.ss[i];
    }
    x.ss[0].xwout = net.xw;
    if (x.last) fa[na++] = energy_ride(st, 0, xwp);
    if (x.it == 0) fa[na++] = energy_ride(st, 1, xpar);
    RbFwdArgs<T> kf{};                                         // the next iteration's flags, in k_fwdr's free rows
    if (st.keep_split && !x.last) {
      kf.keep = keep; kf.n3 = n3; kf.kr = KeepRange{6, 6 * (x.it + 1), 6, 0};
      kf.seed = s->seed; kf.chain = s->chain; kf.step = st.step_id;
    }
    HMCX_HIP(ctx, mlp_fwdr<T>(net, fa, na, &kf));
    HMCX_HIP(ctx, mlp_ga1_batch<T>(net, x.ga, x.nga));
    if (int rc = queue_small(st, x, pn[0], pn[0], true)) return rc;
    HMCX_HIP(ctx, mlp_w1_w2split<T>(pn[0], x.ss[0], st.upd_for(x, 0), pn[x.i2], x.ss[x.i2], w2part));
    if (!set_pending_part(net, 2, UPD_SGHMC, st.upd_for(x, 2), w2part, 4)) return pend_full(ctx);
    if (!x.last) {
      const T* w1[1] = {x.Xnx[0]};
      T* const out[1][2] = {{xwp[0], xwp[1]}};
      HMCX_HIP(ctx, mlp_layer1_split<T>(net, w1, out, 1));
    }
    return HMCX_OK;
  }

  // Layer 1 of the k_mm schedules: iteration 0's xw together with the start state's (E_current reads it); a
  // later iteration's unless the previous iteration's last launch carried it.
  int iter_layer1(Step& st, Iter& x) {
    if (x.it == 0) {
      const T* w1[2] = {qa[0], par[0]};
      T* out[2] = {net.xw, xw_par};
      HMCX_HIP(ctx, mlp_layer1_batch<T>(net, w1, out, 2));
    } else if (!st.l1_done) {
      HMCX_HIP(ctx, mlp_layer1<T>(net, x.Xit[0]));
    }
    st.l1_done = false;
    return HMCX_OK;
  }

  // Schedule quad (quad_ok), 4 launches: the fused forwards of 4 sub-steps | the other 2 (and the energy forwards
  // due) + the W1 / b1 layer-1 backwards | the W1 gradient, every pending bias / W3 update in its extra plane | the
  // next layer 1 beside this iteration's W2 gradient (after the last, or operands unaligned: that gradient alone)
  int iter_quad(Step& st, Iter& x) {
    const int* order = s->order;
    if (int rc = iter_layer1(st, x)) return rc;
    const SubStep<T>* fa[6];
    const SubStep<T>* fb[6];
    int na = 0, nb = 0;
    for (int i = 0; i < 6; ++i)                                // W1, b1, W2 first: the second launch reads their ga2
      if (order[i] <= 2) fa[na++] = &x.ss[i];
    for (int i = 0; i < 6; ++i)
      if (order[i] > 2) {
        if (na < 4) fa[na++] = &x.ss[i];
        else fb[nb++] = &x.ss[i];
      }
    if (x.last) fb[nb++] = energy_ride(st, 0);
    if (x.it == 0 && st.n > 1) fb[nb++] = energy_ride(st, 1);
    MMArgs<T> a;
    MMProbs<T> pr{};
    l23_build(net, fa, na, 0, a, pr);
    ctx->mlp_fwd_counts[1] += 2;                               // both launches carry batched fused forwards
    HMCX_HIP(ctx, (mm<T, MM_L23, 0, 1, OP_H1, OP_PLAIN, true>(net, a, &pr)));
    HMCX_HIP(ctx, mlp_l23_ga1<T>(net, fb, nb, x.ga, x.nga));
    if (int rc = queue_small(st, x, pn[0], pn[0], false)) return rc;
    HMCX_HIP(ctx, mlp_wgrad<T>(pn[0], x.ss[0].q, x.ss[0].ms, 0, UPD_SGHMC, st.upd_for(x, 0)));
    const SubStep<T>& s2 = x.ss[x.i2];
    const Upd<T> u2 = st.upd_for(x, 2);
    if (!x.last) HMCX_HIP(ctx, mlp_l1_w2<T>(net, x.Xnx[0], xwb(x.it + 1), pn[x.i2], s2, u2, &st.l1_done));
    if (!st.l1_done) HMCX_HIP(ctx, mlp_wgrad<T>(pn[x.i2], s2.q, s2.ms, 2, UPD_SGHMC, u2));
    return HMCX_OK;
  }

  // Schedule chunked: layer 1 | the six fused forwards in launches of as many as fit co-resident (f32 at config 3:
  // 4; one 6-problem launch with spilled registers measured 47.8 µs vs 23.8 + 17.4) | the W1 / b1 layer-1 backwards
  // + the W2 gradient (b2 / W3 / b3 updates in the extra plane) | the W1 gradient (b1's update in its extra plane)
  int iter_chunked(Step& st, Iter& x) {
    if (int rc = iter_layer1(st, x)) return rc;
    const int fit = std::min(MAXPROB, net.l23_fit);
    for (int i0 = 0; i0 < 6; i0 += fit) HMCX_HIP(ctx, mlp_forward_batch<T>(net, x.ss + i0, std::min(fit, 6 - i0)));
    if (int rc = queue_small(st, x, pn[0], net, false)) return rc;
    HMCX_HIP(ctx, mlp_ga1_w2<T>(net, x.ga, x.nga, pn[x.i2], x.ss[x.i2], st.upd_for(x, 2)));
    HMCX_HIP(ctx, mlp_wgrad<T>(pn[0], x.ss[0].q, x.ss[0].ms, 0, UPD_SGHMC, st.upd_for(x, 0)));
    return HMCX_OK;
  }

  // Schedule one at a time: per sub-step its forward, the layer-1 backward (W1, b1) and the W1 / W2 gradient; a
  // bias / W3 update waits for the next launch.  Then its energies (hmc.py:67-71: E_new first, then
  // E_current), each with fresh masks.
  int iter_single(Step& st, Iter& x) {
    for (int i = 0; i < 6; ++i) {
      const int v = s->order[i];
      st.cur[v] = x.Xit[v];                                    // drifted position of this iteration
      if (v == 0) net.xw_valid = false;
      const MaskSrc<T> ms = st.masks_for(st.fwd++);
      HMCX_HIP(ctx, mlp_forward<T>(net, st.cur, ms, lp_scr, L3Want{v <= 3, v == 3, v == 5, v == 4}));
      if (v <= 1) HMCX_HIP(ctx, mlp_ga1<T>(net, st.cur, ms, v == 1));
      if (v == 0 || v == 2) HMCX_HIP(ctx, mlp_wgrad<T>(net, st.cur, ms, v, UPD_SGHMC, st.upd_for(x, v)));
      else if (!set_pending(net, v, UPD_SGHMC, st.upd_for(x, v))) return pend_full(ctx);
    }
    return HMCX_OK;
  }
  int energies_single(Step& st) {
    const L3Want none{false, false, false, false};
    HMCX_HIP(ctx, mlp_forward<T>(net, st.cur, st.masks_for(st.fwd++), lp_new, none));
    net.xw_valid = false;
    HMCX_HIP(ctx, mlp_forward<T>(net, par, st.masks_for(st.fwd++), lp_cur, none));
    return HMCX_OK;
  }

  // The schedule of a step, chosen once: one at a time when not batched; k_fwdr when the step-start check
  // (fr_step) and iteration 0's own sub-steps and energy forwards pass fwdr_ok; else quad when iteration 0's
  // sub-steps pass quad_ok (later iterations read workspace buffers, aligned alike); else chunked.  A step that
  // planned split keep flags for k_fwdr and does not run it draws the rest of them here.
  IterFn pick(Step& st) {
    if (!st.batched) return &MlpSghmc::iter_single;
    Iter x;
    iter_begin(st, 0, x);
    SubStep<T> chk[8] = {x.ss[0], x.ss[1], x.ss[2], x.ss[3], x.ss[4], x.ss[5], st.es[0], st.es[1]};
    if (st.fr_step && fwdr_ok(net, chk, 8, fwdr_on)) return &MlpSghmc::iter_fwdr;
    if (st.keep_split) {
      const KeepRange kr{6 * st.n - 6, 6, 6 * st.n - 6, 0};
      const size_t items = (size_t)kr.nf * ((n3 + 63) / 64);
      hipLaunchKernelGGL(k_mlp_keep, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, keep, n3, kr,
                         s->seed, s->chain, st.step_id);
    }
    return quad_ok(net, x.ss) ? &MlpSghmc::iter_quad : &MlpSghmc::iter_chunked;
  }

  // The step's tail: the last pending updates, the kinetic energies, the accept test, and the commit — in the
  // next step's start launch, or here after the call's last step.
  int step_accept(Step& st) {
    const int si = st.si;
    HMCX_HIP(ctx, flush_pending(net));
    VarTab ve{};
    for (int i = 0; i < 6; ++i) {
      const int v = s->order[i];
      ve.q[i] = st.cur[v]; ve.qn[i] = par[v]; ve.p[i] = pv[v]; ve.n[i] = dim[v];
    }
    hipLaunchKernelGGL(k_sumsq12<T>, dim3(NPART, 6), dim3(256), 0, stream, ve, part_new);
    MlpAccept ac{};
    ac.part_cur = part_cur; ac.part_new = part_new; ac.lp_cur = lp_cur; ac.lp_new = lp_new;
    ac.nlb_new = st.e_fr[0] ? net.nrb : net.nlb;
    ac.nlb_cur = st.e_fr[1] ? net.nrb : net.nlb;
    ac.B = s->B;
    for (int i = 0; i < 6; ++i) ac.dim[i] = dim[s->order[i]];
    ac.alpha = s->alpha; ac.u = s->u_accept[si];
    ac.out_A = s->out_A + si; ac.out_acc = s->out_accepted + si; ac.out_loss = s->out_loss + si;
    ac.out_nlp = s->out_nlp ? s->out_nlp + si : nullptr;
    ac.out_E = s->out_E ? s->out_E + 2 * si : nullptr;
    ac.acc_flag = accf;
    hipLaunchKernelGGL(k_mlp_accept, dim3(1), dim3(26 * 32), 0, stream, ac);
    if (st.n > 0 && si + 1 < s->n_steps) {
      commit_pending = true;
      for (int v = 0; v < 6; ++v) prev_prop[v] = st.cur[v];
    } else if (st.n > 0) {
      hipLaunchKernelGGL(k_mlp_commit<T>, dim3(NPART, 6), dim3(256), 0, stream, ve, accf);
    }
    HMCX_HIP(ctx, hipGetLastError());
    return HMCX_OK;
  }

  // HMCX_FWDR_PROF / HMCX_MLP_PROF=<file>: after the call, append the stamps its launches left.
  int profiles() {
    if (net.fr_prof && net.fr_prof_n) {                        // per k_fwdr launch {np, nrb, FR_NPH} + [np][nrb][FR_NPH]
      const size_t per = (size_t)net.nrb * FR_MAXP * FR_NPH;
      auto rec = [&](FILE* f, const unsigned long long* h) {
        for (int l = 0; l < net.fr_prof_n; ++l)
          prof_record(f, {net.fr_prof_np[l], net.nrb, FR_NPH}, h + l * per, (size_t)net.fr_prof_np[l] * net.nrb * FR_NPH);
      };
      if (int rc = prof_append(ctx, stream, fr_prof_path, net.fr_prof, per * net.fr_prof_n, rec)) return rc;
    }
    if (net.prof) {                                            // {launches, nlb, slices, L23_NPH} + their stamps
      const int nl = std::min(net.l23_count, net.prof_cap), S = (net.n_mid + 31) / 32;
      const size_t n = (size_t)nl * net.nlb * S * L23_NPH;
      auto rec = [&](FILE* f, const unsigned long long* h) { prof_record(f, {nl, net.nlb, S, L23_NPH}, h, n); };
      if (int rc = prof_append(ctx, stream, prof_path, net.prof, n, rec)) return rc;
    }
    return HMCX_OK;
  }

  // The call's verdict: the MLP abort word (raised by a timed-out exchange of any fused launch of this call)
  // goes to out_abort and is lowered for the next call — the call's outputs and state are then invalid and
  // the caller re-runs it unfused (sghmc._run_mlp); without out_abort, wait and report.
  int verdict() {
    int32_t* out = s->out_abort;
    if (!net.fuse) {
      if (out) HMCX_HIP(ctx, hipMemsetAsync(out, 0, sizeof(int32_t), stream));
      return HMCX_OK;
    }
    int flag = 0;
    if (out) HMCX_HIP(ctx, hipMemcpyAsync(out, ctx->mlp_abort_dev, sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    else HMCX_HIP(ctx, hipMemcpyAsync(&flag, ctx->mlp_abort_dev, sizeof(int), hipMemcpyDeviceToHost, stream));
    HMCX_HIP(ctx, hipMemsetAsync(ctx->mlp_abort_dev, 0, sizeof(int), stream));
    if (out) return HMCX_OK;
    HMCX_HIP(ctx, hipStreamSynchronize(stream));
    if (flag) return set_error(ctx, HMCX_EHIP, "mlp sghmc: fused layer-2/3 exchange timed out; state is invalid "
                                               "(re-run with hmcx_set_mlp_fuse(ctx, 0))");
    return HMCX_OK;
  }
};
}  // namespace

template <typename T>
int mlp_sghmc_t(hmcx_ctx* ctx, const hmcx_mlp_sghmc_args* s) {
  MlpSghmc<T> c{ctx, s};
  Workspace ws(ctx);
  int rc;
  if ((rc = c.validate()) || (rc = c.plan(ws))) return rc;
  begin_call(ctx);
  if ((rc = timing_begin(ctx, ctx->stream))) return rc;
  GraphScope gs(ctx);
  c.stream = c.net.st = ctx->stream;
  for (int si = 0; si < s->n_steps; ++si) {
    typename MlpSghmc<T>::Step st;
    c.step_begin(si, st);
    c.step_start(st);
    const auto iter = c.pick(st);                               // this step's schedule
    for (int it = 0; it < st.n; ++it) {
      typename MlpSghmc<T>::Iter x;
      c.iter_begin(st, it, x);
      if ((rc = (c.*iter)(st, x))) return rc;
    }
    if ((rc = st.batched ? c.energies_rest(st) : c.energies_single(st)) || (rc = c.step_accept(st))) return rc;
  }
  if ((rc = gs.finish()) || (rc = timing_end(ctx, ctx->stream)) || (rc = c.profiles())) return rc;
  return c.verdict();
}

// HMCX_MLP_DTYPES (bit 0 float, bit 1 double; both by default): the build compiles this file once per
// dtype (__graft_entry__.UNITS), so the two halves of its template instantiations build in parallel.
#ifndef HMCX_MLP_DTYPES
#define HMCX_MLP_DTYPES 3
#endif
// HMCX_MLP_CHAINS_UNIT: the unit holds hmcx_mlp_sgld_chains_run's side alone (mlp_sgld_chains_t and the kernels it
// launches), the units without it everything else — so the code objects of the SGHMC, HMC, SGD and one-chain SGLD
// paths hold the kernels they held before the chain kernels existed, at the same offsets.
#ifdef HMCX_MLP_CHAINS_UNIT
#define HMCX_MLP_INSTANTIATE(T) template int mlp_sgld_chains_t<T>(hmcx_ctx*, const hmcx_mlp_sgld_chains_args*);
#else
#define HMCX_MLP_INSTANTIATE(T)                                                                                       \
  template int mlp_masks_t<T>(hmcx_ctx*, int, int, uint64_t, uint32_t, uint32_t, uint32_t, void*);                    \
  template int mlp_grad_t<T>(hmcx_ctx*, const void*, const int32_t*, int, int, int, int, const hmcx_mlp_params*,      \
                             const void*, double, hmcx_mlp_params*, double*);                                         \
  template int mlp_loss_t<T>(hmcx_ctx*, const void*, const int32_t*, int, int, int, int, const hmcx_mlp_params*,      \
                             const void*, double*, void*);                                                            \
  template int mlp_sghmc_t<T>(hmcx_ctx*, const hmcx_mlp_sghmc_args*);                                                 \
  template int mlp_leapfrog_t<T>(hmcx_ctx*, const hmcx_mlp_leapfrog_args*);                                           \
  template int mlp_sgd_t<T>(hmcx_ctx*, const hmcx_mlp_sgd_args*);                                                     \
  template int mlp_sgld_t<T>(hmcx_ctx*, const hmcx_mlp_sgld_args*);
#endif
#if HMCX_MLP_DTYPES & 1
HMCX_MLP_INSTANTIATE(float)
#endif
#if HMCX_MLP_DTYPES & 2
HMCX_MLP_INSTANTIATE(double)
#endif

}  // namespace hmcx
