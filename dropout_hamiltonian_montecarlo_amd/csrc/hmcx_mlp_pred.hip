// hmcx_mlp_pred.hip — posterior predictive of the dropout MLP (hmcx_mlp_predictive): the mean class
// probabilities over D = S·T draws (S parameter sets × T dropout draws), the entropy of the mean, the mean
// entropy of the draws (their difference is the mutual information) and, with labels, the log pointwise
// predictive density and each draw's cross-entropy and hit count — one call, nothing per draw on the host.
//
// The network is hmcx_mlp.hip's (names in hmcx_mlp_kernels.h: a1 = X·W1ᵀ + b1, h1 = max(a1·m0, 0), h2 = max((h1·W2ᵀ + b2)·m1, 0),
// d3 = h2·m2, z = d3·W3ᵀ + b3).  The softmax of a row and everything summed over draws or rows is float64
// for both dtypes; every sum has a fixed order (no atomics, no exchange between workgroups: what crosses
// workgroups is a partial that a later launch sums in index order), so equal calls give equal bits.
//
// General path (every shape hmcx_mlp_loss accepts): per draw the existing forward (mlp_loss_t: logits, and
// with labels the draw's mean cross-entropy straight into out_draw_nll[d]), then k_pred_reduce — one thread
// per row: softmax, entropy, p[y], argmax, added to the per-row float64 accumulators in draw order (launch
// order on the stream) — and k_pred_finish / k_pred_draws at the end.
//
// Fused path (k_pred_fused; eligibility: pred_fused_shape_ok, the shapes k_fwdr serves): a workgroup owns a
// 16-row block of X, kept in LDS across a contiguous group of draws; per draw it streams W1_s, W2_s, W3_s
// (the [out][in] layout is k-contiguous: 16-byte loads along k, three 16-k chunks in flight per wave) through
// v_mfma_*_16x16x4 with the activations in LDS, in k_fwdr's transposed form — wave w owns the 32 columns
// n ∈ [32w, 32w + 32) of a layer over all of K, A = weight rows, B = the activation tile from LDS — draws
// (Philox: one keep_group per 64 flags of the block's rows, into LDS) or reads the masks, does the softmax
// with 16 lanes per row, and keeps its float64 partials in registers.  Grid: row blocks × draw groups.  The
// group partials [G][N][n_out] are summed in group order by k_pred_finish.
#include "hmcx_common.h"
#include "hmcx_internal.h"
#include "hmcx_mlp_mask.h"
#include <algorithm>

namespace hmcx {

namespace {

constexpr int PF_ROWS = 16;              // rows of X per workgroup (one MFMA tile)
constexpr int PF_NW = 8;                 // waves per workgroup: n_mid ≤ 32·PF_NW
constexpr int PF_NT = PF_NW * 64;
constexpr int PF_NMAX = 32 * PF_NW;
constexpr int PF_OMAX = 16;              // n_out ≤ one MFMA tile
constexpr int PF_KWN = 2 * (PF_ROWS * PF_NMAX / 64 + 1) + 2;   // keep words per mask of a row block (+ one group of slack)
constexpr int PF_MAXG = 32;              // draw groups at most
constexpr size_t PF_LDS_MAX = 160 * 1024;

// ------------------------------------------------------------------ softmax statistics of one row
// The row's logits z (T), in float64: p = exp(z − max) / Σ exp(z − max); H = −Σ p·log p (0·log 0 = 0) with
// log p = (z − max) − log Σ; arg = lowest index of the largest logit.
template <typename T>
__device__ inline void row_stats(const T* z, int K, int yv, double* acc_mean, bool first, double& H, double& py,
                                 int& arg) {
  double mx = (double)z[0];
  arg = 0;
  for (int k = 1; k < K; ++k) {
    const double v = (double)z[k];
    if (v > mx) { mx = v; arg = k; }
    else if (v != v) mx = v;                                   // NaN: the whole row is NaN
  }
  H = 0.0;
  py = 0.0;
  if (K <= 16) {                                               // the exponentials stay in registers: one exp per class
    double e[16], s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      e[k] = k < K ? exp((double)z[k < K ? k : 0] - mx) : 0.0;
      if (k < K) s += e[k];
    }
    const double ls = log(s);
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < K) {
        const double t = (double)z[k] - mx, p = e[k] / s;
        if (p != 0.0) H -= p * (t - ls);
        if (k == yv) py = p;
        acc_mean[k] = first ? p : acc_mean[k] + p;
      }
    return;
  }
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += exp((double)z[k] - mx);
  const double ls = log(s);
  for (int k = 0; k < K; ++k) {
    const double t = (double)z[k] - mx, p = exp(t) / s;
    if (p != 0.0) H -= p * (t - ls);
    if (k == yv) py = p;
    acc_mean[k] = first ? p : acc_mean[k] + p;
  }
}

// One draw's logits [N][K] into the accumulators (general path).  corr_part: this draw's hits per workgroup.
constexpr int PR_NT = 64;                // rows (threads) per k_pred_reduce workgroup: N = 10 000 is 157 workgroups
template <typename T>
__global__ __launch_bounds__(PR_NT) void k_pred_reduce(const T* z, const int32_t* y, int N, int K, int first,
                                                      double* acc_mean, double* acc_H, double* acc_py,
                                                      int32_t* corr_part) {
  __shared__ int hits[PR_NT];
  const int n = blockIdx.x * PR_NT + threadIdx.x;
  int hit = 0;
  if (n < N) {
    double H, py;
    int arg;
    const int yv = y ? y[n] : -1;
    row_stats<T>(z + (size_t)n * K, K, yv, acc_mean + (size_t)n * K, first != 0, H, py, arg);
    acc_H[n] = first ? H : acc_H[n] + H;
    if (y) acc_py[n] = first ? py : acc_py[n] + py;
    hit = (y && arg == yv) ? 1 : 0;
  }
  if (corr_part) {                                             // integer sum: exact in any order
    hits[threadIdx.x] = hit;
    __syncthreads();
    for (int s = PR_NT / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) hits[threadIdx.x] += hits[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) corr_part[blockIdx.x] = hits[0];
  }
}

// Per-row results from the G group partials (general path: G = 1), summed in group order.
struct PredFinish {
  int N, K, D, G;
  const double* gmean; const double* gH; const double* gpy;    // [G][N][K], [G][N], [G][N]
  const int32_t* y;
  double* out_mean; int32_t* out_pred; double* out_entropy; double* out_exp_entropy; double* out_lppd;
};
__global__ __launch_bounds__(256) void k_pred_finish(PredFinish a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.N) return;
  const double D = (double)a.D;
  double ent = 0.0, best = 0.0;
  int arg = 0;
  for (int k = 0; k < a.K; ++k) {
    double s = 0.0;
    for (int g = 0; g < a.G; ++g) s = g == 0 ? a.gmean[(size_t)n * a.K + k] : s + a.gmean[((size_t)g * a.N + n) * a.K + k];
    const double m = s / D;
    if (a.out_mean) a.out_mean[(size_t)n * a.K + k] = m;
    if (m != 0.0) ent -= m * log(m);
    if (k == 0 || m > best) { best = m; arg = k; }
  }
  if (a.out_pred) a.out_pred[n] = arg;
  if (a.out_entropy) a.out_entropy[n] = ent;
  if (a.out_exp_entropy) {
    double s = 0.0;
    for (int g = 0; g < a.G; ++g) s = g == 0 ? a.gH[n] : s + a.gH[(size_t)g * a.N + n];
    a.out_exp_entropy[n] = s / D;
  }
  if (a.out_lppd) {
    double s = 0.0;
    for (int g = 0; g < a.G; ++g) s = g == 0 ? a.gpy[n] : s + a.gpy[(size_t)g * a.N + n];
    a.out_lppd[n] = log(s / D);
  }
}

// Per-draw results from the per-workgroup partials [D][np], summed in workgroup order.
__global__ __launch_bounds__(256) void k_pred_draws(int D, int np, int N, const double* nll_part,
                                                     const int32_t* corr_part, double* out_nll, int32_t* out_correct) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  if (nll_part && out_nll) {
    double s = 0.0;
    for (int b = 0; b < np; ++b) s += nll_part[(size_t)d * np + b];
    out_nll[d] = s / (double)N;
  }
  if (corr_part && out_correct) {
    int c = 0;
    for (int b = 0; b < np; ++b) c += corr_part[(size_t)d * np + b];
    out_correct[d] = c;
  }
}

// ------------------------------------------------------------------ the fused row-block kernel
template <typename T> struct PredFused {
  int N, n_in, n_mid, n_out, Tn, D, dpg;                       // dpg: draws per group (blockIdx.y)
  int xk, xp, hp;                                              // X columns rounded up to 16; LDS pitches (elements)
  const T* X; const int32_t* y;
  const T* p[6];                                               // W1 … b3, S stacked copies each
  const T* masks;                                              // MK_VALS: [D][3][N][n_mid]
  uint64_t seed; uint32_t chain, step, slot0;                  // MK_PHILOX
  double* gmean; double* gH; double* gpy;                      // group partials [G][N][n_out], [G][N], [G][N]
  double* nll_part; int32_t* corr_part;                        // [D][row blocks], null without labels
  DropLaw<T> law;                                              // MK_PHILOX_LAW; last: the fields before it keep their offsets
};

// LDS layout of k_pred_fused (bytes): X tile, h1 tile, d3 tile, per-wave logit partials, keep words, row scratch.
struct PfLds { size_t xs, h1, h2, zr, kw, rown, rowc, total; };
__host__ __device__ inline size_t pf_up16(size_t bytes) { return (bytes + 15) / 16 * 16; }
__host__ __device__ inline PfLds pf_lds(int n_in, int n_mid, size_t elt) {
  const size_t xk = (size_t)((n_in + 15) / 16) * 16, xp = xk + 16 / elt, hp = (size_t)n_mid + 16 / elt;
  PfLds l;
  l.xs = 0;
  l.h1 = l.xs + pf_up16(PF_ROWS * xp * elt);
  l.h2 = l.h1 + pf_up16(PF_ROWS * hp * elt);
  l.zr = l.h2 + pf_up16(PF_ROWS * hp * elt);
  l.kw = l.zr + pf_up16((size_t)PF_NW * 16 * 17 * elt);
  l.rown = l.kw + pf_up16((size_t)3 * PF_KWN * 4);
  l.rowc = l.rown + pf_up16(PF_ROWS * 8);
  l.total = l.rowc + pf_up16(PF_ROWS * 4);
  return l;
}

// k offset, inside a 16-wide k chunk, of MFMA step u for lane group lg (hmcx_mlp_kernels.h's kmap: each lane's k
// values are contiguous, 4 floats or 2 + 2 doubles, so an operand along k is one or two 16-byte loads).
template <typename T> __device__ inline int pf_kmap(int u, int lg);
template <> __device__ inline int pf_kmap<float>(int u, int lg) { return 4 * lg + u; }
template <> __device__ inline int pf_kmap<double>(int u, int lg) { return ((u >> 1) << 3) + 2 * lg + (u & 1); }

// x[u] = P[k0 + kmap(u, lg)] for u = 0 … 3, P 16-byte aligned at those offsets (global or LDS)
template <typename T> __device__ inline void pf_ld16(const T* P, int k0, int lg, T (&x)[4]);
template <> __device__ inline void pf_ld16<float>(const float* P, int k0, int lg, float (&x)[4]) {
  const float4 v = *reinterpret_cast<const float4*>(P + k0 + 4 * lg);
  x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
}
template <> __device__ inline void pf_ld16<double>(const double* P, int k0, int lg, double (&x)[4]) {
  const double2 v = *reinterpret_cast<const double2*>(P + k0 + 2 * lg);
  const double2 w = *reinterpret_cast<const double2*>(P + k0 + 8 + 2 * lg);
  x[0] = v.x; x[1] = v.y; x[2] = w.x; x[3] = w.y;
}
// is chunk k0's piece of lane group lg inside [0, K)?  K % 4 == 0 (float) / K % 2 == 0 (double): a 16-byte
// piece lies entirely inside or entirely outside.  piece 0: u = 0, 1 (double) or all four (float); piece 1: u = 2, 3.
template <typename T> __device__ inline bool pf_in(int k0, int lg, int piece, int K) {
  if constexpr (sizeof(T) == 4) return k0 + 4 * lg < K;
  else return k0 + 8 * piece + 2 * lg < K;
}

// acc[j] += Wᵀ-tile · Bs over k ∈ [0, Kp): acc[j] = rows n0 + 16j + (tile row) of W (W[n][k], leading dimension
// ld, K valid columns, Kp = K rounded up to 16; operand values past K are zero) times the LDS tile Bs[r][k]
// (pitch bp, zero past K).  Three 16-k chunks of W in flight per wave.
template <typename T>
__device__ inline void pf_gemm(typename mfma16<T>::acc_t (&acc)[2], const T* W, int ld, int K, int Kp, int n0,
                               const T* Bs, int bp, int lr, int lg) {
  using Mf = mfma16<T>;
  T av[4][2][4];
  const T* w0 = W + (size_t)(n0 + lr) * ld;
  const T* w1 = W + (size_t)(n0 + 16 + lr) * ld;
  auto load = [&](int s, int k0) {
    if constexpr (sizeof(T) == 4) {
      if (pf_in<T>(k0, lg, 0, K)) { pf_ld16<T>(w0, k0, lg, av[s][0]); pf_ld16<T>(w1, k0, lg, av[s][1]); }
      else {
#pragma unroll
        for (int u = 0; u < 4; ++u) av[s][0][u] = av[s][1][u] = T(0);
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool in = pf_in<T>(k0, lg, h, K);
        const int ko = in ? k0 + 8 * h + 2 * lg : 0;
        const double2 a = *reinterpret_cast<const double2*>(w0 + ko), b = *reinterpret_cast<const double2*>(w1 + ko);
        av[s][0][2 * h] = in ? a.x : 0.0; av[s][0][2 * h + 1] = in ? a.y : 0.0;
        av[s][1][2 * h] = in ? b.x : 0.0; av[s][1][2 * h + 1] = in ? b.y : 0.0;
      }
    }
  };
  auto mf = [&](int s, int k0) {
    T hv[4];
    pf_ld16<T>(Bs + (size_t)lr * bp, k0, lg, hv);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = Mf::fma(av[s][j][u], hv[u], acc[j]);
  };
  load(0, 0);
  if (16 < Kp) load(1, 16);
  if (32 < Kp) load(2, 32);
  for (int k0 = 0; k0 < Kp; k0 += 64) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kk = k0 + 16 * s;
      if (kk < Kp) {
        if (kk + 48 < Kp) load((s + 3) & 3, kk + 48);
        mf(s, kk);
      }
    }
  }
}

// butterfly over the 16 lanes of a row (lanes tid & 15): the same order on every lane, so all 16 agree
__device__ inline double pf_sum16(double v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 16);
  return v;
}

// k_pred_fused's keep-flag draw as calls, not inlined: the kernel sits at its register limit (256 VGPRs in float64)
// and the inlined draw costs it spills and scratch.  The default ratio's law is compiled in (MK_PHILOX), any other
// arrives by value (MK_PHILOX_LAW).
__device__ __noinline__ KeepGroup pred_keep_group_default(uint64_t seed, uint32_t G, uint32_t slot, uint32_t step,
                                                          uint32_t chain) {
  return keep_group(KeepLawDefault{}, seed, G, slot, step, chain);
}
__device__ __noinline__ KeepGroup pred_keep_group_law(KeepLaw law, uint64_t seed, uint32_t G, uint32_t slot,
                                                      uint32_t step, uint32_t chain) {
  return keep_group(law, seed, G, slot, step, chain);
}

template <typename T, int MK>
__global__ __launch_bounds__(PF_NT) void k_pred_fused(PredFused<T> a) {
  using Mf = mfma16<T>;
  extern __shared__ __attribute__((aligned(16))) char pf_smem[];
  const PfLds L = pf_lds(a.n_in, a.n_mid, sizeof(T));
  T* Xs = reinterpret_cast<T*>(pf_smem + L.xs);
  T* H1 = reinterpret_cast<T*>(pf_smem + L.h1);
  T* H2 = reinterpret_cast<T*>(pf_smem + L.h2);
  T* zr = reinterpret_cast<T*>(pf_smem + L.zr);                // [wave][o][17]
  uint32_t* kw = reinterpret_cast<uint32_t*>(pf_smem + L.kw);  // [3][PF_KWN]
  double* rown = reinterpret_cast<double*>(pf_smem + L.rown);
  int* rowc = reinterpret_cast<int*>(pf_smem + L.rowc);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int N = a.N, nm = a.n_mid, No = a.n_out, xp = a.xp, hp = a.hp;
  const int rb = blockIdx.x, m0 = rb * PF_ROWS, nrb = gridDim.x;
  const size_t mn = (size_t)N * nm;
  const int n0 = 32 * wave;
  const bool wact = n0 < nm;                                   // this wave has columns (n_mid % 32 == 0: all 32)
  const bool rok = m0 + lr < N;                                // the row of this lane's accumulator column
  // the keep law: the default ratio's as constants (MK_PHILOX), any other ratio's from the argument block
  // (MK_PHILOX_LAW)
  constexpr bool PHILOX = MK == MK_PHILOX || MK == MK_PHILOX_LAW;
  const T scale = MK == MK_PHILOX_LAW ? a.law.scale : (T)(1.0 / (1.0 - MLP_DROPOUT_DEFAULT));

  // the row block of X, once: rows past N and columns past n_in are zero
  for (int e = tid; e < PF_ROWS * a.xk; e += PF_NT) {
    const int r = e / a.xk, c = e - r * a.xk;
    Xs[(size_t)r * xp + c] = (m0 + r < N && c < a.n_in) ? a.X[(size_t)(m0 + r) * a.n_in + c] : T(0);
  }
  // first flag group of each mask's 16-row range (which·mn + m0·n_mid … + 16·n_mid)
  size_t elo[3];
#pragma unroll
  for (int w = 0; w < 3; ++w) elo[w] = (size_t)w * mn + (size_t)m0 * nm;
  const int ngr = PF_ROWS * nm / 64 + 1;                       // groups that cover a range of any alignment

  // mask value `which` of element (row lr, column n) for draw d
  auto mask = [&](int which, int d, int n) -> T {
    if constexpr (MK == MK_VALS) {
      return rok ? a.masks[((size_t)d * 3 + which) * mn + (size_t)(m0 + lr) * nm + n] : T(1);
    } else if constexpr (PHILOX) {
      const size_t e = elo[which] + (size_t)lr * nm + n;
      const uint32_t wd = kw[which * PF_KWN + (int)((e >> 5) - ((elo[which] >> 6) << 1))];
      return ((wd >> (e & 31)) & 1u) ? scale : T(0);
    } else {
      return T(1);
    }
  };

  // the (row r, class o) pair of the softmax stage and its float64 partials over this group's draws
  const int sr = tid >> 4, so = tid & 15;
  const bool srow = tid < 256 && m0 + sr < N;
  const int32_t yv = (a.y && srow) ? a.y[m0 + sr] : -1;
  double accp = 0.0, accH = 0.0, accpy = 0.0;

  const int g = blockIdx.y, d0 = g * a.dpg, d1 = min(a.D, d0 + a.dpg);
  for (int d = d0; d < d1; ++d) {
    const int s = d / a.Tn;
    const T* W1 = a.p[0] + (size_t)s * nm * a.n_in;
    const T* b1 = a.p[1] + (size_t)s * nm;
    const T* W2 = a.p[2] + (size_t)s * nm * nm;
    const T* b2 = a.p[3] + (size_t)s * nm;
    const T* W3 = a.p[4] + (size_t)s * No * nm;
    const T* b3 = a.p[5] + (size_t)s * No;
    if constexpr (PHILOX) {                                    // the draw's keep flags of this row block
      if (tid < 3 * ngr) {
        const int w = tid / ngr, gi = tid - w * ngr;
        const uint32_t G = (uint32_t)(elo[w] >> 6) + (uint32_t)gi, slot = a.slot0 + (uint32_t)d;
        const KeepGroup k = MK == MK_PHILOX_LAW ? pred_keep_group_law(a.law.keep, a.seed, G, slot, a.step, a.chain)
                                                : pred_keep_group_default(a.seed, G, slot, a.step, a.chain);
        kw[w * PF_KWN + 2 * gi] = k.lo;
        kw[w * PF_KWN + 2 * gi + 1] = k.hi;
      }
    }
    __syncthreads();                                           // X tile (first draw) and keep words are in LDS

    // layer 1: h1ᵀ[n][r] = max((Σ_k W1[n][k]·X[r][k] + b1[n])·m0[r][n], 0)
    if (wact) {
      typename Mf::acc_t acc[2] = {Mf::zero(), Mf::zero()};
      T bb[2][4], mk[2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n0 + 16 * j + Mf::row(lane, q);
          bb[j][q] = b1[n];
          mk[j][q] = mask(0, d, n);
        }
      pf_gemm<T>(acc, W1, a.n_in, a.n_in, a.xk, n0, Xs, xp, lr, lg);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n0 + 16 * j + Mf::row(lane, q);
          const T t = (acc[j][q] + bb[j][q]) * mk[j][q];
          H1[(size_t)lr * hp + n] = t > T(0) ? t : T(0);
        }
    }
    __syncthreads();

    // layer 2: h2 = max((h1·W2ᵀ + b2)·m1, 0), d3 = h2·m2
    if (wact) {
      typename Mf::acc_t acc[2] = {Mf::zero(), Mf::zero()};
      T bb[2][4], mk1[2][4], mk2[2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n0 + 16 * j + Mf::row(lane, q);
          bb[j][q] = b2[n];
          mk1[j][q] = mask(1, d, n);
          mk2[j][q] = mask(2, d, n);
        }
      pf_gemm<T>(acc, W2, nm, nm, nm, n0, H1, hp, lr, lg);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n0 + 16 * j + Mf::row(lane, q);
          const T t = (acc[j][q] + bb[j][q]) * mk1[j][q];
          const T h = t > T(0) ? t : T(0);
          H2[(size_t)lr * hp + n] = h * mk2[j][q];
        }
    }
    __syncthreads();

    // layer 3: zᵀ[o][r] = Σ_n W3[o][n]·d3[r][n], K = n_mid split over the waves (32 columns each)
    if (wact) {
      typename Mf::acc_t acc = Mf::zero();
      const T* w3 = W3 + (size_t)min(lr, No - 1) * nm;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        T wv[4], hv[4];
        pf_ld16<T>(w3, n0 + 16 * c, lg, wv);
        pf_ld16<T>(H2 + (size_t)lr * hp, n0 + 16 * c, lg, hv);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = Mf::fma(lr < No ? wv[u] : T(0), hv[u], acc);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) zr[((size_t)wave * 16 + Mf::row(lane, q)) * 17 + lr] = acc[q];
    }
    __syncthreads();

    // softmax of the 16 rows, 16 lanes per row (lane `so` = class); float64
    if (tid < 256) {
      const int nwv = nm / 32;
      T zt = T(0);
      for (int w = 0; w < nwv; ++w) zt = w == 0 ? zr[((size_t)w * 16 + so) * 17 + sr] : zt + zr[((size_t)w * 16 + so) * 17 + sr];
      const bool ko = so < No;
      zt = zt + b3[ko ? so : 0];
      const double ninf = -__builtin_huge_val();
      const double v = ko ? (double)zt : ninf;
      double mx = v;
      int arg = so;
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        const double ov = __shfl_xor(mx, m, 16);
        const int oa = __shfl_xor(arg, m, 16);
        // the larger logit, the lower index on ties; a NaN takes over and stays
        const bool take = (mx == mx) && (ov != ov || ov > mx || (ov == mx && oa < arg));
        if (take) { mx = ov; arg = oa; }
      }
      const double tt = v - mx, e = ko ? exp(tt) : 0.0;
      const double ssum = pf_sum16(e), ls = log(ssum), p = e / ssum;
      const double H = pf_sum16((ko && p != 0.0) ? -p * (tt - ls) : 0.0);
      accp += p;
      if (so == 0) accH += H;
      if (a.y) {
        const bool mine = ko && so == yv;
        const double py = pf_sum16(mine ? p : 0.0), nll = pf_sum16(mine ? -(tt - ls) : 0.0);
        if (so == 0) {
          accpy += py;
          rown[sr] = srow ? nll : 0.0;
          rowc[sr] = (srow && arg == yv) ? 1 : 0;
        }
      }
    }
    __syncthreads();
    if (a.y && tid == 0) {                                     // the block's rows in row order
      double sn = 0.0;
      int sc = 0;
      for (int r = 0; r < PF_ROWS; ++r) { sn += rown[r]; sc += rowc[r]; }
      a.nll_part[(size_t)d * nrb + rb] = sn;
      a.corr_part[(size_t)d * nrb + rb] = sc;
    }
    // the next draw's first barrier orders its writes of kw / H1 after this draw's reads; rown / rowc are
    // rewritten only after three more barriers
  }
  if (srow) {
    const size_t row = (size_t)g * N + m0 + sr;
    if (so < No) a.gmean[row * No + so] = accp;
    if (so == 0) {
      a.gH[row] = accH;
      if (a.y) a.gpy[row] = accpy;
    }
  }
}

// The shapes the fused kernel serves — k_fwdr's (hmcx_mlp.hip fwdr_ok: n_mid a multiple of 32 up to 256,
// n_out ≤ 16, n_in a multiple of 8) for either dtype, with 16 rows of X, h1 and d3 inside the LDS.
bool pred_fused_shape_ok(int n_in, int n_mid, int n_out, size_t elt, size_t lds_max) {
  if (n_mid % 32 || n_mid > PF_NMAX || n_out > PF_OMAX || n_in % 8) return false;
  return pf_lds(n_in, n_mid, elt).total <= std::min(lds_max, PF_LDS_MAX);
}

inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// draw groups of the fused launch: the fewest (≤ PF_MAXG, ≤ D) whose workgroups fill at least 90 % of the
// rounds they occupy on `slots` resident workgroups, else the count that fills them best
int pred_groups(int nrb, int D, int slots) {
  int best = 1;
  double beff = 0.0;
  for (int G = 1; G <= std::min(D, PF_MAXG); ++G) {
    const long long wg = (long long)nrb * G, rounds = (wg + slots - 1) / slots;
    const double eff = (double)wg / (double)(rounds * slots);
    if (eff >= 0.9) return G;
    if (eff > beff) { beff = eff; best = G; }
  }
  return best;
}

}  // namespace

// the predictive's own device buffer (see hmcx_ctx::pred_ws)
int pred_reserve(hmcx_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->pred_cap) return HMCX_OK;
  if (ctx->pred_ws) {
    HMCX_HIP(ctx, hipDeviceSynchronize());
    (void)hipFree(ctx->pred_ws);
    ctx->pred_ws = nullptr;
    ctx->pred_cap = 0;
  }
  const size_t want = bytes + bytes / 4 + (1 << 16);
  if (hipMalloc((void**)&ctx->pred_ws, want) != hipSuccess) {
    ctx->pred_ws = nullptr;
    return set_error(ctx, HMCX_ENOMEM, "hipMalloc predictive buffer failed");
  }
  ctx->pred_cap = want;
  return HMCX_OK;
}
bool mlp_pred_fused_ok(const hmcx_ctx* ctx, const hmcx_mlp_predictive_args* a) {
  const size_t elt = a->dtype == HMCX_F64 ? 8 : 4;
  if (!pred_fused_shape_ok(a->n_in, a->n_mid, a->n_out, elt, ctx->lds_max)) return false;
  if (!al16(a->X) || !al16(a->par.p[0]) || !al16(a->par.p[2]) || !al16(a->par.p[4])) return false;
  return true;
}

template <typename T>
int mlp_predictive_t(hmcx_ctx* ctx, const hmcx_mlp_predictive_args* a) {
  const int N = a->N, K = a->n_out, nm = a->n_mid, D = a->S * a->T;
  const size_t mn = (size_t)N * nm;
  // path 0: the fused kernel where it is eligible and there are at least two draws — there it took less
  // device time than the general path and than the per-set loop at every point measured (both dtypes, 16 to
  // 10 000 rows, 2 to 64 draws).  A single draw of a few rows is one workgroup streaming the whole network
  // alone, and lost to the general path by 2 - 8 % (784-256-256-10, 16 and 64 rows), so D = 1 stays general
  // (profiles/predictive_f32.txt)
  const bool fused = a->path == 2 || (a->path == 0 && D >= 2 && mlp_pred_fused_ok(ctx, a));
  const bool want_y = a->y != nullptr;
  const bool want_rows = a->out_mean || a->out_pred || a->out_entropy || a->out_exp_entropy || a->out_lppd;
  const size_t sz[6] = {(size_t)nm * a->n_in, (size_t)nm, (size_t)nm * nm, (size_t)nm, (size_t)K * nm, (size_t)K};
  int rc = HMCX_OK;

  PredFinish fin{};
  fin.N = N; fin.K = K; fin.D = D; fin.y = a->y;
  fin.out_mean = a->out_mean; fin.out_pred = a->out_pred; fin.out_entropy = a->out_entropy;
  fin.out_exp_entropy = a->out_exp_entropy; fin.out_lppd = a->out_lppd;
  const double* nll_part = nullptr;
  const int32_t* corr_part = nullptr;
  int nparts = 0;

  if (!fused) {
    const int nb = (N + PR_NT - 1) / PR_NT;
    Bump bp{nullptr};
    T* z = nullptr; T* mbuf = nullptr; double *gm = nullptr, *gH = nullptr, *gpy = nullptr; int32_t* cp = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
      bp.off = 0;
      z = bp.take<T>((size_t)N * K);
      mbuf = a->mask_mode == HMCX_MLP_MASKS_PHILOX ? bp.take<T>(3 * mn) : nullptr;
      gm = bp.take<double>((size_t)N * K);
      gH = bp.take<double>(N);
      gpy = bp.take<double>(N);
      cp = a->out_draw_correct ? bp.take<int32_t>((size_t)D * nb) : nullptr;
      if (pass == 0) {
        if ((rc = pred_reserve(ctx, bp.off))) return rc;
        bp.base = ctx->pred_ws;
      }
    }
    if ((rc = timing_begin(ctx, ctx->stream))) return rc;      // after the buffers: nothing below fails on size
    for (int d = 0; d < D; ++d) {
      const int s = d / a->T;
      hmcx_mlp_params ps;
      for (int v = 0; v < 6; ++v) ps.p[v] = (T*)a->par.p[v] + (size_t)s * sz[v];
      const void* mk = nullptr;
      if (a->mask_mode == HMCX_MLP_MASKS_FIXED) mk = (const T*)a->masks + (size_t)d * 3 * mn;
      if (a->mask_mode == HMCX_MLP_MASKS_PHILOX) {
        if ((rc = mlp_masks_t<T>(ctx, N, nm, a->seed, a->chain, a->step, a->slot0 + (uint32_t)d, mbuf))) return rc;
        mk = mbuf;
      }
      // the draw's mean cross-entropy is the forward's own (the number hmcx_mlp_loss returns)
      double* nll = a->out_draw_nll ? a->out_draw_nll + d : nullptr;
      if ((rc = mlp_loss_t<T>(ctx, a->X, nll ? a->y : nullptr, N, a->n_in, nm, K, &ps, mk, nll, z))) return rc;
      if (want_rows || cp) {
        hipLaunchKernelGGL(k_pred_reduce<T>, dim3(nb), dim3(PR_NT), 0, ctx->stream, (const T*)z, a->y, N, K,
                           d == 0 ? 1 : 0, gm, gH, gpy, cp ? cp + (size_t)d * nb : nullptr);
        HMCX_HIP(ctx, hipGetLastError());
      }
    }
    fin.G = 1; fin.gmean = gm; fin.gH = gH; fin.gpy = gpy;
    corr_part = cp; nparts = nb;
  } else {
    const int nrb = (N + PF_ROWS - 1) / PF_ROWS;
    const PfLds L = pf_lds(a->n_in, nm, sizeof(T));
    const bool any_law = ctx->mlp_dropout != MLP_DROPOUT_DEFAULT;
    const void* kfn = a->mask_mode == HMCX_MLP_MASKS_PHILOX
                          ? (any_law ? (const void*)k_pred_fused<T, MK_PHILOX_LAW> : (const void*)k_pred_fused<T, MK_PHILOX>)
                      : a->mask_mode == HMCX_MLP_MASKS_FIXED ? (const void*)k_pred_fused<T, MK_VALS>
                                                             : (const void*)k_pred_fused<T, MK_NONE>;
    int per_cu = 0;
    if ((rc = kernel_occupancy(ctx, kfn, PF_NT, (int)L.total, &per_cu))) return rc;
    if (per_cu < 1) return set_error(ctx, HMCX_EUNSUPPORTED, "mlp predictive: the fused kernel does not fit a CU");
    int G = pred_groups(nrb, D, ctx->num_cus * per_cu);
    const int dpg = (D + G - 1) / G;
    G = (D + dpg - 1) / dpg;
    Bump bp{nullptr};
    double *gm = nullptr, *gH = nullptr, *gpy = nullptr, *np = nullptr; int32_t* cp = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
      bp.off = 0;
      gm = bp.take<double>((size_t)G * N * K);
      gH = bp.take<double>((size_t)G * N);
      gpy = bp.take<double>((size_t)G * N);
      np = want_y ? bp.take<double>((size_t)D * nrb) : nullptr;
      cp = want_y ? bp.take<int32_t>((size_t)D * nrb) : nullptr;
      if (pass == 0) {
        if ((rc = pred_reserve(ctx, bp.off))) return rc;
        bp.base = ctx->pred_ws;
      }
    }
    PredFused<T> f{};
    f.N = N; f.n_in = a->n_in; f.n_mid = nm; f.n_out = K; f.Tn = a->T; f.D = D; f.dpg = dpg;
    f.xk = (a->n_in + 15) / 16 * 16;
    f.xp = f.xk + 16 / (int)sizeof(T);
    f.hp = nm + 16 / (int)sizeof(T);
    f.X = (const T*)a->X; f.y = a->y;
    for (int v = 0; v < 6; ++v) f.p[v] = (const T*)a->par.p[v];
    f.masks = (const T*)a->masks;
    f.seed = a->seed; f.chain = a->chain; f.step = a->step; f.slot0 = a->slot0; f.law = drop_law<T>(ctx);
    f.gmean = gm; f.gH = gH; f.gpy = gpy; f.nll_part = np; f.corr_part = cp;
    const dim3 grid((unsigned)nrb, (unsigned)G), block(PF_NT);
    if ((rc = timing_begin(ctx, ctx->stream))) return rc;
    if (a->mask_mode == HMCX_MLP_MASKS_PHILOX && any_law)
      hipLaunchKernelGGL((k_pred_fused<T, MK_PHILOX_LAW>), grid, block, L.total, ctx->stream, f);
    else if (a->mask_mode == HMCX_MLP_MASKS_PHILOX)
      hipLaunchKernelGGL((k_pred_fused<T, MK_PHILOX>), grid, block, L.total, ctx->stream, f);
    else if (a->mask_mode == HMCX_MLP_MASKS_FIXED)
      hipLaunchKernelGGL((k_pred_fused<T, MK_VALS>), grid, block, L.total, ctx->stream, f);
    else
      hipLaunchKernelGGL((k_pred_fused<T, MK_NONE>), grid, block, L.total, ctx->stream, f);
    HMCX_HIP(ctx, hipGetLastError());
    fin.G = G; fin.gmean = gm; fin.gH = gH; fin.gpy = gpy;
    nll_part = np; corr_part = cp; nparts = nrb;
  }

  if (want_rows) {
    hipLaunchKernelGGL(k_pred_finish, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, fin);
    HMCX_HIP(ctx, hipGetLastError());
  }
  if ((nll_part && a->out_draw_nll) || (corr_part && a->out_draw_correct)) {
    hipLaunchKernelGGL(k_pred_draws, dim3((D + 255) / 256), dim3(256), 0, ctx->stream, D, nparts, N, nll_part,
                       corr_part, a->out_draw_nll, a->out_draw_correct);
    HMCX_HIP(ctx, hipGetLastError());
  }
  return timing_end(ctx, ctx->stream);
}

template int mlp_predictive_t<float>(hmcx_ctx*, const hmcx_mlp_predictive_args*);
template int mlp_predictive_t<double>(hmcx_ctx*, const hmcx_mlp_predictive_args*);

}  // namespace hmcx
