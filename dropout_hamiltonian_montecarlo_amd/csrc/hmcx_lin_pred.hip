// hmcx_lin_pred.hip — posterior predictive of the softmax and logistic models (hmcx_linear_predictive): the
// mean class probabilities over S·T draws (S parameter sets × T input-dropout masks), the entropy of the mean,
// the mean entropy of the draws and, with labels, the log pointwise predictive density and each draw's
// −log-likelihood / N and hit count — one call, nothing per draw on the host.  hmcx_mlp_pred.hip is the model.
//
// Draw d = s·T + t: z_d = clip((X ⊙ Z_d)·W_s + b_s) in the call's dtype (k_fwd's arithmetic: bias, then the
// clip of softmax.py:40-41); the softmax / sigmoid of a row and everything summed over draws or rows is
// float64 for both dtypes.  Every sum has a fixed order (no atomics, no exchange between workgroups: what
// crosses workgroups is a partial that a later launch sums in index order), so equal calls give equal bits.
//
// General path (every shape hmcx_softmax_predict accepts): draws in chunks.  Without dropout a chunk is up to
// LG_CHUNK parameter sets, packed [D][chunk·K] (k_lpred_pack) for one k_fwd launch in FWD_PRED mode
// (softmax_predict_t) into the chunk buffer; with dropout a chunk is one draw: k_lpred_xmask writes X ⊙ Z_d,
// then k_fwd on W_s as it lies.  A float32 sigmoid call stores k_fwd's clipped logits instead (FWD_PREDZ) and the
// sigmoid is taken in float64 from them, as on the fused path.  k_lpred_reduce — one thread per row, one wave
// per workgroup — adds p, H[p], p[y] of the chunk's draws to the per-row float64 accumulators in draw order and
// leaves each draw's per-workgroup −log-likelihood and hits; k_lpred_finish / k_lpred_draws end the call.
//
// Fused path (k_lpred_fused; eligibility: lpred_fused_shape_ok): a workgroup owns a 16-row block of X, staged
// in LDS once, and a contiguous group of units.  A unit is what one wave carries through D in LF_NACC
// accumulator tiles of v_mfma_*_16x16x4: without dropout 64 columns = ⌊64 / K⌋ parameter sets side by side
// (k_fwd's chain packing; the A fragment from LDS serves all four tiles), with dropout up to four masks of
// one set (the W_s fragment from global memory serves all four; Z is applied while the A fragment is built).
// The wave writes its clipped logits to its own LDS tile and lanes (row, sub-draw) do the float64 softmax /
// sigmoid; per-row partials stay in registers until the group ends.  Grid: row blocks × groups; the group
// partials [G][N][K] and the per-draw partials [S·T][row blocks] are summed in index order by the finish
// launches.  No probability reaches HBM.
#include "hmcx_common.h"
#include "hmcx_internal.h"
#include "hmcx_xdrop.h"
#include <algorithm>
#include <type_traits>

namespace hmcx {

namespace {

enum { LM_NONE = HMCX_MLP_MASKS_NONE, LM_FIXED = HMCX_MLP_MASKS_FIXED, LM_PHILOX = HMCX_MLP_MASKS_PHILOX };

constexpr int LG_NT = 64;                // rows (threads) per k_lpred_reduce workgroup: one wave
constexpr int LG_CHUNK = 64;             // parameter sets per chunk at most (general path, no dropout)
constexpr size_t LG_CHUNK_BYTES = (size_t)64 << 20;   // … and the chunk buffer [N][chunk·K] stays below this

constexpr int LF_ROWS = 16;              // rows of X per workgroup (one MFMA tile)
constexpr int LF_NW = 4;                 // waves per workgroup, one unit each per round
constexpr int LF_NT = LF_NW * 64;
constexpr int LF_NACC = 4;               // accumulator tiles per unit
constexpr int LF_COLS = 16 * LF_NACC;    // logit columns of a unit
constexpr int LF_ZP = LF_COLS + 1;       // pitch of a wave's logit tile
constexpr int LF_KMAX = 16;              // K ≤ one MFMA tile
constexpr int LF_RED = LF_KMAX + 2;      // per-row partials of a wave: mean[K], H, p[y]
constexpr int LF_MAXG = 32;              // groups at most
constexpr size_t LF_LDS_MAX = 160 * 1024;

// butterfly over the 16 lanes lane & 15 of a lane group: the same order on every lane, so all 16 agree
__device__ inline double lp_sum16(double v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 16);
  return v;
}
__device__ inline int lp_sum16(int v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 16);
  return v;
}

// x·log x with 0·log 0 = 0 (a NaN stays a NaN)
__device__ inline double xlogx(double x) { return x != 0.0 ? x * log(x) : 0.0; }

// Sigmoid-link statistics of one logit or probability p = P(class 1) (logistic.py:53-55, 64-72, 84).
__device__ inline void sig_stats(double p, int yv, double& H, double& py, double& nll, int& hit) {
  const double q = 1.0 - p;
  H = -(xlogx(p) + xlogx(q));
  const double yd = yv == 1 ? 1.0 : 0.0;
  py = yv == 1 ? p : q;
  nll = -(yd * log(p) + (1.0 - yd) * log(q));                  // logistic.py:71
  hit = ((p > 0.5) ? 1 : 0) == yv ? 1 : 0;                     // logistic.py:84
}

// ------------------------------------------------------------------ general path
// Wc[k][c·K + j] = W[c][k][j]: a chunk of parameter sets in k_fwd's chain-interleaved layout.
template <typename T>
__global__ __launch_bounds__(256) void k_lpred_pack(const T* W, T* Wc, int D, int K, int nc) {
  const size_t n = (size_t)D * nc * K;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const size_t k = e / ((size_t)nc * K), cj = e - k * ((size_t)nc * K);
    const size_t c = cj / K, j = cj - c * K;
    Wc[e] = W[(c * D + k) * K + j];
  }
}

// Xd = X ⊙ Z_d (np.multiply(X, Z), softmax.py:97): Z from the FIXED block `keep` or from Philox.
template <typename T>
__global__ __launch_bounds__(256) void k_lpred_xmask(const T* X, T* Xd, int64_t n, const uint8_t* keep, double p,
                                                     uint64_t seed, uint32_t chain, uint32_t step) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool z = keep ? keep[i] != 0 : xdrop_keep(seed, chain, step, (uint32_t)i, p);
  Xd[i] = X[i] * (z ? T(1) : T(0));
}

// The probabilities prob [N][nc·K] of draws d0 … d0 + nc − 1 into the accumulators, in draw order.  sig: 0 the
// softmax link, 1 the sigmoid link on probabilities, 2 the sigmoid link on clipped logits (float32 calls: a
// float32 probability is exactly 1 from z = 17.33 on, and log(1 − p) of it is −inf, 0·log 0 a NaN).
// nll_part / corr_part [S·T][gridDim.x]: each draw's −log-likelihood and hits of this workgroup's rows.
template <typename T>
__global__ __launch_bounds__(LG_NT) void k_lpred_reduce(const T* prob, const int32_t* y, int N, int K, int nc, int d0,
                                                        int sig, double* acc_mean, double* acc_H, double* acc_py,
                                                        double* nll_part, int32_t* corr_part) {
  const int n = blockIdx.x * LG_NT + threadIdx.x;
  const bool rok = n < N;
  const int yv = (y && rok) ? y[n] : -1;
  double aH = 0.0, apy = 0.0;
  if (rok && d0 > 0) { aH = acc_H[n]; if (y) apy = acc_py[n]; }
  for (int c = 0; c < nc; ++c) {
    double H = 0.0, py = 0.0, nll = 0.0;
    int hit = 0;
    if (rok) {
      const T* p = prob + (size_t)n * nc * K + (size_t)c * K;
      double* am = acc_mean + (size_t)n * K;
      const bool first = d0 == 0 && c == 0;
      if (sig) {
        // sig == 2: the chunk holds the clipped logit and p is formed in float64, as the fused kernel does
        const double pk = sig == 2 ? 1.0 / (1.0 + exp(-(double)p[0])) : (double)p[0];   // logistic.py:53-55
        am[0] = first ? pk : am[0] + pk;
        sig_stats(pk, yv, H, py, nll, hit);
      } else {
        double best = 0.0;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
          const double pk = (double)p[k];
          am[k] = first ? pk : am[k] + pk;
          H -= xlogx(pk);
          if (k == yv) py = pk;
          if (k == 0 || pk > best) { best = pk; arg = k; }
        }
        nll = -log(py);
        hit = arg == yv ? 1 : 0;
      }
      aH += H;
      apy += py;
    }
    if (nll_part) {                                            // one wave: a butterfly in a fixed order
      double s = (rok && y) ? nll : 0.0;
      int h = (rok && y) ? hit : 0;
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) { s += __shfl_xor(s, m, 64); h += __shfl_xor(h, m, 64); }
      if (threadIdx.x == 0) {
        nll_part[(size_t)(d0 + c) * gridDim.x + blockIdx.x] = s;
        corr_part[(size_t)(d0 + c) * gridDim.x + blockIdx.x] = h;
      }
    }
  }
  if (rok) { acc_H[n] = aH; if (y) acc_py[n] = apy; }
}

// Per-row results from the G group partials (general path: G = 1), summed in group order.
struct LinFinish {
  int N, K, DR, G, sig;
  const double* gmean; const double* gH; const double* gpy;    // [G][N][K], [G][N], [G][N]
  double* out_mean; int32_t* out_pred; double* out_entropy; double* out_exp_entropy; double* out_lppd;
};
__global__ __launch_bounds__(256) void k_lpred_finish(LinFinish a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.N) return;
  const double DR = (double)a.DR;
  double ent = 0.0, best = 0.0;
  int arg = 0;
  for (int k = 0; k < a.K; ++k) {
    double s = 0.0;
    for (int g = 0; g < a.G; ++g) s = g == 0 ? a.gmean[(size_t)n * a.K + k] : s + a.gmean[((size_t)g * a.N + n) * a.K + k];
    const double m = s / DR;
    if (a.out_mean) a.out_mean[(size_t)n * a.K + k] = m;
    if (a.sig) {
      ent = -(xlogx(m) + xlogx(1.0 - m));
      arg = m > 0.5 ? 1 : 0;                                   // logistic.py:84
    } else {
      ent -= xlogx(m);
      if (k == 0 || m > best) { best = m; arg = k; }
    }
  }
  if (a.out_pred) a.out_pred[n] = arg;
  if (a.out_entropy) a.out_entropy[n] = ent;
  if (a.out_exp_entropy) {
    double s = 0.0;
    for (int g = 0; g < a.G; ++g) s = g == 0 ? a.gH[n] : s + a.gH[(size_t)g * a.N + n];
    a.out_exp_entropy[n] = s / DR;
  }
  if (a.out_lppd) {
    double s = 0.0;
    for (int g = 0; g < a.G; ++g) s = g == 0 ? a.gpy[n] : s + a.gpy[(size_t)g * a.N + n];
    a.out_lppd[n] = log(s / DR);
  }
}

// Per-draw results from the per-workgroup partials [S·T][np], summed in workgroup order.
__global__ __launch_bounds__(256) void k_lpred_draws(int DR, int np, int N, const double* nll_part,
                                                     const int32_t* corr_part, double* out_nll, int32_t* out_correct) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= DR) return;
  double s = 0.0;
  int c = 0;
  for (int b = 0; b < np; ++b) { s += nll_part[(size_t)d * np + b]; c += corr_part[(size_t)d * np + b]; }
  if (out_nll) out_nll[d] = s / (double)N;
  if (out_correct) out_correct[d] = c;
}

// ------------------------------------------------------------------ the fused row-block kernel
template <typename T> struct LinFused {
  int N, D, K, S, Tn, sig;
  int Dp, xp;                                                  // D rounded up to 16; LDS pitch of the X tile (elements)
  int nunits, upg, nit;                                        // units in all, per group, rounds of LF_NW per group
  int spu, tu;                                                 // no dropout: sets per unit; dropout: units per set
  const T* X; const int32_t* y; const T* W; const T* b;
  const T* zeros;                                              // a few zero words (hmcx_ctx::zeros_dev)
  const uint8_t* masks;                                        // LM_FIXED
  double keep_p; uint64_t seed; uint32_t chain, step0;         // LM_PHILOX
  T clip_hi, clip_lo;
  double* gmean; double* gH; double* gpy;                      // group partials [G][N][K], [G][N], [G][N]
  double* nll_part; int32_t* corr_part;                        // [S·T][row blocks], null without labels
};

// LDS layout of k_lpred_fused (bytes): X tile, per-wave logit tiles, per-wave row partials.
struct LfLds { size_t xs, zs, red, total; };
__host__ __device__ inline size_t lf_up16(size_t bytes) { return (bytes + 15) / 16 * 16; }
__host__ __device__ inline LfLds lf_lds(int D, size_t elt) {
  const size_t Dp = (size_t)((D + 15) / 16) * 16, xp = Dp + 16 / elt;
  LfLds l;
  l.xs = 0;
  l.zs = l.xs + lf_up16(LF_ROWS * xp * elt);
  l.red = l.zs + lf_up16((size_t)LF_NW * LF_ROWS * LF_ZP * elt);
  l.total = l.red + lf_up16((size_t)LF_NW * LF_ROWS * LF_RED * 8);
  return l;
}

// x[u] = P[u] for u = 0 … 3, P 16-byte aligned (LDS)
__device__ inline void lf_ld4(const float* P, float (&x)[4]) {
  const float4 v = *reinterpret_cast<const float4*>(P);
  x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
}
__device__ inline void lf_ld4(const double* P, double (&x)[4]) {
  const double2 v = *reinterpret_cast<const double2*>(P), w = *reinterpret_cast<const double2*>(P + 2);
  x[0] = v.x; x[1] = v.y; x[2] = w.x; x[3] = w.y;
}

template <typename T, int MK>
__global__ __launch_bounds__(LF_NT) void k_lpred_fused(LinFused<T> a) {
  using Mf = mfma16<T>;
  extern __shared__ __attribute__((aligned(16))) char lf_smem[];
  const LfLds L = lf_lds(a.D, sizeof(T));
  T* Xs = reinterpret_cast<T*>(lf_smem + L.xs);
  T* zs = reinterpret_cast<T*>(lf_smem + L.zs);                // [wave][row][LF_ZP]
  double* red = reinterpret_cast<double*>(lf_smem + L.red);    // [wave][row][LF_RED]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int N = a.N, D = a.D, K = a.K, xp = a.xp;
  const int rb = blockIdx.x, m0 = rb * LF_ROWS, nrb = gridDim.x, grp = blockIdx.y;
  const bool rok = m0 + r < N;                                 // the row this lane loads (A) and scores
  const int32_t yv = (a.y && rok) ? a.y[m0 + r] : -1;
  T* zw = zs + (size_t)wave * LF_ROWS * LF_ZP;

  // the row block of X, once: rows past N and columns past D are zero
  for (int e = tid; e < LF_ROWS * a.Dp; e += LF_NT) {
    const int i = e / a.Dp, c = e - i * a.Dp;
    Xs[(size_t)i * xp + c] = (m0 + i < N && c < D) ? a.X[(size_t)(m0 + i) * D + c] : T(0);
  }
  __syncthreads();

  double accp[LF_KMAX], accH = 0.0, accpy = 0.0;               // this lane's sub-draws of row r
#pragma unroll
  for (int k = 0; k < LF_KMAX; ++k) accp[k] = 0.0;

  const int u0 = grp * a.upg, u1 = min(a.nunits, u0 + a.upg);
  for (int it = 0; it < a.nit; ++it) {
    const int u = u0 + it * LF_NW + wave;
    const bool active = u < u1;                                // wave-uniform
    int s0 = 0, t0 = 0, nsub = 0;                              // first set, first mask, sub-draws of the unit
    if (active) {
      if constexpr (MK == LM_NONE) { s0 = u * a.spu; nsub = min(a.spu, a.S - s0); }
      else { s0 = u / a.tu; t0 = (u - s0 * a.tu) * LF_NACC; nsub = min(LF_NACC, a.Tn - t0); }
      typename Mf::acc_t acc[LF_NACC];
#pragma unroll
      for (int q = 0; q < LF_NACC; ++q) acc[q] = Mf::zero();
      // the lane's column of each tile: (set, class), its W column and the stride along d — a column without a
      // class reads the context's zero words at stride 0, so no load in the loop is conditional
      const T* wp[LF_NACC];
      int wst[LF_NACC];
      T bias[LF_NACC];
#pragma unroll
      for (int q = 0; q < LF_NACC; ++q) {
        int j, kk;
        bool cok;
        if constexpr (MK == LM_NONE) { const int col = 16 * q + r; j = col / K; kk = col - j * K; cok = j < nsub; }
        else { j = 0; kk = r; cok = r < K && q < nsub; }
        wp[q] = cok ? a.W + (size_t)(s0 + j) * D * K + kk : a.zeros;
        wst[q] = cok ? K : 0;
        bias[q] = cok ? a.b[(size_t)(s0 + j) * K + kk] : T(0);
      }
      const T* xr = Xs + (size_t)r * xp;
      const size_t xrow = (size_t)min(m0 + r, N - 1) * D;      // element index of X[m0 + r][0] (clamped past N)
      // one 16-d chunk; TAIL: the last, partial one (d past D reads row D − 1 and counts as zero; the X tile is
      // zero there too, so a mask flag of such an element is never used)
      auto chunk = [&](int k0, auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        const int kb = k0 + 4 * g;
        T xa[4];
        lf_ld4(xr + kb, xa);
        int kd[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) kd[v] = TAIL ? min(kb + v, D - 1) : kb + v;
        if constexpr (MK == LM_NONE) {
          T bv[LF_NACC][4];
#pragma unroll
          for (int q = 0; q < LF_NACC; ++q)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const T w = wp[q][kd[v] * wst[q]];
              bv[q][v] = (!TAIL || kb + v < D) ? w : T(0);
            }
#pragma unroll
          for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int q = 0; q < LF_NACC; ++q) acc[q] = Mf::fma(xa[v], bv[q][v], acc[q]);
        } else {
          T bv[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const T w = wp[0][kd[v] * wst[0]];
            bv[v] = (!TAIL || kb + v < D) ? w : T(0);
          }
#pragma unroll
          for (int q = 0; q < LF_NACC; ++q) {
            if (q < nsub) {                                    // wave-uniform
              const size_t d = (size_t)s0 * a.Tn + t0 + q;
#pragma unroll
              for (int v = 0; v < 4; ++v) {
                const size_t e = xrow + kd[v];
                bool z;
                if constexpr (MK == LM_FIXED) z = a.masks[d * N * D + e] != 0;
                else z = xdrop_keep(a.seed, a.chain, a.step0 + (uint32_t)d, (uint32_t)e, a.keep_p);
                acc[q] = Mf::fma(xa[v] * (z ? T(1) : T(0)), bv[v], acc[q]);
              }
            }
          }
        }
      };
      const int Dfull = D & ~15;
      for (int k0 = 0; k0 < Dfull; k0 += 16) chunk(k0, std::false_type{});
      if (Dfull < D) chunk(Dfull, std::true_type{});
      // z = clip(XW + b) in T (k_fwd pass 1), into the wave's tile
#pragma unroll
      for (int q = 0; q < LF_NACC; ++q)
#pragma unroll
        for (int v = 0; v < 4; ++v)
          zw[Mf::row(lane, v) * LF_ZP + 16 * q + r] = clipz(acc[q][v] + bias[q], a.clip_hi, a.clip_lo);
    }
    __syncthreads();                                           // the tile is written
    if (active) {
      const int cstride = MK == LM_NONE ? K : 16;
      for (int jj = 0; 4 * jj < nsub; ++jj) {                  // wave-uniform bound; lane group g takes sub-draw g + 4·jj
        const int j = g + 4 * jj;
        const bool valid = j < nsub;
        const T* zr = zw + r * LF_ZP + (valid ? j : 0) * cstride;
        const size_t d = MK == LM_NONE ? (size_t)(s0 + j) : (size_t)s0 * a.Tn + t0 + j;
        double H = 0.0, py = 0.0, nll = 0.0;
        int hit = 0;
        if (a.sig) {
          const double p = 1.0 / (1.0 + exp(-(double)zr[0]));  // logistic.py:53-55
          sig_stats(p, yv, H, py, nll, hit);
          if (valid) accp[0] += p;
        } else {
          double zv[LF_KMAX];
#pragma unroll
          for (int k = 0; k < LF_KMAX; ++k) zv[k] = (double)zr[k < K ? k : 0];
          double mx = zv[0];
          int arg = 0;
#pragma unroll
          for (int k = 1; k < LF_KMAX; ++k)
            if (k < K) {
              if (zv[k] > mx) { mx = zv[k]; arg = k; }
              else if (zv[k] != zv[k]) mx = zv[k];             // NaN: the whole row is NaN
            }
          double e[LF_KMAX], sum = 0.0;
#pragma unroll
          for (int k = 0; k < LF_KMAX; ++k) {
            e[k] = k < K ? exp(zv[k] - mx) : 0.0;
            if (k < K) sum += e[k];
          }
          const double ls = log(sum);
#pragma unroll
          for (int k = 0; k < LF_KMAX; ++k)
            if (k < K) {
              const double t = zv[k] - mx, p = e[k] / sum;
              if (p != 0.0) H -= p * (t - ls);
              if (k == yv) { py = p; nll = -(t - ls); }        // softmax.py:17-20
              if (valid) accp[k] += p;
            }
          hit = arg == yv ? 1 : 0;
        }
        if (valid) { accH += H; accpy += py; }
        if (a.y) {                                             // the block's rows of this draw, lane-group butterfly
          const bool in = valid && rok;
          const double sn = lp_sum16(in ? nll : 0.0);
          const int sc = lp_sum16(in ? hit : 0);
          if (valid && r == 0) {
            a.nll_part[d * nrb + rb] = sn;
            a.corr_part[d * nrb + rb] = sc;
          }
        }
      }
    }
    __syncthreads();                                           // the tile is free for the next round
  }

  // the lane groups of a wave, then the waves in wave order
#pragma unroll
  for (int k = 0; k < LF_KMAX; ++k)
    if (k < K) {
      accp[k] += __shfl_xor(accp[k], 16, 64);
      accp[k] += __shfl_xor(accp[k], 32, 64);
    }
  accH += __shfl_xor(accH, 16, 64);
  accH += __shfl_xor(accH, 32, 64);
  accpy += __shfl_xor(accpy, 16, 64);
  accpy += __shfl_xor(accpy, 32, 64);
  if (g == 0) {
    double* rw = red + ((size_t)wave * LF_ROWS + r) * LF_RED;
#pragma unroll
    for (int k = 0; k < LF_KMAX; ++k) rw[k] = accp[k];
    rw[LF_KMAX] = accH;
    rw[LF_KMAX + 1] = accpy;
  }
  __syncthreads();
  for (int e = tid; e < LF_ROWS * (K + 2); e += LF_NT) {
    const int i = e / (K + 2), c = e - i * (K + 2);
    if (m0 + i >= N) continue;
    const int src = c < K ? c : LF_KMAX + (c - K);
    double s = red[(size_t)i * LF_RED + src];
#pragma unroll
    for (int w = 1; w < LF_NW; ++w) s += red[((size_t)w * LF_ROWS + i) * LF_RED + src];
    const size_t row = (size_t)grp * N + m0 + i;
    if (c < K) a.gmean[row * K + c] = s;
    else if (c == K) a.gH[row] = s;
    else if (a.y) a.gpy[row] = s;
  }
}

// The shapes the fused kernel serves: K within one MFMA tile, and 16 rows of X with the waves' logit tiles
// and row partials inside the LDS.  Python twin: tests/_linear_predictive_ref.py::fused_eligible.
bool lpred_fused_shape_ok(int D, int K, size_t elt, size_t lds_max) {
  if (K < 1 || K > LF_KMAX || D < 1) return false;
  return lf_lds(D, elt).total <= std::min(lds_max, LF_LDS_MAX);
}

// groups of the fused launch: the fewest (≤ LF_MAXG, ≤ units) whose workgroups fill at least 90 % of the rounds
// they occupy on `slots` resident workgroups, else the count that fills them best (hmcx_mlp_pred.hip's rule)
int lpred_groups(int nrb, int nunits, int slots) {
  int best = 1;
  double beff = 0.0;
  for (int G = 1; G <= std::min(nunits, LF_MAXG); ++G) {
    const long long wg = (long long)nrb * G, rounds = (wg + slots - 1) / slots;
    const double eff = (double)wg / (double)(rounds * slots);
    if (eff >= 0.9) return G;
    if (eff > beff) { beff = eff; best = G; }
  }
  return best;
}

}  // namespace

bool lin_pred_fused_ok(const hmcx_ctx* ctx, const hmcx_linear_predictive_args* a) {
  return lpred_fused_shape_ok(a->D, a->K, a->dtype == HMCX_F64 ? 8 : 4, ctx->lds_max);
}

// path 0 (profiles/linear_predictive.txt): the fused kernel only where it measured no slower than
// the general path and than hmcx_softmax_predict + a device mean.  Without dropout that was wherever the launch
// has at least LP_FUSED_MIN_UNITS units per row block (a workgroup's four waves all have one) and either at
// least LP_FUSED_MIN_TASKS row-block × unit pairs (below, one launch of k_fwd over all sets is the shorter
// chain) or at least LP_FUSED_MIN_SETS parameter sets (both other routes grow with every set);
// with input dropout, at the points measured, 32 draws and more.
constexpr long long LP_FUSED_MIN_UNITS = 4, LP_FUSED_MIN_TASKS = 1536, LP_FUSED_MIN_SETS = 200, LP_FUSED_MIN_DRAWS = 32;
static bool lin_pred_path0_fused(const hmcx_ctx* ctx, const hmcx_linear_predictive_args* a) {
  if (!lin_pred_fused_ok(ctx, a)) return false;
  if (a->mask_mode != HMCX_MLP_MASKS_NONE) return (long long)a->S * a->T >= LP_FUSED_MIN_DRAWS;
  const long long spu = LF_COLS / a->K, nunits = (a->S + spu - 1) / spu, nrb = (a->N + LF_ROWS - 1) / LF_ROWS;
  return nunits >= LP_FUSED_MIN_UNITS && (nrb * nunits >= LP_FUSED_MIN_TASKS || a->S >= LP_FUSED_MIN_SETS);
}

template <typename T>
int lin_predictive_t(hmcx_ctx* ctx, const hmcx_linear_predictive_args* a) {
  const int N = a->N, D = a->D, K = a->K, S = a->S, Tn = a->T, DR = S * Tn;
  const int sig = a->model == HMCX_MODEL_LOGISTIC ? 1 : 0;
  const bool drop = a->mask_mode != HMCX_MLP_MASKS_NONE;
  const bool fused = a->path == 2 || (a->path == 0 && lin_pred_path0_fused(ctx, a));
  const bool want_y = a->y != nullptr;
  const bool want_rows = a->out_mean || a->out_pred || a->out_entropy || a->out_exp_entropy || a->out_lppd;
  const bool want_draws = a->out_draw_nll || a->out_draw_correct;
  const T* X = (const T*)a->X;
  const T* W = (const T*)a->W;
  const T* b = (const T*)a->b;
  hipStream_t st = ctx->stream;
  int rc = HMCX_OK;

  LinFinish fin{};
  fin.N = N; fin.K = K; fin.DR = DR; fin.sig = sig;
  fin.out_mean = a->out_mean; fin.out_pred = a->out_pred; fin.out_entropy = a->out_entropy;
  fin.out_exp_entropy = a->out_exp_entropy; fin.out_lppd = a->out_lppd;
  const double* nll_part = nullptr;
  const int32_t* corr_part = nullptr;
  int nparts = 0;

  if (!fused) {
    const int nb = (N + LG_NT - 1) / LG_NT;
    int CH = 1;
    if (!drop) {
      const size_t per = (size_t)N * K * sizeof(T);
      CH = (int)std::max<size_t>(1, std::min<size_t>({(size_t)LG_CHUNK, LG_CHUNK_BYTES / per, (size_t)S}));
    }
    Bump bp{nullptr};
    T *prob = nullptr, *Wc = nullptr, *xd = nullptr;
    double *gm = nullptr, *gH = nullptr, *gpy = nullptr, *np = nullptr;
    int32_t* cp = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
      bp.off = 0;
      prob = bp.take<T>((size_t)N * CH * K);
      Wc = CH > 1 ? bp.take<T>((size_t)D * CH * K) : nullptr;
      xd = drop ? bp.take<T>((size_t)N * D) : nullptr;
      gm = bp.take<double>((size_t)N * K);
      gH = bp.take<double>(N);
      gpy = bp.take<double>(N);
      np = want_draws ? bp.take<double>((size_t)DR * nb) : nullptr;
      cp = want_draws ? bp.take<int32_t>((size_t)DR * nb) : nullptr;
      if (pass == 0) {
        if ((rc = pred_reserve(ctx, bp.off))) return rc;
        bp.base = ctx->pred_ws;
      }
    }
    if ((rc = timing_begin(ctx, st))) return rc;               // after the buffers: nothing below fails on size
    const int link = sig ? LINK_SIGMOID : LINK_SOFTMAX;
    // float32 sigmoid: the chunk buffer takes k_fwd's clipped logits, and k_lpred_reduce forms p in float64
    // (the float64 call keeps the probability: it is the same double either way)
    const bool zsig = sig && sizeof(T) == 4;
    for (int d0 = 0; d0 < DR; d0 += CH) {
      const int nc = std::min(CH, DR - d0);
      const T* Xc = X;
      const T* Ws = W + (size_t)(d0 / Tn) * D * K;             // no dropout: Tn = 1, set d0
      if (drop) {
        const int64_t n = (int64_t)N * D;
        const uint8_t* keep = a->mask_mode == HMCX_MLP_MASKS_FIXED ? a->masks + (size_t)d0 * N * D : nullptr;
        hipLaunchKernelGGL(k_lpred_xmask<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, X, xd, n, keep,
                           a->keep_p, a->seed, a->chain, a->step0 + (uint32_t)d0);
        HMCX_HIP(ctx, hipGetLastError());
        Xc = xd;
      } else if (nc > 1) {
        const size_t n = (size_t)D * nc * K;
        hipLaunchKernelGGL(k_lpred_pack<T>, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                           Ws, Wc, D, K, nc);
        HMCX_HIP(ctx, hipGetLastError());
        Ws = Wc;
      }
      if ((rc = softmax_predict_t<T>(ctx, Xc, N, D, K, nc, Ws, b + (size_t)(d0 / Tn) * K, prob, link, zsig))) return rc;
      if (want_rows || want_draws) {
        hipLaunchKernelGGL(k_lpred_reduce<T>, dim3(nb), dim3(LG_NT), 0, st, (const T*)prob, a->y, N, K, nc, d0,
                           zsig ? 2 : sig, gm, gH, gpy, np, cp);
        HMCX_HIP(ctx, hipGetLastError());
      }
    }
    fin.G = 1; fin.gmean = gm; fin.gH = gH; fin.gpy = gpy;
    nll_part = np; corr_part = cp; nparts = nb;
  } else {
    const int nrb = (N + LF_ROWS - 1) / LF_ROWS;
    const LfLds L = lf_lds(D, sizeof(T));
    const void* kfn = a->mask_mode == HMCX_MLP_MASKS_PHILOX ? (const void*)k_lpred_fused<T, LM_PHILOX>
                      : a->mask_mode == HMCX_MLP_MASKS_FIXED ? (const void*)k_lpred_fused<T, LM_FIXED>
                                                             : (const void*)k_lpred_fused<T, LM_NONE>;
    int per_cu = 0;
    if ((rc = kernel_occupancy(ctx, kfn, LF_NT, (int)L.total, &per_cu))) return rc;
    if (per_cu < 1) return set_error(ctx, HMCX_EUNSUPPORTED, "linear predictive: the fused kernel does not fit a CU");
    LinFused<T> f{};
    f.N = N; f.D = D; f.K = K; f.S = S; f.Tn = Tn; f.sig = sig;
    f.Dp = (D + 15) / 16 * 16;
    f.xp = f.Dp + 16 / (int)sizeof(T);
    f.spu = LF_COLS / K;
    f.tu = (Tn + LF_NACC - 1) / LF_NACC;
    f.nunits = drop ? S * f.tu : (S + f.spu - 1) / f.spu;
    // units per group: whole rounds of LF_NW waves once a group has more than one round
    int G = lpred_groups(nrb, f.nunits, ctx->num_cus * per_cu);
    f.upg = (f.nunits + G - 1) / G;
    if (f.upg > LF_NW) f.upg = (f.upg + LF_NW - 1) / LF_NW * LF_NW;
    G = (f.nunits + f.upg - 1) / f.upg;
    f.nit = (f.upg + LF_NW - 1) / LF_NW;
    Bump bp{nullptr};
    double *gm = nullptr, *gH = nullptr, *gpy = nullptr, *np = nullptr;
    int32_t* cp = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
      bp.off = 0;
      gm = bp.take<double>((size_t)G * N * K);
      gH = bp.take<double>((size_t)G * N);
      gpy = bp.take<double>((size_t)G * N);
      np = want_y ? bp.take<double>((size_t)DR * nrb) : nullptr;
      cp = want_y ? bp.take<int32_t>((size_t)DR * nrb) : nullptr;
      if (pass == 0) {
        if ((rc = pred_reserve(ctx, bp.off))) return rc;
        bp.base = ctx->pred_ws;
      }
    }
    f.X = X; f.y = a->y; f.W = W; f.b = b; f.masks = a->masks;
    f.zeros = (const T*)ctx->zeros_dev;
    f.keep_p = a->keep_p; f.seed = a->seed; f.chain = a->chain; f.step0 = a->step0;
    f.clip_hi = (T)CLIP_HI; f.clip_lo = (T)CLIP_LO;
    f.gmean = gm; f.gH = gH; f.gpy = gpy; f.nll_part = np; f.corr_part = cp;
    const dim3 grid((unsigned)nrb, (unsigned)G), block(LF_NT);
    if ((rc = timing_begin(ctx, st))) return rc;
    if (a->mask_mode == HMCX_MLP_MASKS_PHILOX)
      hipLaunchKernelGGL((k_lpred_fused<T, LM_PHILOX>), grid, block, L.total, st, f);
    else if (a->mask_mode == HMCX_MLP_MASKS_FIXED)
      hipLaunchKernelGGL((k_lpred_fused<T, LM_FIXED>), grid, block, L.total, st, f);
    else
      hipLaunchKernelGGL((k_lpred_fused<T, LM_NONE>), grid, block, L.total, st, f);
    HMCX_HIP(ctx, hipGetLastError());
    fin.G = G; fin.gmean = gm; fin.gH = gH; fin.gpy = gpy;
    nll_part = np; corr_part = cp; nparts = nrb;
  }

  if (want_rows) {
    hipLaunchKernelGGL(k_lpred_finish, dim3((N + 255) / 256), dim3(256), 0, st, fin);
    HMCX_HIP(ctx, hipGetLastError());
  }
  if (nll_part && want_draws) {
    hipLaunchKernelGGL(k_lpred_draws, dim3((DR + 255) / 256), dim3(256), 0, st, DR, nparts, N, nll_part, corr_part,
                       a->out_draw_nll, a->out_draw_correct);
    HMCX_HIP(ctx, hipGetLastError());
  }
  return timing_end(ctx, st);
}

template int lin_predictive_t<float>(hmcx_ctx*, const hmcx_linear_predictive_args*);
template int lin_predictive_t<double>(hmcx_ctx*, const hmcx_linear_predictive_args*);

__global__ __launch_bounds__(256) void k_input_masks(int64_t n, double p, uint64_t seed, uint32_t chain, uint32_t step,
                                                     uint8_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = xdrop_keep(seed, chain, step, (uint32_t)i, p) ? 1 : 0;
}

}  // namespace hmcx

using namespace hmcx;

extern "C" {

int hmcx_linear_predictive(hmcx_ctx* ctx, const hmcx_linear_predictive_args* a) {
  if (!ctx) return HMCX_EINVAL;
  const std::string who = "linear predictive: ";
  if (!a) return set_error(ctx, HMCX_EINVAL, who + "null args");
  if (a->dtype != HMCX_F32 && a->dtype != HMCX_F64) return set_error(ctx, HMCX_EINVAL, who + "dtype must be HMCX_F32/HMCX_F64");
  if (a->model != HMCX_MODEL_SOFTMAX && a->model != HMCX_MODEL_LOGISTIC)
    return set_error(ctx, HMCX_EINVAL, who + "model must be HMCX_MODEL_SOFTMAX or HMCX_MODEL_LOGISTIC");
  if (a->N < 1 || a->D < 1 || a->K < 1 || a->S < 1 || a->T < 1)
    return set_error(ctx, HMCX_EINVAL, who + "N, D, K, S and T must be >= 1");
  if (a->model == HMCX_MODEL_LOGISTIC && a->K != 1) return set_error(ctx, HMCX_EINVAL, who + "logistic needs K = 1");
  if (a->K > 64) return set_error(ctx, HMCX_EUNSUPPORTED, who + "K > 64 classes not built");
  const long long DR = (long long)a->S * a->T;
  if (DR > 0x7fffffffLL || (long long)a->N * a->K > 0x7fffffffLL || (long long)a->D * a->K > 0x7fffffffLL)
    return set_error(ctx, HMCX_EUNSUPPORTED, who + "too many draws, rows or parameters");
  if (!a->X || !a->W || !a->b) return set_error(ctx, HMCX_EINVAL, who + "null pointer");
  if (a->mask_mode != HMCX_MLP_MASKS_NONE && a->mask_mode != HMCX_MLP_MASKS_FIXED &&
      a->mask_mode != HMCX_MLP_MASKS_PHILOX)
    return set_error(ctx, HMCX_EINVAL, who + "bad mask_mode");
  if (a->mask_mode == HMCX_MLP_MASKS_NONE && a->T != 1)
    return set_error(ctx, HMCX_EINVAL, who + "without dropout every draw of a set is the same (T must be 1)");
  if (a->mask_mode == HMCX_MLP_MASKS_FIXED && !a->masks) return set_error(ctx, HMCX_EINVAL, who + "FIXED masks required");
  if (a->mask_mode == HMCX_MLP_MASKS_PHILOX) {
    if ((unsigned long long)a->N * (unsigned long long)a->D >= 0x100000000ULL)
      return set_error(ctx, HMCX_EINVAL, who + "PHILOX masks need N*D < 2^32");
    if ((unsigned long long)a->step0 + (unsigned long long)DR > 0x100000000ULL)
      return set_error(ctx, HMCX_EINVAL, who + "step0 + S*T wraps 2^32");
    if (!(a->keep_p >= 0.0 && a->keep_p <= 1.0)) return set_error(ctx, HMCX_EINVAL, who + "keep_p must be in [0, 1]");
  }
  if (!a->y && (a->out_lppd || a->out_draw_nll || a->out_draw_correct))
    return set_error(ctx, HMCX_EINVAL, who + "lppd / draw_nll / draw_correct need labels");
  if (a->path < 0 || a->path > 2) return set_error(ctx, HMCX_EINVAL, who + "path must be 0, 1 or 2");
  if (a->path == 2 && !lin_pred_fused_ok(ctx, a))
    return set_error(ctx, HMCX_EUNSUPPORTED, who + "shape not eligible for the fused path");
  return a->dtype == HMCX_F64 ? lin_predictive_t<double>(ctx, a) : lin_predictive_t<float>(ctx, a);
}

int hmcx_input_masks(hmcx_ctx* ctx, int N, int D, double keep_p, uint64_t seed, uint32_t chain, uint32_t step,
                     uint8_t* out) {
  if (!ctx) return HMCX_EINVAL;
  if (N < 1 || D < 1) return set_error(ctx, HMCX_EINVAL, "input masks: N and D must be >= 1");
  if ((unsigned long long)N * (unsigned long long)D >= 0x100000000ULL)
    return set_error(ctx, HMCX_EINVAL, "input masks: N*D must be below 2^32");
  if (!out) return set_error(ctx, HMCX_EINVAL, "input masks: null pointer");
  const int64_t n = (int64_t)N * D;
  hipLaunchKernelGGL(k_input_masks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, keep_p, seed, chain,
                     step, out);
  HMCX_HIP(ctx, hipGetLastError());
  return HMCX_OK;
}

}  // extern "C"
