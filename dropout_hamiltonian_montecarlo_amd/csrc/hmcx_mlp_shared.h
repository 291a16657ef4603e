// hmcx_mlp_shared.h — the rest of what the MLP's compile units share, behind hmcx_mlp_kernels.h: the SGD / SGLD
// update kernels, the net of one forward / backward (MlpNet), prototypes of the launch helpers that hmcx_mlp.hip
// defines and the launch group of the two chain schedules (ChainGroup, host only).  A unit that sees only the
// prototypes (hmcx_mlp_chains.hip, hmcx_mlp_hmc_chains.hip) instantiates none of the kernels they launch.
// hmcx_mlp.hip includes it behind its own static kernels: those are emitted in definition order.
#pragma once
#include "hmcx_mlp_kernels.h"
#include <vector>

namespace hmcx {
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
  DropLaw<T> law;
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
      if (g * 64 < (size_t)a.n3) mlp_masks_group<T>(a.law, a.masks, a.n3, a.seed, a.chain, a.step, a.slot, (int)g);
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
  DropLaw<T> law;
};
// The one-chain kernel: k_mlp_sgld_chains's statements (hmcx_mlp_chains.hip) without the chain offsets (sharing
// one body cost it 2 – 3 SGPRs); keep the two in step.
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
      if (g * 64 < (size_t)a.n3) mlp_masks_group<T>(a.law, a.masks, a.n3, a.seed, a.chain, a.mstep, a.slot, (int)g);
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

template <typename T>
void mm_set(MMArgs<T>& a, int M, int N, int K, const T* A, int lda, int ta, const T* B, int ldb, int tb, T* C, int ldc) {
  a.M = M; a.N = N; a.K = K; a.A = A; a.lda = lda; a.ta = ta; a.B = B; a.ldb = ldb; a.tb = tb; a.C = C; a.ldc = ldc;
}

// What the layer-3 kernel produces besides the loss
struct L3Want { bool ga2, pb2, pb3, pw3; };

// hmcx_mlp.hip: the workspace of a net, xw = X·W1ᵀ for np (W1, out) pairs in one launch, the forward (see there)
template <typename T> void mlp_workspace(Workspace& ws, MlpNet<T>& net);
template <typename T> hipError_t mlp_layer1_batch(MlpNet<T>& net, const T* const* W1, T* const* out, int np);
template <typename T>
hipError_t mlp_forward(MlpNet<T>& net, T* const* q, const MaskSrc<T>& ms, double* lpart, L3Want w, T* logits = nullptr);

// hmcx_mlp_chains.hip: a list of chains as the problems of batched launches (k_mmc).  Entry j is one chain: its net
// (every buffer of a forward / backward is the chain's own; X, y and the dimensions are read from net[0]), its θ
// and gradient outputs (six pointers each, canonical order), the masks of the forward and its loss partials.  The
// list need not be dense in the caller's chains: a chain that has nothing to do is left out and writes nothing.
template <typename T> struct ChainList {
  int n;                              // 1 .. MAXPROB
  MlpNet<T>* net[MAXPROB];
  T* const* q[MAXPROB];
  T* const* g[MAXPROB];
  MaskSrc<T> ms[MAXPROB];
  double* lpart[MAXPROB];
};
// The forward of every listed chain at its θ: layer 1 (`layer1`: one batched launch into the chains' xw), then
// layers 2 and 3 with the layer-3 backward pieces the gradient components `want` (bit v) use — two k_mmc launches
// (n_out ≤ 32) or mlp_forward chain by chain.  Then the rest of the gradient: layer-1 backward (want & 3), the W1
// (bit 0) and W2 (bit 2) gradients into g; the bias / W3 gradients stay as the chains' row-block partials
// (pb1, pb2, pw3, pb3) for the caller's element-wise kernel.  mlp_grad_launch's launches and flags per chain.
template <typename T> int mlp_chains_forward(hmcx_ctx* ctx, ChainList<T>& L, unsigned want, bool layer1);
template <typename T> int mlp_chains_backward(hmcx_ctx* ctx, ChainList<T>& L, unsigned want, double alpha);

// The launch group of the two chain schedules (mlp_sgld_chains_t, mlp_hmc_chains_t), host only: the nets of up to
// MAXPROB chains that share dimensions, minibatch and stream, and what follows from them.  The schedules keep
// their own buffers, kernels, argument blocks and step loops.
template <typename T> struct ChainGroup {
  MlpNet<T> cn[MAXPROB];
  int G;                                 // chains of a full group: min(C, MAXPROB)
  int n3, ng;                            // mask values of one forward and their groups of 64 (one thread each)
  size_t mstride;                        // a chain's mask scratch: 16-byte aligned like the first
  int64_t pstride = 0;                   // elements between two chains' gradient partials (spacing())
  ChainGroup(int C, int B, int n_in, int n_mid, int n_out, hipStream_t st)
      : G(C < MAXPROB ? C : MAXPROB), n3(3 * B * n_mid), ng((n3 + 63) / 64), mstride(((size_t)n3 + 63) / 64 * 64) {
    for (int c = 0; c < G; ++c) net_init(cn[c], B, n_in, n_mid, n_out, st);
  }
  // grid rows of NPART blocks that draw the masks of `forwards` forwards behind `extra` other blocks
  unsigned mask_rows(int forwards, int extra = 0) const {
    return (unsigned)(((size_t)((size_t)forwards * ng + 255) / 256 + extra + NPART - 1) / NPART);
  }
  void take(Workspace& ws) { for (int c = 0; c < G; ++c) mlp_workspace<T>(ws, cn[c]); }
  // the row-block partials of a bias / W3 gradient (canonical v = 1, 3, 4, 5; null for W1 and W2)
  static const T* part_of(const MlpNet<T>& n, int v) {
    return v == 1 ? n.pb1 : v == 3 ? n.pb2 : v == 4 ? n.pw3 : v == 5 ? n.pb3 : nullptr;
  }
  // after the takes: the element-wise kernels reach chain c's partials at c·pstride behind the first chain's
  int spacing(hmcx_ctx* ctx, const char* who) {
    pstride = G > 1 ? (int64_t)(cn[1].pb1 - cn[0].pb1) : 0;
    for (int c = 0; c < G; ++c)
      for (int v : {1, 3, 4, 5})
        if (part_of(cn[c], v) != part_of(cn[0], v) + (int64_t)c * pstride)
          return set_error(ctx, HMCX_EINVAL, std::string(who) + "the chains' workspaces are not equally spaced");
    return HMCX_OK;
  }
  // the noise layout: variable after variable in `order`
  void noise_layout(const int* order, int* e0) const {
    for (int i = 0, off = 0; i < 6; ++i) {
      e0[order[i]] = off;
      off += cn[0].nvar(order[i]);
    }
  }
  // the masks of a forward of chain c: FIXED at fixed_ptr, PHILOX the chain's part of `scratch`, NONE nothing
  MaskSrc<T> mask_src(int c, int mode, const T* fixed_ptr, const T* scratch) {
    const T* m = mode == HMCX_MLP_MASKS_FIXED ? fixed_ptr : mode == HMCX_MLP_MASKS_PHILOX ? scratch + c * mstride : nullptr;
    cn[c].vec_masks = cn[c].n_mid % 4 == 0 && !(m && (uintptr_t)m % 16);
    return MaskSrc<T>{m, nullptr, T(1), cn[c].B * cn[c].n_mid};
  }
};
}  // namespace hmcx
