// hmcx_mlp.hip — the reference's dropout MLP (config 3) on gfx950: gradient, loss and fused SGHMC.
//
// Reference: hamiltonian/models/gpu/mlp.py:19-31 (MyNetwork: relu(dropout(l1 x)) → relu(dropout(l2 ·))
// → l3(dropout(·)), dropout ratio 0.1 in train mode) and :47-82 (grad = ∇ mean softmax-CE + ½αθ,
// log_likelihood returns the mean CE, nlp = loss + log_prior).  Chainer/CuPy are not available, so
// the arithmetic follows the NumPy restatement in oracle/models.py::mlp (parity with injected masks).
//
// The device side (names, argument blocks, kernels) is hmcx_mlp_kernels.h, then hmcx_mlp_shared.h: the SGD / SGLD
// update kernels, MlpNet and prototypes of the helpers that hmcx_mlp_chains.hip (multi-chain SGLD, units of its own)
// calls.  Here: the launch helpers, the one-off entries, the full-batch trajectory, momentum SGD, one-chain SGLD and
// the SGHMC sampler.  Batched iterations (mlp_sghmc_t): the six sub-steps of a leapfrog iteration only depend on
// the previous iteration, so their kernels go out as multi-problem launches (k_mmb, blockIdx.z = sub-step) and
// one dual launch (k_mm2: layer-1 backwards + W2 gradient); ≈1.0 GFLOP per iteration at 784-256-256-10, B = 500
// (layer 1 runs once, after W1 moved), 5 launches per iteration (11 one sub-step at a time).
#include "hmcx_mlp_kernels.h"
#include <algorithm>
#include <cstring>

namespace hmcx {
// The static kernels only this unit launches (a static kernel is emitted by every unit that sees it).
// The keep flags alone (the forwards a k_fwdr step left undrawn when it falls back to the k_mm forwards).
static __global__ __launch_bounds__(256) void k_mlp_keep(uint32_t* keep, int n3, KeepRange kr, uint64_t seed, uint32_t chain,
                                                  uint32_t step, KeepLaw law) {
  keep_flags(law, keep, n3, kr, seed, chain, step, (size_t)blockIdx.x * 256 + threadIdx.x);
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

static __global__ void k_loss_final(const double* lpart, int nlb, int B, double* out) {
  double s = 0.0;
  for (int b = 0; b < nlb; ++b) s += lpart[b];
  *out = s / (double)B;
}

}  // namespace hmcx
#include "hmcx_mlp_shared.h"   // behind the three static kernels above: its k_mlp_sgd_eval is emitted after them
namespace hmcx {

// ------------------------------------------------------------------ host side
namespace {

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

// What mlp_sgd_t and mlp_sgld_t share: the call's unfused net with a gradient workspace, the Σθ² partials of their
// update kernels, the PHILOX mask scratches, a step's minibatch and masks, and the evaluation at the updated θ.
template <typename T> struct MlpFit {
  hmcx_ctx* ctx; MlpNet<T> net{}; Workspace ws; MaskSrc<T> ms;
  double *lpart, *part;                                        // loss partials [nlb], Σθ² partials [6][NPART]
  T *g[6], *mscr = nullptr, *escr = nullptr;                   // gradient; PHILOX masks of a step, of an evaluation
  const T *X0, *masks; const int32_t* y0;
  int B, n_in, n_mid, n3; bool philox, fixed;
  unsigned xrows;                                              // rows of the update kernel's grid that draw n3 mask values
  explicit MlpFit(hmcx_ctx* c) : ctx(c), ws(c) {}
  int init(const void* X, const int32_t* y, int B_, int n_in_, int n_mid_, int n_out, int mask_mode, const void* masks_) {
    B = B_; n_in = n_in_; n_mid = n_mid_; n3 = 3 * B * n_mid;
    X0 = (const T*)X; y0 = y; masks = (const T*)masks_;
    philox = mask_mode == HMCX_MLP_MASKS_PHILOX; fixed = mask_mode == HMCX_MLP_MASKS_FIXED;
    if (int rc = oneoff_net<T>(ctx, ws, net, X, y, B, n_in, n_mid, n_out, nullptr, &lpart, &ms)) return rc;
    do {                                                       // oneoff_net's takes again, then this call's own
      ws.reset();
      mlp_workspace<T>(ws, net);
      lpart = ws.take<double>(net.nlb);
      for (int v = 0; v < 6; ++v) g[v] = ws.take<T>((size_t)net.nvar(v));
      part = ws.take<double>(6 * NPART);
      if (philox) { mscr = ws.take<T>((size_t)n3); escr = ws.take<T>((size_t)n3); }
    } while (ws.retry());
    xrows = (unsigned)(((size_t)((n3 + 63) / 64 + 255) / 256 + 1 + NPART - 1) / NPART);   // one thread per 64 values
    return ws.failed ? HMCX_ENOMEM : HMCX_OK;
  }
  // the masks of a forward: FIXED at `off` of the caller's buffer, PHILOX in `scr`, NONE nothing
  void masks_of(int64_t off, const T* scr) {
    ms.vals = fixed ? masks + off : philox ? scr : nullptr;
    net.vec_masks = n_mid % 4 == 0 && !(ms.vals && (uintptr_t)ms.vals % 16);
  }
  void minibatch(int64_t row0, int64_t mask_off) {             // a step's rows and masks
    net.X = X0 + (size_t)row0 * n_in;
    net.y = y0 + row0;
    net.xw_valid = false;
    masks_of(mask_off, mscr);
  }
  // the state after the update: same minibatch, fresh masks (PHILOX: drawn under `step`, `slot`), then k_mlp_sgd_eval
  int eval(T* const* q, uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot, int64_t mask_off, double* out_loss,
           double* out_sumsq) {
    if (philox)
      if (int rc = mlp_masks_t<T>(ctx, B, n_mid, seed, chain, step, slot, escr)) return rc;
    masks_of(mask_off, escr);
    net.xw_valid = false;                                      // W1 moved
    HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, lpart, L3Want{false, false, false, false}));
    hipLaunchKernelGGL(k_mlp_sgd_eval, dim3(1), dim3(64), 0, ctx->stream, lpart, net.nlb, B, part, out_loss, out_sumsq);
    HMCX_HIP(ctx, hipGetLastError());
    return HMCX_OK;
  }
};

}  // namespace

template <typename T>
__attribute__((used)) void mlp_workspace(Workspace& ws, MlpNet<T>& net) {
  const size_t mn = (size_t)net.B * net.n_mid;
  net.xw = ws.take<T>(mn); net.h2 = ws.take<T>(mn); net.d3 = ws.take<T>(mn);
  net.ga2 = ws.take<T>(mn); net.ga1 = ws.take<T>(mn);
  net.z = ws.take<T>((size_t)net.B * net.n_out); net.gz = ws.take<T>((size_t)net.B * net.n_out);
  net.pb1 = ws.take<T>((size_t)net.nlb * net.n_mid);
  net.pb2 = ws.take<T>((size_t)net.nlb * net.n_mid);
  net.pb3 = ws.take<T>((size_t)net.nlb * net.n_out);
  net.pw3 = ws.take<T>((size_t)net.nlb * net.n_out * net.n_mid);
}

// xw = X·W1ᵀ for np (W1, out) pairs in one launch
template <typename T>
__attribute__((used)) hipError_t mlp_layer1_batch(MlpNet<T>& net, const T* const* W1, T* const* out, int np) {
  MMArgs<T> a{};
  MMProbs<T> pr{};
  pr.n = np;
  for (int p = 0; p < np; ++p) {
    pr.p[p].A = net.X; pr.p[p].B = W1[p]; pr.p[p].C = out[p];
  }
  mm_set<T>(a, net.B, net.n_mid, net.n_in, net.X, net.n_in, 0, W1[0], net.n_in, 1, out[0], net.n_mid);
  return mm<T, MM_STORE, 0, 1, OP_PLAIN, OP_PLAIN, true>(net, a, &pr);
}

// Forward with masks `ms` at parameters q (+ the requested layer-3 backward pieces); loss partials
// into lpart (null: no loss); logits (optional) stored without b3.  Layer 1 only when xw is stale.
template <typename T>
__attribute__((used)) hipError_t mlp_forward(MlpNet<T>& net, T* const* q, const MaskSrc<T>& ms, double* lpart, L3Want w,
                                             T* logits) {
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

// The gradient components `want` (bit v) at q into g[v], unfused, on net's minibatch: forward (+ the layer-3 backward
// pieces the wanted components use), layer-1 backward, W1 / W2 gradients, then the bias / W3 gradients as pending
// updates (element-wise: the same bits whichever launch applies them) — one k_pending launch each (GRAD_FLUSH_EACH:
// four at want = 63), one for all of them (GRAD_FLUSH_ONCE), or none: the caller's next launch takes them (GRAD_DEFER).
enum GradFlush { GRAD_FLUSH_EACH, GRAD_FLUSH_ONCE, GRAD_DEFER };
template <typename T>
int mlp_grad_launch(hmcx_ctx* ctx, MlpNet<T>& net, T* const* q, const MaskSrc<T>& ms, double* lpart, T* const* g,
                    double alpha, unsigned want, GradFlush flush) {
  HMCX_HIP(ctx, mlp_forward<T>(net, q, ms, lpart,
                               L3Want{(want & 15u) != 0, (want & 8u) != 0, (want & 32u) != 0, (want & 16u) != 0}));
  if (want & 3u) HMCX_HIP(ctx, mlp_ga1<T>(net, q, ms, true));
  Upd<T> u{};
  u.half_alpha = (T)(0.5 * alpha);
  for (int v : {0, 2})
    if (want & (1u << v)) {
      u.W = q[v]; u.G = g[v];
      HMCX_HIP(ctx, mlp_wgrad<T>(net, q, ms, v, UPD_GRAD, u));
    }
  for (int v : {1, 3, 4, 5})
    if (want & (1u << v)) {
      u.W = q[v]; u.G = g[v];
      if (!set_pending(net, v, UPD_GRAD, u)) return pend_full(ctx);
      if (flush == GRAD_FLUSH_EACH) HMCX_HIP(ctx, flush_pending(net));
    }
  if (flush == GRAD_FLUSH_ONCE) HMCX_HIP(ctx, flush_pending(net));
  return HMCX_OK;
}

template <typename T>
int mlp_masks_t(hmcx_ctx* ctx, int B, int n_mid, uint64_t seed, uint32_t chain, uint32_t step, uint32_t slot,
                void* out) {
  const int n3 = 3 * B * n_mid;
  hipLaunchKernelGGL(k_mlp_masks<T>, dim3((unsigned)(((n3 + 63) / 64 + 255) / 256)), dim3(256), 0, ctx->stream,
                     drop_law<T>(ctx), (T*)out, n3, seed, chain, step, slot);
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
  T *q[6], *g[6];
  for (int v = 0; v < 6; ++v) { q[v] = (T*)par->p[v]; g[v] = (T*)grads->p[v]; }
  if (int rc = mlp_grad_launch<T>(ctx, net, q, ms, lpart, g, alpha, 63u, GRAD_FLUSH_EACH)) return rc;
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
  // the gradient components `want` (bit v) at q (mlp_grad_launch; the bias / W3 updates in one k_pending launch,
  // or deferred: the next kicks launch applies them).  The call's masks are drawn by the kicks launch before it
  // (draw = false), except for the first call.
  auto grad = [&](unsigned want, bool draw, bool defer) -> int {
    if (pmasks && draw)
      if (int rc = mlp_masks_t<T>(ctx, s->B, s->n_mid, s->seed, s->chain, s->step, slot++, s->masks)) return rc;
    return mlp_grad_launch<T>(ctx, net, q, ms, lpart, g, s->alpha, want, defer ? GRAD_DEFER : GRAD_FLUSH_ONCE);
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
      k.slot = slot++; k.law = drop_law<T>(ctx);
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

// Momentum SGD of hmcx_mlp_sgd_run (sgd.py:36-42): per step mlp_grad_launch on the step's minibatch (the bias / W3
// gradients in ONE k_pending launch) into a gradient workspace, then k_mlp_sgd.  With n_out ≤ 32 that is 8 launches
// per step: layer 1, layer 2, layer 3 + CE, layer-1 backward, two weight gradients, k_pending, k_mlp_sgd (n_out > 32:
// 9, layer 3 takes two).  A marked step adds the evaluation (MlpFit::eval).  lpart is written by the gradient forward,
// read by the k_mlp_sgd behind it (out_loss[s]) and only then rewritten by the evaluation forward or the next step:
// stream order keeps the three apart.
template <typename T>
int mlp_sgd_t(hmcx_ctx* ctx, const hmcx_mlp_sgd_args* s) {
  MlpFit<T> f(ctx);
  if (int rc = f.init(s->X, s->y, s->B, s->n_in, s->n_mid, s->n_out, s->mask_mode, s->masks)) return rc;
  if (int rc = timing_begin(ctx, ctx->stream)) return rc;
  MlpNet<T>& net = f.net;
  T* q[6];
  MlpSgd<T> k{};
  k.law = drop_law<T>(ctx);
  for (int v = 0; v < 6; ++v) {
    q[v] = (T*)s->par.p[v];
    k.vt.q[v] = q[v]; k.vt.p[v] = s->mom.p[v]; k.vt.qn[v] = f.g[v]; k.vt.n[v] = net.nvar(v);
  }
  k.gamma = (T)s->gamma; k.lr = (T)s->step_size;
  k.part = f.part; k.lpart = f.lpart; k.nlb = net.nlb; k.B = f.B;
  k.n3 = f.n3; k.seed = s->seed; k.chain = s->chain; k.slot = MASK_SLOT0;
  if (f.philox)
    if (int rc = mlp_masks_t<T>(ctx, f.B, f.n_mid, s->seed, s->chain, s->step_base, MASK_SLOT0, f.mscr)) return rc;
  int n_eval = 0;
  for (int si = 0; si < s->n_steps; ++si) {
    f.minibatch(s->row0[si], f.fixed ? s->mask_off[si] : 0);
    if (int rc = mlp_grad_launch<T>(ctx, net, q, f.ms, f.lpart, f.g, s->alpha, 63u, GRAD_FLUSH_ONCE)) return rc;
    const bool next_masks = f.philox && si + 1 < s->n_steps;
    k.out_loss = s->out_loss ? s->out_loss + si : nullptr;
    k.masks = next_masks ? f.mscr : nullptr;
    k.step = s->step_base + (uint32_t)(si + 1);
    const unsigned rows = next_masks ? f.xrows : k.out_loss ? 1u : 0u;
    hipLaunchKernelGGL(k_mlp_sgd<T>, dim3(NPART, 6 + rows), dim3(256), 0, ctx->stream, k);
    HMCX_HIP(ctx, hipGetLastError());
    if (!(s->want_eval && s->want_eval[si])) continue;
    // sgd.py:42: the state after the update on the same minibatch, fresh masks (forward 1 of the step)
    if (int rc = f.eval(q, s->seed, s->chain, s->step_base + (uint32_t)si, MASK_SLOT0 + 1u,
                        f.fixed ? s->eval_mask_off[si] : 0, s->out_eval_loss + n_eval,
                        s->out_eval_sumsq ? s->out_eval_sumsq + 6 * (size_t)n_eval : nullptr))
      return rc;
    ++n_eval;
  }
  return timing_end(ctx, ctx->stream);
}

// SGLD of hmcx_mlp_sgld_run (sgld.py step inside sgmcmc.py's minibatch loop): mlp_sgd_t's schedule and use of lpart
// with another last kernel, k_mlp_sgld: noise, update, draw store, Σθ² partials, the step's loss and the next step's
// Philox masks — 8 launches per ordinary step with n_out ≤ 32 (9 above: layer 3 takes two).  Each set bit of
// want_eval[s] adds an evaluation at the updated θ (MlpFit::eval, Philox slot 0x80000000 + f).
template <typename T>
int mlp_sgld_t(hmcx_ctx* ctx, const hmcx_mlp_sgld_args* s) {
  MlpFit<T> f(ctx);
  if (int rc = f.init(s->X, s->y, s->B, s->n_in, s->n_mid, s->n_out, s->mask_mode, s->masks)) return rc;
  MlpNet<T>& net = f.net;
  if (int rc = timing_begin(ctx, ctx->stream)) return rc;
  T* q[6];
  MlpSgld<T> k{};
  k.law = drop_law<T>(ctx);
  for (int v = 0; v < 6; ++v) {
    q[v] = (T*)s->par.p[v];
    k.vt.q[v] = q[v]; k.vt.p[v] = s->variant == 1 ? s->mom.p[v] : nullptr; k.vt.qn[v] = f.g[v]; k.vt.n[v] = net.nvar(v);
  }
  for (int i = 0, off = 0; i < 6; ++i) {                       // the noise layout: variable after variable in `order`
    k.vt.e0[s->order[i]] = off;
    off += net.nvar(s->order[i]);
  }
  k.variant = s->variant; k.noise_mode = s->noise_mode;
  k.seed = s->seed; k.chain = s->chain;
  k.part = f.part; k.lpart = f.lpart; k.nlb = net.nlb; k.B = f.B;
  k.n3 = f.n3; k.slot = MASK_SLOT0;
  if (f.philox)
    if (int rc = mlp_masks_t<T>(ctx, f.B, f.n_mid, s->seed, s->chain, s->step_base, MASK_SLOT0, f.mscr)) return rc;
  int n_eval = 0, n_draw = 0;
  for (int si = 0; si < s->n_steps; ++si) {
    f.minibatch(s->row0[si], f.fixed ? s->mask_off[si] : 0);
    if (int rc = mlp_grad_launch<T>(ctx, net, q, f.ms, f.lpart, f.g, s->alpha, 63u, GRAD_FLUSH_ONCE)) return rc;
    const double eps = s->eps[si];
    k.two_eps = (T)(2.0 * eps);
    k.half_eps = s->variant == 0 ? (T)(-0.5 * eps) : (T)(0.5 * eps);
    k.noise = s->noise_mode == HMCX_NOISE_BUFFER ? s->noise + s->noise_off[si] : nullptr;
    k.step = s->step_base + (uint32_t)si;
    const bool keep = s->want_draw && s->want_draw[si];
    for (int v = 0; v < 6; ++v)
      k.vt.qc[v] = keep ? (void*)((T*)s->draws.p[v] + (size_t)n_draw * (size_t)net.nvar(v)) : nullptr;
    n_draw += keep ? 1 : 0;
    const bool next_masks = f.philox && si + 1 < s->n_steps;
    k.out_loss = s->out_loss ? s->out_loss + si : nullptr;
    k.masks = next_masks ? f.mscr : nullptr;
    k.mstep = s->step_base + (uint32_t)(si + 1);
    const unsigned rows = next_masks ? f.xrows : k.out_loss ? 1u : 0u;
    hipLaunchKernelGGL(k_mlp_sgld<T>, dim3(NPART, 6 + rows), dim3(256), 0, ctx->stream, k);
    HMCX_HIP(ctx, hipGetLastError());
    const int want = s->want_eval ? s->want_eval[si] : 0;
    // the state after the update on the same minibatch, fresh masks: forward 1, then 2, of the step in call
    // order (sgmcmc.py:60-62 / 74-76 the log line, :79 the epoch-end negative_log_posterior)
    for (int bit = 0, fw = 1; bit < 2; ++bit) {
      if (!((want >> bit) & 1)) continue;
      if (int rc = f.eval(q, s->seed, s->chain, s->step_base + (uint32_t)si, MASK_SLOT0 + (uint32_t)fw,
                          f.fixed ? s->eval_mask_off[2 * (size_t)si + (size_t)(fw - 1)] : 0, s->out_eval_loss + n_eval,
                          s->out_eval_sumsq ? s->out_eval_sumsq + 6 * (size_t)n_eval : nullptr))
        return rc;
      ++n_eval;
      ++fw;
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
      const T scale = (T)c->ctx->mlp_scale;
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
                         st.nz, s->seed, s->chain, st.step_id, part_cur, prev_acc, keep, n3, kr, ctx->mlp_keep);
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
      const KeepRange kr{6, 6 * (x.it + 1), 6, 0};
      if (ctx->mlp_dropout == MLP_DROPOUT_DEFAULT) {
        kf.keep = keep; kf.n3 = n3; kf.kr = kr;
        kf.seed = s->seed; kf.chain = s->chain; kf.step = st.step_id;
      } else {                                                  // k_fwdr's rows hold the default law: a launch of its own
        const size_t items = (size_t)kr.nf * ((n3 + 63) / 64);
        hipLaunchKernelGGL(k_mlp_keep, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, keep, n3, kr,
                           s->seed, s->chain, st.step_id, ctx->mlp_keep);
      }
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
                         s->seed, s->chain, st.step_id, ctx->mlp_keep);
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
// The code object holds the template kernels in the order in which these statements first reach them, so the list is
// part of the measured layout (DESIGN.md §5.3 "Build"; compare the code objects' hashes after a change): hence
// mlp_grad_launch ahead of mlp_grad_t, and the helpers of hmcx_mlp_shared.h kept by __attribute__((used)) instead.
#define HMCX_MLP_INSTANTIATE(T)                                                                                       \
  template int mlp_masks_t<T>(hmcx_ctx*, int, int, uint64_t, uint32_t, uint32_t, uint32_t, void*);                    \
  template int mlp_grad_launch<T>(hmcx_ctx*, MlpNet<T>&, T* const*, const MaskSrc<T>&, double*, T* const*, double,    \
                                  unsigned, GradFlush);                                                               \
  template int mlp_grad_t<T>(hmcx_ctx*, const void*, const int32_t*, int, int, int, int, const hmcx_mlp_params*,      \
                             const void*, double, hmcx_mlp_params*, double*);                                         \
  template int mlp_loss_t<T>(hmcx_ctx*, const void*, const int32_t*, int, int, int, int, const hmcx_mlp_params*,      \
                             const void*, double*, void*);                                                            \
  template int mlp_sghmc_t<T>(hmcx_ctx*, const hmcx_mlp_sghmc_args*);                                                 \
  template int mlp_leapfrog_t<T>(hmcx_ctx*, const hmcx_mlp_leapfrog_args*);                                           \
  template int mlp_sgd_t<T>(hmcx_ctx*, const hmcx_mlp_sgd_args*);                                                     \
  template int mlp_sgld_t<T>(hmcx_ctx*, const hmcx_mlp_sgld_args*);
#if HMCX_MLP_DTYPES & 1
HMCX_MLP_INSTANTIATE(float)
#endif
#if HMCX_MLP_DTYPES & 2
HMCX_MLP_INSTANTIATE(double)
#endif

}  // namespace hmcx
