// hmcx_mlp_chains.hip — chains as problems on the dropout MLP (hmcx_mlp_sgld_chains_run): several SGLD chains on
// shared minibatches run the one-chain schedule (mlp_sgld_t, hmcx_mlp.hip) with every launch widened over a group
// of up to MAXPROB chains — k_mmc (k_mmb with a problem table that also carries the buffers a chain owns),
// k_pending_chains, k_mlp_sgld_chains.  The group forward / gradient launches are helpers (mlp_chains_forward,
// mlp_chains_backward) that the multi-chain HMC of hmcx_mlp_hmc_chains.hip calls as well; the group's nets, mask
// sizes, workspaces and mask sources are ChainGroup's (hmcx_mlp_shared.h), the arguments are checked in
// hmcx_mlp_checks.h before this unit is reached.
// A unit of its own, once per dtype, so that hmcx_mlp.hip's code objects keep the layout they were measured with
// (DESIGN.md §5.3).  The launches shared with the one-chain paths (layer 1, the n_out > 32 forward, the mask draws)
// go through helpers of hmcx_mlp.hip seen here as prototypes only (hmcx_mlp_shared.h, hmcx_internal.h): including
// a helper's definition would put a second copy of every kernel it launches into this unit.
#include "hmcx_mlp_kernels.h"
#include "hmcx_mlp_shared.h"
#include <algorithm>

namespace hmcx {
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
      if (g * 64 < (size_t)a.n3) mlp_masks_group<T>(a.law, masks, a.n3, a.seed, chain, a.mstep, a.slot, (int)g);
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

// Launch k_mmc for a group of chains: mm()'s choices — tile grid, vector paths (over every chain's operands), mask
// kind (explicit values or none: the chains never read keep flags) — with one plane per chain and no pending plane.
template <typename T, int EPI, int TA, int TB, int AOP = OP_PLAIN, int BOP = OP_PLAIN>
hipError_t mmc(hipStream_t st, bool vec_masks, MMArgs<T>& a, const MMChains<T>& pr) {
  if (a.ta != TA || a.tb != TB || pr.n < 1 || pr.n > MAXPROB || a.ms.keep) return hipErrorInvalidValue;
  a.pend.n = 0;
  dim3 grid((a.M + 31) / 32, (a.N + 31) / 32, pr.n), blk(MM_NT);
  if (EPI == MM_L3CE) grid.y = (unsigned)std::max(1, std::min(8, a.n_mid / 32));   // n_mid column slices
  const bool h1ok = AOP != OP_H1 || vec_masks;
  const bool kvec = a.K % (int)(16 / sizeof(T)) == 0;
  bool aal = true, bal = true;
  for (int p = 0; p < pr.n; ++p) {
    aal = aal && vec_ok(pr.p[p].A, a.lda, sizeof(T));
    bal = bal && vec_ok(pr.p[p].B, a.ldb, sizeof(T));
  }
  const bool av = !TA && h1ok && kvec && aal;
  const bool bv = TB && kvec && bal;
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

// The group forward / gradient launches (hmcx_mlp_shared.h), shared by the multi-chain SGLD below and the multi-chain
// HMC of hmcx_mlp_hmc_chains.hip, which sees them as prototypes.
template <typename T> static bool list_vec_masks(const ChainList<T>& L) {
  bool v = true;
  for (int c = 0; c < L.n; ++c) v = v && L.net[c]->vec_masks;
  return v;
}
template <typename T>
__attribute__((used)) int mlp_chains_forward(hmcx_ctx* ctx, ChainList<T>& L, unsigned want, bool layer1) {
  MlpNet<T>& net = *L.net[0];
  const int np = L.n, B = net.B, nm = net.n_mid, n_out = net.n_out;
  if (np < 1 || np > MAXPROB) return set_error(ctx, HMCX_EINVAL, "mlp chains: bad chain list");
  const L3Want w{(want & 15u) != 0, (want & 8u) != 0, (want & 32u) != 0, (want & 16u) != 0};
  if (layer1) {
    const T* W1[MAXPROB];
    T* xw[MAXPROB];
    for (int c = 0; c < np; ++c) { W1[c] = L.q[c][0]; xw[c] = L.net[c]->xw; }
    HMCX_HIP(ctx, mlp_layer1_batch<T>(net, W1, xw, np));
  }
  if (n_out > 32) {
    for (int c = 0; c < np; ++c) {
      L.net[c]->xw_valid = true;
      HMCX_HIP(ctx, mlp_forward<T>(*L.net[c], L.q[c], L.ms[c], L.lpart[c], w));
    }
    return HMCX_OK;
  }
  const bool vm = list_vec_masks(L);
  MMChains<T> pr{};
  pr.n = np;
  for (int c = 0; c < np; ++c) {
    MMProbC<T>& p = pr.p[c];
    p.A = L.net[c]->xw; p.B = L.q[c][2]; p.C = L.net[c]->h2; p.C2 = L.net[c]->d3;
    p.b1 = L.q[c][1]; p.bias = L.q[c][3]; p.ms = L.ms[c];
  }
  MMArgs<T> a{};
  mm_set<T>(a, B, nm, nm, net.xw, nm, 0, L.q[0][2], nm, 1, net.h2, nm);
  a.ms = L.ms[0];
  HMCX_HIP(ctx, (mmc<T, MM_L2, 0, 1, OP_H1>(net.st, vm, a, pr)));
  pr = MMChains<T>{};
  pr.n = np;
  for (int c = 0; c < np; ++c) {
    MMProbC<T>& p = pr.p[c];
    const MlpNet<T>& cn = *L.net[c];
    p.A = cn.d3; p.B = L.q[c][4]; p.C = cn.gz; p.bias = L.q[c][5]; p.ms = L.ms[c];
    p.lpart = L.lpart[c];
    p.W3 = L.q[c][4]; p.h2 = cn.h2; p.d3 = cn.d3;
    p.ga2 = w.ga2 ? cn.ga2 : nullptr;
    p.pb2 = w.pb2 ? cn.pb2 : nullptr;
    p.pb3 = w.pb3 ? cn.pb3 : nullptr;
    p.pw3 = w.pw3 ? cn.pw3 : nullptr;
  }
  a = MMArgs<T>{};
  mm_set<T>(a, B, n_out, nm, net.d3, nm, 0, L.q[0][4], nm, 1, net.gz, n_out);
  a.y = net.y; a.n_mid = nm; a.ms = L.ms[0];
  HMCX_HIP(ctx, (mmc<T, MM_L3CE, 0, 1>(net.st, vm, a, pr)));
  return HMCX_OK;
}

template <typename T>
__attribute__((used)) int mlp_chains_backward(hmcx_ctx* ctx, ChainList<T>& L, unsigned want, double alpha) {
  MlpNet<T>& net = *L.net[0];
  const int np = L.n, B = net.B, nm = net.n_mid;
  if (np < 1 || np > MAXPROB) return set_error(ctx, HMCX_EINVAL, "mlp chains: bad chain list");
  const bool vm = list_vec_masks(L);
  MMChains<T> pr{};
  MMArgs<T> a{};
  if (want & 3u) {
    pr.n = np;
    for (int c = 0; c < np; ++c) {                           // layer-1 backward (+ b1 partials)
      MMProbC<T>& p = pr.p[c];
      const MlpNet<T>& cn = *L.net[c];
      p.A = cn.ga2; p.B = L.q[c][2]; p.C = cn.ga1; p.b1 = L.q[c][1]; p.ms = L.ms[c];
      p.colpart = cn.pb1; p.H = cn.xw;
    }
    mm_set<T>(a, B, nm, nm, net.ga2, nm, 0, L.q[0][2], nm, 0, net.ga1, nm);
    a.ms = L.ms[0];
    HMCX_HIP(ctx, (mmc<T, MM_GA1, 0, 0>(net.st, vm, a, pr)));
  }
  if (want & 1u) {
    pr = MMChains<T>{};
    pr.n = np;
    for (int c = 0; c < np; ++c) {                           // W1 gradient: ga1ᵀ·X
      MMProbC<T>& p = pr.p[c];
      p.A = L.net[c]->ga1; p.B = net.X; p.uW = L.q[c][0]; p.uG = L.g[c][0];
    }
    a = MMArgs<T>{};
    mm_set<T>(a, nm, net.n_in, B, net.ga1, nm, 1, net.X, net.n_in, 0, nullptr, net.n_in);
    a.upd_mode = UPD_GRAD; a.u.half_alpha = (T)(0.5 * alpha);
    HMCX_HIP(ctx, (mmc<T, MM_UPD, 1, 0>(net.st, vm, a, pr)));
  }
  if (want & 4u) {
    pr = MMChains<T>{};
    pr.n = np;
    for (int c = 0; c < np; ++c) {                           // W2 gradient: ga2ᵀ·h1, h1 from xw, b1 and m0
      MMProbC<T>& p = pr.p[c];
      p.A = L.net[c]->ga2; p.B = L.net[c]->xw; p.b1 = L.q[c][1]; p.ms = L.ms[c];
      p.uW = L.q[c][2]; p.uG = L.g[c][2];
    }
    a = MMArgs<T>{};
    mm_set<T>(a, nm, nm, B, net.ga2, nm, 1, net.xw, nm, 0, nullptr, nm);
    a.ms = L.ms[0];
    a.upd_mode = UPD_GRAD; a.u.half_alpha = (T)(0.5 * alpha);
    HMCX_HIP(ctx, (mmc<T, MM_UPD, 1, 0, OP_PLAIN, OP_H1>(net.st, vm, a, pr)));
  }
  return HMCX_OK;
}

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
  const int B = s->B, n_mid = s->n_mid, C = s->C;
  const bool philox = s->mask_mode == HMCX_MLP_MASKS_PHILOX, fixed = s->mask_mode == HMCX_MLP_MASKS_FIXED;
  ChainGroup<T> grp(C, B, s->n_in, n_mid, s->n_out, ctx->stream);
  MlpNet<T>* const cn = grp.cn;
  MlpNet<T>& net = cn[0];                                      // the group's shared dimensions, minibatch and stream
  const int G = grp.G, n3 = grp.n3, nlb = net.nlb;
  const size_t mstride = grp.mstride;
  Workspace ws(ctx);
  T *g[6], *mscr = nullptr, *escr = nullptr;
  double *lpart, *part;
  do {
    ws.reset();
    grp.take(ws);
    lpart = ws.take<double>((size_t)G * nlb);
    for (int v = 0; v < 6; ++v) g[v] = ws.take<T>((size_t)G * net.nvar(v));
    part = ws.take<double>((size_t)G * 6 * NPART);
    if (philox) { mscr = ws.take<T>(G * mstride); escr = ws.take<T>(G * mstride); }
  } while (ws.retry());
  if (ws.failed) return HMCX_ENOMEM;
  if (int rc = grp.spacing(ctx, "mlp sgld chains: ")) return rc;
  const int64_t pstride = grp.pstride;
  if (int rc = timing_begin(ctx, ctx->stream)) return rc;
  const T* const X0 = (const T*)s->X;
  const int nm = n_mid, n_out = s->n_out;
  const unsigned xrows = grp.mask_rows(1, 1);                  // behind the loss block
  int nmax_pend = 0;
  for (int v : {1, 3, 4, 5}) nmax_pend = std::max(nmax_pend, net.nvar(v));
  for (int c0 = 0; c0 < C; c0 += MAXPROB) {
    const int np = std::min(MAXPROB, C - c0);
    T* q[MAXPROB][6];
    T* gc[MAXPROB][6];
    ChainList<T> L{};
    L.n = np;
    for (int c = 0; c < np; ++c) {
      for (int v = 0; v < 6; ++v) {
        q[c][v] = (T*)s->par.p[v] + (size_t)(c0 + c) * (size_t)net.nvar(v);
        gc[c][v] = g[v] + (size_t)c * net.nvar(v);
      }
      L.net[c] = &cn[c]; L.q[c] = q[c]; L.g[c] = gc[c]; L.lpart[c] = lpart + (size_t)c * nlb;
    }
    MlpSgld<T> k{};
    k.law = drop_law<T>(ctx);
    for (int v = 0; v < 6; ++v) {
      k.vt.q[v] = q[0][v];
      k.vt.p[v] = s->variant == 1 ? (void*)((T*)s->mom.p[v] + (size_t)c0 * (size_t)net.nvar(v)) : nullptr;
      k.vt.qn[v] = g[v]; k.vt.n[v] = net.nvar(v);
    }
    grp.noise_layout(s->order, k.vt.e0);
    k.variant = s->variant; k.noise_mode = s->noise_mode;
    k.seed = s->seed; k.chain = s->chain0 + (uint32_t)c0;
    k.part = part; k.lpart = lpart; k.nlb = nlb; k.B = B;
    k.n3 = n3; k.slot = MASK_SLOT0;
    const SgldStrides cs{s->draw_stride, (int64_t)mstride};
    // the masks of a forward: FIXED at `off` of the caller's buffer (every chain's), PHILOX the chain's part of
    // `scr`, NONE nothing
    MaskSrc<T>* const ms = L.ms;
    auto masks_of = [&](int64_t off, const T* scr) {
      for (int c = 0; c < np; ++c) ms[c] = grp.mask_src(c, s->mask_mode, fixed ? (const T*)s->masks + off : nullptr, scr);
    };
    // the group's forward at its chains' θ (want: with the layer-3 backward pieces of the gradient)
    auto forward = [&](bool want) -> int { return mlp_chains_forward<T>(ctx, L, want ? 63u : 0u, true); };
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
      if (int rc = mlp_chains_backward<T>(ctx, L, 63u, s->alpha)) return rc;
      PendChains<T> pc{};                                      // the bias / W3 gradients from the row-block partials
      pc.nparts = nlb; pc.half_alpha = (T)(0.5 * s->alpha); pc.pstride = pstride;
      {
        int j = 0;
        for (int v : {1, 3, 4, 5}) {
          pc.n[j] = net.nvar(v);
          pc.part[j] = grp.part_of(cn[0], v);
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

#if !defined(HMCX_MLP_DTYPES) || (HMCX_MLP_DTYPES & 1)   // bit 0 float, bit 1 double, as hmcx_mlp.hip
template int mlp_sgld_chains_t<float>(hmcx_ctx*, const hmcx_mlp_sgld_chains_args*);
template int mlp_chains_forward<float>(hmcx_ctx*, ChainList<float>&, unsigned, bool);
template int mlp_chains_backward<float>(hmcx_ctx*, ChainList<float>&, unsigned, double);
#endif
#if !defined(HMCX_MLP_DTYPES) || (HMCX_MLP_DTYPES & 2)
template int mlp_sgld_chains_t<double>(hmcx_ctx*, const hmcx_mlp_sgld_chains_args*);
template int mlp_chains_forward<double>(hmcx_ctx*, ChainList<double>&, unsigned, bool);
template int mlp_chains_backward<double>(hmcx_ctx*, ChainList<double>&, unsigned, double);
#endif
}  // namespace hmcx
