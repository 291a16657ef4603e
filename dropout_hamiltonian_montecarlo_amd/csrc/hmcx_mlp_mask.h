// hmcx_mlp_mask.h — the dropout masks of the MLP: where a forward's masks come from (MaskSrc: the caller's
// values or a step's stored keep flags), the Philox keep flags (keep_group / keep_flags) and the per-kernel
// mask reads (mraw … mvals).  Shared by hmcx_mlp.hip (gradient, loss, SGHMC), whose kernels only ever load
// masks, and hmcx_mlp_pred.hip (posterior predictive), whose kernel draws keep_group itself: one definition.
#pragma once
#include "hmcx_common.h"
#include "hmcx_keep_law.h"

namespace hmcx {

// Mask slots live above the noise slots (0 = momentum, it+1 = iteration it) of the same counter space.
constexpr uint32_t MASK_SLOT0 = 0x80000000u;

// Dropout masks of one forward: m0, m1, m2 at offsets 0, mn, 2·mn.
template <typename T> struct MaskSrc {
  const T* vals;          // explicit mask values (API / BUFFER mode), or
  const uint32_t* keep;   // keep flags, one bit per element (bit e % 32 of word e / 32): value = keep ? scale : 0
                          // (Philox mode: element e = which·mn + i of forward f is bit e % 64 of keep_group(e / 64)
                          // under slot MASK_SLOT0 + f, stored once per step — the values hmcx_mlp_masks gives);
                          // neither vals nor keep: no dropout
  T scale;
  int mn;
};

// The keep law (KeepLaw, DropLaw, keep_group) is hmcx_keep_law.h's, which the host compiler reads too.
// Keep flags of a step's forwards, one bit per element (bit e % 32 of word e / 32; forward f's words start
// at f·⌈n3/32⌉): work item gi = fl·⌈n3/64⌉ + G draws keep_group(G) of forward f (slot MASK_SLOT0 + f) and
// stores its two words (flags past n3 zero).  The nf forwards drawn: f = f0 + fl for fl < nlo, then
// fhi + (fl − nlo) — a contiguous range, or one range and the step's two energy forwards.
struct KeepRange { int nf, f0, nlo, fhi; };
template <class Law>
__device__ inline void keep_flags(const Law& law, uint32_t* keep, int n3, KeepRange kr, uint64_t seed, uint32_t chain,
                                  uint32_t step, size_t gi) {
  const int W = (n3 + 31) / 32, ng = (n3 + 63) / 64;
  if (gi >= (size_t)kr.nf * ng) return;
  const int fl = (int)(gi / (size_t)ng), G = (int)(gi - (size_t)fl * ng);
  const int f = fl < kr.nlo ? kr.f0 + fl : kr.fhi + (fl - kr.nlo);
  const KeepGroup k = keep_group(law, seed, (uint32_t)G, MASK_SLOT0 + (uint32_t)f, step, chain);
  const int e0 = 64 * G;
  const uint32_t lo = n3 - e0 >= 32 ? k.lo : k.lo & ((1u << (n3 - e0)) - 1u);
  const uint32_t hi = n3 - e0 >= 64 ? k.hi : n3 - e0 > 32 ? k.hi & ((1u << (n3 - e0 - 32)) - 1u) : 0u;
  uint32_t* dst = keep + (size_t)f * W + 2 * G;
  dst[0] = lo;
  if (2 * G + 1 < W) dst[1] = hi;
}

// Where the masks come from is a compile-time parameter (MK) of every kernel that reads them, so a
// mask read is one load of the one source (MK_KEEP / MK_VALS) or nothing.  Loaded values are pinned by
// an empty asm after the batch they belong to, so hipcc cannot sink a load into a branch (which it then
// waits for on the spot).  MK_PHILOX and MK_PHILOX_LAW tag the predictive kernel alone (hmcx_mlp_pred.hip), which
// draws its flags with keep_group — under the default law as compile-time constants, or under the law of its
// argument block; mraw … mvals have no such case.
enum MaskKind { MK_NONE = 0, MK_KEEP = 1, MK_VALS = 2, MK_PHILOX = 3, MK_PHILOX_LAW = 4 };
template <typename T> struct MRaw { T v; uint32_t k; };
template <typename T, int MK> __device__ inline MRaw<T> mraw(const MaskSrc<T>& s, int which, size_t i) {
  MRaw<T> r{T(1), 1u};
  const size_t e = (size_t)which * s.mn + i;
  if constexpr (MK == MK_KEEP) r.k = (s.keep[e >> 5] >> (e & 31)) & 1u;
  if constexpr (MK == MK_VALS) r.v = s.vals[e];
  return r;
}
template <typename T, int MK> __device__ inline void mpin(MRaw<T>& r) {
  if constexpr (MK == MK_KEEP) asm volatile("" : "+v"(r.k));
  if constexpr (MK == MK_VALS) asm volatile("" : "+v"(r.v));
}
template <typename T, int MK> __device__ inline T mfin(const MaskSrc<T>& s, const MRaw<T>& r) {
  if constexpr (MK == MK_KEEP) return r.k ? s.scale : T(0);
  else if constexpr (MK == MK_VALS) return r.v;
  else return T(1);
}
template <typename T, int MK> __device__ inline T mval(const MaskSrc<T>& s, int which, size_t i) {
  MRaw<T> r = mraw<T, MK>(s, which, i);
  mpin<T, MK>(r);
  return mfin<T, MK>(s, r);
}
// V consecutive mask values from an element index that is a multiple of V (V = 16 / sizeof T)
template <typename T, int V, int MK> __device__ inline void mvals(const MaskSrc<T>& s, int which, size_t i, T (&m)[V]) {
  const size_t e = (size_t)which * s.mn + i;
  if constexpr (MK == MK_VALS) {
    T v[V];
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = s.vals[e + q];
#pragma unroll
    for (int q = 0; q < V; ++q) asm volatile("" : "+v"(v[q]));
#pragma unroll
    for (int q = 0; q < V; ++q) m[q] = v[q];
  } else if constexpr (MK == MK_KEEP) {
    uint32_t k = s.keep[e >> 5];                                 // e % V == 0: V bits of one word
    asm volatile("" : "+v"(k));
    k >>= (e & 31);
#pragma unroll
    for (int q = 0; q < V; ++q) m[q] = ((k >> q) & 1u) ? s.scale : T(0);
  } else {
#pragma unroll
    for (int q = 0; q < V; ++q) m[q] = T(1);
  }
}

}  // namespace hmcx
