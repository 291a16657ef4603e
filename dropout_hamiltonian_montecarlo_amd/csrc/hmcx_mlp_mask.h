// hmcx_mlp_mask.h — the dropout masks of the MLP: where a forward's masks come from (MaskSrc: the caller's
// values or a step's stored keep flags), the Philox keep flags (keep_group / keep_flags) and the per-kernel
// mask reads (mraw … mvals).  Shared by hmcx_mlp.hip (gradient, loss, SGHMC), whose kernels only ever load
// masks, and hmcx_mlp_pred.hip (posterior predictive), whose kernel draws keep_group itself: one definition.
#pragma once
#include "hmcx_common.h"

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

// Dropout keep flags (Chainer, mlp.py:30-31: keep iff u >= ratio 0.1, u a 24-bit float32 uniform — keep iff
// x >= 0x19999A for x uniform on [0, 2^24)), 64 elements per group G of one forward's flag space: element
// 64G + p is bit p of {lo, hi} (bit p % 32 of word p / 32: the keep-word layout).  Its x takes its top byte
// from byte p / 8 % 4 of word 8·(p / 32) + p % 8 of blocks 4G … 4G + 3 = Philox4x32-10({4G + k, slot, step,
// chain}, seed) (word k·4 + q of the group = word q of block k): a byte below 0x19 drops, above keeps;
// a byte equal to 0x19 (p = 1/256) takes x's low 16 bits from the fallback blocks Philox({0x80000000 |
// 8G + j, slot, step, chain}) — the a-th such element of the group (ascending p) reads 16-bit half a % 8
// (low half first) of block j = a / 8 — and keeps iff they are >= 0x999A.  Exactly the 24-bit law, at 16
// flags per Philox block plus about one fallback block per group (the round-5 form drew 4 per block).
// Host twin: tests/test_gpu_mlp.py::_keep_group_host.
__host__ __device__ inline uint32_t bytes_gt19(uint32_t w) {       // bit 8b + 7: byte b > 0x19
  return (((w & 0x7F7F7F7Fu) + 0x66666666u) | w) & 0x80808080u;
}
__host__ __device__ inline uint32_t bytes_eq19(uint32_t w) {       // bit 8b + 7: byte b == 0x19
  const uint32_t z = w ^ 0x19191919u;
  return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
}
struct KeepGroup { uint32_t lo, hi; };
__host__ __device__ inline KeepGroup keep_group(uint64_t seed, uint32_t G, uint32_t slot, uint32_t step,
                                                uint32_t chain) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t f0 = 0, f1 = 0, a0 = 0, a1 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const u32x4 r = philox4x32_10(u32x4{{4u * G + (uint32_t)k, slot, step, chain}}, k0, k1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = (k & 1) * 4 + q;                           // word of the half: bits 8b + j
      const uint32_t gt = bytes_gt19(r.v[q]) >> (7 - j), eq = bytes_eq19(r.v[q]) >> (7 - j);
      if (k < 2) { f0 |= gt; a0 |= eq; } else { f1 |= gt; a1 |= eq; }
    }
  }
  for (uint32_t j = 0; (a0 | a1) != 0u; ++j) {                 // at most 8 blocks (64 ambiguous bytes)
    const u32x4 r = philox4x32_10(u32x4{{0x80000000u | (G << 3) | j, slot, step, chain}}, k0, k1);
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const bool keep = ((r.v[h >> 1] >> (16 * (h & 1))) & 0xFFFFu) >= 0x999Au;
      if (a0) {
        const uint32_t low = a0 & (0u - a0);
        if (keep) f0 |= low;
        a0 ^= low;
      } else if (a1) {
        const uint32_t low = a1 & (0u - a1);
        if (keep) f1 |= low;
        a1 ^= low;
      }
    }
  }
  return KeepGroup{f0, f1};
}
// Keep flags of a step's forwards, one bit per element (bit e % 32 of word e / 32; forward f's words start
// at f·⌈n3/32⌉): work item gi = fl·⌈n3/64⌉ + G draws keep_group(G) of forward f (slot MASK_SLOT0 + f) and
// stores its two words (flags past n3 zero).  The nf forwards drawn: f = f0 + fl for fl < nlo, then
// fhi + (fl − nlo) — a contiguous range, or one range and the step's two energy forwards.
struct KeepRange { int nf, f0, nlo, fhi; };
__device__ inline void keep_flags(uint32_t* keep, int n3, KeepRange kr, uint64_t seed, uint32_t chain, uint32_t step,
                                  size_t gi) {
  const int W = (n3 + 31) / 32, ng = (n3 + 63) / 64;
  if (gi >= (size_t)kr.nf * ng) return;
  const int fl = (int)(gi / (size_t)ng), G = (int)(gi - (size_t)fl * ng);
  const int f = fl < kr.nlo ? kr.f0 + fl : kr.fhi + (fl - kr.nlo);
  const KeepGroup k = keep_group(seed, (uint32_t)G, MASK_SLOT0 + (uint32_t)f, step, chain);
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
// waits for on the spot).  MK_PHILOX tags the predictive kernel alone (hmcx_mlp_pred.hip), which draws
// its flags with keep_group; mraw … mvals have no such case.
enum MaskKind { MK_NONE = 0, MK_KEEP = 1, MK_VALS = 2, MK_PHILOX = 3 };
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
