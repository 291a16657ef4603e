// hmcx_keep_law.h — the dropout keep law of the MLP for any ratio: the threshold and its compare constants from
// the ratio (keep_law_of, with the validation hmcx_set_mlp_dropout applies), and the Philox keep flags of 64
// elements (keep_group).  Compiles with the device compiler and with a plain host compiler (hmcx.h, hmcx_philox.h
// and the C library only), so a stand-alone host program can print the flags the kernels draw
// (tests/test_mlp_dropout_cpu.py).
#pragma once
#include "hmcx.h"
#include "hmcx_philox.h"
#include <math.h>

namespace hmcx {

// An element with 24-bit uniform x is kept iff x >= t, t = ⌈ratio·2^24⌉ (Chainer, mlp.py:30-31: keep iff
// u >= ratio for u a 24-bit float32 uniform; ratio 0.1: t = 0x19999A).  With tb = t >> 16 and tl = t & 0xFFFF:
// kept iff x's top byte > tb, or == tb and x's low 16 bits >= tl.  The law travels by value inside the kernels'
// argument blocks — wavefront-uniform words, scalar registers — never through device memory.
struct KeepLaw {
  uint32_t tb4;   // tb in each of the four bytes
  uint32_t add;   // 0x7F − (tb & 0x7F) in each byte: added to a byte's low seven bits, bit 7 of the sum is
                  // (byte & 0x7F) > (tb & 0x7F)
  uint32_t tl;    // t & 0xFFFF; 0: every tie keeps and no fallback block is drawn
};
// The law and the value of a kept element, (T)(1 / (1 − ratio)), as a kernel computing in T takes them.
template <typename T> struct DropLaw { KeepLaw keep; T scale; };

constexpr double MLP_DROPOUT_DEFAULT = 0.1;
// The law of the default ratio, t = 0x19999A: the value a context starts with, and — KeepLawDefault — the type a
// kernel passes that keeps the law as compile-time constants (nothing travels; the compares below are written out
// with their constants).
constexpr KeepLaw KEEP_LAW_DEFAULT = {0x19191919u, 0x66666666u, 0x999Au};
struct KeepLawDefault {};
constexpr const char* MLP_DROPOUT_MSG = "mlp dropout: ratio must satisfy 0 <= ratio and ceil(ratio * 2^24) < 2^24";

// The threshold of a ratio; false for a ratio that has none (negative, NaN, or ⌈ratio·2^24⌉ >= 2^24).
inline bool keep_threshold(double ratio, uint32_t* t) {
  if (!(ratio >= 0.0)) return false;                       // NaN and negatives; −0.0 passes
  const double c = ceil(ratio * 16777216.0);               // exact: a power-of-two scaling
  if (!(c < 16777216.0)) return false;
  *t = (uint32_t)c;
  return true;
}
// hmcx_set_mlp_dropout's rule: HMCX_OK with the law and the float64 scale 1 / (1 − ratio) (at 0.1 the bits of
// 1.0 / 0.9), or HMCX_EINVAL with *msg = MLP_DROPOUT_MSG and the outputs untouched.
inline int keep_law_of(double ratio, KeepLaw* law, double* scale, const char** msg) {
  uint32_t t;
  if (!keep_threshold(ratio, &t)) {
    if (msg) *msg = MLP_DROPOUT_MSG;
    return HMCX_EINVAL;
  }
  const uint32_t tb = t >> 16;
  law->tb4 = tb * 0x01010101u;
  law->add = (0x7Fu - (tb & 0x7Fu)) * 0x01010101u;
  law->tl = t & 0xFFFFu;
  *scale = 1.0 / (1.0 - ratio);
  return HMCX_OK;
}

// Byte compares on four bytes at once, the answer of byte b in bit 8b + 7.  s holds in that bit whether the
// byte's low seven bits exceed tb's (no carry leaves a byte: 0x7F + 0x7F < 0x100).  Where tb < 0x80 a byte is
// greater iff its own top bit is set or s's is (w | s); where tb >= 0x80 iff both are (w & s): one three-input
// bit function of w, s and tb4, so the law needs no second form for ratios of a half and above.
HMCX_HD inline uint32_t bytes_gt(uint32_t w, const KeepLaw& L) {
  const uint32_t s = (w & 0x7F7F7F7Fu) + L.add;
  return ((w & s) | ((w | s) & ~L.tb4)) & 0x80808080u;
}
HMCX_HD inline uint32_t bytes_eq(uint32_t w, const KeepLaw& L) {
  const uint32_t z = w ^ L.tb4;
  return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
}
HMCX_HD inline uint32_t law_tl(const KeepLaw& L) { return L.tl; }
// The default law's compares in their two-input forms, constants in place.  They are not the forms above with
// KEEP_LAW_DEFAULT's values filled in: hipcc (ROCm 7, gfx950) folded that constant three-input form together with
// the exclusive-or that produces a Philox word into one v_bitop3_b32 with the wrong truth table (s | c instead of
// s | (b ^ c)) and dropped an operand — wrong flags in k_fwdr's rows, which
// tests/test_gpu_mlp.py::test_sampler_philox_masks_equal_api_masks[fwdr-f32] caught.
HMCX_HD inline uint32_t bytes_gt(uint32_t w, KeepLawDefault) {     // bit 8b + 7: byte b > 0x19
  return (((w & 0x7F7F7F7Fu) + 0x66666666u) | w) & 0x80808080u;
}
HMCX_HD inline uint32_t bytes_eq(uint32_t w, KeepLawDefault) {     // bit 8b + 7: byte b == 0x19
  const uint32_t z = w ^ 0x19191919u;
  return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
}
HMCX_HD inline uint32_t law_tl(KeepLawDefault) { return 0x999Au; }

// Dropout keep flags, 64 elements per group G of one forward's flag space: element 64G + p is bit p of {lo, hi}
// (bit p % 32 of word p / 32: the keep-word layout).  Its x takes its top byte from byte p / 8 % 4 of word
// 8·(p / 32) + p % 8 of blocks 4G … 4G + 3 = Philox4x32-10({4G + k, slot, step, chain}, seed) (word k·4 + q of
// the group = word q of block k): a byte below tb drops, above keeps; a byte equal to tb (p = 1/256) takes x's
// low 16 bits from the fallback blocks Philox({0x80000000 | 8G + j, slot, step, chain}) — the a-th such element
// of the group (ascending p) reads 16-bit half a % 8 (low half first) of block j = a / 8 — and keeps iff they
// are >= tl.  Exactly the 24-bit law, at 16 flags per Philox block plus about one fallback block per group;
// where tl == 0 every tie keeps and the fallback blocks are not drawn.
// Host twins: tests/test_gpu_mlp.py::_keep_group_host (ratio 0.1), tests/_mlp_dropout.py::keep_group_host.
// Law: KeepLaw (the law by value) or KeepLawDefault (the default's constants).
struct KeepGroup { uint32_t lo, hi; };
template <class Law>
HMCX_HD inline KeepGroup keep_group(const Law& L, uint64_t seed, uint32_t G, uint32_t slot, uint32_t step,
                                    uint32_t chain) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), tl = law_tl(L);
  uint32_t f0 = 0, f1 = 0, a0 = 0, a1 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const u32x4 r = philox4x32_10(u32x4{{4u * G + (uint32_t)k, slot, step, chain}}, k0, k1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = (k & 1) * 4 + q;                           // word of the half: bits 8b + j
      const uint32_t gt = bytes_gt(r.v[q], L) >> (7 - j), eq = bytes_eq(r.v[q], L) >> (7 - j);
      if (k < 2) { f0 |= gt; a0 |= eq; } else { f1 |= gt; a1 |= eq; }
    }
  }
  if (tl == 0u) {                                            // uniform: x >= tb·2^16 whatever the low bits
    f0 |= a0;
    f1 |= a1;
    a0 = a1 = 0u;
  }
  for (uint32_t j = 0; (a0 | a1) != 0u; ++j) {                 // at most 8 blocks (64 ambiguous bytes)
    const u32x4 r = philox4x32_10(u32x4{{0x80000000u | (G << 3) | j, slot, step, chain}}, k0, k1);
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const bool keep = ((r.v[h >> 1] >> (16 * (h & 1))) & 0xFFFFu) >= tl;
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

}  // namespace hmcx
