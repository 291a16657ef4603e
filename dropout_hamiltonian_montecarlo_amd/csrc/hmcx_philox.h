// hmcx_philox.h — the Philox4x32-10 block function alone, for the device compiler and for a plain host
// compiler (no HIP header needed there): what hmcx_common.h builds its uniforms and normals on and what the
// dropout keep law (hmcx_keep_law.h) draws its bytes from.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HMCX_HD __host__ __device__
#else
#define HMCX_HD
#endif

namespace hmcx {

struct u32x4 { uint32_t v[4]; };

HMCX_HD inline u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one 32 × 32 → 64-bit product per multiplier: a single v_mad_u64_u32 on gfx950 instead of
    // v_mul_hi_u32 + v_mul_lo_u32 (tools/microbench_philox.hip: same words, 12–18 % more blocks/s)
    const uint64_t p0 = (uint64_t)M0 * c.v[0], p1 = (uint64_t)M1 * c.v[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    u32x4 n;
    n.v[0] = hi1 ^ c.v[1] ^ k0;
    n.v[1] = lo1;
    n.v[2] = hi0 ^ c.v[3] ^ k1;
    n.v[3] = lo0;
    c = n;
    k0 += W0;
    k1 += W1;
  }
  return c;
}

}  // namespace hmcx
