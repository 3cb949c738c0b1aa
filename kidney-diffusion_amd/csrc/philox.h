// Philox4x32-10 standard normals on the device: the one generator of every kernel that draws (kernels_sampler.hip,
// kernels_tiles.hip) and of kd_philox_normal.  Element j of stream `sid` under key `seed` is component j % 4 of the block
// at counter (j / 4, sid); one call serves one float4.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Philox4 {
  uint32_t v[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += W0; k1 += W1;
  }
  Philox4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }
// four standard normals for elements 4*i4 .. 4*i4+3 of stream `sid`
__device__ __forceinline__ f32x4 philox_normal4(uint64_t seed, uint64_t sid, uint64_t i4) {
  Philox4 r = philox4x32_10((uint32_t)i4, (uint32_t)(i4 >> 32), (uint32_t)sid, (uint32_t)(sid >> 32),
                            (uint32_t)seed, (uint32_t)(seed >> 32));
  f32x4 z;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    float u1 = u01(r.v[2 * p]), u2 = u01(r.v[2 * p + 1]);
    float rad = sqrtf(-2.0f * logf(u1));
    float th = 6.283185307179586f * u2;
    z[2 * p] = rad * cosf(th);
    z[2 * p + 1] = rad * sinf(th);
  }
  return z;
}

}  // namespace kd
