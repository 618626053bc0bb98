// Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85) and the uniform the
// drawing passes make of one block — shared by sample.hip and simulate.hip, on the host (hyphy_hip_*_uniforms) and on the device.
// key = (seed low, seed high), counter = (site, node, replicate, stream); u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53 in [0, 1).
// `stream` keeps the passes' draws disjoint under one seed: 0 sample_ancestral, 1 simulate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hyhip {

struct Philox {
  uint32_t x[4];
};
__host__ __device__ inline Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; round++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}
__host__ __device__ inline double philox_uniform(uint64_t seed, uint32_t site, uint32_t node, uint32_t rep, uint32_t stream) {
  const Philox r = philox4x32_10(site, node, rep, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (double)(((uint64_t)(r.x[0] >> 5) << 26) + (uint64_t)(r.x[1] >> 6)) * (1.0 / 9007199254740992.0);
}
constexpr uint32_t kPhiloxSample = 0u, kPhiloxSimulate = 1u;

}  // namespace hyhip
