// The counter-based Philox4x32-10 generator (Salmon et al., SC 2011) of the augmentation kernels (csrc/augment.hip) and of the W-MSE permutation
// (csrc/whiten.hip): key = seed, counter = (sample, view key in the upper half of word 1, step, block number).  Device code only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// ---- Philox4x32-10 ------------------------------------------------------------------------------
struct Philox {
  uint32_t c[4], k[2], buf[4];
  int left;
  __device__ Philox(uint64_t seed, uint64_t step, uint64_t sample, uint32_t view) {
    k[0] = (uint32_t)seed; k[1] = (uint32_t)(seed >> 32);
    c[0] = (uint32_t)sample; c[1] = ((uint32_t)(sample >> 32) & 0xFFFFu) | ((view & 0xFFFFu) << 16);
    c[2] = (uint32_t)step; c[3] = 0; left = 0;
  }
  __device__ void block() {
    uint32_t x0 = c[0], x1 = c[1], x2 = c[2], x3 = c[3], k0 = k[0], k1 = k[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      const uint32_t lo0 = 0xD2511F53u * x0, hi0 = __umulhi(0xD2511F53u, x0);
      const uint32_t lo1 = 0xCD9E8D57u * x2, hi1 = __umulhi(0xCD9E8D57u, x2);
      const uint32_t n0 = hi1 ^ x1 ^ k0, n1 = lo1, n2 = hi0 ^ x3 ^ k1, n3 = lo0;
      x0 = n0; x1 = n1; x2 = n2; x3 = n3;
      k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    buf[0] = x0; buf[1] = x1; buf[2] = x2; buf[3] = x3;
    c[3] += 1; left = 4;
  }
  __device__ double uniform() {
    if (left == 0) block();
    const uint32_t v = buf[4 - left];
    --left;
    return (double)v * (1.0 / 4294967296.0);
  }
};
