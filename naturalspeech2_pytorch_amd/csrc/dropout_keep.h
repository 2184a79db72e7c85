// The keep decision of the attention dropout of the TRAINING kernels (ATT:100-101, 146: F.dropout on the softmax output):
// a stateless counter-based function of (seed, call index, b, h, q, k), so the forward kernel and both roles of the backward kernel
// see the same mask without anyone storing it (DESIGN.md §9 "attention dropout").
//
//   mix(x)      = the 32-bit integer finaliser  x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16
//   head key    = mix(mix(seed[0] ^ mix(seed[1] + call * 0x9E3779B9)) + (b H + h) * 0x85EBCA77)
//   value(q, k) = mix(head key + q * 0x9E3779B1 + k * 0x27D4EB2F)                      (all arithmetic modulo 2^32)
//   keep        = value >= threshold,  threshold = round(p * 2^32)                      (p = 0: threshold 0, everything is kept)
//
// seed = two 32-bit words READ FROM DEVICE MEMORY by the kernels (a captured graph draws a fresh mask per replay: Python refills the
// words with PyTorch's graph-aware generator); call = the index of the attention inside the pass (one seed serves every layer).
// tests/test_encoder_training_gpu.py restates this file in torch integer arithmetic.
#pragma once
#include <cstdint>

namespace ns2 {

__host__ __device__ inline uint32_t drop_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du;
  x ^= x >> 15; x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint32_t drop_head_key(uint32_t seed0, uint32_t seed1, uint32_t call, uint32_t bh) {
  return drop_mix(drop_mix(seed0 ^ drop_mix(seed1 + call * 0x9E3779B9u)) + bh * 0x85EBCA77u);
}
__host__ __device__ inline uint32_t drop_value(uint32_t head_key, uint32_t q, uint32_t k) {
  return drop_mix(head_key + q * 0x9E3779B1u + k * 0x27D4EB2Fu);
}
// threshold of a drop probability p in [0, 1): round(p 2^32)
inline uint32_t drop_threshold(float p) {
  const double t = (double)p * 4294967296.0 + 0.5;
  return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}

}  // namespace ns2
