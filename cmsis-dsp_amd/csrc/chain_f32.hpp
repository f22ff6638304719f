// The pieces the ordered f32 chain kernels of statistics.hip and distance.hip share: the thresholds of their two
// mappings (one wave per item, one lane per item), the in-order sum over a wave's lanes, and arm_sqrt_f32.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

constexpr int kSumChunk = 16;                    // words per item and LDS stage (a 64-byte row segment)
constexpr uint32_t kSumLaneMinBatch = 4096;      // from here on one lane per item, below one wave per item
constexpr uint32_t kVarKeep = 1024;              // words of an item the wave form keeps in LDS between var's passes

__device__ __forceinline__ float sqrt_or_zero(float v) { return v >= 0.0f ? sqrtf(v) : 0.0f; }   // arm_sqrt_f32

// sum + t[0] + t[1] + ... + t[cnt - 1], lane j holding t[j], in that order.
__device__ __forceinline__ float chain_lanes(float sum, float t, uint32_t cnt) {
  if (cnt == 64) {
#pragma unroll
    for (int j = 0; j < 64; ++j)
      sum = sum + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t), j));
  } else {
    for (uint32_t j = 0; j < cnt; ++j) sum = sum + __shfl(t, (int)j, 64);   // uniform trip count
  }
  return sum;
}

}  // namespace
}  // namespace mi355x
