// arm_quaternion_{norm,inverse,conjugate,normalize,product,product_single}_f32, arm_quaternion2rotation_f32 and
// arm_rotation2quaternion_f32 over an array of quaternions, bit-exact with the reference's scalar branches
// (Source/QuaternionMathFunctions: the final #else, no FMA contraction).  sqrtf and the divisions are the correctly
// rounded ones.
//
//   One lane per quaternion.  A quaternion is one 16-B access where the array is 16-B aligned, four words otherwise.
//   The norm is one word per lane.  product: B is A's neighbour (bStride 4) or one quaternion for every lane (0).
//   A rotation is 9 words, 36 B, which no lane can fetch in one aligned access and whose per-lane word accesses would
//   be 36 B apart.  A workgroup's 256 rotations (2304 consecutive words) pass through LDS instead: towards global
//   memory lane t moves word t, t + 256, ... of the tile, so a wave's access is 64 consecutive words; towards the
//   registers lane t moves words 9 t .. 9 t + 8, a stride of 9 words, which is odd and so free of bank conflicts.
#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

constexpr int kRotWords = 9;

__device__ __forceinline__ float4 qt_load(const float* p, size_t i, bool vec) {
  if (vec) return ((const float4*)p)[i];
  return make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
}
__device__ __forceinline__ void qt_store(float* p, size_t i, bool vec, float4 q) {
  if (vec) {
    ((float4*)p)[i] = q;
  } else {
    p[4 * i] = q.x;
    p[4 * i + 1] = q.y;
    p[4 * i + 2] = q.z;
    p[4 * i + 3] = q.w;
  }
}

// arm_quaternion_norm_f32.c: the four squares summed left to right
__device__ __forceinline__ float qt_squares(float4 q) { return q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w; }

// arm_quaternion_product_single_f32.c
__device__ __forceinline__ float4 qt_product(float4 a, float4 b) {
  float4 r;
  r.x = a.x * b.x - a.y * b.y - a.z * b.z - a.w * b.w;
  r.y = a.x * b.y + a.y * b.x + a.z * b.w - a.w * b.z;
  r.z = a.x * b.z + a.z * b.x + a.w * b.y - a.y * b.w;
  r.w = a.x * b.w + a.w * b.x + a.y * b.z - a.z * b.y;
  return r;
}

// arm_rotation2quaternion_f32.c: strict comparisons, so a trace of exactly 0 takes the second test and a NaN trace
// (every comparison false) ends in the last branch.
__device__ __forceinline__ float4 qt_from_rotation(const float* r) {
  const float r00 = r[0], r01 = r[1], r02 = r[2], r10 = r[3], r11 = r[4], r12 = r[5], r20 = r[6], r21 = r[7], r22 = r[8];
  const float trace = r00 + r11 + r22;
  float4 q;
  if (trace > 0.0f) {
    const float doubler = sqrtf(trace + 1.0f) * 2.0f;
    const float s = 1.0f / doubler;
    q.x = 0.25f * doubler;
    q.y = (r21 - r12) * s;
    q.z = (r02 - r20) * s;
    q.w = (r10 - r01) * s;
  } else if (r00 > r11 && r00 > r22) {
    const float doubler = sqrtf(1.0f + r00 - r11 - r22) * 2.0f;
    const float s = 1.0f / doubler;
    q.x = (r21 - r12) * s;
    q.y = 0.25f * doubler;
    q.z = (r01 + r10) * s;
    q.w = (r02 + r20) * s;
  } else if (r11 > r22) {
    const float doubler = sqrtf(1.0f + r11 - r00 - r22) * 2.0f;
    const float s = 1.0f / doubler;
    q.x = (r02 - r20) * s;
    q.y = (r01 + r10) * s;
    q.z = 0.25f * doubler;
    q.w = (r12 + r21) * s;
  } else {
    const float doubler = sqrtf(1.0f + r22 - r00 - r11) * 2.0f;
    const float s = 1.0f / doubler;
    q.x = (r10 - r01) * s;
    q.y = (r02 + r20) * s;
    q.z = (r12 + r21) * s;
    q.w = 0.25f * doubler;
  }
  return q;
}

// arm_quaternion2rotation_f32.c
__device__ __forceinline__ void qt_to_rotation(float4 q, float* r) {
  const float q00 = q.x * q.x, q11 = q.y * q.y, q22 = q.z * q.z, q33 = q.w * q.w;
  const float q01 = q.x * q.y, q02 = q.x * q.z, q03 = q.x * q.w, q12 = q.y * q.z, q13 = q.y * q.w, q23 = q.z * q.w;
  r[0] = q00 + q11 - q22 - q33;
  r[1] = 2 * (q12 - q03);
  r[2] = 2 * (q13 + q02);
  r[3] = 2 * (q12 + q03);
  r[4] = q00 - q11 + q22 - q33;
  r[5] = 2 * (q23 - q01);
  r[6] = 2 * (q13 - q02);
  r[7] = 2 * (q23 + q01);
  r[8] = q00 - q11 - q22 + q33;
}

// The forms without a rotation.  n: quaternions; veca / vecb / vecd: that array is 16-B aligned.
template <int OP>
__global__ __launch_bounds__(kBlock) void quaternion_kernel(const float* a, const float* b, uint32_t bStride, float* d,
                                                            uint32_t n, bool veca, bool vecb, bool vecd) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;                                        // the kernel has no barrier
  const float4 q = qt_load(a, i, veca);
  if constexpr (OP == kQtNorm) {
    d[i] = sqrtf(qt_squares(q));
  } else if constexpr (OP == kQtInverse) {
    const float t = qt_squares(q);
    qt_store(d, i, vecd, make_float4(q.x / t, -q.y / t, -q.z / t, -q.w / t));
  } else if constexpr (OP == kQtConjugate) {
    qt_store(d, i, vecd, make_float4(q.x, -q.y, -q.z, -q.w));
  } else if constexpr (OP == kQtNormalize) {
    const float t = sqrtf(qt_squares(q));
    qt_store(d, i, vecd, make_float4(q.x / t, q.y / t, q.z / t, q.w / t));
  } else {
    qt_store(d, i, vecd, qt_product(q, qt_load(b, bStride ? i : 0, vecb)));
  }
}

// kQtToRotation (a: quaternions, d: rotations) and kQtFromRotation (a: rotations, d: quaternions).
template <int OP>
__global__ __launch_bounds__(kBlock) void rotation_kernel(const float* a, float* d, uint32_t n, bool vec) {
  __shared__ float tile[kBlock * kRotWords];
  const uint32_t t = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * kBlock;
  const uint32_t cnt = (uint32_t)min((size_t)kBlock, (size_t)n - first);      // the grid has no block past n
  const uint32_t words = cnt * kRotWords;
  if constexpr (OP == kQtFromRotation) {
    const float* src = a + first * kRotWords;
    for (uint32_t w = t; w < words; w += kBlock) tile[w] = src[w];
    __syncthreads();
    if (t < cnt) qt_store(d, first + t, vec, qt_from_rotation(tile + t * kRotWords));
  } else {
    if (t < cnt) qt_to_rotation(qt_load(a, first + t, vec), tile + t * kRotWords);
    __syncthreads();
    float* dst = d + first * kRotWords;
    for (uint32_t w = t; w < words; w += kBlock) dst[w] = tile[w];
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

hipError_t quaternion_launch(int op, const float* a, const float* b, uint32_t bStride, float* d, uint32_t n,
                             hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 block(kBlock);
  const uint32_t blocks = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
  const bool va = aligned16(a), vb = aligned16(b), vd = aligned16(d);
  switch (op) {
#define MI355X_QT(OP)                                                                                     \
  case OP:                                                                                                \
    hipLaunchKernelGGL(quaternion_kernel<OP>, dim3(blocks), block, 0, st, a, b, bStride, d, n, va, vb, vd); \
    break;
    MI355X_QT(kQtNorm)
    MI355X_QT(kQtInverse)
    MI355X_QT(kQtConjugate)
    MI355X_QT(kQtNormalize)
    MI355X_QT(kQtProduct)
#undef MI355X_QT
    case kQtToRotation:
      hipLaunchKernelGGL(rotation_kernel<kQtToRotation>, dim3(blocks), block, 0, st, a, d, n, va);
      break;
    case kQtFromRotation:
      hipLaunchKernelGGL(rotation_kernel<kQtFromRotation>, dim3(blocks), block, 0, st, a, d, n, vd);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace mi355x
