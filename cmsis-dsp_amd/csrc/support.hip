// arm_{float,q31,q15,q7}_to_{float,q31,q15,q7}, arm_copy_* and arm_fill_* for f32 / q31 / q15 / q7 over a batch of
// contiguous items, and arm_barycenter_f32, bit-exact with the reference's scalar branches
// (Source/SupportFunctions/arm_*.c: the final #else of ARM_MATH_MVE* / ARM_MATH_NEON, no ARM_MATH_DSP, with
// ARM_MATH_LOOPUNROLL and without ARM_MATH_ROUNDING).  arm_weighted_average_f32 is an operation of the f32 chain
// kernels (statistics.hip); the sorts are in sort.hip.
//
//   One streaming kernel over the batch's words as one flat array, templated on (source type, destination type,
//   operation), the plan of basic_ew_kernel (basic_math.hip).  A lane's unit is one 16-B pack of the narrower type
//   (4 / 8 / 16 elements), so the wider stream moves 1, 2 or 4 packs per unit; 16-B loads and stores when both
//   pointers are 16-B aligned, kSpUnroll units in flight per lane; one element per lane otherwise and for the ragged
//   end.  copy is the same-type case; fill has no source, its value is a kernel argument.  A lane reads its elements
//   before it writes them, so dst may be src exactly where the element widths are equal.
//
//   float -> q   p = x * 2^31 / 2^15 / 2^7 rounded to f32 (subnormals kept), truncated toward zero, then clipped to
//                32 bits (q31) or __SSAT to 16 / 8 bits.  Where the reference's C cast is defined (|p| < 2^63 for q31,
//                |p| < 2^31 otherwise) the explicit clamp of p to [-2^31, 2^31) before the cast gives the same word;
//                outside it saturates by sign, and NaN gives 0.
//   q -> float   (float)x / 2^31 / 2^15 / 2^7: the int -> float step rounds to nearest even (q31 only; q15, q7 are
//                exact), the division by a power of two is exact, written as the multiplication by its inverse.
//   q -> q       << 16, << 24, << 8 widening; arithmetic >> 16, >> 24, >> 8 narrowing.
//   barycenter   one lane per (item, dimension): out = out + in[v][d] * w[v] over v in order from 0.0f, accum += w in
//                the same order, out / accum (a division, as the reference's scalar branch).  Neighbouring lanes read
//                neighbouring d, so the loads coalesce.
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

enum : int { kSpConvert = 0, kSpFill = 1 };

// float -> int32_t as the reference's cast where that is defined: toward zero; saturating by sign outside; NaN: 0.
__device__ __forceinline__ int32_t trunc_sat(float p) {
  if (!(p == p)) return 0;
  if (p >= 2147483648.0f) return INT32_MAX;
  if (p <= -2147483648.0f) return INT32_MIN;
  return (int32_t)p;
}

template <typename S, typename D>
__device__ __forceinline__ D sp_elem(S x) {
  constexpr bool sf = std::is_same<S, float>::value, df = std::is_same<D, float>::value;
  if constexpr (std::is_same<S, D>::value) {
    return x;
  } else if constexpr (sf) {
    if constexpr (sizeof(D) == 4) return trunc_sat(x * 2147483648.0f);
    else if constexpr (sizeof(D) == 2) return (D)ssat16(trunc_sat(x * 32768.0f));
    else return (D)ssat8(trunc_sat(x * 128.0f));
  } else if constexpr (df) {
    constexpr float inv = sizeof(S) == 4 ? 4.656612873077392578125e-10f : sizeof(S) == 2 ? 3.0517578125e-05f : 0.0078125f;
    return (float)(int32_t)x * inv;
  } else if constexpr (sizeof(S) < sizeof(D)) {
    return (D)wshl((int32_t)x, 8 * (int)(sizeof(D) - sizeof(S)));
  } else {
    return (D)((int32_t)x >> (8 * (int)(sizeof(S) - sizeof(D))));
  }
}

constexpr int kSpUnroll = 4;   // units per lane and tile

// count: words of the whole batch.  vec: s and d are 16-B aligned.  OP == kSpFill: s is unused, every word is value.
template <int OP, typename S, typename D>
__global__ __launch_bounds__(kBlock) void support_ew_kernel(const S* s, D* d, size_t count, bool vec, D value) {
  constexpr int V = 16 / (sizeof(S) < sizeof(D) ? sizeof(S) : sizeof(D)), U = kSpUnroll;   // elements per unit
  constexpr int PS = V * sizeof(S) / 16, PD = V * sizeof(D) / 16;                          // packs per unit
  struct alignas(16) Unit16 { uint32_t w[4]; };
  struct SrcUnit { Unit16 p[PS]; };
  struct DstUnit { Unit16 p[PD]; };
  const size_t units = vec ? count / V : 0;
  for (size_t tile = blockIdx.x; tile * (U * kBlock) < units; tile += gridDim.x) {
    const size_t i0 = tile * (U * kBlock) + threadIdx.x;
    SrcUnit x[U];
    if constexpr (OP == kSpConvert) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t i = i0 + u * kBlock;
        if (i < units) {
#pragma unroll
          for (int q = 0; q < PS; ++q) x[u].p[q] = ((const Unit16*)s)[i * PS + q];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * kBlock;
      if (i < units) {
        S xs[V];
        D r[V];
        DstUnit o;
        if constexpr (OP == kSpConvert) __builtin_memcpy(xs, &x[u], sizeof(xs));
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = OP == kSpFill ? value : sp_elem<S, D>(xs[j]);
        __builtin_memcpy(&o, r, sizeof(o));
#pragma unroll
        for (int q = 0; q < PD; ++q) ((Unit16*)d)[i * PD + q] = o.p[q];
      }
    }
  }
  // the ragged end, or everything when a pointer is not 16-B aligned: one element per lane
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = units * V + (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
    if constexpr (OP == kSpFill) d[i] = value;
    else d[i] = sp_elem<S, D>(s[i]);
  }
}

template <int OP, typename S, typename D>
hipError_t sp_launch(const S* s, D* d, size_t count, D value, hipStream_t st) {
  if (count == 0) return hipSuccess;
  const bool vec = (((OP == kSpFill ? (uintptr_t)0 : (uintptr_t)s) | (uintptr_t)d) & 15) == 0;
  constexpr size_t V = 16 / (sizeof(S) < sizeof(D) ? sizeof(S) : sizeof(D));
  const size_t per = vec ? V * kSpUnroll * kBlock : kBlock;      // words a workgroup takes per step
  const size_t blocks = (count + per - 1) / per;
  const size_t cap = 0x7fffffff;
  const uint32_t grid = (uint32_t)(blocks < cap ? blocks : cap);
  hipLaunchKernelGGL((support_ew_kernel<OP, S, D>), dim3(grid), dim3(kBlock), 0, st, s, d, count, vec, value);
  return hipGetLastError();
}

// One lane per (item, dimension).
__global__ __launch_bounds__(kBlock) void barycenter_kernel(const float* in, const float* w, size_t wStride, float* out,
                                                            uint32_t nbVectors, uint32_t vecDim, size_t total) {
  const size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const size_t item = idx / vecDim;
  const uint32_t d = (uint32_t)(idx - item * vecDim);
  const float* pin = in + item * ((size_t)nbVectors * vecDim) + d;
  const float* pw = w + item * wStride;
  float acc = 0.0f, accum = 0.0f;
  for (uint32_t v = 0; v < nbVectors; ++v) {
    const float wv = pw[v];
    accum = accum + wv;
    const float t = pin[(size_t)v * vecDim] * wv;
    acc = acc + t;
  }
  out[idx] = acc / accum;
}

}  // namespace

template <typename S, typename D>
hipError_t support_convert_launch(const S* s, D* d, size_t count, hipStream_t st) {
  return sp_launch<kSpConvert, S, D>(s, d, count, (D)0, st);
}
template <typename T>
hipError_t support_fill_launch(T value, T* d, size_t count, hipStream_t st) {
  return sp_launch<kSpFill, T, T>((const T*)nullptr, d, count, value, st);
}
#define MI355X_SUPPORT_CONVERT(S, D) \
  template hipError_t support_convert_launch<S, D>(const S*, D*, size_t, hipStream_t);
#define MI355X_SUPPORT_TYPE(T)       \
  MI355X_SUPPORT_CONVERT(T, float)   \
  MI355X_SUPPORT_CONVERT(T, int32_t) \
  MI355X_SUPPORT_CONVERT(T, int16_t) \
  MI355X_SUPPORT_CONVERT(T, int8_t)  \
  template hipError_t support_fill_launch<T>(T, T*, size_t, hipStream_t);
MI355X_SUPPORT_TYPE(float)
MI355X_SUPPORT_TYPE(int32_t)
MI355X_SUPPORT_TYPE(int16_t)
MI355X_SUPPORT_TYPE(int8_t)
#undef MI355X_SUPPORT_TYPE
#undef MI355X_SUPPORT_CONVERT

hipError_t barycenter_launch(const float* in, const float* w, size_t wStride, float* out, uint32_t nbVectors,
                             uint32_t vecDim, uint32_t batch, hipStream_t st) {
  const size_t total = (size_t)batch * vecDim;
  if (total == 0) return hipSuccess;
  const size_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(barycenter_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, st, in, w, wStride, out, nbVectors,
                     vecDim, total);
  return hipGetLastError();
}

}  // namespace mi355x
