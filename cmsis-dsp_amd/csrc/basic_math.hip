// arm_{add,sub,mult,offset,scale,clip,abs,negate}_{f32,q31,q15,q7}, arm_shift_{q31,q15,q7} and
// arm_{and,or,xor,not}_{u32,u16,u8} over a batch of contiguous items, bit-exact with the reference's scalar branches
// (Source/BasicMathFunctions/arm_*.c: the final #else of ARM_MATH_MVE* / ARM_MATH_NEON, no ARM_MATH_DSP, with
// ARM_MATH_LOOPUNROLL).  The four arm_dot_prod_* are operations of the sum kernels (statistics.hip).
//
//   One streaming kernel over the batch's words as one flat array, templated on the operation and the element
//   type.  A lane's unit is one 16-B pack of every stream (4 / 8 / 16 elements), moved with 16-B loads and stores
//   when every pointer is 16-B aligned, kBmUnroll packs in flight per lane; one element per lane otherwise and for
//   the ragged end.  A lane reads its elements before it writes them, so dst may be a source exactly.  The scalars
//   (offset, scale and shift, low and high) are kernel arguments; the operations are separated with if constexpr.
//
//   q31   add / sub / offset: the 64-bit sum clipped (__QADD, __QSUB, clip_q63_to_q31).  mult: __SSAT(hi32(a*b), 31)
//         << 1.  scale: in = hi32(x * scale), then << kShift with saturation or >> -kShift (kShift = shift + 1);
//         shift: the same on x itself.  The saturating left shift is clip((q63_t)in << k): the reference's test
//         `in != (out >> k)` on the wrapped 32-bit out is true exactly when the 64-bit value leaves 32 bits.
//   q15   __SSAT(.., 16) of a + b, a - b, (a*b) >> 15, x + offset, (x*scale) >> (15 - shift); shift left:
//         __SSAT((q31_t)x << s, 16) with the 32-bit product of the shift wrapped first (s > 16 shows it).
//   q7    as q15 with 8 bits: (a*b) >> 7, (x*scale) >> (7 - shift).
//   abs / negate saturate the most negative word to the most positive; abs_f32 clears the sign bit, negate_f32
//   flips it.  clip: x > high ? high : x < low ? low : x (a NaN passes; low > high: the first comparison wins).
#include <limits>
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

template <typename T> constexpr bool kIsF32 = std::is_same<T, float>::value;
template <typename T> constexpr bool kIsBits = std::is_unsigned<T>::value;

__device__ __forceinline__ int32_t clip64(int64_t v) {
  return v > INT32_MAX ? INT32_MAX : (v < INT32_MIN ? INT32_MIN : (int32_t)v);
}
// __SSAT(v, 8 * sizeof(T))
template <typename T> __device__ __forceinline__ T ssat_to(int32_t v) {
  return (T)(sizeof(T) == 2 ? ssat16(v) : ssat8(v));
}

// One element.  s0: offset, scale or low; s1: high; sh: shift (shiftBits), scale (kShift: q31 shift + 1 with the
// sign telling the direction, q15 15 - shift, q7 7 - shift).
template <int OP, typename T>
__device__ __forceinline__ T bm_elem(T a, T b, T s0, T s1, int sh) {
  if constexpr (kIsBits<T>) {
    if constexpr (OP == kBmAnd) return (T)(a & b);
    else if constexpr (OP == kBmOr) return (T)(a | b);
    else if constexpr (OP == kBmXor) return (T)(a ^ b);
    else return (T)~a;
  } else if constexpr (OP == kBmClip) {
    return a > s1 ? s1 : (a < s0 ? s0 : a);
  } else if constexpr (kIsF32<T>) {
    if constexpr (OP == kBmAdd) return a + b;
    else if constexpr (OP == kBmSub) return a - b;
    else if constexpr (OP == kBmMult) return a * b;
    else if constexpr (OP == kBmOffset) return a + s0;
    else if constexpr (OP == kBmScale) return a * s0;
    else if constexpr (OP == kBmAbs) return __builtin_fabsf(a);
    else return -a;
  } else if constexpr (OP == kBmAbs || OP == kBmNegate) {
    constexpr T lo = std::numeric_limits<T>::min(), hi = std::numeric_limits<T>::max();
    if (OP == kBmAbs && a > 0) return a;
    return a == lo ? hi : (T)-a;
  } else if constexpr (std::is_same<T, int32_t>::value) {
    if constexpr (OP == kBmAdd) return clip64((int64_t)a + b);
    else if constexpr (OP == kBmSub) return clip64((int64_t)a - b);
    else if constexpr (OP == kBmOffset) return clip64((int64_t)a + s0);
    else if constexpr (OP == kBmMult) {
      const int32_t p = mulhi(a, b);                      // only min * min leaves 31 bits, upwards
      return wshl(p > 0x3FFFFFFF ? 0x3FFFFFFF : p, 1);
    } else {                                              // scale, shift
      const int32_t in = OP == kBmScale ? mulhi(a, s0) : a;
      return sh >= 0 ? clip64((int64_t)((uint64_t)(int64_t)in << sh)) : in >> -sh;
    }
  } else {
    const int32_t x = a, y = b;
    if constexpr (OP == kBmAdd) return ssat_to<T>(x + y);
    else if constexpr (OP == kBmSub) return ssat_to<T>(x - y);
    else if constexpr (OP == kBmMult) return ssat_to<T>((x * y) >> (sizeof(T) == 2 ? 15 : 7));
    else if constexpr (OP == kBmOffset) return ssat_to<T>(x + (int32_t)s0);
    else if constexpr (OP == kBmScale) return ssat_to<T>((x * (int32_t)s0) >> sh);
    else return sh >= 0 ? ssat_to<T>(wshl(x, sh)) : (T)(x >> -sh);   // shift
  }
}

constexpr int kBmUnroll = 4;   // packs per lane and tile

template <int OP> constexpr bool kBmTwo = OP == kBmAdd || OP == kBmSub || OP == kBmMult || OP == kBmAnd ||
                                          OP == kBmOr || OP == kBmXor;

// count: words of the whole batch.  vec: a, b and d are 16-B aligned.
template <int OP, typename T>
__global__ __launch_bounds__(kBlock) void basic_ew_kernel(const T* a, const T* b, T* d, size_t count, bool vec, T s0,
                                                          T s1, int sh) {
  constexpr int V = 16 / sizeof(T), U = kBmUnroll;
  struct alignas(16) Pack { T v[V]; };
  const size_t packs = vec ? count / V : 0;
  for (size_t tile = blockIdx.x; tile * (U * kBlock) < packs; tile += gridDim.x) {
    const size_t i0 = tile * (U * kBlock) + threadIdx.x;
    Pack x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * kBlock;
      if (i < packs) {
        x[u] = ((const Pack*)a)[i];
        if constexpr (kBmTwo<OP>) y[u] = ((const Pack*)b)[i];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * kBlock;
      if (i < packs) {
        Pack r;
        if constexpr (kIsBits<T>) {                        // bitwise: the pack's four 32-bit words, whatever T's width
          uint32_t xw[4], yw[4] = {}, rw[4];
          __builtin_memcpy(xw, &x[u], 16);
          if constexpr (kBmTwo<OP>) __builtin_memcpy(yw, &y[u], 16);
#pragma unroll
          for (int j = 0; j < 4; ++j) rw[j] = bm_elem<OP, uint32_t>(xw[j], yw[j], 0u, 0u, 0);
          __builtin_memcpy(&r, rw, 16);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) r.v[j] = bm_elem<OP, T>(x[u].v[j], kBmTwo<OP> ? y[u].v[j] : (T)0, s0, s1, sh);
        }
        ((Pack*)d)[i] = r;
      }
    }
  }
  // the ragged end, or everything when a pointer is not 16-B aligned: one element per lane
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = packs * V + (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
    const T x = a[i];
    T y = (T)0;
    if constexpr (kBmTwo<OP>) y = b[i];
    d[i] = bm_elem<OP, T>(x, y, s0, s1, sh);
  }
}

template <int OP, typename T>
hipError_t bm_launch(const T* a, const T* b, T* d, size_t count, T s0, T s1, int sh, hipStream_t st) {
  const bool vec = (((uintptr_t)a | (uintptr_t)(kBmTwo<OP> ? b : a) | (uintptr_t)d) & 15) == 0;
  constexpr size_t V = 16 / sizeof(T);
  const size_t per = vec ? V * kBmUnroll * kBlock : kBlock;      // words a workgroup takes per step
  const size_t blocks = (count + per - 1) / per;
  const size_t cap = 0x7fffffff;
  const uint32_t grid = (uint32_t)(blocks < cap ? blocks : cap);
  hipLaunchKernelGGL((basic_ew_kernel<OP, T>), dim3(grid), dim3(kBlock), 0, st, a, b, d, count, vec, s0, s1, sh);
  return hipGetLastError();
}

}  // namespace

template <typename T>
hipError_t basic_ew_launch(int op, const T* a, const T* b, T* d, size_t count, T s0, T s1, int sh, hipStream_t st) {
  if (count == 0) return hipSuccess;
  if constexpr (kIsBits<T>) {
    switch (op) {
      case kBmAnd: return bm_launch<kBmAnd, T>(a, b, d, count, s0, s1, sh, st);
      case kBmOr: return bm_launch<kBmOr, T>(a, b, d, count, s0, s1, sh, st);
      case kBmXor: return bm_launch<kBmXor, T>(a, b, d, count, s0, s1, sh, st);
      case kBmNot: return bm_launch<kBmNot, T>(a, b, d, count, s0, s1, sh, st);
    }
  } else {
    switch (op) {
      case kBmAdd: return bm_launch<kBmAdd, T>(a, b, d, count, s0, s1, sh, st);
      case kBmSub: return bm_launch<kBmSub, T>(a, b, d, count, s0, s1, sh, st);
      case kBmMult: return bm_launch<kBmMult, T>(a, b, d, count, s0, s1, sh, st);
      case kBmOffset: return bm_launch<kBmOffset, T>(a, b, d, count, s0, s1, sh, st);
      case kBmScale: return bm_launch<kBmScale, T>(a, b, d, count, s0, s1, sh, st);
      case kBmClip: return bm_launch<kBmClip, T>(a, b, d, count, s0, s1, sh, st);
      case kBmAbs: return bm_launch<kBmAbs, T>(a, b, d, count, s0, s1, sh, st);
      case kBmNegate: return bm_launch<kBmNegate, T>(a, b, d, count, s0, s1, sh, st);
      case kBmShift:
        if constexpr (!kIsF32<T>) return bm_launch<kBmShift, T>(a, b, d, count, s0, s1, sh, st);
        break;
    }
  }
  return hipErrorInvalidValue;
}
#define MI355X_BASIC_EW(T) \
  template hipError_t basic_ew_launch<T>(int, const T*, const T*, T*, size_t, T, T, int, hipStream_t);
MI355X_BASIC_EW(float)
MI355X_BASIC_EW(int32_t)
MI355X_BASIC_EW(int16_t)
MI355X_BASIC_EW(int8_t)
MI355X_BASIC_EW(uint32_t)
MI355X_BASIC_EW(uint16_t)
MI355X_BASIC_EW(uint8_t)
#undef MI355X_BASIC_EW

}  // namespace mi355x
