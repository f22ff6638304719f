// The pieces cmplx_math.hip and statistics.hip share: the lanes-per-item mapping of the reductions, the
// (value, index) search kernel, and the fixed-point square roots (arm_sqrt_q31.c, arm_sqrt_q15.c).
//
//   mapping   An item of `chunks` loads gets lpi lanes: the power of two that leaves a lane about kRedLoads loads,
//             at most a wave; short items are packed kBlock / lpi to a workgroup; items of more than kRedWaveMax
//             loads get the whole workgroup.  16-B loads when every item starts 16-B aligned and holds whole
//             packs, one element per load otherwise.  The lanes' partial results meet in a butterfly of lane
//             shuffles (and four LDS words for a whole workgroup).
//   search    (value, index) pairs: the better value wins, equal values keep the lower index, a NaN never enters a
//             pair.  MAP maps an element before it is compared (the abs searches).
#pragma once
#include <cfloat>
#include <limits>
#include <type_traits>

#include "common.hpp"
#include "mfcc_fixed_ops.hpp"

namespace mi355x {
namespace {

// (int32_t)(((int64_t)a * b) >> s) for 0 <= s <= 31: bits s .. s + 31 of the signed product, taken from its two
// halves with one v_alignbit.  Written out because the compiler builds the 64-bit shifts of arm_sqrt_q31 from
// about twice as many instructions, and the q15 magnitude is bound by instruction issue.
__device__ __forceinline__ int32_t mulshr(int32_t a, int32_t b, int s) {
  return (int32_t)__builtin_amdgcn_alignbit((uint32_t)mulhi(a, b), (uint32_t)a * (uint32_t)b, (uint32_t)s);
}

// arm_sqrt_q31.c:55-125 with the start value read from lut (LDS): Newton on 1 / sqrt, 3 iterations.
__device__ __forceinline__ int32_t cm_sqrt_q31(int32_t in, const int32_t* lut) {
  // branch-free: in <= 0 runs the same arithmetic on a masked table index and selects 0 at the end
  const int e = ((int)mq_clz((uint32_t)in) - 1) & 30;       // signBits1 rounded down to even
  const int32_t number = wshl(in, e);
  int32_t v = lut[((number >> 26) - (0x20000000 >> 26)) & 31];
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    int32_t t = mulshr(v, v, 28);
    t = mulshr(number, t, 31);
    t = wsub(0x30000000, t);
    v = mulshr(v, t, 29);
  }
  v = mulshr(number, v, 28);
  return in > 0 ? v >> (e >> 1) : 0;
}

// Word k of arm_sqrt_q15.c's start table: round(2^13 / sqrt(1 + k / 4)) = round(2^14 / sqrt(4 + k)), the q12
// reciprocal root of the q15 number (4 + k) / 16.  w is that rounding exactly when (2w - 1)^2 (4 + k) <= 2^30
// < (2w + 1)^2 (4 + k); no tie is possible, since 2^15 / sqrt(4 + k) is an odd integer for no k.
constexpr int16_t sqrt_q15_seed(int k) {
  int64_t w = 1;
  while ((2 * w + 1) * (2 * w + 1) * (4 + k) <= ((int64_t)1 << 30)) ++w;
  return (int16_t)w;
}
#define MI355X_SQ15(k) sqrt_q15_seed(k), sqrt_q15_seed(k + 1), sqrt_q15_seed(k + 2), sqrt_q15_seed(k + 3)
constexpr int16_t kSqrtLutQ15[16] = {MI355X_SQ15(0), MI355X_SQ15(4), MI355X_SQ15(8), MI355X_SQ15(12)};
#undef MI355X_SQ15

// arm_sqrt_q15.c:55-135: Newton on 1 / sqrt, 3 iterations, every assignment truncated to 16 bits as its q15_t
// variables do.  lut: the 16 start words (LDS or a local copy).  in <= 0 gives 0.
template <typename LUT>
__host__ __device__ __forceinline__ int16_t cm_sqrt_q15(int16_t in, const LUT* lut) {
  if (in <= 0) return 0;
  const int sb = __builtin_clz((uint32_t)in) - 17, e = sb & ~1;
  const int16_t number = (int16_t)((int32_t)in << e);
  int16_t v = (int16_t)lut[((number >> 11) - (0x2000 >> 11)) & 15];
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    int16_t t = (int16_t)(((int32_t)v * v) >> 12);
    t = (int16_t)(((int32_t)number * t) >> 15);
    t = (int16_t)(0x3000 - t);
    v = (int16_t)(((int32_t)v * t) >> 13);
  }
  v = (int16_t)(((int32_t)number * v) >> 12);
  return (int16_t)(v >> (e >> 1));
}

// ---- the mapping ---------------------------------------------------------------------------------------------
constexpr int kRedLoads = 2;
constexpr uint32_t kRedWaveMax = 64 * 8;
inline int red_lpi_log(uint64_t chunks) {
  if (chunks > kRedWaveMax) return 8;
  int l = 0;
  while (l < 6 && ((uint64_t)kRedLoads << l) < chunks) ++l;
  return l;
}

// ---- search --------------------------------------------------------------------------------------------------
template <typename T> struct Best {
  T v;
  uint32_t i;
  bool has;
};

template <bool MAX, typename T>
__device__ __forceinline__ void best_take(Best<T>& s, T x, uint32_t i) {
  // a NaN fails x == x and never enters; the scan runs with i ascending, so a tie keeps the earlier index
  if (x == x && (!s.has || (MAX ? s.v < x : s.v > x))) { s.v = x; s.i = i; s.has = true; }
}
template <bool MAX, typename T>
__device__ __forceinline__ void best_merge(Best<T>& s, const Best<T>& o) {
  if (o.has && (!s.has || (MAX ? s.v < o.v : s.v > o.v) || (s.v == o.v && o.i < s.i))) s = o;
}
template <typename T>
__device__ __forceinline__ Best<T> best_shfl_xor(const Best<T>& s, int m) {
  using W = typename std::conditional<std::is_same<T, float>::value, float, int>::type;
  Best<T> o;
  o.v = (T)__shfl_xor((W)s.v, m, 64);
  o.i = (uint32_t)__shfl_xor((int)s.i, m, 64);
  o.has = __shfl_xor((int)s.has, m, 64) != 0;
  return o;
}

struct MapNone {
  template <typename T> __device__ __forceinline__ static T map(T x) { return x; }
};
// arm_abs{max,min}*: (x > 0) ? x : -x, the negation saturating in fixed point.  f32: +0.0 becomes -0.0 and a
// NaN keeps its payload with the sign flipped.
struct MapAbs {
  template <typename T> __device__ __forceinline__ static T map(T x) {
    if constexpr (std::is_same<T, float>::value) {
      return (x > 0.0f) ? x : -x;
    } else {
      constexpr T lo = std::numeric_limits<T>::min(), hi = std::numeric_limits<T>::max();
      return x > 0 ? x : (x == lo ? hi : (T)-x);
    }
  }
};

// result[item], index[item] (index may be null) = the extreme of MAP(src[item]) and its first index.
// FLOOR false: the reference's searches that start from element 0 (n > 0): item word 0 is stored as it is
// (mapped) when it is a NaN, since no comparison with it is true.  FLOOR true (f32 only): arm_max_no_idx_f32 /
// arm_min_no_idx_f32, which start from -FLT_MAX / FLT_MAX and replace it on a strict comparison only: a NaN never
// wins, an item with nothing beyond the start value (n == 0 included) returns the start value.
// wide: every item starts 16-B aligned and holds a whole number of 16-B packs.
template <bool MAX, typename T, typename MAP, bool FLOOR>
__global__ __launch_bounds__(kBlock) void search_kernel(const T* src, uint32_t n, T* result, uint32_t* index,
                                                        uint32_t batch, int lpiLog, bool wide) {
  constexpr int V = 16 / sizeof(T);
  struct alignas(16) Pack { T v[V]; };
  __shared__ Best<T> part[kBlock / 64];
  const uint32_t lpi = 1u << lpiLog, ipw = kBlock >> lpiLog;
  const uint32_t li = threadIdx.x >> lpiLog, l = threadIdx.x & (lpi - 1);
  const uint32_t item = blockIdx.x * ipw + li;
  const bool live = item < batch;
  const T* s = src + (size_t)(live ? item : 0) * n;
  Best<T> b{(T)0, 0u, false};
  if (live) {
    if (wide) {
      for (uint64_t c = l; c < n / V; c += lpi) {          // 64-bit: c + lpi may pass 2^32
        const Pack p = ((const Pack*)s)[c];
#pragma unroll
        for (int j = 0; j < V; ++j) best_take<MAX, T>(b, MAP::map(p.v[j]), (uint32_t)(c * V + j));
      }
    } else {
      for (uint64_t k = l; k < n; k += lpi) best_take<MAX, T>(b, MAP::map(s[k]), (uint32_t)k);
    }
  }
  const int waveLanes = lpiLog < 6 ? lpiLog : 6;
  for (int m = 1; m < (1 << waveLanes); m <<= 1) best_merge<MAX, T>(b, best_shfl_xor(b, m));
  if (lpiLog > 6) {            // the whole workgroup on one item
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < kBlock / 64; ++w) best_merge<MAX, T>(b, part[w]);
  }
  if (live && l == 0) {
    if constexpr (FLOOR) {
      const T start = MAX ? (T)-FLT_MAX : (T)FLT_MAX;
      result[item] = (b.has && (MAX ? start < b.v : start > b.v)) ? b.v : start;
    } else {
      const T first = MAP::map(s[0]);
      const bool pin = !(first == first) || !b.has;      // word 0 a NaN: it is never replaced
      result[item] = pin ? first : b.v;
      if (index) index[item] = pin ? 0u : b.i;
    }
  }
}

template <bool MAX, typename T, typename MAP, bool FLOOR>
hipError_t search_run(const T* src, uint32_t n, T* result, uint32_t* index, uint32_t batch, hipStream_t st) {
  constexpr uint32_t V = 16 / sizeof(T);
  const bool wide = (((uintptr_t)src | ((size_t)n * sizeof(T))) & 15) == 0;
  const int lpiLog = red_lpi_log(wide ? n / V : n);
  const uint32_t ipw = kBlock >> lpiLog;
  const uint64_t grid = ((uint64_t)batch + ipw - 1) / ipw;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL((search_kernel<MAX, T, MAP, FLOOR>), dim3((uint32_t)grid), dim3(kBlock), 0, st, src, n, result,
                     index, batch, lpiLog, wide);
  return hipGetLastError();
}

}  // namespace
}  // namespace mi355x
