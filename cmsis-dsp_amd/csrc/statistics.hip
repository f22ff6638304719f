// arm_{mean,power,rms,var,std,mse}_{f32,q31,q15,q7}, arm_accumulate_f32 and arm_{max,min,absmax,absmin}[_no_idx]_*
// over a batch of contiguous items, one result word per item, bit-exact with the reference's scalar branches
// (Source/StatisticsFunctions/arm_*.c: the final #else of ARM_MATH_MVE* / ARM_MATH_NEON, no ARM_MATH_DSP, with
// ARM_MATH_LOOPUNROLL; FastMathFunctions/arm_sqrt_q31.c, arm_sqrt_q15.c).
//
//   integer sums   the lanes-per-item mapping of reduce_lanes.hpp (as max / min and the integer dot products use
//                  it).  One kernel, templated on the operation and the type: an element (mse: a pair) gives one
//                  term, var / std two (the element and its square), summed mod 2^64 -- associative, so the
//                  lanes' partial sums meet in a butterfly.  Inside a 16-B pack q7 / q15 terms are first summed
//                  in 32 bits where that cannot overflow (16 q7 terms; 8 q15 elements; 2 q15 squares).  One lane
//                  per item then does the reference's divisions, shifts, saturations and square root.  The
//                  reference's 32-bit sums (mean_q7 / q15, var / std_q15, power_q7, mse_q7) are the low 32 bits
//                  of the 64-bit ones whenever they do not overflow (where they do, the reference is undefined).
//   searches       search_kernel of reduce_lanes.hpp with the element mapped first (abs), without the index
//                  (_no_idx), or from the start value -FLT_MAX / FLT_MAX (max / min_no_idx_f32).
//   f32 chains     sum = sum + term, element by element from 0.0f, the term rounded before the add: an ordered
//                  chain, as dot_prod_f32 (cmplx_math.hip).  From kSumLaneMinBatch items on: one lane per item, the
//                  workgroup staging kSumChunk words of its 256 items in LDS with coalesced row-segment loads.
//                  Below: one wave per item; the wave loads 64 elements, every lane forms its element's term, and
//                  the chain takes them in order through v_readlane (one dependent add per element).  var / std
//                  run the mean's chain first and then the chain of (x - mean)^2: the wave form keeps an item
//                  of up to kVarKeep words in LDS for the second pass and reads a longer one again; the lane form
//                  always reads it again.
//   dot products   arm_dot_prod_* (kStDot) are one more operation of these kernels: the term is a*b (q31: >> 14), the
//                  second source's items are bStride words apart (0: one for every item, which the lane form stages
//                  once per row all the same; mse passes the item length).
//   weighted mean  arm_weighted_average_f32 (kStWavg): the dot product's chain of in*w beside a second chain of w in
//                  the same element order, then one IEEE division sum / wsum (blockSize 0: 0 / 0).
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"
#include "chain_f32.hpp"
#include "reduce_lanes.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

template <typename T> constexpr bool kIsQ31 = std::is_same<T, int32_t>::value;
template <int OP> constexpr bool kIsVar = OP == kStVar || OP == kStStd;
// kStDot: arm_dot_prod_*, kStWavg: arm_weighted_average_f32
template <int OP> constexpr bool kTwoSources = OP == kStMse || OP == kStDot || OP == kStWavg;

__device__ __forceinline__ int32_t ssat8(int32_t v) { return v > 127 ? 127 : (v < -128 ? -128 : v); }

// ---- integer sums ------------------------------------------------------------------------------------------
// The term of one element that goes into the first sum: int64_t for q31, otherwise an int32_t (a square: below
// 2^31).  b: the second source's element (mse).
template <int OP, typename T>
__device__ __forceinline__ auto sum_term0(T a, T b) {
  const int32_t x = a, y = b;
  if constexpr (kIsQ31<T>) {
    if constexpr (OP == kStMean) return (int64_t)x;
    else if constexpr (OP == kStPower) return ((int64_t)x * x) >> 14;
    else if constexpr (OP == kStRms) return (int64_t)x * x;
    else if constexpr (kIsVar<OP>) return (int64_t)(x >> 8);
    else if constexpr (OP == kStDot) return ((int64_t)x * y) >> 14;
    else {                                                  // mse: __QSUB of the halves
      int64_t d = (int64_t)(x >> 1) - (int64_t)(y >> 1);
      d = d > INT32_MAX ? INT32_MAX : (d < INT32_MIN ? INT32_MIN : d);
      return (d * d) >> 14;
    }
  } else {
    if constexpr (OP == kStMean || kIsVar<OP>) return x;
    else if constexpr (OP == kStPower || OP == kStRms) return x * x;
    else if constexpr (OP == kStDot) return x * y;
    else {
      const int32_t d = sizeof(T) == 2 ? ssat16((x >> 1) - (y >> 1)) : ssat8((x >> 1) - (y >> 1));
      return d * d;
    }
  }
}
// var / std: the square that goes into the second sum.
template <typename T>
__device__ __forceinline__ auto sum_term1(T a) {
  if constexpr (kIsQ31<T>) {
    const int64_t in = (int32_t)a >> 8;
    return in * in;
  } else {
    return (int32_t)a * (int32_t)a;
  }
}

template <int OP, typename T>
__device__ __forceinline__ void sum_take(uint64_t& s0, uint64_t& s1, T a, T b) {
  s0 += (uint64_t)(int64_t)sum_term0<OP, T>(a, b);
  if constexpr (kIsVar<OP>) s1 += (uint64_t)(int64_t)sum_term1<T>(a);
}

// One 16-B pack.  q7 / q15: groups of G terms are summed in 32 bits first: every element when the terms are the
// elements themselves or q7 squares (16 x 2^14), pairs of q15 squares (2 x 2^30 < 2^32).  The dot products' terms are
// signed: 16 q7 products fit 32 bits, two q15 products (min * min twice: 2^31) do not.
template <int OP, typename T, int V>
__device__ __forceinline__ void sum_take_pack(uint64_t& s0, uint64_t& s1, const T* x, const T* y) {
  if constexpr (kIsQ31<T>) {
#pragma unroll
    for (int j = 0; j < V; ++j) sum_take<OP, T>(s0, s1, x[j], y[j]);
  } else {
    constexpr bool kPlain = OP == kStMean || kIsVar<OP> || OP == kStDot;   // signed terms
    constexpr int G0 = OP == kStDot ? (sizeof(T) == 1 ? V : 1) : (kPlain || sizeof(T) == 1) ? V : 2;
#pragma unroll
    for (int g = 0; g < V; g += G0) {
      uint32_t p = 0;
#pragma unroll
      for (int j = 0; j < G0; ++j) p += (uint32_t)sum_term0<OP, T>(x[g + j], y[g + j]);
      s0 += kPlain ? (uint64_t)(int64_t)(int32_t)p : (uint64_t)p;
    }
    if constexpr (kIsVar<OP>) {
#pragma unroll
      for (int g = 0; g < V; g += 2) s1 += (uint64_t)((uint32_t)sum_term1<T>(x[g]) + (uint32_t)sum_term1<T>(x[g + 1]));
    }
  }
}

// sum / (int32_t)blockSize of mean_q7 / mean_q15 in 32 bits (a 64-bit division costs several times as much, once
// per item); d == -1 (blockSize 2^32 - 1) is the one divisor a 32-bit division could overflow on.
__device__ __forceinline__ int32_t div_q31(int32_t s, int32_t d) { return d == -1 ? wsub(0, s) : s / d; }

// The reference's epilogue on the item's sums.  lut: sqrt_initial_lut_q31 in LDS (q31 rms / std).
template <int OP, typename T, typename R>
__device__ __forceinline__ R sum_finish(uint64_t s0, uint64_t s1, uint32_t n, const int32_t* lut) {
  if constexpr (OP == kStPower || OP == kStDot) {
    return (R)(int64_t)s0;                                  // q7: the low 32 bits
  } else if constexpr (kIsVar<OP>) {
    if (n <= 1u) return (R)0;
    const int64_t den = (int64_t)(uint32_t)(n * (n - 1u));  // the reference's uint32_t product: wraps from 65537 on
    if constexpr (kIsQ31<T>) {
      const int64_t meanOfSquares = (int64_t)s1 / (int64_t)(n - 1u);
      const int64_t squareOfMean = (int64_t)(s0 * s0) / den;
      const int32_t d = (int32_t)((int64_t)((uint64_t)meanOfSquares - (uint64_t)squareOfMean) >> 15);
      return (R)(OP == kStVar ? d : cm_sqrt_q31(d, lut));
    } else {
      const int32_t sum = (int32_t)s0;
      const int32_t meanOfSquares = (int32_t)((int64_t)s1 / (int64_t)(n - 1u));
      const int32_t squareOfMean = (int32_t)(((int64_t)sum * sum) / den);
      const int32_t d = wsub(meanOfSquares, squareOfMean) >> 15;
      return (R)(OP == kStVar ? (int16_t)d : cm_sqrt_q15((int16_t)ssat16(d), kSqrtLutQ15));
    }
  } else if constexpr (kIsQ31<T>) {
    if constexpr (OP == kStMean) return (R)((int64_t)s0 / (int64_t)n);
    else if constexpr (OP == kStMse) return (R)(((int64_t)s0 / (int64_t)n) >> 15);
    else {                                                  // rms: an unsigned sum and an unsigned division
      const uint64_t u = (s0 / (uint64_t)n) >> 31;
      return (R)cm_sqrt_q31(u > (uint64_t)INT32_MAX ? INT32_MAX : (int32_t)u, lut);   // clip_q63_to_q31
    }
  } else if constexpr (sizeof(T) == 2) {
    if constexpr (OP == kStMean) return (R)div_q31((int32_t)s0, (int32_t)n);
    else if constexpr (OP == kStMse) return (R)ssat16((int32_t)((int64_t)s0 / (int64_t)n) >> 13);
    else return (R)cm_sqrt_q15((int16_t)ssat16((int32_t)(((int64_t)s0 / (int64_t)n) >> 15)), kSqrtLutQ15);
  } else {
    if constexpr (OP == kStMean) return (R)div_q31((int32_t)s0, (int32_t)n);
    else return (R)ssat8((int16_t)((uint32_t)s0 / n) >> 5);  // mse_q7: int / uint32_t is an unsigned division
  }
}

// wide: every item of a (and b) starts 16-B aligned and holds a whole number of 16-B packs.  bStride: words between
// the items' second sources (0: one for every item).
template <int OP, typename T, typename R>
__global__ __launch_bounds__(kBlock) void sum_int_kernel(const T* pa, const T* pb, size_t bStride, uint32_t n,
                                                         R* result, uint32_t batch, int lpiLog, bool wide,
                                                         const int32_t* lut) {
  constexpr int V = 16 / sizeof(T);
  constexpr bool kTwoSrc = kTwoSources<OP>;
  constexpr bool kLut = kIsQ31<T> && (OP == kStRms || OP == kStStd);
  struct alignas(16) Pack { T v[V]; };
  __shared__ uint64_t part[kBlock / 64][2];
  __shared__ int32_t slut[32];
  if constexpr (kLut) {
    if (threadIdx.x < 32) slut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
  }
  const uint32_t lpi = 1u << lpiLog, ipw = kBlock >> lpiLog;
  const uint32_t li = threadIdx.x >> lpiLog, l = threadIdx.x & (lpi - 1);
  const uint32_t item = blockIdx.x * ipw + li;
  const bool live = item < batch;
  const T* a = pa + (size_t)(live ? item : 0) * n;
  const T* b = kTwoSrc ? pb + (size_t)(live ? item : 0) * bStride : a;
  uint64_t s0 = 0, s1 = 0;
  if (live) {
    if (wide) {
      for (uint64_t c = l; c < n / V; c += lpi) {          // 64-bit: c + lpi may pass 2^32
        const Pack x = ((const Pack*)a)[c];
        Pack y = x;
        if constexpr (kTwoSrc) y = ((const Pack*)b)[c];
        sum_take_pack<OP, T, V>(s0, s1, x.v, y.v);
      }
    } else {
      for (uint64_t k = l; k < n; k += lpi) sum_take<OP, T>(s0, s1, a[k], b[k]);
    }
  }
  const int waveLanes = lpiLog < 6 ? lpiLog : 6;
  for (int m = 1; m < (1 << waveLanes); m <<= 1) {
    s0 += (uint64_t)__shfl_xor((long long)s0, m, 64);
    if constexpr (kIsVar<OP>) s1 += (uint64_t)__shfl_xor((long long)s1, m, 64);
  }
  if (lpiLog > 6) {            // the whole workgroup on one item
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = s0; part[threadIdx.x >> 6][1] = s1; }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < kBlock / 64; ++w) { s0 += part[w][0]; s1 += part[w][1]; }
  }
  if (live && l == 0) result[item] = sum_finish<OP, T, R>(s0, s1, n, slut);
}

// ---- f32 chains ----------------------------------------------------------------------------------------------
// The term of the chain's first (or only) pass.  y: the second source's element (mse).
template <int OP>
__device__ __forceinline__ float chain_term(float x, float y) {
  if constexpr (OP == kStPower || OP == kStRms) {
    return x * x;
  } else if constexpr (OP == kStMse) {
    const float d = x - y;
    return d * d;
  } else if constexpr (OP == kStDot || OP == kStWavg) {
    return x * y;
  } else {
    return x;                                               // mean, accumulate, the mean pass of var / std
  }
}

// sum: the last pass's chain; n > 1 for var / std.
template <int OP>
__device__ __forceinline__ float chain_finish(float sum, uint32_t n) {
  if constexpr (OP == kStMean || OP == kStMse) return sum / (float)n;
  else if constexpr (OP == kStRms) return sqrt_or_zero(sum / (float)n);
  else if constexpr (OP == kStVar) return sum / (float)((float)n - 1.0f);
  else if constexpr (OP == kStStd) return sqrt_or_zero(sum / (float)((float)n - 1.0f));
  else return sum;                                          // power, accumulate, dot_prod
}

// One wave per item.
template <int OP>
__global__ __launch_bounds__(kBlock) void sum_f32_wave_kernel(const float* pa, const float* pb, size_t bStride,
                                                              uint32_t n, float* result, uint32_t batch) {
  __shared__ float keep[kIsVar<OP> ? kBlock / 64 : 1][kIsVar<OP> ? kVarKeep : 1];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t item = blockIdx.x * (uint32_t)(kBlock / 64) + w;
  if (item >= batch) return;                               // wave-uniform; the kernel has no barrier
  if (kIsVar<OP> && n <= 1u) {
    if (lane == 0) result[item] = 0.0f;
    return;
  }
  const float* a = pa + (size_t)item * n;
  const float* b = kTwoSources<OP> ? pb + (size_t)item * bStride : a;
  const bool kept = kIsVar<OP> && n <= kVarKeep;
  float sum = 0.0f, wsum = 0.0f;                           // wsum: the weights' chain of kStWavg
  for (uint64_t k0 = 0; k0 < n; k0 += 64) {
    const uint32_t cnt = (uint32_t)min((uint64_t)64, n - k0);
    float x = 0.0f, y = 0.0f;
    if (lane < cnt) {
      x = a[k0 + lane];
      if constexpr (kTwoSources<OP>) y = b[k0 + lane];
      if constexpr (kIsVar<OP>)
        if (kept) keep[w][k0 + lane] = x;                  // read back by this lane only
    }
    sum = chain_lanes(sum, chain_term<OP>(x, y), cnt);
    if constexpr (OP == kStWavg) wsum = chain_lanes(wsum, y, cnt);
  }
  if constexpr (OP == kStWavg) {
    if (lane == 0) result[item] = sum / wsum;
    return;
  }
  if constexpr (kIsVar<OP>) {
    const float mean = sum / (float)n;
    sum = 0.0f;
    for (uint64_t k0 = 0; k0 < n; k0 += 64) {
      const uint32_t cnt = (uint32_t)min((uint64_t)64, n - k0);
      float x = 0.0f;
      if (lane < cnt) x = kept ? keep[w][k0 + lane] : a[k0 + lane];
      const float d = x - mean;
      sum = chain_lanes(sum, d * d, cnt);
    }
  }
  if (lane == 0) result[item] = chain_finish<OP>(sum, n);
}

// One lane per item.  LDS rows of kSumChunk + 1 words: a lane walks its own row, 17 words from its neighbour's.
template <int OP>
__global__ __launch_bounds__(kBlock) void sum_f32_lane_kernel(const float* pa, const float* pb, size_t bStride,
                                                              uint32_t n, float* result, uint32_t batch) {
  constexpr int KW = kSumChunk, LD = KW + 1;
  constexpr bool kTwoSrc = kTwoSources<OP>;
  __shared__ float am[kBlock * LD];
  __shared__ float bm[kTwoSrc ? kBlock * LD : 1];
  const uint32_t item0 = blockIdx.x * (uint32_t)kBlock, item = item0 + threadIdx.x;
  const float* arow = am + threadIdx.x * LD;
  const float* brow = kTwoSrc ? bm + threadIdx.x * LD : arow;
  float sum = 0.0f, mean = 0.0f, wsum = 0.0f;              // wsum: the weights' chain of kStWavg
#pragma unroll
  for (int pass = 0; pass < (kIsVar<OP> ? 2 : 1); ++pass) {
    float acc = 0.0f;
    for (uint64_t k0 = 0; k0 < n; k0 += KW) {
      const uint32_t kc = (uint32_t)min((uint64_t)KW, n - k0);
      for (uint32_t idx = threadIdx.x; idx < (uint32_t)kBlock * KW; idx += kBlock) {
        const uint32_t r = idx / KW, wd = idx % KW, it = item0 + r;
        if (wd < kc && it < batch) {
          am[r * LD + wd] = pa[(size_t)it * n + k0 + wd];
          if constexpr (kTwoSrc) bm[r * LD + wd] = pb[(size_t)it * bStride + k0 + wd];
        }
      }
      __syncthreads();
      if (item < batch) {
        for (uint32_t k = 0; k < kc; ++k) {
          float t;
          if (pass == 0) {
            t = chain_term<OP>(arow[k], brow[k]);
          } else {
            const float d = arow[k] - mean;
            t = d * d;
          }
          acc = acc + t;
          if constexpr (OP == kStWavg) wsum = wsum + brow[k];
        }
      }
      __syncthreads();
    }
    if (kIsVar<OP> && pass == 0) mean = acc / (float)n;
    sum = acc;
  }
  if constexpr (OP == kStWavg) {
    if (item < batch) result[item] = sum / wsum;
    return;
  }
  if (item < batch) result[item] = (kIsVar<OP> && n <= 1u) ? 0.0f : chain_finish<OP>(sum, n);
}

template <typename T> struct PowerResult { using type = T; };
template <> struct PowerResult<int32_t> { using type = int64_t; };
template <> struct PowerResult<int16_t> { using type = int64_t; };
template <> struct PowerResult<int8_t> { using type = int32_t; };

// The (operation, type, result type) triples the reference has (dot_prod's result types are power's).
template <int OP, typename T, typename R>
constexpr bool stat_sum_exists() {
  constexpr bool f32 = std::is_same<T, float>::value, q7 = std::is_same<T, int8_t>::value;
  if (OP == kStPower || OP == kStDot) return std::is_same<R, typename PowerResult<T>::type>::value;
  if (!std::is_same<R, T>::value) return false;
  if (OP == kStAccumulate || OP == kStWavg) return f32;
  if (OP == kStRms || OP == kStVar || OP == kStStd) return !q7;
  return OP == kStMean || OP == kStMse;
}

template <int OP, typename T, typename R>
hipError_t sum_run(const T* a, const T* b, size_t bStride, uint32_t n, R* result, uint32_t batch, const int32_t* lut,
                   hipStream_t st) {
  if constexpr (!stat_sum_exists<OP, T, R>()) {
    return hipErrorInvalidValue;
  } else if constexpr (std::is_same<T, float>::value) {
    if (batch >= kSumLaneMinBatch) {
      const dim3 grid((batch + kBlock - 1) / kBlock);
      hipLaunchKernelGGL((sum_f32_lane_kernel<OP>), grid, dim3(kBlock), 0, st, a, b, bStride, n, result, batch);
    } else {
      const dim3 grid((batch + kBlock / 64 - 1) / (kBlock / 64));
      hipLaunchKernelGGL((sum_f32_wave_kernel<OP>), grid, dim3(kBlock), 0, st, a, b, bStride, n, result, batch);
    }
    return hipGetLastError();
  } else {
    constexpr uint32_t V = 16 / sizeof(T);
    const bool wide = (((uintptr_t)a | (uintptr_t)(kTwoSources<OP> ? b : a) | ((size_t)n * sizeof(T)) |
                        (kTwoSources<OP> ? bStride * sizeof(T) : 0)) & 15) == 0;
    const int lpiLog = red_lpi_log(wide ? n / V : n);
    const uint32_t ipw = kBlock >> lpiLog;
    const uint64_t grid = ((uint64_t)batch + ipw - 1) / ipw;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((sum_int_kernel<OP, T, R>), dim3((uint32_t)grid), dim3(kBlock), 0, st, a, b, bStride, n, result,
                       batch, lpiLog, wide, lut);
    return hipGetLastError();
  }
}

}  // namespace

template <typename T, typename R>
hipError_t stat_sum_launch(int op, const T* a, const T* b, uint32_t n, R* result, uint32_t batch, const int32_t* lut,
                           hipStream_t st) {
  if (batch == 0) return hipSuccess;
  switch (op) {
    case kStMean: return sum_run<kStMean, T, R>(a, b, n, n, result, batch, lut, st);
    case kStPower: return sum_run<kStPower, T, R>(a, b, n, n, result, batch, lut, st);
    case kStRms: return sum_run<kStRms, T, R>(a, b, n, n, result, batch, lut, st);
    case kStVar: return sum_run<kStVar, T, R>(a, b, n, n, result, batch, lut, st);
    case kStStd: return sum_run<kStStd, T, R>(a, b, n, n, result, batch, lut, st);
    case kStMse: return sum_run<kStMse, T, R>(a, b, n, n, result, batch, lut, st);
    case kStAccumulate: return sum_run<kStAccumulate, T, R>(a, b, n, n, result, batch, lut, st);
  }
  return hipErrorInvalidValue;
}
#define MI355X_STAT_SUM(T, R)                                                                              \
  template hipError_t stat_sum_launch<T, R>(int, const T*, const T*, uint32_t, R*, uint32_t, const int32_t*, \
                                            hipStream_t);
MI355X_STAT_SUM(float, float)
MI355X_STAT_SUM(int32_t, int32_t)
MI355X_STAT_SUM(int32_t, int64_t)
MI355X_STAT_SUM(int16_t, int16_t)
MI355X_STAT_SUM(int16_t, int64_t)
MI355X_STAT_SUM(int8_t, int8_t)
MI355X_STAT_SUM(int8_t, int32_t)
#undef MI355X_STAT_SUM

template <typename T, typename R>
hipError_t dot_prod_launch(const T* a, const T* b, size_t bStride, uint32_t n, R* result, uint32_t batch,
                           hipStream_t st) {
  if (batch == 0) return hipSuccess;
  return sum_run<kStDot, T, R>(a, b, bStride, n, result, batch, nullptr, st);
}
template hipError_t dot_prod_launch<float, float>(const float*, const float*, size_t, uint32_t, float*, uint32_t,
                                                  hipStream_t);
template hipError_t dot_prod_launch<int32_t, int64_t>(const int32_t*, const int32_t*, size_t, uint32_t, int64_t*,
                                                      uint32_t, hipStream_t);
template hipError_t dot_prod_launch<int16_t, int64_t>(const int16_t*, const int16_t*, size_t, uint32_t, int64_t*,
                                                      uint32_t, hipStream_t);
template hipError_t dot_prod_launch<int8_t, int32_t>(const int8_t*, const int8_t*, size_t, uint32_t, int32_t*,
                                                     uint32_t, hipStream_t);

hipError_t weighted_average_launch(const float* a, const float* w, size_t wStride, uint32_t n, float* result,
                                   uint32_t batch, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  return sum_run<kStWavg, float, float>(a, w, wStride, n, result, batch, nullptr, st);
}

template <typename T>
hipError_t stat_search_launch(bool max, bool abs, const T* src, uint32_t n, T* result, uint32_t* index, uint32_t batch,
                              hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if constexpr (std::is_same<T, float>::value) {
    if (!abs && !index)
      return max ? search_run<true, T, MapNone, true>(src, n, result, index, batch, st)
                 : search_run<false, T, MapNone, true>(src, n, result, index, batch, st);
  }
  if (n == 0) return hipErrorInvalidValue;                  // the reference reads pSrc[0]
  if (abs)
    return max ? search_run<true, T, MapAbs, false>(src, n, result, index, batch, st)
               : search_run<false, T, MapAbs, false>(src, n, result, index, batch, st);
  return max ? search_run<true, T, MapNone, false>(src, n, result, index, batch, st)
             : search_run<false, T, MapNone, false>(src, n, result, index, batch, st);
}
template hipError_t stat_search_launch<float>(bool, bool, const float*, uint32_t, float*, uint32_t*, uint32_t,
                                              hipStream_t);
template hipError_t stat_search_launch<int32_t>(bool, bool, const int32_t*, uint32_t, int32_t*, uint32_t*, uint32_t,
                                                hipStream_t);
template hipError_t stat_search_launch<int16_t>(bool, bool, const int16_t*, uint32_t, int16_t*, uint32_t*, uint32_t,
                                                hipStream_t);
template hipError_t stat_search_launch<int8_t>(bool, bool, const int8_t*, uint32_t, int8_t*, uint32_t*, uint32_t,
                                               hipStream_t);

int16_t sqrt_q15_host(int16_t in) { return cm_sqrt_q15(in, kSqrtLutQ15); }

}  // namespace mi355x
