// arm_cmplx_{mag,mag_squared,conj,mult_cmplx,mult_real,dot_prod}_{f32,q31,q15} and arm_{max,min}_{f32,q31,q15,q7}
// over a batch of contiguous items, bit-exact with the reference's scalar branches
// (Source/ComplexMathFunctions/arm_cmplx_*.c, Source/StatisticsFunctions/arm_max_*.c, arm_min_*.c: the final
// #else of ARM_MATH_MVE* / ARM_MATH_NEON, no ARM_MATH_DSP; FastMathFunctions/arm_sqrt_q31.c).
//
//   element-wise   one streaming kernel over the batch's complex samples as one flat array, templated on the
//                  operation and the type.  A lane's unit is the samples behind 16 bytes of its narrowest stream
//                  (conj / mult_cmplx: 16 B in, 16 B out; mag / mag_squared: 32 B in, 16 B out; mult_real: 32 B +
//                  16 B in, 32 B out), moved with 16-B loads and stores when every pointer is 16-B aligned,
//                  kCmUnroll units in flight per lane; one sample per lane otherwise and for the ragged end.  A
//                  lane reads its samples before it writes them, so dst may be a source exactly where both have
//                  the same words per sample (conj, mult_cmplx, mult_real).  The q31 / q15 magnitudes read
//                  sqrt_initial_lut_q31 from LDS (32 words staged per workgroup): no lane shuffle, so the ragged
//                  loops may diverge.  arm_cmplx_mag_fast_q15 is one more operation of this kernel: arm_sqrt_q15 of
//                  (re*re + im*im) >> 17, its 16 start words in the same LDS array.
//   integer dot    (mapping and search kernel: reduce_lanes.hpp, shared with statistics.hip)
//   max / min      lanes-per-item = the power of two that leaves a lane about two loads of its item (1 .. 64, or
//                  the whole workgroup); short items are packed kBlock / lanes-per-item to a workgroup.  16-B
//                  loads when every item starts 16-B aligned, one element per load otherwise.  The lanes' partial
//                  results meet in a butterfly of lane shuffles (and four LDS words for a whole workgroup).
//                  Integer sums are associative.  max / min combine (value, index) pairs: the better value wins,
//                  equal values keep the lower index, a NaN never enters a pair; item word 0 is stored as it is
//                  when it is a NaN (the reference's `out` starts there and no comparison with it is true).
//   dot_prod_f32   re = (re + a*c) - b*d, im = (im + a*d) + b*c is an ordered chain per item.  From
//                  kDotLaneMinBatch items on: one lane per item, the workgroup staging kDotChunk samples of its
//                  256 items in LDS with coalesced row-segment loads (B once when shared).  Below: one wave per
//                  item; the wave loads 64 samples, every lane forms its sample's four products, and the chain
//                  takes them in order through v_readlane (two dependent adds per sample and chain).
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"
#include "mfcc_fixed_ops.hpp"
#include "reduce_lanes.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

// ---- element-wise ------------------------------------------------------------------------------------------
// One complex sample: a = (a[0], a[1]); b the second operand's sample (mult_cmplx: 2 words, mult_real: 1 word).
template <int OP, typename T>
__device__ __forceinline__ void cm_sample(const T* a, const T* b, T* d, const int32_t* lut) {
  if constexpr (std::is_same<T, float>::value) {
    if constexpr (OP == kCmMag) {
      const float s = a[0] * a[0] + a[1] * a[1];
      d[0] = s >= 0.0f ? sqrtf(s) : 0.0f;                   // arm_sqrt_f32: a NaN sum gives +0.0
    } else if constexpr (OP == kCmMagSquared) {
      d[0] = a[0] * a[0] + a[1] * a[1];
    } else if constexpr (OP == kCmConj) {
      d[0] = a[0];
      d[1] = -a[1];
    } else if constexpr (OP == kCmMultCmplx) {
      const float re = (a[0] * b[0]) - (a[1] * b[1]), im = (a[0] * b[1]) + (a[1] * b[0]);
      d[0] = re;
      d[1] = im;
    } else {
      const float re = a[0] * b[0], im = a[1] * b[0];
      d[0] = re;
      d[1] = im;
    }
  } else if constexpr (std::is_same<T, int32_t>::value) {
    if constexpr (OP == kCmMag || OP == kCmMagSquared) {
      const int32_t s = (int32_t)(((int64_t)a[0] * a[0]) >> 33) + (int32_t)(((int64_t)a[1] * a[1]) >> 33);
      d[0] = OP == kCmMag ? cm_sqrt_q31(s, lut) : s;
    } else if constexpr (OP == kCmConj) {
      d[0] = a[0];
      d[1] = a[1] == INT32_MIN ? INT32_MAX : -a[1];
    } else if constexpr (OP == kCmMultCmplx) {
      const int32_t ac = (int32_t)(((int64_t)a[0] * b[0]) >> 33), bd = (int32_t)(((int64_t)a[1] * b[1]) >> 33);
      const int32_t ad = (int32_t)(((int64_t)a[0] * b[1]) >> 33), bc = (int32_t)(((int64_t)a[1] * b[0]) >> 33);
      d[0] = wsub(ac, bd);
      d[1] = wadd(ad, bc);
    } else {                                                // clip_q63_to_q31(((q63_t)x * r) >> 31)
      const int64_t re = ((int64_t)a[0] * b[0]) >> 31, im = ((int64_t)a[1] * b[0]) >> 31;
      d[0] = re > INT32_MAX ? INT32_MAX : (int32_t)re;      // only min * min leaves the range, upwards
      d[1] = im > INT32_MAX ? INT32_MAX : (int32_t)im;
    }
  } else {
    const int32_t x = a[0], y = a[1];
    if constexpr (OP == kCmMag) {
      const uint32_t s = ((uint32_t)(x * x) + (uint32_t)(y * y)) >> 1;
      d[0] = (T)(cm_sqrt_q31((int32_t)s, lut) >> 16);
    } else if constexpr (OP == kCmMagFast) {               // arm_cmplx_mag_fast_q15: lut holds arm_sqrt_q15's table
      d[0] = (T)cm_sqrt_q15((int16_t)(((int64_t)(x * x) + (int64_t)(y * y)) >> 17), lut);
    } else if constexpr (OP == kCmMagSquared) {
      d[0] = (T)(((int64_t)(x * x) + (int64_t)(y * y)) >> 17);
    } else if constexpr (OP == kCmConj) {
      d[0] = a[0];
      d[1] = (T)(y == -32768 ? 32767 : -y);
    } else if constexpr (OP == kCmMultCmplx) {
      const int32_t c = b[0], e = b[1];
      const T re = (T)(((x * c) >> 17) - ((y * e) >> 17)), im = (T)(((x * e) >> 17) + ((y * c) >> 17));
      d[0] = re;
      d[1] = im;
    } else {
      const int32_t r = b[0];
      const T re = (T)ssat16((x * r) >> 15), im = (T)ssat16((y * r) >> 15);
      d[0] = re;
      d[1] = im;
    }
  }
}

constexpr int kCmUnroll = 4;   // units per lane and tile

// Words of a, b and d per complex sample.
template <int OP> struct CmShape {
  static constexpr int WA = 2;
  static constexpr int WB = OP == kCmMultCmplx ? 2 : OP == kCmMultReal ? 1 : 0;
  static constexpr int WD = (OP == kCmMag || OP == kCmMagSquared || OP == kCmMagFast) ? 1 : 2;
};

// count: complex samples of the whole batch.  vec: a, b and d are 16-B aligned.
template <int OP, typename T>
__global__ __launch_bounds__(kBlock) void cmplx_ew_kernel(const T* a, const T* b, T* d, size_t count, bool vec,
                                                          const int32_t* lut) {
  using S = CmShape<OP>;
  constexpr int V = 16 / sizeof(T), U = kCmUnroll;
  // samples per unit: 16 bytes of the narrowest stream
  constexpr int SU = V / (S::WD == 1 || S::WB == 1 ? 1 : 2);
  constexpr int PA = SU * S::WA / V, PB = S::WB ? (SU * S::WB / V) : 0, PD = SU * S::WD / V;
  struct alignas(16) Pack { T v[V]; };
  constexpr bool kLut = OP == kCmMag && !std::is_same<T, float>::value;
  __shared__ int32_t slut[32];
  if constexpr (kLut) {
    if (threadIdx.x < 32) slut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
  }
  if constexpr (OP == kCmMagFast) {
    if (threadIdx.x < 16) slut[threadIdx.x] = kSqrtLutQ15[threadIdx.x];
    __syncthreads();
  }
  const size_t units = vec ? count / SU : 0;
  for (size_t tile = blockIdx.x; tile * (U * kBlock) < units; tile += gridDim.x) {
    const size_t i0 = tile * (U * kBlock) + threadIdx.x;
    T x[U][SU * S::WA], y[U][S::WB ? SU * S::WB : 1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * kBlock;
      if (i < units) {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
          const Pack k = ((const Pack*)a)[i * PA + p];
#pragma unroll
          for (int j = 0; j < V; ++j) x[u][p * V + j] = k.v[j];
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) {
          const Pack k = ((const Pack*)b)[i * PB + p];
#pragma unroll
          for (int j = 0; j < V; ++j) y[u][p * V + j] = k.v[j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * kBlock;
      if (i < units) {
        T r[SU * S::WD];
#pragma unroll
        for (int s = 0; s < SU; ++s) cm_sample<OP, T>(x[u] + s * S::WA, y[u] + s * S::WB, r + s * S::WD, slut);
#pragma unroll
        for (int p = 0; p < PD; ++p) {
          Pack k;
#pragma unroll
          for (int j = 0; j < V; ++j) k.v[j] = r[p * V + j];
          ((Pack*)d)[i * PD + p] = k;
        }
      }
    }
  }
  // the ragged end, or everything when a pointer is not 16-B aligned: one sample per lane
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = units * SU + (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
    T xa[2] = {a[2 * i], a[2 * i + 1]}, xb[2] = {}, r[2];
    if constexpr (S::WB == 2) { xb[0] = b[2 * i]; xb[1] = b[2 * i + 1]; }
    if constexpr (S::WB == 1) xb[0] = b[i];
    cm_sample<OP, T>(xa, xb, r, slut);
    if constexpr (S::WD == 2) { d[2 * i] = r[0]; d[2 * i + 1] = r[1]; }
    else d[i] = r[0];
  }
}

template <int OP, typename T>
hipError_t ew_launch(const T* a, const T* b, T* d, size_t count, const int32_t* lut, hipStream_t st) {
  using S = CmShape<OP>;
  const bool vec = (((uintptr_t)a | (uintptr_t)(S::WB ? b : a) | (uintptr_t)d) & 15) == 0;
  constexpr size_t V = 16 / sizeof(T), SU = V / (S::WD == 1 || S::WB == 1 ? 1 : 2);
  const size_t per = vec ? SU * kCmUnroll * kBlock : kBlock;     // samples a workgroup takes per step
  const size_t blocks = (count + per - 1) / per;
  const size_t cap = 0x7fffffff;
  const uint32_t grid = (uint32_t)(blocks < cap ? blocks : cap);
  hipLaunchKernelGGL((cmplx_ew_kernel<OP, T>), dim3(grid), dim3(kBlock), 0, st, a, b, d, count, vec, lut);
  return hipGetLastError();
}

// ---- lanes-per-item reductions: the integer dot products, max / min --------------------------------------
// The mapping (red_lpi_log) and the search kernel: reduce_lanes.hpp.

// Integer complex dot product of one sample into (re, im).  q31: each product >> 14, sums mod 2^64; q15: exact.
template <typename T>
__device__ __forceinline__ void dot_take(int64_t& re, int64_t& im, T a, T b, T c, T d) {
  if constexpr (std::is_same<T, int32_t>::value) {
    const uint64_t ac = (uint64_t)(((int64_t)a * c) >> 14), bd = (uint64_t)(((int64_t)b * d) >> 14);
    const uint64_t ad = (uint64_t)(((int64_t)a * d) >> 14), bc = (uint64_t)(((int64_t)b * c) >> 14);
    re = (int64_t)((uint64_t)re + ac - bd);
    im = (int64_t)((uint64_t)im + ad + bc);
  } else {
    re += (int64_t)((int32_t)a * c) - (int64_t)((int32_t)b * d);
    im += (int64_t)((int32_t)a * d) + (int64_t)((int32_t)b * c);
  }
}

// n: complex samples per item; bStride: complex samples between the items' B vectors (0: one shared B).
template <typename T, typename R>
__global__ __launch_bounds__(kBlock) void dot_int_kernel(const T* pa, const T* pb, size_t bStride, uint32_t n,
                                                         R* outRe, R* outIm, uint32_t batch, int lpiLog, bool wide) {
  constexpr int V = 16 / sizeof(T);
  struct alignas(16) Pack { T v[V]; };
  __shared__ int64_t part[kBlock / 64][2];
  const uint32_t lpi = 1u << lpiLog, ipw = kBlock >> lpiLog;
  const uint32_t li = threadIdx.x >> lpiLog, l = threadIdx.x & (lpi - 1);
  const uint32_t item = blockIdx.x * ipw + li;
  const bool live = item < batch;
  const T* a = pa + (size_t)(live ? item : 0) * 2 * n;
  const T* b = pb + (size_t)(live ? item : 0) * 2 * bStride;
  int64_t re = 0, im = 0;
  if (live) {
    if (wide) {
      const uint64_t packs = ((uint64_t)2 * n) / V;
      for (uint64_t c = l; c < packs; c += lpi) {
        const Pack x = ((const Pack*)a)[c], y = ((const Pack*)b)[c];
#pragma unroll
        for (int j = 0; j < V; j += 2) dot_take<T>(re, im, x.v[j], x.v[j + 1], y.v[j], y.v[j + 1]);
      }
    } else {
      for (uint64_t k = l; k < n; k += lpi) dot_take<T>(re, im, a[2 * k], a[2 * k + 1], b[2 * k], b[2 * k + 1]);
    }
  }
  const int waveLanes = lpiLog < 6 ? lpiLog : 6;
  for (int m = 1; m < (1 << waveLanes); m <<= 1) {
    re = (int64_t)((uint64_t)re + (uint64_t)__shfl_xor((long long)re, m, 64));
    im = (int64_t)((uint64_t)im + (uint64_t)__shfl_xor((long long)im, m, 64));
  }
  if (lpiLog > 6) {
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = re; part[threadIdx.x >> 6][1] = im; }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < kBlock / 64; ++w) {
        re = (int64_t)((uint64_t)re + (uint64_t)part[w][0]);
        im = (int64_t)((uint64_t)im + (uint64_t)part[w][1]);
      }
  }
  if (live && l == 0) {
    if constexpr (std::is_same<T, int32_t>::value) { outRe[item] = re; outIm[item] = im; }
    else { outRe[item] = (R)(re >> 6); outIm[item] = (R)(im >> 6); }
  }
}

// ---- dot_prod_f32 ------------------------------------------------------------------------------------------
constexpr int kDotChunk = 8;                     // complex samples per item and LDS stage (a 64-byte row segment)
constexpr uint32_t kDotLaneMinBatch = 4096;      // from here on one lane per item, below one wave per item

// One lane per item.  LDS rows of 2 kDotChunk + 1 words: a lane walks its own row, 17 words from its neighbour's.
template <bool SHARED>
__global__ __launch_bounds__(kBlock) void dot_f32_lane_kernel(const float* pa, const float* pb, size_t bStride,
                                                              uint32_t n, float* outRe, float* outIm,
                                                              uint32_t batch) {
  constexpr int KW = 2 * kDotChunk, LD = KW + 1;
  __shared__ float am[kBlock * LD];
  __shared__ float bm[(SHARED ? 1 : kBlock) * LD];
  const uint32_t item0 = blockIdx.x * (uint32_t)kBlock, item = item0 + threadIdx.x;
  const float* arow = am + threadIdx.x * LD;
  const float* brow = bm + (SHARED ? 0 : threadIdx.x * LD);
  float re = 0.0f, im = 0.0f;
  for (uint64_t k0 = 0; k0 < n; k0 += kDotChunk) {
    const uint32_t kc = (uint32_t)min((uint64_t)kDotChunk, n - k0);
    for (uint32_t idx = threadIdx.x; idx < (uint32_t)kBlock * KW; idx += kBlock) {
      const uint32_t r = idx / KW, w = idx % KW, it = item0 + r;
      if (w < 2 * kc && it < batch) {
        am[r * LD + w] = pa[((size_t)it * n + k0) * 2 + w];
        if constexpr (!SHARED) bm[r * LD + w] = pb[((size_t)it * bStride + k0) * 2 + w];
      }
    }
    if constexpr (SHARED)
      if (threadIdx.x < 2 * kc) bm[threadIdx.x] = pb[(size_t)k0 * 2 + threadIdx.x];
    __syncthreads();
    if (item < batch) {
      for (uint32_t k = 0; k < kc; ++k) {
        const float a = arow[2 * k], b = arow[2 * k + 1], c = brow[2 * k], d = brow[2 * k + 1];
        re = (re + a * c) - b * d;
        im = (im + a * d) + b * c;
      }
    }
    __syncthreads();
  }
  if (item < batch) {
    outRe[item] = re;
    outIm[item] = im;
  }
}

// One wave per item: lane j of a step holds sample k0 + j's products, the chain reads them lane by lane.
__global__ __launch_bounds__(kBlock) void dot_f32_wave_kernel(const float* pa, const float* pb, size_t bStride,
                                                              uint32_t n, float* outRe, float* outIm,
                                                              uint32_t batch) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t item = blockIdx.x * (uint32_t)(kBlock / 64) + (threadIdx.x >> 6);
  if (item >= batch) return;                               // wave-uniform
  struct alignas(4) Cf { float x, y; };                   // a complex sample is only 4-byte aligned
  const Cf* a = (const Cf*)pa + (size_t)item * n;
  const Cf* b = (const Cf*)pb + (size_t)item * bStride;
  float re = 0.0f, im = 0.0f;
  for (uint64_t k0 = 0; k0 < n; k0 += 64) {
    const uint32_t cnt = (uint32_t)min((uint64_t)64, n - k0);
    Cf x{0.0f, 0.0f}, y = x;
    if (lane < cnt) { x = a[(size_t)k0 + lane]; y = b[(size_t)k0 + lane]; }
    const float ac = x.x * y.x, bd = x.y * y.y, ad = x.x * y.y, bc = x.y * y.x;
    if (cnt == 64) {
#pragma unroll
      for (int j = 0; j < 64; ++j) {
        re = (re + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ac), j))) -
             __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bd), j));
        im = (im + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ad), j))) +
             __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bc), j));
      }
    } else {
      for (uint32_t j = 0; j < cnt; ++j) {                 // uniform trip count
        re = (re + __shfl(ac, (int)j, 64)) - __shfl(bd, (int)j, 64);
        im = (im + __shfl(ad, (int)j, 64)) + __shfl(bc, (int)j, 64);
      }
    }
  }
  if (lane == 0) {
    outRe[item] = re;
    outIm[item] = im;
  }
}

}  // namespace

template <typename T>
hipError_t cmplx_ew_launch(int op, const T* a, const T* b, T* d, size_t count, const int32_t* lut, hipStream_t st) {
  if (count == 0) return hipSuccess;
  switch (op) {
    case kCmMag: return ew_launch<kCmMag, T>(a, b, d, count, lut, st);
    case kCmMagSquared: return ew_launch<kCmMagSquared, T>(a, b, d, count, lut, st);
    case kCmConj: return ew_launch<kCmConj, T>(a, b, d, count, lut, st);
    case kCmMultCmplx: return ew_launch<kCmMultCmplx, T>(a, b, d, count, lut, st);
    case kCmMultReal: return ew_launch<kCmMultReal, T>(a, b, d, count, lut, st);
    case kCmMagFast:
      if constexpr (std::is_same<T, int16_t>::value) return ew_launch<kCmMagFast, T>(a, b, d, count, lut, st);
      break;
  }
  return hipErrorInvalidValue;
}
template hipError_t cmplx_ew_launch<float>(int, const float*, const float*, float*, size_t, const int32_t*,
                                           hipStream_t);
template hipError_t cmplx_ew_launch<int32_t>(int, const int32_t*, const int32_t*, int32_t*, size_t, const int32_t*,
                                             hipStream_t);
template hipError_t cmplx_ew_launch<int16_t>(int, const int16_t*, const int16_t*, int16_t*, size_t, const int32_t*,
                                             hipStream_t);

template <typename T>
hipError_t search_launch(bool max, const T* src, uint32_t n, T* result, uint32_t* index, uint32_t batch,
                         hipStream_t st) {
  if (n == 0 || batch == 0) return hipSuccess;
  return max ? search_run<true, T, MapNone, false>(src, n, result, index, batch, st)
             : search_run<false, T, MapNone, false>(src, n, result, index, batch, st);
}
template hipError_t search_launch<float>(bool, const float*, uint32_t, float*, uint32_t*, uint32_t, hipStream_t);
template hipError_t search_launch<int32_t>(bool, const int32_t*, uint32_t, int32_t*, uint32_t*, uint32_t, hipStream_t);
template hipError_t search_launch<int16_t>(bool, const int16_t*, uint32_t, int16_t*, uint32_t*, uint32_t, hipStream_t);
template hipError_t search_launch<int8_t>(bool, const int8_t*, uint32_t, int8_t*, uint32_t*, uint32_t, hipStream_t);

template <typename T, typename R>
hipError_t cmplx_dot_launch(const T* a, const T* b, size_t bStride, uint32_t n, R* re, R* im, uint32_t batch,
                            hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if constexpr (std::is_same<T, float>::value) {
    if (batch >= kDotLaneMinBatch) {
      const dim3 grid((batch + kBlock - 1) / kBlock);
      if (bStride == 0)
        hipLaunchKernelGGL((dot_f32_lane_kernel<true>), grid, dim3(kBlock), 0, st, a, b, bStride, n, re, im, batch);
      else
        hipLaunchKernelGGL((dot_f32_lane_kernel<false>), grid, dim3(kBlock), 0, st, a, b, bStride, n, re, im, batch);
    } else {
      const dim3 grid((batch + kBlock / 64 - 1) / (kBlock / 64));
      hipLaunchKernelGGL(dot_f32_wave_kernel, grid, dim3(kBlock), 0, st, a, b, bStride, n, re, im, batch);
    }
  } else {
    constexpr uint32_t V = 16 / sizeof(T);
    const bool wide = (((uintptr_t)a | (uintptr_t)b | ((size_t)n * 2 * sizeof(T)) | (bStride * 2 * sizeof(T))) & 15) == 0;
    const int lpiLog = red_lpi_log(wide ? ((uint64_t)2 * n) / V : n);
    const uint32_t ipw = kBlock >> lpiLog;
    const uint64_t grid = ((uint64_t)batch + ipw - 1) / ipw;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((dot_int_kernel<T, R>), dim3((uint32_t)grid), dim3(kBlock), 0, st, a, b, bStride, n, re, im,
                       batch, lpiLog, wide);
  }
  return hipGetLastError();
}
template hipError_t cmplx_dot_launch<float, float>(const float*, const float*, size_t, uint32_t, float*, float*,
                                                   uint32_t, hipStream_t);
template hipError_t cmplx_dot_launch<int32_t, int64_t>(const int32_t*, const int32_t*, size_t, uint32_t, int64_t*,
                                                       int64_t*, uint32_t, hipStream_t);
template hipError_t cmplx_dot_launch<int16_t, int32_t>(const int16_t*, const int16_t*, size_t, uint32_t, int32_t*,
                                                       int32_t*, uint32_t, hipStream_t);

}  // namespace mi355x
