// arm_{braycurtis,canberra,chebyshev,cityblock,correlation,cosine,euclidean,jensenshannon}_distance_f32, the nine
// boolean distances on packed uint32_t words, and arm_dtw_{init_window_q7,distance_f32,path_f32}, over a batch of
// items, bit-exact with the reference's scalar branches (Source/DistanceFunctions/arm_*.c: the final #else, with
// ARM_MATH_LOOPUNROLL and no FMA contraction).  arm_minkowski_distance_f32 rests on the host libm's powf and is left
// out, as arm_entropy_f32 and the other libm-bound statistics are.
//
//   f32 distances   Every sum is an ordered chain from 0.0f in element order, the term rounded before its add; the
//                   two mappings are those of the chain kernels of statistics.hip (chain_f32.hpp): one wave per item
//                   below kSumLaneMinBatch items (each lane forms its element's terms, however costly: a division for
//                   canberra, two host_logf for jensenshannon; only the adds are serial), one lane per item from
//                   there on, staging kSumChunk words of both sources in LDS.  braycurtis and jensenshannon carry two
//                   chains, cosine and correlation three, side by side in the same pass, so their add latencies
//                   overlap.  correlation runs the two means' chains first and then the power / dot chains of the
//                   shifted words x + (-mean): the wave form keeps both items in LDS between the passes up to
//                   kVarKeep words each and reads longer ones again; the lane form always reads them again.  The
//                   drop-in's wave form also stores the shifted words back, as the reference does.  canberra's
//                   skipped element (both words compare equal to zero) adds -0.0f in the wave form, which leaves
//                   every sum as it is.  chebyshev is no chain: max over |a - b| on strict >, which is associative
//                   once element 0's NaN is set aside (a NaN at element 0 is the result, a NaN elsewhere never wins).
//   boolean         One kernel counts TT, TF and FT of an item with population counts of a & b, a & ~b, ~a & b, in
//                   the lanes-per-item mapping of reduce_lanes.hpp (16-B packs where every item is aligned); of the
//                   last, partial word only the top numberOfBools % 32 bits count, and no word past
//                   ceil(numberOfBools / 32) is read.  FF = numberOfBools - TT - TF - FT.  One lane per item then
//                   evaluates the function's epilogue exactly as its C states it: uint32_t sums and products wrap,
//                   a count becomes a float where the C converts it, float additions run left to right.
//   DTW             arm_dtw_distance_f32: one wave per item, lanes over the rows of a 64-row strip, stepping over the
//                   strip's anti-diagonals; a cell's upper and diagonal neighbours come from the lane above (lane 0:
//                   from the previous strip's last row, read back from pDTW in 64-word segments), its left neighbour
//                   is the lane's own previous cell.  Cells outside the window are stored as F32_MAX and their
//                   distance word is never loaded.  MIN is a compare and a select, as the reference's macro.
//                   arm_dtw_path_f32: one lane per item walks back from the last cell.  arm_dtw_init_window_q7:
//                   element-wise.
#include "chain_f32.hpp"
#include "common.hpp"
#include "host_logf.hpp"
#include "kernels.hpp"
#include "reduce_lanes.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

// ---- f32 distances -------------------------------------------------------------------------------------------
template <int OP>
constexpr int kChains = (OP == kDsCosine || OP == kDsCorrelation) ? 3 : (OP == kDsBraycurtis || OP == kDsJensenshannon) ? 2 : 1;

// The terms of one element for the item's chains (correlation: of the shifted words).
template <int OP>
__device__ __forceinline__ void dist_terms(float x, float y, float (&t)[3]) {
  t[1] = 0.0f;
  t[2] = 0.0f;
  if constexpr (OP == kDsBraycurtis) {
    t[0] = fabsf(x - y);
    t[1] = fabsf(x + y);
  } else if constexpr (OP == kDsCanberra) {
    const float diff = fabsf(x - y), sum = fabsf(x) + fabsf(y);
    t[0] = (x != 0.0f || y != 0.0f) ? diff / sum : -0.0f;   // sum + (-0.0f) == sum for every sum
  } else if constexpr (OP == kDsCityblock) {
    t[0] = fabsf(x - y);
  } else if constexpr (OP == kDsEuclidean) {
    const float d = x - y;
    t[0] = d * d;
  } else if constexpr (OP == kDsJensenshannon) {
    const float m = (x + y) / 2.0f;
    t[0] = x * host_logf(x / m);
    t[1] = y * host_logf(y / m);
  } else {                                                  // cosine, correlation: power A, power B, dot
    t[0] = x * x;
    t[1] = y * y;
    t[2] = x * y;
  }
}

template <int OP>
__device__ __forceinline__ float dist_finish(const float (&s)[3], uint32_t n) {
  if constexpr (OP == kDsBraycurtis) {
    return s[0] / s[1];
  } else if constexpr (OP == kDsEuclidean) {
    return sqrt_or_zero(s[0]);
  } else if constexpr (OP == kDsJensenshannon) {
    const float sum = s[0] + s[1];
    return sqrt_or_zero(sum / 2.0f);
  } else if constexpr (OP == kDsCosine) {
    return 1.0f - s[2] / sqrt_or_zero(s[0] * s[1]);
  } else if constexpr (OP == kDsCorrelation) {
    const float dot = s[2] / (float)n, pwra = s[0] / (float)n, pwrb = s[1] / (float)n;
    return 1.0f - dot / sqrt_or_zero(pwra * pwrb);
  } else {
    return s[0];                                            // canberra, cityblock
  }
}

// One wave per item.  wa / wb (correlation, the drop-in): where the shifted words are stored, or null.
template <int OP>
__global__ __launch_bounds__(kBlock) void dist_f32_wave_kernel(const float* pa, const float* pb, size_t bStride,
                                                               uint32_t n, float* result, uint32_t batch, float* wa,
                                                               float* wb) {
  constexpr bool kCorr = OP == kDsCorrelation;
  constexpr int NC = kChains<OP>;
  __shared__ float keep[kCorr ? kBlock / 64 : 1][2][kCorr ? kVarKeep : 1];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t item = blockIdx.x * (uint32_t)(kBlock / 64) + w;
  if (item >= batch) return;                               // wave-uniform; the kernel has no barrier
  const float* a = pa + (size_t)item * n;
  const float* b = pb + (size_t)item * bStride;
  if constexpr (OP == kDsChebyshev) {                       // n > 0
    float m = -1.0f;                                        // below every |a - b|
    for (uint64_t k = lane; k < n; k += 64) {
      const float d = fabsf(a[k] - b[k]);
      if (d > m) m = d;
    }
    for (int x = 1; x < 64; x <<= 1) {
      const float o = __shfl_xor(m, x, 64);
      if (o > m) m = o;
    }
    if (lane == 0) {
      const float d0 = fabsf(a[0] - b[0]);
      result[item] = d0 == d0 ? m : d0;                     // a NaN at element 0 is never replaced
    }
    return;
  } else {
    const bool kept = kCorr && n <= kVarKeep;
    float ma = 0.0f, mb = 0.0f;
    if constexpr (kCorr) {                                  // arm_mean_f32 of both
      float sa = 0.0f, sb = 0.0f;
      for (uint64_t k0 = 0; k0 < n; k0 += 64) {
        const uint32_t cnt = (uint32_t)min((uint64_t)64, n - k0);
        float x = 0.0f, y = 0.0f;
        if (lane < cnt) {
          x = a[k0 + lane];
          y = b[k0 + lane];
          if (kept) { keep[w][0][k0 + lane] = x; keep[w][1][k0 + lane] = y; }   // read back by this lane only
        }
        sa = chain_lanes(sa, x, cnt);
        sb = chain_lanes(sb, y, cnt);
      }
      ma = sa / (float)n;
      mb = sb / (float)n;
    }
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (uint64_t k0 = 0; k0 < n; k0 += 64) {
      const uint32_t cnt = (uint32_t)min((uint64_t)64, n - k0);
      float x = 0.0f, y = 0.0f;
      if (lane < cnt) {
        x = kept ? keep[w][0][k0 + lane] : a[k0 + lane];
        y = kept ? keep[w][1][k0 + lane] : b[k0 + lane];
        if constexpr (kCorr) {                              // arm_offset_f32 by -mean
          x = x + (-ma);
          y = y + (-mb);
          if (wa) { wa[(size_t)item * n + k0 + lane] = x; wb[(size_t)item * bStride + k0 + lane] = y; }
        }
      }
      float t[3];
      dist_terms<OP>(x, y, t);
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = chain_lanes(s[c], t[c], cnt);
    }
    if (lane == 0) result[item] = dist_finish<OP>(s, n);
  }
}

// One lane per item; the LDS rows of sum_f32_lane_kernel (statistics.hip) for both sources.
template <int OP>
__global__ __launch_bounds__(kBlock) void dist_f32_lane_kernel(const float* pa, const float* pb, size_t bStride,
                                                               uint32_t n, float* result, uint32_t batch) {
  constexpr int KW = kSumChunk, LD = KW + 1;
  constexpr bool kCorr = OP == kDsCorrelation;
  __shared__ float am[kBlock * LD];
  __shared__ float bm[kBlock * LD];
  const uint32_t item0 = blockIdx.x * (uint32_t)kBlock, item = item0 + threadIdx.x;
  const float* arow = am + threadIdx.x * LD;
  const float* brow = bm + threadIdx.x * LD;
  float s[3] = {0.0f, 0.0f, 0.0f};
  float ma = 0.0f, mb = 0.0f;
#pragma unroll
  for (int pass = 0; pass < (kCorr ? 2 : 1); ++pass) {
    const bool means = kCorr && pass == 0;
    for (uint64_t k0 = 0; k0 < n; k0 += KW) {
      const uint32_t kc = (uint32_t)min((uint64_t)KW, n - k0);
      for (uint32_t idx = threadIdx.x; idx < (uint32_t)kBlock * KW; idx += kBlock) {
        const uint32_t r = idx / KW, wd = idx % KW, it = item0 + r;
        if (wd < kc && it < batch) {
          am[r * LD + wd] = pa[(size_t)it * n + k0 + wd];
          bm[r * LD + wd] = pb[(size_t)it * bStride + k0 + wd];
        }
      }
      __syncthreads();
      if (item < batch) {
        for (uint32_t k = 0; k < kc; ++k) {
          float x = arow[k], y = brow[k];
          if constexpr (OP == kDsChebyshev) {
            const float d = fabsf(x - y);
            if (k0 == 0 && k == 0) s[0] = d;
            else if (d > s[0]) s[0] = d;
          } else if constexpr (OP == kDsCanberra) {
            if (x != 0.0f || y != 0.0f) s[0] = s[0] + fabsf(x - y) / (fabsf(x) + fabsf(y));
          } else if (means) {
            s[0] = s[0] + x;
            s[1] = s[1] + y;
          } else {
            if constexpr (kCorr) { x = x + (-ma); y = y + (-mb); }
            float t[3];
            dist_terms<OP>(x, y, t);
#pragma unroll
            for (int c = 0; c < kChains<OP>; ++c) s[c] = s[c] + t[c];
          }
        }
      }
      __syncthreads();
    }
    if (means) {
      ma = s[0] / (float)n;
      mb = s[1] / (float)n;
      s[0] = 0.0f;
      s[1] = 0.0f;
    }
  }
  if (item < batch) result[item] = dist_finish<OP>(s, n);
}

template <int OP>
hipError_t dist_f32_run(const float* a, const float* b, size_t bStride, uint32_t n, float* result, uint32_t batch,
                        float* wa, float* wb, hipStream_t st) {
  if (batch >= kSumLaneMinBatch && !wa) {
    const dim3 grid((batch + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((dist_f32_lane_kernel<OP>), grid, dim3(kBlock), 0, st, a, b, bStride, n, result, batch);
  } else {
    const dim3 grid((batch + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL((dist_f32_wave_kernel<OP>), grid, dim3(kBlock), 0, st, a, b, bStride, n, result, batch, wa, wb);
  }
  return hipGetLastError();
}

// ---- boolean distances ---------------------------------------------------------------------------------------
struct BoolCounts {
  uint32_t tt, tf, ft;
};
__device__ __forceinline__ void bool_take(BoolCounts& c, uint32_t a, uint32_t b, uint32_t mask) {
  c.tt += (uint32_t)__popc(a & b & mask);
  c.tf += (uint32_t)__popc(a & ~b & mask);
  c.ft += (uint32_t)__popc(~a & b & mask);
}

// The function's return expression on the item's counts, as its file states it.
__device__ __forceinline__ float bool_finish(int op, uint32_t ctt, uint32_t ctf, uint32_t cft, uint32_t n) {
  const uint32_t cff = n - ctt - ctf - cft;
  switch (op) {
    case kBdDice: return (float)(ctf + cft) / (2.0f * (float)ctt + (float)cft + (float)ctf);
    case kBdHamming: return (float)(ctf + cft) / (float)n;
    case kBdJaccard: return (float)(ctf + cft) / (float)(ctt + cft + ctf);
    case kBdKulsinski: return (float)(ctf + cft - ctt + n) / (float)(cft + ctf + n);
    case kBdRogerstanimoto: {
      const uint32_t r = 2u * (ctf + cft);
      return (float)r / (float)(r + ctt + cff);
    }
    case kBdRussellrao: return (float)(n - ctt) / (float)n;
    case kBdSokalmichener: {
      const float r = 2.0f * (float)(ctf + cft), s = (float)(cff + ctt);
      return r / (s + r);
    }
    case kBdSokalsneath: {
      const float r = 2.0f * (float)(ctf + cft);
      return r / (r + (float)ctt);
    }
    default: {                                              // yule
      const uint32_t r = 2u * (ctf * cft);
      return (float)r / ((float)r / 2.0f + (float)(ctt * cff));
    }
  }
}

// words: ceil(n / 32), the item's length and the stride of pa's items.  wide: every item of a and b starts 16-B
// aligned and holds a whole number of 16-B packs.
__global__ __launch_bounds__(kBlock) void bool_dist_kernel(int op, const uint32_t* pa, const uint32_t* pb,
                                                           size_t bStride, uint32_t n, uint32_t words, float* result,
                                                           uint32_t batch, int lpiLog, bool wide) {
  __shared__ BoolCounts part[kBlock / 64];
  const uint32_t lpi = 1u << lpiLog, ipw = kBlock >> lpiLog;
  const uint32_t li = threadIdx.x >> lpiLog, l = threadIdx.x & (lpi - 1);
  const uint32_t item = blockIdx.x * ipw + li;
  const bool live = item < batch;
  const uint32_t* a = pa + (size_t)(live ? item : 0) * words;
  const uint32_t* b = pb + (size_t)(live ? item : 0) * bStride;
  // the partial word, if any, is word n / 32 (the last one); its top n % 32 bits count
  const uint32_t tailWord = (n & 31u) ? n >> 5 : 0xffffffffu, tailMask = ~0u << ((32u - (n & 31u)) & 31u);
  BoolCounts c{0u, 0u, 0u};
  if (live) {
    if (wide) {
      for (uint32_t p = l; p < words / 4; p += lpi) {
        const uint4 x = ((const uint4*)a)[p], y = ((const uint4*)b)[p];
        const uint32_t k = p * 4;
        bool_take(c, x.x, y.x, k == tailWord ? tailMask : ~0u);
        bool_take(c, x.y, y.y, k + 1 == tailWord ? tailMask : ~0u);
        bool_take(c, x.z, y.z, k + 2 == tailWord ? tailMask : ~0u);
        bool_take(c, x.w, y.w, k + 3 == tailWord ? tailMask : ~0u);
      }
    } else {
      for (uint32_t k = l; k < words; k += lpi) bool_take(c, a[k], b[k], k == tailWord ? tailMask : ~0u);
    }
  }
  const int waveLanes = lpiLog < 6 ? lpiLog : 6;
  for (int m = 1; m < (1 << waveLanes); m <<= 1) {
    c.tt += (uint32_t)__shfl_xor((int)c.tt, m, 64);
    c.tf += (uint32_t)__shfl_xor((int)c.tf, m, 64);
    c.ft += (uint32_t)__shfl_xor((int)c.ft, m, 64);
  }
  if (lpiLog > 6) {            // the whole workgroup on one item
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < kBlock / 64; ++w) { c.tt += part[w].tt; c.tf += part[w].tf; c.ft += part[w].ft; }
  }
  if (live && l == 0) result[item] = bool_finish(op, c.tt, c.tf, c.ft, n);
}

// ---- dynamic time warping ------------------------------------------------------------------------------------
constexpr float kF32Max = 3.40282347e+38f;                  // the reference's F32_MAX

__global__ __launch_bounds__(kBlock) void dtw_window_kernel(int type, int32_t windowSize, int8_t* dst, uint32_t Q,
                                                            uint32_t T, size_t count) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const size_t cell = i % ((size_t)Q * T);
  const int32_t q = (int32_t)(cell / T), t = (int32_t)(cell % T);
  bool in;
  if (type == 1) {                                          // ARM_DTW_SAKOE_CHIBA_WINDOW
    in = abs(q - t) <= windowSize;
  } else {                                                  // ARM_DTW_SLANTED_BAND_WINDOW
    const float diag = 1.0f * (float)q * (float)(int32_t)T / (float)(int32_t)Q;
    in = fabsf((float)t - diag) <= (float)windowSize;
  }
  dst[i] = in ? 1 : 0;
}

// MIN of the reference: x < y ? x : y, a compare and a select (a NaN in x gives y, a NaN in y gives y).
__device__ __forceinline__ float ref_min(float x, float y) { return x < y ? x : y; }

// One wave per item.
__global__ __launch_bounds__(kBlock) void dtw_distance_kernel(const float* pd, const int8_t* pw, size_t wStride,
                                                              float* pdtw, uint32_t Q, uint32_t T, float* result,
                                                              int32_t* status, uint32_t batch) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t item = blockIdx.x * (uint32_t)(kBlock / 64) + wv;
  if (item >= batch) return;                               // wave-uniform; the kernel has no barrier
  const size_t cells = (size_t)Q * T;
  const float* D = pd + (size_t)item * cells;
  const int8_t* W = pw ? pw + (size_t)item * wStride : nullptr;
  float* C = pdtw + (size_t)item * cells;
  for (uint32_t q0 = 0; q0 < Q; q0 += 64) {
    const uint32_t q = q0 + lane;
    const bool row = q < Q;
    const uint32_t rows = min(64u, Q - q0);
    const float* Drow = D + (size_t)(row ? q : 0) * T;
    const int8_t* Wrow = W ? W + (size_t)(row ? q : 0) * T : nullptr;
    float* Crow = C + (size_t)(row ? q : 0) * T;
    const float* above = C + (size_t)(q0 ? q0 - 1 : 0) * T;   // the previous strip's last row
    float cur = kF32Max, prev = kF32Max;                    // this lane's cells of the last two steps
    float seg = kF32Max, up0 = kF32Max, diag0 = kF32Max;    // lane 0's neighbours in the row above
    const uint32_t steps = T + rows - 1;
    for (uint32_t d = 0; d < steps; ++d) {
      if (q0 && (d & 63u) == 0) seg = d + lane < T ? above[d + lane] : kF32Max;   // columns d .. d + 63
      float up = __shfl_up(cur, 1, 64), diag = __shfl_up(prev, 1, 64);
      if (q0) {
        diag0 = up0;
        up0 = __shfl(seg, (int)(d & 63u), 64);              // column d: lane 0's column at this step
      }
      if (lane == 0) { up = up0; diag = diag0; }
      const uint32_t t = d - lane;                          // wraps below zero for the lanes not yet started
      const bool active = row && d >= lane && t < T;
      float v = cur;
      if (active) {
        const bool in = (q == 0 && t == 0) || !Wrow || Wrow[t] == 1;
        v = kF32Max;
        if (in) {
          const float x = Drow[t];
          if (q == 0 && t == 0) v = x;
          else if (t == 0) v = up + x;
          else if (q == 0) v = cur + x;
          else v = ref_min(diag + 2.0f * x, ref_min(cur + x, up + x));
        }
        Crow[t] = v;
      }
      prev = cur;
      cur = v;
    }
    __threadfence();                                        // the next strip (and the epilogue) read this one's last row
  }
  if (lane == 0) {
    const float last = C[cells - 1];
    if (last == kF32Max) {
      if (status) status[item] = -1;                        // ARM_MATH_ARGUMENT_ERROR: no path inside the window
    } else {
      if (status) status[item] = 0;
      result[item] = last / (float)(Q + T);
    }
  }
}

// One lane per item: the reference's walk back from the last cell.  A cell none of whose neighbours is below F32_MAX
// (the reference never leaves it) ends the walk with path length 0.
__global__ __launch_bounds__(kBlock) void dtw_path_kernel(const float* pdtw, uint32_t Q, uint32_t T, int16_t* ppath,
                                                          uint32_t* plen, uint32_t batch) {
  const uint32_t item = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (item >= batch) return;
  const float* C = pdtw + (size_t)item * Q * T;
  int16_t* path = ppath + (size_t)item * 2 * ((size_t)Q + T);
  uint32_t len = 0;
  int q = (int)Q - 1, t = (int)T - 1;
  bool ok = true;
  while (q > 0 || t > 0) {
    int p = -1;
    float current = kF32Max;
    if (q > 0) {
      const float temp = C[(size_t)(q - 1) * T + t];
      if (temp < current) { current = temp; p = 2; }
    }
    if (t > 0) {
      const float temp = C[(size_t)q * T + t - 1];
      if (temp < current) { current = temp; p = 0; }
    }
    if (q > 0 && t > 0) {
      const float temp = C[(size_t)(q - 1) * T + t - 1];
      if (temp < current) { current = temp; p = 1; }
    }
    if (p < 0 || len + 1 >= Q + T) { ok = false; break; }
    path[2 * len] = (int16_t)q;
    path[2 * len + 1] = (int16_t)t;
    ++len;
    if (p <= 1) --t;
    if (p >= 1) --q;
  }
  if (!ok) {
    plen[item] = 0;
    return;
  }
  path[2 * len] = 0;
  path[2 * len + 1] = 0;
  ++len;
  for (uint32_t i = 0, j = len - 1; i < j; ++i, --j) {      // reverse in place
    const int16_t a0 = path[2 * i], a1 = path[2 * i + 1];
    path[2 * i] = path[2 * j];
    path[2 * i + 1] = path[2 * j + 1];
    path[2 * j] = a0;
    path[2 * j + 1] = a1;
  }
  plen[item] = len;
}

}  // namespace

hipError_t distance_f32_launch(int op, const float* a, const float* b, size_t bStride, uint32_t n, float* result,
                               uint32_t batch, float* wa, float* wb, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if ((wa || wb) && (op != kDsCorrelation || !wa || !wb)) return hipErrorInvalidValue;
  switch (op) {
    case kDsBraycurtis: return dist_f32_run<kDsBraycurtis>(a, b, bStride, n, result, batch, wa, wb, st);
    case kDsCanberra: return dist_f32_run<kDsCanberra>(a, b, bStride, n, result, batch, wa, wb, st);
    case kDsChebyshev:
      if (n == 0) return hipErrorInvalidValue;              // the reference reads element 0
      return dist_f32_run<kDsChebyshev>(a, b, bStride, n, result, batch, wa, wb, st);
    case kDsCityblock: return dist_f32_run<kDsCityblock>(a, b, bStride, n, result, batch, wa, wb, st);
    case kDsCorrelation: return dist_f32_run<kDsCorrelation>(a, b, bStride, n, result, batch, wa, wb, st);
    case kDsCosine: return dist_f32_run<kDsCosine>(a, b, bStride, n, result, batch, wa, wb, st);
    case kDsEuclidean: return dist_f32_run<kDsEuclidean>(a, b, bStride, n, result, batch, wa, wb, st);
    case kDsJensenshannon: return dist_f32_run<kDsJensenshannon>(a, b, bStride, n, result, batch, wa, wb, st);
  }
  return hipErrorInvalidValue;
}

hipError_t boolean_distance_launch(int op, const uint32_t* a, const uint32_t* b, size_t bStride, uint32_t n,
                                   float* result, uint32_t batch, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if (op < kBdDice || op > kBdYule) return hipErrorInvalidValue;
  const uint32_t words = (uint32_t)(((uint64_t)n + 31) / 32);
  const bool wide = (((uintptr_t)a | (uintptr_t)b | ((size_t)words * 4) | (bStride * 4)) & 15) == 0;
  const int lpiLog = red_lpi_log(wide ? words / 4 : words);
  const uint32_t ipw = kBlock >> lpiLog;
  const uint64_t grid = ((uint64_t)batch + ipw - 1) / ipw;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bool_dist_kernel, dim3((uint32_t)grid), dim3(kBlock), 0, st, op, a, b, bStride, n, words, result,
                     batch, lpiLog, wide);
  return hipGetLastError();
}

hipError_t dtw_init_window_launch(int type, int32_t windowSize, int8_t* dst, uint32_t rows, uint32_t cols,
                                  uint32_t batch, hipStream_t st) {
  const size_t count = (size_t)rows * cols * batch;
  if (count == 0) return hipSuccess;
  if (type != 1 && type != 3) return hipErrorInvalidValue;
  const uint64_t grid = (count + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dtw_window_kernel, dim3((uint32_t)grid), dim3(kBlock), 0, st, type, windowSize, dst, rows, cols,
                     count);
  return hipGetLastError();
}

hipError_t dtw_distance_launch(const float* dist, const int8_t* window, size_t wStride, float* dtw, uint32_t rows,
                               uint32_t cols, float* result, int32_t* status, uint32_t batch, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if (rows == 0 || cols == 0) return hipErrorInvalidValue;
  const dim3 grid((batch + kBlock / 64 - 1) / (kBlock / 64));
  hipLaunchKernelGGL(dtw_distance_kernel, grid, dim3(kBlock), 0, st, dist, window, wStride, dtw, rows, cols, result,
                     status, batch);
  return hipGetLastError();
}

hipError_t dtw_path_launch(const float* dtw, uint32_t rows, uint32_t cols, int16_t* path, uint32_t* pathLength,
                           uint32_t batch, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if (rows == 0 || cols == 0 || rows > 32768 || cols > 32768) return hipErrorInvalidValue;
  const dim3 grid((batch + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(dtw_path_kernel, grid, dim3(kBlock), 0, st, dtw, rows, cols, path, pathLength, batch);
  return hipGetLastError();
}

}  // namespace mi355x
