// arm_vexp_f32 / arm_vlog_f32, arm_entropy_f32, arm_kullback_leibler_f32, arm_logsumexp_f32,
// arm_logsumexp_dot_prod_f32, arm_svm_{linear,polynomial,rbf}_predict_f32 and arm_gaussian_naive_bayes_predict_f32 over
// a batch of items, bit-exact with the reference's scalar branches (Source/{FastMath,Statistics,SVM,Bayes}Functions:
// the final #else, no FMA contraction).  Every expf and logf is the pinned glibc's (host_expf.hpp, host_logf.hpp).
//
//   vexp, vlog     element-wise, 16-B packs where source and destination are aligned; dst may be src.
//   log domain     entropy, kullback_leibler: one ordered chain from 0.0f of p * logf(p) or pA * logf(pB / pA), negated
//                  at the end.  logsumexp: the maximum by strict > from element 0 (a NaN there stays, a later NaN never
//                  wins), then the chain of expf(x - max), then max + logf(accum); logsumexp_dot_prod forms x = a + b
//                  in registers.  The maximum is associative once element 0's NaN is set aside; which of +0.0 / -0.0
//                  it is does not reach the result (expf(+-0) is 1, and max + logf(accum) has logf(accum) >= +0).
//                  The two mappings are those of chain_f32.hpp: one wave per item below kSumLaneMinBatch items (every
//                  lane forms its element's logf / expf, only the adds are serial), one lane per item from there on.
//   SVM, Bayes     A chain is one support vector's dot product (SVM) or one class's sum over the dimensions (Bayes);
//                  an item has nbOfSupportVectors or numberOfClasses independent chains.  One mapping: the lanes of a
//                  group of G = 2^k <= 64 lanes (the smallest power of two that holds the item's chains, so a wave
//                  takes 64 / G items) run one chain each, in rounds of G chains; the ordered sum over the support
//                  vectors (its terms dual * f(dot) formed in the chains' lanes), or arm_max_f32 over the classes,
//                  then walks the group's lanes in order.  The model is staged in LDS once per workgroup, rows padded
//                  to an odd stride, where it fits 64 KiB; otherwise it is read from global memory.  A workgroup
//                  takes several tiles of items, so the staging (and Bayes' per-class prologue: the chain of
//                  logf(2 pi sigma) and logf(prior), which do not depend on the item) is paid once.
#include "chain_f32.hpp"
#include "common.hpp"
#include "host_expf.hpp"
#include "host_logf.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

// ---- vexp, vlog --------------------------------------------------------------------------------------------
template <int OP>
__device__ __forceinline__ float fm_elem(float x) {
  if constexpr (OP == kFmExp) return host_expf(x);
  else return host_logf(x);
}

// count: words of the whole batch.  vec: a and d are 16-B aligned.
template <int OP>
__global__ __launch_bounds__(kBlock) void fast_math_kernel(const float* a, float* d, size_t count, bool vec) {
  const size_t packs = vec ? count / 4 : 0;
  const size_t stride = (size_t)gridDim.x * kBlock, first = (size_t)blockIdx.x * kBlock + threadIdx.x;
  for (size_t i = first; i < packs; i += stride) {
    const float4 x = ((const float4*)a)[i];
    float4 r;
    r.x = fm_elem<OP>(x.x);
    r.y = fm_elem<OP>(x.y);
    r.z = fm_elem<OP>(x.z);
    r.w = fm_elem<OP>(x.w);
    ((float4*)d)[i] = r;
  }
  for (size_t i = packs * 4 + first; i < count; i += stride) d[i] = fm_elem<OP>(a[i]);
}

// ---- entropy, kullback_leibler, logsumexp, logsumexp_dot_prod --------------------------------------------------
template <int OP> constexpr bool kLdTwo = OP == kLdKullbackLeibler || OP == kLdLogsumexpDot;
template <int OP> constexpr bool kLdMax = OP == kLdLogsumexp || OP == kLdLogsumexpDot;

// the word the chains work on: logsumexp_dot_prod's arm_add_f32
template <int OP>
__device__ __forceinline__ float ld_word(float x, float y) {
  if constexpr (OP == kLdLogsumexpDot) return x + y;
  else return x;
}
template <int OP>
__device__ __forceinline__ float ld_term(float x, float y, float mx) {
  if constexpr (OP == kLdEntropy) return x * host_logf(x);
  else if constexpr (OP == kLdKullbackLeibler) return x * host_logf(y / x);
  else return host_expf(x - mx);                             // x: ld_word
}
template <int OP>
__device__ __forceinline__ float ld_finish(float s, float mx) {
  if constexpr (kLdMax<OP>) return mx + host_logf(s);
  else return -s;
}

// One wave per item.  tmp (logsumexp_dot_prod's drop-in): where a + b is stored, or null.  kLdMax: n > 0.
template <int OP>
__global__ __launch_bounds__(kBlock) void logdom_wave_kernel(const float* pa, const float* pb, size_t bStride,
                                                             uint32_t n, float* result, uint32_t batch, float* tmp) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t item = blockIdx.x * (uint32_t)(kBlock / 64) + w;
  if (item >= batch) return;                                 // wave-uniform; the kernel has no barrier
  const float* a = pa + (size_t)item * n;
  const float* b = kLdTwo<OP> ? pb + (size_t)item * bStride : a;
  float mx = 0.0f;
  if constexpr (kLdMax<OP>) {
    float m = -__builtin_inff();                             // below or equal to every word
    for (uint64_t k = lane; k < n; k += 64) {
      const float x = ld_word<OP>(a[k], b[k]);
      if (x > m) m = x;
    }
    for (int x = 1; x < 64; x <<= 1) {
      const float o = __shfl_xor(m, x, 64);
      if (o > m) m = o;
    }
    const float x0 = ld_word<OP>(a[0], b[0]);
    mx = x0 == x0 ? m : x0;                                  // a NaN at element 0 is never replaced
  }
  float s = 0.0f;
  for (uint64_t k0 = 0; k0 < n; k0 += 64) {
    const uint32_t cnt = (uint32_t)min((uint64_t)64, n - k0);
    float t = 0.0f;
    if (lane < cnt) {
      const float x = ld_word<OP>(a[k0 + lane], b[k0 + lane]);
      if (OP == kLdLogsumexpDot && tmp) tmp[(size_t)item * n + k0 + lane] = x;
      t = ld_term<OP>(x, b[k0 + lane], mx);
    }
    s = chain_lanes(s, t, cnt);
  }
  if (lane == 0) result[item] = ld_finish<OP>(s, mx);
}

// One lane per item; the LDS rows of sum_f32_lane_kernel (statistics.hip) for both sources.  logsumexp reads its
// item twice: the maximum, then the chain.
template <int OP>
__global__ __launch_bounds__(kBlock) void logdom_lane_kernel(const float* pa, const float* pb, size_t bStride,
                                                             uint32_t n, float* result, uint32_t batch) {
  constexpr int KW = kSumChunk, LD = KW + 1;
  __shared__ float am[kBlock * LD];
  __shared__ float bm[kLdTwo<OP> ? kBlock * LD : 1];
  const uint32_t item0 = blockIdx.x * (uint32_t)kBlock, item = item0 + threadIdx.x;
  const float* arow = am + threadIdx.x * LD;
  const float* brow = kLdTwo<OP> ? bm + threadIdx.x * LD : arow;
  float s = 0.0f, mx = 0.0f;
#pragma unroll
  for (int pass = 0; pass < (kLdMax<OP> ? 2 : 1); ++pass) {
    const bool maxPass = kLdMax<OP> && pass == 0;
    for (uint64_t k0 = 0; k0 < n; k0 += KW) {
      const uint32_t kc = (uint32_t)min((uint64_t)KW, n - k0);
      for (uint32_t idx = threadIdx.x; idx < (uint32_t)kBlock * KW; idx += kBlock) {
        const uint32_t r = idx / KW, wd = idx % KW, it = item0 + r;
        if (wd < kc && it < batch) {
          am[r * LD + wd] = pa[(size_t)it * n + k0 + wd];
          if constexpr (kLdTwo<OP>) bm[r * LD + wd] = pb[(size_t)it * bStride + k0 + wd];
        }
      }
      __syncthreads();
      if (item < batch) {
        for (uint32_t k = 0; k < kc; ++k) {
          const float x = ld_word<OP>(arow[k], brow[k]);
          if (maxPass) {
            if (k0 == 0 && k == 0) mx = x;
            else if (x > mx) mx = x;
          } else {
            s = s + ld_term<OP>(x, brow[k], mx);
          }
        }
      }
      __syncthreads();
    }
  }
  if (item < batch) result[item] = ld_finish<OP>(s, mx);
}

template <int OP>
hipError_t logdom_run(const float* a, const float* b, size_t bStride, uint32_t n, float* result, uint32_t batch,
                      float* tmp, hipStream_t st) {
  if (batch >= kSumLaneMinBatch && !tmp) {
    const dim3 grid((batch + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((logdom_lane_kernel<OP>), grid, dim3(kBlock), 0, st, a, b, bStride, n, result, batch);
  } else {
    const dim3 grid((batch + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL((logdom_wave_kernel<OP>), grid, dim3(kBlock), 0, st, a, b, bStride, n, result, batch, tmp);
  }
  return hipGetLastError();
}

// ---- SVM and naive Bayes ---------------------------------------------------------------------------------------
constexpr uint32_t kMlLdsWords = 16384;                      // 64 KiB: the staged model's limit
constexpr uint32_t kMlMaxGrid = 2048;                        // workgroups; each takes every kMlMaxGrid-th tile

// the smallest k with 2^k >= chains, at most 6
int group_log(uint32_t chains) {
  int k = 0;
  while (k < 6 && (1u << k) < chains) ++k;
  return k;
}

// arm_exponent_f32
__device__ __forceinline__ float exponent_f32(float x, int32_t nb) {
  float r = x;
  for (--nb; nb > 0; --nb) r = r * x;
  return r;
}

// The model's arrays are staged as sv rows of ld = dim | 1 words, then dual.  items > 0.
template <int KIND>
__global__ __launch_bounds__(kBlock) void svm_kernel(SvmModel m, const float* in, int32_t* result, float* decision,
                                                     uint32_t items, int gLog, bool staged) {
  extern __shared__ float lds[];
  const uint32_t ld = staged ? (m.dim | 1u) : m.dim;
  if (staged) {
    for (uint32_t idx = threadIdx.x; idx < m.nsv * m.dim; idx += kBlock)
      lds[(idx / m.dim) * ld + idx % m.dim] = m.sv[idx];
    for (uint32_t idx = threadIdx.x; idx < m.nsv; idx += kBlock) lds[m.nsv * ld + idx] = m.dual[idx];
    __syncthreads();
  }
  const float* sv = staged ? lds : m.sv;
  const float* dual = staged ? lds + m.nsv * ld : m.dual;
  const uint32_t G = 1u << gLog, ipb = (uint32_t)kBlock >> gLog;
  const uint32_t l = threadIdx.x & (G - 1), base = (threadIdx.x & 63u) & ~(G - 1);
  const uint32_t tiles = (items + ipb - 1) / ipb;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t item = tile * ipb + (threadIdx.x >> gLog);
    const bool live = item < items;                          // a lane without an item works on the last one
    const float* x = in + (size_t)(live ? item : items - 1) * m.dim;
    float sum = m.intercept;
    for (uint32_t i0 = 0; i0 < m.nsv; i0 += G) {
      const uint32_t cnt = min(G, m.nsv - i0), i = i0 + l;
      float t = 0.0f;
      if (l < cnt) {
        const float* row = sv + (size_t)i * ld;
        float dot = 0.0f;
        for (uint32_t j = 0; j < m.dim; ++j) {
          if constexpr (KIND == kSvmRbf) {
            const float d = x[j] - row[j];
            dot = dot + d * d;
          } else {
            dot = dot + x[j] * row[j];
          }
        }
        if constexpr (KIND == kSvmLinear) t = dual[i] * dot;
        else if constexpr (KIND == kSvmPolynomial) t = dual[i] * exponent_f32(m.gamma * dot + m.coef0, m.degree);
        else t = dual[i] * host_expf(-m.gamma * dot);
      }
      for (uint32_t j = 0; j < cnt; ++j) sum = sum + __shfl(t, (int)(base + j), 64);   // uniform trip count
    }
    if (live && l == 0) {
      result[item] = m.classes[sum <= 0.0f ? 0 : 1];         // STEP: a NaN gives class 1
      if (decision) decision[item] = sum;
    }
  }
}

constexpr float kTwoPi = 2.0f * 3.14159265358979f;           // 2.0f * PI_F

// Staged: theta rows and sigma + epsilon rows of ld = dim | 1 words, then -0.5f * acc1 and logf(prior) per class.
__global__ __launch_bounds__(kBlock) void bayes_kernel(BayesModel m, const float* in, float* prob, uint32_t* cls,
                                                       uint32_t items, int gLog, bool staged) {
  extern __shared__ float lds[];
  const uint32_t C = m.classes, D = m.dim, ld = D | 1u;
  float* theta = lds;
  float* sig = lds + (size_t)C * ld;
  float* half1 = sig + (size_t)C * ld;
  float* lprior = half1 + C;
  if (staged) {
    for (uint32_t idx = threadIdx.x; idx < C * D; idx += kBlock) {
      const uint32_t at = (idx / D) * ld + idx % D;
      theta[at] = m.theta[idx];
      sig[at] = m.sigma[idx] + m.eps;
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < C; c += kBlock) {
      float acc1 = 0.0f;
      for (uint32_t j = 0; j < D; ++j) acc1 = acc1 + host_logf(kTwoPi * sig[c * ld + j]);
      half1[c] = -0.5f * acc1;
      lprior[c] = host_logf(m.priors[c]);
    }
    __syncthreads();
  }
  const uint32_t G = 1u << gLog, ipb = (uint32_t)kBlock >> gLog;
  const uint32_t l = threadIdx.x & (G - 1), base = (threadIdx.x & 63u) & ~(G - 1);
  const uint32_t tiles = (items + ipb - 1) / ipb;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t item = tile * ipb + (threadIdx.x >> gLog);
    const bool live = item < items;
    const float* x = in + (size_t)(live ? item : items - 1) * D;
    float best = 0.0f;
    uint32_t bestAt = 0;
    for (uint32_t c0 = 0; c0 < C; c0 += G) {
      const uint32_t cnt = min(G, C - c0), c = c0 + l;
      float out = 0.0f;
      if (l < cnt) {
        float acc2 = 0.0f, h1, lp;
        if (staged) {
          const float* th = theta + (size_t)c * ld;
          const float* sg = sig + (size_t)c * ld;
          for (uint32_t j = 0; j < D; ++j) {
            const float d = x[j] - th[j];
            acc2 = acc2 + (d * d) / sg[j];
          }
          h1 = half1[c];
          lp = lprior[c];
        } else {
          const float* th = m.theta + (size_t)c * D;
          const float* sg = m.sigma + (size_t)c * D;
          float acc1 = 0.0f;
          for (uint32_t j = 0; j < D; ++j) {
            const float sigma = sg[j] + m.eps, d = x[j] - th[j];
            acc1 = acc1 + host_logf(kTwoPi * sigma);
            acc2 = acc2 + (d * d) / sigma;
          }
          h1 = -0.5f * acc1;
          lp = host_logf(m.priors[c]);
        }
        float tmp = h1;
        tmp = tmp - 0.5f * acc2;
        out = tmp + lp;
        if (live) prob[(size_t)item * C + c] = out;
      }
      for (uint32_t j = 0; j < cnt; ++j) {                   // arm_max_f32: from element 0, replaced on best < v only
        const float v = __shfl(out, (int)(base + j), 64);
        if (c0 == 0 && j == 0) best = v;
        else if (best < v) { best = v; bestAt = c0 + j; }
      }
    }
    if (live && l == 0) cls[item] = bestAt;
  }
}

uint32_t ml_grid(uint32_t items, int gLog) {
  const uint32_t ipb = (uint32_t)kBlock >> gLog, tiles = (items + ipb - 1) / ipb;
  return tiles < kMlMaxGrid ? tiles : kMlMaxGrid;
}

}  // namespace

hipError_t fast_math_launch(int op, const float* a, float* d, size_t count, hipStream_t st) {
  if (count == 0) return hipSuccess;
  const bool vec = (((uintptr_t)a | (uintptr_t)d) & 15) == 0;
  const size_t per = vec ? 4 * (size_t)kBlock : (size_t)kBlock, blocks = (count + per - 1) / per, cap = 0x7fffffff;
  const dim3 grid((uint32_t)(blocks < cap ? blocks : cap));
  if (op == kFmExp) hipLaunchKernelGGL((fast_math_kernel<kFmExp>), grid, dim3(kBlock), 0, st, a, d, count, vec);
  else if (op == kFmLog) hipLaunchKernelGGL((fast_math_kernel<kFmLog>), grid, dim3(kBlock), 0, st, a, d, count, vec);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t logdom_launch(int op, const float* a, const float* b, size_t bStride, uint32_t n, float* result,
                         uint32_t batch, float* tmp, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if (tmp && op != kLdLogsumexpDot) return hipErrorInvalidValue;
  switch (op) {
    case kLdEntropy: return logdom_run<kLdEntropy>(a, a, 0, n, result, batch, nullptr, st);
    case kLdKullbackLeibler: return logdom_run<kLdKullbackLeibler>(a, b, bStride, n, result, batch, nullptr, st);
    case kLdLogsumexp:
      if (n == 0) return hipErrorInvalidValue;                // the reference reads element 0
      return logdom_run<kLdLogsumexp>(a, a, 0, n, result, batch, nullptr, st);
    case kLdLogsumexpDot:
      if (n == 0) return hipErrorInvalidValue;
      return logdom_run<kLdLogsumexpDot>(a, b, bStride, n, result, batch, tmp, st);
  }
  return hipErrorInvalidValue;
}

bool svm_model_staged(uint32_t nsv, uint32_t dim) {
  return (uint64_t)nsv * (dim | 1u) + nsv <= kMlLdsWords;
}

hipError_t svm_predict_launch(int kind, const SvmModel& m, const float* in, int32_t* result, float* decision,
                              uint32_t items, hipStream_t st) {
  if (items == 0) return hipSuccess;
  if ((uint64_t)m.nsv * m.dim > 0xffffffffull) return hipErrorInvalidValue;
  const bool staged = svm_model_staged(m.nsv, m.dim);
  const size_t lds = staged ? sizeof(float) * ((size_t)m.nsv * (m.dim | 1u) + m.nsv) : 0;
  const int gLog = group_log(m.nsv);
  const dim3 grid(ml_grid(items, gLog));
  switch (kind) {
    case kSvmLinear:
      hipLaunchKernelGGL((svm_kernel<kSvmLinear>), grid, dim3(kBlock), lds, st, m, in, result, decision, items, gLog, staged);
      break;
    case kSvmPolynomial:
      hipLaunchKernelGGL((svm_kernel<kSvmPolynomial>), grid, dim3(kBlock), lds, st, m, in, result, decision, items, gLog, staged);
      break;
    case kSvmRbf:
      hipLaunchKernelGGL((svm_kernel<kSvmRbf>), grid, dim3(kBlock), lds, st, m, in, result, decision, items, gLog, staged);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

bool bayes_model_staged(uint32_t classes, uint32_t dim) {
  return 2 * (uint64_t)classes * (dim | 1u) + 2 * (uint64_t)classes <= kMlLdsWords;
}

hipError_t bayes_predict_launch(const BayesModel& m, const float* in, float* prob, uint32_t* cls, uint32_t items,
                                hipStream_t st) {
  if (items == 0) return hipSuccess;
  if (m.classes == 0 || (uint64_t)m.classes * m.dim > 0xffffffffull) return hipErrorInvalidValue;
  const bool staged = bayes_model_staged(m.classes, m.dim);
  const size_t lds = staged ? sizeof(float) * (2 * (size_t)m.classes * (m.dim | 1u) + 2 * (size_t)m.classes) : 0;
  const int gLog = group_log(m.classes);
  hipLaunchKernelGGL(bayes_kernel, dim3(ml_grid(items, gLog)), dim3(kBlock), lds, st, m, in, prob, cls, items, gLog,
                     staged);
  return hipGetLastError();
}

}  // namespace mi355x
