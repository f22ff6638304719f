// IIR lattice filters: arm_iir_lattice_f32 / _q31 / _q15, `batch` independent streams sharing the
// reflection (k) and ladder (v) coefficients.
//
// Reference (Source/FilteringFunctions/arm_iir_lattice_f32.c, _q31.c, _q15.c, scalar branch): the
// live state is N = numStages words s[0..N-1]; per sample, f = x, acc = 0, then for j = 0..N-1 (the
// pkCoeffs order, stage N - j):
//   g = s[j];  f' = f - k[j] g;  g' = g + k[j] f';  acc += g' v[j];  s[j-1] = g' (j > 0);  f = f'
// and after the last stage acc += f v[N], s[N-1] = f, y = acc.  (The reference's buffer slides by one
// word per sample, which is this in-place shift; its remaining blockSize words are scratch.)
// Arithmetic per type: f32 multiply then add / subtract, never fused; q31 (q31)(((q63) a k) >> 31)
// with clip_q63_to_q31 on f' and g', a wrapping q63 acc, y = (q31)(acc >> 31); q15 32-bit products
// >> 15 with __SSAT(., 16) on f' and g', a q63 acc of 32-bit products, y = __SSAT(acc >> 15, 16).
//
// Mapping: one lane per stream, one wave per workgroup, 64 streams per wave.  The recursion runs over
// time and over stages, so a stream is a serial chain; 64 of them fill a wave and the stages' state
// stays in the lane: in registers (N <= kIirReg, with k and v; instances of 4, 8, 16 and kIirReg stages,
// whose stage loop is free of guards when N is exactly the instance's count), in LDS as [stage][lane]
// (bank = lane, conflict-free; N <= kIirLds) or, beyond that, in the caller's d_state itself (the slow path).
// Global I/O is [batch][blockSize] stream-major, so a wave moves 64 x kIirTS tiles through LDS rows of
// pitch kIirTS + 1: coalesced row segments on the global side, conflict-free column reads per lane.
// d_src == d_dst is fine: a tile is read whole before it is written.
#include "common.hpp"
#include "kernels.hpp"

namespace mi355x {

namespace {

__device__ __forceinline__ int32_t clip_q63_q31(int64_t v) {
  return v > 0x7FFFFFFFLL ? 0x7FFFFFFF : (v < -0x80000000LL ? (int32_t)0x80000000 : (int32_t)v);
}

template <int OP> struct IirT;
template <> struct IirT<kIirF32> {
  using T = float; using V = float; using A = float;
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ V fnext(V f, V k, V g) { const float p = k * g; return f - p; }
  static __device__ __forceinline__ V gnext(V g, V k, V f) { const float p = k * f; return g + p; }
  static __device__ __forceinline__ A mac(A acc, V g, V v) { const float p = g * v; return acc + p; }
  static __device__ __forceinline__ V result(A acc) { return acc; }
};
template <> struct IirT<kIirQ31> {
  using T = int32_t; using V = int32_t; using A = uint64_t;
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ int32_t mul31(V a, V b) { return (int32_t)(((int64_t)a * b) >> 31); }
  static __device__ __forceinline__ V fnext(V f, V k, V g) { return clip_q63_q31((int64_t)f - mul31(g, k)); }
  static __device__ __forceinline__ V gnext(V g, V k, V f) { return clip_q63_q31((int64_t)g + mul31(f, k)); }
  static __device__ __forceinline__ A mac(A acc, V g, V v) { return acc + (uint64_t)((int64_t)g * v); }
  static __device__ __forceinline__ V result(A acc) { return (int32_t)((int64_t)acc >> 31); }
};
template <> struct IirT<kIirQ15> {
  using T = int16_t; using V = int32_t; using A = uint64_t;
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return (T)v; }
  // |f|, |g|, |k| <= 2^15: the products fit 32 bits
  static __device__ __forceinline__ V fnext(V f, V k, V g) { return ssat16(f - ((g * k) >> 15)); }
  static __device__ __forceinline__ V gnext(V g, V k, V f) { return ssat16(((f * k) >> 15) + g); }
  static __device__ __forceinline__ A mac(A acc, V g, V v) { return acc + (uint64_t)(int64_t)(g * v); }
  // __SSAT takes an int32_t: acc >> 15 is truncated to 32 bits first (none.h)
  static __device__ __forceinline__ V result(A acc) { return ssat16((int32_t)((int64_t)acc >> 15)); }
};

constexpr int kIirTS = MI355X_IIR_TS;      // samples per tile row
constexpr int kIirPitch = kIirTS + 1;
constexpr int kIirReg = MI355X_IIR_REG;    // stages held in registers
constexpr int kIirLds = MI355X_IIR_LDS;    // stages held in LDS

// NR > 0: register tier (N <= NR; EXACT: N == NR, the stage loop has no guards); NR == 0: LDS tier;
// NR < 0: the state stays in d_state.
template <int OP, int NR, bool EXACT>
__global__ __launch_bounds__(64) void iir_lattice_kernel(const typename IirT<OP>::T* __restrict__ pk,
                                                         const typename IirT<OP>::T* __restrict__ pv,
                                                         const typename IirT<OP>::T* src, typename IirT<OP>::T* dst,
                                                         typename IirT<OP>::T* state, uint32_t batch, uint32_t B,
                                                         int N) {
  using Op = IirT<OP>;
  using T = typename Op::T;
  using V = typename Op::V;
  using A = typename Op::A;
  extern __shared__ int32_t iir_smem[];
  V* tile = (V*)iir_smem;                          // [64][kIirPitch]
  V* kv = tile + 64 * kIirPitch;                   // {k_j, v_j} pairs, then v_N (NR >= 0)
  V* gl = kv + 2 * N + 2;                          // [N][64] (NR == 0)
  const int lane = threadIdx.x;
  const uint64_t f0 = (uint64_t)blockIdx.x * 64, f = f0 + lane;
  const bool live = f < batch;
  const uint32_t rows = (uint32_t)min((uint64_t)64, batch - f0);
  T* gs = state + f * (uint64_t)N;                 // this lane's state words (dereferenced when live)

  if constexpr (NR >= 0) {
    for (int j = lane; j < N; j += 64) { kv[2 * j] = Op::in(pk[j]); kv[2 * j + 1] = Op::in(pv[j]); }
    if (lane == 0) kv[2 * N] = Op::in(pv[N]);
  }
  if constexpr (NR == 0) {                         // coalesced: element e of the wave's rows x N words
    const T* s0 = state + f0 * (uint64_t)N;
    for (uint32_t e = lane; e < rows * (uint32_t)N; e += 64) gl[(e % N) * 64 + e / N] = Op::in(s0[e]);
  }
  __syncthreads();
  V g[NR > 0 ? NR : 1], kr[NR > 0 ? NR : 1], vr[NR > 0 ? NR : 1];
  V vlast = 0;
  if constexpr (NR > 0) {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      g[j] = (live && j < N) ? Op::in(gs[j]) : (V)0;
      kr[j] = j < N ? kv[2 * j] : (V)0;
      vr[j] = j < N ? kv[2 * j + 1] : (V)0;
    }
    vlast = kv[2 * N];
  }

  // a tile's words are fetched into registers one tile ahead, all loads in flight under the previous tile's stages
  V xr[kIirTS];
  auto fetch = [&](uint32_t n0) {
#pragma unroll
    for (int i = 0; i < kIirTS; ++i) {
      const uint32_t e = i * 64 + lane, row = e / kIirTS, col = e % kIirTS;
      const bool ok = row < rows && n0 + col < B;
      xr[i] = ok ? Op::in(src[(f0 + row) * B + n0 + col]) : (V)0;
    }
  };
  fetch(0);
  for (uint32_t n0 = 0; n0 < B; n0 += kIirTS) {
    const uint32_t cnt = min((uint32_t)kIirTS, B - n0);
#pragma unroll
    for (int i = 0; i < kIirTS; ++i) {
      const uint32_t e = i * 64 + lane;
      tile[(e / kIirTS) * kIirPitch + e % kIirTS] = xr[i];
    }
    __syncthreads();
    if (n0 + kIirTS < B) fetch(n0 + kIirTS);
    if (live) {
      V* my = tile + lane * kIirPitch;
      for (uint32_t c = 0; c < cnt; ++c) {
        V fc = my[c];
        A acc = 0;
        if constexpr (NR > 0) {
#pragma unroll
          for (int j = 0; j < NR; ++j) {
            if (EXACT || j < N) {
              const V gc = g[j];
              const V fn = Op::fnext(fc, kr[j], gc);
              const V gn = Op::gnext(gc, kr[j], fn);
              acc = Op::mac(acc, gn, vr[j]);
              if (j > 0) g[j - 1] = gn;
              if (EXACT ? j == NR - 1 : j == N - 1) g[j] = fn;
              fc = fn;
            }
          }
          acc = Op::mac(acc, fc, vlast);
        } else {
          for (int j = 0; j < N; ++j) {
            V gc, kj, vj;
            if constexpr (NR == 0) { gc = gl[j * 64 + lane]; kj = kv[2 * j]; vj = kv[2 * j + 1]; }
            else { gc = Op::in(gs[j]); kj = Op::in(pk[j]); vj = Op::in(pv[j]); }
            const V fn = Op::fnext(fc, kj, gc);
            const V gn = Op::gnext(gc, kj, fn);
            acc = Op::mac(acc, gn, vj);
            if (j > 0) {
              if constexpr (NR == 0) gl[(j - 1) * 64 + lane] = gn;
              else gs[j - 1] = Op::out(gn);
            }
            fc = fn;
          }
          if constexpr (NR == 0) { gl[(N - 1) * 64 + lane] = fc; acc = Op::mac(acc, fc, kv[2 * N]); }
          else { gs[N - 1] = Op::out(fc); acc = Op::mac(acc, fc, Op::in(pv[N])); }
        }
        my[c] = Op::result(acc);
      }
    }
    __syncthreads();
    V yr[kIirTS];
#pragma unroll
    for (int i = 0; i < kIirTS; ++i) {
      const uint32_t e = i * 64 + lane;
      yr[i] = tile[(e / kIirTS) * kIirPitch + e % kIirTS];
    }
#pragma unroll
    for (int i = 0; i < kIirTS; ++i) {
      const uint32_t e = i * 64 + lane, row = e / kIirTS, col = e % kIirTS;
      if (row < rows && col < cnt) dst[(f0 + row) * B + n0 + col] = Op::out(yr[i]);
    }
    __syncthreads();
  }

  if constexpr (NR > 0) {
    if (live) {
#pragma unroll
      for (int j = 0; j < NR; ++j)
        if (j < N) gs[j] = Op::out(g[j]);
    }
  }
  if constexpr (NR == 0) {
    T* s0 = state + f0 * (uint64_t)N;
    for (uint32_t e = lane; e < rows * (uint32_t)N; e += 64) s0[e] = Op::out(gl[(e % N) * 64 + e / N]);
  }
}

template <int OP>
hipError_t iir_launch(const void* pk, const void* pv, int N, const void* src, void* dst, uint32_t B, uint32_t batch,
                      void* state, hipStream_t st) {
  using T = typename IirT<OP>::T;
  if (batch == 0 || B == 0) return hipSuccess;
  if (N < 1 || !pk || !pv || !src || !dst || !state) return hipErrorInvalidValue;
  const dim3 grid((batch + 63) / 64), block(64);
  const size_t base = sizeof(int32_t) * 64 * kIirPitch, kvb = sizeof(int32_t) * (2 * (size_t)N + 2);
#define MI355X_IIR_GO(NR, EXACT, LDS)                                                                       \
  hipLaunchKernelGGL((iir_lattice_kernel<OP, NR, EXACT>), grid, block, LDS, st, (const T*)pk, (const T*)pv, \
                     (const T*)src, (T*)dst, (T*)state, batch, B, N)
#define MI355X_IIR_TIER(NR)                                  \
  do {                                                      \
    if (N == NR) MI355X_IIR_GO(NR, true, base + kvb);       \
    else MI355X_IIR_GO(NR, false, base + kvb);              \
  } while (0)
  if (N <= 4) MI355X_IIR_TIER(4);
  else if (N <= 8) MI355X_IIR_TIER(8);
  else if (N <= 16) MI355X_IIR_TIER(16);
  else if (N <= kIirReg) MI355X_IIR_TIER(kIirReg);
  else if (N <= kIirLds) MI355X_IIR_GO(0, false, base + kvb + sizeof(int32_t) * 64 * (size_t)N);
  else MI355X_IIR_GO(-1, false, base);
#undef MI355X_IIR_TIER
#undef MI355X_IIR_GO
  return hipGetLastError();
}

}  // namespace

hipError_t iir_lattice_run(int op, const void* pk, const void* pv, int num_stages, const void* src, void* dst,
                           uint32_t block_size, uint32_t batch, void* state, hipStream_t st) {
  switch (op) {
    case kIirF32: return iir_launch<kIirF32>(pk, pv, num_stages, src, dst, block_size, batch, state, st);
    case kIirQ31: return iir_launch<kIirQ31>(pk, pv, num_stages, src, dst, block_size, batch, state, st);
    case kIirQ15: return iir_launch<kIirQ15>(pk, pv, num_stages, src, dst, block_size, batch, state, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mi355x
