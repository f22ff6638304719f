// Biquad cascades: arm_biquad_cascade_df1_{f32,q31,fast_q31,q15,fast_q15}, arm_biquad_cas_df1_32x64_q31,
// arm_biquad_cascade_df2T_f32 and arm_biquad_cascade_stereo_df2T_f32 over `batch` independent streams.
//
// Reference (Source/FilteringFunctions/arm_biquad_cascade_*.c, scalar path): stages run one after
// another, each over the whole block (the first from pSrc, the rest in place over pDst), with the
// stage's state read before the block and written after it.  Per sample, with the stage state
// {x1, x2, y1, y2} (DF1) or {d1, d2} (DF2T):
//   df1_f32       y = ((((b0 x + b1 x1) + b2 x2) + a1 y1) + a2 y2), every product rounded (no FMA)
//   df1_q31       acc = the five 64-bit products, q63 wrap-around; y = low word of acc >> (31 - postShift)
//   df1_fast_q31  acc = sum of (p + 2^31) >> 32, 32-bit wrap-around; y = acc << (postShift + 1)
//   df1_q15       acc = 64-bit sum of the five 16x16 products; y = SSAT(acc >> (15 - postShift), 16)
//   df1_fast_q15  the same with the sum wrapped to 32 bits; coefficients {b0, 0, b1, b2, a1, a2}
//   32x64_q31     acc = x b0 + x1 b1 + x2 b2 + mult32x64(y1, a1) + mult32x64(y2, a2), q63 wrap-around;
//                 y1 (q63 state) = acc << (postShift + 1); output = low word of acc >> (31 - postShift)
//   df2T_f32      y = b0 x + d1; d1 = (b1 x + d2) + a1 y; d2 = b2 x + a2 y
//   stereo_df2T   per channel y = b0 x + d1; d1 = (b1 x + a1 y) + d2; d2 = b2 x + a2 y
//
// Time cannot be split bit-exactly, so the parallelism is batch x numStages: lane = (stream, stage), a
// systolic pipeline over tiles of kBqT words.  A wave packs P = 64 / S streams of S <= 64 stages; at
// step k the lane of stage s runs tile k - s with its state in registers, and hands its output tile to
// the next lane with wave_shr:1 DPP moves.  Stage-0 lanes take their tile from the wave's LDS input
// rows, last-stage lanes put theirs into the LDS output rows; both are filled / drained kBqG tiles at a
// time with coalesced global accesses (a row of kBqGW words per stream, pitch kBqGW + 1: the row reads
// of the stage-0 lanes hit distinct banks), the next group's loads in flight under the current group's
// arithmetic.  More than 64 stages run as passes of at most 64 in stream order, the first from src and
// the rest in place over dst: the reference's own stage loop.  A wave writes a stream's words only after
// it has read them and no other wave touches the stream, so src == dst needs no copy.
// Long cascades are bound by the one dependent chain a lane runs, so from Op::NS2 stages per pass (and
// a batch that still fills the SIMDs) a lane runs two streams with half tiles, their steps interleaved
// (tuning.hpp gives the measurements).
#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mi355x {

template <int OP> struct BqT;

// ---- DF1 f32
template <> struct BqT<kBqDf1F32> {
  using T = float; using V = float; using ST = float;
  static constexpr int CH = 1, KS = 4, NC = 5, NS2 = MI355X_BQ_NS2_F32;
  struct Co { float b0, b1, b2, a1, a2; };
  struct St { float x1, x2, y1, y2; };
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ void load_c(const T* c, Co& o) { o = {c[0], c[1], c[2], c[3], c[4]}; }
  static __device__ __forceinline__ void load_s(const ST* p, St& s) { s = {p[0], p[1], p[2], p[3]}; }
  static __device__ __forceinline__ void store_s(ST* p, const St& s) { p[0] = s.x1; p[1] = s.x2; p[2] = s.y1; p[3] = s.y2; }
  static __device__ __forceinline__ void step(St& s, const Co& c, const V* x, V* y, int) {
    const float xn = x[0];
    float acc = c.b0 * xn;                 // arm_biquad_cascade_df1_f32.c: left to right
    acc = acc + c.b1 * s.x1;
    acc = acc + c.b2 * s.x2;
    acc = acc + c.a1 * s.y1;
    acc = acc + c.a2 * s.y2;
    s.x2 = s.x1; s.x1 = xn; s.y2 = s.y1; s.y1 = acc;
    y[0] = acc;
  }
};

// ---- DF1 q31 / fast q31 (one state and coefficient layout)
struct BqQ31Base {
  using T = int32_t; using V = int32_t; using ST = int32_t;
  static constexpr int CH = 1, KS = 4, NC = 5, NS2 = MI355X_BQ_NS2_FX;
  struct Co { int32_t b0, b1, b2, a1, a2; };
  struct St { int32_t x1, x2, y1, y2; };
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ void load_c(const T* c, Co& o) { o = {c[0], c[1], c[2], c[3], c[4]}; }
  static __device__ __forceinline__ void load_s(const ST* p, St& s) { s = {p[0], p[1], p[2], p[3]}; }
  static __device__ __forceinline__ void store_s(ST* p, const St& s) { p[0] = s.x1; p[1] = s.x2; p[2] = s.y1; p[3] = s.y2; }
};
__device__ __forceinline__ uint64_t prod64(int32_t a, int32_t b) { return (uint64_t)((int64_t)a * (int64_t)b); }

template <> struct BqT<kBqDf1Q31> : BqQ31Base {
  static __device__ __forceinline__ void step(St& s, const Co& c, const V* x, V* y, int ps) {
    const int32_t xn = x[0];
    const uint64_t acc = prod64(c.b0, xn) + prod64(c.b1, s.x1) + prod64(c.b2, s.x2) + prod64(c.a1, s.y1) +
                         prod64(c.a2, s.y2);
    const int32_t yn = (int32_t)(uint32_t)(acc >> ((31 - ps) & 63));   // low word: the sign fill is cut off
    s.x2 = s.x1; s.x1 = xn; s.y2 = s.y1; s.y1 = yn;
    y[0] = yn;
  }
};
template <> struct BqT<kBqDf1FastQ31> : BqQ31Base {
  static __device__ __forceinline__ void step(St& s, const Co& c, const V* x, V* y, int ps) {
    const int32_t xn = x[0];
    int32_t acc = mult_R(c.b0, xn);        // mult_32x32_keep32_R / multAcc_32x32_keep32_R
    acc = multAcc_R(acc, c.b1, s.x1);
    acc = multAcc_R(acc, c.b2, s.x2);
    acc = multAcc_R(acc, c.a1, s.y1);
    acc = multAcc_R(acc, c.a2, s.y2);
    const int32_t yn = wshl(acc, (ps + 1) & 31);
    s.x2 = s.x1; s.x1 = xn; s.y2 = s.y1; s.y1 = yn;
    y[0] = yn;
  }
};

// ---- DF1 q15 / fast q15: coefficients {b0, 0, b1, b2, a1, a2}
struct BqQ15Base {
  using T = int16_t; using V = int32_t; using ST = int16_t;
  static constexpr int CH = 1, KS = 4, NC = 6, NS2 = MI355X_BQ_NS2_FX;
  struct Co { int32_t b0, b1, b2, a1, a2; };
  struct St { int32_t x1, x2, y1, y2; };
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return (T)v; }
  static __device__ __forceinline__ void load_c(const T* c, Co& o) { o = {c[0], c[2], c[3], c[4], c[5]}; }
  static __device__ __forceinline__ void load_s(const ST* p, St& s) { s = {p[0], p[1], p[2], p[3]}; }
  static __device__ __forceinline__ void store_s(ST* p, const St& s) {
    p[0] = (ST)s.x1; p[1] = (ST)s.x2; p[2] = (ST)s.y1; p[3] = (ST)s.y2;
  }
};
template <> struct BqT<kBqDf1Q15> : BqQ15Base {
  static __device__ __forceinline__ void step(St& s, const Co& c, const V* x, V* y, int ps) {
    const int32_t xn = x[0];               // |words| <= 2^15: the 24-bit products are exact
    const int64_t acc = (int64_t)__mul24(c.b0, xn) + __mul24(c.b1, s.x1) + __mul24(c.b2, s.x2) +
                        __mul24(c.a1, s.y1) + __mul24(c.a2, s.y2);
    const int32_t yn = ssat16((int32_t)(acc >> ((15 - ps) & 63)));
    s.x2 = s.x1; s.x1 = xn; s.y2 = s.y1; s.y1 = yn;
    y[0] = yn;
  }
};
template <> struct BqT<kBqDf1FastQ15> : BqQ15Base {
  static __device__ __forceinline__ void step(St& s, const Co& c, const V* x, V* y, int ps) {
    const int32_t xn = x[0];               // __SMUAD / __SMLAD: 32-bit wrap-around
    const uint32_t acc = (uint32_t)__mul24(c.b0, xn) + (uint32_t)__mul24(c.b1, s.x1) + (uint32_t)__mul24(c.b2, s.x2) +
                         (uint32_t)__mul24(c.a1, s.y1) + (uint32_t)__mul24(c.a2, s.y2);
    const int32_t yn = ssat16((int32_t)acc >> ((15 - ps) & 31));
    s.x2 = s.x1; s.x1 = xn; s.y2 = s.y1; s.y1 = yn;
    y[0] = yn;
  }
};

// ---- 32x64 q31: q63 state {x1, x2 (widened), y1, y2}
template <> struct BqT<kBq32x64> {
  using T = int32_t; using V = int32_t; using ST = int64_t;
  static constexpr int CH = 1, KS = 4, NC = 5, NS2 = MI355X_BQ_NS2_FX;
  struct Co { int32_t b0, b1, b2, a1, a2; };
  struct St { int32_t x1, x2; int64_t y1, y2; };
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ void load_c(const T* c, Co& o) { o = {c[0], c[1], c[2], c[3], c[4]}; }
  static __device__ __forceinline__ void load_s(const ST* p, St& s) { s = {(int32_t)p[0], (int32_t)p[1], p[2], p[3]}; }
  static __device__ __forceinline__ void store_s(ST* p, const St& s) { p[0] = s.x1; p[1] = s.x2; p[2] = s.y1; p[3] = s.y2; }
  // none.h mult32x64: (((q63)(x & 0xFFFFFFFF) * y) >> 32) + ((q63)(x >> 32) * y); both products fit 64 bits
  static __device__ __forceinline__ uint64_t m32x64(int64_t x, int32_t y) {
    const int64_t lo = (int64_t)(uint32_t)x * (int64_t)y;
    return (uint64_t)(lo >> 32) + prod64((int32_t)(x >> 32), y);
  }
  static __device__ __forceinline__ void step(St& s, const Co& c, const V* x, V* y, int ps) {
    const int32_t xn = x[0];
    const uint64_t acc = prod64(xn, c.b0) + prod64(s.x1, c.b1) + prod64(s.x2, c.b2) + m32x64(s.y1, c.a1) +
                         m32x64(s.y2, c.a2);
    s.x2 = s.x1; s.x1 = xn; s.y2 = s.y1;
    s.y1 = (int64_t)(acc << ((ps + 1) & 63));
    y[0] = (int32_t)(uint32_t)(acc >> ((31 - ps) & 63));
  }
};

// ---- DF2T f32, mono and stereo (a frame is CH interleaved words)
template <> struct BqT<kBqDf2TF32> {
  using T = float; using V = float; using ST = float;
  static constexpr int CH = 1, KS = 2, NC = 5, NS2 = MI355X_BQ_NS2_F32;
  struct Co { float b0, b1, b2, a1, a2; };
  struct St { float d1, d2; };
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ void load_c(const T* c, Co& o) { o = {c[0], c[1], c[2], c[3], c[4]}; }
  static __device__ __forceinline__ void load_s(const ST* p, St& s) { s = {p[0], p[1]}; }
  static __device__ __forceinline__ void store_s(ST* p, const St& s) { p[0] = s.d1; p[1] = s.d2; }
  static __device__ __forceinline__ void step(St& s, const Co& c, const V* x, V* y, int) {
    const float xn = x[0];
    const float acc = c.b0 * xn + s.d1;
    const float t = c.b1 * xn + s.d2;      // arm_biquad_cascade_df2T_f32.c: (b1 x + d2) + a1 y
    s.d1 = t + c.a1 * acc;
    s.d2 = c.b2 * xn + c.a2 * acc;
    y[0] = acc;
  }
};
template <> struct BqT<kBqStereoDf2TF32> {
  using T = float; using V = float; using ST = float;
  static constexpr int CH = 2, KS = 4, NC = 5, NS2 = MI355X_BQ_NS2_F32;
  struct Co { float b0, b1, b2, a1, a2; };
  struct St { float d1a, d2a, d1b, d2b; };
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ void load_c(const T* c, Co& o) { o = {c[0], c[1], c[2], c[3], c[4]}; }
  static __device__ __forceinline__ void load_s(const ST* p, St& s) { s = {p[0], p[1], p[2], p[3]}; }
  static __device__ __forceinline__ void store_s(ST* p, const St& s) { p[0] = s.d1a; p[1] = s.d2a; p[2] = s.d1b; p[3] = s.d2b; }
  static __device__ __forceinline__ void chan(float& d1, float& d2, const Co& c, float xn, float& yo) {
    const float acc = c.b0 * xn + d1;
    const float t = c.b1 * xn + c.a1 * acc;   // arm_biquad_cascade_stereo_df2T_f32.c: (b1 x + a1 y) + d2
    d1 = t + d2;
    d2 = c.b2 * xn + c.a2 * acc;
    yo = acc;
  }
  static __device__ __forceinline__ void step(St& s, const Co& c, const V* x, V* y, int) {
    chan(s.d1a, s.d2a, c, x[0], y[0]);
    chan(s.d1b, s.d2b, c, x[1], y[1]);
  }
};

constexpr int kBqT = MI355X_BQ_T;          // words per tile (a lane's registers)
constexpr int kBqG = MI355X_BQ_G;          // tiles per coalesced I/O group
constexpr int kBqGW = kBqT * kBqG;         // words of a stream per group
constexpr int kBqPitch = kBqGW + 1;        // LDS row pitch: stride 1 mod 32 banks across streams
// From Op::NS2 stages per pass a lane runs two streams, if that still leaves a wave for each of the SIMDs
constexpr int kBqNs2Waves = 1024;
static_assert(kBqT % 4 == 0 && 64 % kBqGW == 0 && kBqGW <= 64 && MI355X_BQ_NS2_F32 >= 2 && MI355X_BQ_NS2_FX >= 2,
              "whole stereo frames per half tile, whole rows per 64 lanes, at most 64 rows per wave");

__device__ __forceinline__ void bq_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename V>
__device__ __forceinline__ V bq_shift_up1(V v) {   // lane l <- lane l - 1
  const int r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  return __builtin_bit_cast(V, r);
}

// Makes every word of s count as used here, so the wait for the loads that filled it is placed here.
// Without it the wait for the coefficient and state loads lands inside the step loop (their first
// use) as vmcnt(0), and there it also waits for the next group's loads in every step.
template <typename S>
__device__ __forceinline__ void bq_pin(S& s) {
  static_assert(sizeof(S) % 4 == 0, "32-bit words");
  uint32_t w[sizeof(S) / 4];
  __builtin_memcpy(w, &s, sizeof(S));
#pragma unroll
  for (unsigned i = 0; i < sizeof(S) / 4; ++i) asm volatile("" : "+v"(w[i]));
  __builtin_memcpy(&s, w, sizeof(S));
}

struct BqIn {
  uint32_t B;         // frames per stream and call
  uint32_t batch;
  int S;              // stages of this pass (1 .. 64)
  int P;              // streams per wave: 64 / S, times the streams per lane
  int ps;             // postShift
  uint32_t sstride;   // state words per stream (all passes)
  uint32_t nT;        // tiles per stream
};

// src and dst may be the same buffer: no __restrict__ on them.
// NS streams per lane (independent recurrences interleaved in one instruction stream), each with tiles of
// kBqT / NS words, so a lane holds kBqT words per step either way; in.P counts all streams of the wave.
template <int OP, int NS>
__global__ __launch_bounds__(kBlock) void biquad_kernel(const typename BqT<OP>::T* __restrict__ coeffs,
                                                        const typename BqT<OP>::T* src, typename BqT<OP>::T* dst,
                                                        typename BqT<OP>::ST* __restrict__ state, BqIn in) {
  using Op = BqT<OP>;
  using V = typename Op::V;
  using ST = typename Op::ST;
  constexpr int CH = Op::CH, T = kBqT / NS, G = kBqGW / T, TF = T / CH;
  static_assert(T % 2 == 0 && T * G == kBqGW, "whole stereo frames per tile, whole tiles per group");
  extern __shared__ int bq_lds[];
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;   // wave-uniform
  const uint64_t f0 = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + wib) * (uint32_t)in.P;
  if (f0 >= in.batch) return;              // whole waves; the kernel has no workgroup barrier
  V* tin = reinterpret_cast<V*>(bq_lds) + wib * 2 * in.P * kBqPitch;
  V* tout = tin + in.P * kBqPitch;
  const int pl = lane / in.S, s = lane - pl * in.S, p0 = pl * NS;   // the lane's streams: p0 .. p0 + NS - 1
  const bool live = p0 < in.P && f0 + p0 < in.batch;
  const uint64_t BW = (uint64_t)in.B * CH;
  const int ni = (in.P * kBqGW + 63) / 64;  // 64-lane rounds per group

  typename Op::Co c;
  typename Op::St stt[NS];
  Op::load_c(coeffs + s * Op::NC, c);
  ST* sp = state + (f0 + p0) * in.sstride + s * Op::KS;
  bool valid[NS];
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    stt[u] = {};
    valid[u] = live && f0 + p0 + u < in.batch;
    if (valid[u]) Op::load_s(sp + (uint64_t)u * in.sstride, stt[u]);
  }
  bq_pin(c);
#pragma unroll
  for (int u = 0; u < NS; ++u) bq_pin(stt[u]);

  // Round i of a group moves row r0 + i kRows, word o0 of the wave's rows.  The row stride and count
  // pass through an empty asm at each use: hoisted out of the step loop, the 2 x kBqGW 64-bit addresses
  // and their masks would take more registers than the filter itself.
  constexpr int kRows = 64 / kBqGW;        // rows per 64-lane round
  const int r0 = lane / kBqGW, o0 = lane % kBqGW;
  const int nrows = (int)min((uint64_t)in.P, (uint64_t)in.batch - f0);
  const int lrow = r0 * kBqPitch + o0;
  V pf[kBqGW];
  auto prefetch = [&](uint32_t g) {        // addresses clamped to the wave's first word, no branch per load
    uint64_t stride = BW * kRows;
    int rows = nrows;
    asm volatile("" : "+s"(stride), "+s"(rows));
    const uint64_t wd = (uint64_t)g * kBqGW + o0;
    const typename Op::T* base = src + f0 * BW;
    const typename Op::T* q = base + (uint64_t)r0 * BW + wd;
    const bool wok = wd < BW;
#pragma unroll
    for (int i = 0; i < kBqGW; ++i) {
      if (i < ni) {
        pf[i] = Op::in(*((wok && r0 + i * kRows < rows) ? q : base));
        q += stride;
      }
    }
  };
  auto stage_in = [&]() {
    int rows = in.P;
    asm volatile("" : "+s"(rows));
#pragma unroll
    for (int i = 0; i < kBqGW; ++i) {
      if (i < ni) {
        if (r0 + i * kRows < rows) tin[lrow + i * kRows * kBqPitch] = pf[i];
      }
    }
  };
  auto flush = [&](uint32_t g) {
    uint64_t stride = BW * kRows;
    int rows = nrows;
    asm volatile("" : "+s"(stride), "+s"(rows));
    const uint64_t wd = (uint64_t)g * kBqGW + o0;
    typename Op::T* q = dst + (f0 + r0) * BW + wd;
    const bool wok = wd < BW;
#pragma unroll
    for (int i = 0; i < kBqGW; ++i) {
      if (i < ni) {
        if (wok && r0 + i * kRows < rows) *q = Op::out(tout[lrow + i * kRows * kBqPitch]);
        q += stride;
      }
    }
  };

  // tile counts fit 31 bits (the host checks): the step loop runs on 32-bit indices
  const int nT = (int)in.nT, steps = nT + in.S - 1;
  const int last_nv = (int)(BW - (uint64_t)(nT - 1) * T) / CH;   // frames of the stream's last tile
  const bool ragged = last_nv != TF;
  V y[NS][T];
#pragma unroll
  for (int u = 0; u < NS; ++u)
#pragma unroll
    for (int j = 0; j < T; ++j) y[u][j] = (V)0;
  prefetch(0);
  for (int k = 0; k < steps; ++k) {
    const int kg = k % G;
    if (kg == 0 && k < nT) {
      bq_wave_sync();                      // the previous group's row reads are done
      stage_in();
      bq_wave_sync();
      if (k + G < nT) prefetch((uint32_t)(k / G + 1));   // in flight under this group's arithmetic
    }
    V x[NS][T];
#pragma unroll
    for (int u = 0; u < NS; ++u)
#pragma unroll
      for (int j = 0; j < T; ++j) x[u][j] = bq_shift_up1(y[u][j]);   // the previous stage's tiles of the last step
    if (s == 0 && live && k < nT) {
#pragma unroll
      for (int u = 0; u < NS; ++u)
#pragma unroll
        for (int j = 0; j < T; ++j) x[u][j] = tin[(p0 + u) * kBqPitch + kg * T + j];
    }
    const int t = k - s;
    // a lane whose second stream lies past the batch runs it on zeros; nothing of it is stored
    if (live && t >= 0 && t < nT) {
      if (!(ragged && t == nT - 1)) {
#pragma unroll
        for (int j = 0; j < TF; ++j)
#pragma unroll
          for (int u = 0; u < NS; ++u) Op::step(stt[u], c, &x[u][j * CH], &y[u][j * CH], in.ps);
      } else {                             // the streams' last, partial tile
#pragma unroll
        for (int j = 0; j < TF; ++j)
          if (j < last_nv) {
#pragma unroll
            for (int u = 0; u < NS; ++u) Op::step(stt[u], c, &x[u][j * CH], &y[u][j * CH], in.ps);
          }
      }
    }
    const int tl = k - (in.S - 1);         // the tile the last stage finished in this step
    if (tl >= 0) {
      const int lg = tl % G;
      if (s == in.S - 1 && live) {
#pragma unroll
        for (int u = 0; u < NS; ++u)
#pragma unroll
          for (int j = 0; j < T; ++j) tout[(p0 + u) * kBqPitch + lg * T + j] = y[u][j];
      }
      if (lg == G - 1 || tl == nT - 1) {
        bq_wave_sync();
        flush((uint32_t)(tl / G));
        bq_wave_sync();
      }
    }
  }
#pragma unroll
  for (int u = 0; u < NS; ++u)
    if (valid[u]) Op::store_s(sp + (uint64_t)u * in.sstride, stt[u]);
}

template <int OP>
static hipError_t biquad_launch(const void* coeffs, uint32_t num_stages, int ps, const void* src, void* dst, uint32_t B,
                                uint32_t batch, void* state, hipStream_t st) {
  using Op = BqT<OP>;
  using T = typename Op::T;
  using ST = typename Op::ST;
  if (batch == 0 || B == 0) return hipSuccess;
  if (num_stages == 0 || !coeffs || !src || !dst || !state) return hipErrorInvalidValue;
  const uint64_t BW = (uint64_t)B * Op::CH;
  const uint64_t sstride = (uint64_t)num_stages * Op::KS;
  if (sstride > 0xffffffffu) return hipErrorInvalidValue;
  const size_t ib = sizeof(T) * (size_t)batch * BW;
  T* src_copy = nullptr;                   // partial overlap: another stream's input would be overwritten
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  hipError_t e = hipSuccess;
  if (s0 != d0 && s0 < d0 + ib && d0 < s0 + ib) {
    e = hipMallocAsync((void**)&src_copy, ib, st);
    if (e == hipSuccess) e = hipMemcpyAsync(src_copy, src, ib, hipMemcpyDeviceToDevice, st);
    src = src_copy;
  }
  for (uint32_t m0 = 0; e == hipSuccess && m0 < num_stages; m0 += 64) {
    BqIn in;
    in.B = B;
    in.batch = batch;
    in.S = (int)(num_stages - m0 < 64u ? num_stages - m0 : 64u);
    // two streams per lane once the arithmetic, not the memory, sets the pace and the batch still gives
    // every SIMD a wave
    const int ns = in.S >= Op::NS2 && (uint64_t)batch >= (uint64_t)kBqNs2Waves * 2 * (64 / in.S) ? 2 : 1;
    in.P = 64 / in.S * ns;
    in.ps = ps;
    in.sstride = (uint32_t)sstride;
    in.nT = (uint32_t)((BW + kBqT / ns - 1) / (kBqT / ns));   // <= 2^33 / 8 words: fits the kernel's int
    const int wpb = in.P > 32 ? 2 : 4;     // LDS: 2 P rows per wave, at most 33 KiB per workgroup
    const uint64_t waves = ((uint64_t)batch + in.P - 1) / in.P;
    const uint64_t blocks = (waves + wpb - 1) / wpb;
    if (blocks > 0x7fffffffu) { e = hipErrorInvalidValue; break; }
    const size_t lds = sizeof(int) * (size_t)wpb * 2 * in.P * kBqPitch;
    const T* cs = (const T*)coeffs + (size_t)m0 * Op::NC;
    const T* in_p = m0 ? (const T*)dst : (const T*)src;
    ST* st_p = (ST*)state + (size_t)m0 * Op::KS;
    if (ns == 2)
      hipLaunchKernelGGL((biquad_kernel<OP, 2>), dim3((uint32_t)blocks), dim3(wpb * 64), lds, st, cs, in_p, (T*)dst,
                         st_p, in);
    else
      hipLaunchKernelGGL((biquad_kernel<OP, 1>), dim3((uint32_t)blocks), dim3(wpb * 64), lds, st, cs, in_p, (T*)dst,
                         st_p, in);
    e = hipGetLastError();
  }
  if (src_copy) (void)hipFreeAsync(src_copy, st);
  return e;
}

hipError_t biquad_run(int op, const void* coeffs, uint32_t num_stages, int post_shift, const void* src, void* dst,
                      uint32_t block_size, uint32_t batch, void* state, hipStream_t st) {
  switch (op) {
#define MI355X_BQ_CASE(OP) \
  case OP: return biquad_launch<OP>(coeffs, num_stages, post_shift, src, dst, block_size, batch, state, st);
    MI355X_BQ_CASE(kBqDf1F32)
    MI355X_BQ_CASE(kBqDf1Q31)
    MI355X_BQ_CASE(kBqDf1FastQ31)
    MI355X_BQ_CASE(kBqDf1Q15)
    MI355X_BQ_CASE(kBqDf1FastQ15)
    MI355X_BQ_CASE(kBq32x64)
    MI355X_BQ_CASE(kBqDf2TF32)
    MI355X_BQ_CASE(kBqStereoDf2TF32)
#undef MI355X_BQ_CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mi355x
