// LMS and normalised LMS adaptive filters: arm_lms_f32 / _q31 / _q15, arm_lms_norm_f32 / _q15, `batch`
// independent streams, each with its own coefficients, history and (normalised) energy / x0.
//
// Reference (Source/FilteringFunctions/arm_lms_*.c, arm_lms_norm_*.c, scalar branch; arm_recip_q15 in
// Include/dsp/utils.h): the window w[0..T-1] is the T = numTaps newest samples, oldest first (the state
// is its first T - 1 words); the coefficients are stored time-reversed and updated in place.  Per
// sample: acc = sum_i w[i] c[i] (i ascending, one accumulator), out = acc (f32) or the lShift / uShift
// recombination (fixed point), e = ref - out, then c[i] += weight w[i] with
//   f32   weight = e mu                       (normalised: (e mu) / (energy + 0.000000119209289f))
//   q31   alpha = (q31)(((q63) e mu) >> 31); c = clip(c + (((q31)(((q63) alpha w) >> 32)) << 1))
//   q15   alpha = (q15)((e mu) >> 15);       c = __SSAT(c + ((alpha w) >> 15), 16)
//   q15 normalised: alpha = __SSAT((((q15)((e mu) >> 15)) oneByEnergy) >> (15 - postShift'), 16) with
//         (oneByEnergy, postShift') = arm_recip_q15((q15_t)(energy + 5)), the argument wrapped to 16 bits
// and, normalised, energy -= x0^2, energy += in^2 before the sum and x0 = w[0] after the update.
//
// Mapping: one lane per stream (every coefficient depends on the previous sample's error, and the f32
// sum is a serial chain over the taps, so a stream offers no parallelism; the fixed-point kinds take
// the same mapping so that one kernel serves all five functions).  A wave owns 64 streams; a stream's
// coefficients and its history live in the lane's registers while T <= kLmsReg (instances of 4, 8, 16 and
// kLmsReg taps, free of guards when T is exactly the instance's count; the window moves by register moves),
// in LDS as [tap][lane] (bank = lane: conflict-free), the history a ring of T words with a moving head (no
// shifting), while T <= kLmsLds, and beyond that in global memory: the caller's d_coeffs in place and a ring
// in a workspace.  Global I/O as iir_lattice.hip: 64 x kLmsTS
// tiles through padded LDS rows; out overwrites the src tile and err the ref tile, so d_out == d_src
// and d_err == d_ref are fine.
#include "common.hpp"
#include "kernels.hpp"

namespace mi355x {

namespace {

__device__ __forceinline__ int32_t clip_q63_q31(int64_t v) {
  return v > 0x7FFFFFFFLL ? 0x7FFFFFFF : (v < -0x80000000LL ? (int32_t)0x80000000 : (int32_t)v);
}

// acc_l >> lShift | acc_h << uShift on 32-bit halves (arm_lms_q31.c:154-159, arm_lms_q15.c:141-147)
__device__ __forceinline__ int32_t recombine(uint64_t acc, int lshift, int ushift) {
  const uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
  return (int32_t)((lo >> (lshift & 31)) | (hi << (ushift & 31)));
}

// arm_recip_q15 (utils.h:116-161) on the 16-bit argument `in`; returns signBits + 1
__device__ __forceinline__ int recip_q15(int32_t in, int32_t* dst, const int16_t* __restrict__ table) {
  const uint32_t sign_bits = (uint32_t)(__clz(in > 0 ? in : -in) - 17);
  in = (int16_t)((uint32_t)in << (sign_bits & 31));
  int32_t out = table[(uint32_t)(in >> 8) & 63u];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int32_t t = 0x7FFF - ((in * out) >> 15);
    out = (int16_t)((out * t) >> 14);
  }
  *dst = out;
  return (int)(sign_bits + 1);
}

struct LmsScalars {
  int32_t mu;            // the type's word (f32: its bits)
  int32_t post_shift;
};

template <int OP> struct LmsT;
template <> struct LmsT<kLmsF32> {
  using T = float; using V = float; using A = float;
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ A mac(A acc, V x, V c) { const float p = x * c; return acc + p; }
  static __device__ __forceinline__ V result(A acc, const LmsScalars&) { return acc; }
  static __device__ __forceinline__ V error(V ref, V out) { return ref - out; }
  static __device__ __forceinline__ V weight(V e, const LmsScalars& s) { return e * __int_as_float(s.mu); }
  static __device__ __forceinline__ V update(V c, V w, V x) { const float p = w * x; return c + p; }
  static __device__ __forceinline__ V energy(V en, V x0, V x) {
    const float a = x0 * x0, b = x * x;
    en = en - a;
    return en + b;
  }
  static __device__ __forceinline__ V norm_weight(V e, V en, const LmsScalars& s, const int16_t*) {
    const float num = e * __int_as_float(s.mu), den = en + 0.000000119209289f;
    return __fdiv_rn(num, den);
  }
};
template <> struct LmsT<kLmsQ31> {
  using T = int32_t; using V = int32_t; using A = uint64_t;
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return v; }
  static __device__ __forceinline__ A mac(A acc, V x, V c) { return acc + (uint64_t)((int64_t)x * c); }
  static __device__ __forceinline__ V result(A acc, const LmsScalars& s) {
    const int us = s.post_shift + 1;
    return recombine(acc, 32 - us, us);
  }
  static __device__ __forceinline__ V error(V ref, V out) { return wsub(ref, out); }
  static __device__ __forceinline__ V weight(V e, const LmsScalars& s) { return (int32_t)(((int64_t)e * s.mu) >> 31); }
  static __device__ __forceinline__ V update(V c, V w, V x) {
    return clip_q63_q31((int64_t)c + wshl((int32_t)(((int64_t)w * x) >> 32), 1));
  }
  static __device__ __forceinline__ V energy(V en, V, V) { return en; }
  static __device__ __forceinline__ V norm_weight(V, V, const LmsScalars&, const int16_t*) { return 0; }
};
template <> struct LmsT<kLmsQ15> {
  using T = int16_t; using V = int32_t; using A = uint64_t;
  static __device__ __forceinline__ V in(T v) { return v; }
  static __device__ __forceinline__ T out(V v) { return (T)v; }
  static __device__ __forceinline__ A mac(A acc, V x, V c) { return acc + (uint64_t)(int64_t)(x * c); }
  static __device__ __forceinline__ V result(A acc, const LmsScalars& s) {
    const int ls = 15 - s.post_shift;
    return ssat16(recombine(acc, ls, 32 - ls));
  }
  static __device__ __forceinline__ V error(V ref, V out) { return (int16_t)(ref - out); }
  static __device__ __forceinline__ V weight(V e, const LmsScalars& s) { return (int16_t)((e * s.mu) >> 15); }
  static __device__ __forceinline__ V update(V c, V w, V x) { return ssat16(c + ((w * x) >> 15)); }
  static __device__ __forceinline__ V energy(V en, V x0, V x) {
    en -= (x0 * x0) >> 15;
    en += (x * x) >> 15;
    return ssat16(en);
  }
  static __device__ __forceinline__ V norm_weight(V e, V en, const LmsScalars& s, const int16_t* __restrict__ table) {
    int32_t one_by_energy;
    const int ps = (int16_t)recip_q15((int16_t)(en + 5), &one_by_energy, table);
    const int32_t emu = (int16_t)((e * s.mu) >> 15);
    return ssat16((emu * one_by_energy) >> ((15 - ps) & 31));
  }
};

constexpr int kLmsTS = MI355X_LMS_TS;      // samples per tile row
constexpr int kLmsPitch = kLmsTS + 1;
constexpr int kLmsReg = MI355X_LMS_REG;    // taps with coefficients and window in registers
constexpr int kLmsLds = MI355X_LMS_LDS;    // taps with coefficients and ring in LDS

// LDS: coefficients and ring in LDS as [tap][lane]; otherwise d_coeffs in place and the ring in `ws`
// ([batch][T] words).  The ring holds the window: slot `head` is w[0], the sample before it in ring
// order is the newest.
template <int OP, bool NORM, bool LDS>
__global__ __launch_bounds__(64) void lms_kernel(const typename LmsT<OP>::T* src, const typename LmsT<OP>::T* ref,
                                                 typename LmsT<OP>::T* outp, typename LmsT<OP>::T* errp,
                                                 typename LmsT<OP>::T* coeffs, typename LmsT<OP>::T* state,
                                                 typename LmsT<OP>::T* ex, typename LmsT<OP>::T* ws,
                                                 const int16_t* __restrict__ recip, uint32_t batch, uint32_t B, int T_,
                                                 LmsScalars sc) {
  using Op = LmsT<OP>;
  using T = typename Op::T;
  using V = typename Op::V;
  using A = typename Op::A;
  extern __shared__ int32_t lms_smem[];
  V* tx = (V*)lms_smem;                            // src, then out: [64][kLmsPitch]
  V* td = tx + 64 * kLmsPitch;                     // ref, then err
  V* cl = td + 64 * kLmsPitch;                     // [T][64] (LDS)
  V* rl = cl + 64 * T_;                            // [T][64] (LDS)
  const int lane = threadIdx.x;
  const int NT = T_, H = NT - 1;
  const uint64_t f0 = (uint64_t)blockIdx.x * 64, f = f0 + lane;
  const bool live = f < batch;
  const uint32_t rows = (uint32_t)min((uint64_t)64, batch - f0);
  T* cg = coeffs + f * (uint64_t)NT;               // this lane's words (dereferenced when live)
  T* rg = ws + f * (uint64_t)NT;

  auto ldc = [&](int i) -> V { if constexpr (LDS) return cl[i * 64 + lane]; else return Op::in(cg[i]); };
  auto stc = [&](int i, V v) { if constexpr (LDS) cl[i * 64 + lane] = v; else cg[i] = Op::out(v); };
  auto ldr = [&](int i) -> V { if constexpr (LDS) return rl[i * 64 + lane]; else return Op::in(rg[i]); };
  auto str = [&](int i, V v) { if constexpr (LDS) rl[i * 64 + lane] = v; else rg[i] = Op::out(v); };

  if constexpr (LDS) {                             // coalesced: element e of the wave's rows x T (T - 1) words
    const T* c0 = coeffs + f0 * (uint64_t)NT;
    for (uint32_t e = lane; e < rows * (uint32_t)NT; e += 64) cl[(e % NT) * 64 + e / NT] = Op::in(c0[e]);
    if (H > 0) {
      const T* s0 = state + f0 * (uint64_t)H;
      for (uint32_t e = lane; e < rows * (uint32_t)H; e += 64) rl[(e % H) * 64 + e / H] = Op::in(s0[e]);
    }
  } else if (live) {
    const T* s0 = state + f * (uint64_t)H;
    for (int i = 0; i < H; ++i) rg[i] = s0[i];
  }
  V energy = 0, x0 = 0;
  if (NORM && live) { energy = Op::in(ex[2 * f]); x0 = Op::in(ex[2 * f + 1]); }
  __syncthreads();
  int head = 0;                                    // slot of w[0]; the free slot is the one before it

  for (uint32_t n0 = 0; n0 < B; n0 += kLmsTS) {
    const uint32_t cnt = min((uint32_t)kLmsTS, B - n0);
#pragma unroll 4
    for (int i = 0; i < kLmsTS; ++i) {
      const uint32_t e = i * 64 + lane, row = e / kLmsTS, col = e % kLmsTS;
      const bool ok = row < rows && col < cnt;
      const uint64_t at = (f0 + row) * B + n0 + col;
      tx[row * kLmsPitch + col] = ok ? Op::in(src[at]) : (V)0;
      td[row * kLmsPitch + col] = ok ? Op::in(ref[at]) : (V)0;
    }
    __syncthreads();
    if (live) {
      V* mx = tx + lane * kLmsPitch;
      V* md = td + lane * kLmsPitch;
      for (uint32_t c = 0; c < cnt; ++c) {
        const V x = mx[c];
        const int w = head == 0 ? H : head - 1;    // free slot: takes the new sample
        str(w, x);
        if constexpr (NORM) energy = Op::energy(energy, x0, x);
        A acc = 0;
        int ci = 0;
#pragma unroll 4
        for (int r = head; r < NT; ++r, ++ci) acc = Op::mac(acc, ldr(r), ldc(ci));
#pragma unroll 4
        for (int r = 0; r < head; ++r, ++ci) acc = Op::mac(acc, ldr(r), ldc(ci));
        const V y = Op::result(acc, sc);
        const V e = Op::error(md[c], y);
        mx[c] = y;
        md[c] = e;
        V wt;
        if constexpr (NORM) wt = Op::norm_weight(e, energy, sc, recip);
        else wt = Op::weight(e, sc);
        ci = 0;
#pragma unroll 4
        for (int r = head; r < NT; ++r, ++ci) stc(ci, Op::update(ldc(ci), wt, ldr(r)));
#pragma unroll 4
        for (int r = 0; r < head; ++r, ++ci) stc(ci, Op::update(ldc(ci), wt, ldr(r)));
        if constexpr (NORM) x0 = ldr(head);
        head = head + 1 == NT ? 0 : head + 1;
      }
    } else {
      for (uint32_t c = 0; c < cnt; ++c) head = head + 1 == NT ? 0 : head + 1;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < kLmsTS; ++i) {
      const uint32_t e = i * 64 + lane, row = e / kLmsTS, col = e % kLmsTS;
      if (row < rows && col < cnt) {
        const uint64_t at = (f0 + row) * B + n0 + col;
        outp[at] = Op::out(tx[row * kLmsPitch + col]);
        errp[at] = Op::out(td[row * kLmsPitch + col]);
      }
    }
    __syncthreads();
  }

  // the new state: w[0..T-2] of the next sample's window, i.e. ring order from `head`
  if (NORM && live) { ex[2 * f] = Op::out(energy); ex[2 * f + 1] = Op::out(x0); }
  if constexpr (LDS) {
    T* c0 = coeffs + f0 * (uint64_t)NT;
    for (uint32_t e = lane; e < rows * (uint32_t)NT; e += 64) c0[e] = Op::out(cl[(e % NT) * 64 + e / NT]);
    if (H > 0) {
      T* s0 = state + f0 * (uint64_t)H;
      for (uint32_t e = lane; e < rows * (uint32_t)H; e += 64) {
        int r = head + (int)(e % H);
        r = r >= NT ? r - NT : r;
        s0[e] = Op::out(rl[r * 64 + e / H]);
      }
    }
  } else if (live) {
    T* s0 = state + f * (uint64_t)H;
    for (int i = 0; i < H; ++i) {
      int r = head + i;
      r = r >= NT ? r - NT : r;
      s0[i] = rg[r];
    }
  }
}

// Register tier, T <= NR: coefficients and window in the lane's registers, the T real taps in slots
// NR - T .. NR - 1 (slot NR - 1 takes the new sample; the window moves down one slot per sample, a
// v_mov per tap where the ring costs LDS traffic).  EXACT: T == NR, the tap loops have no guards.
template <int OP, bool NORM, int NR, bool EXACT>
__global__ __launch_bounds__(64) void lms_reg_kernel(const typename LmsT<OP>::T* src, const typename LmsT<OP>::T* ref,
                                                     typename LmsT<OP>::T* outp, typename LmsT<OP>::T* errp,
                                                     typename LmsT<OP>::T* coeffs, typename LmsT<OP>::T* state,
                                                     typename LmsT<OP>::T* ex, const int16_t* __restrict__ recip,
                                                     uint32_t batch, uint32_t B, int T_, LmsScalars sc) {
  using Op = LmsT<OP>;
  using T = typename Op::T;
  using V = typename Op::V;
  using A = typename Op::A;
  extern __shared__ int32_t lms_smem[];
  V* tx = (V*)lms_smem;                            // src, then out: [64][kLmsPitch]
  V* td = tx + 64 * kLmsPitch;                     // ref, then err
  const int lane = threadIdx.x;
  const int NT = EXACT ? NR : T_, P = NR - NT;     // first real slot
  const uint64_t f0 = (uint64_t)blockIdx.x * 64, f = f0 + lane;
  const bool live = f < batch;
  const uint32_t rows = (uint32_t)min((uint64_t)64, batch - f0);
  T* cg = coeffs + f * (uint64_t)NT;               // this lane's words (dereferenced when live)
  T* sg = state + f * (uint64_t)(NT - 1);
  V c[NR], h[NR];
#pragma unroll
  for (int s = 0; s < NR; ++s) {
    c[s] = (live && s >= P) ? Op::in(cg[s - P]) : (V)0;
    h[s] = (live && s >= P && s < NR - 1) ? Op::in(sg[s - P]) : (V)0;
  }
  V energy = 0, x0 = 0;
  if (NORM && live) { energy = Op::in(ex[2 * f]); x0 = Op::in(ex[2 * f + 1]); }

  V xr[kLmsTS], dr[kLmsTS];                        // one tile ahead, in flight under the previous tile's taps
  auto fetch = [&](uint32_t n0) {
#pragma unroll
    for (int i = 0; i < kLmsTS; ++i) {
      const uint32_t e = i * 64 + lane, row = e / kLmsTS, col = e % kLmsTS;
      const bool ok = row < rows && n0 + col < B;
      const uint64_t at = (f0 + row) * B + n0 + col;
      xr[i] = ok ? Op::in(src[at]) : (V)0;
      dr[i] = ok ? Op::in(ref[at]) : (V)0;
    }
  };
  fetch(0);
  for (uint32_t n0 = 0; n0 < B; n0 += kLmsTS) {
    const uint32_t cnt = min((uint32_t)kLmsTS, B - n0);
#pragma unroll
    for (int i = 0; i < kLmsTS; ++i) {
      const uint32_t e = i * 64 + lane, at = (e / kLmsTS) * kLmsPitch + e % kLmsTS;
      tx[at] = xr[i];
      td[at] = dr[i];
    }
    __syncthreads();
    if (n0 + kLmsTS < B) fetch(n0 + kLmsTS);
    if (live) {
      V* mx = tx + lane * kLmsPitch;
      V* md = td + lane * kLmsPitch;
      for (uint32_t n = 0; n < cnt; ++n) {
        const V x = mx[n];
        h[NR - 1] = x;
        if constexpr (NORM) energy = Op::energy(energy, x0, x);
        A acc = 0;
#pragma unroll
        for (int s = 0; s < NR; ++s)
          if (EXACT || s >= P) acc = Op::mac(acc, h[s], c[s]);
        const V y = Op::result(acc, sc);
        const V e = Op::error(md[n], y);
        mx[n] = y;
        md[n] = e;
        V wt;
        if constexpr (NORM) wt = Op::norm_weight(e, energy, sc, recip);
        else wt = Op::weight(e, sc);
#pragma unroll
        for (int s = 0; s < NR; ++s) {
          if (EXACT || s >= P) c[s] = Op::update(c[s], wt, h[s]);
          if (NORM && (EXACT ? s == 0 : s == P)) x0 = h[s];
        }
#pragma unroll
        for (int s = 0; s < NR - 1; ++s) h[s] = h[s + 1];
      }
    }
    __syncthreads();
    V yr[kLmsTS], er[kLmsTS];
#pragma unroll
    for (int i = 0; i < kLmsTS; ++i) {
      const uint32_t e = i * 64 + lane, at = (e / kLmsTS) * kLmsPitch + e % kLmsTS;
      yr[i] = tx[at];
      er[i] = td[at];
    }
#pragma unroll
    for (int i = 0; i < kLmsTS; ++i) {
      const uint32_t e = i * 64 + lane, row = e / kLmsTS, col = e % kLmsTS;
      if (row < rows && col < cnt) {
        const uint64_t at = (f0 + row) * B + n0 + col;
        outp[at] = Op::out(yr[i]);
        errp[at] = Op::out(er[i]);
      }
    }
    __syncthreads();
  }
  if (live) {
    if (NORM) { ex[2 * f] = Op::out(energy); ex[2 * f + 1] = Op::out(x0); }
#pragma unroll
    for (int s = 0; s < NR; ++s) {
      if (s >= P) cg[s - P] = Op::out(c[s]);
      if (s >= P && s < NR - 1) sg[s - P] = Op::out(h[s]);
    }
  }
}

template <int OP, bool NORM>
hipError_t lms_launch(const void* src, const void* ref, void* out, void* err, uint32_t B, uint32_t batch, int taps,
                      void* coeffs, void* state, void* ex, int32_t mu, int32_t post_shift, const int16_t* recip,
                      hipStream_t st) {
  using T = typename LmsT<OP>::T;
  if (batch == 0 || B == 0) return hipSuccess;
  if (taps < 1 || !src || !ref || !out || !err || !coeffs || (taps > 1 && !state) || (NORM && !ex))
    return hipErrorInvalidValue;
  if (NORM && OP == kLmsQ15 && !recip) return hipErrorInvalidValue;
  const dim3 grid((batch + 63) / 64), block(64);
  const size_t base = sizeof(int32_t) * 2 * 64 * kLmsPitch;
  const LmsScalars sc{mu, post_shift};
#define MI355X_LMS_TIER(NR)                                                                                       \
  do {                                                                                                           \
    if (taps == NR)                                                                                              \
      hipLaunchKernelGGL((lms_reg_kernel<OP, NORM, NR, true>), grid, block, base, st, (const T*)src, (const T*)ref, \
                         (T*)out, (T*)err, (T*)coeffs, (T*)state, (T*)ex, recip, batch, B, taps, sc);            \
    else                                                                                                         \
      hipLaunchKernelGGL((lms_reg_kernel<OP, NORM, NR, false>), grid, block, base, st, (const T*)src, (const T*)ref, \
                         (T*)out, (T*)err, (T*)coeffs, (T*)state, (T*)ex, recip, batch, B, taps, sc);            \
    return hipGetLastError();                                                                                    \
  } while (0)
  if (taps <= 4) MI355X_LMS_TIER(4);
  if (taps <= 8) MI355X_LMS_TIER(8);
  if (taps <= 16) MI355X_LMS_TIER(16);
  if (taps <= kLmsReg) MI355X_LMS_TIER(kLmsReg);
#undef MI355X_LMS_TIER
  if (taps <= kLmsLds) {
    hipLaunchKernelGGL((lms_kernel<OP, NORM, true>), grid, block, base + sizeof(int32_t) * 2 * 64 * (size_t)taps, st,
                       (const T*)src, (const T*)ref, (T*)out, (T*)err, (T*)coeffs, (T*)state, (T*)ex, (T*)nullptr, recip,
                       batch, B, taps, sc);
    return hipGetLastError();
  }
  T* ws = nullptr;
  hipError_t e = hipMallocAsync((void**)&ws, sizeof(T) * (size_t)batch * taps, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((lms_kernel<OP, NORM, false>), grid, block, base, st, (const T*)src, (const T*)ref, (T*)out,
                     (T*)err, (T*)coeffs, (T*)state, (T*)ex, ws, recip, batch, B, taps, sc);
  e = hipGetLastError();
  (void)hipFreeAsync(ws, st);
  return e;
}

}  // namespace

hipError_t lms_run(int op, bool norm, const void* src, const void* ref, void* out, void* err, uint32_t block_size,
                   uint32_t batch, int num_taps, void* coeffs, void* state, void* energy_x0, int32_t mu,
                   int32_t post_shift, const int16_t* recip_table, hipStream_t st) {
#define MI355X_LMS_GO(OP, NORM)                                                                                  \
  return lms_launch<OP, NORM>(src, ref, out, err, block_size, batch, num_taps, coeffs, state, energy_x0, mu, \
                              post_shift, recip_table, st)
  switch (op) {
    case kLmsF32: if (norm) MI355X_LMS_GO(kLmsF32, true); else MI355X_LMS_GO(kLmsF32, false);
    case kLmsQ31: if (norm) return hipErrorInvalidValue; else MI355X_LMS_GO(kLmsQ31, false);
    case kLmsQ15: if (norm) MI355X_LMS_GO(kLmsQ15, true); else MI355X_LMS_GO(kLmsQ15, false);
    default: return hipErrorInvalidValue;
  }
#undef MI355X_LMS_GO
}

}  // namespace mi355x
