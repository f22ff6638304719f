// expf as the reference's host build computes it: glibc 2.35's expf (the table-driven algorithm of
// sysdeps/ieee754/flt-32/e_expf.c, Arm optimized-routines; x86-64 selects the FMA-compiled instance on CPUs with
// FMA/AVX2, which this restates operation for operation).  The reference calls it from arm_vexp_f32.c,
// arm_logsumexp_f32.c and arm_svm_rbf_predict_f32.c.
//
// Algorithm: x = (k / 32) ln2 + r' with k an integer; exp(x) = 2^(k / 32) * exp(r'), the first factor from a table of
// 32 doubles (T[i] = bits(2^(i / 32)) - (i << 47), so that adding k << 47 puts k / 32 into the exponent field), the
// second a cubic in r = 32 x / ln2 - k.  r is one fma of InvLn2N, x and -kd: the compiler contracts the source's
// "z - kd" with z = InvLn2N * x into it, and the separately rounded difference is one ulp off on 2 of the 2^32
// inputs.
// Constants: the pinned glibc's __exp2f_data (tab[32], shift, invln2_scaled, poly_scaled[3]), read from the installed
// libm or computed by tools/expf_table.py; tools/expf_check.cpp proves this restatement equal to the host expf on all
// 2^32 inputs (NaN payloads aside).
#pragma once
#include <stdint.h>

// Also compiled on the host by tools/expf_check.cpp (g++), which checks this exact source.
#ifdef __HIPCC__
#define MI355X_EXPF_FN __device__ __forceinline__
#define MI355X_EXPF_TAB static __constant__ const
#else
#define MI355X_EXPF_FN static inline
#define MI355X_EXPF_TAB static const
#endif

namespace mi355x {

MI355X_EXPF_TAB uint64_t kHostExpfTab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};

MI355X_EXPF_FN float host_expf(float x) {
  constexpr double kInvLn2N = 0x1.71547652b82fep+0 * 32.0, kShift = 0x1.8p+52;
  constexpr double C0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0, C1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0,
                   C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
  const uint32_t abstop = (__builtin_bit_cast(uint32_t, x) >> 20) & 0x7ffu;
  if (abstop >= 0x42bu) {                                     // |x| >= 88 or x is NaN
    if (__builtin_bit_cast(uint32_t, x) == 0xff800000u) return 0.0f;
    if (abstop >= 0x7f8u) return x + x;
    if (x > 0x1.62e42ep6f) return __builtin_inff();           // overflow
    if (x < -0x1.9fe368p6f) return 0.0f;                      // underflow
    if (x < -0x1.9d1d9ep6f) return 0x1p-149f;                 // may underflow
  }
  const double xd = (double)x;
  const double z = kInvLn2N * xd;
  double kd = z + kShift;                                     // round to the nearest integer, in the low bits
  const uint64_t ki = __builtin_bit_cast(uint64_t, kd);
  kd -= kShift;
  const double r = __builtin_fma(kInvLn2N, xd, -kd);
  const uint64_t t = kHostExpfTab[ki % 32u] + (ki << 47);
  const double s = __builtin_bit_cast(double, t);
  const double zz = __builtin_fma(C0, r, C1);
  const double r2 = r * r;
  const double y = __builtin_fma(C2, r, 1.0);
  return (float)(__builtin_fma(zz, r2, y) * s);
}

}  // namespace mi355x
