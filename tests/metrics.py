"""The reference test framework's acceptance checks (Testing/FrameworkSource/Error.cpp:515-705,
Testing/FrameworkInclude/Error.h:165-179), restated for numpy."""
import numpy as np


def snr_db(ref, out):
    """ASSERT_SNR: 10*log10(sum ref^2 / sum (ref-out)^2), computed in double."""
    ref = np.asarray(ref, dtype=np.float64)
    err = ref - np.asarray(out, dtype=np.float64)
    e = np.sum(err * err)
    return np.inf if e == 0 else 10.0 * np.log10(np.sum(ref * ref) / e)


def close_error(out, ref, abs_err, rel_err):
    """ASSERT_CLOSE_ERROR: |out - ref| <= abs + rel*|ref| elementwise."""
    out = np.asarray(out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(out - ref) <= abs_err + rel_err * np.abs(ref)))


def rel_error(out, ref, rel_err):
    """ASSERT_REL_ERROR: |out - ref| <= rel*|ref| (where ref != 0)."""
    out = np.asarray(out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    nz = ref != 0
    return bool(np.all(np.abs(out[nz] - ref[nz]) <= rel_err * np.abs(ref[nz])))


def near_eq(out, ref, abs_err):
    """ASSERT_NEAR_EQ on integer words."""
    return int(np.max(np.abs(np.asarray(out, np.int64) - np.asarray(ref, np.int64)))) <= abs_err


def relative_error(out, ref, rel_err):
    """ASSERT_REL_ERROR as Error.cpp:217-235 computes it: |a - b| / ((|a| + |b|) / 2) <= rel wherever the mean
    magnitude is not zero (rel_error above bounds the same difference by rel * |ref|; the replayed suites ask both)."""
    out = np.asarray(out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    mean = (np.abs(out) + np.abs(ref)) / 2.0
    nz = mean != 0
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.abs(out[nz] - ref[nz]) / mean[nz] <= rel_err))


def equal(out, ref):
    """ASSERT_EQ (Error.h:165, Error.cpp assert_equal): the same length and every word equal."""
    out, ref = np.asarray(out), np.asarray(ref)
    return out.shape == ref.shape and bool(np.all(out == ref))


def snr_passes(ref, out, threshold):
    """ASSERT_SNR as arm_snr_* decide it (Error.cpp:515-705): a NaN operand or a NaN ratio (0 / 0) fails, no error
    energy at all passes, otherwise snr_db (in double) >= threshold."""
    ref = np.asarray(ref, dtype=np.float64)
    out = np.asarray(out, dtype=np.float64)
    if np.isnan(ref).any() or np.isnan(out).any() or not np.any(ref):
        return False
    return bool(snr_db(ref, out) >= threshold)


# Per-suite thresholds of the reference tests (Testing/Source/Tests/*.cpp)
CFFT_TOL = {"f32": dict(snr=120, abs=8e-5, rel=2e-5),     # TransformCF32.cpp:6-8
            "q31": dict(snr=90, abs=53),                   # TransformCQ31.cpp:6-7
            "q15": dict(snr=30, abs=15)}                   # TransformCQ15.cpp:6-7
FIR_TOL = {"f32": dict(snr=120, rel=3e-5),                 # FIRF32.cpp:5,13
           "q31": dict(snr=100, abs=2),                    # FIRQ31.cpp:5-7
           "q15": dict(snr=59, abs=2),                     # FIRQ15.cpp:5-7
           "q7": dict(snr=10, abs=2)}                      # FIRQ7.cpp:5-7
# DECIM F32 / Q31 / Q15: the decimators and the interpolators share each suite's pair
DECIM_TOL = {"f32": dict(snr=120, rel=8.0e-4),             # DECIMF32.cpp:5,13
             "q31": dict(snr=100, abs=2),                  # DECIMQ31.cpp:5,13
             "q15": dict(snr=70, abs=5)}                   # DECIMQ15.cpp:5,13
# MISC F32 / Q31 / Q15 / Q7: arm_conv_* / arm_correlate_* / arm_conv_partial_*; the fast and opt forms of the partial
# convolution have ABS_ERROR_FAST_<type>
MISC_TOL = {"f32": dict(snr=120, abs=1.0e-5, rel=1.0e-6),  # MISCF32.cpp:8,15-16
            "q31": dict(snr=100, abs=2, abs_fast=11),      # MISCQ31.cpp:8,15-17
            "q15": dict(snr=65, abs=10, abs_fast=20),      # MISCQ15.cpp:8,15-17
            "q7": dict(snr=15, abs=5, abs_fast=5)}         # MISCQ7.cpp:8,15-16
# TransformR F32 / Q31 / Q15.  Q31 asserts no SNR and has a bound of its own for the inverse of 4096 samples
# (scaling == 12); Q15's inverse has its own pair
RFFT_TOL = {"f32": dict(snr=120, abs=5.0e-5, rel=1.0e-5),                                    # TransformRF32.cpp:7-9
            "q31": dict(abs=33, abs_ifft=52000, abs_ifft_long=209000),                       # TransformRQ31.cpp:8-10,90
            "q15": dict(snr=40, snr_ifft=25, abs=14, abs_ifft=1250)}                         # TransformRQ15.cpp:7-11
# MFCC F32 / Q31 / Q15
MFCC_TOL = {"f32": dict(snr=115, abs=1.0e-5, rel=1.2e-3),  # MFCCF32.cpp:7,15-16
            "q31": dict(snr=66, abs=49000),                # MFCCQ31.cpp:7,15
            "q15": dict(snr=34, abs=30)}                   # MFCCQ15.cpp:5-6
MAT_TOL = dict(snr=120, abs=1e-5, rel=1e-6)                # BinaryTestsF32.cpp:5,13-17
# Basic Tests F32 / Q31 / Q15 / Q7: SNR_THRESHOLD, REL_ERROR / ABS_ERROR_<type>, the dot products' ABS_ERROR_Q63 (q7:
# ABS_ERROR_Q31), Q15's MULT_SNR_THRESHOLD (mult and dot_prod), Q7's test_mult_short_q7 (SNR_THRESHOLD - 1.0f)
BASIC_TOL = {"f32": dict(snr=120, rel=5.0e-5),                                  # BasicTestsF32.cpp:5,13
             "q31": dict(snr=100, abs=4, abs_dot=1 << 17),                      # BasicTestsQ31.cpp:5,13-14
             "q15": dict(snr=70, snr_mult=60, abs=2, abs_dot=1 << 17),          # BasicTestsQ15.cpp:5,13-16
             "q7": dict(snr=20, snr_mult_short=19, abs=2, abs_dot=1 << 15)}     # BasicTestsQ7.cpp:5-8,94
# Statistics Tests F32 / Q31 / Q15 / Q7: SNR_THRESHOLD, REL_ERROR / ABS_ERROR_<type>; arm_power_*'s wider result
# (ABS_ERROR_Q63, q7: ABS_ERROR_Q31); arm_mse_*'s own pair; Q7's arm_mean_q7 (SNR 5); test_std_stability_f32's
# ASSERT_TRUE(fabs(5.47723f - result) < 1.0e-4f)
STATS_TOL = {"f32": dict(snr=120, rel=1.0e-5, stability=(5.47723, 1.0e-4)),                  # StatsTestsF32.cpp:7,14,351
             "q31": dict(snr=100, abs=100, abs_power=1 << 18, snr_mse=100, abs_mse=100),     # StatsTestsQ31.cpp:8-20
             "q15": dict(snr=50, abs=100, abs_power=1 << 17, snr_mse=50, abs_mse=100),       # StatsTestsQ15.cpp:8-20
             "q7": dict(snr=20, snr_mean=5, abs=20, abs_power=1 << 15, snr_mse=20, abs_mse=6)}   # StatsTestsQ7.cpp:8-20,234
# BIQUAD F32 / Q31 / Q15 (arm_biquad_cas_df1_32x64_q31 has its own pair)
BIQUAD_TOL = {"f32": dict(snr=94, rel=2.0e-4),                                               # BIQUADF32.cpp:5,13
              "q31": dict(snr=115, abs=1000, snr_32x64=140, abs_32x64=25),                   # BIQUADQ31.cpp:6-12
              "q15": dict(snr=30, abs=500)}                                                  # BIQUADQ15.cpp:12-14
# FastMathF32: arm_vlog_f32 / arm_vexp_f32 (SNR_THRESHOLD, ABS_ERROR, REL_ERROR)
FASTMATH_TOL = {"f32": dict(snr=119, abs=1.0e-5, rel=1.0e-6)}                                # FastMathF32.cpp:10,19-20
# ComplexTests F32 / Q31 / Q15: the dot products' wider result (ABS_ERROR_Q63 / ABS_ERROR_Q31), Q15's own pairs for
# arm_cmplx_mag_q15 (SNR_MAG_THRESHOLD, MAG_ERROR_Q15) and arm_cmplx_mag_fast_q15 (SNR_MAG_FAST_THRESHOLD, MAG_FAST_ERROR_Q15)
COMPLEX_TOL = {"f32": dict(snr=120, rel=7.0e-6),                                             # ComplexTestsF32.cpp:5-7
               "q31": dict(snr=100, abs=100, abs_dot_prod=1 << 18),                          # ComplexTestsQ31.cpp:5,13-14
               "q15": dict(snr=60, snr_mag=80, snr_mag_fast=60, abs=5, abs_mag=1, abs_mag_fast=50,
                           abs_dot_prod=550)}                                                # ComplexTestsQ15.cpp:5-19
# BayesF32: ASSERT_REL_ERROR(outputProbas, probas, 5e-6) (the predictions and SVMF32's classes are ASSERT_EQ)
BAYES_TOL = dict(rel=5e-6)                                                                   # BayesF32.cpp:28
# DistanceTestsF32: ASSERT_NEAR_EQ(output, ref, (float32_t)1e-3) in every test; the DTW path is ASSERT_EQ_PARTIAL.
# DistanceTestsU32: ERROR_THRESHOLD 1e-8 (DistanceTestsU32.cpp:6)
DISTANCE_TOL = dict(abs=1e-3, bool=1e-8)                                                                # DistanceTestsF32.cpp:99,120
# BinaryTests F32 / Q31 / Q15 / Q7 (f32: MAT_TOL above); Q15's real products use SNR_LOW_THRESHOLD / ABS_HIGH_ERROR_Q15,
# its complex product MULT_SNR_THRESHOLD / ABS_ERROR_Q15
BINARY_TOL = {"f32": MAT_TOL,
              "q31": dict(snr=100, abs=20),                                                  # BinaryTestsQ31.cpp:5,13
              "q15": dict(snr_low=30, abs_high=2000, snr_mult=60, abs=1000),                 # BinaryTestsQ15.cpp:6-20
              "q7": dict(snr=20, abs=5)}                                                     # BinaryTestsQ7.cpp:6,14
# UnaryTests F32 / Q31 / Q15 / Q7.  F32: SNR_THRESHOLD / ABS_ERROR / REL_ERROR, and the pairs of its own that the
# inverse (_INV), Cholesky (_CHOL) and LDLT (REL_ERROR_LDLT / ABS_ERROR_LDLT, semi-definite: _SPDO / _SDPO) tests use;
# the LDLT tests have no SNR check.  Q7's matrix x vector uses SNR_LOW_THRESHOLD
UNARY_TOL = {"f32": {"default": dict(snr=120, rel=1.0e-5, abs=1.0e-5),                       # UnaryTestsF32.cpp:5,13-14
                     "inverse": dict(snr=99, rel=3.0e-5, abs=2.0e-5),                        # UnaryTestsF32.cpp:43-45
                     "cholesky": dict(snr=92, rel=1.0e-5, abs=5.0e-4),                       # UnaryTestsF32.cpp:52-54
                     "ldlt": dict(rel=1e-5, abs=1e-5),                                       # UnaryTestsF32.cpp:58-59
                     "ldlt_sdpo": dict(rel=1e-5, abs=2e-1)},                                 # UnaryTestsF32.cpp:61-62
             "q31": dict(snr=100, abs=2),                                                    # UnaryTestsQ31.cpp:5,13
             "q15": dict(snr=70, abs=4),                                                     # UnaryTestsQ15.cpp:5,13
             "q7": dict(snr=20, snr_low=11, abs=2)}                                          # UnaryTestsQ7.cpp:5-6,14
# SupportTests F32 / Q31 / Q15 / Q7 (REL_ERROR, ABS_Q15_ERROR, ABS_Q31_ERROR, ABS_Q7_ERROR; Q7's conversions to float
# are ASSERT_CLOSE_ERROR(ref, out, 0.01, REL_ERROR)) and SupportBarTestsF32 (ASSERT_NEAR_EQ 1e-3)
SUPPORT_TOL = {"f32": dict(rel=1.0e-5, abs_q15=10, abs_q31=80, abs_q7=10),                   # SupportTestsF32.cpp:8-11
               "q31": dict(rel=1.0e-5, abs_q15=10, abs_q7=10),                               # SupportTestsQ31.cpp:7-10
               "q15": dict(rel=1.0e-3, abs_q31=40000, abs_q7=10),                            # SupportTestsQ15.cpp:7-10
               "q7": dict(rel=1.0e-5, abs_float=0.01, abs_q15=1 << 8, abs_q31=1 << 24),      # SupportTestsQ7.cpp:7-10,72
               "bar": 1e-3}                                                                  # SupportBarTestsF32.cpp:32
