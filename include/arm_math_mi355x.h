/*
 * arm_math_mi355x.h — additive batched API of the MI355X CMSIS-DSP backend.
 *
 * The drop-in functions of arm_math.h process one transform / block / matrix per call,
 * synchronously.  These entry points are the path that can reach the HBM roofline:
 *   - all data pointers are DEVICE pointers (hipMalloc'd, or managed memory);
 *   - `batch` items are contiguous (stride = one item), processed in one launch;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*, NULL = legacy default
 *     stream) and the call returns without synchronising;
 *   - results are bit-identical to calling the reference scalar function on each item in
 *     turn (f32 CFFT/RFFT/FIR and all fixed-point functions), or within the stated
 *     tolerance (arm_mat_mult_f32_batch and arm_mat_cmplx_mult_f32_batch, MFMA accumulation —
 *     DESIGN.md §mat_mult and "complex matrix multiply");
 *   - return ARM_MATH_SUCCESS, ARM_MATH_ARGUMENT_ERROR (unsupported length, NULL pointer,
 *     launch failure; details in arm_mi355x_last_error_string()).
 * Batch counts: `batch` rides on grid x, which takes 2,147,483,647 workgroups; no entry point has
 * a limit at 65,535 items.  batch == 0 returns ARM_MATH_SUCCESS and writes nothing.  A call whose
 * workgroup count would exceed the limit (matrix multiplies: tiles x batch; beyond K = 32,704
 * ceil(N / 256) x M x batch; convolutions: chunks x batch; the other families at most one per item)
 * launches nothing and returns ARM_MATH_ARGUMENT_ERROR; arm_mi355x_last_error_string() then names the
 * entry point and, for the matrix multiplies, the product ("tiles x batch > 2147483647 workgroups").
 * Instance structs are the reference's own (arm_math.h).  Tables and coefficients they point
 * to: a device pointer is used in place; the library's own CommonTables are uploaded once per
 * device and cached by address; any other host table is cached by CONTENT (hash + compare) in
 * an LRU bounded in bytes (arm_mi355x_set_table_cache_limit), so changing coefficients
 * between calls is always seen and never grows device memory without bound.
 * Multi-GPU: either one process (or host thread) per device, each calling these on its
 * own shard with that device current (the library's caches, scratch and internal streams
 * are per device and per thread), or one call of the *_batch_multi entry points below,
 * which enqueue every shard on its device before waiting for any.
 */
#ifndef ARM_MATH_MI355X_BATCH_H
#define ARM_MATH_MI355X_BATCH_H

#include "arm_math.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Complex FFT over `batch` contiguous transforms of 2*fftLen words each, in place.
 * Per-item semantics: arm_cfft_f32 / _q31 / _q15 (arm_cfft_f32.c:1243, arm_cfft_q31.c:704,
 * arm_cfft_q15.c:671). */
arm_status arm_cfft_f32_batch(const arm_cfft_instance_f32 *S, float32_t *d_p1, uint32_t batch,
                              uint8_t ifftFlag, uint8_t bitReverseFlag, void *stream);
arm_status arm_cfft_q31_batch(const arm_cfft_instance_q31 *S, q31_t *d_p1, uint32_t batch,
                              uint8_t ifftFlag, uint8_t bitReverseFlag, void *stream);
arm_status arm_cfft_q15_batch(const arm_cfft_instance_q15 *S, q15_t *d_p1, uint32_t batch,
                              uint8_t ifftFlag, uint8_t bitReverseFlag, void *stream);

/* Real FFT (fast) over `batch` contiguous signals of fftLenRFFT floats.
 * Per-item semantics: arm_rfft_fast_f32 (arm_rfft_fast_f32.c:675-699), including the
 * reference's overwrite of d_p on the forward transform. */
arm_status arm_rfft_fast_f32_batch(const arm_rfft_fast_instance_f32 *S, float32_t *d_p,
                                   float32_t *d_out, uint32_t batch, uint8_t ifftFlag, void *stream);
/* The same with flags.  ARM_MI355X_RFFT_P_SCRATCH: d_p is scratch, as the reference documents
 * pIn of arm_rfft_fast_f32 ("the input buffer is modified by this function"): the forward
 * transform may leave it with any contents, which lets the batched kernels skip writing the
 * inner CFFT's output back (8 instead of 12 bytes of HBM traffic per real sample).  d_out is
 * bit-identical either way; the inverse never writes d_p.  Other flag bits: ARM_MATH_ARGUMENT_ERROR. */
#define ARM_MI355X_RFFT_P_SCRATCH 1u
arm_status arm_rfft_fast_f32_batch_ex(const arm_rfft_fast_instance_f32 *S, float32_t *d_p,
                                      float32_t *d_out, uint32_t batch, uint8_t ifftFlag, uint32_t flags,
                                      void *stream);

/* Real FFT, q31 / q15, over `batch` signals (per item: arm_rfft_q31 / arm_rfft_q15,
 * arm_rfft_q31.c:148-183).  Forward (S->ifftFlagR != 1): d_src [batch][N] is overwritten
 * by the inner CFFT as in the reference, d_dst [batch][2N] receives the spectra.
 * Inverse: d_src [batch][2N] spectrum rows (words 0 .. N+1 of each row are read; the
 * layout of the forward output), d_dst [batch][N]. */
arm_status arm_rfft_q31_batch(const arm_rfft_instance_q31 *S, q31_t *d_src, q31_t *d_dst, uint32_t batch,
                              void *stream);
arm_status arm_rfft_q15_batch(const arm_rfft_instance_q15 *S, q15_t *d_src, q15_t *d_dst, uint32_t batch,
                              void *stream);

/* MFCC over `batch` contiguous frames of S->fftLen samples (arm_mfcc_f32.c:83-160 per
 * frame).  d_src: [batch][fftLen] input frames (used as work space: overwritten);
 * d_tmp: [batch][fftLen] work space; d_dst: [batch][nbDctOutputs].  The instance's
 * coefficient tables may be host or device pointers (host tables are uploaded on each
 * call through the calling thread's staging buffers, in stream order). */
arm_status arm_mfcc_f32_batch(const arm_mfcc_instance_f32 *S, float32_t *d_src, float32_t *d_dst,
                              float32_t *d_tmp, uint32_t batch, void *stream);
/* MFCC q31 over `batch` contiguous frames (arm_mfcc_q31.c:88-225 per frame, bit-exact):
 * d_src [batch][fftLen] (overwritten), d_tmp [batch][2*fftLen] work, d_dst [batch][nbDct]. */
arm_status arm_mfcc_q31_batch(const arm_mfcc_instance_q31 *S, q31_t *d_src, q31_t *d_dst, q31_t *d_tmp,
                              uint32_t batch, void *stream);
/* MFCC q15 over `batch` contiguous frames (arm_mfcc_q15.c:96-228 per frame, bit-exact):
 * d_src [batch][fftLen] (overwritten), d_tmp [batch][2*fftLen] q15 work, d_dst [batch][nbDct]. */
arm_status arm_mfcc_q15_batch(const arm_mfcc_instance_q15 *S, q15_t *d_src, q15_t *d_dst, q15_t *d_tmp,
                              uint32_t batch, void *stream);

/* FIR over `batch` independent filters sharing S->numTaps / S->pCoeffs (host or device
 * pointer; S->pState is not used).  d_src/d_dst: [batch][blockSize].  d_hist:
 * [batch][numTaps-1] streaming state, read as the history before the block and
 * overwritten with the history after it, so consecutive calls equal one long call
 * (arm_fir_f32.c:1242-1278).  Zero it to start a stream (arm_fir_init_f32). */
arm_status arm_fir_f32_batch(const arm_fir_instance_f32 *S, const float32_t *d_src, float32_t *d_dst,
                             uint32_t blockSize, uint32_t batch, float32_t *d_hist, void *stream);
/* Opt-in TOLERANCE path of arm_fir_f32_batch (same arguments and state contract): every
 * output still sums its taps in the reference's order, but each MAC is one fused multiply-add
 * (v_fma_f32: the product is not rounded before the add), so results differ from the reference
 * in the last bits: |y - y_exact| <= numTaps * 2^-24 * sum_k |x b| (checked against float64 in
 * tests/test_fir_fma.py, with the reference suite's thresholds, FIRF32.cpp).  About twice the
 * bit-exact kernel's throughput (one VALU instruction per MAC instead of two). */
arm_status arm_fir_f32_batch_fma(const arm_fir_instance_f32 *S, const float32_t *d_src, float32_t *d_dst,
                                 uint32_t blockSize, uint32_t batch, float32_t *d_hist, void *stream);
arm_status arm_fir_q15_batch(const arm_fir_instance_q15 *S, const q15_t *d_src, q15_t *d_dst,
                             uint32_t blockSize, uint32_t batch, q15_t *d_hist, void *stream);
arm_status arm_fir_fast_q15_batch(const arm_fir_instance_q15 *S, const q15_t *d_src, q15_t *d_dst,
                                  uint32_t blockSize, uint32_t batch, q15_t *d_hist, void *stream);
arm_status arm_fir_q31_batch(const arm_fir_instance_q31 *S, const q31_t *d_src, q31_t *d_dst,
                             uint32_t blockSize, uint32_t batch, q31_t *d_hist, void *stream);
arm_status arm_fir_fast_q31_batch(const arm_fir_instance_q31 *S, const q31_t *d_src, q31_t *d_dst,
                                  uint32_t blockSize, uint32_t batch, q31_t *d_hist, void *stream);
arm_status arm_fir_q7_batch(const arm_fir_instance_q7 *S, const q7_t *d_src, q7_t *d_dst,
                            uint32_t blockSize, uint32_t batch, q7_t *d_hist, void *stream);

/* Multirate FIR over `batch` independent streams sharing one instance's coefficients (the
 * instance's pState is not used): d_src [batch][blockSize]; decimators write
 * d_dst [batch][blockSize / M] with d_hist [batch][numTaps - 1]; interpolators write
 * d_dst [batch][blockSize * L] with d_hist [batch][phaseLength - 1].  Per-stream semantics:
 * arm_fir_decimate_* / arm_fir_interpolate_*. */
arm_status arm_fir_decimate_f32_batch(const arm_fir_decimate_instance_f32 *S, const float32_t *d_src,
                                      float32_t *d_dst, uint32_t blockSize, uint32_t batch, float32_t *d_hist,
                                      void *stream);
arm_status arm_fir_decimate_q15_batch(const arm_fir_decimate_instance_q15 *S, const q15_t *d_src, q15_t *d_dst,
                                      uint32_t blockSize, uint32_t batch, q15_t *d_hist, void *stream);
arm_status arm_fir_decimate_fast_q15_batch(const arm_fir_decimate_instance_q15 *S, const q15_t *d_src, q15_t *d_dst,
                                           uint32_t blockSize, uint32_t batch, q15_t *d_hist, void *stream);
arm_status arm_fir_decimate_q31_batch(const arm_fir_decimate_instance_q31 *S, const q31_t *d_src, q31_t *d_dst,
                                      uint32_t blockSize, uint32_t batch, q31_t *d_hist, void *stream);
arm_status arm_fir_decimate_fast_q31_batch(const arm_fir_decimate_instance_q31 *S, const q31_t *d_src, q31_t *d_dst,
                                           uint32_t blockSize, uint32_t batch, q31_t *d_hist, void *stream);
arm_status arm_fir_interpolate_f32_batch(const arm_fir_interpolate_instance_f32 *S, const float32_t *d_src,
                                         float32_t *d_dst, uint32_t blockSize, uint32_t batch, float32_t *d_hist,
                                         void *stream);
arm_status arm_fir_interpolate_q15_batch(const arm_fir_interpolate_instance_q15 *S, const q15_t *d_src, q15_t *d_dst,
                                         uint32_t blockSize, uint32_t batch, q15_t *d_hist, void *stream);
arm_status arm_fir_interpolate_q31_batch(const arm_fir_interpolate_instance_q31 *S, const q31_t *d_src, q31_t *d_dst,
                                         uint32_t blockSize, uint32_t batch, q31_t *d_hist, void *stream);

/* Sparse FIR over `batch` independent streams sharing S's taps and delays (host or device
 * arrays): d_src / d_dst [batch][blockSize], d_hist [batch][maxDelay] = each stream's last
 * maxDelay input samples, oldest first (zero-initialise, updated in place; the linear form of
 * the reference's circular state, which the batched call does not use).  Delays outside
 * [0, maxDelay] read zero.  Per-stream semantics: arm_fir_sparse_f32 / _q31 / _q15 / _q7. */
arm_status arm_fir_sparse_f32_batch(const arm_fir_sparse_instance_f32 *S, const float32_t *d_src, float32_t *d_dst,
                                    uint32_t blockSize, uint32_t batch, float32_t *d_hist, void *stream);
arm_status arm_fir_sparse_q31_batch(const arm_fir_sparse_instance_q31 *S, const q31_t *d_src, q31_t *d_dst,
                                    uint32_t blockSize, uint32_t batch, q31_t *d_hist, void *stream);
arm_status arm_fir_sparse_q15_batch(const arm_fir_sparse_instance_q15 *S, const q15_t *d_src, q15_t *d_dst,
                                    uint32_t blockSize, uint32_t batch, q15_t *d_hist, void *stream);
arm_status arm_fir_sparse_q7_batch(const arm_fir_sparse_instance_q7 *S, const q7_t *d_src, q7_t *d_dst,
                                   uint32_t blockSize, uint32_t batch, q7_t *d_hist, void *stream);

/* FIR lattice over `batch` independent streams sharing S's coefficients: d_src / d_dst
 * [batch][blockSize], d_state [batch][numStages] (each stream's state in the reference's
 * layout, zero-initialise; updated in place).  Per-stream semantics: arm_fir_lattice_*. */
arm_status arm_fir_lattice_f32_batch(const arm_fir_lattice_instance_f32 *S, const float32_t *d_src, float32_t *d_dst,
                                     uint32_t blockSize, uint32_t batch, float32_t *d_state, void *stream);
arm_status arm_fir_lattice_q31_batch(const arm_fir_lattice_instance_q31 *S, const q31_t *d_src, q31_t *d_dst,
                                     uint32_t blockSize, uint32_t batch, q31_t *d_state, void *stream);
arm_status arm_fir_lattice_q15_batch(const arm_fir_lattice_instance_q15 *S, const q15_t *d_src, q15_t *d_dst,
                                     uint32_t blockSize, uint32_t batch, q15_t *d_state, void *stream);

/* Biquad cascades over `batch` independent streams sharing S's coefficients (host pointer, content-
 * cached, or device pointer) and postShift: d_src / d_dst [batch][blockSize] (stereo: [batch][2*blockSize]
 * interleaved L,R), d_state [batch][K*numStages] with each stream's state in the reference's own
 * layout (K = 4; DF2T mono 2; 32x64: q63 words), zero-initialise to start a stream; updated in place, so
 * consecutive calls equal one long call.  S->pState is unused.  d_src == d_dst is allowed.
 * numStages == 0 or a NULL pointer: ARM_MATH_ARGUMENT_ERROR; blockSize == 0 or batch == 0: success,
 * nothing touched.  Per-stream semantics: the drop-in functions of arm_math.h. */
arm_status arm_biquad_cascade_df1_f32_batch(const arm_biquad_casd_df1_inst_f32 *S, const float32_t *d_src,
                                            float32_t *d_dst, uint32_t blockSize, uint32_t batch, float32_t *d_state,
                                            void *stream);
arm_status arm_biquad_cascade_df1_q31_batch(const arm_biquad_casd_df1_inst_q31 *S, const q31_t *d_src, q31_t *d_dst,
                                            uint32_t blockSize, uint32_t batch, q31_t *d_state, void *stream);
arm_status arm_biquad_cascade_df1_fast_q31_batch(const arm_biquad_casd_df1_inst_q31 *S, const q31_t *d_src,
                                                 q31_t *d_dst, uint32_t blockSize, uint32_t batch, q31_t *d_state,
                                                 void *stream);
arm_status arm_biquad_cascade_df1_q15_batch(const arm_biquad_casd_df1_inst_q15 *S, const q15_t *d_src, q15_t *d_dst,
                                            uint32_t blockSize, uint32_t batch, q15_t *d_state, void *stream);
arm_status arm_biquad_cascade_df1_fast_q15_batch(const arm_biquad_casd_df1_inst_q15 *S, const q15_t *d_src,
                                                 q15_t *d_dst, uint32_t blockSize, uint32_t batch, q15_t *d_state,
                                                 void *stream);
arm_status arm_biquad_cas_df1_32x64_q31_batch(const arm_biquad_cas_df1_32x64_ins_q31 *S, const q31_t *d_src,
                                              q31_t *d_dst, uint32_t blockSize, uint32_t batch, q63_t *d_state,
                                              void *stream);
arm_status arm_biquad_cascade_df2T_f32_batch(const arm_biquad_cascade_df2T_instance_f32 *S, const float32_t *d_src,
                                             float32_t *d_dst, uint32_t blockSize, uint32_t batch, float32_t *d_state,
                                             void *stream);
arm_status arm_biquad_cascade_stereo_df2T_f32_batch(const arm_biquad_cascade_stereo_df2T_instance_f32 *S,
                                                    const float32_t *d_src, float32_t *d_dst, uint32_t blockSize,
                                                    uint32_t batch, float32_t *d_state, void *stream);

/* IIR lattice over `batch` independent streams sharing S's pkCoeffs / pvCoeffs (host pointers, content-
 * cached, or device pointers): d_src / d_dst [batch][blockSize], d_state [batch][numStages], each
 * stream's live state words as the drop-in leaves them at the head of pState; zero-initialise to start
 * a stream; updated in place, so consecutive calls equal one long call.  S->pState is unused.
 * d_src == d_dst is allowed.  numStages == 0 or a NULL pointer: ARM_MATH_ARGUMENT_ERROR; blockSize == 0
 * or batch == 0: success, nothing touched. */
arm_status arm_iir_lattice_f32_batch(const arm_iir_lattice_instance_f32 *S, const float32_t *d_src, float32_t *d_dst,
                                     uint32_t blockSize, uint32_t batch, float32_t *d_state, void *stream);
arm_status arm_iir_lattice_q31_batch(const arm_iir_lattice_instance_q31 *S, const q31_t *d_src, q31_t *d_dst,
                                     uint32_t blockSize, uint32_t batch, q31_t *d_state, void *stream);
arm_status arm_iir_lattice_q15_batch(const arm_iir_lattice_instance_q15 *S, const q15_t *d_src, q15_t *d_dst,
                                     uint32_t blockSize, uint32_t batch, q15_t *d_state, void *stream);

/* LMS / normalised LMS over `batch` independent adaptive filters: d_src / d_ref / d_out / d_err
 * [batch][blockSize]; d_coeffs [batch][numTaps], each stream's own taps (time-reversed), read and
 * updated; d_state [batch][numTaps - 1], the previous samples, oldest first (may be NULL when
 * numTaps == 1), updated; normalised: d_energy_x0 [batch][2] words {energy, x0}, updated.  numTaps, mu
 * and postShift come from S (the q15 normalised kind reads S->recipTable, NULL = armRecipTableQ15);
 * S->pCoeffs, S->pState, S->energy and S->x0 are unused.  d_out == d_src and d_err == d_ref are allowed.
 * numTaps == 0, a NULL pointer or a postShift outside the reference's defined range:
 * ARM_MATH_ARGUMENT_ERROR; blockSize == 0 or batch == 0: success, nothing touched. */
arm_status arm_lms_f32_batch(const arm_lms_instance_f32 *S, const float32_t *d_src, const float32_t *d_ref,
                             float32_t *d_out, float32_t *d_err, uint32_t blockSize, uint32_t batch,
                             float32_t *d_coeffs, float32_t *d_state, void *stream);
arm_status arm_lms_q31_batch(const arm_lms_instance_q31 *S, const q31_t *d_src, const q31_t *d_ref, q31_t *d_out,
                             q31_t *d_err, uint32_t blockSize, uint32_t batch, q31_t *d_coeffs, q31_t *d_state,
                             void *stream);
arm_status arm_lms_q15_batch(const arm_lms_instance_q15 *S, const q15_t *d_src, const q15_t *d_ref, q15_t *d_out,
                             q15_t *d_err, uint32_t blockSize, uint32_t batch, q15_t *d_coeffs, q15_t *d_state,
                             void *stream);
arm_status arm_lms_norm_f32_batch(const arm_lms_norm_instance_f32 *S, const float32_t *d_src, const float32_t *d_ref,
                                  float32_t *d_out, float32_t *d_err, uint32_t blockSize, uint32_t batch,
                                  float32_t *d_coeffs, float32_t *d_state, float32_t *d_energy_x0, void *stream);
arm_status arm_lms_norm_q15_batch(const arm_lms_norm_instance_q15 *S, const q15_t *d_src, const q15_t *d_ref,
                                  q15_t *d_out, q15_t *d_err, uint32_t blockSize, uint32_t batch, q15_t *d_coeffs,
                                  q15_t *d_state, q15_t *d_energy_x0, void *stream);

/* Convolution of `batch` pairs: item i convolves d_a + i*strideA (srcALen samples) with
 * d_b + i*strideB (srcBLen samples; strideB = 0 shares one kernel) into
 * d_dst + i*(srcALen + srcBLen - 1).  Per-item semantics: arm_conv_f32 / _q15 / _q31. */
arm_status arm_conv_f32_batch(const float32_t *d_a, uint32_t srcALen, uint32_t strideA, const float32_t *d_b,
                              uint32_t srcBLen, uint32_t strideB, float32_t *d_dst, uint32_t batch, void *stream);
arm_status arm_conv_q15_batch(const q15_t *d_a, uint32_t srcALen, uint32_t strideA, const q15_t *d_b,
                              uint32_t srcBLen, uint32_t strideB, q15_t *d_dst, uint32_t batch, void *stream);
arm_status arm_conv_q31_batch(const q31_t *d_a, uint32_t srcALen, uint32_t strideA, const q31_t *d_b,
                              uint32_t srcBLen, uint32_t strideB, q31_t *d_dst, uint32_t batch, void *stream);
arm_status arm_conv_fast_q15_batch(const q15_t *d_a, uint32_t srcALen, uint32_t strideA, const q15_t *d_b,
                                   uint32_t srcBLen, uint32_t strideB, q15_t *d_dst, uint32_t batch, void *stream);
arm_status arm_conv_fast_q31_batch(const q31_t *d_a, uint32_t srcALen, uint32_t strideA, const q31_t *d_b,
                                   uint32_t srcBLen, uint32_t strideB, q31_t *d_dst, uint32_t batch, void *stream);
arm_status arm_conv_q7_batch(const q7_t *d_a, uint32_t srcALen, uint32_t strideA, const q7_t *d_b,
                             uint32_t srcBLen, uint32_t strideB, q7_t *d_dst, uint32_t batch, void *stream);

/* Partial convolution of `batch` pairs (strides as arm_conv_*_batch): item i's numPoints
 * outputs firstIndex .. firstIndex + numPoints - 1 go COMPACTLY to d_dst + i*numPoints.
 * ARM_MATH_ARGUMENT_ERROR when firstIndex + numPoints > srcALen + srcBLen - 1. */
arm_status arm_conv_partial_f32_batch(const float32_t *d_a, uint32_t srcALen, uint32_t strideA,
                                      const float32_t *d_b, uint32_t srcBLen, uint32_t strideB, float32_t *d_dst,
                                      uint32_t firstIndex, uint32_t numPoints, uint32_t batch, void *stream);
arm_status arm_conv_partial_q15_batch(const q15_t *d_a, uint32_t srcALen, uint32_t strideA, const q15_t *d_b,
                                      uint32_t srcBLen, uint32_t strideB, q15_t *d_dst, uint32_t firstIndex,
                                      uint32_t numPoints, uint32_t batch, void *stream);
arm_status arm_conv_partial_q31_batch(const q31_t *d_a, uint32_t srcALen, uint32_t strideA, const q31_t *d_b,
                                      uint32_t srcBLen, uint32_t strideB, q31_t *d_dst, uint32_t firstIndex,
                                      uint32_t numPoints, uint32_t batch, void *stream);
arm_status arm_conv_partial_fast_q15_batch(const q15_t *d_a, uint32_t srcALen, uint32_t strideA, const q15_t *d_b,
                                           uint32_t srcBLen, uint32_t strideB, q15_t *d_dst, uint32_t firstIndex,
                                           uint32_t numPoints, uint32_t batch, void *stream);
arm_status arm_conv_partial_fast_q31_batch(const q31_t *d_a, uint32_t srcALen, uint32_t strideA, const q31_t *d_b,
                                           uint32_t srcBLen, uint32_t strideB, q31_t *d_dst, uint32_t firstIndex,
                                           uint32_t numPoints, uint32_t batch, void *stream);
arm_status arm_conv_partial_q7_batch(const q7_t *d_a, uint32_t srcALen, uint32_t strideA, const q7_t *d_b,
                                     uint32_t srcBLen, uint32_t strideB, q7_t *d_dst, uint32_t firstIndex,
                                     uint32_t numPoints, uint32_t batch, void *stream);

/* Correlation of `batch` pairs: item i writes d_dst + i*(2*max(srcALen, srcBLen) - 1) at the
 * positions arm_correlate_* writes (the others are left untouched). */
arm_status arm_correlate_f32_batch(const float32_t *d_a, uint32_t srcALen, uint32_t strideA, const float32_t *d_b,
                                   uint32_t srcBLen, uint32_t strideB, float32_t *d_dst, uint32_t batch,
                                   void *stream);
arm_status arm_correlate_q15_batch(const q15_t *d_a, uint32_t srcALen, uint32_t strideA, const q15_t *d_b,
                                   uint32_t srcBLen, uint32_t strideB, q15_t *d_dst, uint32_t batch, void *stream);
arm_status arm_correlate_q31_batch(const q31_t *d_a, uint32_t srcALen, uint32_t strideA, const q31_t *d_b,
                                   uint32_t srcBLen, uint32_t strideB, q31_t *d_dst, uint32_t batch, void *stream);
arm_status arm_correlate_fast_q15_batch(const q15_t *d_a, uint32_t srcALen, uint32_t strideA, const q15_t *d_b,
                                        uint32_t srcBLen, uint32_t strideB, q15_t *d_dst, uint32_t batch,
                                        void *stream);
arm_status arm_correlate_fast_q31_batch(const q31_t *d_a, uint32_t srcALen, uint32_t strideA, const q31_t *d_b,
                                        uint32_t srcBLen, uint32_t strideB, q31_t *d_dst, uint32_t batch,
                                        void *stream);
arm_status arm_correlate_q7_batch(const q7_t *d_a, uint32_t srcALen, uint32_t strideA, const q7_t *d_b,
                                  uint32_t srcBLen, uint32_t strideB, q7_t *d_dst, uint32_t batch, void *stream);

/* Row-major C[b] = A[b] * B[b] for `batch` contiguous (numRows x numCols) matrices with
 * the shapes of the three instances (their pData must be device pointers to the first
 * item).  Returns ARM_MATH_SIZE_MISMATCH on incompatible shapes (arm_mat_mult_f32.c:618-630). */
arm_status arm_mat_mult_f32_batch(const arm_matrix_instance_f32 *pSrcA, const arm_matrix_instance_f32 *pSrcB,
                                  arm_matrix_instance_f32 *pDst, uint32_t batch, void *stream);
/* q7 / q15 / q31 analogues (bit-exact; q7 on one i8 matrix-core plane, q15 / q31 byte-sliced
 * planes on the i8 matrix cores). */
arm_status arm_mat_mult_q7_batch(const arm_matrix_instance_q7 *pSrcA, const arm_matrix_instance_q7 *pSrcB,
                                 arm_matrix_instance_q7 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_mult_q15_batch(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                                  arm_matrix_instance_q15 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_mult_q31_batch(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                                  arm_matrix_instance_q31 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_mult_fast_q15_batch(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                                       arm_matrix_instance_q15 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_mult_fast_q31_batch(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                                       arm_matrix_instance_q31 *pDst, uint32_t batch, void *stream);
/* Complex analogues (arm_mat_cmplx_mult_f32 / _q31 / _q15 per matrix; numRows / numCols count
 * complex elements, items are contiguous interleaved matrices).  q31 / q15 bit-exact, f32 the
 * stated fmaf chain; no scratch is taken or written. */
arm_status arm_mat_cmplx_mult_f32_batch(const arm_matrix_instance_f32 *pSrcA, const arm_matrix_instance_f32 *pSrcB,
                                        arm_matrix_instance_f32 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_cmplx_mult_q31_batch(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                                        arm_matrix_instance_q31 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_cmplx_mult_q15_batch(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                                        arm_matrix_instance_q15 *pDst, uint32_t batch, void *stream);
/* Inverse, Cholesky, LDLT and triangular solves of `batch` independent items (per item: arm_mat_inverse_f32,
 * arm_mat_cholesky_f32, arm_mat_ldlt_f32, arm_mat_solve_{lower,upper}_triangular_f32, bit-exact).  pData
 * points at the first of `batch` contiguous row-major items of the instance's shape; each item of a solve has
 * its own triangular matrix and right-hand sides; d_pp holds batch rows of n words.  d_status (device, may
 * be NULL) receives one int32 per item: ARM_MATH_SUCCESS, ARM_MATH_SINGULAR or
 * ARM_MATH_DECOMPOSITION_FAILURE; a failing item leaves the words the reference leaves and does not disturb
 * its neighbours.  The return value reports shape, argument and launch errors only.  The inverse destroys
 * pSrc's items; Cholesky's pDst->pData may be pSrc->pData and a solve's dst->pData may be a->pData.
 * batch == 0 and n == 0 are successful no-ops.  There are no _batch_multi forms. */
arm_status arm_mat_inverse_f32_batch(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pDst,
                                     uint32_t batch, int32_t *d_status, void *stream);
arm_status arm_mat_cholesky_f32_batch(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pDst,
                                      uint32_t batch, int32_t *d_status, void *stream);
arm_status arm_mat_solve_lower_triangular_f32_batch(const arm_matrix_instance_f32 *lt,
                                                    const arm_matrix_instance_f32 *a, arm_matrix_instance_f32 *dst,
                                                    uint32_t batch, int32_t *d_status, void *stream);
arm_status arm_mat_solve_upper_triangular_f32_batch(const arm_matrix_instance_f32 *ut,
                                                    const arm_matrix_instance_f32 *a, arm_matrix_instance_f32 *dst,
                                                    uint32_t batch, int32_t *d_status, void *stream);
arm_status arm_mat_ldlt_f32_batch(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pl,
                                  arm_matrix_instance_f32 *pd, uint16_t *d_pp, uint32_t batch, void *stream);
/* Element-wise add, sub and scale, the transposes and matrix x vector over `batch` independent items (per item:
 * arm_mat_add_*, arm_mat_sub_*, arm_mat_scale_*, arm_mat_trans_*, arm_mat_cmplx_trans_*, arm_mat_vec_mult_*,
 * bit-exact).  Every pData is a device pointer to `batch` contiguous row-major items of the instance's shape.
 * Stream-ordered, no host synchronisation.  One scale (and shift) serves the whole batch.  pDst->pData of add /
 * sub / scale may equal a source's pData exactly; no other overlap is defined.  batch == 0 and a zero dimension
 * are successful no-ops; shape, shift and null-pointer errors as for the drop-ins.
 * arm_mat_vec_mult_*_batch: item i multiplies the matrix at pSrcMat->pData + i * matStride (elements) by
 * d_vec[i] (numCols words) into d_dst[i] (numRows words).  matStride == 0: one matrix shared by every item;
 * otherwise matStride >= numRows * numCols, or ARM_MATH_ARGUMENT_ERROR.  The uint16_t row offset that _q15
 * and _q31 keep wraps inside an item; item bases are full-width.  There are no _batch_multi forms. */
#define MI355X_DECL_MAT_EW(SUF, INST)                                                                          \
  arm_status arm_mat_add_##SUF##_batch(const INST *pSrcA, const INST *pSrcB, INST *pDst, uint32_t batch,       \
                                       void *stream);                                                          \
  arm_status arm_mat_sub_##SUF##_batch(const INST *pSrcA, const INST *pSrcB, INST *pDst, uint32_t batch,       \
                                       void *stream);
MI355X_DECL_MAT_EW(f32, arm_matrix_instance_f32)
MI355X_DECL_MAT_EW(q31, arm_matrix_instance_q31)
MI355X_DECL_MAT_EW(q15, arm_matrix_instance_q15)
#undef MI355X_DECL_MAT_EW
arm_status arm_mat_scale_f32_batch(const arm_matrix_instance_f32 *pSrc, float32_t scale,
                                   arm_matrix_instance_f32 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_scale_q31_batch(const arm_matrix_instance_q31 *pSrc, q31_t scaleFract, int32_t shift,
                                   arm_matrix_instance_q31 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_scale_q15_batch(const arm_matrix_instance_q15 *pSrc, q15_t scaleFract, int32_t shift,
                                   arm_matrix_instance_q15 *pDst, uint32_t batch, void *stream);
arm_status arm_mat_trans_f32_batch(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pDst,
                                   uint32_t batch, void *stream);
arm_status arm_mat_trans_q31_batch(const arm_matrix_instance_q31 *pSrc, arm_matrix_instance_q31 *pDst,
                                   uint32_t batch, void *stream);
arm_status arm_mat_trans_q15_batch(const arm_matrix_instance_q15 *pSrc, arm_matrix_instance_q15 *pDst,
                                   uint32_t batch, void *stream);
arm_status arm_mat_trans_q7_batch(const arm_matrix_instance_q7 *pSrc, arm_matrix_instance_q7 *pDst,
                                  uint32_t batch, void *stream);
arm_status arm_mat_cmplx_trans_f32_batch(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pDst,
                                         uint32_t batch, void *stream);
arm_status arm_mat_cmplx_trans_q31_batch(const arm_matrix_instance_q31 *pSrc, arm_matrix_instance_q31 *pDst,
                                         uint32_t batch, void *stream);
arm_status arm_mat_cmplx_trans_q15_batch(const arm_matrix_instance_q15 *pSrc, arm_matrix_instance_q15 *pDst,
                                         uint32_t batch, void *stream);
arm_status arm_mat_vec_mult_f32_batch(const arm_matrix_instance_f32 *pSrcMat, uint32_t matStride,
                                      const float32_t *d_vec, float32_t *d_dst, uint32_t batch, void *stream);
arm_status arm_mat_vec_mult_q31_batch(const arm_matrix_instance_q31 *pSrcMat, uint32_t matStride,
                                      const q31_t *d_vec, q31_t *d_dst, uint32_t batch, void *stream);
arm_status arm_mat_vec_mult_q15_batch(const arm_matrix_instance_q15 *pSrcMat, uint32_t matStride,
                                      const q15_t *d_vec, q15_t *d_dst, uint32_t batch, void *stream);
arm_status arm_mat_vec_mult_q7_batch(const arm_matrix_instance_q7 *pSrcMat, uint32_t matStride,
                                     const q7_t *d_vec, q7_t *d_dst, uint32_t batch, void *stream);
/* Complex math and max / min over `batch` independent items (per item: arm_cmplx_mag_*, _mag_squared_*, _conj_*,
 * _mult_cmplx_*, _mult_real_*, _dot_prod_*, arm_max_*, arm_min_*, bit-exact).  Every pointer is a device pointer
 * to `batch` contiguous items: numSamples complex samples (interleaved re, im) per item, one word per sample in the
 * real vector of mult_real and in the output of mag / mag_squared, one result (and one uint32_t index) per item
 * for dot_prod / max / min.  Stream-ordered, no host synchronisation.
 * d_dst may equal a source exactly for conj (d_src), mult_cmplx (d_srcA or d_srcB) and mult_real (d_cmplx); any
 * other overlap of an output with a source returns ARM_MATH_ARGUMENT_ERROR (arm_mi355x_last_error() set).
 * arm_cmplx_dot_prod_*_batch: item i multiplies d_a[i] by the vector at d_b + i * bStride complex samples.
 * bStride == 0: one d_b shared by every item (correlation against a template); otherwise bStride >= numSamples,
 * or ARM_MATH_ARGUMENT_ERROR.  numSamples == 0 stores zeros.
 * ARM_MATH_ARGUMENT_ERROR on a null pointer; batch == 0, and numSamples == 0 where nothing is to be written, are
 * successful no-ops; blockSize == 0 with batch > 0 is an ARM_MATH_ARGUMENT_ERROR (the reference reads pSrc[0]).
 * There are no _batch_multi forms. */
#define MI355X_DECL_CMPLX_BATCH(SUF, T, R)                                                                     \
  arm_status arm_cmplx_mag_##SUF##_batch(const T *d_src, T *d_dst, uint32_t numSamples, uint32_t batch,        \
                                         void *stream);                                                        \
  arm_status arm_cmplx_mag_squared_##SUF##_batch(const T *d_src, T *d_dst, uint32_t numSamples, uint32_t batch, \
                                                 void *stream);                                                \
  arm_status arm_cmplx_conj_##SUF##_batch(const T *d_src, T *d_dst, uint32_t numSamples, uint32_t batch,       \
                                          void *stream);                                                       \
  arm_status arm_cmplx_mult_cmplx_##SUF##_batch(const T *d_srcA, const T *d_srcB, T *d_dst, uint32_t numSamples, \
                                                uint32_t batch, void *stream);                                 \
  arm_status arm_cmplx_mult_real_##SUF##_batch(const T *d_cmplx, const T *d_real, T *d_dst, uint32_t numSamples, \
                                               uint32_t batch, void *stream);                                  \
  arm_status arm_cmplx_dot_prod_##SUF##_batch(const T *d_a, const T *d_b, uint32_t bStride, uint32_t numSamples, \
                                              R *d_re, R *d_im, uint32_t batch, void *stream);
MI355X_DECL_CMPLX_BATCH(f32, float32_t, float32_t)
MI355X_DECL_CMPLX_BATCH(q31, q31_t, q63_t)
MI355X_DECL_CMPLX_BATCH(q15, q15_t, q31_t)
#undef MI355X_DECL_CMPLX_BATCH
#define MI355X_DECL_SEARCH_BATCH(SUF, T)                                                                       \
  arm_status arm_max_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t *d_index,         \
                                   uint32_t batch, void *stream);                                              \
  arm_status arm_min_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t *d_index,         \
                                   uint32_t batch, void *stream);
MI355X_DECL_SEARCH_BATCH(f32, float32_t)
MI355X_DECL_SEARCH_BATCH(q31, q31_t)
MI355X_DECL_SEARCH_BATCH(q15, q15_t)
MI355X_DECL_SEARCH_BATCH(q7, q7_t)
#undef MI355X_DECL_SEARCH_BATCH

/* Batched statistics (arm_math.h: "The level measures and the remaining searches"): item i is the blockSize
 * contiguous words at d_src + i * blockSize (arm_mse_*: of d_a and of d_b), and d_result[i] (d_index[i]) is what
 * the drop-in stores for it; the result words have the drop-in's result type (arm_power_*: float32_t, q63_t,
 * q63_t, q31_t).  Device pointers, stream-ordered.  The integer sums and the searches use the lanes-per-item
 * mapping of arm_max_*_batch; the f32 sums are ordered chains, one wave per item below 4096 items and one lane per
 * item from there on.  ARM_MATH_ARGUMENT_ERROR on a null pointer, on a result that overlaps a source or the index,
 * and on blockSize == 0 where the drop-in refuses it; batch == 0 is a successful no-op.
 * arm_cmplx_mag_fast_q15_batch: as arm_cmplx_mag_q15_batch. */
#define MI355X_DECL_STAT_BATCH(SUF, T, PR)                                                                      \
  arm_status arm_mean_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t batch, void *stream);  \
  arm_status arm_power_##SUF##_batch(const T *d_src, uint32_t blockSize, PR *d_result, uint32_t batch,          \
                                     void *stream);                                                             \
  arm_status arm_mse_##SUF##_batch(const T *d_a, const T *d_b, uint32_t blockSize, T *d_result, uint32_t batch, \
                                   void *stream);                                                               \
  arm_status arm_absmax_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t *d_index,       \
                                      uint32_t batch, void *stream);                                            \
  arm_status arm_absmin_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t *d_index,       \
                                      uint32_t batch, void *stream);                                            \
  arm_status arm_max_no_idx_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t batch,      \
                                          void *stream);                                                        \
  arm_status arm_min_no_idx_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t batch,      \
                                          void *stream);                                                        \
  arm_status arm_absmax_no_idx_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t batch,   \
                                             void *stream);                                                     \
  arm_status arm_absmin_no_idx_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t batch,   \
                                             void *stream);
#define MI355X_DECL_STAT_LEVELS_BATCH(SUF, T)                                                                       \
  arm_status arm_rms_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t batch, void *stream);  \
  arm_status arm_var_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t batch, void *stream);  \
  arm_status arm_std_##SUF##_batch(const T *d_src, uint32_t blockSize, T *d_result, uint32_t batch, void *stream);
MI355X_DECL_STAT_BATCH(f32, float32_t, float32_t)
MI355X_DECL_STAT_BATCH(q31, q31_t, q63_t)
MI355X_DECL_STAT_BATCH(q15, q15_t, q63_t)
MI355X_DECL_STAT_BATCH(q7, q7_t, q31_t)
MI355X_DECL_STAT_LEVELS_BATCH(f32, float32_t)
MI355X_DECL_STAT_LEVELS_BATCH(q31, q31_t)
MI355X_DECL_STAT_LEVELS_BATCH(q15, q15_t)
#undef MI355X_DECL_STAT_LEVELS_BATCH
#undef MI355X_DECL_STAT_BATCH
arm_status arm_accumulate_f32_batch(const float32_t *d_src, uint32_t blockSize, float32_t *d_result, uint32_t batch,
                                    void *stream);
arm_status arm_cmplx_mag_fast_q15_batch(const q15_t *d_src, q15_t *d_dst, uint32_t numSamples, uint32_t batch,
                                        void *stream);

/* Batched basic math (arm_math.h: "The basic math functions").  Element-wise: item i is the blockSize contiguous
 * words at d_src + i * blockSize and d_dst + i * blockSize, so the call runs over batch * blockSize words as one
 * flat array (16-byte loads and stores when every pointer is 16-byte aligned, single elements otherwise); one scalar
 * (offset, scale and shift, low and high) serves the whole call.  Device pointers, stream-ordered.
 * arm_dot_prod_*_batch: d_result[i] = the dot product of d_a + i * blockSize and d_b + i * bStride (words); bStride
 * 0 means one d_b for every item (a bank of signals against one template), otherwise bStride >= blockSize;
 * blockSize == 0 stores zeros.  The integer forms use the lanes-per-item mapping of arm_mse_*_batch, the f32 form
 * the ordered chains of arm_mse_f32_batch (one wave per item below 4096 items, one lane per item from there on).
 * ARM_MATH_ARGUMENT_ERROR on a null pointer, on a shift outside the drop-in's range, on bStride < blockSize, and on
 * an output that overlaps a source (d_dst may equal a source exactly); batch == 0 is a successful no-op. */
#define MI355X_DECL_BASIC_BATCH(SUF, T, DR)                                                                      \
  arm_status arm_add_##SUF##_batch(const T *d_srcA, const T *d_srcB, T *d_dst, uint32_t blockSize, uint32_t batch, \
                                   void *stream);                                                                \
  arm_status arm_sub_##SUF##_batch(const T *d_srcA, const T *d_srcB, T *d_dst, uint32_t blockSize, uint32_t batch, \
                                   void *stream);                                                                \
  arm_status arm_mult_##SUF##_batch(const T *d_srcA, const T *d_srcB, T *d_dst, uint32_t blockSize,              \
                                    uint32_t batch, void *stream);                                               \
  arm_status arm_offset_##SUF##_batch(const T *d_src, T offset, T *d_dst, uint32_t blockSize, uint32_t batch,    \
                                      void *stream);                                                             \
  arm_status arm_clip_##SUF##_batch(const T *d_src, T *d_dst, T low, T high, uint32_t numSamples, uint32_t batch, \
                                    void *stream);                                                               \
  arm_status arm_abs_##SUF##_batch(const T *d_src, T *d_dst, uint32_t blockSize, uint32_t batch, void *stream);  \
  arm_status arm_negate_##SUF##_batch(const T *d_src, T *d_dst, uint32_t blockSize, uint32_t batch,              \
                                      void *stream);                                                             \
  arm_status arm_dot_prod_##SUF##_batch(const T *d_a, const T *d_b, uint32_t bStride, uint32_t blockSize,        \
                                        DR *d_result, uint32_t batch, void *stream);
#define MI355X_DECL_BASIC_FIXED_BATCH(SUF, T)                                                                    \
  arm_status arm_scale_##SUF##_batch(const T *d_src, T scaleFract, int8_t shift, T *d_dst, uint32_t blockSize,   \
                                     uint32_t batch, void *stream);                                              \
  arm_status arm_shift_##SUF##_batch(const T *d_src, int8_t shiftBits, T *d_dst, uint32_t blockSize,             \
                                     uint32_t batch, void *stream);
#define MI355X_DECL_BITWISE_BATCH(SUF, T)                                                                        \
  arm_status arm_and_##SUF##_batch(const T *d_srcA, const T *d_srcB, T *d_dst, uint32_t blockSize, uint32_t batch, \
                                   void *stream);                                                                \
  arm_status arm_or_##SUF##_batch(const T *d_srcA, const T *d_srcB, T *d_dst, uint32_t blockSize, uint32_t batch, \
                                  void *stream);                                                                 \
  arm_status arm_xor_##SUF##_batch(const T *d_srcA, const T *d_srcB, T *d_dst, uint32_t blockSize, uint32_t batch, \
                                   void *stream);                                                                \
  arm_status arm_not_##SUF##_batch(const T *d_src, T *d_dst, uint32_t blockSize, uint32_t batch, void *stream);
MI355X_DECL_BASIC_BATCH(f32, float32_t, float32_t)
MI355X_DECL_BASIC_BATCH(q31, q31_t, q63_t)
MI355X_DECL_BASIC_BATCH(q15, q15_t, q63_t)
MI355X_DECL_BASIC_BATCH(q7, q7_t, q31_t)
MI355X_DECL_BASIC_FIXED_BATCH(q31, q31_t)
MI355X_DECL_BASIC_FIXED_BATCH(q15, q15_t)
MI355X_DECL_BASIC_FIXED_BATCH(q7, q7_t)
MI355X_DECL_BITWISE_BATCH(u32, uint32_t)
MI355X_DECL_BITWISE_BATCH(u16, uint16_t)
MI355X_DECL_BITWISE_BATCH(u8, uint8_t)
#undef MI355X_DECL_BITWISE_BATCH
#undef MI355X_DECL_BASIC_FIXED_BATCH
#undef MI355X_DECL_BASIC_BATCH
arm_status arm_scale_f32_batch(const float32_t *d_src, float32_t scale, float32_t *d_dst, uint32_t blockSize,
                               uint32_t batch, void *stream);

/* Batched support functions (arm_math.h: "The support functions").  Device pointers, stream-ordered.
 * Conversions, copy, fill: item i is the blockSize contiguous words at d_src + i * blockSize and d_dst + i *
 * blockSize, so the call runs over batch * blockSize words as one flat array (16-byte loads and stores on both
 * streams when both pointers are 16-byte aligned, single elements otherwise).  d_dst may equal d_src exactly where
 * both element widths are equal; any other overlap is refused.
 * arm_sort_f32_batch / arm_merge_sort_f32_batch (the same kernels): every item of blockSize words is sorted on its
 * own in the IEEE total order, dir ARM_SORT_ASCENDING or ARM_SORT_DESCENDING; d_dst may equal d_src exactly,
 * otherwise d_src is only read.  blockSize <= 2^31.  Padded lengths up to 256 take one wave per item, up to 16384 one
 * workgroup per item, longer items several launches in stream order.
 * arm_weighted_average_f32_batch: d_result[i] = the weighted average of d_in + i * blockSize under the weights at
 * d_weights + i * wStride (words); arm_barycenter_f32_batch: d_out + i * vecDim = the barycenter of the nbVectors
 * vectors at d_in + i * nbVectors * vecDim under the weights at d_weights + i * wStride.  wStride 0 means one weight
 * vector for every item, otherwise wStride >= the item's weight count (blockSize, nbVectors).
 * ARM_MATH_ARGUMENT_ERROR on a null pointer, an unknown dir, a wStride below the weight count and a refused
 * overlap; batch == 0 is a successful no-op. */
#define MI355X_DECL_SUPPORT_TO_BATCH(SN, ST, DN, DT)                                                             \
  arm_status arm_##SN##_to_##DN##_batch(const ST *d_src, DT *d_dst, uint32_t blockSize, uint32_t batch, void *stream);
MI355X_DECL_SUPPORT_TO_BATCH(float, float32_t, q31, q31_t)
MI355X_DECL_SUPPORT_TO_BATCH(float, float32_t, q15, q15_t)
MI355X_DECL_SUPPORT_TO_BATCH(float, float32_t, q7, q7_t)
MI355X_DECL_SUPPORT_TO_BATCH(q31, q31_t, float, float32_t)
MI355X_DECL_SUPPORT_TO_BATCH(q31, q31_t, q15, q15_t)
MI355X_DECL_SUPPORT_TO_BATCH(q31, q31_t, q7, q7_t)
MI355X_DECL_SUPPORT_TO_BATCH(q15, q15_t, float, float32_t)
MI355X_DECL_SUPPORT_TO_BATCH(q15, q15_t, q31, q31_t)
MI355X_DECL_SUPPORT_TO_BATCH(q15, q15_t, q7, q7_t)
MI355X_DECL_SUPPORT_TO_BATCH(q7, q7_t, float, float32_t)
MI355X_DECL_SUPPORT_TO_BATCH(q7, q7_t, q31, q31_t)
MI355X_DECL_SUPPORT_TO_BATCH(q7, q7_t, q15, q15_t)
#undef MI355X_DECL_SUPPORT_TO_BATCH
#define MI355X_DECL_SUPPORT_COPY_BATCH(SUF, T)                                                                   \
  arm_status arm_copy_##SUF##_batch(const T *d_src, T *d_dst, uint32_t blockSize, uint32_t batch, void *stream); \
  arm_status arm_fill_##SUF##_batch(T value, T *d_dst, uint32_t blockSize, uint32_t batch, void *stream);
MI355X_DECL_SUPPORT_COPY_BATCH(f32, float32_t)
MI355X_DECL_SUPPORT_COPY_BATCH(q31, q31_t)
MI355X_DECL_SUPPORT_COPY_BATCH(q15, q15_t)
MI355X_DECL_SUPPORT_COPY_BATCH(q7, q7_t)
#undef MI355X_DECL_SUPPORT_COPY_BATCH
arm_status arm_sort_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t blockSize, arm_sort_dir dir,
                              uint32_t batch, void *stream);
arm_status arm_merge_sort_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t blockSize, arm_sort_dir dir,
                                    uint32_t batch, void *stream);
arm_status arm_weighted_average_f32_batch(const float32_t *d_in, const float32_t *d_weights, uint32_t wStride,
                                          uint32_t blockSize, float32_t *d_result, uint32_t batch, void *stream);
arm_status arm_barycenter_f32_batch(const float32_t *d_in, const float32_t *d_weights, uint32_t wStride,
                                    float32_t *d_out, uint32_t nbVectors, uint32_t vecDim, uint32_t batch,
                                    void *stream);

/* Batched distance functions (arm_math.h: "The distance functions").  Device pointers, stream-ordered.
 * f32: d_result[i] = the distance of the blockSize words at d_a + i * blockSize and d_b + i * bStride; boolean: of the
 * ceil(numberOfBools / 32) words at d_a + i * that count and d_b + i * bStride.  bStride (words) 0 means one B vector
 * for every item (one query against many stored vectors), otherwise bStride >= the item's word count.  The sources are
 * only read, arm_correlation_distance_f32_batch included.  Below 4096 items an f32 item gets one wave, from there on
 * one lane; a boolean item gets the lanes its word count asks for (16-byte loads when both pointers, the item size
 * and bStride are multiples of 16 bytes).
 * arm_dtw_init_window_q7_batch fills `batch` contiguous queryLength x templateLength windows (all alike).
 * arm_dtw_distance_f32_batch: item i is the matrix at d_distance + i * queryLength * templateLength, its cost matrix
 * at d_dtw + the same offset (every word written), its window at d_window + i * wStride (d_window null: no window;
 * wStride 0: one window for every item, otherwise >= queryLength * templateLength).  d_status[i] (may be null) is
 * ARM_MATH_SUCCESS, or ARM_MATH_ARGUMENT_ERROR where no path exists inside the window; d_result[i] is written only
 * on success.  One wave per item.
 * arm_dtw_path_f32_batch: d_path + i * 2 * (queryLength + templateLength) receives item i's (query, template) index
 * pairs from (0, 0) to the last cell and d_pathLength[i] their count, or 0 where the walk cannot leave a cell (the
 * path words of such an item are unspecified).
 * ARM_MATH_ARGUMENT_ERROR, nothing written: a null pointer (d_window and d_status excepted), a stride below the item
 * size, a result that overlaps a source, blockSize 0 for chebyshev, a DTW length of 0 or above 32768, an unknown
 * window type.  batch == 0 is a successful no-op, and so is arm_dtw_init_window_q7_batch with a length of 0. */
#define MI355X_DECL_DISTANCE_F32_BATCH(NAME)                                                                     \
  arm_status arm_##NAME##_distance_f32_batch(const float32_t *d_a, const float32_t *d_b, uint32_t bStride,       \
                                             uint32_t blockSize, float32_t *d_result, uint32_t batch, void *stream);
MI355X_DECL_DISTANCE_F32_BATCH(braycurtis)
MI355X_DECL_DISTANCE_F32_BATCH(canberra)
MI355X_DECL_DISTANCE_F32_BATCH(chebyshev)
MI355X_DECL_DISTANCE_F32_BATCH(cityblock)
MI355X_DECL_DISTANCE_F32_BATCH(correlation)
MI355X_DECL_DISTANCE_F32_BATCH(cosine)
MI355X_DECL_DISTANCE_F32_BATCH(euclidean)
MI355X_DECL_DISTANCE_F32_BATCH(jensenshannon)
#undef MI355X_DECL_DISTANCE_F32_BATCH
#define MI355X_DECL_DISTANCE_BOOL_BATCH(NAME)                                                                    \
  arm_status arm_##NAME##_distance_batch(const uint32_t *d_a, const uint32_t *d_b, uint32_t bStride,             \
                                         uint32_t numberOfBools, float32_t *d_result, uint32_t batch, void *stream);
MI355X_DECL_DISTANCE_BOOL_BATCH(dice)
MI355X_DECL_DISTANCE_BOOL_BATCH(hamming)
MI355X_DECL_DISTANCE_BOOL_BATCH(jaccard)
MI355X_DECL_DISTANCE_BOOL_BATCH(kulsinski)
MI355X_DECL_DISTANCE_BOOL_BATCH(rogerstanimoto)
MI355X_DECL_DISTANCE_BOOL_BATCH(russellrao)
MI355X_DECL_DISTANCE_BOOL_BATCH(sokalmichener)
MI355X_DECL_DISTANCE_BOOL_BATCH(sokalsneath)
MI355X_DECL_DISTANCE_BOOL_BATCH(yule)
#undef MI355X_DECL_DISTANCE_BOOL_BATCH
arm_status arm_dtw_init_window_q7_batch(arm_dtw_window windowType, int32_t windowSize, q7_t *d_window,
                                        uint32_t queryLength, uint32_t templateLength, uint32_t batch, void *stream);
arm_status arm_dtw_distance_f32_batch(const float32_t *d_distance, const q7_t *d_window, uint32_t wStride,
                                      float32_t *d_dtw, uint32_t queryLength, uint32_t templateLength,
                                      float32_t *d_result, int32_t *d_status, uint32_t batch, void *stream);
arm_status arm_dtw_path_f32_batch(const float32_t *d_dtw, uint32_t queryLength, uint32_t templateLength,
                                  int16_t *d_path, uint32_t *d_pathLength, uint32_t batch, void *stream);

/* Batched vexp / vlog, log-domain statistics, SVMs and naive Bayes (arm_math.h: "arm_vexp_f32 / arm_vlog_f32 ...").
 * Device pointers, stream-ordered.
 * arm_vexp_f32_batch / arm_vlog_f32_batch: blockSize * batch words; d_dst may be d_src exactly.
 * The statistics give one word per item: d_result[i] of the blockSize words at d_src (d_a) + i * blockSize and, for
 * kullback_leibler and logsumexp_dot_prod, d_b + i * bStride; bStride (words) 0 means one B vector for every item,
 * otherwise bStride >= blockSize.  logsumexp_dot_prod takes no scratch: a + b is formed in registers.  Below 4096
 * items an item gets one wave, from there on one lane.
 * The classifiers share one model among the nbItems vectors at d_in + i * vectorDimension; the arrays of S are device
 * pointers (S itself is host memory).  SVM: d_result[i] is the class, d_decision[i] (d_decision may be null) the
 * final sum the class was taken from.  Bayes: d_probabilities + i * numberOfClasses receives the classes' words,
 * d_class[i] the index.  An item's chains (one per support vector or class) run in the lanes of a group of 1 to 64
 * lanes; the model is held in LDS where it fits 64 KiB (SVM: nbOfSupportVectors * (vectorDimension | 1) +
 * nbOfSupportVectors words; Bayes: 2 * numberOfClasses * ((vectorDimension | 1) + 1) words) and is read from global
 * memory otherwise.
 * ARM_MATH_ARGUMENT_ERROR, nothing written: a null pointer (d_decision excepted), a stride below blockSize, a result
 * that overlaps a source or another result, blockSize 0 for the logsumexp forms, numberOfClasses 0.  batch == 0 or
 * nbItems == 0 is a successful no-op. */
arm_status arm_vexp_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t blockSize, uint32_t batch,
                              void *stream);
arm_status arm_vlog_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t blockSize, uint32_t batch,
                              void *stream);
arm_status arm_entropy_f32_batch(const float32_t *d_src, uint32_t blockSize, float32_t *d_result, uint32_t batch,
                                 void *stream);
arm_status arm_logsumexp_f32_batch(const float32_t *d_src, uint32_t blockSize, float32_t *d_result, uint32_t batch,
                                   void *stream);
arm_status arm_kullback_leibler_f32_batch(const float32_t *d_a, const float32_t *d_b, uint32_t bStride,
                                          uint32_t blockSize, float32_t *d_result, uint32_t batch, void *stream);
arm_status arm_logsumexp_dot_prod_f32_batch(const float32_t *d_a, const float32_t *d_b, uint32_t bStride,
                                            uint32_t blockSize, float32_t *d_result, uint32_t batch, void *stream);
arm_status arm_svm_linear_predict_f32_batch(const arm_svm_linear_instance_f32 *S, const float32_t *d_in,
                                            int32_t *d_result, float32_t *d_decision, uint32_t nbItems,
                                            void *stream);
arm_status arm_svm_polynomial_predict_f32_batch(const arm_svm_polynomial_instance_f32 *S, const float32_t *d_in,
                                                int32_t *d_result, float32_t *d_decision, uint32_t nbItems,
                                                void *stream);
arm_status arm_svm_rbf_predict_f32_batch(const arm_svm_rbf_instance_f32 *S, const float32_t *d_in, int32_t *d_result,
                                         float32_t *d_decision, uint32_t nbItems, void *stream);
arm_status arm_gaussian_naive_bayes_predict_f32_batch(const arm_gaussian_naive_bayes_instance_f32 *S,
                                                      const float32_t *d_in, float32_t *d_probabilities,
                                                      uint32_t *d_class, uint32_t nbItems, void *stream);

/* Batched interpolation (arm_math.h: "Interpolation ...").  Device pointers, stream-ordered; every device table is read
 * on `stream`, so a table written on that stream immediately before the call is seen.  S is host memory, its table
 * pointer a device pointer.
 * Linear: d_y[i] = arm_linear_interp_<t>(d_x[i]) for blockSize samples that share one table.  The table is staged in
 * LDS where it fits 64 KiB (16384 f32 words; a fixed-point table is only read up to entry 2048) and read from global
 * memory otherwise.
 * Bilinear: d_out[i] = arm_bilinear_interp_<t>(S, d_X[i], d_Y[i]), four table reads per point from global memory.
 * Spline, over `batch` independent items: arm_spline_init_f32_batch reads item i's n knots at d_x + i * xStride
 * (xStride 0: one knot vector for every item, otherwise xStride >= n) and its values at d_y + i * n, and writes 3 (n -
 * 1) words at d_coeffs + i * 3 (n - 1) (b, c, d) and 2 n - 1 words at d_temp + i * (2 n - 1) (u, z); one lane takes
 * one item, whatever the batch.  arm_spline_f32_batch evaluates item i's blockSize queries at d_xq + i * xqStride
 * (xqStride 0: one query vector for every item, otherwise xqStride >= blockSize) into d_dst + i * blockSize; one wave
 * takes one item.
 * ARM_MATH_ARGUMENT_ERROR, nothing written: a null pointer, nValues == 0, numRows * numCols >= 2^31, n < 2, a type other
 * than ARM_SPLINE_NATURAL and ARM_SPLINE_PARABOLIC_RUNOUT, a stride below the item length, a result that overlaps a
 * source or another result.  blockSize == 0 or batch == 0 is a successful no-op. */
arm_status arm_linear_interp_f32_batch(const arm_linear_interp_instance_f32 *S, const float32_t *d_x, float32_t *d_y,
                                       uint32_t blockSize, void *stream);
arm_status arm_linear_interp_q31_batch(const q31_t *d_table, uint32_t nValues, const q31_t *d_x, q31_t *d_y,
                                       uint32_t blockSize, void *stream);
arm_status arm_linear_interp_q15_batch(const q15_t *d_table, uint32_t nValues, const q31_t *d_x, q15_t *d_y,
                                       uint32_t blockSize, void *stream);
arm_status arm_linear_interp_q7_batch(const q7_t *d_table, uint32_t nValues, const q31_t *d_x, q7_t *d_y,
                                      uint32_t blockSize, void *stream);
arm_status arm_bilinear_interp_f32_batch(const arm_bilinear_interp_instance_f32 *S, const float32_t *d_X,
                                         const float32_t *d_Y, float32_t *d_out, uint32_t blockSize, void *stream);
arm_status arm_bilinear_interp_q31_batch(const arm_bilinear_interp_instance_q31 *S, const q31_t *d_X, const q31_t *d_Y,
                                         q31_t *d_out, uint32_t blockSize, void *stream);
arm_status arm_bilinear_interp_q15_batch(const arm_bilinear_interp_instance_q15 *S, const q31_t *d_X, const q31_t *d_Y,
                                         q15_t *d_out, uint32_t blockSize, void *stream);
arm_status arm_bilinear_interp_q7_batch(const arm_bilinear_interp_instance_q7 *S, const q31_t *d_X, const q31_t *d_Y,
                                        q7_t *d_out, uint32_t blockSize, void *stream);
arm_status arm_spline_init_f32_batch(arm_spline_type type, const float32_t *d_x, uint32_t xStride,
                                     const float32_t *d_y, uint32_t n, float32_t *d_coeffs, float32_t *d_temp,
                                     uint32_t batch, void *stream);
arm_status arm_spline_f32_batch(const float32_t *d_x, uint32_t xStride, const float32_t *d_y,
                                const float32_t *d_coeffs, uint32_t n, const float32_t *d_xq, uint32_t xqStride,
                                float32_t *d_dst, uint32_t blockSize, uint32_t batch, void *stream);

/* Batched quaternion functions (arm_math.h: "The quaternion functions ...").  Device pointers, stream-ordered; the
 * arrays are read and written on `stream`, so a source written on that stream immediately before the call is seen.
 * One lane takes one quaternion: a 16-byte access where the array is 16-byte aligned, four words otherwise.  The
 * 36-byte rotations pass through LDS so that a wave's global accesses are 64 consecutive words.
 * arm_quaternion_product_f32_batch: bStride (words) is 4, or 0 to multiply every d_qa[i] by the one quaternion at d_qb.
 * ARM_MATH_ARGUMENT_ERROR, nothing written: a null pointer, a bStride other than 0 and 4, a result that overlaps a
 * source (a result of quaternions may be a source of quaternions exactly).  nbQuaternions == 0 is a successful
 * no-op. */
arm_status arm_quaternion_norm_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t nbQuaternions,
                                         void *stream);
arm_status arm_quaternion_inverse_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t nbQuaternions,
                                            void *stream);
arm_status arm_quaternion_conjugate_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t nbQuaternions,
                                              void *stream);
arm_status arm_quaternion_normalize_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t nbQuaternions,
                                              void *stream);
arm_status arm_quaternion_product_f32_batch(const float32_t *d_qa, const float32_t *d_qb, uint32_t bStride,
                                            float32_t *d_qr, uint32_t nbQuaternions, void *stream);
arm_status arm_quaternion2rotation_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t nbQuaternions,
                                             void *stream);
arm_status arm_rotation2quaternion_f32_batch(const float32_t *d_src, float32_t *d_dst, uint32_t nbQuaternions,
                                             void *stream);

/* Multi-GPU complex FFT (SURVEY §8b "a multi-GPU entry point"; per item: arm_cfft_f32 /
 * _q31 / _q15, transform_functions.h:456-460).  Shard s of `nshards` is batch[s] contiguous
 * transforms at DEVICE pointer d_p1[s] on HIP device devices[s] (a device may appear in
 * several shards).  Every shard is launched on an internal stream of its device before any
 * is waited for, so the devices run concurrently; the call returns when all shards are
 * done (synchronous, like the drop-in API).  Input written on other streams must be
 * complete before the call.  Arguments are validated before anything is launched:
 * ARM_MATH_ARGUMENT_ERROR for a bad device index, NULL pointer or unsupported length.
 * The calling thread's current device is restored. */
arm_status arm_cfft_f32_batch_multi(const arm_cfft_instance_f32 *S, uint32_t nshards, const int *devices,
                                    float32_t *const *d_p1, const uint32_t *batch, uint8_t ifftFlag,
                                    uint8_t bitReverseFlag);
arm_status arm_cfft_q31_batch_multi(const arm_cfft_instance_q31 *S, uint32_t nshards, const int *devices,
                                    q31_t *const *d_p1, const uint32_t *batch, uint8_t ifftFlag,
                                    uint8_t bitReverseFlag);
arm_status arm_cfft_q15_batch_multi(const arm_cfft_instance_q15 *S, uint32_t nshards, const int *devices,
                                    q15_t *const *d_p1, const uint32_t *batch, uint8_t ifftFlag,
                                    uint8_t bitReverseFlag);

/* Multi-GPU FIR (the batch is sliced by filter, so each filter's history stays on
 * its device; per filter: arm_fir_f32.c:911-1280, arm_fir_q15.c:458-726, ...).  Shard s of
 * `nshards` is batch[s] filters of blockSize samples on HIP device devices[s]: DEVICE pointers
 * d_src[s] / d_dst[s] [batch[s]][blockSize] and d_hist[s] [batch[s]][numTaps-1] with the
 * arm_fir_*_batch state contract.  S->pCoeffs: a host pointer (uploaded once per device), or a
 * device pointer every shard's device can read.  Launch/validate/wait semantics as
 * arm_cfft_f32_batch_multi. */
arm_status arm_fir_f32_batch_multi(const arm_fir_instance_f32 *S, uint32_t nshards, const int *devices,
                                   const float32_t *const *d_src, float32_t *const *d_dst, float32_t *const *d_hist,
                                   uint32_t blockSize, const uint32_t *batch);
arm_status arm_fir_q15_batch_multi(const arm_fir_instance_q15 *S, uint32_t nshards, const int *devices,
                                   const q15_t *const *d_src, q15_t *const *d_dst, q15_t *const *d_hist,
                                   uint32_t blockSize, const uint32_t *batch);
arm_status arm_fir_fast_q15_batch_multi(const arm_fir_instance_q15 *S, uint32_t nshards, const int *devices,
                                        const q15_t *const *d_src, q15_t *const *d_dst, q15_t *const *d_hist,
                                        uint32_t blockSize, const uint32_t *batch);
arm_status arm_fir_q31_batch_multi(const arm_fir_instance_q31 *S, uint32_t nshards, const int *devices,
                                   const q31_t *const *d_src, q31_t *const *d_dst, q31_t *const *d_hist,
                                   uint32_t blockSize, const uint32_t *batch);
arm_status arm_fir_fast_q31_batch_multi(const arm_fir_instance_q31 *S, uint32_t nshards, const int *devices,
                                        const q31_t *const *d_src, q31_t *const *d_dst, q31_t *const *d_hist,
                                        uint32_t blockSize, const uint32_t *batch);
arm_status arm_fir_q7_batch_multi(const arm_fir_instance_q7 *S, uint32_t nshards, const int *devices,
                                  const q7_t *const *d_src, q7_t *const *d_dst, q7_t *const *d_hist,
                                  uint32_t blockSize, const uint32_t *batch);

/* Multi-GPU matrix multiply (per matrix: arm_mat_mult_f32.c:600-730 / _q15 / _q31): shard s is
 * batch[s] contiguous matrices with the instances' shapes (their pData are not used) at DEVICE
 * pointers d_a[s], d_b[s], d_c[s] on devices[s].  ARM_MATH_SIZE_MISMATCH on incompatible
 * shapes; otherwise as arm_cfft_f32_batch_multi. */
arm_status arm_mat_mult_f32_batch_multi(const arm_matrix_instance_f32 *pSrcA, const arm_matrix_instance_f32 *pSrcB,
                                        arm_matrix_instance_f32 *pDst, uint32_t nshards, const int *devices,
                                        const float32_t *const *d_a, const float32_t *const *d_b,
                                        float32_t *const *d_c, const uint32_t *batch);
arm_status arm_mat_mult_q7_batch_multi(const arm_matrix_instance_q7 *pSrcA, const arm_matrix_instance_q7 *pSrcB,
                                       arm_matrix_instance_q7 *pDst, uint32_t nshards, const int *devices,
                                       const q7_t *const *d_a, const q7_t *const *d_b, q7_t *const *d_c,
                                       const uint32_t *batch);
arm_status arm_mat_mult_q15_batch_multi(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                                        arm_matrix_instance_q15 *pDst, uint32_t nshards, const int *devices,
                                        const q15_t *const *d_a, const q15_t *const *d_b, q15_t *const *d_c,
                                        const uint32_t *batch);
arm_status arm_mat_mult_q31_batch_multi(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                                        arm_matrix_instance_q31 *pDst, uint32_t nshards, const int *devices,
                                        const q31_t *const *d_a, const q31_t *const *d_b, q31_t *const *d_c,
                                        const uint32_t *batch);
/* ... and of the complex matrix multiply. */
arm_status arm_mat_cmplx_mult_f32_batch_multi(const arm_matrix_instance_f32 *pSrcA,
                                              const arm_matrix_instance_f32 *pSrcB, arm_matrix_instance_f32 *pDst,
                                              uint32_t nshards, const int *devices, const float32_t *const *d_a,
                                              const float32_t *const *d_b, float32_t *const *d_c,
                                              const uint32_t *batch);
arm_status arm_mat_cmplx_mult_q31_batch_multi(const arm_matrix_instance_q31 *pSrcA,
                                              const arm_matrix_instance_q31 *pSrcB, arm_matrix_instance_q31 *pDst,
                                              uint32_t nshards, const int *devices, const q31_t *const *d_a,
                                              const q31_t *const *d_b, q31_t *const *d_c, const uint32_t *batch);
arm_status arm_mat_cmplx_mult_q15_batch_multi(const arm_matrix_instance_q15 *pSrcA,
                                              const arm_matrix_instance_q15 *pSrcB, arm_matrix_instance_q15 *pDst,
                                              uint32_t nshards, const int *devices, const q15_t *const *d_a,
                                              const q15_t *const *d_b, q15_t *const *d_c, const uint32_t *batch);

/* Number of HIP devices visible to the process (0 when none). */
int arm_mi355x_device_count(void);

/* Error channel for the void-returning drop-in functions: 0 = no error, otherwise the
 * hipError_t of the last failure on this thread. */
int arm_mi355x_last_error(void);
const char *arm_mi355x_last_error_string(void);
void arm_mi355x_clear_error(void);

/* Device bytes held by the content-keyed cache of host tables / coefficients (all devices),
 * and its limit PER DEVICE (default 256 MiB).  Lowering it evicts least-recently-used entries
 * now.  An entry in use by a call that is still being enqueued is never evicted, and an
 * evicted entry's memory is released in stream order after the work that read it (an event
 * recorded after each call's launches; no device synchronize, no lock held while waiting). */
size_t arm_mi355x_table_cache_bytes(void);
void arm_mi355x_set_table_cache_limit(size_t bytes);

/* Per-thread runtime resources.  A thread that calls the synchronous (drop-in) functions gets a
 * stream per device, device scratch, pinned staging buffers and a completion word, grown on
 * demand (the reference allocates nothing: this is the backend's cost of being a drop-in).
 * They are released automatically when a thread other than the process's main thread exits;
 * arm_mi355x_release_thread_resources() releases the calling thread's set now (call it between
 * calls, e.g. before a pool retires a worker, or on the main thread; the next call re-creates
 * what it needs).  arm_mi355x_thread_resource_owners() counts the threads holding a set. */
void arm_mi355x_release_thread_resources(void);
int arm_mi355x_thread_resource_owners(void);

/* Library identification: "cmsisdsp-mi355x <version> gfx950 src:<id>", where <id> is a hash of
 * the sources the library was built from (cmsis-dsp_amd/Makefile SRC_ID), followed by
 * " [macros]" when the library was built with any non-default tuning macro (bench lines print
 * it). */
const char *arm_mi355x_version(void);

#ifdef __cplusplus
}
#endif
#endif
