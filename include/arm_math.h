/*
 * arm_math.h — drop-in subset of the CMSIS-DSP public API, served by the MI355X backend
 * (libcmsisdsp_mi355x.so).  Only the hot path named in BASELINE.json `north_star` lives
 * here: complex FFT f32/q31/q15, real FFT (fast) f32, FIR f32/q15, matrix multiply f32.
 *
 * Every type and prototype keeps the reference's layout and signature so that existing
 * C callers recompile unchanged.  Each declaration cites the reference interface it
 * replaces (paths relative to the reference tree, xavierbrgt/CMSIS-DSP).
 *
 * Semantics contract:
 *   - processing functions are synchronous: when they return, the result is in p1/pDst;
 *   - buffers may be host memory (staged through pinned memory) or device memory
 *     (hipMalloc'd; used in place, no copies);
 *   - an unsupported fftLen is a silent no-op, exactly like the reference switch;
 *   - no processing function aborts or throws: a device failure is reported through
 *     arm_mi355x_last_error() (arm_math_mi355x.h).
 * The batched, stream-ordered, device-pointer API lives in arm_math_mi355x.h.
 */
#ifndef ARM_MATH_MI355X_DROPIN_H
#define ARM_MATH_MI355X_DROPIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scalar types: Include/arm_math_types.h:324-351 ---------------------------- */
typedef int8_t   q7_t;
typedef int16_t  q15_t;
typedef int32_t  q31_t;
typedef int64_t  q63_t;
typedef float    float32_t;
typedef double   float64_t;

/* ---- status codes: Include/arm_math_types.h:603-613 ---------------------------- */
typedef enum {
  ARM_MATH_SUCCESS               =  0,
  ARM_MATH_ARGUMENT_ERROR        = -1,
  ARM_MATH_LENGTH_ERROR          = -2,
  ARM_MATH_SIZE_MISMATCH         = -3,
  ARM_MATH_NANINF                = -4,
  ARM_MATH_SINGULAR              = -5,
  ARM_MATH_TEST_FAILURE          = -6,
  ARM_MATH_DECOMPOSITION_FAILURE = -7
} arm_status;

/* ---- transform buffer-size helpers: Include/arm_math_types.h:667-700 (enums, default target)
 * and Include/dsp/transform_functions.h:1307-1398 (functions; bodies in
 * Source/TransformFunctions/arm_transform_buffer_sizes.c:47-330).  Lengths in real elements;
 * 0 = buffer not needed, -1 = configuration not supported.  This library is a scalar-API build:
 * ARM_MATH_DEFAULT_TARGET_ARCH is ARM_MATH_SCALAR_ARCH, and the MFCC is RFFT-based
 * (ARM_MFCC_USE_CFFT undefined, as in the reference's default build). ---------------------- */
typedef enum {
  ARM_MATH_F16 = 16,
  ARM_MATH_F32 = 32,
  ARM_MATH_F64 = 64,
  ARM_MATH_Q7  = 7,
  ARM_MATH_Q15 = 15,
  ARM_MATH_Q31 = 31
} arm_math_datatype;

typedef enum {
  ARM_MATH_SCALAR_ARCH         = 1,
  ARM_MATH_DSP_EXTENSIONS_ARCH = 2,
  ARM_MATH_HELIUM_ARCH         = 3,
  ARM_MATH_NEON_ARCH           = 4
} arm_math_target_arch;

#define ARM_MATH_DEFAULT_TARGET_ARCH ARM_MATH_SCALAR_ARCH

int32_t arm_cfft_tmp_buffer_size(arm_math_target_arch arch, arm_math_datatype dt, uint32_t nb_samples,
                                 uint32_t buf_id);
int32_t arm_cfft_output_buffer_size(arm_math_target_arch arch, arm_math_datatype dt, uint32_t nb_samples);
int32_t arm_cifft_output_buffer_size(arm_math_target_arch arch, arm_math_datatype dt, uint32_t nb_samples);
int32_t arm_rfft_tmp_buffer_size(arm_math_target_arch arch, arm_math_datatype dt, uint32_t nb_samples,
                                 uint32_t buf_id);
int32_t arm_rfft_output_buffer_size(arm_math_target_arch arch, arm_math_datatype dt, uint32_t nb_samples);
int32_t arm_rifft_input_buffer_size(arm_math_target_arch arch, arm_math_datatype dt, uint32_t nb_samples);
int32_t arm_mfcc_tmp_buffer_size(arm_math_target_arch arch, arm_math_datatype dt, uint32_t nb_samples,
                                 uint32_t buf_id, uint32_t use_cfft);

/* ---- complex FFT instances: Include/dsp/transform_functions.h:282-296,347-361,410-424
 * (scalar/non-Helium layout: {fftLen, pTwiddle, pBitRevTable, bitRevLength}) -------- */
typedef struct {
        uint16_t   fftLen;
  const float32_t *pTwiddle;
  const uint16_t  *pBitRevTable;
        uint16_t   bitRevLength;
} arm_cfft_instance_f32;

typedef struct {
        uint16_t   fftLen;
  const q31_t     *pTwiddle;
  const uint16_t  *pBitRevTable;
        uint16_t   bitRevLength;
} arm_cfft_instance_q31;

typedef struct {
        uint16_t   fftLen;
  const q15_t     *pTwiddle;
  const uint16_t  *pBitRevTable;
        uint16_t   bitRevLength;
} arm_cfft_instance_q15;

/* ---- real FFT (fast) instance: Include/dsp/transform_functions.h:813-818 ---------- */
typedef struct {
        arm_cfft_instance_f32 Sint;
        uint16_t              fftLenRFFT;
  const float32_t            *pTwiddleRFFT;
} arm_rfft_fast_instance_f32;

/* ---- real FFT instances, q31 / q15 (non-Neon, non-MVE build):
 * Include/dsp/transform_functions.h:636-649 (q31), :508-521 (q15) */
typedef struct {
        uint32_t   fftLenReal;            /* real length N (32 ... 8192) */
        uint8_t    ifftFlagR;             /* 0 forward, 1 inverse */
        uint8_t    bitReverseFlagR;       /* passed to the inner CFFT */
        uint32_t   twidCoefRModifier;     /* 8192 / N: stride into realCoefA/BQ31 */
  const q31_t     *pTwiddleAReal;
  const q31_t     *pTwiddleBReal;
  const arm_cfft_instance_q31 *pCfft;     /* inner CFFT of N/2 */
} arm_rfft_instance_q31;

typedef struct {
        uint32_t   fftLenReal;
        uint8_t    ifftFlagR;
        uint8_t    bitReverseFlagR;
        uint32_t   twidCoefRModifier;
  const q15_t     *pTwiddleAReal;
  const q15_t     *pTwiddleBReal;
  const arm_cfft_instance_q15 *pCfft;
} arm_rfft_instance_q15;

/* ---- MFCC instance (RFFT-based default build): Include/dsp/transform_functions.h:856-873 */
typedef struct {
  const float32_t *dctCoefs;        /* nbDctOutputs x nbMelFilters, row-major */
  const float32_t *filterCoefs;     /* concatenated Mel filters (sum of filterLengths) */
  const float32_t *windowCoefs;     /* fftLen */
  const uint32_t  *filterPos;       /* first FFT bin of each Mel filter */
  const uint32_t  *filterLengths;   /* bins per Mel filter */
        uint32_t   fftLen;
        uint32_t   nbMelFilters;
        uint32_t   nbDctOutputs;
  arm_rfft_fast_instance_f32 rfft;
} arm_mfcc_instance_f32;

/* Include/dsp/transform_functions.h:1000-1020 (RFFT-based default build) */
typedef struct {
  const q31_t    *dctCoefs;
  const q31_t    *filterCoefs;
  const q31_t    *windowCoefs;
  const uint32_t *filterPos;
  const uint32_t *filterLengths;
        uint32_t   fftLen;
        uint32_t   nbMelFilters;
        uint32_t   nbDctOutputs;
  arm_rfft_instance_q31 rfft;
} arm_mfcc_instance_q31;

/* Include/dsp/transform_functions.h:1150-1168 (RFFT-based default build) */
typedef struct {
  const q15_t    *dctCoefs;
  const q15_t    *filterCoefs;
  const q15_t    *windowCoefs;
  const uint32_t *filterPos;
  const uint32_t *filterLengths;
        uint32_t   fftLen;
        uint32_t   nbMelFilters;
        uint32_t   nbDctOutputs;
  arm_rfft_instance_q15 rfft;
} arm_mfcc_instance_q15;

/* ---- FIR instances: Include/dsp/filtering_functions.h:56-61 (q7), 66-71, 76-81, 86-91 */
typedef struct {
        uint16_t   numTaps;
        q7_t      *pState;
  const q7_t      *pCoeffs;
} arm_fir_instance_q7;

typedef struct {
        uint16_t   numTaps;
        q15_t     *pState;
  const q15_t     *pCoeffs;
} arm_fir_instance_q15;

typedef struct {
        uint16_t   numTaps;
        q31_t     *pState;
  const q31_t     *pCoeffs;
} arm_fir_instance_q31;

typedef struct {
        uint16_t   numTaps;
        float32_t *pState;
  const float32_t *pCoeffs;
} arm_fir_instance_f32;

/* ---- multirate FIR instances: Include/dsp/filtering_functions.h:803-831 (decimators),
 * :1012-1040 (interpolators) */
typedef struct {
        uint8_t    M;
        uint16_t   numTaps;
  const q15_t     *pCoeffs;
        q15_t     *pState;
} arm_fir_decimate_instance_q15;

typedef struct {
        uint8_t    M;
        uint16_t   numTaps;
  const q31_t     *pCoeffs;
        q31_t     *pState;
} arm_fir_decimate_instance_q31;

typedef struct {
        uint8_t    M;
        uint16_t   numTaps;
  const float32_t *pCoeffs;
        float32_t *pState;
} arm_fir_decimate_instance_f32;

typedef struct {
        uint8_t    L;
        uint16_t   phaseLength;
  const q15_t     *pCoeffs;
        q15_t     *pState;
} arm_fir_interpolate_instance_q15;

typedef struct {
        uint8_t    L;
        uint16_t   phaseLength;
  const q31_t     *pCoeffs;
        q31_t     *pState;
} arm_fir_interpolate_instance_q31;

typedef struct {
        uint8_t    L;
        uint16_t   phaseLength;
  const float32_t *pCoeffs;
        float32_t *pState;
} arm_fir_interpolate_instance_f32;

/* Sparse FIR instances (Include/dsp/filtering_functions.h:2033-2091), same layout for each type. */
#define MI355X_SPARSE_INST(T, ET)                                                               \
  typedef struct {                                                                              \
          uint16_t numTaps;    /* nonzero taps */                                               \
          uint16_t stateIndex; /* circular write position in pState */                          \
          ET      *pState;     /* maxDelay + blockSize words (circular) */                      \
    const ET      *pCoeffs;    /* numTaps */                                                    \
          uint16_t maxDelay;                                                                    \
          int32_t *pTapDelay;  /* numTaps delays, each in [0, maxDelay] */                      \
  } arm_fir_sparse_instance_##T;
MI355X_SPARSE_INST(f32, float32_t)
MI355X_SPARSE_INST(q31, q31_t)
MI355X_SPARSE_INST(q15, q15_t)
MI355X_SPARSE_INST(q7, q7_t)
#undef MI355X_SPARSE_INST

/* FIR lattice instances (Include/dsp/filtering_functions.h:1312-1340), same layout per type. */
#define MI355X_LATTICE_INST(T, ET)                                                              \
  typedef struct {                                                                              \
          uint16_t numStages;                                                                   \
          ET      *pState;     /* numStages words: g_m at the previous sample */                \
    const ET      *pCoeffs;    /* numStages reflection coefficients */                          \
  } arm_fir_lattice_instance_##T;
MI355X_LATTICE_INST(q15, q15_t)
MI355X_LATTICE_INST(q31, q31_t)
MI355X_LATTICE_INST(f32, float32_t)
#undef MI355X_LATTICE_INST

/* Biquad cascade instances (Include/dsp/filtering_functions.h:285-312, :1148-1203).  State words per
 * stage: DF1 4 {x1, x2, y1, y2} (32x64: q63 words), DF2T 2 {d1, d2}, stereo DF2T 4 {d1a, d2a, d1b, d2b};
 * coefficients per stage 5 {b0, b1, b2, a1, a2}, q15 6 {b0, 0, b1, b2, a1, a2}. */
typedef struct {
        int8_t  numStages;
        q15_t  *pState;      /* 4*numStages */
  const q15_t  *pCoeffs;     /* 6*numStages */
        int8_t  postShift;
} arm_biquad_casd_df1_inst_q15;
typedef struct {
        uint32_t numStages;
        q31_t   *pState;     /* 4*numStages */
  const q31_t   *pCoeffs;    /* 5*numStages */
        uint8_t  postShift;
} arm_biquad_casd_df1_inst_q31;
typedef struct {
        uint32_t   numStages;
        float32_t *pState;   /* 4*numStages */
  const float32_t *pCoeffs;  /* 5*numStages */
} arm_biquad_casd_df1_inst_f32;
typedef struct {
        uint8_t  numStages;
        q63_t   *pState;     /* 4*numStages */
  const q31_t   *pCoeffs;    /* 5*numStages */
        uint8_t  postShift;
} arm_biquad_cas_df1_32x64_ins_q31;
typedef struct {
        uint8_t    numStages;
        float32_t *pState;   /* 2*numStages */
  const float32_t *pCoeffs;  /* 5*numStages */
} arm_biquad_cascade_df2T_instance_f32;
typedef struct {
        uint8_t    numStages;
        float32_t *pState;   /* 4*numStages */
  const float32_t *pCoeffs;  /* 5*numStages */
} arm_biquad_cascade_stereo_df2T_instance_f32;

/* IIR lattice instances (Include/dsp/filtering_functions.h:1428-1458).  pState: numStages + blockSize
 * words, of which the first numStages are the live state between calls; pkCoeffs: numStages reflection
 * words; pvCoeffs: numStages + 1 ladder words. */
#define MI355X_IIR_LATTICE_INST(T, CT)                                        \
  typedef struct {                                                            \
    uint16_t numStages;                                                       \
    CT *pState;                                                               \
    CT *pkCoeffs;                                                             \
    CT *pvCoeffs;                                                             \
  } arm_iir_lattice_instance_##T;
MI355X_IIR_LATTICE_INST(q15, q15_t)
MI355X_IIR_LATTICE_INST(q31, q31_t)
MI355X_IIR_LATTICE_INST(f32, float32_t)
#undef MI355X_IIR_LATTICE_INST

/* LMS / normalised LMS instances (filtering_functions.h:1560-1566, :1608-1615, :1659-1666, :1710-1718,
 * :1813-1824).  pState: numTaps + blockSize - 1 words, of which the first numTaps - 1 are the live
 * history (oldest first) between calls; pCoeffs: numTaps words, time-reversed, updated in place. */
typedef struct {
  uint16_t   numTaps;
  float32_t *pState;
  float32_t *pCoeffs;
  float32_t  mu;
} arm_lms_instance_f32;
typedef struct {
  uint16_t numTaps;
  q15_t   *pState;
  q15_t   *pCoeffs;
  q15_t    mu;
  uint32_t postShift;
} arm_lms_instance_q15;
typedef struct {
  uint16_t numTaps;
  q31_t   *pState;
  q31_t   *pCoeffs;
  q31_t    mu;
  uint32_t postShift;
} arm_lms_instance_q31;
typedef struct {
  uint16_t   numTaps;
  float32_t *pState;
  float32_t *pCoeffs;
  float32_t  mu;
  float32_t  energy;
  float32_t  x0;
} arm_lms_norm_instance_f32;
typedef struct {
        uint16_t numTaps;
        q15_t   *pState;
        q15_t   *pCoeffs;
        q15_t    mu;
        uint8_t  postShift;
  const q15_t   *recipTable;   /* armRecipTableQ15 (arm_common_tables.h) */
        q15_t    energy;
        q15_t    x0;
} arm_lms_norm_instance_q15;

/* ---- matrix instances: Include/dsp/matrix_functions.h:118-123 (f32), :139-143 (q7),
 * :139-144 (q15), :149-154 (q31) */
typedef struct {
  uint16_t   numRows;
  uint16_t   numCols;
  q7_t      *pData;
} arm_matrix_instance_q7;

typedef struct {
  uint16_t   numRows;
  uint16_t   numCols;
  float32_t *pData;
} arm_matrix_instance_f32;

typedef struct {
  uint16_t   numRows;
  uint16_t   numCols;
  q15_t     *pData;
} arm_matrix_instance_q15;

typedef struct {
  uint16_t   numRows;
  uint16_t   numCols;
  q31_t     *pData;
} arm_matrix_instance_q31;

/* ===================================================================================
 * Complex FFT, f32.  Prototypes: Include/dsp/transform_functions.h:428-460
 * Reference bodies: Source/TransformFunctions/arm_cfft_init_f32.c:121-136,291-354,
 *                   Source/TransformFunctions/arm_cfft_f32.c:1243-1298
 * =================================================================================== */
arm_status arm_cfft_init_4096_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_2048_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_1024_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_512_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_256_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_128_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_64_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_32_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_16_f32(arm_cfft_instance_f32 *S);
arm_status arm_cfft_init_f32(arm_cfft_instance_f32 *S, uint16_t fftLen);
void arm_cfft_f32(const arm_cfft_instance_f32 *S, float32_t *p1,
                  uint8_t ifftFlag, uint8_t bitReverseFlag);

/* ===================================================================================
 * Complex FFT, q31.  Prototypes: Include/dsp/transform_functions.h:364-394
 * Reference bodies: Source/TransformFunctions/arm_cfft_init_q31.c,
 *                   Source/TransformFunctions/arm_cfft_q31.c:704-755
 * =================================================================================== */
arm_status arm_cfft_init_4096_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_2048_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_1024_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_512_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_256_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_128_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_64_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_32_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_16_q31(arm_cfft_instance_q31 *S);
arm_status arm_cfft_init_q31(arm_cfft_instance_q31 *S, uint16_t fftLen);
void arm_cfft_q31(const arm_cfft_instance_q31 *S, q31_t *p1,
                  uint8_t ifftFlag, uint8_t bitReverseFlag);

/* ===================================================================================
 * Complex FFT, q15.  Prototypes: Include/dsp/transform_functions.h:299-331
 * Reference bodies: Source/TransformFunctions/arm_cfft_init_q15.c,
 *                   Source/TransformFunctions/arm_cfft_q15.c:671-722
 * =================================================================================== */
arm_status arm_cfft_init_4096_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_2048_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_1024_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_512_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_256_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_128_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_64_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_32_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_16_q15(arm_cfft_instance_q15 *S);
arm_status arm_cfft_init_q15(arm_cfft_instance_q15 *S, uint16_t fftLen);
void arm_cfft_q15(const arm_cfft_instance_q15 *S, q15_t *p1,
                  uint8_t ifftFlag, uint8_t bitReverseFlag);

/* ===================================================================================
 * Real FFT (fast), f32.  Prototypes: Include/dsp/transform_functions.h:820-849
 * Reference bodies: Source/TransformFunctions/arm_rfft_fast_init_f32.c:228-244,
 *                   Source/TransformFunctions/arm_rfft_fast_f32.c:675-699
 * Note (reference behaviour kept): the forward transform overwrites p.
 * =================================================================================== */
arm_status arm_rfft_fast_init_32_f32(arm_rfft_fast_instance_f32 *S);
arm_status arm_rfft_fast_init_64_f32(arm_rfft_fast_instance_f32 *S);
arm_status arm_rfft_fast_init_128_f32(arm_rfft_fast_instance_f32 *S);
arm_status arm_rfft_fast_init_256_f32(arm_rfft_fast_instance_f32 *S);
arm_status arm_rfft_fast_init_512_f32(arm_rfft_fast_instance_f32 *S);
arm_status arm_rfft_fast_init_1024_f32(arm_rfft_fast_instance_f32 *S);
arm_status arm_rfft_fast_init_2048_f32(arm_rfft_fast_instance_f32 *S);
arm_status arm_rfft_fast_init_4096_f32(arm_rfft_fast_instance_f32 *S);
arm_status arm_rfft_fast_init_f32(arm_rfft_fast_instance_f32 *S, uint16_t fftLen);
void arm_rfft_fast_f32(const arm_rfft_fast_instance_f32 *S, float32_t *p,
                       float32_t *pOut, uint8_t ifftFlag);

/* ===================================================================================
 * Real FFT, q31 / q15.  Prototypes: Include/dsp/transform_functions.h:695-749 (q31),
 * :566-620 (q15).  Reference bodies: Source/TransformFunctions/arm_rfft_init_q31.c:99-124,
 * :429-478, arm_rfft_q31.c:148-183 (+ arm_split_rfft_q31 / arm_split_rifft_q31, scalar
 * branches), arm_rfft_init_q15.c, arm_rfft_q15.c (scalar, !ARM_MATH_DSP branches).
 * Lengths 32 ... 8192.  Forward: pSrc (N words) is overwritten by the inner CFFT, pDst
 * receives 2N words (the full conjugate-symmetric spectrum).  Inverse: pSrc holds the
 * spectrum (words 0 .. N+1 are read), pDst receives N words (<< 1, saturated).
 * =================================================================================== */
#define ARM_MI355X_DECL_RFFT_INIT(N)                                                        \
  arm_status arm_rfft_init_##N##_q31(arm_rfft_instance_q31 *S, uint32_t ifftFlagR,          \
                                     uint32_t bitReverseFlag);                              \
  arm_status arm_rfft_init_##N##_q15(arm_rfft_instance_q15 *S, uint32_t ifftFlagR,          \
                                     uint32_t bitReverseFlag);
ARM_MI355X_DECL_RFFT_INIT(32)
ARM_MI355X_DECL_RFFT_INIT(64)
ARM_MI355X_DECL_RFFT_INIT(128)
ARM_MI355X_DECL_RFFT_INIT(256)
ARM_MI355X_DECL_RFFT_INIT(512)
ARM_MI355X_DECL_RFFT_INIT(1024)
ARM_MI355X_DECL_RFFT_INIT(2048)
ARM_MI355X_DECL_RFFT_INIT(4096)
ARM_MI355X_DECL_RFFT_INIT(8192)
#undef ARM_MI355X_DECL_RFFT_INIT
arm_status arm_rfft_init_q31(arm_rfft_instance_q31 *S, uint32_t fftLenReal, uint32_t ifftFlagR,
                             uint32_t bitReverseFlag);
arm_status arm_rfft_init_q15(arm_rfft_instance_q15 *S, uint32_t fftLenReal, uint32_t ifftFlagR,
                             uint32_t bitReverseFlag);
void arm_rfft_q31(const arm_rfft_instance_q31 *S, q31_t *pSrc, q31_t *pDst);
void arm_rfft_q15(const arm_rfft_instance_q15 *S, q15_t *pSrc, q15_t *pDst);

/* ===================================================================================
 * MFCC, f32.  Prototypes: Include/dsp/transform_functions.h:875-990
 * Reference bodies: Source/TransformFunctions/arm_mfcc_init_f32.c (init by length and
 * generic), Source/TransformFunctions/arm_mfcc_f32.c:83-160 (RFFT-based path).
 * pTmp: 2*fftLen floats as in the reference.  After the call the contents of pSrc and
 * pTmp are unspecified (the reference documents pSrc as modified); Mel filters must lie
 * within bins [0, fftLen/2) -- the reference reads uninitialised pTmp words beyond them.
 * =================================================================================== */
arm_status arm_mfcc_init_32_f32(arm_mfcc_instance_f32 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                                const float32_t *dctCoefs, const uint32_t *filterPos,
                                const uint32_t *filterLengths, const float32_t *filterCoefs,
                                const float32_t *windowCoefs);
arm_status arm_mfcc_init_64_f32(arm_mfcc_instance_f32 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                                const float32_t *dctCoefs, const uint32_t *filterPos,
                                const uint32_t *filterLengths, const float32_t *filterCoefs,
                                const float32_t *windowCoefs);
arm_status arm_mfcc_init_128_f32(arm_mfcc_instance_f32 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                                 const float32_t *dctCoefs, const uint32_t *filterPos,
                                 const uint32_t *filterLengths, const float32_t *filterCoefs,
                                 const float32_t *windowCoefs);
arm_status arm_mfcc_init_256_f32(arm_mfcc_instance_f32 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                                 const float32_t *dctCoefs, const uint32_t *filterPos,
                                 const uint32_t *filterLengths, const float32_t *filterCoefs,
                                 const float32_t *windowCoefs);
arm_status arm_mfcc_init_512_f32(arm_mfcc_instance_f32 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                                 const float32_t *dctCoefs, const uint32_t *filterPos,
                                 const uint32_t *filterLengths, const float32_t *filterCoefs,
                                 const float32_t *windowCoefs);
arm_status arm_mfcc_init_1024_f32(arm_mfcc_instance_f32 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                                  const float32_t *dctCoefs, const uint32_t *filterPos,
                                  const uint32_t *filterLengths, const float32_t *filterCoefs,
                                  const float32_t *windowCoefs);
arm_status arm_mfcc_init_2048_f32(arm_mfcc_instance_f32 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                                  const float32_t *dctCoefs, const uint32_t *filterPos,
                                  const uint32_t *filterLengths, const float32_t *filterCoefs,
                                  const float32_t *windowCoefs);
arm_status arm_mfcc_init_4096_f32(arm_mfcc_instance_f32 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                                  const float32_t *dctCoefs, const uint32_t *filterPos,
                                  const uint32_t *filterLengths, const float32_t *filterCoefs,
                                  const float32_t *windowCoefs);
arm_status arm_mfcc_init_f32(arm_mfcc_instance_f32 *S, uint32_t fftLen, uint32_t nbMelFilters,
                             uint32_t nbDctOutputs, const float32_t *dctCoefs, const uint32_t *filterPos,
                             const uint32_t *filterLengths, const float32_t *filterCoefs,
                             const float32_t *windowCoefs);
void arm_mfcc_f32(const arm_mfcc_instance_f32 *S, float32_t *pSrc, float32_t *pDst, float32_t *pTmp);

/* MFCC q31.  Reference bodies: Source/TransformFunctions/arm_mfcc_init_q31.c (generic and
 * per-length init: RFFT q31 forward with bit reversal), arm_mfcc_q31.c:88-225 (RFFT-based
 * default path; output q8.23).  pSrc and pTmp are work buffers of the reference; the GPU
 * path uses device scratch and leaves them as they were.  Mel filters must lie within the
 * fftLen/2 + 1 spectrum magnitudes (ARM_MATH_ARGUMENT_ERROR otherwise). */
arm_status arm_mfcc_init_q31(arm_mfcc_instance_q31 *S, uint32_t fftLen, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                             const q31_t *dctCoefs, const uint32_t *filterPos, const uint32_t *filterLengths,
                             const q31_t *filterCoefs, const q31_t *windowCoefs);
#define ARM_MI355X_DECL_MFCC_Q31_INIT(N)                                                                    \
  arm_status arm_mfcc_init_##N##_q31(arm_mfcc_instance_q31 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs, \
                                     const q31_t *dctCoefs, const uint32_t *filterPos,                       \
                                     const uint32_t *filterLengths, const q31_t *filterCoefs,                \
                                     const q31_t *windowCoefs);
ARM_MI355X_DECL_MFCC_Q31_INIT(32)
ARM_MI355X_DECL_MFCC_Q31_INIT(64)
ARM_MI355X_DECL_MFCC_Q31_INIT(128)
ARM_MI355X_DECL_MFCC_Q31_INIT(256)
ARM_MI355X_DECL_MFCC_Q31_INIT(512)
ARM_MI355X_DECL_MFCC_Q31_INIT(1024)
ARM_MI355X_DECL_MFCC_Q31_INIT(2048)
ARM_MI355X_DECL_MFCC_Q31_INIT(4096)
#undef ARM_MI355X_DECL_MFCC_Q31_INIT
arm_status arm_mfcc_q31(const arm_mfcc_instance_q31 *S, q31_t *pSrc, q31_t *pDst, q31_t *pTmp);

/* MFCC q15.  Reference bodies: Source/TransformFunctions/arm_mfcc_init_q15.c, arm_mfcc_q15.c:96-228
 * (RFFT-based default path; q15 input, q8.7 output, q31 work buffer).  Same buffer contract as
 * arm_mfcc_q31. */
arm_status arm_mfcc_init_q15(arm_mfcc_instance_q15 *S, uint32_t fftLen, uint32_t nbMelFilters, uint32_t nbDctOutputs,
                             const q15_t *dctCoefs, const uint32_t *filterPos, const uint32_t *filterLengths,
                             const q15_t *filterCoefs, const q15_t *windowCoefs);
#define ARM_MI355X_DECL_MFCC_Q15_INIT(N)                                                                    \
  arm_status arm_mfcc_init_##N##_q15(arm_mfcc_instance_q15 *S, uint32_t nbMelFilters, uint32_t nbDctOutputs, \
                                     const q15_t *dctCoefs, const uint32_t *filterPos,                       \
                                     const uint32_t *filterLengths, const q15_t *filterCoefs,                \
                                     const q15_t *windowCoefs);
ARM_MI355X_DECL_MFCC_Q15_INIT(32)
ARM_MI355X_DECL_MFCC_Q15_INIT(64)
ARM_MI355X_DECL_MFCC_Q15_INIT(128)
ARM_MI355X_DECL_MFCC_Q15_INIT(256)
ARM_MI355X_DECL_MFCC_Q15_INIT(512)
ARM_MI355X_DECL_MFCC_Q15_INIT(1024)
ARM_MI355X_DECL_MFCC_Q15_INIT(2048)
ARM_MI355X_DECL_MFCC_Q15_INIT(4096)
#undef ARM_MI355X_DECL_MFCC_Q15_INIT
arm_status arm_mfcc_q15(const arm_mfcc_instance_q15 *S, q15_t *pSrc, q15_t *pDst, q31_t *pTmp);

/* ===================================================================================
 * FIR.  Prototypes: Include/dsp/filtering_functions.h:141-145,175-180,233-237,260-265
 * Reference bodies: Source/FilteringFunctions/arm_fir_f32.c:911-1280,
 *                   arm_fir_init_f32.c:74-95, arm_fir_q15.c:458-726, arm_fir_init_q15.c:86-139
 * pState holds numTaps+blockSize-1 samples; the last numTaps-1 are carried to the
 * next call (streaming state), as in the reference.
 * =================================================================================== */
void arm_fir_init_f32(arm_fir_instance_f32 *S, uint16_t numTaps,
                      const float32_t *pCoeffs, float32_t *pState, uint32_t blockSize);
void arm_fir_f32(const arm_fir_instance_f32 *S, const float32_t *pSrc,
                 float32_t *pDst, uint32_t blockSize);
arm_status arm_fir_init_q15(arm_fir_instance_q15 *S, uint16_t numTaps,
                            const q15_t *pCoeffs, q15_t *pState, uint32_t blockSize);
void arm_fir_q15(const arm_fir_instance_q15 *S, const q15_t *pSrc,
                 q15_t *pDst, uint32_t blockSize);

/* Further FIR variants.  Prototypes: Include/dsp/filtering_functions.h
 * :154-158 (fast q15), :189-193 (q31), :202-206 (fast q31), :219-224 (init q31).
 * Reference bodies: Source/FilteringFunctions/arm_fir_fast_q15.c (q31_t accumulator, __SMLAD:
 * mod-2^32 sum, __SSAT(acc >> 15, 16)), arm_fir_q31.c (q63 sum of exact products,
 * (q31)(acc >> 31)), arm_fir_fast_q31.c (multAcc_32x32_keep32_R per tap, (q31)(acc << 1)),
 * arm_fir_init_q31.c.  numTaps must be even for the q15 variants, as in the reference. */
void arm_fir_init_q31(arm_fir_instance_q31 *S, uint16_t numTaps,
                      const q31_t *pCoeffs, q31_t *pState, uint32_t blockSize);
void arm_fir_q31(const arm_fir_instance_q31 *S, const q31_t *pSrc,
                 q31_t *pDst, uint32_t blockSize);
void arm_fir_fast_q31(const arm_fir_instance_q31 *S, const q31_t *pSrc,
                      q31_t *pDst, uint32_t blockSize);
void arm_fir_fast_q15(const arm_fir_instance_q15 *S, const q15_t *pSrc,
                      q15_t *pDst, uint32_t blockSize);
/* q7 FIR.  Prototypes: Include/dsp/filtering_functions.h:110-114 (arm_fir_q7), :127-132
 * (arm_fir_init_q7).  Reference bodies: Source/FilteringFunctions/arm_fir_q7.c:446-560 (q31_t
 * accumulator of q7 x q7 products, wrapping int32 adds, __SSAT(acc >> 7, 8)),
 * arm_fir_init_q7.c:67-85 (state numTaps + blockSize - 1 words, zeroed). */
void arm_fir_init_q7(arm_fir_instance_q7 *S, uint16_t numTaps, const q7_t *pCoeffs, q7_t *pState,
                     uint32_t blockSize);
void arm_fir_q7(const arm_fir_instance_q7 *S, const q7_t *pSrc, q7_t *pDst, uint32_t blockSize);

/* ===================================================================================
 * Multirate FIR.  Prototypes: Include/dsp/filtering_functions.h:886-1007 (decimators),
 * :1050-1150 (interpolators).  Reference bodies: Source/FilteringFunctions/
 * arm_fir_decimate_{f32,q15,fast_q15,q31,fast_q31}.c and arm_fir_interpolate_{f32,q15,q31}.c
 * (generic C paths), arm_fir_decimate_init_*.c (ARM_MATH_LENGTH_ERROR unless blockSize % M
 * == 0; state numTaps + blockSize - 1 words), arm_fir_interpolate_init_*.c
 * (ARM_MATH_LENGTH_ERROR unless numTaps % L == 0; phaseLength = numTaps / L; state
 * blockSize + phaseLength - 1 words).  Decimator output j = sum_t s[M j + t] h[t] (blockSize / M
 * outputs); interpolator output n L + q = sum_i s[n + i] h[(L-1-q) + i L] (blockSize L outputs);
 * s = [history ; block].  Accumulators: f32 mul then add, q15 / q31 q63 sums (__SSAT(>> 15) /
 * >> 31), fast q15 a wrapping q31 sum with __SSAT(>> 15), fast q31 acc + floor(x h / 2^32)
 * (no rounding term), output << 1.  M == 0 / L == 0 return ARM_MATH_LENGTH_ERROR (the
 * reference divides by zero).
 * =================================================================================== */
arm_status arm_fir_decimate_init_f32(arm_fir_decimate_instance_f32 *S, uint16_t numTaps, uint8_t M,
                                     const float32_t *pCoeffs, float32_t *pState, uint32_t blockSize);
arm_status arm_fir_decimate_init_q15(arm_fir_decimate_instance_q15 *S, uint16_t numTaps, uint8_t M,
                                     const q15_t *pCoeffs, q15_t *pState, uint32_t blockSize);
arm_status arm_fir_decimate_init_q31(arm_fir_decimate_instance_q31 *S, uint16_t numTaps, uint8_t M,
                                     const q31_t *pCoeffs, q31_t *pState, uint32_t blockSize);
void arm_fir_decimate_f32(const arm_fir_decimate_instance_f32 *S, const float32_t *pSrc, float32_t *pDst,
                          uint32_t blockSize);
void arm_fir_decimate_q15(const arm_fir_decimate_instance_q15 *S, const q15_t *pSrc, q15_t *pDst,
                          uint32_t blockSize);
void arm_fir_decimate_fast_q15(const arm_fir_decimate_instance_q15 *S, const q15_t *pSrc, q15_t *pDst,
                               uint32_t blockSize);
void arm_fir_decimate_q31(const arm_fir_decimate_instance_q31 *S, const q31_t *pSrc, q31_t *pDst,
                          uint32_t blockSize);
void arm_fir_decimate_fast_q31(const arm_fir_decimate_instance_q31 *S, const q31_t *pSrc, q31_t *pDst,
                               uint32_t blockSize);
arm_status arm_fir_interpolate_init_f32(arm_fir_interpolate_instance_f32 *S, uint8_t L, uint16_t numTaps,
                                        const float32_t *pCoeffs, float32_t *pState, uint32_t blockSize);
arm_status arm_fir_interpolate_init_q15(arm_fir_interpolate_instance_q15 *S, uint8_t L, uint16_t numTaps,
                                        const q15_t *pCoeffs, q15_t *pState, uint32_t blockSize);
arm_status arm_fir_interpolate_init_q31(arm_fir_interpolate_instance_q31 *S, uint8_t L, uint16_t numTaps,
                                        const q31_t *pCoeffs, q31_t *pState, uint32_t blockSize);
void arm_fir_interpolate_f32(const arm_fir_interpolate_instance_f32 *S, const float32_t *pSrc, float32_t *pDst,
                             uint32_t blockSize);
void arm_fir_interpolate_q15(const arm_fir_interpolate_instance_q15 *S, const q15_t *pSrc, q15_t *pDst,
                             uint32_t blockSize);
void arm_fir_interpolate_q31(const arm_fir_interpolate_instance_q31 *S, const q31_t *pSrc, q31_t *pDst,
                             uint32_t blockSize);

/* ===================================================================================
 * Sparse FIR (widening).  Prototypes: Include/dsp/filtering_functions.h:2094-2231.  Reference
 * bodies: Source/FilteringFunctions/arm_fir_sparse_{f32,q31,q15,q7}.c, inits
 * arm_fir_sparse_init_*.c.  y[n] = sum over k ascending of x[n - pTapDelay[k]] pCoeffs[k]:
 * f32 first tap x c, then mul-then-add; q31 (q31)((q63 x c) >> 32) terms summed with wrap,
 * output << 1; q15 / q7 q31 product sums (wrap) then __SSAT(>> 15, 16) / __SSAT(>> 7, 8).
 * The block is written into the circular pState at stateIndex and every tap read back from it
 * at the reference's indices, so the state and stateIndex evolve exactly as the reference's.
 * pScratchIn / pScratchOut are accepted and not used.  numTaps == 1 is one product per output
 * (the reference's numTaps - 2 tap loop counter underflows there).
 * =================================================================================== */
void arm_fir_sparse_init_f32(arm_fir_sparse_instance_f32 *S, uint16_t numTaps, const float32_t *pCoeffs,
                             float32_t *pState, int32_t *pTapDelay, uint16_t maxDelay, uint32_t blockSize);
void arm_fir_sparse_init_q31(arm_fir_sparse_instance_q31 *S, uint16_t numTaps, const q31_t *pCoeffs, q31_t *pState,
                             int32_t *pTapDelay, uint16_t maxDelay, uint32_t blockSize);
void arm_fir_sparse_init_q15(arm_fir_sparse_instance_q15 *S, uint16_t numTaps, const q15_t *pCoeffs, q15_t *pState,
                             int32_t *pTapDelay, uint16_t maxDelay, uint32_t blockSize);
void arm_fir_sparse_init_q7(arm_fir_sparse_instance_q7 *S, uint16_t numTaps, const q7_t *pCoeffs, q7_t *pState,
                            int32_t *pTapDelay, uint16_t maxDelay, uint32_t blockSize);
void arm_fir_sparse_f32(arm_fir_sparse_instance_f32 *S, const float32_t *pSrc, float32_t *pDst,
                        float32_t *pScratchIn, uint32_t blockSize);
void arm_fir_sparse_q31(arm_fir_sparse_instance_q31 *S, const q31_t *pSrc, q31_t *pDst, q31_t *pScratchIn,
                        uint32_t blockSize);
void arm_fir_sparse_q15(arm_fir_sparse_instance_q15 *S, const q15_t *pSrc, q15_t *pDst, q15_t *pScratchIn,
                        q31_t *pScratchOut, uint32_t blockSize);
void arm_fir_sparse_q7(arm_fir_sparse_instance_q7 *S, const q7_t *pSrc, q7_t *pDst, q7_t *pScratchIn,
                       q31_t *pScratchOut, uint32_t blockSize);

/* ===================================================================================
 * FIR lattice (widening).  Prototypes: Include/dsp/filtering_functions.h:1350-1410.
 * Reference bodies: Source/FilteringFunctions/arm_fir_lattice_{f32,q31,q15}.c, inits
 * arm_fir_lattice_init_*.c (zero numStages state words).  f_m(n) = g_{m-1}(n-1) k_m +
 * f_{m-1}(n), g_m(n) = f_{m-1}(n) k_m + g_{m-1}(n-1), y = f_M: f32 mul then add; q31
 * ((q31)((q63 a k) >> 32) << 1) + b with wrap; q15 __SSAT(((a k) >> 15) + b, 16).
 * =================================================================================== */
void arm_fir_lattice_init_f32(arm_fir_lattice_instance_f32 *S, uint16_t numStages, const float32_t *pCoeffs,
                              float32_t *pState);
void arm_fir_lattice_init_q31(arm_fir_lattice_instance_q31 *S, uint16_t numStages, const q31_t *pCoeffs,
                              q31_t *pState);
void arm_fir_lattice_init_q15(arm_fir_lattice_instance_q15 *S, uint16_t numStages, const q15_t *pCoeffs,
                              q15_t *pState);
void arm_fir_lattice_f32(const arm_fir_lattice_instance_f32 *S, const float32_t *pSrc, float32_t *pDst,
                         uint32_t blockSize);
void arm_fir_lattice_q31(const arm_fir_lattice_instance_q31 *S, const q31_t *pSrc, q31_t *pDst, uint32_t blockSize);
void arm_fir_lattice_q15(const arm_fir_lattice_instance_q15 *S, const q15_t *pSrc, q15_t *pDst, uint32_t blockSize);

/* ===================================================================================
 * Biquad cascades.  Prototypes: Include/dsp/filtering_functions.h:331-441, :1163-1182, :1223-1295.
 * Reference bodies: Source/FilteringFunctions/arm_biquad_cascade_df1_{f32,q31,fast_q31,q15,fast_q15}.c,
 * arm_biquad_cascade_df1_32x64_q31.c, arm_biquad_cascade_df2T_f32.c, arm_biquad_cascade_stereo_df2T_f32.c
 * (scalar path); the inits set the fields and zero the state.  Stages run in order, the first from
 * pSrc and the rest in place over pDst (pSrc == pDst is allowed); the state is read before the
 * block and written after it.  Stereo: pSrc / pDst hold 2*blockSize interleaved words.
 * =================================================================================== */
void arm_biquad_cascade_df1_init_f32(arm_biquad_casd_df1_inst_f32 *S, uint8_t numStages, const float32_t *pCoeffs,
                                     float32_t *pState);
void arm_biquad_cascade_df1_f32(const arm_biquad_casd_df1_inst_f32 *S, const float32_t *pSrc, float32_t *pDst,
                                uint32_t blockSize);
void arm_biquad_cascade_df1_init_q31(arm_biquad_casd_df1_inst_q31 *S, uint8_t numStages, const q31_t *pCoeffs,
                                     q31_t *pState, int8_t postShift);
void arm_biquad_cascade_df1_q31(const arm_biquad_casd_df1_inst_q31 *S, const q31_t *pSrc, q31_t *pDst,
                                uint32_t blockSize);
void arm_biquad_cascade_df1_fast_q31(const arm_biquad_casd_df1_inst_q31 *S, const q31_t *pSrc, q31_t *pDst,
                                     uint32_t blockSize);
void arm_biquad_cascade_df1_init_q15(arm_biquad_casd_df1_inst_q15 *S, uint8_t numStages, const q15_t *pCoeffs,
                                     q15_t *pState, int8_t postShift);
void arm_biquad_cascade_df1_q15(const arm_biquad_casd_df1_inst_q15 *S, const q15_t *pSrc, q15_t *pDst,
                                uint32_t blockSize);
void arm_biquad_cascade_df1_fast_q15(const arm_biquad_casd_df1_inst_q15 *S, const q15_t *pSrc, q15_t *pDst,
                                     uint32_t blockSize);
void arm_biquad_cas_df1_32x64_init_q31(arm_biquad_cas_df1_32x64_ins_q31 *S, uint8_t numStages, const q31_t *pCoeffs,
                                       q63_t *pState, uint8_t postShift);
void arm_biquad_cas_df1_32x64_q31(const arm_biquad_cas_df1_32x64_ins_q31 *S, const q31_t *pSrc, q31_t *pDst,
                                  uint32_t blockSize);
void arm_biquad_cascade_df2T_init_f32(arm_biquad_cascade_df2T_instance_f32 *S, uint8_t numStages,
                                      const float32_t *pCoeffs, float32_t *pState);
void arm_biquad_cascade_df2T_f32(const arm_biquad_cascade_df2T_instance_f32 *S, const float32_t *pSrc,
                                 float32_t *pDst, uint32_t blockSize);
void arm_biquad_cascade_stereo_df2T_init_f32(arm_biquad_cascade_stereo_df2T_instance_f32 *S, uint8_t numStages,
                                             const float32_t *pCoeffs, float32_t *pState);
void arm_biquad_cascade_stereo_df2T_f32(const arm_biquad_cascade_stereo_df2T_instance_f32 *S, const float32_t *pSrc,
                                        float32_t *pDst, uint32_t blockSize);

/* ===================================================================================
 * IIR lattice.  Prototypes: Include/dsp/filtering_functions.h:1468-1554.  Reference bodies:
 * Source/FilteringFunctions/arm_iir_lattice_{f32,q31,q15}.c (scalar path); the inits set the fields
 * and zero numStages + blockSize state words.  pDst == pSrc is allowed.  After a call the first
 * numStages state words are the reference's; the remaining blockSize words are its scratch and are
 * left as they were.
 * =================================================================================== */
void arm_iir_lattice_init_f32(arm_iir_lattice_instance_f32 *S, uint16_t numStages, float32_t *pkCoeffs,
                              float32_t *pvCoeffs, float32_t *pState, uint32_t blockSize);
void arm_iir_lattice_f32(const arm_iir_lattice_instance_f32 *S, const float32_t *pSrc, float32_t *pDst,
                         uint32_t blockSize);
void arm_iir_lattice_init_q31(arm_iir_lattice_instance_q31 *S, uint16_t numStages, q31_t *pkCoeffs, q31_t *pvCoeffs,
                              q31_t *pState, uint32_t blockSize);
void arm_iir_lattice_q31(const arm_iir_lattice_instance_q31 *S, const q31_t *pSrc, q31_t *pDst, uint32_t blockSize);
void arm_iir_lattice_init_q15(arm_iir_lattice_instance_q15 *S, uint16_t numStages, q15_t *pkCoeffs, q15_t *pvCoeffs,
                              q15_t *pState, uint32_t blockSize);
void arm_iir_lattice_q15(const arm_iir_lattice_instance_q15 *S, const q15_t *pSrc, q15_t *pDst, uint32_t blockSize);

/* ===================================================================================
 * LMS and normalised LMS adaptive filters.  Prototypes: filtering_functions.h:1578-1704, :1730-1762,
 * :1836-1864.  Reference bodies: Source/FilteringFunctions/arm_lms_{f32,q31,q15}.c,
 * arm_lms_norm_{f32,q15}.c (scalar path); the inits set the fields and zero numTaps + blockSize - 1
 * state words.  S->pCoeffs is updated in place; the normalised kinds write S->energy and S->x0 back.
 * pOut == pSrc and pErr == pRef are allowed.  A postShift for which the reference's shift counts leave
 * 0...31 (q15: > 14, q31: > 30) is refused through arm_mi355x_last_error.  arm_lms_norm_q31 is not
 * provided.
 * =================================================================================== */
void arm_lms_init_f32(arm_lms_instance_f32 *S, uint16_t numTaps, float32_t *pCoeffs, float32_t *pState, float32_t mu,
                      uint32_t blockSize);
void arm_lms_f32(const arm_lms_instance_f32 *S, const float32_t *pSrc, float32_t *pRef, float32_t *pOut,
                 float32_t *pErr, uint32_t blockSize);
void arm_lms_init_q31(arm_lms_instance_q31 *S, uint16_t numTaps, q31_t *pCoeffs, q31_t *pState, q31_t mu,
                      uint32_t blockSize, uint32_t postShift);
void arm_lms_q31(const arm_lms_instance_q31 *S, const q31_t *pSrc, q31_t *pRef, q31_t *pOut, q31_t *pErr,
                 uint32_t blockSize);
void arm_lms_init_q15(arm_lms_instance_q15 *S, uint16_t numTaps, q15_t *pCoeffs, q15_t *pState, q15_t mu,
                      uint32_t blockSize, uint32_t postShift);
void arm_lms_q15(const arm_lms_instance_q15 *S, const q15_t *pSrc, q15_t *pRef, q15_t *pOut, q15_t *pErr,
                 uint32_t blockSize);
void arm_lms_norm_init_f32(arm_lms_norm_instance_f32 *S, uint16_t numTaps, float32_t *pCoeffs, float32_t *pState,
                           float32_t mu, uint32_t blockSize);
void arm_lms_norm_f32(arm_lms_norm_instance_f32 *S, const float32_t *pSrc, float32_t *pRef, float32_t *pOut,
                      float32_t *pErr, uint32_t blockSize);
void arm_lms_norm_init_q15(arm_lms_norm_instance_q15 *S, uint16_t numTaps, q15_t *pCoeffs, q15_t *pState, q15_t mu,
                           uint32_t blockSize, uint8_t postShift);
void arm_lms_norm_q15(arm_lms_norm_instance_q15 *S, const q15_t *pSrc, q15_t *pRef, q15_t *pOut, q15_t *pErr,
                      uint32_t blockSize);

/* ===================================================================================
 * Convolution.  Prototypes: Include/dsp/filtering_functions.h
 * (arm_conv_f32 / _q15 / _q31).  Reference bodies: Source/FilteringFunctions/arm_conv_f32.c
 * (per output a sum over the overlap from 0.0f in ascending index of pSrcA, mul then add), arm_conv_q15.c (!ARM_MATH_DSP: q63 sum,
 * __SSAT(sum >> 15, 16)), arm_conv_q31.c (q63 sum, (q31)(sum >> 31)).  pDst holds
 * srcALen + srcBLen - 1 samples.
 * =================================================================================== */
void arm_conv_f32(const float32_t *pSrcA, uint32_t srcALen, const float32_t *pSrcB, uint32_t srcBLen,
                  float32_t *pDst);
void arm_conv_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen, q15_t *pDst);
void arm_conv_q31(const q31_t *pSrcA, uint32_t srcALen, const q31_t *pSrcB, uint32_t srcBLen, q31_t *pDst);

/* Fast fixed-point convolution (filtering_functions.h:503,555; arm_conv_fast_q15.c,
 * arm_conv_fast_q31.c): modular q31_t accumulators.  q15: __SMLAD sums, (q15)(sum >> 15),
 * including the reference's single-sample __SMLAD high-halfword term (+1 per MAC with both
 * samples negative in its stage-1/stage-3 remainder loops); q31: sum of (x*y) >> 32, output
 * sum << 1. */
void arm_conv_fast_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen, q15_t *pDst);
void arm_conv_fast_q31(const q31_t *pSrcA, uint32_t srcALen, const q31_t *pSrcB, uint32_t srcBLen, q31_t *pDst);

/* Partial convolution (filtering_functions.h:610,656,723; arm_conv_partial_{f32,q15,q31}.c
 * !ARM_MATH_DSP branch): outputs firstIndex .. firstIndex + numPoints - 1 of arm_conv_*,
 * written at pDst[firstIndex ...]; ARM_MATH_ARGUMENT_ERROR when firstIndex + numPoints >
 * srcALen + srcBLen - 1. */
arm_status arm_conv_partial_f32(const float32_t *pSrcA, uint32_t srcALen, const float32_t *pSrcB, uint32_t srcBLen,
                                float32_t *pDst, uint32_t firstIndex, uint32_t numPoints);
arm_status arm_conv_partial_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen,
                                q15_t *pDst, uint32_t firstIndex, uint32_t numPoints);
arm_status arm_conv_partial_q31(const q31_t *pSrcA, uint32_t srcALen, const q31_t *pSrcB, uint32_t srcBLen,
                                q31_t *pDst, uint32_t firstIndex, uint32_t numPoints);
/* filtering_functions.h:677,744 (arm_conv_partial_fast_q15.c / _q31.c): words firstIndex ..
 * firstIndex + numPoints - 1 of arm_conv_fast_q15 / _q31.  The reference's bodies read
 * outside the inputs for most ranges on the host build (segfault), so parity is pinned to
 * arm_conv_fast_* over the range. */
arm_status arm_conv_partial_fast_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen,
                                     q15_t *pDst, uint32_t firstIndex, uint32_t numPoints);
arm_status arm_conv_partial_fast_q31(const q31_t *pSrcA, uint32_t srcALen, const q31_t *pSrcB, uint32_t srcBLen,
                                     q31_t *pDst, uint32_t firstIndex, uint32_t numPoints);

/* Correlation (filtering_functions.h:1873,1923,1939,1973,1989; arm_correlate_f32.c:1013-1096,
 * arm_correlate_q15.c:814-895, arm_correlate_q31.c, arm_correlate_fast_q15.c,
 * arm_correlate_fast_q31.c).  pDst has 2 * max(srcALen, srcBLen) - 1 words; the
 * srcALen + srcBLen - 1 computed ones are written from pDst[srcALen - srcBLen] forward, or,
 * when srcALen < srcBLen, from pDst[srcALen + srcBLen - 2] backward; the others are left
 * untouched (the reference asks the caller to zero pDst). */
void arm_correlate_f32(const float32_t *pSrcA, uint32_t srcALen, const float32_t *pSrcB, uint32_t srcBLen,
                       float32_t *pDst);
void arm_correlate_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen, q15_t *pDst);
void arm_correlate_q31(const q31_t *pSrcA, uint32_t srcALen, const q31_t *pSrcB, uint32_t srcBLen, q31_t *pDst);
void arm_correlate_fast_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen, q15_t *pDst);
void arm_correlate_fast_q31(const q31_t *pSrcA, uint32_t srcALen, const q31_t *pSrcB, uint32_t srcBLen, q31_t *pDst);

/* q7 convolution family.  Prototypes: Include/dsp/filtering_functions.h:591-596
 * (arm_conv_q7), :790-797 (arm_conv_partial_q7), :2025-2030 (arm_correlate_q7).  Reference
 * bodies: Source/FilteringFunctions/arm_conv_q7.c, arm_conv_partial_q7.c (!ARM_MATH_DSP,
 * :688-735), arm_correlate_q7.c: q31_t sum of q7 x q7 products (int32 adds and __SMLAD pairs,
 * both wrapping: a modular sum), __SSAT(sum >> 7, 8).  Output placement as the q15 forms. */
void arm_conv_q7(const q7_t *pSrcA, uint32_t srcALen, const q7_t *pSrcB, uint32_t srcBLen, q7_t *pDst);
arm_status arm_conv_partial_q7(const q7_t *pSrcA, uint32_t srcALen, const q7_t *pSrcB, uint32_t srcBLen,
                               q7_t *pDst, uint32_t firstIndex, uint32_t numPoints);
void arm_correlate_q7(const q7_t *pSrcA, uint32_t srcALen, const q7_t *pSrcB, uint32_t srcBLen, q7_t *pDst);

/* Scratch-buffer ("_opt") forms.  Prototypes: Include/dsp/filtering_functions.h:469-476,
 * :521-528, :573-580, :633-642, :700-709, :767-776, :1906-1912, :1956-1962, :2007-2014.
 * Reference bodies: Source/FilteringFunctions/arm_conv_opt_q15.c, arm_conv_opt_q7.c,
 * arm_conv_fast_opt_q15.c, arm_conv_partial_opt_q15.c, arm_conv_partial_opt_q7.c,
 * arm_conv_partial_fast_opt_q15.c, arm_correlate_opt_q15.c, arm_correlate_opt_q7.c,
 * arm_correlate_fast_opt_q15.c.  The exact forms return the plain functions' words; the fast
 * q15 forms are a modular q31 sum with __SSAT(acc >> 15, 16) (arm_conv_fast_q15 casts
 * instead).  The scratch buffers may be NULL: the GPU path does not use them.  (The exact q15
 * forms accumulate exactly, as the Arm SMLALD instruction does; the reference's host C
 * emulation of __SMLALD, Include/dsp/none.h:503-505, wraps a pair of two (-32768)^2 products
 * in int32.) */
void arm_conv_opt_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen, q15_t *pDst,
                      q15_t *pScratch1, q15_t *pScratch2);
void arm_conv_fast_opt_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen, q15_t *pDst,
                           q15_t *pScratch1, q15_t *pScratch2);
void arm_conv_opt_q7(const q7_t *pSrcA, uint32_t srcALen, const q7_t *pSrcB, uint32_t srcBLen, q7_t *pDst,
                     q15_t *pScratch1, q15_t *pScratch2);
arm_status arm_conv_partial_opt_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen,
                                    q15_t *pDst, uint32_t firstIndex, uint32_t numPoints, q15_t *pScratch1,
                                    q15_t *pScratch2);
arm_status arm_conv_partial_fast_opt_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen,
                                         q15_t *pDst, uint32_t firstIndex, uint32_t numPoints, q15_t *pScratch1,
                                         q15_t *pScratch2);
arm_status arm_conv_partial_opt_q7(const q7_t *pSrcA, uint32_t srcALen, const q7_t *pSrcB, uint32_t srcBLen,
                                   q7_t *pDst, uint32_t firstIndex, uint32_t numPoints, q15_t *pScratch1,
                                   q15_t *pScratch2);
void arm_correlate_opt_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen, q15_t *pDst,
                           q15_t *pScratch);
void arm_correlate_fast_opt_q15(const q15_t *pSrcA, uint32_t srcALen, const q15_t *pSrcB, uint32_t srcBLen,
                                q15_t *pDst, q15_t *pScratch);
void arm_correlate_opt_q7(const q7_t *pSrcA, uint32_t srcALen, const q7_t *pSrcB, uint32_t srcBLen, q7_t *pDst,
                          q15_t *pScratch1, q15_t *pScratch2);

/* ===================================================================================
 * Matrix multiply, f32.  Prototypes: Include/dsp/matrix_functions.h:341-344,630-634
 * Reference bodies: Source/MatrixFunctions/arm_mat_mult_f32.c:600-730,
 *                   Source/MatrixFunctions/arm_mat_init_f32.c
 * Size check: always performed (the reference checks only under ARM_MATH_MATRIX_CHECK,
 * arm_mat_mult_f32.c:618-630; a mismatched call is undefined there).
 * =================================================================================== */
void arm_mat_init_f32(arm_matrix_instance_f32 *S, uint16_t nRows, uint16_t nColumns,
                      float32_t *pData);
arm_status arm_mat_mult_f32(const arm_matrix_instance_f32 *pSrcA,
                            const arm_matrix_instance_f32 *pSrcB,
                            arm_matrix_instance_f32 *pDst);

/* Matrix multiply q15 / q31.  Prototypes: Include/dsp/matrix_functions.h
 * (arm_mat_mult_q15 with its pState transpose buffer, arm_mat_mult_q31, arm_mat_init_q15/_q31).
 * Reference bodies: Source/MatrixFunctions/arm_mat_mult_q15.c:741-912 (!ARM_MATH_DSP: q63
 * sum of exact products, __SSAT(sum >> 15, 16)), arm_mat_mult_q31.c:53-163 (q63 sum,
 * (q31)(sum >> 31)).  Bit-exact; pState is accepted and unused.  Size check always on. */
void arm_mat_init_q15(arm_matrix_instance_q15 *S, uint16_t nRows, uint16_t nColumns, q15_t *pData);
/* q7: matrix_functions.h:379-383 (arm_mat_mult_q7), :617-621 (arm_mat_init_q7); body
 * Source/MatrixFunctions/arm_mat_mult_q7.c:689-790 (scalar branch: q31_t sum of exact products,
 * (q7)__SSAT(sum >> 7, 8)), Source/MatrixFunctions/arm_mat_init_q7.c.  Bit-exact on one i8 MFMA
 * plane; pState is accepted and unused. */
void arm_mat_init_q7(arm_matrix_instance_q7 *S, uint16_t nRows, uint16_t nColumns, q7_t *pData);
arm_status arm_mat_mult_q7(const arm_matrix_instance_q7 *pSrcA, const arm_matrix_instance_q7 *pSrcB,
                           arm_matrix_instance_q7 *pDst, q7_t *pState);
void arm_mat_init_q31(arm_matrix_instance_q31 *S, uint16_t nRows, uint16_t nColumns, q31_t *pData);
arm_status arm_mat_mult_q15(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                            arm_matrix_instance_q15 *pDst, q15_t *pState);
arm_status arm_mat_mult_q31(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                            arm_matrix_instance_q31 *pDst);
/* matrix_functions.h:459-463.  The scalar branch of Source/MatrixFunctions/arm_mat_mult_opt_q31.c:
 * 648-780 is arm_mat_mult_q31's (q63 sum of exact products, (q31)(sum >> 31)) with an unused
 * pState, so this runs the same bit-exact i8-plane GEMM. */
arm_status arm_mat_mult_opt_q31(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                                arm_matrix_instance_q31 *pDst, q31_t *pState);
/* Fast fixed-point matrix multiply (matrix_functions.h:431-435,484-487):
 * arm_mat_mult_fast_q15.c (!ARM_MATH_DSP): q31_t modular sum of q15 products, (q15)(sum >> 15);
 * arm_mat_mult_fast_q31.c: sum = (q31)(((q63)sum << 32 + a*b) >> 32) per product, output
 * sum << 1.  pState (the reference's transpose buffer) is not used. */
arm_status arm_mat_mult_fast_q15(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                                 arm_matrix_instance_q15 *pDst, q15_t *pState);
arm_status arm_mat_mult_fast_q31(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                                 arm_matrix_instance_q31 *pDst);

/* Complex matrix multiply (matrix_functions.h: arm_mat_cmplx_mult_f32 / _q15 / _q31).  numRows and
 * numCols count complex elements; pData holds interleaved (re, im) words.  Bodies:
 * Source/MatrixFunctions/arm_mat_cmplx_mult_q15.c:433-582 (!ARM_MATH_DSP: q63 sums of exact
 * products, __SSAT(sum >> 15, 16); pScratch, host or device, receives B transposed (numColsB rows of
 * numRowsB complex words) as the reference leaves it, NULL is tolerated),
 * arm_mat_cmplx_mult_q31.c:836-1057 (q63 sums wrapping mod 2^64, clip_q63_to_q31(sum >> 31)): both
 * bit-exact.  arm_mat_cmplx_mult_f32.c:1225-1392: the k-ascending fmaf chain
 * re = fma(-b, d, fma(a, c, re)), im = fma(b, c, fma(a, d, im)) from +0, within
 * 2K 2^-24 (|A||B'|)ij of the exact product (finite inputs; DESIGN.md, complex matrix multiply).
 * Size check always on. */
arm_status arm_mat_cmplx_mult_f32(const arm_matrix_instance_f32 *pSrcA, const arm_matrix_instance_f32 *pSrcB,
                                  arm_matrix_instance_f32 *pDst);
arm_status arm_mat_cmplx_mult_q15(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                                  arm_matrix_instance_q15 *pDst, q15_t *pScratch);
arm_status arm_mat_cmplx_mult_q31(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                                  arm_matrix_instance_q31 *pDst);

/* Inverse, Cholesky, LDLT and triangular solves (matrix_functions.h:659-777, groups MatrixInv and
 * MatrixChol), bit-exact with the reference's scalar branches: the status and the words an early return
 * leaves included.  Host or device pData (and pp), synchronous.
 *   arm_mat_inverse_f32   Gauss-Jordan with the reference's pivot rule.  pSrc is destroyed as there (its final
 *                         words are written back); ARM_MATH_SINGULAR on a zero pivot, with both matrices as
 *                         they stand at that moment.
 *   arm_mat_cholesky_f32  writes the lower triangle of pDst only; ARM_MATH_DECOMPOSITION_FAILURE at the first
 *                         diagonal <= 0 (that column unscaled, later columns untouched).  pDst->pData may be
 *                         pSrc->pData.
 *   arm_mat_ldlt_f32      P A P^T = L D L^T as the reference computes it (pivot rule, 1.0e-8f rank cut and
 *                         its diag = k - 1 included); always ARM_MATH_SUCCESS.
 *   arm_mat_solve_{lower,upper}_triangular_f32   dst (n x cols) from lt / ut (n x n) and a (n x cols);
 *                         ARM_MATH_SINGULAR at a zero diagonal (then only column 0's earlier rows are
 *                         written).  dst->pData may be a->pData.
 * ARM_MATH_SIZE_MISMATCH on the shapes the reference rejects under ARM_MATH_MATRIX_CHECK (always on here) and
 * when a and dst differ; ARM_MATH_ARGUMENT_ERROR on a null pointer.  Any overlap but the two exact aliases
 * named above is undefined. */
arm_status arm_mat_inverse_f32(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pDst);
arm_status arm_mat_cholesky_f32(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pDst);
arm_status arm_mat_ldlt_f32(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pl,
                            arm_matrix_instance_f32 *pd, uint16_t *pp);
arm_status arm_mat_solve_lower_triangular_f32(const arm_matrix_instance_f32 *lt, const arm_matrix_instance_f32 *a,
                                              arm_matrix_instance_f32 *dst);
arm_status arm_mat_solve_upper_triangular_f32(const arm_matrix_instance_f32 *ut, const arm_matrix_instance_f32 *a,
                                              arm_matrix_instance_f32 *dst);

/* Element-wise add, sub and scale, the transposes and matrix x vector (matrix_functions.h groups MatrixAdd,
 * MatrixSub, MatrixScale, MatrixTrans, MatrixComplexTrans, and arm_mat_vec_mult_* of MatrixMult), bit-exact
 * with the reference's scalar branches.  Host or device pData / pVec / pDst, synchronous.
 *   add / sub   f32: one IEEE operation per word; q31: saturating (__QADD / __QSUB); q15: __SSAT(a +- b, 16).
 *   scale       f32: x * scale.  q31: in = (q31_t)(((q63_t)x * scaleFract) >> 32), out = in << (shift + 1) with
 *               saturation; -1 <= shift <= 30.  q15: __SSAT(((q31_t)x * scaleFract) >> (15 - shift), 16);
 *               -16 <= shift <= 15.  A shift outside these ranges (a negative or too large shift count in the
 *               reference) returns ARM_MATH_ARGUMENT_ERROR and leaves pDst alone.
 *   trans / cmplx_trans   pure data movement; the complex forms count (re, im) pairs in numRows / numCols and
 *               do not conjugate.
 *   vec_mult    pDst[r] = sum_k pSrcMat[r][k] pVec[k], k ascending.  f32: product and sum rounded separately;
 *               q31: the sum mod 2^64, >> 31, not saturated; q15: a q63 sum of __SMLALD pairs,
 *               __SSAT(sum >> 15, 16); q7: __SSAT(sum >> 7, 8).  q15 and q31 keep the reference's uint16_t row
 *               offset: past 65535 elements into the matrix a row is read from its offset mod 65536
 *               (INTEGRATION.md).  A null pointer: no work, arm_mi355x_last_error() set.
 * ARM_MATH_SIZE_MISMATCH on the shapes the reference rejects under ARM_MATH_MATRIX_CHECK (always on here: add /
 * sub three equal shapes, scale two, a transpose's pDst the swapped shape); ARM_MATH_ARGUMENT_ERROR on a null
 * pointer; a zero dimension is a successful no-op (vec_mult with numCols == 0 stores the empty sums, zeros, as the
 * reference does).  pDst->pData of add / sub / scale may equal a source's pData exactly; any other overlap is
 * undefined (it does not fault). */
arm_status arm_mat_add_f32(const arm_matrix_instance_f32 *pSrcA, const arm_matrix_instance_f32 *pSrcB,
                           arm_matrix_instance_f32 *pDst);
arm_status arm_mat_add_q31(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                           arm_matrix_instance_q31 *pDst);
arm_status arm_mat_add_q15(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                           arm_matrix_instance_q15 *pDst);
arm_status arm_mat_sub_f32(const arm_matrix_instance_f32 *pSrcA, const arm_matrix_instance_f32 *pSrcB,
                           arm_matrix_instance_f32 *pDst);
arm_status arm_mat_sub_q31(const arm_matrix_instance_q31 *pSrcA, const arm_matrix_instance_q31 *pSrcB,
                           arm_matrix_instance_q31 *pDst);
arm_status arm_mat_sub_q15(const arm_matrix_instance_q15 *pSrcA, const arm_matrix_instance_q15 *pSrcB,
                           arm_matrix_instance_q15 *pDst);
arm_status arm_mat_scale_f32(const arm_matrix_instance_f32 *pSrc, float32_t scale, arm_matrix_instance_f32 *pDst);
arm_status arm_mat_scale_q31(const arm_matrix_instance_q31 *pSrc, q31_t scaleFract, int32_t shift,
                             arm_matrix_instance_q31 *pDst);
arm_status arm_mat_scale_q15(const arm_matrix_instance_q15 *pSrc, q15_t scaleFract, int32_t shift,
                             arm_matrix_instance_q15 *pDst);
arm_status arm_mat_trans_f32(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pDst);
arm_status arm_mat_trans_q31(const arm_matrix_instance_q31 *pSrc, arm_matrix_instance_q31 *pDst);
arm_status arm_mat_trans_q15(const arm_matrix_instance_q15 *pSrc, arm_matrix_instance_q15 *pDst);
arm_status arm_mat_trans_q7(const arm_matrix_instance_q7 *pSrc, arm_matrix_instance_q7 *pDst);
arm_status arm_mat_cmplx_trans_f32(const arm_matrix_instance_f32 *pSrc, arm_matrix_instance_f32 *pDst);
arm_status arm_mat_cmplx_trans_q31(const arm_matrix_instance_q31 *pSrc, arm_matrix_instance_q31 *pDst);
arm_status arm_mat_cmplx_trans_q15(const arm_matrix_instance_q15 *pSrc, arm_matrix_instance_q15 *pDst);
void arm_mat_vec_mult_f32(const arm_matrix_instance_f32 *pSrcMat, const float32_t *pVec, float32_t *pDst);
void arm_mat_vec_mult_q31(const arm_matrix_instance_q31 *pSrcMat, const q31_t *pVec, q31_t *pDst);
void arm_mat_vec_mult_q15(const arm_matrix_instance_q15 *pSrcMat, const q15_t *pVec, q15_t *pDst);
void arm_mat_vec_mult_q7(const arm_matrix_instance_q7 *pSrcMat, const q7_t *pVec, q7_t *pDst);

/* Complex math (complex_math_functions.h: ComplexMag, ComplexMagSquared, ComplexConj, CmplxByCmplxMult,
 * CmplxByRealMult, ComplexDotProduct) and the max / min searches of statistics_functions.h, bit-exact with the
 * reference's scalar branches.  Complex vectors are interleaved (re, im) words and numSamples counts complex
 * samples.  Host or device pointers, synchronous.
 *   mag          f32: arm_sqrt_f32(re*re + im*im): a NaN sum stores +0.0.  q31: arm_sqrt_q31((re*re >> 33) +
 *                (im*im >> 33)), 2.30.  q15: arm_sqrt_q31((re*re + im*im) >> 1) >> 16, 2.14.
 *   mag_squared  f32: re*re + im*im.  q31: (re*re >> 33) + (im*im >> 33), 3.29.  q15: (re*re + im*im) >> 17, 3.13.
 *   conj         the imaginary word negated (fixed point: the minimum maps to the maximum; f32: the sign bit).
 *   mult_cmplx   (a*c) - (b*d), (a*d) + (b*c); q31: every product >> 33 first (3.29); q15: >> 17 first (3.13).
 *   mult_real    f32: x * r; q31 / q15: the product >> 31 / >> 15, saturated.
 *   dot_prod     f32: re = (re + a*c) - b*d, im = (im + a*d) + b*c sample by sample from 0.0f, every product
 *                rounded on its own.  q31: products >> 14 in two 64-bit sums (16.48).  q15: 64-bit sums of exact
 *                products, >> 6, stored as q31_t (8.24).  numSamples == 0 stores zeros.
 *   max / min    the value and the first index that holds it (a strict comparison replaces the running result);
 *                +0.0 and -0.0 tie; a NaN after pSrc[0] is never selected and a NaN in pSrc[0] never replaced.
 * Left out: the f16 / f64 forms (arm_cmplx_mag_fast_q15, the _no_idx and absmax / absmin searches: below).
 * A null pointer, and blockSize == 0 in max / min (the reference reads pSrc[0]): nothing is written and
 * arm_mi355x_last_error() is set.  numSamples == 0 writes nothing (dot_prod: zeros).
 * Aliasing.  pDst may equal a source exactly for conj (pSrc), mult_cmplx (pSrcA or pSrcB) and mult_real
 * (pSrcCmplx).  With host pointers the operands are staged separately, so any other overlap, mag / mag_squared
 * into their own source included, behaves as if every source were read before the first store.  With device
 * pointers any other overlap of an output with a source is refused: nothing is written and
 * arm_mi355x_last_error() is set. */
#define MI355X_DECL_CMPLX(SUF, T, R)                                                                            \
  void arm_cmplx_mag_##SUF(const T *pSrc, T *pDst, uint32_t numSamples);                                        \
  void arm_cmplx_mag_squared_##SUF(const T *pSrc, T *pDst, uint32_t numSamples);                                \
  void arm_cmplx_conj_##SUF(const T *pSrc, T *pDst, uint32_t numSamples);                                       \
  void arm_cmplx_mult_cmplx_##SUF(const T *pSrcA, const T *pSrcB, T *pDst, uint32_t numSamples);                \
  void arm_cmplx_mult_real_##SUF(const T *pSrcCmplx, const T *pSrcReal, T *pCmplxDst, uint32_t numSamples);     \
  void arm_cmplx_dot_prod_##SUF(const T *pSrcA, const T *pSrcB, uint32_t numSamples, R *realResult,             \
                                R *imagResult);
MI355X_DECL_CMPLX(f32, float32_t, float32_t)
MI355X_DECL_CMPLX(q31, q31_t, q63_t)
MI355X_DECL_CMPLX(q15, q15_t, q31_t)
#undef MI355X_DECL_CMPLX
void arm_max_f32(const float32_t *pSrc, uint32_t blockSize, float32_t *pResult, uint32_t *pIndex);
void arm_max_q31(const q31_t *pSrc, uint32_t blockSize, q31_t *pResult, uint32_t *pIndex);
void arm_max_q15(const q15_t *pSrc, uint32_t blockSize, q15_t *pResult, uint32_t *pIndex);
void arm_max_q7(const q7_t *pSrc, uint32_t blockSize, q7_t *pResult, uint32_t *pIndex);
void arm_min_f32(const float32_t *pSrc, uint32_t blockSize, float32_t *pResult, uint32_t *pIndex);
void arm_min_q31(const q31_t *pSrc, uint32_t blockSize, q31_t *pResult, uint32_t *pIndex);
void arm_min_q15(const q15_t *pSrc, uint32_t blockSize, q15_t *pResult, uint32_t *pIndex);
void arm_min_q7(const q7_t *pSrc, uint32_t blockSize, q7_t *pResult, uint32_t *pIndex);

/* The level measures and the remaining searches of statistics_functions.h, bit-exact with the reference's scalar
 * branches (built with ARM_MATH_LOOPUNROLL, no ARM_MATH_DSP), arm_sqrt_q15 of fast_math_functions.h and
 * arm_cmplx_mag_fast_q15.  Host or device pointers, synchronous; one result word.
 *   f32          every sum is one chain in element order from 0.0f, each product rounded before its add; divisions
 *                and square roots correctly rounded.  mean: sum / (float)blockSize.  power: the sum of x*x.  rms:
 *                arm_sqrt_f32(power / (float)blockSize), which stores +0.0 for a NaN.  mse: the sum of (a-b)*(a-b) over
 *                (float)blockSize.  var: the mean's chain first, then the chain of (x-mean)*(x-mean) over
 *                ((float)blockSize - 1.0f); std: arm_sqrt_f32(var).  accumulate: the sum.
 *   q31          mean: (q31_t)(sum / blockSize), truncated toward zero.  power: the 64-bit sum of x*x >> 14 (16.48).
 *                rms: arm_sqrt_q31(clip((sum of x*x, unsigned, / blockSize) >> 31)).  mse: halved inputs, a saturating
 *                difference, d*d >> 14 summed, (q31_t)((sum / blockSize) >> 15).  var: in = x >> 8;
 *                (sumOfSquares / (blockSize-1) - sum*sum / (uint32_t)(blockSize*(blockSize-1))) >> 15; std: its
 *                arm_sqrt_q31.
 *   q15          mean: a 32-bit sum / blockSize.  power: the 64-bit sum of x*x (34.30).  rms: arm_sqrt_q15(sat16((sum /
 *                blockSize) >> 15)).  mse: halved inputs, saturating difference, sat16((q31_t)(sum / blockSize) >> 13).
 *                var: a 32-bit sum and 64-bit squares, both quotients cast to q31_t, the difference >> 15; std:
 *                arm_sqrt_q15 of its saturation to 16 bits.  The divisor blockSize*(blockSize-1) is a uint32_t product
 *                and wraps from blockSize 65537 on, as in the reference.
 *   q7           mean: a 32-bit sum / blockSize.  power: a 32-bit sum of x*x (18.14).  mse: sat8((q15_t)(sum / blockSize)
 *                >> 5).
 *   absmax / absmin   max / min over (x > 0) ? x : -x, the negation saturating in fixed point (|minimum| is the
 *                maximum); f32: +0.0 maps to -0.0 and a NaN keeps its place rules (pSrc[0] only) with its sign flipped.
 *   _no_idx      the same searches without the index.  arm_max_no_idx_f32 / arm_min_no_idx_f32 start from -FLT_MAX /
 *                FLT_MAX instead of pSrc[0]: a NaN never wins and an all -Inf (+Inf) vector returns -FLT_MAX (FLT_MAX).
 *   arm_sqrt_q15 Newton on 1 / sqrt, three steps from a 16-word table; in < 0 stores 0 and returns
 *                ARM_MATH_ARGUMENT_ERROR.  Computed on the host.  arm_cmplx_mag_fast_q15: arm_sqrt_q15((re*re + im*im)
 *                >> 17), 2.14.
 * Out of contract, as in the reference (a signed intermediate overflows there, which is undefined in C): a 32-bit sum
 * leaving its range in mean_q7 (possible from blockSize 2^24 + 1), mean_q15 / var_q15 / std_q15 (from 65537),
 * power_q7 (from 131072) and mse_q7 (from 133145); the 64-bit sum of power_q31 / mse_q31 (from 32768); in var_q31 /
 * std_q31 sum * sum reaching 2^63 (from blockSize 363 at full scale) or the sum of squares doing so (from 2^17); in
 * var_q15 / std_q15 also the 32-bit difference of the two quotients.  Here such a call returns what the low bits of
 * the exact sums give.
 * blockSize == 0: power and accumulate store 0, mean_f32 / mse_f32 a NaN (0 / 0), rms_f32 +0.0, var / std 0,
 * max / min_no_idx_f32 their start value; every other function would divide an integer by zero or read pSrc[0]:
 * nothing is written and arm_mi355x_last_error() is set, as for a null pointer.  blockSize 1 gives 0 in var / std.
 * With device pointers a result that overlaps a source, or the index, is refused in the same way.
 * arm_entropy_f32, arm_kullback_leibler_f32, arm_logsumexp_f32 and arm_logsumexp_dot_prod_f32 (they rest on the host
 * libm's expf / logf) are declared further down, with the SVM and naive Bayes functions.
 * Left out: every f16 / f64 form. */
#define MI355X_DECL_STAT(SUF, T, PR)                                                     \
  void arm_mean_##SUF(const T *pSrc, uint32_t blockSize, T *pResult);                    \
  void arm_power_##SUF(const T *pSrc, uint32_t blockSize, PR *pResult);                  \
  void arm_mse_##SUF(const T *pSrcA, const T *pSrcB, uint32_t blockSize, T *pResult);    \
  void arm_absmax_##SUF(const T *pSrc, uint32_t blockSize, T *pResult, uint32_t *pIndex); \
  void arm_absmin_##SUF(const T *pSrc, uint32_t blockSize, T *pResult, uint32_t *pIndex); \
  void arm_max_no_idx_##SUF(const T *pSrc, uint32_t blockSize, T *pResult);              \
  void arm_min_no_idx_##SUF(const T *pSrc, uint32_t blockSize, T *pResult);              \
  void arm_absmax_no_idx_##SUF(const T *pSrc, uint32_t blockSize, T *pResult);           \
  void arm_absmin_no_idx_##SUF(const T *pSrc, uint32_t blockSize, T *pResult);
#define MI355X_DECL_STAT_LEVELS(SUF, T)                                \
  void arm_rms_##SUF(const T *pSrc, uint32_t blockSize, T *pResult);   \
  void arm_var_##SUF(const T *pSrc, uint32_t blockSize, T *pResult);   \
  void arm_std_##SUF(const T *pSrc, uint32_t blockSize, T *pResult);
MI355X_DECL_STAT(f32, float32_t, float32_t)
MI355X_DECL_STAT(q31, q31_t, q63_t)
MI355X_DECL_STAT(q15, q15_t, q63_t)
MI355X_DECL_STAT(q7, q7_t, q31_t)
MI355X_DECL_STAT_LEVELS(f32, float32_t)
MI355X_DECL_STAT_LEVELS(q31, q31_t)
MI355X_DECL_STAT_LEVELS(q15, q15_t)
#undef MI355X_DECL_STAT_LEVELS
#undef MI355X_DECL_STAT
void arm_accumulate_f32(const float32_t *pSrc, uint32_t blockSize, float32_t *pResult);
arm_status arm_sqrt_q15(q15_t in, q15_t *pOut);
void arm_cmplx_mag_fast_q15(const q15_t *pSrc, q15_t *pDst, uint32_t numSamples);

/* The basic math functions of basic_math_functions.h (BasicAdd, BasicSub, BasicMult, BasicOffset, BasicScale,
 * BasicShift, BasicClip, BasicAbs, BasicNegate, BasicDotProd, And, Or, Xor, Not), bit-exact with the reference's
 * scalar branches (built with ARM_MATH_LOOPUNROLL, no ARM_MATH_DSP).  Host or device pointers, synchronous; pDst may
 * be a source exactly.
 *   f32   a + b, a - b, a * b, x + offset, x * scale, each rounded once; abs clears the sign bit (-0.0 -> +0.0),
 *         negate flips it; dot_prod is one ordered chain sum = sum + a*b from 0.0f, the product rounded before the add.
 *   q31   add / sub / offset saturate to 32 bits.  mult: __SSAT((a*b) >> 32, 31) << 1 (the low bit is 0).  scale:
 *         in = (x * scaleFract) >> 32, then in << (shift + 1) saturated (0x7FFFFFFF ^ (in >> 31) when bits are lost),
 *         or an arithmetic in >> -(shift + 1).  shift: the same on x with shiftBits.  dot_prod: every product >> 14
 *         summed into 64 bits (16.48), mod 2^64.
 *   q15   __SSAT(.., 16) of a + b, a - b, (a*b) >> 15, x + offset, (x * scaleFract) >> (15 - shift).  shift left:
 *         __SSAT((q31_t)x << shiftBits, 16), the 32-bit shift wrapping first (counts above 16 show it); right:
 *         arithmetic.  dot_prod: the exact products summed into 64 bits (34.30).
 *   q7    as q15 with 8 bits: (a*b) >> 7, (x * scaleFract) >> (7 - shift).  dot_prod: a 32-bit sum (18.14), in range
 *         up to 131071 words at full scale.
 *   abs / negate of the most negative word give the most positive.  clip: x > high ? high : x < low ? low : x; a NaN
 *         passes through, and with low > high the first comparison wins.
 *   and / or / xor / not on uint32_t, uint16_t, uint8_t words.
 * Shift counts: the ones at which the reference's C is defined (a count below 32 either way on its promoted int
 * operands): arm_shift_* -31 .. 31, arm_scale_q31 -32 .. 30, arm_scale_q15 -16 .. 15, arm_scale_q7 -24 .. 7.  Outside,
 * and for a null pointer, nothing is written and arm_mi355x_last_error() is set.  With device pointers an output
 * that overlaps a source other than exactly is refused in the same way.  blockSize == 0 writes nothing (dot_prod
 * stores 0).
 * Left out: the f16 / f64 forms. */
#define MI355X_DECL_BASIC(SUF, T, DR)                                                        \
  void arm_add_##SUF(const T *pSrcA, const T *pSrcB, T *pDst, uint32_t blockSize);           \
  void arm_sub_##SUF(const T *pSrcA, const T *pSrcB, T *pDst, uint32_t blockSize);           \
  void arm_mult_##SUF(const T *pSrcA, const T *pSrcB, T *pDst, uint32_t blockSize);          \
  void arm_offset_##SUF(const T *pSrc, T offset, T *pDst, uint32_t blockSize);               \
  void arm_clip_##SUF(const T *pSrc, T *pDst, T low, T high, uint32_t numSamples);           \
  void arm_abs_##SUF(const T *pSrc, T *pDst, uint32_t blockSize);                            \
  void arm_negate_##SUF(const T *pSrc, T *pDst, uint32_t blockSize);                         \
  void arm_dot_prod_##SUF(const T *pSrcA, const T *pSrcB, uint32_t blockSize, DR *result);
#define MI355X_DECL_BASIC_FIXED(SUF, T)                                                              \
  void arm_scale_##SUF(const T *pSrc, T scaleFract, int8_t shift, T *pDst, uint32_t blockSize);      \
  void arm_shift_##SUF(const T *pSrc, int8_t shiftBits, T *pDst, uint32_t blockSize);
#define MI355X_DECL_BITWISE(SUF, T)                                                          \
  void arm_and_##SUF(const T *pSrcA, const T *pSrcB, T *pDst, uint32_t blockSize);           \
  void arm_or_##SUF(const T *pSrcA, const T *pSrcB, T *pDst, uint32_t blockSize);            \
  void arm_xor_##SUF(const T *pSrcA, const T *pSrcB, T *pDst, uint32_t blockSize);           \
  void arm_not_##SUF(const T *pSrc, T *pDst, uint32_t blockSize);
MI355X_DECL_BASIC(f32, float32_t, float32_t)
MI355X_DECL_BASIC(q31, q31_t, q63_t)
MI355X_DECL_BASIC(q15, q15_t, q63_t)
MI355X_DECL_BASIC(q7, q7_t, q31_t)
MI355X_DECL_BASIC_FIXED(q31, q31_t)
MI355X_DECL_BASIC_FIXED(q15, q15_t)
MI355X_DECL_BASIC_FIXED(q7, q7_t)
MI355X_DECL_BITWISE(u32, uint32_t)
MI355X_DECL_BITWISE(u16, uint16_t)
MI355X_DECL_BITWISE(u8, uint8_t)
#undef MI355X_DECL_BITWISE
#undef MI355X_DECL_BASIC_FIXED
#undef MI355X_DECL_BASIC
void arm_scale_f32(const float32_t *pSrc, float32_t scale, float32_t *pDst, uint32_t blockSize);

/* The support functions of support_functions.h (float_to_x, q31_to_x, q15_to_x, q7_to_x, copy, Fill, Sorting,
 * weightedaverage, barycenter).  Host or device pointers, synchronous.  Every word of the conversions, copy, fill,
 * arm_weighted_average_f32 and arm_barycenter_f32 equals the reference's scalar branches (ARM_MATH_LOOPUNROLL, no
 * ARM_MATH_ROUNDING, no ARM_MATH_DSP).
 *   float -> q   the f32 product x * 2^31 / 2^15 / 2^7 (subnormals kept), truncated toward zero, then clipped to 32
 *                bits or __SSAT to 16 / 8 bits.  The reference's C cast is undefined for NaN and outside |x| < 2^32
 *                (q31), 65536 (q15), 2^24 (q7); there these functions saturate by sign and turn NaN into 0.
 *   q -> float   (float)x / 2^31 / 2^15 / 2^7; q31 words above 2^24 round to nearest even (0x7FFFFFFF gives 1.0f).
 *   q -> q       << 16, << 24, << 8 widening; arithmetic >> 16, >> 24, >> 8 narrowing.
 *   pDst may equal pSrc exactly where both element widths are equal (float_to_q31, q31_to_float, copy); with device
 *   pointers any other overlap is refused.  A refusal or a null pointer writes nothing and sets
 *   arm_mi355x_last_error().  blockSize == 0 writes nothing.
 *   sort         arm_sort_f32 and arm_merge_sort_f32 both run one bitonic network on the IEEE total order of the
 *                words: ascending is negative NaNs, -Inf .. -0.0, +0.0 .. +Inf, positive NaNs; descending the reverse.
 *                Without NaNs and without both signs of zero every output word equals the reference's (with both
 *                zeros: equal as values and as multisets of words).  S->alg only selects among equal results (a value
 *                outside arm_sort_alg is a no-op, as in the reference's switch); unlike the reference,
 *                ARM_SORT_BITONIC also sorts when blockSize is no power of two and when dir is ARM_SORT_DESCENDING.
 *                arm_merge_sort_f32 neither reads nor writes S->buffer.  pSrc is unchanged unless it is pDst.
 *   arm_weighted_average_f32   sum(in * w) / sum(w): two ordered f32 chains from 0.0f, the product rounded before its
 *                add, one division (blockSize 0: 0 / 0, a NaN; a failure also returns a NaN and sets the last error).
 *   arm_barycenter_f32         out[d] = (sum_v in[v][d] * w[v]) / (sum_v w[v]), chains over v in order, a division.
 * Left out: the f16 / f64 forms. */
typedef enum {
  ARM_SORT_BITONIC = 0,
  ARM_SORT_BUBBLE = 1,
  ARM_SORT_HEAP = 2,
  ARM_SORT_INSERTION = 3,
  ARM_SORT_QUICK = 4,
  ARM_SORT_SELECTION = 5
} arm_sort_alg;
typedef enum { ARM_SORT_DESCENDING = 0, ARM_SORT_ASCENDING = 1 } arm_sort_dir;
typedef struct {
  arm_sort_alg alg;
  arm_sort_dir dir;
} arm_sort_instance_f32;
typedef struct {
  arm_sort_dir dir;
  float32_t *buffer;
} arm_merge_sort_instance_f32;
void arm_sort_init_f32(arm_sort_instance_f32 *S, arm_sort_alg alg, arm_sort_dir dir);
void arm_sort_f32(const arm_sort_instance_f32 *S, float32_t *pSrc, float32_t *pDst, uint32_t blockSize);
void arm_merge_sort_init_f32(arm_merge_sort_instance_f32 *S, arm_sort_dir dir, float32_t *buffer);
void arm_merge_sort_f32(const arm_merge_sort_instance_f32 *S, float32_t *pSrc, float32_t *pDst, uint32_t blockSize);
float32_t arm_weighted_average_f32(const float32_t *in, const float32_t *weights, uint32_t blockSize);
void arm_barycenter_f32(const float32_t *in, const float32_t *weights, float32_t *out, uint32_t nbVectors,
                        uint32_t vecDim);
#define MI355X_DECL_SUPPORT_TO(SN, ST, DN, DT) void arm_##SN##_to_##DN(const ST *pSrc, DT *pDst, uint32_t blockSize);
MI355X_DECL_SUPPORT_TO(float, float32_t, q31, q31_t)
MI355X_DECL_SUPPORT_TO(float, float32_t, q15, q15_t)
MI355X_DECL_SUPPORT_TO(float, float32_t, q7, q7_t)
MI355X_DECL_SUPPORT_TO(q31, q31_t, float, float32_t)
MI355X_DECL_SUPPORT_TO(q31, q31_t, q15, q15_t)
MI355X_DECL_SUPPORT_TO(q31, q31_t, q7, q7_t)
MI355X_DECL_SUPPORT_TO(q15, q15_t, float, float32_t)
MI355X_DECL_SUPPORT_TO(q15, q15_t, q31, q31_t)
MI355X_DECL_SUPPORT_TO(q15, q15_t, q7, q7_t)
MI355X_DECL_SUPPORT_TO(q7, q7_t, float, float32_t)
MI355X_DECL_SUPPORT_TO(q7, q7_t, q31, q31_t)
MI355X_DECL_SUPPORT_TO(q7, q7_t, q15, q15_t)
#undef MI355X_DECL_SUPPORT_TO
#define MI355X_DECL_SUPPORT_COPY(SUF, T)                          \
  void arm_copy_##SUF(const T *pSrc, T *pDst, uint32_t blockSize); \
  void arm_fill_##SUF(T value, T *pDst, uint32_t blockSize);
MI355X_DECL_SUPPORT_COPY(f32, float32_t)
MI355X_DECL_SUPPORT_COPY(q31, q31_t)
MI355X_DECL_SUPPORT_COPY(q15, q15_t)
MI355X_DECL_SUPPORT_COPY(q7, q7_t)
#undef MI355X_DECL_SUPPORT_COPY

/* The distance functions of distance_functions.h: the f32 distances, the boolean distances on packed uint32_t words
 * and dynamic time warping.  Host or device pointers, synchronous.  Every result word equals the reference's scalar
 * branches (ARM_MATH_LOOPUNROLL, no FMA contraction); NaN results are NaNs, their bits are not pinned.
 *   f32       every sum is an ordered chain from 0.0f in element order, each term rounded before its add; divisions
 *             and square roots are correctly rounded; arm_sqrt_f32 gives +0.0 for a negative or NaN argument (so
 *             euclidean, cosine, correlation and jensenshannon never return the NaN of a square root).  canberra
 *             skips an element whose two words both compare equal to zero.  chebyshev starts from element 0 and
 *             replaces on diff > maxVal only.  jensenshannon evaluates x * logf(x / m), m = (a + b) / 2.0f, with the
 *             glibc logf the MFCC uses.  arm_correlation_distance_f32 writes x + (-mean) back into pA and pB, as the
 *             reference does (its pointers are not const); pA and pB must not overlap.
 *             blockSize == 0: chebyshev (which would read element 0) writes nothing, returns a NaN and sets
 *             arm_mi355x_last_error(); every other function returns what its arithmetic gives on empty sums.
 *   boolean   an item is ceil(numberOfBools / 32) words and no further word is read (the reference loads one more
 *             when numberOfBools is a multiple of 32).  Of a last, partial word the top numberOfBools % 32 bits
 *             count.  The epilogues are the reference's expressions: uint32_t sums and products wrap (yule's from
 *             about 2^17 booleans on), counts above 2^24 round to nearest even when they become floats.
 *             numberOfBools == 0 evaluates the epilogue on zero counts (mostly 0 / 0).
 *   DTW       arm_dtw_distance_f32 writes every word of pDTW (F32_MAX outside the window) and *distance unless it
 *             returns ARM_MATH_ARGUMENT_ERROR (the last cell is F32_MAX: no path inside the window); pWindow may be
 *             NULL; a distance word outside the window is never read.  MIN(x, y) is x < y ? x : y, NaNs included.
 *             arm_dtw_path_f32: the reference's walk; where the reference would never return (a cell with no
 *             neighbour below F32_MAX) *pathLength is 0 and the last error is set.  arm_dtw_distance_f32 and
 *             arm_dtw_path_f32 refuse lengths of 0 or above 32768.  arm_dtw_init_window_q7 returns
 *             ARM_MATH_ARGUMENT_ERROR and writes nothing for an unknown window type or a length above 32768; with 0
 *             rows or 0 columns it succeeds and writes nothing, as the reference does.
 * A failure of a function that returns a float returns a NaN and sets the last error.
 * Left out: arm_minkowski_distance_f32 (the host libm's powf, of which there is no device restatement) and the
 * f16 / f64 forms. */
typedef enum {
  ARM_DTW_SAKOE_CHIBA_WINDOW = 1,
  /*ARM_DTW_ITAKURA_WINDOW = 2,*/
  ARM_DTW_SLANTED_BAND_WINDOW = 3
} arm_dtw_window;
#define MI355X_DECL_DISTANCE_F32(NAME) \
  float32_t arm_##NAME##_distance_f32(const float32_t *pA, const float32_t *pB, uint32_t blockSize);
MI355X_DECL_DISTANCE_F32(braycurtis)
MI355X_DECL_DISTANCE_F32(canberra)
MI355X_DECL_DISTANCE_F32(chebyshev)
MI355X_DECL_DISTANCE_F32(cityblock)
MI355X_DECL_DISTANCE_F32(cosine)
MI355X_DECL_DISTANCE_F32(euclidean)
MI355X_DECL_DISTANCE_F32(jensenshannon)
#undef MI355X_DECL_DISTANCE_F32
float32_t arm_correlation_distance_f32(float32_t *pA, float32_t *pB, uint32_t blockSize);
#define MI355X_DECL_DISTANCE_BOOL(NAME) \
  float32_t arm_##NAME##_distance(const uint32_t *pA, const uint32_t *pB, uint32_t numberOfBools);
MI355X_DECL_DISTANCE_BOOL(dice)
MI355X_DECL_DISTANCE_BOOL(hamming)
MI355X_DECL_DISTANCE_BOOL(jaccard)
MI355X_DECL_DISTANCE_BOOL(kulsinski)
MI355X_DECL_DISTANCE_BOOL(rogerstanimoto)
MI355X_DECL_DISTANCE_BOOL(russellrao)
MI355X_DECL_DISTANCE_BOOL(sokalmichener)
MI355X_DECL_DISTANCE_BOOL(sokalsneath)
MI355X_DECL_DISTANCE_BOOL(yule)
#undef MI355X_DECL_DISTANCE_BOOL
arm_status arm_dtw_init_window_q7(const arm_dtw_window windowType, const int32_t windowSize,
                                  arm_matrix_instance_q7 *pWindow);
arm_status arm_dtw_distance_f32(const arm_matrix_instance_f32 *pDistance, const arm_matrix_instance_q7 *pWindow,
                                arm_matrix_instance_f32 *pDTW, float32_t *distance);
void arm_dtw_path_f32(const arm_matrix_instance_f32 *pDTW, int16_t *pPath, uint32_t *pathLength);

/* arm_vexp_f32 / arm_vlog_f32 (fast_math_functions.h), arm_entropy_f32, arm_kullback_leibler_f32, arm_logsumexp_f32,
 * arm_logsumexp_dot_prod_f32 (statistics_functions.h), the linear, polynomial and rbf SVMs (svm_functions.h) and the
 * Gaussian naive Bayes estimator (bayes_functions.h).  Host or device pointers, synchronous.  Every result word
 * equals the reference's scalar branches built without FMA contraction on a host whose libm is glibc 2.35: expf and
 * logf are that libm's, restated operation for operation and proven equal on all 2^32 inputs.  NaN results are NaNs,
 * their bits are not pinned.
 *   vexp, vlog    element-wise; pDst may be pSrc exactly; blockSize == 0 writes nothing.
 *   entropy       accum += p * logf(p) in element order from 0.0f, returns -accum (p == 0 gives a NaN, blockSize == 0
 *                 gives -0.0f).  kullback_leibler: accum += pA * logf(pB / pA), returns -accum.
 *   logsumexp     the maximum by strict > from in[0] (a NaN there stays, a later NaN never wins), accum += expf(x - max)
 *                 in element order, returns max + logf(accum).  logsumexp_dot_prod: arm_add_f32 into pTmpBuffer
 *                 (blockSize words, written), then logsumexp of it.  blockSize == 0 would read element 0: nothing is
 *                 written, a NaN is returned and arm_mi355x_last_error() is set.
 *   SVM           per support vector, in row order, dot is an ordered chain over the dimensions (linear, polynomial:
 *                 dot + in[j] * sv[j]; rbf: dot + (in[j] - sv[j])^2), then from sum = intercept: sum += dual[i] * dot,
 *                 dual[i] * arm_exponent_f32(gamma * dot + coef0, degree) (degree < 1 as degree 1) or dual[i] *
 *                 expf(-gamma * dot).  *pResult = classes[sum <= 0 ? 0 : 1]: a NaN sum gives classes[1].
 *                 nbOfSupportVectors == 0 classifies the intercept.  The init functions only fill the instance.
 *   naive Bayes   per class, over the dimensions: sigma = S->sigma[] + epsilon, acc1 += logf((2.0f * PI_F) * sigma),
 *                 acc2 += ((in - theta) * (in - theta)) / sigma; the class's word is (-0.5f * acc1 - 0.5f * acc2) +
 *                 logf(prior), stored to pOutputProbabilities; the return value is arm_max_f32's index over them.
 *                 pBufferB is not used and may be NULL.  numberOfClasses == 0, or any other failure, returns
 *                 UINT32_MAX and sets the last error.
 * Left out: arm_svm_sigmoid_* (the host libm's tanhf, glibc's expm1f path, which would need a restatement of its
 * own) and the f16 / f64 forms. */
typedef struct {
  uint32_t nbOfSupportVectors;
  uint32_t vectorDimension;
  float32_t intercept;
  const float32_t *dualCoefficients;
  const float32_t *supportVectors;
  const int32_t *classes;
} arm_svm_linear_instance_f32;
typedef struct {
  uint32_t nbOfSupportVectors;
  uint32_t vectorDimension;
  float32_t intercept;
  const float32_t *dualCoefficients;
  const float32_t *supportVectors;
  const int32_t *classes;
  int32_t degree;
  float32_t coef0;
  float32_t gamma;
} arm_svm_polynomial_instance_f32;
typedef struct {
  uint32_t nbOfSupportVectors;
  uint32_t vectorDimension;
  float32_t intercept;
  const float32_t *dualCoefficients;
  const float32_t *supportVectors;
  const int32_t *classes;
  float32_t gamma;
} arm_svm_rbf_instance_f32;
typedef struct {                       /* the type only: arm_svm_sigmoid_* are left out */
  uint32_t nbOfSupportVectors;
  uint32_t vectorDimension;
  float32_t intercept;
  const float32_t *dualCoefficients;
  const float32_t *supportVectors;
  const int32_t *classes;
  float32_t coef0;
  float32_t gamma;
} arm_svm_sigmoid_instance_f32;
typedef struct {
  uint32_t vectorDimension;
  uint32_t numberOfClasses;
  const float32_t *theta;
  const float32_t *sigma;
  const float32_t *classPriors;
  float32_t epsilon;
} arm_gaussian_naive_bayes_instance_f32;
void arm_vexp_f32(const float32_t *pSrc, float32_t *pDst, uint32_t blockSize);
void arm_vlog_f32(const float32_t *pSrc, float32_t *pDst, uint32_t blockSize);
float32_t arm_entropy_f32(const float32_t *pSrcA, uint32_t blockSize);
float32_t arm_kullback_leibler_f32(const float32_t *pSrcA, const float32_t *pSrcB, uint32_t blockSize);
float32_t arm_logsumexp_f32(const float32_t *in, uint32_t blockSize);
float32_t arm_logsumexp_dot_prod_f32(const float32_t *pSrcA, const float32_t *pSrcB, uint32_t blockSize,
                                     float32_t *pTmpBuffer);
void arm_svm_linear_init_f32(arm_svm_linear_instance_f32 *S, uint32_t nbOfSupportVectors, uint32_t vectorDimension,
                             float32_t intercept, const float32_t *dualCoefficients, const float32_t *supportVectors,
                             const int32_t *classes);
void arm_svm_polynomial_init_f32(arm_svm_polynomial_instance_f32 *S, uint32_t nbOfSupportVectors,
                                 uint32_t vectorDimension, float32_t intercept, const float32_t *dualCoefficients,
                                 const float32_t *supportVectors, const int32_t *classes, int32_t degree,
                                 float32_t coef0, float32_t gamma);
void arm_svm_rbf_init_f32(arm_svm_rbf_instance_f32 *S, uint32_t nbOfSupportVectors, uint32_t vectorDimension,
                          float32_t intercept, const float32_t *dualCoefficients, const float32_t *supportVectors,
                          const int32_t *classes, float32_t gamma);
void arm_svm_linear_predict_f32(const arm_svm_linear_instance_f32 *S, const float32_t *in, int32_t *pResult);
void arm_svm_polynomial_predict_f32(const arm_svm_polynomial_instance_f32 *S, const float32_t *in, int32_t *pResult);
void arm_svm_rbf_predict_f32(const arm_svm_rbf_instance_f32 *S, const float32_t *in, int32_t *pResult);
uint32_t arm_gaussian_naive_bayes_predict_f32(const arm_gaussian_naive_bayes_instance_f32 *S, const float32_t *in,
                                              float32_t *pOutputProbabilities, float32_t *pBufferB);

/* Interpolation (interpolation_functions.h): linear, bilinear and cubic spline.  The f16 forms are left out.
 *
 * arm_linear_interp_* and arm_bilinear_interp_* take one sample and return one sample.  They are computed on the
 * HOST, as arm_sqrt_q15 is: the table (S->pYData, pYData, S->pData) must be host-readable memory.  The vector forms
 * on device pointers are the _batch functions of arm_math_mi355x.h.  Every result equals the reference's scalar code
 * built without FMA contraction:
 *   linear f32    i = (int32_t)((x - S->x1) / xSpacing); x < S->x1 gives pYData[0] (tested first), (uint32_t)i >=
 *                 nValues - 1 gives pYData[nValues - 1], otherwise y0 + (x - x0) * ((y1 - y0) / (x1 - x0)) with x0 =
 *                 S->x1 + i * xSpacing and x1 = S->x1 + (i + 1) * xSpacing, every operation rounded on its own.
 *   linear q31, q15, q7   x is 12.20: a signed 12-bit index (q7: x < 0 gives pYData[0], then an unsigned one) and a
 *                 20-bit fraction; past either end the result is the table's end; inside, the reference's shifts
 *                 and truncations (0x7FFFFFFF - fract in q31, 0xFFFFF - fract in q15 and q7).
 *   bilinear f32  xIndex = (int32_t)X, yIndex = (int32_t)Y; 0 outside [0, numCols - 2] x [0, numRows - 2]; otherwise
 *                 b1 + b2 * xdiff + b3 * ydiff + b4 * xdiff * ydiff, left to right, b4 = f00 - f01 - f10 + f11.
 *   bilinear q31, q15, q7   X and Y are 12.20; X's index is bounded by numCols - 2 and Y's by numRows - 2, the word
 *                 is pData[xi + numCols * yi]; 0 outside; the reference's four products and shifts inside.
 * Defined here where the reference is not: the casts (int32_t)((x - x1) / xSpacing), (int32_t)X and (int32_t)Y
 * saturate by sign outside the int32_t range and give 0 for a NaN.  Refused (0 is returned, a NaN by the f32 forms,
 * and arm_mi355x_last_error() is set): a null pointer, nValues == 0, a bilinear table of numRows * numCols >= 2^31
 * words.
 *
 * arm_spline_init_f32 and arm_spline_f32 take host or device pointers, are synchronous and are computed on the GPU.
 * init solves the tridiagonal system exactly as written: the forward chain li -> u[i] -> z[i] into tempBuffer (2 n - 1
 * words), the backward chain into coeffs (b, c, d: 3 (n - 1) words), for both boundary types; it sets S->x, S->y,
 * S->n_x and S->coeffs as the reference does (not S->type).  arm_spline_f32 walks xq as the reference does, with an
 * interval that never goes back: output k uses interval min(n - 2, max over j <= k of f(xq[j])), f(v) the first i
 * with v <= x[i + 1] and n - 1 where there is none (a NaN); the value is y + b t + c t t + d t t t, left to right, t =
 * xq - x[i].  Refused (nothing written, last error set): a null pointer, n < 2 (the reference reads y[-1]), a type
 * other than the two, a destination that overlaps a source.  blockSize == 0 writes nothing. */
typedef struct {
  uint32_t nValues;
  float32_t x1;
  float32_t xSpacing;
  const float32_t *pYData;
} arm_linear_interp_instance_f32;
typedef struct {
  uint16_t numRows;
  uint16_t numCols;
  const float32_t *pData;
} arm_bilinear_interp_instance_f32;
typedef struct {
  uint16_t numRows;
  uint16_t numCols;
  const q31_t *pData;
} arm_bilinear_interp_instance_q31;
typedef struct {
  uint16_t numRows;
  uint16_t numCols;
  const q15_t *pData;
} arm_bilinear_interp_instance_q15;
typedef struct {
  uint16_t numRows;
  uint16_t numCols;
  const q7_t *pData;
} arm_bilinear_interp_instance_q7;
typedef enum { ARM_SPLINE_NATURAL = 0, ARM_SPLINE_PARABOLIC_RUNOUT = 1 } arm_spline_type;
typedef struct {
  arm_spline_type type;
  const float32_t *x;
  const float32_t *y;
  uint32_t n_x;
  float32_t *coeffs;
} arm_spline_instance_f32;
float32_t arm_linear_interp_f32(const arm_linear_interp_instance_f32 *S, float32_t x);
q31_t arm_linear_interp_q31(const q31_t *pYData, q31_t x, uint32_t nValues);
q15_t arm_linear_interp_q15(const q15_t *pYData, q31_t x, uint32_t nValues);
q7_t arm_linear_interp_q7(const q7_t *pYData, q31_t x, uint32_t nValues);
float32_t arm_bilinear_interp_f32(const arm_bilinear_interp_instance_f32 *S, float32_t X, float32_t Y);
q31_t arm_bilinear_interp_q31(arm_bilinear_interp_instance_q31 *S, q31_t X, q31_t Y);
q15_t arm_bilinear_interp_q15(arm_bilinear_interp_instance_q15 *S, q31_t X, q31_t Y);
q7_t arm_bilinear_interp_q7(arm_bilinear_interp_instance_q7 *S, q31_t X, q31_t Y);
void arm_spline_init_f32(arm_spline_instance_f32 *S, arm_spline_type type, const float32_t *x, const float32_t *y,
                         uint32_t n, float32_t *coeffs, float32_t *tempBuffer);
void arm_spline_f32(arm_spline_instance_f32 *S, const float32_t *xq, float32_t *pDst, uint32_t blockSize);

/* The quaternion functions (quaternion_math_functions.h), f32.  Host or device pointers, synchronous.  A quaternion
 * is 4 words (w, x, y, z), a rotation 9 words in row order.  Every result word equals the reference's scalar branch
 * built without FMA contraction: the sums in the order written there, a correctly rounded sqrtf and division.  NaN
 * results are NaNs, their bits are not pinned.
 *   norm          sqrtf(w*w + x*x + y*y + z*z), the sum left to right; one word per quaternion.
 *   inverse       (w, -x, -y, -z) each divided by that sum of squares; the zero quaternion gives NaNs.
 *   conjugate     (w, -x, -y, -z).   normalize: each word divided by the norm; the zero quaternion gives NaNs.
 *   product       qr[i] = qa[i] * qb[i] (Hamilton product); product_single is one such product.
 *   quaternion2rotation   the 3 x 3 matrix of each quaternion, which need not be normalised.
 *   rotation2quaternion   the reference's four branches with their strict comparisons: trace > 0, else r00 the
 *                 largest diagonal word, else r11 > r22, else the last; a trace of exactly 0 takes the second test, a
 *                 NaN trace ends in the last branch.
 * A destination of quaternions may be a source of quaternions exactly (in place); any other overlap of a destination
 * with a source, or a null pointer, writes nothing and sets arm_mi355x_last_error().  nbQuaternions == 0 writes
 * nothing. */
void arm_quaternion_norm_f32(const float32_t *pInputQuaternions, float32_t *pNorms, uint32_t nbQuaternions);
void arm_quaternion_inverse_f32(const float32_t *pInputQuaternions, float32_t *pInverseQuaternions,
                                uint32_t nbQuaternions);
void arm_quaternion_conjugate_f32(const float32_t *pInputQuaternions, float32_t *pConjugateQuaternions,
                                  uint32_t nbQuaternions);
void arm_quaternion_normalize_f32(const float32_t *pInputQuaternions, float32_t *pNormalizedQuaternions,
                                  uint32_t nbQuaternions);
void arm_quaternion_product_single_f32(const float32_t *qa, const float32_t *qb, float32_t *qr);
void arm_quaternion_product_f32(const float32_t *qa, const float32_t *qb, float32_t *qr, uint32_t nbQuaternions);
void arm_quaternion2rotation_f32(const float32_t *pInputQuaternions, float32_t *pOutputRotations,
                                 uint32_t nbQuaternions);
void arm_rotation2quaternion_f32(const float32_t *pInputRotations, float32_t *pOutputQuaternions,
                                 uint32_t nbQuaternions);

#ifdef __cplusplus
}
#endif

#include "arm_const_structs.h"

#endif /* ARM_MATH_MI355X_DROPIN_H */
