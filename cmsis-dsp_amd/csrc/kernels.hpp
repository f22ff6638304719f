// Internal launch entry points of the HIP kernels (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi355x {

// The largest 1-D grid the launches use.  Batches go on grid x (grid y and z stop at 65,535); a call
// whose workgroup count exceeds this is refused: grid_limit_error records which product it was, the
// error channel's next message carries it ("... > 2147483647 workgroups"), and the entry point
// returns ARM_MATH_ARGUMENT_ERROR.
constexpr uint64_t kMaxGridX = 0x7fffffffull;
hipError_t grid_limit_error(const char* product);   // runtime.cpp; returns hipErrorInvalidValue

// Grid of a persistent kernel: every CU filled to the occupancy the compiled kernel allows
// (hipOccupancyMaxActiveBlocksPerMultiprocessor x CU count), never more blocks than items.
// The CU count is per device (cached for the first 16 ordinals).
inline int persistent_grid(const void* kernel, int block, size_t lds, uint64_t items, int fallback_per_cu = 2) {
  static int cus_cache[16] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  int cus = (dev >= 0 && dev < 16) ? cus_cache[dev] : 0;
  if (!cus) {
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
    if (dev >= 0 && dev < 16) cus_cache[dev] = cus;
  }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess || per_cu <= 0)
    per_cu = fallback_per_cu;
  const uint64_t g = (uint64_t)cus * per_cu;
  return (int)(g < items ? g : items);
}

// In-place batched CFFT over `batch` contiguous transforms of n complex samples.
// tw: device copy of the instance's twiddle table.  perm: optional device permutation
// (nullptr = the reference tables' canonical digit reversal).  flags: kIfft | kBitrev
// (| kSatShl1 for q31 / q15).
hipError_t cfft_f32_launch(int n, float* data, uint32_t batch, const float* tw, const uint16_t* perm,
                           uint32_t flags, hipStream_t st);
// N = 256 / 512 / 1024 / 2048 with the reference's own bit-reversal table (cfft_fixed_r16.hip);
// false if N is not one of those lengths.
bool cfft_q31_r16_launch(int n, int32_t* data, uint32_t batch, const int32_t* tw, uint32_t flags, hipStream_t st);
bool cfft_q15_r16_launch(int n, int16_t* data, uint32_t batch, const int16_t* tw, uint32_t flags, hipStream_t st);
// The same kernels with the MFCC front end fused into their load phase (PRE): forward, frame
// maxima to maxv[frame * mstride]; false when n is not 256..2048.
// Stores v into *dflag (a device-mapped coherent host word) after the stream's earlier work
// (sync.hip): the drop-in calls' completion signal.
hipError_t done_flag_launch(uint32_t* dflag, uint32_t v, hipStream_t st);
// One arm_cfft_f32 N = 1024 call of the drop-in (the reference's table, batch within one
// workgroup) whose workgroup stores seq into done when its stores are visible; false: not this
// case, nothing launched.
bool cfft_f32_n1024_done_launch(float* data, uint32_t batch, const float* tw, const uint16_t* perm, uint32_t flags,
                                uint32_t* done, uint32_t seq, hipStream_t st);

// The whole MFCC q31 / q15 in one launch (front end + CFFT + back end, cfft_fixed_r16.hip);
// n = fftLen / 2.  hipErrorNotSupported: not handled (take the two-launch schedule).
hipError_t mfcc_q31_fused_launch(int n, const int32_t* frames, uint32_t batch, const int32_t* tw, const int32_t* win,
                                 bool brev, const int4* stw, int nb_mel, const int32_t* coefs, const uint32_t* bf,
                                 int total, int kmin, int kcnt, int nb_dct, const int32_t* dct, const int32_t* lut,
                                 int32_t* dst, hipStream_t st);
hipError_t mfcc_q15_fused_launch(int n, const int16_t* frames, uint32_t batch, const int16_t* tw, const int16_t* win,
                                 bool brev, const int4* stw, int nb_mel, const int16_t* coefs, const uint32_t* bf,
                                 int total, int kmin, int kcnt, int nb_dct, const int16_t* dct, const int32_t* lut,
                                 int16_t* dst, hipStream_t st);
bool cfft_q31_r16_mfcc_launch(int n, int32_t* data, uint32_t batch, const int32_t* tw, const int32_t* win,
                              int32_t* maxv, int mstride, bool brev, hipStream_t st);
bool cfft_q15_r16_mfcc_launch(int n, int16_t* data, uint32_t batch, const int16_t* tw, const int16_t* win,
                              int16_t* maxv, int mstride, bool brev, hipStream_t st);
hipError_t cfft_q31_launch(int n, int32_t* data, uint32_t batch, const int32_t* tw, const uint16_t* perm,
                           uint32_t flags, hipStream_t st);
hipError_t cfft_q15_launch(int n, int16_t* data, uint32_t batch, const int16_t* tw, const uint16_t* perm,
                           uint32_t flags, hipStream_t st);

// Real FFT split (forward, after the N/2 CFFT) / merge (inverse, before it) passes.
hipError_t rfft_f32_stage_launch(int n_real, const float* p, float* out, uint32_t batch,
                                 const float* tw_rfft, hipStream_t st);
// Single-launch RFFT for the reference's canonical CFFT tables: tw = CFFT(n/2) twiddles,
// tw_rfft = twiddleCoef_rfft_n.  Forward writes the spectrum to `out` and, when pcopy is
// non-null, the inner CFFT output to pcopy (the reference leaves it in p).
hipError_t rfft_f32_fused_launch(int n_real, bool inverse, const float* p, float* pcopy, float* out, uint32_t batch,
                                 const float* tw, const float* tw_rfft, hipStream_t st);
hipError_t rfft_f32_merge_launch(int n_real, const float* p, float* out, uint32_t batch,
                                 const float* tw_rfft, hipStream_t st);

// RFFT q31 / q15 split (forward: src = [batch][N] CFFT(N/2) output -> dst [batch][2N]
// spectrum) or merge (inverse: src = [batch][2N] spectrum rows -> dst [batch][N] inverse
// CFFT input) pass.  ta / tb: device realCoef{A,B}; mod = the instance's modifier.
// forward arm_rfft_q31, N = 8192 (reference tables), inner CFFT + split in one launch (cfft_fixed.hip)
// forward arm_rfft_q31 / _q15 of fftLenReal = 2n, n = 256 .. 2048, in one launch (false: other n);
// rec = device_split_records(A, B, mod, n, sizeof word)
bool rfft_q31_r16_fused_launch(int n, int32_t* src, int32_t* dst, uint32_t batch, const int32_t* tw, const void* rec,
                               hipStream_t st);
bool rfft_q15_r16_fused_launch(int n, int16_t* src, int16_t* dst, uint32_t batch, const int16_t* tw, const void* rec,
                               hipStream_t st);
// inverse arm_rfft_q31 / _q15 of fftLenReal = 2n, n = 256 .. 2048, in one launch (merge fused into
// the radix-16 CFFT's first pass; false: other n); spec [batch][4n], dst [batch][2n]
bool rfft_q31_r16_inv_fused_launch(int n, const int32_t* spec, int32_t* dst, uint32_t batch, const int32_t* tw,
                                   const void* rec, hipStream_t st);
bool rfft_q15_r16_inv_fused_launch(int n, const int16_t* spec, int16_t* dst, uint32_t batch, const int16_t* tw,
                                   const void* rec, hipStream_t st);
// ... and fftLenReal = 8192 (the CFFT-4096 specialists), from the instance's realCoefA / B
hipError_t rfft_q31_8192_fused_launch(int32_t* src, int32_t* dst, uint32_t batch, const int32_t* tw, const int32_t* ta,
                                      const int32_t* tb, uint32_t mod, hipStream_t st);
hipError_t rfft_q31_8192_inv_fused_launch(const int32_t* spec, int32_t* dst, uint32_t batch, const int32_t* tw,
                                          const void* rec, hipStream_t st);
hipError_t rfft_q15_8192_inv_fused_launch(const int16_t* spec, int16_t* dst, uint32_t batch, const int16_t* tw,
                                          const void* rec, hipStream_t st);
hipError_t rfft_q15_8192_fused_launch(int16_t* src, int16_t* dst, uint32_t batch, const int16_t* tw, const int16_t* ta,
                                      const int16_t* tb, uint32_t mod, hipStream_t st);
hipError_t rfft_q31_pass_launch(bool inverse, int n, const int32_t* src, int32_t* dst, uint32_t batch,
                                const int32_t* ta, const int32_t* tb, uint32_t mod, hipStream_t st);
hipError_t rfft_q15_pass_launch(bool inverse, int n, const int16_t* src, int16_t* dst, uint32_t batch,
                                const int16_t* ta, const int16_t* tb, uint32_t mod, hipStream_t st);

// FIR: `batch` independent filters sharing one coefficient set, any of the five reference
// variants (kind).  hist: [batch][numTaps-1] streaming state (read, then overwritten with
// the new tail).  Element type: f32 float, q15/fast_q15 int16, q31/fast_q31 int32, q7 int8.
enum FirKind { kFirF32 = 0, kFirQ15 = 1, kFirQ31 = 2, kFirFastQ15 = 3, kFirFastQ31 = 4, kFirQ7 = 5,
               kFirF32Fma = 6 };   // kFirF32Fma: the opt-in fused-multiply-add f32 path (tolerance)
// done / seq (the synchronous drop-in): when the pass ends in one workgroup it also stores seq into
// the completion word done (runtime.cpp done_slot) and sets *flagged.
// arm_fir_q15 on the i8 matrix cores (fir_mfma.hip): false when the shape is not its (the caller
// then runs fir_q15_kernel)
bool fir_q15_mfma_launch(const int16_t* coeffs, int T, const int16_t* src, int16_t* dst, uint32_t B, uint32_t batch,
                         const int16_t* hist_in, hipStream_t st, bool fast = false);   // fast: arm_fir_fast_q15
// arm_fir_q7 likewise (numTaps <= 157)
bool fir_q7_mfma_launch(const int8_t* coeffs, int T, const int8_t* src, int8_t* dst, uint32_t B, uint32_t batch,
                        const int8_t* hist_in, hipStream_t st);
// arm_fir_q31 likewise (numTaps <= 161)
bool fir_q31_mfma_launch(const int32_t* coeffs, int T, const int32_t* src, int32_t* dst, uint32_t B, uint32_t batch,
                         const int32_t* hist_in, hipStream_t st);
hipError_t fir_run(int kind, const void* coeffs, int num_taps, const void* src, void* dst, uint32_t block_size,
                   uint32_t batch, void* hist, hipStream_t st, uint32_t* done = nullptr, uint32_t seq = 0,
                   bool* flagged = nullptr);

// Multirate FIR (fir.hip): `batch` independent decimators / interpolators sharing one
// coefficient set.  Decimator: outputs [batch][blockSize / M], hist [batch][numTaps - 1].
// Interpolator (phase_len = numTaps / L): outputs [batch][blockSize * L], hist
// [batch][phase_len - 1].  The interpolator takes kMrF32 / kMrQ15 / kMrQ31.
enum MrOp { kMrF32 = 0, kMrQ15 = 1, kMrQ31 = 2, kMrFastQ15 = 3, kMrFastQ31 = 4 };
hipError_t fir_decimate_run(int op, const void* coeffs, int num_taps, int M, const void* src, void* dst,
                            uint32_t block_size, uint32_t batch, void* hist, hipStream_t st);
hipError_t fir_interpolate_run(int op, const void* coeffs, int L, int phase_len, const void* src, void* dst,
                               uint32_t block_size, uint32_t batch, void* hist, hipStream_t st);
// Sparse FIR (fir.hip): `batch` streams sharing taps c[k] at delays D[k] (device arrays).
// circ_len == 0: block [batch][B] + history [batch][max_delay] (oldest first, updated);
// circ_len = L > 0: one stream whose samples are the reference's circular state buffer `src`
// of L words (block already written), tap k starting at circ_r0 - D[k] (wrapped), hist unused.
enum SpOp { kSpF32 = 0, kSpQ31 = 1, kSpQ15 = 2, kSpQ7 = 3 };
hipError_t fir_sparse_run(int op, const void* coeffs, const int32_t* delays, int num_taps, int max_delay,
                          const void* src, void* dst, uint32_t block_size, uint32_t batch, void* hist, int circ_len,
                          int circ_r0, hipStream_t st);
// FIR lattice (fir_lattice.hip): `batch` streams sharing numStages reflection coefficients;
// state [batch][numStages] = g_m at each stream's previous sample (updated in place).
enum LatOp { kLatF32 = 0, kLatQ31 = 1, kLatQ15 = 2 };
hipError_t fir_lattice_run(int op, const void* coeffs, int num_stages, const void* src, void* dst,
                           uint32_t block_size, uint32_t batch, void* state, hipStream_t st);
// Biquad cascades (biquad.hip): `batch` streams sharing numStages sections; coeffs 5 words per stage
// (q15: 6, {b0, 0, b1, b2, a1, a2}); state [batch][K numStages] in the reference's layout (K = 4, DF2T
// mono 2; 32x64: int64 words), updated in place.  Stereo: src / dst [batch][2 block_size] interleaved.
enum BqOp { kBqDf1F32 = 0, kBqDf1Q31 = 1, kBqDf1FastQ31 = 2, kBqDf1Q15 = 3, kBqDf1FastQ15 = 4, kBq32x64 = 5,
            kBqDf2TF32 = 6, kBqStereoDf2TF32 = 7 };
hipError_t biquad_run(int op, const void* coeffs, uint32_t num_stages, int post_shift, const void* src, void* dst,
                      uint32_t block_size, uint32_t batch, void* state, hipStream_t st);
// IIR lattice (iir_lattice.hip): `batch` streams sharing pk (num_stages reflection words) and pv
// (num_stages + 1 ladder words); state [batch][num_stages], the reference's live words, updated in place.
enum IirOp { kIirF32 = 0, kIirQ31 = 1, kIirQ15 = 2 };
hipError_t iir_lattice_run(int op, const void* pk, const void* pv, int num_stages, const void* src, void* dst,
                           uint32_t block_size, uint32_t batch, void* state, hipStream_t st);
// LMS / normalised LMS (lms.hip): per stream coeffs [batch][num_taps] (time-reversed, updated), state
// [batch][num_taps - 1] (oldest first, updated) and, normalised, energy_x0 [batch][2] words {energy, x0};
// mu is the type's word (f32: its bits); recip_table: the 64 device words of armRecipTableQ15 (q15
// normalised only).  kLmsQ31 has no normalised form here.
enum LmsOp { kLmsF32 = 0, kLmsQ31 = 1, kLmsQ15 = 2 };
hipError_t lms_run(int op, bool norm, const void* src, const void* ref, void* out, void* err, uint32_t block_size,
                   uint32_t batch, int num_taps, void* coeffs, void* state, void* energy_x0, int32_t mu,
                   int32_t post_shift, const int16_t* recip_table, hipStream_t st);

// MFCC f32 around the batched RFFT (mfcc_f32.hip): frame normalisation + window, then the
// spectrum -> Mel -> log -> DCT tail.  post needs mfcc_f32_post_lds(n, nb_mel) bytes of LDS.
// Fused single-launch MFCC for the reference's canonical CFFT tables (nb_mel <= n/2):
// tw = the inner CFFT(n/2) twiddles, twr = the RFFT split twiddles (twiddleCoef_rfft_n).
hipError_t mfcc_f32_fused_launch(int n, const float* src, const float* win, const float* tw, const float* twr,
                                 int nb_mel, const uint32_t* pos, const uint32_t* len, const uint32_t* off,
                                 const float* coefs, int nb_dct, const float* dct, float* dst, uint32_t batch,
                                 int total, hipStream_t st);
// The frame maximum of frame f is written to / read from maxv[f * maxv_stride].
hipError_t mfcc_f32_pre_launch(int n, const float* src, const float* win, float* x, float* maxv, uint32_t batch,
                               int maxv_stride, hipStream_t st);
// MFCC q31 around the batched q31 RFFT (mfcc_q31.hip); post needs mfcc_q31_post_lds bytes.
hipError_t mfcc_q31_pre_launch(int n, const int32_t* src, const int32_t* win, int32_t* x, int32_t* maxv,
                               uint32_t batch, int maxv_stride, hipStream_t st);
size_t mfcc_q31_post_lds(int n, int nb_mel);
hipError_t mfcc_q15_pre_launch(int n, const int16_t* src, const int16_t* win, int16_t* x, int16_t* maxv,
                               uint32_t batch, int maxv_stride, hipStream_t st);
hipError_t mfcc_q15_post_launch(int n, const int16_t* y, const int4* tw, const int16_t* maxv, int maxv_stride, int nb_mel,
                                int kmin, int kcnt, const int16_t* coefs,
                                const uint32_t* bf, int total, int nb_dct, const int16_t* dct, const int32_t* lut, int16_t* dst, uint32_t batch,
                                hipStream_t st);

hipError_t mfcc_q31_post_launch(int n, const int32_t* y, const int4* tw, const int32_t* maxv, int maxv_stride, int nb_mel,
                                int kmin, int kcnt, const int32_t* coefs,
                                const uint32_t* bf, int total, int nb_dct, const int32_t* dct, const int32_t* lut, int32_t* dst, uint32_t batch,
                                hipStream_t st);
size_t mfcc_f32_post_lds(int n, int nb_mel);
hipError_t mfcc_f32_post_launch(int n, const float* y, const float* maxv, int maxv_stride, int nb_mel,
                                const uint32_t* pos,
                                const uint32_t* len, const uint32_t* off, const float* coefs, int nb_dct,
                                const float* dct, float* dst, uint32_t batch, hipStream_t st);

// Row-major C[b] = A[b] (m x k) * B[b] (k x n), contiguous batch.
hipError_t mat_mult_f32_launch(int m, int k, int n, const float* a, const float* b, float* c,
                               uint32_t batch, hipStream_t st);

// Convolution / correlation family (conv.hip), bit-exact per op:
//   v[n] = sum_k x[k] * g[n-k], k ascending, g = h (convolution) or h time-reversed
//   (corr: correlation), for n in [first, first + num), stored at
//   y[item * sy + yoff + ydir * n].  x / h item strides sx / sh (0 = shared).
// kConvFastQ15 requires A >= B (the reference's x is the longer input).
enum ConvOp { kConvF32 = 0, kConvQ15 = 1, kConvQ31 = 2, kConvFastQ15 = 3, kConvFastQ31 = 4, kConvQ7 = 5,
              kConvFastOptQ15 = 6 };
struct ConvJob {
  int op;
  bool corr;
  const void* x; uint32_t A; uint64_t sx;
  const void* h; uint32_t B; uint64_t sh;
  void* y; uint64_t sy; int64_t yoff; int ydir;
  uint32_t first, num, batch;
};
hipError_t conv_family_run(const ConvJob& job, hipStream_t st);
// f32 windowed outputs through the FIR kernel (fir.hip): v[n] = sum_t w[n + t] c[t],
// w[j] = x[j - (T-1)], n = first .. first + num - 1, stored at y[item sy + off + dir (n - first)].
hipError_t fir_f32_conv_pass(const float* c, uint64_t cstride, int T, const float* x, uint64_t sx, uint32_t A,
                             uint32_t first, float* y, uint64_t sy, int64_t off, int dir, uint32_t num, uint32_t batch,
                             hipStream_t st);

// Row-major q15 / q31 C[b] = A[b] * B[b] (arm_mat_mult_q15 / _q31 semantics, bit-exact):
// byte-sliced planes on the i8 matrix cores (mat_mult_fixed.hip).
hipError_t mat_mult_q15_launch(int m, int k, int n, const int16_t* a, const int16_t* b, int16_t* c, uint32_t batch,
                               hipStream_t st);
hipError_t mat_mult_q31_launch(int m, int k, int n, const int32_t* a, const int32_t* b, int32_t* c, uint32_t batch,
                               hipStream_t st);
// Row-major q7 C[b] = A[b] * B[b] (arm_mat_mult_q7 semantics, bit-exact): one i8 MFMA plane
// (mat_mult_q7.hip).
hipError_t mat_mult_q7_launch(int m, int k, int n, const int8_t* a, const int8_t* b, int8_t* c, uint32_t batch,
                              hipStream_t st);
// arm_mat_mult_fast_q15 (exact i8-plane GEMM, modular q31 sum, (q15)(sum >> 15)) and
// arm_mat_mult_fast_q31 (VALU: sum of per-product (a*b) >> 32, output << 1).
hipError_t mat_mult_fast_q15_launch(int m, int k, int n, const int16_t* a, const int16_t* b, int16_t* c,
                                    uint32_t batch, hipStream_t st);
hipError_t mat_mult_fast_q31_launch(int m, int k, int n, const int32_t* a, const int32_t* b, int32_t* c,
                                    uint32_t batch, hipStream_t st);
// Complex C[b] = A[b] (m x k) * B[b] (k x n), interleaved (re, im) words, contiguous batch; m, k, n
// count complex elements.  The real kernels above on the embedded product A (m x 2k) * B' (2k x 2n),
// B' formed while staging B: f32 is the k-ascending fmaf chain re = fma(-b, d, fma(a, c, re)),
// im = fma(b, c, fma(a, d, im)); q15 / q31 are bit-exact (arm_mat_cmplx_mult_q15 / _q31: wrapping q63
// sum, >> 15 / >> 31, saturated).
hipError_t mat_cmplx_mult_f32_launch(int m, int k, int n, const float* a, const float* b, float* c, uint32_t batch,
                                     hipStream_t st);
hipError_t mat_cmplx_mult_q15_launch(int m, int k, int n, const int16_t* a, const int16_t* b, int16_t* c,
                                     uint32_t batch, hipStream_t st);
hipError_t mat_cmplx_mult_q31_launch(int m, int k, int n, const int32_t* a, const int32_t* b, int32_t* c,
                                     uint32_t batch, hipStream_t st);
// bt (n rows of k complex words) = b (k rows of n complex words) transposed: the pScratch contents of
// arm_mat_cmplx_mult_q15 (arm_mat_cmplx_mult_q15.c:433-468).
hipError_t mat_cmplx_trans_q15_launch(int k, int n, const int16_t* b, int16_t* bt, hipStream_t st);

// Inverse, Cholesky, LDLT and triangular solves over `batch` contiguous row-major n x n items (solves: t n x n,
// a and x n x cols), bit-exact with the reference's scalar branches, failures included (mat_solve.hip).
// status (may be null): one int32 per item, 0 / ARM_MATH_SINGULAR / ARM_MATH_DECOMPOSITION_FAILURE.  Any
// n >= 1: an item lives in LDS while a workgroup's share fits kMatSolveLds (inverse, 2 n^2 words: n <= 143;
// Cholesky and LDLT, n (n | 1) words: n <= 201), past that one workgroup works on it in global memory; the
// solves read t and a from global memory and keep x in LDS as well up to n = 64.
// The inverse destroys src as the reference does; cholesky's dst may be src, a solve's x may be a.
constexpr size_t kMatSolveLds = 160 * 1024;
hipError_t mat_inverse_f32_launch(int n, float* src, float* dst, uint32_t batch, int32_t* status, hipStream_t st);
hipError_t mat_cholesky_f32_launch(int n, const float* src, float* dst, uint32_t batch, int32_t* status,
                                   hipStream_t st);
hipError_t mat_ldlt_f32_launch(int n, const float* src, float* pl, float* pd, uint16_t* pp, uint32_t batch,
                               hipStream_t st);
hipError_t mat_solve_tri_f32_launch(bool lower, int n, int cols, const float* t, const float* a, float* x,
                                    uint32_t batch, int32_t* status, hipStream_t st);

// Element-wise add / sub / scale, the transposes and matrix x vector, bit-exact with the reference's scalar
// branches (mat_basic.hip); T is float, int32_t (q31), int16_t (q15) and, for vec_mult, int8_t (q7).
// mat_ew_launch: d[i] = a[i] op b[i] over `count` words (the whole batch as one flat array; b unused by
// kMatScale, which takes scale and, fixed point only, shift: q31 -1..30, q15 -16..15, else
// hipErrorInvalidValue).  d may be a or b exactly.
enum : int { kMatAdd = 0, kMatSub = 1, kMatScale = 2 };
template <typename T>
hipError_t mat_ew_launch(int op, const T* a, const T* b, T* d, size_t count, T scale, int shift, hipStream_t st);
// dst[i] (cols x rows) = transpose of src[i] (rows x cols) for `batch` contiguous items of elemBytes-byte
// elements (1, 2, 4, 8; a complex element is one (re, im) pair, not conjugated).  src and dst must not overlap.
hipError_t mat_trans_launch(int elemBytes, int rows, int cols, const void* src, void* dst, uint32_t batch,
                            hipStream_t st);
// dst[i] (rows words) = mat_i (rows x cols) x vec[i] (cols words); mat_i = mat + i * matStride elements
// (0: one matrix for every item).  int16_t and int32_t read row r where the reference's uint16_t offset
// puts it (mat_basic.hip vm_row_offset), inside the item.
template <typename T>
hipError_t mat_vec_mult_launch(int rows, int cols, const T* mat, size_t matStride, const T* vec, T* dst,
                               uint32_t batch, hipStream_t st);

// Complex math and max / min, bit-exact with the reference's scalar branches (cmplx_math.hip); T is float,
// int32_t (q31), int16_t (q15) and, for the searches, int8_t (q7).  Complex vectors are interleaved (re, im).
// cmplx_ew_launch: `count` complex samples (the whole batch as one flat array).  kCmMag / kCmMagSquared write one
// word per sample, the others two; b is the second complex vector (kCmMultCmplx), the real vector (kCmMultReal)
// or unused.  d may be a (or b) exactly for kCmConj / kCmMultCmplx / kCmMultReal; no other overlap.  lut: the
// device copy of sqrt_initial_lut_q31 (read by the q31 / q15 kCmMag only).  kCmMagFast (int16_t only) is
// arm_cmplx_mag_fast_q15: one word per sample, no lut.
enum : int { kCmMag = 0, kCmMagSquared = 1, kCmConj = 2, kCmMultCmplx = 3, kCmMultReal = 4, kCmMagFast = 5 };
template <typename T>
hipError_t cmplx_ew_launch(int op, const T* a, const T* b, T* d, size_t count, const int32_t* lut, hipStream_t st);
// re[i], im[i] = the complex dot product of a[i] and b_i (n samples each), b_i = b + i * bStride samples (0: one
// b for every item).  R: float, int64_t (q31: the two 64-bit sums as they are) or int32_t (q15: >> 6).  n == 0
// stores zeros.  The float chain is ordered sample by sample.
template <typename T, typename R>
hipError_t cmplx_dot_launch(const T* a, const T* b, size_t bStride, uint32_t n, R* re, R* im, uint32_t batch,
                            hipStream_t st);
// result[i], index[i] = the maximum (max) or minimum of src[i] (n words, n > 0) and the first index that holds it;
// NaN as the reference's strict comparisons treat it.
template <typename T>
hipError_t search_launch(bool max, const T* src, uint32_t n, T* result, uint32_t* index, uint32_t batch,
                         hipStream_t st);

// The statistics functions, bit-exact with the reference's scalar branches (statistics.hip).  One result word per
// item of n contiguous words; items n words apart.
// stat_sum_launch: T float, int32_t (q31), int16_t (q15), int8_t (q7); R the reference's result type (as T, but
// power: float, int64_t, int64_t, int32_t).  b: the second source of kStMse, otherwise unused.  lut: the device copy
// of sqrt_initial_lut_q31 (read by the q31 kStRms / kStStd only).  n == 0 stores what the empty sums give (the
// caller refuses the integer forms that would divide by zero).  The float sums are ordered chains.
enum : int { kStMean = 0, kStPower = 1, kStRms = 2, kStVar = 3, kStStd = 4, kStMse = 5, kStAccumulate = 6,
             kStDot = 7 /* dot_prod_launch only */, kStWavg = 8 /* weighted_average_launch only */ };
template <typename T, typename R>
hipError_t stat_sum_launch(int op, const T* a, const T* b, uint32_t n, R* result, uint32_t batch, const int32_t* lut,
                           hipStream_t st);
// arm_{max,min,absmax,absmin}[_no_idx]: abs maps every element to (x > 0) ? x : -x (saturating) first; index null:
// the _no_idx forms, which for float without abs start from -FLT_MAX / FLT_MAX (and accept n == 0) instead of
// element 0.  Otherwise n > 0.
template <typename T>
hipError_t stat_search_launch(bool max, bool abs, const T* src, uint32_t n, T* result, uint32_t* index, uint32_t batch,
                              hipStream_t st);
// arm_sqrt_q15 on the host (the scalar drop-in): 0 for in <= 0.
int16_t sqrt_q15_host(int16_t in);

// The basic math functions, bit-exact with the reference's scalar branches (basic_math.hip).
// basic_ew_launch: d[i] = op(a[i], b[i]) over `count` words (the whole batch as one flat array).  T is float,
// int32_t (q31), int16_t (q15), int8_t (q7) for kBmAdd .. kBmNegate (kBmShift: fixed point only) and uint32_t,
// uint16_t, uint8_t for kBmAnd .. kBmNot; anything else is hipErrorInvalidValue.  b: the second source of add, sub,
// mult, and, or, xor, otherwise unused.  s0: the offset, the scale or clip's low; s1: clip's high.  sh: kBmShift:
// shiftBits, -31 .. 31; kBmScale: the reference's kShift, q31 shift + 1 (-31 .. 31, negative: a right shift), q15
// 15 - shift and q7 7 - shift (0 .. 31).  The caller checks the ranges.  d may be a or b exactly.
enum : int {
  kBmAdd = 0, kBmSub, kBmMult, kBmOffset, kBmScale, kBmShift, kBmClip, kBmAbs, kBmNegate, kBmAnd, kBmOr, kBmXor,
  kBmNot
};
template <typename T>
hipError_t basic_ew_launch(int op, const T* a, const T* b, T* d, size_t count, T s0, T s1, int sh, hipStream_t st);
// result[i] = arm_dot_prod_* of a[i] and b_i (n words each), b_i = b + i * bStride words (0: one b for every item).
// R: float, int64_t (q31: every product >> 14; q15: exact products) or int32_t (q7).  n == 0 stores zeros.  The
// float sum is one ordered chain sum + a*b.  An operation of the sum kernels of statistics.hip.
template <typename T, typename R>
hipError_t dot_prod_launch(const T* a, const T* b, size_t bStride, uint32_t n, R* result, uint32_t batch,
                           hipStream_t st);

// The support functions, bit-exact with the reference's scalar branches (support.hip, sort.hip).
// support_convert_launch<S, D>: d[i] = the reference's arm_<S>_to_<D> of s[i] over `count` words (the whole batch as
// one flat array); S == D is arm_copy_*.  S, D: float, int32_t (q31), int16_t (q15), int8_t (q7).  d may equal s
// exactly where the element widths are equal.  float -> q outside the range where the reference's C is defined
// saturates by sign, NaN gives 0.
template <typename S, typename D>
hipError_t support_convert_launch(const S* s, D* d, size_t count, hipStream_t st);
// d[i] = value over `count` words (arm_fill_*).
template <typename T>
hipError_t support_fill_launch(T value, T* d, size_t count, hipStream_t st);
// out[i][d] = (sum_v in[i][v][d] * w_i[v]) / (sum_v w_i[v]), both sums ordered chains over v from 0.0f, the product
// rounded before the add; w_i = w + i * wStride words (0: one weight vector for every item).
hipError_t barycenter_launch(const float* in, const float* w, size_t wStride, float* out, uint32_t nbVectors,
                             uint32_t vecDim, uint32_t batch, hipStream_t st);
// result[i] = (sum_k a[i][k] * w_i[k]) / (sum_k w_i[k]): two ordered chains and one division (n == 0: 0 / 0).  An
// operation (kStWavg) of the f32 chain kernels of statistics.hip.
hipError_t weighted_average_launch(const float* a, const float* w, size_t wStride, uint32_t n, float* result,
                                   uint32_t batch, hipStream_t st);
// Sorts each of `batch` items of n 32-bit words (items n words apart) by the IEEE total order of the words read as
// float32 (ascending: negative NaNs, -Inf .. -0.0, +0.0 .. +Inf, positive NaNs; descending: the reverse).  dst may
// equal src exactly; otherwise src is only read.  n <= 2^31.
constexpr uint32_t kSortWaveMax = 256;     // padded length up to which one wave sorts an item in registers
constexpr uint32_t kSortLdsMax = 16384;    // padded length up to which one workgroup sorts an item in LDS (64 KiB)
hipError_t sort_launch(const uint32_t* src, uint32_t* dst, uint32_t n, bool ascending, uint32_t batch,
                       hipStream_t st);

// The distance functions, bit-exact with the reference's scalar branches (distance.hip).
// result[i] = arm_<op>_distance_f32 of a + i * n and b + i * bStride (n words each; bStride 0: one b for every item).
// The sums are ordered chains.  wa / wb (kDsCorrelation only, both or neither): where the shifted words x + (-mean)
// of a and b are stored, item for item (the drop-in passes a and b themselves); null: the sources are only read.
// kDsChebyshev needs n > 0.
enum : int {
  kDsBraycurtis = 0, kDsCanberra, kDsChebyshev, kDsCityblock, kDsCorrelation, kDsCosine, kDsEuclidean,
  kDsJensenshannon
};
hipError_t distance_f32_launch(int op, const float* a, const float* b, size_t bStride, uint32_t n, float* result,
                               uint32_t batch, float* wa, float* wb, hipStream_t st);
// result[i] = arm_<op>_distance of the n booleans packed at a + i * ceil(n / 32) and b + i * bStride words; of a
// partial last word the top n % 32 bits count; no word past ceil(n / 32) is read.
enum : int {
  kBdDice = 0, kBdHamming, kBdJaccard, kBdKulsinski, kBdRogerstanimoto, kBdRussellrao, kBdSokalmichener,
  kBdSokalsneath, kBdYule
};
hipError_t boolean_distance_launch(int op, const uint32_t* a, const uint32_t* b, size_t bStride, uint32_t n,
                                   float* result, uint32_t batch, hipStream_t st);
// arm_dtw_init_window_q7 into `batch` contiguous rows x cols windows; type 1 (Sakoe-Chiba) or 3 (slanted band).
hipError_t dtw_init_window_launch(int type, int32_t windowSize, int8_t* dst, uint32_t rows, uint32_t cols,
                                  uint32_t batch, hipStream_t st);
// arm_dtw_distance_f32 on `batch` contiguous rows x cols matrices (rows, cols > 0): dtw receives every cost cell,
// status[i] (may be null) 0 or -1 (ARM_MATH_ARGUMENT_ERROR), result[i] the distance where the status is 0.  window:
// null, or item i's at window + i * wStride bytes (0: one for every item).
hipError_t dtw_distance_launch(const float* dist, const int8_t* window, size_t wStride, float* dtw, uint32_t rows,
                               uint32_t cols, float* result, int32_t* status, uint32_t batch, hipStream_t st);
// arm_dtw_path_f32: path + i * 2 * (rows + cols) and pathLength[i] (0: the walk cannot leave a cell); rows, cols in
// 1 .. 32768.
hipError_t dtw_path_launch(const float* dtw, uint32_t rows, uint32_t cols, int16_t* path, uint32_t* pathLength,
                           uint32_t batch, hipStream_t st);

// vexp / vlog, the log-domain statistics, the SVMs and naive Bayes, bit-exact with the reference's scalar branches
// and the pinned glibc's expf / logf (ml.hip).
// d[i] = expf(a[i]) or logf(a[i]) over `count` words (the whole batch as one flat array); d may be a exactly.
enum : int { kFmExp = 0, kFmLog = 1 };
hipError_t fast_math_launch(int op, const float* a, float* d, size_t count, hipStream_t st);
// result[i] = arm_entropy_f32 / arm_kullback_leibler_f32 / arm_logsumexp_f32 / arm_logsumexp_dot_prod_f32 of a + i * n
// (and b + i * bStride: the second source of kLdKullbackLeibler and kLdLogsumexpDot; bStride 0: one b for every
// item).  The two logsumexp forms need n > 0.  tmp (kLdLogsumexpDot only, may be null): where a + b is stored, item
// for item (the drop-in's pTmpBuffer).
enum : int { kLdEntropy = 0, kLdKullbackLeibler, kLdLogsumexp, kLdLogsumexpDot };
hipError_t logdom_launch(int op, const float* a, const float* b, size_t bStride, uint32_t n, float* result,
                         uint32_t batch, float* tmp, hipStream_t st);
// arm_svm_<kind>_predict_f32 of the `items` vectors at in + i * dim against one model (device pointers): result[i] =
// classes[sum <= 0 ? 0 : 1], decision[i] (may be null) = the final sum.  degree, coef0: polynomial; gamma: polynomial
// and rbf.  svm_model_staged: whether the kernel holds the model in LDS (otherwise it reads it from global memory).
enum : int { kSvmLinear = 0, kSvmPolynomial, kSvmRbf };
struct SvmModel {
  uint32_t nsv, dim;
  float intercept;
  const float* dual;
  const float* sv;
  const int32_t* classes;
  int32_t degree;
  float coef0, gamma;
};
hipError_t svm_predict_launch(int kind, const SvmModel& m, const float* in, int32_t* result, float* decision,
                              uint32_t items, hipStream_t st);
bool svm_model_staged(uint32_t nsv, uint32_t dim);
// arm_gaussian_naive_bayes_predict_f32 of the `items` vectors at in + i * dim: prob + i * classes receives the
// classes' words, cls[i] the index arm_max_f32 gives on them.  classes > 0.
struct BayesModel {
  uint32_t dim, classes;
  const float* theta;
  const float* sigma;
  const float* priors;
  float eps;
};
hipError_t bayes_predict_launch(const BayesModel& m, const float* in, float* prob, uint32_t* cls, uint32_t items,
                                hipStream_t st);
bool bayes_model_staged(uint32_t classes, uint32_t dim);

// Linear, bilinear and cubic-spline interpolation, bit-exact with the reference's scalar code (interp.hip).
// y[i] = arm_linear_interp_<t>(x[i]) over `count` samples against one table of nValues > 0 words; T is int32_t,
// int16_t or int8_t and x is in 12.20.  linear_interp_staged: whether the kernel holds the table in LDS.
hipError_t linear_interp_f32_launch(const float* table, uint32_t nValues, float x1, float xSpacing, const float* x,
                                    float* y, uint32_t count, hipStream_t st);
template <typename T>
hipError_t linear_interp_q_launch(const T* table, uint32_t nValues, const int32_t* x, T* y, uint32_t count,
                                  hipStream_t st);
bool linear_interp_staged(uint32_t nValues, uint32_t wordBytes);
// out[i] = arm_bilinear_interp_<t>(px[i], py[i]) against one rows x cols table, rows * cols < 2^31.
hipError_t bilinear_interp_f32_launch(const float* table, uint32_t rows, uint32_t cols, const float* px,
                                      const float* py, float* out, uint32_t count, hipStream_t st);
template <typename T>
hipError_t bilinear_interp_q_launch(const T* table, uint32_t rows, uint32_t cols, const int32_t* px, const int32_t* py,
                                    T* out, uint32_t count, hipStream_t st);
// arm_spline_init_f32 of `batch` items: knots x + i * xStride (0: one vector for every item), values y + i * n,
// coeffs + i * 3 (n - 1) (b, c, d) and temp + i * (2 n - 1) (u, z); n >= 2, type 0 or 1.
hipError_t spline_init_launch(int type, const float* x, size_t xStride, const float* y, uint32_t n, float* coeffs,
                              float* temp, uint32_t batch, hipStream_t st);
// arm_spline_f32 of `batch` items: blockSize queries at xq + i * xqStride (0: one vector for every item) into
// dst + i * blockSize.
hipError_t spline_launch(const float* x, size_t xStride, const float* y, const float* coeffs, uint32_t n,
                         const float* xq, size_t xqStride, float* dst, uint32_t blockSize, uint32_t batch,
                         hipStream_t st);
// one sample on the host: the scalar drop-ins
float linear_interp_f32_host(const float* table, uint32_t nValues, float x1, float xSpacing, float x);
int32_t linear_interp_q31_host(const int32_t* table, uint32_t nValues, int32_t x);
int16_t linear_interp_q15_host(const int16_t* table, uint32_t nValues, int32_t x);
int8_t linear_interp_q7_host(const int8_t* table, uint32_t nValues, int32_t x);
float bilinear_interp_f32_host(const float* table, uint32_t rows, uint32_t cols, float X, float Y);
int32_t bilinear_interp_q31_host(const int32_t* table, uint32_t rows, uint32_t cols, int32_t X, int32_t Y);
int16_t bilinear_interp_q15_host(const int16_t* table, uint32_t rows, uint32_t cols, int32_t X, int32_t Y);
int8_t bilinear_interp_q7_host(const int8_t* table, uint32_t rows, uint32_t cols, int32_t X, int32_t Y);

// The quaternion functions, bit-exact with the reference's scalar branches (quaternion.hip), over n quaternions at
// 4 words each.  d: n norms (kQtNorm), n quaternions, or n rotations of 9 words (kQtToRotation); a: n rotations for
// kQtFromRotation.  b (kQtProduct only): the second factor, item i's at b + i * bStride, bStride 4 or 0 (one for
// every item).  d may be a (or b at bStride 4) exactly where both hold quaternions.
enum : int { kQtNorm = 0, kQtInverse, kQtConjugate, kQtNormalize, kQtProduct, kQtToRotation, kQtFromRotation };
hipError_t quaternion_launch(int op, const float* a, const float* b, uint32_t bStride, float* d, uint32_t n,
                             hipStream_t st);

}  // namespace mi355x
