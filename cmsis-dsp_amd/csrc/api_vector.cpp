// C ABI of the stateless vector and matrix families: the f32 solves, the basic matrix functions, complex math
// with max / min, statistics, basic math, the support functions, interpolation and the quaternions, each as the
// drop-in of arm_math.h and the batched device form of arm_math_mi355x.h.  Every family describes a call as a table
// of operands and hands it to one driver (VecCall); api.cpp holds the transforms, filters, convolution, MFCC and the
// matrix multiplies.
#include <type_traits>

#include "../../include/arm_math.h"
#include "../../include/arm_math_mi355x.h"
#include "api_status.hpp"
#include "kernels.hpp"
#include "runtime.hpp"

using namespace mi355x;

namespace {

// ---- the call driver --------------------------------------------------------------------------------------
// The calling contract of these families ("Calling contract of the vector and matrix families"):
//   * sync (the drop-in): operands are host or device pointers.  A null operand is refused first; void functions
//     report it through the last error, the matrix functions that return a status through that alone (kQuietNull).
//     Host words are staged into device scratch (slot = operand index), a device pointer is used in place, and the
//     call returns after the stream has drained.
//   * batched: operands are device pointers, the call only enqueues.  A null operand is refused after the family's
//     parameter refusals and its empty-call rule, with ARM_MATH_ARGUMENT_ERROR and no last error.
//   * the overlap rule, on the pointers the kernel is given (the caller's in a batched call; the staged ones in a
//     sync call, where host operands that are exactly the same buffer share one scratch slot and any other host
//     overlap has gone): a result must not overlap a source, except that it may be exactly the source where the
//     source allows it (kExactOk), and must not overlap another result.  A refusal is hipErrorInvalidValue under
//     `what`.  The matrix functions and the solves have no overlap rule (kNoOverlapRule).
enum : unsigned { kIn = 1, kOut = 2, kExactOk = 4 };        // Operand::role: a source, a result, or both
enum : unsigned { kNoOverlapRule = 1, kQuietNull = 2 };     // VecCall::flags
constexpr int kMaxOperands = 6;

// One operand of a call: its byte span over the whole call.  A sync call copies a host source in (a span without
// words is not copied) and a host result out.
struct Operand {
  const void* p;
  size_t bytes;
  unsigned role;
};

bool spans_overlap(const void* d, size_t db, const void* s, size_t sb, bool exactOk) {
  if (!db || !sb) return false;
  if (d == s && db == sb && exactOk) return false;
  const uintptr_t d0 = (uintptr_t)d, s0 = (uintptr_t)s;
  return d0 < s0 + sb && s0 < d0 + db;
}

struct VecCall {
  const char* what;
  bool sync;
  void* stream;          // batched calls; a sync call runs on sync_stream()
  unsigned flags;
  int n;
  Operand op[kMaxOperands];

  bool any_null() const {
    for (int i = 0; i < n; ++i)
      if (!op[i].p) return true;
    return false;
  }

  // The first test of a helper: a drop-in refuses a null operand before anything else.
  bool null_in_sync() const {
    if (!sync || !any_null()) return false;
    if (!(flags & kQuietNull)) set_error(hipErrorInvalidValue, what);
    return true;
  }

  bool overlap_refused(void* const* p) const {
    if (flags & kNoOverlapRule) return false;
    for (int i = 0; i < n; ++i) {
      if (!(op[i].role & kOut)) continue;
      for (int j = 0; j < n; ++j) {
        const bool source = op[j].role & kIn;
        if (j == i || (!source && j < i)) continue;          // a pair of results is tested once
        if (spans_overlap(p[i], op[i].bytes, p[j], op[j].bytes, source && (op[j].role & kExactOk))) return true;
      }
    }
    return false;
  }

  // The last step of a helper, after its parameter refusals and its empty-call rule.  launch(p, st) -> hipError_t
  // receives the device pointer of every operand (p[i] for op[i], null past n) and the stream.
  template <typename Launch>
  arm_status run(Launch&& launch) const {
    void* p[kMaxOperands] = {};
    if (!sync) {
      if (any_null()) return ARM_MATH_ARGUMENT_ERROR;
      for (int i = 0; i < n; ++i) p[i] = const_cast<void*>(op[i].p);
      return batch_status(overlap_refused(p) ? hipErrorInvalidValue : launch(p, (hipStream_t)stream), what);
    }
    hipStream_t st = sync_stream();
    bool dev[kMaxOperands];
    for (int i = 0; i < n; ++i) {
      dev[i] = is_device_ptr(op[i].p);
      p[i] = dev[i] ? const_cast<void*>(op[i].p) : scratch(op[i].bytes + 16, i);
      for (int j = 0; j < i; ++j)          // exact alias (add / sub / scale in place): one staged copy
        if (!dev[i] && op[j].p == op[i].p && op[j].bytes == op[i].bytes) p[i] = p[j];
      if (!p[i]) { set_error(hipErrorOutOfMemory, what); return ARM_MATH_ARGUMENT_ERROR; }
    }
    HostIO io(st);
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i)
      if (!dev[i] && (op[i].role & kIn) && op[i].bytes) e = io.in(p[i], op[i].p, op[i].bytes);
    if (e == hipSuccess) e = overlap_refused(p) ? hipErrorInvalidValue : launch(p, st);
    for (int i = 0; i < n && e == hipSuccess; ++i)
      if (!dev[i] && (op[i].role & kOut)) e = io.out(const_cast<void*>(op[i].p), p[i], op[i].bytes);
    if (e == hipSuccess) e = io.finish();
    return batch_status(e, what);
  }

  // run() for the solves, whose items report a status word.  launch(p, d_status, st): a batched call passes the
  // caller's d_status (may be null) through; a sync call stages one word out as one more result operand and returns
  // it once the call itself has succeeded.
  template <typename Launch>
  arm_status run_with_status(int32_t* d_status, Launch&& launch) {
    if (!sync) return run([&](void* const* p, hipStream_t st) { return launch(p, d_status, st); });
    int32_t status = ARM_MATH_SUCCESS;
    const int k = n++;
    op[k] = {&status, sizeof(status), kOut};
    const arm_status r = run([&](void* const* p, hipStream_t st) { return launch(p, (int32_t*)p[k], st); });
    return r != ARM_MATH_SUCCESS ? r : (arm_status)status;
  }
};

// a refusal of a parameter: a drop-in (most are void) also records it
arm_status refuse(bool sync, const char* what) {
  if (sync) set_error(hipErrorInvalidValue, what);
  return ARM_MATH_ARGUMENT_ERROR;
}

// The reductions over a second source at a stride: the dot products (words 1), the weighted average (words 1) and
// the complex dot products (words 2: interleaved samples and two results, otherwise r1 is null).  bStride (samples;
// the drop-in passes n): 0 shares one b, otherwise >= n.  n == 0 stores what the empty sums give.
// launch(a, b, r0, r1, st) -> hipError_t.
template <typename T, typename R, typename Launch>
arm_status strided_reduce(int words, const T* a, const T* b, uint32_t bStride, uint32_t n, R* r0, R* r1, bool sync,
                          uint32_t batch, void* stream, const char* what, Launch&& launch) {
  const size_t ab = sizeof(T) * words * n * batch, rb = sizeof(R) * batch;
  const size_t bb = sizeof(T) * words * ((size_t)bStride * (batch - 1) + n);
  const VecCall c{what, sync, stream, 0, words == 2 ? 4 : 3, {{a, ab, kIn}, {b, bb, kIn}, {r0, rb, kOut}, {r1, rb, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (bStride != 0 && bStride < n) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return launch((const T*)p[0], (const T*)p[1], (R*)p[2], (R*)p[3], st);
  });
}

// The max / min searches of cmplx_math.hip (abs false, idx true) and the abs / no-index searches of statistics.hip
// (idx false: the _no_idx forms, index unused).  n == 0 is refused where the reference reads pSrc[0].
template <typename T>
arm_status search(bool max, bool abs, bool idx, const T* src, uint32_t n, T* result, uint32_t* index, bool sync,
                  uint32_t batch, void* stream, const char* what) {
  const VecCall c{what, sync, stream, 0, idx ? 3 : 2,
                  {{src, sizeof(T) * n * batch, kIn}, {result, sizeof(T) * batch, kOut},
                   {index, sizeof(uint32_t) * batch, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  const bool fromStart = std::is_same<T, float>::value && !abs && !idx;   // max / min_no_idx_f32 read no pSrc[0]
  if (n == 0 && !fromStart) return refuse(sync, what);
  return c.run([&](void* const* p, hipStream_t st) {
    if (!abs && idx) return search_launch<T>(max, (const T*)p[0], n, (T*)p[1], (uint32_t*)p[2], batch, st);
    return stat_search_launch<T>(max, abs, (const T*)p[0], n, (T*)p[1], (uint32_t*)p[2], batch, st);
  });
}

}  // namespace

// ---- inverse, Cholesky, LDLT, triangular solves (f32) ---------------------------------
// matrix_functions.h:659-777; kernels and the reference bodies they restate: mat_solve.hip.  The shape rules
// are those the reference states under ARM_MATH_MATRIX_CHECK, applied always, plus a / dst agreement in the
// solves.  No overlap rule; a null instance or pData is a status, not a last error.
namespace {
using MatF = arm_matrix_instance_f32;
constexpr unsigned kMatrixCall = kNoOverlapRule | kQuietNull;

bool square(const MatF* m) { return m->numRows == m->numCols; }

// The inverse writes src back: the reference destroys it, and its final words are part of the contract.  Cholesky
// stages dst in as well: its strict upper triangle, and the columns past a failure, are never written.
arm_status solve_square(bool inverse, const MatF* src, MatF* dst, bool sync, uint32_t batch, int32_t* d_status,
                        void* stream, const char* what) {
  if (!src || !dst) return ARM_MATH_ARGUMENT_ERROR;
  const int n = src->numRows;
  const size_t bytes = sizeof(float) * n * n * batch;
  VecCall c{what, sync, stream, kMatrixCall, 2,
            {{src->pData, bytes, inverse ? kIn | kOut : kIn}, {dst->pData, bytes, inverse ? kOut : kIn | kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(src) || !square(dst) || src->numRows != dst->numRows) return ARM_MATH_SIZE_MISMATCH;
  if (batch == 0 || n == 0) return ARM_MATH_SUCCESS;
  return c.run_with_status(d_status, [&](void* const* p, int32_t* ds, hipStream_t st) {
    return inverse ? mat_inverse_f32_launch(n, (float*)p[0], (float*)p[1], batch, ds, st)
                   : mat_cholesky_f32_launch(n, (const float*)p[0], (float*)p[1], batch, ds, st);
  });
}

arm_status solve_ldlt(const MatF* src, MatF* pl, MatF* pd, uint16_t* pp, bool sync, uint32_t batch, void* stream,
                      const char* what) {
  if (!src || !pl || !pd) return ARM_MATH_ARGUMENT_ERROR;
  const int n = src->numRows;
  const size_t bytes = sizeof(float) * n * n * batch;
  VecCall c{what, sync, stream, kMatrixCall, 4,
            {{src->pData, bytes, kIn}, {pl->pData, bytes, kOut}, {pd->pData, bytes, kOut},
             {pp, sizeof(uint16_t) * n * batch, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(src) || !square(pl) || !square(pd) || pl->numRows != pd->numRows || src->numRows != pl->numRows)
    return ARM_MATH_SIZE_MISMATCH;
  if (batch == 0 || n == 0) return ARM_MATH_SUCCESS;
  // the function cannot fail: the drop-in's status word is cleared, the batched form has none
  return c.run_with_status(nullptr, [&](void* const* p, int32_t* ds, hipStream_t st) {
    hipError_t e = ds ? hipMemsetAsync(ds, 0, sizeof(int32_t), st) : hipSuccess;
    if (e == hipSuccess)
      e = mat_ldlt_f32_launch(n, (const float*)p[0], (float*)p[1], (float*)p[2], (uint16_t*)p[3], batch, st);
    return e;
  });
}

arm_status solve_tri(bool lower, const MatF* t, const MatF* a, MatF* dst, bool sync, uint32_t batch,
                     int32_t* d_status, void* stream, const char* what) {
  if (!t || !a || !dst) return ARM_MATH_ARGUMENT_ERROR;
  const int n = t->numRows, cols = a->numCols;
  const size_t xb = sizeof(float) * n * cols * batch;
  // dst is staged in as well: a failing solve leaves most of its words alone
  VecCall c{what, sync, stream, kMatrixCall, 3,
            {{t->pData, sizeof(float) * n * n * batch, kIn}, {a->pData, xb, kIn}, {dst->pData, xb, kIn | kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(t) || t->numRows != a->numRows || a->numRows != dst->numRows || a->numCols != dst->numCols)
    return ARM_MATH_SIZE_MISMATCH;
  if (batch == 0 || n == 0 || cols == 0) return ARM_MATH_SUCCESS;
  return c.run_with_status(d_status, [&](void* const* p, int32_t* ds, hipStream_t st) {
    return mat_solve_tri_f32_launch(lower, n, cols, (const float*)p[0], (const float*)p[1], (float*)p[2], batch, ds, st);
  });
}
}  // namespace

extern "C" {
arm_status arm_mat_inverse_f32(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pDst) {
  return solve_square(true, pSrc, pDst, true, 1, nullptr, nullptr, "arm_mat_inverse_f32");
}
arm_status arm_mat_cholesky_f32(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pDst) {
  return solve_square(false, pSrc, pDst, true, 1, nullptr, nullptr, "arm_mat_cholesky_f32");
}
arm_status arm_mat_ldlt_f32(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pl,
                            arm_matrix_instance_f32* pd, uint16_t* pp) {
  return solve_ldlt(pSrc, pl, pd, pp, true, 1, nullptr, "arm_mat_ldlt_f32");
}
arm_status arm_mat_solve_lower_triangular_f32(const arm_matrix_instance_f32* lt, const arm_matrix_instance_f32* a,
                                              arm_matrix_instance_f32* dst) {
  return solve_tri(true, lt, a, dst, true, 1, nullptr, nullptr, "arm_mat_solve_lower_triangular_f32");
}
arm_status arm_mat_solve_upper_triangular_f32(const arm_matrix_instance_f32* ut, const arm_matrix_instance_f32* a,
                                              arm_matrix_instance_f32* dst) {
  return solve_tri(false, ut, a, dst, true, 1, nullptr, nullptr, "arm_mat_solve_upper_triangular_f32");
}

arm_status arm_mat_inverse_f32_batch(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pDst,
                                     uint32_t batch, int32_t* d_status, void* stream) {
  return solve_square(true, pSrc, pDst, false, batch, d_status, stream, "arm_mat_inverse_f32_batch");
}
arm_status arm_mat_cholesky_f32_batch(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pDst,
                                      uint32_t batch, int32_t* d_status, void* stream) {
  return solve_square(false, pSrc, pDst, false, batch, d_status, stream, "arm_mat_cholesky_f32_batch");
}
arm_status arm_mat_ldlt_f32_batch(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pl,
                                  arm_matrix_instance_f32* pd, uint16_t* d_pp, uint32_t batch, void* stream) {
  return solve_ldlt(pSrc, pl, pd, d_pp, false, batch, stream, "arm_mat_ldlt_f32_batch");
}
arm_status arm_mat_solve_lower_triangular_f32_batch(const arm_matrix_instance_f32* lt,
                                                    const arm_matrix_instance_f32* a, arm_matrix_instance_f32* dst,
                                                    uint32_t batch, int32_t* d_status, void* stream) {
  return solve_tri(true, lt, a, dst, false, batch, d_status, stream, "arm_mat_solve_lower_triangular_f32_batch");
}
arm_status arm_mat_solve_upper_triangular_f32_batch(const arm_matrix_instance_f32* ut,
                                                    const arm_matrix_instance_f32* a, arm_matrix_instance_f32* dst,
                                                    uint32_t batch, int32_t* d_status, void* stream) {
  return solve_tri(false, ut, a, dst, false, batch, d_status, stream, "arm_mat_solve_upper_triangular_f32_batch");
}
}  // extern "C"

// ---- add / sub / scale, transposes, matrix x vector (mat_basic.hip) ------------------------------
// matrix_functions.h groups MatrixAdd, MatrixSub, MatrixScale, MatrixTrans, MatrixComplexTrans and the
// arm_mat_vec_mult_* of MatrixMult.  The shape rules are the reference's ARM_MATH_MATRIX_CHECK ones, applied
// always.  No overlap rule (add / sub / scale work in place; a transpose onto its source is the caller's error).
namespace {
template <typename M>
bool same_shape(const M* a, const M* b) { return a->numRows == b->numRows && a->numCols == b->numCols; }

// op: kMatAdd / kMatSub (b != null) or kMatScale (b == null, scale and shift used).
template <typename T, typename M>
arm_status mat_ew(int op, const M* a, const M* b, M* d, T scale, int32_t shift, bool sync, uint32_t batch,
                  void* stream, const char* what) {
  const bool two = op != kMatScale;
  if (!a || (two && !b) || !d) return ARM_MATH_ARGUMENT_ERROR;
  const size_t n = (size_t)a->numRows * a->numCols, bytes = sizeof(T) * n * batch;
  const VecCall c{what, sync, stream, kMatrixCall, two ? 3 : 2,
                  {{a->pData, bytes, kIn}, {d->pData, bytes, kOut}, {two ? b->pData : nullptr, bytes, kIn}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (!same_shape(a, d) || (two && !same_shape(a, b))) return ARM_MATH_SIZE_MISMATCH;
  if (op == kMatScale && !std::is_same<T, float>::value) {
    // past these the reference shifts by a negative or too large count
    const int lo = sizeof(T) == 4 ? -1 : -16, hi = sizeof(T) == 4 ? 30 : 15;
    if (shift < lo || shift > hi) return ARM_MATH_ARGUMENT_ERROR;
  }
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return mat_ew_launch<T>(op, (const T*)p[0], (const T*)p[2], (T*)p[1], n * batch, scale, shift, st);
  });
}

// words: T words per element (2: interleaved complex).
template <typename T, typename M>
arm_status mat_trans(const M* s, M* d, int words, bool sync, uint32_t batch, void* stream, const char* what) {
  if (!s || !d) return ARM_MATH_ARGUMENT_ERROR;
  const size_t n = (size_t)s->numRows * s->numCols;
  const int eb = (int)sizeof(T) * words;
  const VecCall c{what, sync, stream, kMatrixCall, 2, {{s->pData, eb * n * batch, kIn}, {d->pData, eb * n * batch, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (s->numRows != d->numCols || s->numCols != d->numRows) return ARM_MATH_SIZE_MISMATCH;
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return mat_trans_launch(eb, s->numRows, s->numCols, p[0], p[1], batch, st);
  });
}

// matStride (elements; the drop-in passes 0): 0 shares one matrix, otherwise >= numRows * numCols.  The drop-in is
// void and reports a null operand through the last error.  numCols == 0: every sum is empty and the outputs are
// zero, as in the reference; no operand word is read.
template <typename T, typename M>
arm_status mat_vec_mult(const M* m, size_t matStride, const T* vec, T* dst, bool sync, uint32_t batch, void* stream,
                        const char* what) {
  if (!m) return refuse(sync, what);
  const size_t rows = m->numRows, cols = m->numCols;
  const VecCall c{what, sync, stream, kNoOverlapRule, 3,
                  {{m->pData, sizeof(T) * (matStride * (batch - 1) + rows * cols), kIn},
                   {vec, sizeof(T) * cols * batch, kIn}, {dst, sizeof(T) * rows * batch, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (matStride != 0 && matStride < rows * cols) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0 || rows == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return mat_vec_mult_launch<T>((int)rows, (int)cols, (const T*)p[0], matStride, (const T*)p[1], (T*)p[2], batch, st);
  });
}
}  // namespace

extern "C" {
#define MI355X_MAT_EW(SUF, INST, T, CT)                                                                          \
  arm_status arm_mat_add_##SUF(const INST* pSrcA, const INST* pSrcB, INST* pDst) {                               \
    return mat_ew<CT>(kMatAdd, pSrcA, pSrcB, pDst, (CT)0, 0, true, 1, nullptr, "arm_mat_add_" #SUF);             \
  }                                                                                                              \
  arm_status arm_mat_sub_##SUF(const INST* pSrcA, const INST* pSrcB, INST* pDst) {                               \
    return mat_ew<CT>(kMatSub, pSrcA, pSrcB, pDst, (CT)0, 0, true, 1, nullptr, "arm_mat_sub_" #SUF);             \
  }                                                                                                              \
  arm_status arm_mat_add_##SUF##_batch(const INST* pSrcA, const INST* pSrcB, INST* pDst, uint32_t batch,         \
                                       void* stream) {                                                           \
    return mat_ew<CT>(kMatAdd, pSrcA, pSrcB, pDst, (CT)0, 0, false, batch, stream, "arm_mat_add_" #SUF "_batch"); \
  }                                                                                                              \
  arm_status arm_mat_sub_##SUF##_batch(const INST* pSrcA, const INST* pSrcB, INST* pDst, uint32_t batch,         \
                                       void* stream) {                                                           \
    return mat_ew<CT>(kMatSub, pSrcA, pSrcB, pDst, (CT)0, 0, false, batch, stream, "arm_mat_sub_" #SUF "_batch"); \
  }
MI355X_MAT_EW(f32, arm_matrix_instance_f32, float32_t, float)
MI355X_MAT_EW(q31, arm_matrix_instance_q31, q31_t, int32_t)
MI355X_MAT_EW(q15, arm_matrix_instance_q15, q15_t, int16_t)
#undef MI355X_MAT_EW

arm_status arm_mat_scale_f32(const arm_matrix_instance_f32* pSrc, float32_t scale, arm_matrix_instance_f32* pDst) {
  return mat_ew<float>(kMatScale, pSrc, (const arm_matrix_instance_f32*)nullptr, pDst, scale, 0, true, 1, nullptr,
                       "arm_mat_scale_f32");
}
arm_status arm_mat_scale_f32_batch(const arm_matrix_instance_f32* pSrc, float32_t scale,
                                   arm_matrix_instance_f32* pDst, uint32_t batch, void* stream) {
  return mat_ew<float>(kMatScale, pSrc, (const arm_matrix_instance_f32*)nullptr, pDst, scale, 0, false, batch, stream,
                       "arm_mat_scale_f32_batch");
}
#define MI355X_MAT_SCALE(SUF, INST, T, CT)                                                                       \
  arm_status arm_mat_scale_##SUF(const INST* pSrc, T scaleFract, int32_t shift, INST* pDst) {                    \
    return mat_ew<CT>(kMatScale, pSrc, (const INST*)nullptr, pDst, scaleFract, shift, true, 1, nullptr,          \
                      "arm_mat_scale_" #SUF);                                                                    \
  }                                                                                                              \
  arm_status arm_mat_scale_##SUF##_batch(const INST* pSrc, T scaleFract, int32_t shift, INST* pDst,              \
                                         uint32_t batch, void* stream) {                                         \
    return mat_ew<CT>(kMatScale, pSrc, (const INST*)nullptr, pDst, scaleFract, shift, false, batch, stream,      \
                      "arm_mat_scale_" #SUF "_batch");                                                           \
  }
MI355X_MAT_SCALE(q31, arm_matrix_instance_q31, q31_t, int32_t)
MI355X_MAT_SCALE(q15, arm_matrix_instance_q15, q15_t, int16_t)
#undef MI355X_MAT_SCALE

// NAME: trans / cmplx_trans; WORDS: CT words per element
#define MI355X_MAT_TRANS(NAME, SUF, INST, CT, WORDS)                                                             \
  arm_status arm_mat_##NAME##_##SUF(const INST* pSrc, INST* pDst) {                                              \
    return mat_trans<CT>(pSrc, pDst, WORDS, true, 1, nullptr, "arm_mat_" #NAME "_" #SUF);                        \
  }                                                                                                              \
  arm_status arm_mat_##NAME##_##SUF##_batch(const INST* pSrc, INST* pDst, uint32_t batch, void* stream) {        \
    return mat_trans<CT>(pSrc, pDst, WORDS, false, batch, stream, "arm_mat_" #NAME "_" #SUF "_batch");           \
  }
MI355X_MAT_TRANS(trans, f32, arm_matrix_instance_f32, float, 1)
MI355X_MAT_TRANS(trans, q31, arm_matrix_instance_q31, int32_t, 1)
MI355X_MAT_TRANS(trans, q15, arm_matrix_instance_q15, int16_t, 1)
MI355X_MAT_TRANS(trans, q7, arm_matrix_instance_q7, int8_t, 1)
MI355X_MAT_TRANS(cmplx_trans, f32, arm_matrix_instance_f32, float, 2)
MI355X_MAT_TRANS(cmplx_trans, q31, arm_matrix_instance_q31, int32_t, 2)
MI355X_MAT_TRANS(cmplx_trans, q15, arm_matrix_instance_q15, int16_t, 2)
#undef MI355X_MAT_TRANS

#define MI355X_MAT_VEC(SUF, INST, T, CT)                                                                         \
  void arm_mat_vec_mult_##SUF(const INST* pSrcMat, const T* pVec, T* pDst) {                                     \
    mat_vec_mult<CT>(pSrcMat, 0, (const CT*)pVec, (CT*)pDst, true, 1, nullptr, "arm_mat_vec_mult_" #SUF);        \
  }                                                                                                              \
  arm_status arm_mat_vec_mult_##SUF##_batch(const INST* pSrcMat, uint32_t matStride, const T* d_vec, T* d_dst,   \
                                            uint32_t batch, void* stream) {                                      \
    return mat_vec_mult<CT>(pSrcMat, matStride, (const CT*)d_vec, (CT*)d_dst, false, batch, stream,              \
                            "arm_mat_vec_mult_" #SUF "_batch");                                                  \
  }
MI355X_MAT_VEC(f32, arm_matrix_instance_f32, float32_t, float)
MI355X_MAT_VEC(q31, arm_matrix_instance_q31, q31_t, int32_t)
MI355X_MAT_VEC(q15, arm_matrix_instance_q15, q15_t, int16_t)
MI355X_MAT_VEC(q7, arm_matrix_instance_q7, q7_t, int8_t)
#undef MI355X_MAT_VEC
}  // extern "C"

// ---- complex math, max / min (cmplx_math.hip) ---------------------------------------------------
// complex_math_functions.h and arm_max_* / arm_min_* of statistics_functions.h.  dst may be a source exactly where
// the kernel allows it (conj: the source; mult_cmplx: either source; mult_real: the complex source).
namespace {
template <typename T>
arm_status cmplx_ew(int op, const T* a, const T* b, T* d, uint32_t n, bool sync, uint32_t batch, void* stream,
                    const char* what) {
  const int wb = op == kCmMultCmplx ? 2 : op == kCmMultReal ? 1 : 0;
  const int wd = op == kCmMag || op == kCmMagSquared || op == kCmMagFast ? 1 : 2;
  const size_t count = (size_t)n * batch;
  const VecCall c{what, sync, stream, 0, wb ? 3 : 2,
                  {{a, sizeof(T) * 2 * count, wd == 2 ? kIn | kExactOk : kIn}, {d, sizeof(T) * wd * count, kOut},
                   {b, sizeof(T) * wb * count, op == kCmMultCmplx ? kIn | kExactOk : kIn}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  const bool lut = op == kCmMag && !std::is_same<T, float>::value;
  return c.run([&](void* const* p, hipStream_t st) -> hipError_t {
    const int32_t* dl = lut ? (const int32_t*)device_table(sqrt_initial_lut_q31, sizeof(int32_t) * 32) : nullptr;
    if (lut && !dl) return hipErrorOutOfMemory;
    return cmplx_ew_launch<T>(op, (const T*)p[0], (const T*)p[2], (T*)p[1], count, dl, st);
  });
}

template <typename T, typename R>
arm_status cmplx_dot(const T* a, const T* b, uint32_t bStride, uint32_t n, R* re, R* im, bool sync, uint32_t batch,
                     void* stream, const char* what) {
  return strided_reduce(2, a, b, bStride, n, re, im, sync, batch, stream, what,
                        [&](const T* da, const T* db, R* dre, R* dim, hipStream_t st) {
                          return cmplx_dot_launch<T, R>(da, db, bStride, n, dre, dim, batch, st);
                        });
}
}  // namespace

extern "C" {
// one source: mag, mag_squared, conj
#define MI355X_CMPLX_1(NAME, OP, SUF, T, CT)                                                                     \
  void arm_cmplx_##NAME##_##SUF(const T* pSrc, T* pDst, uint32_t numSamples) {                                   \
    cmplx_ew<CT>(OP, (const CT*)pSrc, (const CT*)nullptr, (CT*)pDst, numSamples, true, 1, nullptr,               \
                 "arm_cmplx_" #NAME "_" #SUF);                                                                   \
  }                                                                                                              \
  arm_status arm_cmplx_##NAME##_##SUF##_batch(const T* d_src, T* d_dst, uint32_t numSamples, uint32_t batch,     \
                                              void* stream) {                                                    \
    return cmplx_ew<CT>(OP, (const CT*)d_src, (const CT*)nullptr, (CT*)d_dst, numSamples, false, batch, stream,  \
                        "arm_cmplx_" #NAME "_" #SUF "_batch");                                                   \
  }
// two sources: mult_cmplx (pSrcB complex), mult_real (pSrcB real)
#define MI355X_CMPLX_2(NAME, OP, SUF, T, CT)                                                                     \
  void arm_cmplx_##NAME##_##SUF(const T* pSrcA, const T* pSrcB, T* pDst, uint32_t numSamples) {                  \
    cmplx_ew<CT>(OP, (const CT*)pSrcA, (const CT*)pSrcB, (CT*)pDst, numSamples, true, 1, nullptr,                \
                 "arm_cmplx_" #NAME "_" #SUF);                                                                   \
  }                                                                                                              \
  arm_status arm_cmplx_##NAME##_##SUF##_batch(const T* d_srcA, const T* d_srcB, T* d_dst, uint32_t numSamples,   \
                                              uint32_t batch, void* stream) {                                    \
    return cmplx_ew<CT>(OP, (const CT*)d_srcA, (const CT*)d_srcB, (CT*)d_dst, numSamples, false, batch, stream,  \
                        "arm_cmplx_" #NAME "_" #SUF "_batch");                                                   \
  }
#define MI355X_CMPLX_DOT(SUF, T, CT, R, CR)                                                                      \
  void arm_cmplx_dot_prod_##SUF(const T* pSrcA, const T* pSrcB, uint32_t numSamples, R* realResult,              \
                                R* imagResult) {                                                                 \
    cmplx_dot<CT, CR>((const CT*)pSrcA, (const CT*)pSrcB, numSamples, numSamples, (CR*)realResult,               \
                      (CR*)imagResult, true, 1, nullptr, "arm_cmplx_dot_prod_" #SUF);                            \
  }                                                                                                              \
  arm_status arm_cmplx_dot_prod_##SUF##_batch(const T* d_a, const T* d_b, uint32_t bStride, uint32_t numSamples, \
                                              R* d_re, R* d_im, uint32_t batch, void* stream) {                  \
    return cmplx_dot<CT, CR>((const CT*)d_a, (const CT*)d_b, bStride, numSamples, (CR*)d_re, (CR*)d_im, false,   \
                             batch, stream, "arm_cmplx_dot_prod_" #SUF "_batch");                                \
  }
#define MI355X_CMPLX_TYPE(SUF, T, CT, R, CR)                   \
  MI355X_CMPLX_1(mag, kCmMag, SUF, T, CT)                      \
  MI355X_CMPLX_1(mag_squared, kCmMagSquared, SUF, T, CT)       \
  MI355X_CMPLX_1(conj, kCmConj, SUF, T, CT)                    \
  MI355X_CMPLX_2(mult_cmplx, kCmMultCmplx, SUF, T, CT)         \
  MI355X_CMPLX_2(mult_real, kCmMultReal, SUF, T, CT)           \
  MI355X_CMPLX_DOT(SUF, T, CT, R, CR)
MI355X_CMPLX_TYPE(f32, float32_t, float, float32_t, float)
MI355X_CMPLX_TYPE(q31, q31_t, int32_t, q63_t, int64_t)
MI355X_CMPLX_TYPE(q15, q15_t, int16_t, q31_t, int32_t)
#undef MI355X_CMPLX_TYPE
#undef MI355X_CMPLX_DOT
#undef MI355X_CMPLX_2
#undef MI355X_CMPLX_1

// NAME: max, min, absmax, absmin, with the index
#define MI355X_SEARCH(NAME, MAX, ABS, SUF, T, CT)                                                                \
  void arm_##NAME##_##SUF(const T* pSrc, uint32_t blockSize, T* pResult, uint32_t* pIndex) {                     \
    search<CT>(MAX, ABS, true, (const CT*)pSrc, blockSize, (CT*)pResult, pIndex, true, 1, nullptr,               \
               "arm_" #NAME "_" #SUF);                                                                           \
  }                                                                                                              \
  arm_status arm_##NAME##_##SUF##_batch(const T* d_src, uint32_t blockSize, T* d_result, uint32_t* d_index,      \
                                        uint32_t batch, void* stream) {                                          \
    return search<CT>(MAX, ABS, true, (const CT*)d_src, blockSize, (CT*)d_result, d_index, false, batch, stream, \
                      "arm_" #NAME "_" #SUF "_batch");                                                           \
  }
// the same four without it
#define MI355X_SEARCH_NO_IDX(NAME, MAX, ABS, SUF, T, CT)                                                         \
  void arm_##NAME##_no_idx_##SUF(const T* pSrc, uint32_t blockSize, T* pResult) {                                \
    search<CT>(MAX, ABS, false, (const CT*)pSrc, blockSize, (CT*)pResult, nullptr, true, 1, nullptr,             \
               "arm_" #NAME "_no_idx_" #SUF);                                                                    \
  }                                                                                                              \
  arm_status arm_##NAME##_no_idx_##SUF##_batch(const T* d_src, uint32_t blockSize, T* d_result, uint32_t batch,  \
                                               void* stream) {                                                   \
    return search<CT>(MAX, ABS, false, (const CT*)d_src, blockSize, (CT*)d_result, nullptr, false, batch,        \
                      stream, "arm_" #NAME "_no_idx_" #SUF "_batch");                                            \
  }
#define MI355X_SEARCH_TYPE(SUF, T, CT)                    \
  MI355X_SEARCH(max, true, false, SUF, T, CT)             \
  MI355X_SEARCH(min, false, false, SUF, T, CT)            \
  MI355X_SEARCH(absmax, true, true, SUF, T, CT)           \
  MI355X_SEARCH(absmin, false, true, SUF, T, CT)          \
  MI355X_SEARCH_NO_IDX(max, true, false, SUF, T, CT)      \
  MI355X_SEARCH_NO_IDX(min, false, false, SUF, T, CT)     \
  MI355X_SEARCH_NO_IDX(absmax, true, true, SUF, T, CT)    \
  MI355X_SEARCH_NO_IDX(absmin, false, true, SUF, T, CT)
MI355X_SEARCH_TYPE(f32, float32_t, float)
MI355X_SEARCH_TYPE(q31, q31_t, int32_t)
MI355X_SEARCH_TYPE(q15, q15_t, int16_t)
MI355X_SEARCH_TYPE(q7, q7_t, int8_t)
#undef MI355X_SEARCH_TYPE
#undef MI355X_SEARCH_NO_IDX
#undef MI355X_SEARCH

// arm_cmplx_mag_fast_q15: one more operation of the element-wise kernel
void arm_cmplx_mag_fast_q15(const q15_t* pSrc, q15_t* pDst, uint32_t numSamples) {
  cmplx_ew<int16_t>(kCmMagFast, pSrc, (const int16_t*)nullptr, pDst, numSamples, true, 1, nullptr,
                    "arm_cmplx_mag_fast_q15");
}
arm_status arm_cmplx_mag_fast_q15_batch(const q15_t* d_src, q15_t* d_dst, uint32_t numSamples, uint32_t batch,
                                        void* stream) {
  return cmplx_ew<int16_t>(kCmMagFast, d_src, (const int16_t*)nullptr, d_dst, numSamples, false, batch, stream,
                           "arm_cmplx_mag_fast_q15_batch");
}
// the scalar of fast_math_functions.h, computed on the host
arm_status arm_sqrt_q15(q15_t in, q15_t* pOut) {
  if (!pOut) return ARM_MATH_ARGUMENT_ERROR;
  *pOut = sqrt_q15_host(in);
  return in >= 0 ? ARM_MATH_SUCCESS : ARM_MATH_ARGUMENT_ERROR;
}
}  // extern "C"

// ---- statistics (statistics.hip) ------------------------------------------------------------------
// The sums and level measures of statistics_functions.h (op: kStMean ... kStAccumulate; b: the second source of
// kStMse); the abs / no-index searches are stamped out with max / min above.  blockSize == 0: what the reference's
// empty sums give is stored (power, accumulate: 0; mean_f32, mse_f32: 0 / 0; rms_f32: +0.0; var, std: 0; max /
// min_no_idx_f32: their start value); where it would divide an integer by zero or read pSrc[0] the call is refused.
namespace {
template <typename T, typename R>
arm_status st_sum(int op, const T* a, const T* b, uint32_t n, R* result, bool sync, uint32_t batch, void* stream,
                  const char* what) {
  constexpr bool f32 = std::is_same<T, float>::value;
  const bool two = op == kStMse;
  const size_t sb = sizeof(T) * n * batch;
  const VecCall c{what, sync, stream, 0, two ? 3 : 2, {{a, sb, kIn}, {result, sizeof(R) * batch, kOut}, {b, sb, kIn}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  if (n == 0 && !f32 && (op == kStMean || op == kStRms || op == kStMse)) return refuse(sync, what);
  const bool lut = std::is_same<T, int32_t>::value && (op == kStRms || op == kStStd);
  return c.run([&](void* const* p, hipStream_t st) -> hipError_t {
    const int32_t* dl = lut ? (const int32_t*)device_table(sqrt_initial_lut_q31, sizeof(int32_t) * 32) : nullptr;
    if (lut && !dl) return hipErrorOutOfMemory;
    return stat_sum_launch<T, R>(op, (const T*)p[0], (const T*)p[2], n, (R*)p[1], batch, dl, st);
  });
}
}  // namespace

extern "C" {
#define MI355X_STAT_1(NAME, OP, SUF, T, CT, R, CR)                                                               \
  void arm_##NAME##_##SUF(const T* pSrc, uint32_t blockSize, R* pResult) {                                       \
    st_sum<CT, CR>(OP, (const CT*)pSrc, (const CT*)nullptr, blockSize, (CR*)pResult, true, 1, nullptr,           \
                   "arm_" #NAME "_" #SUF);                                                                       \
  }                                                                                                              \
  arm_status arm_##NAME##_##SUF##_batch(const T* d_src, uint32_t blockSize, R* d_result, uint32_t batch,         \
                                        void* stream) {                                                          \
    return st_sum<CT, CR>(OP, (const CT*)d_src, (const CT*)nullptr, blockSize, (CR*)d_result, false, batch,      \
                          stream, "arm_" #NAME "_" #SUF "_batch");                                               \
  }
#define MI355X_STAT_MSE(SUF, T, CT)                                                                              \
  void arm_mse_##SUF(const T* pSrcA, const T* pSrcB, uint32_t blockSize, T* pResult) {                           \
    st_sum<CT, CT>(kStMse, (const CT*)pSrcA, (const CT*)pSrcB, blockSize, (CT*)pResult, true, 1, nullptr,        \
                   "arm_mse_" #SUF);                                                                             \
  }                                                                                                              \
  arm_status arm_mse_##SUF##_batch(const T* d_a, const T* d_b, uint32_t blockSize, T* d_result, uint32_t batch,  \
                                   void* stream) {                                                               \
    return st_sum<CT, CT>(kStMse, (const CT*)d_a, (const CT*)d_b, blockSize, (CT*)d_result, false, batch,        \
                          stream, "arm_mse_" #SUF "_batch");                                                     \
  }
#define MI355X_STAT_LEVELS(SUF, T, CT)               \
  MI355X_STAT_1(rms, kStRms, SUF, T, CT, T, CT)      \
  MI355X_STAT_1(var, kStVar, SUF, T, CT, T, CT)      \
  MI355X_STAT_1(std, kStStd, SUF, T, CT, T, CT)
#define MI355X_STAT_TYPE(SUF, T, CT, PR, CPR)        \
  MI355X_STAT_1(mean, kStMean, SUF, T, CT, T, CT)    \
  MI355X_STAT_1(power, kStPower, SUF, T, CT, PR, CPR) \
  MI355X_STAT_MSE(SUF, T, CT)
MI355X_STAT_TYPE(f32, float32_t, float, float32_t, float)
MI355X_STAT_TYPE(q31, q31_t, int32_t, q63_t, int64_t)
MI355X_STAT_TYPE(q15, q15_t, int16_t, q63_t, int64_t)
MI355X_STAT_TYPE(q7, q7_t, int8_t, q31_t, int32_t)
MI355X_STAT_LEVELS(f32, float32_t, float)
MI355X_STAT_LEVELS(q31, q31_t, int32_t)
MI355X_STAT_LEVELS(q15, q15_t, int16_t)
MI355X_STAT_1(accumulate, kStAccumulate, f32, float32_t, float, float32_t, float)
#undef MI355X_STAT_TYPE
#undef MI355X_STAT_LEVELS
#undef MI355X_STAT_MSE
#undef MI355X_STAT_1
}  // extern "C"

// ---- basic math (basic_math.hip; the dot products: statistics.hip) ---------------------------------
// basic_math_functions.h.  dst may be a source exactly.  One scalar (offset, scale and shift, low and high) serves
// the whole call.  shift: the counts at which the reference's C is defined (a count below 32 either way on its
// promoted int operands): arm_shift_* -31 .. 31; arm_scale_q31 -32 .. 30 (kShift = shift + 1), _q15 -16 .. 15
// (kShift = 15 - shift in 0 .. 31), _q7 -24 .. 7 (kShift = 7 - shift); outside the call is refused.
namespace {
bool bm_two(int op) { return op == kBmAdd || op == kBmSub || op == kBmMult || op == kBmAnd || op == kBmOr || op == kBmXor; }

template <typename T>
arm_status bm_ew(int op, const T* a, const T* b, T* d, uint32_t n, T s0, T s1, int shift, bool sync, uint32_t batch,
                 void* stream, const char* what) {
  const bool two = bm_two(op);
  const size_t count = (size_t)n * batch, bytes = sizeof(T) * count;
  const VecCall c{what, sync, stream, 0, two ? 3 : 2,
                  {{a, bytes, kIn | kExactOk}, {d, bytes, kOut}, {b, bytes, kIn | kExactOk}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  int sh = 0;
  if (op == kBmShift) {
    if (shift < -31 || shift > 31) return refuse(sync, what);
    sh = shift;
  } else if (op == kBmScale && !std::is_same<T, float>::value) {
    const int lo = sizeof(T) == 4 ? -32 : sizeof(T) == 2 ? -16 : -24, hi = sizeof(T) == 4 ? 30 : sizeof(T) == 2 ? 15 : 7;
    if (shift < lo || shift > hi) return refuse(sync, what);
    sh = sizeof(T) == 4 ? shift + 1 : hi - shift;
  }
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return basic_ew_launch<T>(op, (const T*)p[0], (const T*)p[2], (T*)p[1], count, s0, s1, sh, st);
  });
}

template <typename T, typename R>
arm_status bm_dot(const T* a, const T* b, uint32_t bStride, uint32_t n, R* result, bool sync, uint32_t batch,
                  void* stream, const char* what) {
  return strided_reduce(1, a, b, bStride, n, result, (R*)nullptr, sync, batch, stream, what,
                        [&](const T* da, const T* db, R* dr, R*, hipStream_t st) {
                          return dot_prod_launch<T, R>(da, db, bStride, n, dr, batch, st);
                        });
}
}  // namespace

extern "C" {
#define MI355X_BM_2(NAME, OP, SUF, T, CT)                                                                        \
  void arm_##NAME##_##SUF(const T* pSrcA, const T* pSrcB, T* pDst, uint32_t blockSize) {                         \
    bm_ew<CT>(OP, (const CT*)pSrcA, (const CT*)pSrcB, (CT*)pDst, blockSize, (CT)0, (CT)0, 0, true, 1, nullptr,   \
              "arm_" #NAME "_" #SUF);                                                                            \
  }                                                                                                              \
  arm_status arm_##NAME##_##SUF##_batch(const T* d_srcA, const T* d_srcB, T* d_dst, uint32_t blockSize,          \
                                        uint32_t batch, void* stream) {                                          \
    return bm_ew<CT>(OP, (const CT*)d_srcA, (const CT*)d_srcB, (CT*)d_dst, blockSize, (CT)0, (CT)0, 0, false,    \
                     batch, stream, "arm_" #NAME "_" #SUF "_batch");                                             \
  }
#define MI355X_BM_1(NAME, OP, SUF, T, CT)                                                                        \
  void arm_##NAME##_##SUF(const T* pSrc, T* pDst, uint32_t blockSize) {                                          \
    bm_ew<CT>(OP, (const CT*)pSrc, (const CT*)nullptr, (CT*)pDst, blockSize, (CT)0, (CT)0, 0, true, 1, nullptr,  \
              "arm_" #NAME "_" #SUF);                                                                            \
  }                                                                                                              \
  arm_status arm_##NAME##_##SUF##_batch(const T* d_src, T* d_dst, uint32_t blockSize, uint32_t batch,            \
                                        void* stream) {                                                          \
    return bm_ew<CT>(OP, (const CT*)d_src, (const CT*)nullptr, (CT*)d_dst, blockSize, (CT)0, (CT)0, 0, false,    \
                     batch, stream, "arm_" #NAME "_" #SUF "_batch");                                             \
  }
#define MI355X_BM_OFFSET(NAME, OP, SUF, T, CT)                                                                   \
  void arm_##NAME##_##SUF(const T* pSrc, T value, T* pDst, uint32_t blockSize) {                                 \
    bm_ew<CT>(OP, (const CT*)pSrc, (const CT*)nullptr, (CT*)pDst, blockSize, (CT)value, (CT)0, 0, true, 1,       \
              nullptr, "arm_" #NAME "_" #SUF);                                                                   \
  }                                                                                                              \
  arm_status arm_##NAME##_##SUF##_batch(const T* d_src, T value, T* d_dst, uint32_t blockSize, uint32_t batch,   \
                                        void* stream) {                                                          \
    return bm_ew<CT>(OP, (const CT*)d_src, (const CT*)nullptr, (CT*)d_dst, blockSize, (CT)value, (CT)0, 0,       \
                     false, batch, stream, "arm_" #NAME "_" #SUF "_batch");                                      \
  }
#define MI355X_BM_SCALE(SUF, T, CT)                                                                              \
  void arm_scale_##SUF(const T* pSrc, T scaleFract, int8_t shift, T* pDst, uint32_t blockSize) {                 \
    bm_ew<CT>(kBmScale, (const CT*)pSrc, (const CT*)nullptr, (CT*)pDst, blockSize, (CT)scaleFract, (CT)0, shift, \
              true, 1, nullptr, "arm_scale_" #SUF);                                                              \
  }                                                                                                              \
  arm_status arm_scale_##SUF##_batch(const T* d_src, T scaleFract, int8_t shift, T* d_dst, uint32_t blockSize,   \
                                     uint32_t batch, void* stream) {                                             \
    return bm_ew<CT>(kBmScale, (const CT*)d_src, (const CT*)nullptr, (CT*)d_dst, blockSize, (CT)scaleFract,      \
                     (CT)0, shift, false, batch, stream, "arm_scale_" #SUF "_batch");                            \
  }
#define MI355X_BM_SHIFT(SUF, T, CT)                                                                              \
  void arm_shift_##SUF(const T* pSrc, int8_t shiftBits, T* pDst, uint32_t blockSize) {                           \
    bm_ew<CT>(kBmShift, (const CT*)pSrc, (const CT*)nullptr, (CT*)pDst, blockSize, (CT)0, (CT)0, shiftBits,      \
              true, 1, nullptr, "arm_shift_" #SUF);                                                              \
  }                                                                                                              \
  arm_status arm_shift_##SUF##_batch(const T* d_src, int8_t shiftBits, T* d_dst, uint32_t blockSize,             \
                                     uint32_t batch, void* stream) {                                             \
    return bm_ew<CT>(kBmShift, (const CT*)d_src, (const CT*)nullptr, (CT*)d_dst, blockSize, (CT)0, (CT)0,        \
                     shiftBits, false, batch, stream, "arm_shift_" #SUF "_batch");                               \
  }
#define MI355X_BM_CLIP(SUF, T, CT)                                                                               \
  void arm_clip_##SUF(const T* pSrc, T* pDst, T low, T high, uint32_t numSamples) {                              \
    bm_ew<CT>(kBmClip, (const CT*)pSrc, (const CT*)nullptr, (CT*)pDst, numSamples, (CT)low, (CT)high, 0, true,   \
              1, nullptr, "arm_clip_" #SUF);                                                                     \
  }                                                                                                              \
  arm_status arm_clip_##SUF##_batch(const T* d_src, T* d_dst, T low, T high, uint32_t numSamples,                \
                                    uint32_t batch, void* stream) {                                              \
    return bm_ew<CT>(kBmClip, (const CT*)d_src, (const CT*)nullptr, (CT*)d_dst, numSamples, (CT)low, (CT)high,   \
                     0, false, batch, stream, "arm_clip_" #SUF "_batch");                                        \
  }
#define MI355X_BM_DOT(SUF, T, CT, R, CR)                                                                         \
  void arm_dot_prod_##SUF(const T* pSrcA, const T* pSrcB, uint32_t blockSize, R* result) {                       \
    bm_dot<CT, CR>((const CT*)pSrcA, (const CT*)pSrcB, blockSize, blockSize, (CR*)result, true, 1, nullptr,      \
                   "arm_dot_prod_" #SUF);                                                                        \
  }                                                                                                              \
  arm_status arm_dot_prod_##SUF##_batch(const T* d_a, const T* d_b, uint32_t bStride, uint32_t blockSize,        \
                                        R* d_result, uint32_t batch, void* stream) {                             \
    return bm_dot<CT, CR>((const CT*)d_a, (const CT*)d_b, bStride, blockSize, (CR*)d_result, false, batch,       \
                          stream, "arm_dot_prod_" #SUF "_batch");                                                \
  }
#define MI355X_BM_TYPE(SUF, T, CT, R, CR)          \
  MI355X_BM_2(add, kBmAdd, SUF, T, CT)             \
  MI355X_BM_2(sub, kBmSub, SUF, T, CT)             \
  MI355X_BM_2(mult, kBmMult, SUF, T, CT)           \
  MI355X_BM_OFFSET(offset, kBmOffset, SUF, T, CT)  \
  MI355X_BM_CLIP(SUF, T, CT)                       \
  MI355X_BM_1(abs, kBmAbs, SUF, T, CT)             \
  MI355X_BM_1(negate, kBmNegate, SUF, T, CT)       \
  MI355X_BM_DOT(SUF, T, CT, R, CR)
#define MI355X_BM_BITS(SUF, T)                     \
  MI355X_BM_2(and, kBmAnd, SUF, T, T)              \
  MI355X_BM_2(or, kBmOr, SUF, T, T)                \
  MI355X_BM_2(xor, kBmXor, SUF, T, T)              \
  MI355X_BM_1(not, kBmNot, SUF, T, T)
MI355X_BM_TYPE(f32, float32_t, float, float32_t, float)
MI355X_BM_TYPE(q31, q31_t, int32_t, q63_t, int64_t)
MI355X_BM_TYPE(q15, q15_t, int16_t, q63_t, int64_t)
MI355X_BM_TYPE(q7, q7_t, int8_t, q31_t, int32_t)
MI355X_BM_OFFSET(scale, kBmScale, f32, float32_t, float)
MI355X_BM_SCALE(q31, q31_t, int32_t)
MI355X_BM_SCALE(q15, q15_t, int16_t)
MI355X_BM_SCALE(q7, q7_t, int8_t)
MI355X_BM_SHIFT(q31, q31_t, int32_t)
MI355X_BM_SHIFT(q15, q15_t, int16_t)
MI355X_BM_SHIFT(q7, q7_t, int8_t)
MI355X_BM_BITS(u32, uint32_t)
MI355X_BM_BITS(u16, uint16_t)
MI355X_BM_BITS(u8, uint8_t)
#undef MI355X_BM_BITS
#undef MI355X_BM_TYPE
#undef MI355X_BM_DOT
#undef MI355X_BM_CLIP
#undef MI355X_BM_SHIFT
#undef MI355X_BM_SCALE
#undef MI355X_BM_OFFSET
#undef MI355X_BM_1
#undef MI355X_BM_2
}  // extern "C"

// ---- support functions (support.hip, sort.hip; the weighted average: statistics.hip) --------------
// support_functions.h.  dst may be src exactly where both element widths are equal (float_to_q31, q31_to_float,
// copy) and in the sorts.
namespace {
template <typename S, typename D>
arm_status sp_convert(const S* s, D* d, uint32_t n, bool sync, uint32_t batch, void* stream, const char* what) {
  const size_t count = (size_t)n * batch;
  const VecCall c{what, sync, stream, 0, 2,
                  {{s, sizeof(S) * count, sizeof(S) == sizeof(D) ? kIn | kExactOk : kIn}, {d, sizeof(D) * count, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return support_convert_launch<S, D>((const S*)p[0], (D*)p[1], count, st);
  });
}

template <typename T>
arm_status sp_fill(T value, T* d, uint32_t n, bool sync, uint32_t batch, void* stream, const char* what) {
  const size_t count = (size_t)n * batch;
  const VecCall c{what, sync, stream, 0, 1, {{d, sizeof(T) * count, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) { return support_fill_launch<T>(value, (T*)p[0], count, st); });
}

// dir: ARM_SORT_DESCENDING (0) or ARM_SORT_ASCENDING (1), anything else is refused.
arm_status sp_sort(int dir, const float* src, float* dst, uint32_t n, bool sync, uint32_t batch, void* stream,
                   const char* what) {
  const size_t bytes = sizeof(float) * n * batch;
  const VecCall c{what, sync, stream, 0, 2, {{src, bytes, kIn | kExactOk}, {dst, bytes, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if ((dir != 0 && dir != 1) || n > 0x80000000u) return refuse(sync, what);
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return sort_launch((const uint32_t*)p[0], (uint32_t*)p[1], n, dir == 1, batch, st);
  });
}

arm_status sp_wavg(const float* a, const float* w, uint32_t wStride, uint32_t n, float* result, bool sync,
                   uint32_t batch, void* stream, const char* what) {
  return strided_reduce(1, a, w, wStride, n, result, (float*)nullptr, sync, batch, stream, what,
                        [&](const float* da, const float* dw, float* dr, float*, hipStream_t st) {
                          return weighted_average_launch(da, dw, wStride, n, dr, batch, st);
                        });
}

// wStride (words; the drop-in passes nbVectors): 0 shares one weight vector, otherwise >= nbVectors.  vecDim == 0
// writes nothing; nbVectors == 0 stores 0 / 0.
arm_status sp_barycenter(const float* in, const float* w, uint32_t wStride, float* out, uint32_t nv, uint32_t dim,
                         bool sync, uint32_t batch, void* stream, const char* what) {
  const VecCall c{what, sync, stream, 0, 3,
                  {{in, sizeof(float) * nv * dim * batch, kIn},
                   {w, sizeof(float) * ((size_t)wStride * (batch - 1) + nv), kIn},
                   {out, sizeof(float) * dim * batch, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (wStride != 0 && wStride < nv) return refuse(sync, what);
  if (batch == 0 || dim == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return barycenter_launch((const float*)p[0], (const float*)p[1], wStride, (float*)p[2], nv, dim, batch, st);
  });
}
}  // namespace

extern "C" {
#define MI355X_SP_TO(SN, ST, SCT, DN, DT, DCT)                                                                   \
  void arm_##SN##_to_##DN(const ST* pSrc, DT* pDst, uint32_t blockSize) {                                        \
    sp_convert<SCT, DCT>((const SCT*)pSrc, (DCT*)pDst, blockSize, true, 1, nullptr, "arm_" #SN "_to_" #DN);      \
  }                                                                                                              \
  arm_status arm_##SN##_to_##DN##_batch(const ST* d_src, DT* d_dst, uint32_t blockSize, uint32_t batch,          \
                                        void* stream) {                                                          \
    return sp_convert<SCT, DCT>((const SCT*)d_src, (DCT*)d_dst, blockSize, false, batch, stream,                 \
                                "arm_" #SN "_to_" #DN "_batch");                                                 \
  }
#define MI355X_SP_COPY(SUF, T, CT)                                                                               \
  void arm_copy_##SUF(const T* pSrc, T* pDst, uint32_t blockSize) {                                              \
    sp_convert<CT, CT>((const CT*)pSrc, (CT*)pDst, blockSize, true, 1, nullptr, "arm_copy_" #SUF);               \
  }                                                                                                              \
  arm_status arm_copy_##SUF##_batch(const T* d_src, T* d_dst, uint32_t blockSize, uint32_t batch, void* stream) { \
    return sp_convert<CT, CT>((const CT*)d_src, (CT*)d_dst, blockSize, false, batch, stream,                     \
                              "arm_copy_" #SUF "_batch");                                                        \
  }                                                                                                              \
  void arm_fill_##SUF(T value, T* pDst, uint32_t blockSize) {                                                    \
    sp_fill<CT>((CT)value, (CT*)pDst, blockSize, true, 1, nullptr, "arm_fill_" #SUF);                            \
  }                                                                                                              \
  arm_status arm_fill_##SUF##_batch(T value, T* d_dst, uint32_t blockSize, uint32_t batch, void* stream) {       \
    return sp_fill<CT>((CT)value, (CT*)d_dst, blockSize, false, batch, stream, "arm_fill_" #SUF "_batch");       \
  }
MI355X_SP_TO(float, float32_t, float, q31, q31_t, int32_t)
MI355X_SP_TO(float, float32_t, float, q15, q15_t, int16_t)
MI355X_SP_TO(float, float32_t, float, q7, q7_t, int8_t)
MI355X_SP_TO(q31, q31_t, int32_t, float, float32_t, float)
MI355X_SP_TO(q31, q31_t, int32_t, q15, q15_t, int16_t)
MI355X_SP_TO(q31, q31_t, int32_t, q7, q7_t, int8_t)
MI355X_SP_TO(q15, q15_t, int16_t, float, float32_t, float)
MI355X_SP_TO(q15, q15_t, int16_t, q31, q31_t, int32_t)
MI355X_SP_TO(q15, q15_t, int16_t, q7, q7_t, int8_t)
MI355X_SP_TO(q7, q7_t, int8_t, float, float32_t, float)
MI355X_SP_TO(q7, q7_t, int8_t, q31, q31_t, int32_t)
MI355X_SP_TO(q7, q7_t, int8_t, q15, q15_t, int16_t)
MI355X_SP_COPY(f32, float32_t, float)
MI355X_SP_COPY(q31, q31_t, int32_t)
MI355X_SP_COPY(q15, q15_t, int16_t)
MI355X_SP_COPY(q7, q7_t, int8_t)
#undef MI355X_SP_COPY
#undef MI355X_SP_TO

// S->alg selects among equal results: a value of arm_sort_alg sorts, any other is the no-op of the reference's switch.
void arm_sort_f32(const arm_sort_instance_f32* S, float32_t* pSrc, float32_t* pDst, uint32_t blockSize) {
  if (!S) { refuse(true, "arm_sort_f32"); return; }
  if ((int)S->alg < (int)ARM_SORT_BITONIC || (int)S->alg > (int)ARM_SORT_SELECTION) return;
  sp_sort((int)S->dir, pSrc, pDst, blockSize, true, 1, nullptr, "arm_sort_f32");
}
// S->buffer is neither read nor written.
void arm_merge_sort_f32(const arm_merge_sort_instance_f32* S, float32_t* pSrc, float32_t* pDst, uint32_t blockSize) {
  if (!S) { refuse(true, "arm_merge_sort_f32"); return; }
  sp_sort((int)S->dir, pSrc, pDst, blockSize, true, 1, nullptr, "arm_merge_sort_f32");
}
arm_status arm_sort_f32_batch(const float32_t* d_src, float32_t* d_dst, uint32_t blockSize, arm_sort_dir dir,
                              uint32_t batch, void* stream) {
  return sp_sort((int)dir, d_src, d_dst, blockSize, false, batch, stream, "arm_sort_f32_batch");
}
arm_status arm_merge_sort_f32_batch(const float32_t* d_src, float32_t* d_dst, uint32_t blockSize, arm_sort_dir dir,
                                    uint32_t batch, void* stream) {
  return sp_sort((int)dir, d_src, d_dst, blockSize, false, batch, stream, "arm_merge_sort_f32_batch");
}
float32_t arm_weighted_average_f32(const float32_t* in, const float32_t* weights, uint32_t blockSize) {
  float32_t r = 0.0f;
  if (sp_wavg(in, weights, blockSize, blockSize, &r, true, 1, nullptr, "arm_weighted_average_f32") !=
      ARM_MATH_SUCCESS)
    return __builtin_nanf("");
  return r;
}
arm_status arm_weighted_average_f32_batch(const float32_t* d_in, const float32_t* d_weights, uint32_t wStride,
                                          uint32_t blockSize, float32_t* d_result, uint32_t batch, void* stream) {
  return sp_wavg(d_in, d_weights, wStride, blockSize, d_result, false, batch, stream,
                 "arm_weighted_average_f32_batch");
}
void arm_barycenter_f32(const float32_t* in, const float32_t* weights, float32_t* out, uint32_t nbVectors,
                        uint32_t vecDim) {
  sp_barycenter(in, weights, nbVectors, out, nbVectors, vecDim, true, 1, nullptr, "arm_barycenter_f32");
}
arm_status arm_barycenter_f32_batch(const float32_t* d_in, const float32_t* d_weights, uint32_t wStride,
                                    float32_t* d_out, uint32_t nbVectors, uint32_t vecDim, uint32_t batch,
                                    void* stream) {
  return sp_barycenter(d_in, d_weights, wStride, d_out, nbVectors, vecDim, false, batch, stream,
                       "arm_barycenter_f32_batch");
}
}  // extern "C"

// ---- distance functions (distance.hip) ------------------------------------------------------------
// distance_functions.h.  The two-source reductions go through strided_reduce (bStride in words, 0: one B vector for
// every item).  blockSize == 0 stores what the reference's arithmetic gives on empty sums, except chebyshev, which
// would read element 0 and is refused.  A drop-in returns its float; a failure returns a NaN with the last error set.
namespace {
arm_status ds_f32(int op, const float* a, const float* b, uint32_t bStride, uint32_t n, float* result, bool sync,
                  uint32_t batch, void* stream, const char* what) {
  if (op == kDsChebyshev && n == 0) return refuse(sync, what);
  return strided_reduce(1, a, b, bStride, n, result, (float*)nullptr, sync, batch, stream, what,
                        [&](const float* da, const float* db, float* dr, float*, hipStream_t st) {
                          return distance_f32_launch(op, da, db, bStride, n, dr, batch, nullptr, nullptr, st);
                        });
}

// The drop-in of the correlation distance: pA and pB are results as well (the shifted words).
arm_status ds_correlation_sync(float* a, float* b, uint32_t n, float* result, const char* what) {
  const size_t sb = sizeof(float) * n;
  const VecCall c{what, true, nullptr, 0, 3, {{a, sb, kIn | kOut}, {b, sb, kIn | kOut}, {result, sizeof(float), kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  return c.run([&](void* const* p, hipStream_t st) {
    return distance_f32_launch(kDsCorrelation, (const float*)p[0], (const float*)p[1], n, n, (float*)p[2], 1,
                               (float*)p[0], (float*)p[1], st);
  });
}

arm_status ds_bool(int op, const uint32_t* a, const uint32_t* b, uint32_t bStride, uint32_t nbools, float* result,
                   bool sync, uint32_t batch, void* stream, const char* what) {
  const uint32_t words = (uint32_t)(((uint64_t)nbools + 31) / 32);
  return strided_reduce(1, a, b, bStride, words, result, (float*)nullptr, sync, batch, stream, what,
                        [&](const uint32_t* da, const uint32_t* db, float* dr, float*, hipStream_t st) {
                          return boolean_distance_launch(op, da, db, bStride, nbools, dr, batch, st);
                        });
}

bool dtw_length_ok(uint32_t q, uint32_t t) { return q >= 1 && t >= 1 && q <= 32768 && t <= 32768; }

arm_status ds_dtw_window(int type, int32_t size, int8_t* w, uint32_t q, uint32_t t, bool sync, uint32_t batch,
                         void* stream, const char* what) {
  const VecCall c{what, sync, stream, 0, 1, {{w, (size_t)q * t * batch, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if ((type != ARM_DTW_SAKOE_CHIBA_WINDOW && type != ARM_DTW_SLANTED_BAND_WINDOW) || q > 32768 || t > 32768)
    return ARM_MATH_ARGUMENT_ERROR;                         // the reference's default: a status, no last error
  if (batch == 0 || q == 0 || t == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return dtw_init_window_launch(type, size, (int8_t*)p[0], q, t, batch, st);
  });
}

// result is staged in as well: an item without a path leaves its word alone.
arm_status ds_dtw_distance(const float* dist, const int8_t* window, uint32_t wStride, float* dtw, uint32_t q,
                           uint32_t t, float* result, int32_t* d_status, bool sync, uint32_t batch, void* stream,
                           const char* what) {
  const size_t cells = (size_t)q * t;
  VecCall c{what, sync, stream, 0, window ? 4 : 3,
            {{dist, sizeof(float) * cells * batch, kIn}, {dtw, sizeof(float) * cells * batch, kOut},
             {result, sizeof(float) * batch, kIn | kOut}, {window, (size_t)wStride * (batch - 1) + cells, kIn}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (!dtw_length_ok(q, t) || (window && wStride != 0 && wStride < cells)) return refuse(sync, what);
  if (batch == 0) return ARM_MATH_SUCCESS;
  return c.run_with_status(d_status, [&](void* const* p, int32_t* ds, hipStream_t st) {
    // without a window operand 3 is the drop-in's status word
    return dtw_distance_launch((const float*)p[0], window ? (const int8_t*)p[3] : nullptr, wStride, (float*)p[1], q, t,
                               (float*)p[2], ds, batch, st);
  });
}

arm_status ds_dtw_path(const float* dtw, uint32_t q, uint32_t t, int16_t* path, uint32_t* len, bool sync,
                       uint32_t batch, void* stream, const char* what) {
  const VecCall c{what, sync, stream, 0, 3,
                  {{dtw, sizeof(float) * q * t * batch, kIn},
                   {path, sizeof(int16_t) * 2 * ((size_t)q + t) * batch, kIn | kOut},
                   {len, sizeof(uint32_t) * batch, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (!dtw_length_ok(q, t)) return refuse(sync, what);
  if (batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return dtw_path_launch((const float*)p[0], q, t, (int16_t*)p[1], (uint32_t*)p[2], batch, st);
  });
}

template <typename M>
bool same_dims(const M* m, uint32_t q, uint32_t t) { return m->numRows == q && m->numCols == t; }
}  // namespace

extern "C" {
#define MI355X_DS_F32(NAME, OP)                                                                                  \
  float32_t arm_##NAME##_distance_f32(const float32_t* pA, const float32_t* pB, uint32_t blockSize) {            \
    float32_t r = 0.0f;                                                                                          \
    if (ds_f32(OP, pA, pB, blockSize, blockSize, &r, true, 1, nullptr, "arm_" #NAME "_distance_f32") !=          \
        ARM_MATH_SUCCESS)                                                                                        \
      return __builtin_nanf("");                                                                                 \
    return r;                                                                                                    \
  }
#define MI355X_DS_F32_BATCH(NAME, OP)                                                                            \
  arm_status arm_##NAME##_distance_f32_batch(const float32_t* d_a, const float32_t* d_b, uint32_t bStride,       \
                                             uint32_t blockSize, float32_t* d_result, uint32_t batch,            \
                                             void* stream) {                                                     \
    return ds_f32(OP, d_a, d_b, bStride, blockSize, d_result, false, batch, stream,                              \
                  "arm_" #NAME "_distance_f32_batch");                                                           \
  }
#define MI355X_DS_BOOL(NAME, OP)                                                                                 \
  float32_t arm_##NAME##_distance(const uint32_t* pA, const uint32_t* pB, uint32_t numberOfBools) {              \
    float32_t r = 0.0f;                                                                                          \
    const uint32_t words = (uint32_t)(((uint64_t)numberOfBools + 31) / 32);                                      \
    if (ds_bool(OP, pA, pB, words, numberOfBools, &r, true, 1, nullptr, "arm_" #NAME "_distance") !=             \
        ARM_MATH_SUCCESS)                                                                                        \
      return __builtin_nanf("");                                                                                 \
    return r;                                                                                                    \
  }                                                                                                              \
  arm_status arm_##NAME##_distance_batch(const uint32_t* d_a, const uint32_t* d_b, uint32_t bStride,             \
                                         uint32_t numberOfBools, float32_t* d_result, uint32_t batch,            \
                                         void* stream) {                                                         \
    return ds_bool(OP, d_a, d_b, bStride, numberOfBools, d_result, false, batch, stream,                         \
                   "arm_" #NAME "_distance_batch");                                                              \
  }
MI355X_DS_F32(braycurtis, kDsBraycurtis)
MI355X_DS_F32(canberra, kDsCanberra)
MI355X_DS_F32(chebyshev, kDsChebyshev)
MI355X_DS_F32(cityblock, kDsCityblock)
MI355X_DS_F32(cosine, kDsCosine)
MI355X_DS_F32(euclidean, kDsEuclidean)
MI355X_DS_F32(jensenshannon, kDsJensenshannon)
MI355X_DS_F32_BATCH(braycurtis, kDsBraycurtis)
MI355X_DS_F32_BATCH(canberra, kDsCanberra)
MI355X_DS_F32_BATCH(chebyshev, kDsChebyshev)
MI355X_DS_F32_BATCH(cityblock, kDsCityblock)
MI355X_DS_F32_BATCH(correlation, kDsCorrelation)
MI355X_DS_F32_BATCH(cosine, kDsCosine)
MI355X_DS_F32_BATCH(euclidean, kDsEuclidean)
MI355X_DS_F32_BATCH(jensenshannon, kDsJensenshannon)
MI355X_DS_BOOL(dice, kBdDice)
MI355X_DS_BOOL(hamming, kBdHamming)
MI355X_DS_BOOL(jaccard, kBdJaccard)
MI355X_DS_BOOL(kulsinski, kBdKulsinski)
MI355X_DS_BOOL(rogerstanimoto, kBdRogerstanimoto)
MI355X_DS_BOOL(russellrao, kBdRussellrao)
MI355X_DS_BOOL(sokalmichener, kBdSokalmichener)
MI355X_DS_BOOL(sokalsneath, kBdSokalsneath)
MI355X_DS_BOOL(yule, kBdYule)
#undef MI355X_DS_BOOL
#undef MI355X_DS_F32_BATCH
#undef MI355X_DS_F32

float32_t arm_correlation_distance_f32(float32_t* pA, float32_t* pB, uint32_t blockSize) {
  float32_t r = 0.0f;
  if (ds_correlation_sync(pA, pB, blockSize, &r, "arm_correlation_distance_f32") != ARM_MATH_SUCCESS)
    return __builtin_nanf("");
  return r;
}

arm_status arm_dtw_init_window_q7(const arm_dtw_window windowType, const int32_t windowSize,
                                  arm_matrix_instance_q7* pWindow) {
  if (!pWindow) return ARM_MATH_ARGUMENT_ERROR;
  return ds_dtw_window((int)windowType, windowSize, pWindow->pData, pWindow->numRows, pWindow->numCols, true, 1,
                       nullptr, "arm_dtw_init_window_q7");
}
arm_status arm_dtw_init_window_q7_batch(arm_dtw_window windowType, int32_t windowSize, q7_t* d_window,
                                        uint32_t queryLength, uint32_t templateLength, uint32_t batch, void* stream) {
  return ds_dtw_window((int)windowType, windowSize, d_window, queryLength, templateLength, false, batch, stream,
                       "arm_dtw_init_window_q7_batch");
}
arm_status arm_dtw_distance_f32(const arm_matrix_instance_f32* pDistance, const arm_matrix_instance_q7* pWindow,
                                arm_matrix_instance_f32* pDTW, float32_t* distance) {
  if (!pDistance || !pDTW) return ARM_MATH_ARGUMENT_ERROR;
  const uint32_t q = pDistance->numRows, t = pDistance->numCols;
  if (!same_dims(pDTW, q, t) || (pWindow && !same_dims(pWindow, q, t))) return ARM_MATH_SIZE_MISMATCH;
  if (pWindow && !pWindow->pData) return refuse(true, "arm_dtw_distance_f32");
  return ds_dtw_distance(pDistance->pData, pWindow ? pWindow->pData : nullptr, 0, pDTW->pData, q, t, distance, nullptr,
                         true, 1, nullptr, "arm_dtw_distance_f32");
}
arm_status arm_dtw_distance_f32_batch(const float32_t* d_distance, const q7_t* d_window, uint32_t wStride,
                                      float32_t* d_dtw, uint32_t queryLength, uint32_t templateLength,
                                      float32_t* d_result, int32_t* d_status, uint32_t batch, void* stream) {
  return ds_dtw_distance(d_distance, d_window, wStride, d_dtw, queryLength, templateLength, d_result, d_status, false,
                         batch, stream, "arm_dtw_distance_f32_batch");
}
// *pathLength goes through a local word, so a refusal can clear it and an empty path can be reported.
void arm_dtw_path_f32(const arm_matrix_instance_f32* pDTW, int16_t* pPath, uint32_t* pathLength) {
  const char* what = "arm_dtw_path_f32";
  if (!pDTW || !pathLength) { refuse(true, what); return; }
  uint32_t len = 0;
  const arm_status r = ds_dtw_path(pDTW->pData, pDTW->numRows, pDTW->numCols, pPath, &len, true, 1, nullptr, what);
  if (r == ARM_MATH_SUCCESS && len == 0) set_error(hipErrorInvalidValue, what);   // the reference would not return
  if (is_device_ptr(pathLength)) {
    if (hipMemcpy(pathLength, &len, sizeof(len), hipMemcpyHostToDevice) != hipSuccess) set_error(hipErrorInvalidValue, what);
  } else {
    *pathLength = len;
  }
}
arm_status arm_dtw_path_f32_batch(const float32_t* d_dtw, uint32_t queryLength, uint32_t templateLength,
                                  int16_t* d_path, uint32_t* d_pathLength, uint32_t batch, void* stream) {
  return ds_dtw_path(d_dtw, queryLength, templateLength, d_path, d_pathLength, false, batch, stream,
                     "arm_dtw_path_f32_batch");
}
}  // extern "C"

// ---- vexp / vlog, log-domain statistics, SVM, naive Bayes (ml.hip) ------------------------------------
// fast_math_functions.h (arm_vexp_f32, arm_vlog_f32), statistics_functions.h (entropy, kullback_leibler, logsumexp,
// logsumexp_dot_prod), svm_functions.h and bayes_functions.h.  The two logsumexp forms read element 0 and refuse
// blockSize == 0; entropy and kullback_leibler return the -0.0f of their empty sums.  A drop-in that returns a float
// returns a NaN on a failure, arm_gaussian_naive_bayes_predict_f32 returns UINT32_MAX; both set the last error.
namespace {
arm_status ml_ew(int op, const float* src, float* dst, uint32_t n, bool sync, uint32_t batch, void* stream,
                 const char* what) {
  const size_t count = (size_t)n * batch, bytes = sizeof(float) * count;
  const VecCall c{what, sync, stream, 0, 2, {{src, bytes, kIn | kExactOk}, {dst, bytes, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (count == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return fast_math_launch(op, (const float*)p[0], (float*)p[1], count, st);
  });
}

// entropy and logsumexp: one source
arm_status ml_logdom_1(int op, const float* a, uint32_t n, float* result, bool sync, uint32_t batch, void* stream,
                       const char* what) {
  const VecCall c{what, sync, stream, 0, 2, {{a, sizeof(float) * n * batch, kIn}, {result, sizeof(float) * batch, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (op == kLdLogsumexp && n == 0) return refuse(sync, what);
  if (batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return logdom_launch(op, (const float*)p[0], nullptr, 0, n, (float*)p[1], batch, nullptr, st);
  });
}

// kullback_leibler and the batched logsumexp_dot_prod: two sources, the second at a stride
arm_status ml_logdom_2(int op, const float* a, const float* b, uint32_t bStride, uint32_t n, float* result, bool sync,
                       uint32_t batch, void* stream, const char* what) {
  if (op == kLdLogsumexpDot && n == 0) return refuse(sync, what);
  return strided_reduce(1, a, b, bStride, n, result, (float*)nullptr, sync, batch, stream, what,
                        [&](const float* da, const float* db, float* dr, float*, hipStream_t st) {
                          return logdom_launch(op, da, db, bStride, n, dr, batch, nullptr, st);
                        });
}

// The drop-in of logsumexp_dot_prod: pTmpBuffer receives a + b.
arm_status ml_logsumexp_dot_sync(const float* a, const float* b, uint32_t n, float* tmp, float* result,
                                 const char* what) {
  const size_t sb = sizeof(float) * n;
  const VecCall c{what, true, nullptr, 0, 4, {{a, sb, kIn}, {b, sb, kIn}, {tmp, sb, kOut}, {result, sizeof(float), kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (n == 0) return refuse(true, what);
  return c.run([&](void* const* p, hipStream_t st) {
    return logdom_launch(kLdLogsumexpDot, (const float*)p[0], (const float*)p[1], n, n, (float*)p[3], 1, (float*)p[2], st);
  });
}

// m's arrays are host or device pointers in a drop-in and device pointers in a batched call.  decision may be null.
arm_status ml_svm(int kind, SvmModel m, const float* in, int32_t* result, float* decision, bool sync, uint32_t items,
                  void* stream, const char* what) {
  const size_t nsv = m.nsv, dim = m.dim;
  const VecCall c{what, sync, stream, 0, decision ? 6 : 5,
                  {{m.dual, sizeof(float) * nsv, kIn}, {m.sv, sizeof(float) * nsv * dim, kIn},
                   {m.classes, 2 * sizeof(int32_t), kIn}, {in, sizeof(float) * dim * items, kIn},
                   {result, sizeof(int32_t) * items, kOut}, {decision, sizeof(float) * items, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (nsv * dim > 0xffffffffull) return refuse(sync, what);
  if (items == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    m.dual = (const float*)p[0];
    m.sv = (const float*)p[1];
    m.classes = (const int32_t*)p[2];
    return svm_predict_launch(kind, m, (const float*)p[3], (int32_t*)p[4], (float*)p[5], items, st);
  });
}

arm_status ml_bayes(const arm_gaussian_naive_bayes_instance_f32* S, const float* in, float* prob, uint32_t* cls,
                    bool sync, uint32_t items, void* stream, const char* what) {
  if (!S) return refuse(sync, what);
  const size_t C = S->numberOfClasses, D = S->vectorDimension;
  BayesModel m{S->vectorDimension, S->numberOfClasses, S->theta, S->sigma, S->classPriors, S->epsilon};
  const VecCall c{what, sync, stream, 0, 6,
                  {{m.theta, sizeof(float) * C * D, kIn}, {m.sigma, sizeof(float) * C * D, kIn},
                   {m.priors, sizeof(float) * C, kIn}, {in, sizeof(float) * D * items, kIn},
                   {prob, sizeof(float) * C * items, kOut}, {cls, sizeof(uint32_t) * items, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (C == 0 || C * D > 0xffffffffull) return refuse(sync, what);
  if (items == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    m.theta = (const float*)p[0];
    m.sigma = (const float*)p[1];
    m.priors = (const float*)p[2];
    return bayes_predict_launch(m, (const float*)p[3], (float*)p[4], (uint32_t*)p[5], items, st);
  });
}

SvmModel svm_model(const arm_svm_linear_instance_f32* S) {
  return {S->nbOfSupportVectors, S->vectorDimension, S->intercept, S->dualCoefficients, S->supportVectors, S->classes,
          0, 0.0f, 0.0f};
}
SvmModel svm_model(const arm_svm_polynomial_instance_f32* S) {
  return {S->nbOfSupportVectors, S->vectorDimension, S->intercept, S->dualCoefficients, S->supportVectors, S->classes,
          S->degree, S->coef0, S->gamma};
}
SvmModel svm_model(const arm_svm_rbf_instance_f32* S) {
  return {S->nbOfSupportVectors, S->vectorDimension, S->intercept, S->dualCoefficients, S->supportVectors, S->classes,
          0, 0.0f, S->gamma};
}
}  // namespace

extern "C" {
#define MI355X_ML_EW(NAME, OP)                                                                                   \
  void arm_##NAME##_f32(const float32_t* pSrc, float32_t* pDst, uint32_t blockSize) {                            \
    ml_ew(OP, pSrc, pDst, blockSize, true, 1, nullptr, "arm_" #NAME "_f32");                                     \
  }                                                                                                              \
  arm_status arm_##NAME##_f32_batch(const float32_t* d_src, float32_t* d_dst, uint32_t blockSize, uint32_t batch, \
                                    void* stream) {                                                              \
    return ml_ew(OP, d_src, d_dst, blockSize, false, batch, stream, "arm_" #NAME "_f32_batch");                  \
  }
MI355X_ML_EW(vexp, kFmExp)
MI355X_ML_EW(vlog, kFmLog)
#undef MI355X_ML_EW

float32_t arm_entropy_f32(const float32_t* pSrcA, uint32_t blockSize) {
  float32_t r = 0.0f;
  if (ml_logdom_1(kLdEntropy, pSrcA, blockSize, &r, true, 1, nullptr, "arm_entropy_f32") != ARM_MATH_SUCCESS)
    return __builtin_nanf("");
  return r;
}
float32_t arm_logsumexp_f32(const float32_t* in, uint32_t blockSize) {
  float32_t r = 0.0f;
  if (ml_logdom_1(kLdLogsumexp, in, blockSize, &r, true, 1, nullptr, "arm_logsumexp_f32") != ARM_MATH_SUCCESS)
    return __builtin_nanf("");
  return r;
}
float32_t arm_kullback_leibler_f32(const float32_t* pSrcA, const float32_t* pSrcB, uint32_t blockSize) {
  float32_t r = 0.0f;
  if (ml_logdom_2(kLdKullbackLeibler, pSrcA, pSrcB, blockSize, blockSize, &r, true, 1, nullptr,
                  "arm_kullback_leibler_f32") != ARM_MATH_SUCCESS)
    return __builtin_nanf("");
  return r;
}
float32_t arm_logsumexp_dot_prod_f32(const float32_t* pSrcA, const float32_t* pSrcB, uint32_t blockSize,
                                     float32_t* pTmpBuffer) {
  float32_t r = 0.0f;
  if (ml_logsumexp_dot_sync(pSrcA, pSrcB, blockSize, pTmpBuffer, &r, "arm_logsumexp_dot_prod_f32") != ARM_MATH_SUCCESS)
    return __builtin_nanf("");
  return r;
}
arm_status arm_entropy_f32_batch(const float32_t* d_src, uint32_t blockSize, float32_t* d_result, uint32_t batch,
                                 void* stream) {
  return ml_logdom_1(kLdEntropy, d_src, blockSize, d_result, false, batch, stream, "arm_entropy_f32_batch");
}
arm_status arm_logsumexp_f32_batch(const float32_t* d_src, uint32_t blockSize, float32_t* d_result, uint32_t batch,
                                   void* stream) {
  return ml_logdom_1(kLdLogsumexp, d_src, blockSize, d_result, false, batch, stream, "arm_logsumexp_f32_batch");
}
arm_status arm_kullback_leibler_f32_batch(const float32_t* d_a, const float32_t* d_b, uint32_t bStride,
                                          uint32_t blockSize, float32_t* d_result, uint32_t batch, void* stream) {
  return ml_logdom_2(kLdKullbackLeibler, d_a, d_b, bStride, blockSize, d_result, false, batch, stream,
                     "arm_kullback_leibler_f32_batch");
}
arm_status arm_logsumexp_dot_prod_f32_batch(const float32_t* d_a, const float32_t* d_b, uint32_t bStride,
                                            uint32_t blockSize, float32_t* d_result, uint32_t batch, void* stream) {
  return ml_logdom_2(kLdLogsumexpDot, d_a, d_b, bStride, blockSize, d_result, false, batch, stream,
                     "arm_logsumexp_dot_prod_f32_batch");
}

void arm_svm_linear_init_f32(arm_svm_linear_instance_f32* S, uint32_t nbOfSupportVectors, uint32_t vectorDimension,
                             float32_t intercept, const float32_t* dualCoefficients, const float32_t* supportVectors,
                             const int32_t* classes) {
  if (!S) { refuse(true, "arm_svm_linear_init_f32"); return; }
  *S = {nbOfSupportVectors, vectorDimension, intercept, dualCoefficients, supportVectors, classes};
}
void arm_svm_polynomial_init_f32(arm_svm_polynomial_instance_f32* S, uint32_t nbOfSupportVectors,
                                 uint32_t vectorDimension, float32_t intercept, const float32_t* dualCoefficients,
                                 const float32_t* supportVectors, const int32_t* classes, int32_t degree,
                                 float32_t coef0, float32_t gamma) {
  if (!S) { refuse(true, "arm_svm_polynomial_init_f32"); return; }
  *S = {nbOfSupportVectors, vectorDimension, intercept, dualCoefficients, supportVectors, classes, degree, coef0, gamma};
}
void arm_svm_rbf_init_f32(arm_svm_rbf_instance_f32* S, uint32_t nbOfSupportVectors, uint32_t vectorDimension,
                          float32_t intercept, const float32_t* dualCoefficients, const float32_t* supportVectors,
                          const int32_t* classes, float32_t gamma) {
  if (!S) { refuse(true, "arm_svm_rbf_init_f32"); return; }
  *S = {nbOfSupportVectors, vectorDimension, intercept, dualCoefficients, supportVectors, classes, gamma};
}

#define MI355X_ML_SVM(NAME, KIND)                                                                                \
  void arm_svm_##NAME##_predict_f32(const arm_svm_##NAME##_instance_f32* S, const float32_t* in,                 \
                                    int32_t* pResult) {                                                          \
    const char* what = "arm_svm_" #NAME "_predict_f32";                                                          \
    if (!S) { refuse(true, what); return; }                                                                      \
    ml_svm(KIND, svm_model(S), in, pResult, nullptr, true, 1, nullptr, what);                                    \
  }                                                                                                              \
  arm_status arm_svm_##NAME##_predict_f32_batch(const arm_svm_##NAME##_instance_f32* S, const float32_t* d_in,   \
                                                int32_t* d_result, float32_t* d_decision, uint32_t nbItems,      \
                                                void* stream) {                                                  \
    if (!S) return ARM_MATH_ARGUMENT_ERROR;                                                                      \
    return ml_svm(KIND, svm_model(S), d_in, d_result, d_decision, false, nbItems, stream,                        \
                  "arm_svm_" #NAME "_predict_f32_batch");                                                        \
  }
MI355X_ML_SVM(linear, kSvmLinear)
MI355X_ML_SVM(polynomial, kSvmPolynomial)
MI355X_ML_SVM(rbf, kSvmRbf)
#undef MI355X_ML_SVM

uint32_t arm_gaussian_naive_bayes_predict_f32(const arm_gaussian_naive_bayes_instance_f32* S, const float32_t* in,
                                              float32_t* pOutputProbabilities, float32_t* pBufferB) {
  (void)pBufferB;                                            // unused, as in the reference's scalar branch
  uint32_t index = 0;
  if (ml_bayes(S, in, pOutputProbabilities, &index, true, 1, nullptr, "arm_gaussian_naive_bayes_predict_f32") !=
      ARM_MATH_SUCCESS)
    return 0xffffffffu;
  return index;
}
arm_status arm_gaussian_naive_bayes_predict_f32_batch(const arm_gaussian_naive_bayes_instance_f32* S,
                                                      const float32_t* d_in, float32_t* d_probabilities,
                                                      uint32_t* d_class, uint32_t nbItems, void* stream) {
  return ml_bayes(S, d_in, d_probabilities, d_class, false, nbItems, stream,
                  "arm_gaussian_naive_bayes_predict_f32_batch");
}
}  // extern "C"

// ---- quaternions (quaternion.hip) --------------------------------------------------------------------------
// quaternion_math_functions.h.  One helper: a source of wa words per item, an optional second factor at bStride
// words (0 or 4), a result of wd words per item.  A result of quaternions may be a source of quaternions exactly;
// any other overlap is refused.  nbQuaternions == 0 is a successful no-op.
namespace {
arm_status qt_call(int op, const float* a, const float* b, uint32_t bStride, float* d, uint32_t n, bool sync,
                   void* stream, const char* what) {
  const size_t wa = op == kQtFromRotation ? 9 : 4, wd = op == kQtNorm ? 1 : op == kQtToRotation ? 9 : 4;
  const bool two = op == kQtProduct;
  const unsigned in = wa == wd ? kIn | kExactOk : kIn;
  const size_t bwords = n ? (size_t)bStride * (n - 1) + 4 : 0;
  const VecCall c{what, sync, stream, 0, two ? 3 : 2,
                  {{a, sizeof(float) * wa * n, in}, {d, sizeof(float) * wd * n, kOut}, {b, sizeof(float) * bwords, in}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (two && bStride != 0 && bStride != 4) return refuse(sync, what);
  if (n == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return quaternion_launch(op, (const float*)p[0], (const float*)p[2], bStride, (float*)p[1], n, st);
  });
}
}  // namespace

extern "C" {
#define MI355X_QT_1(NAME, OP)                                                                                    \
  void arm_##NAME##_f32(const float32_t* pSrc, float32_t* pDst, uint32_t nbQuaternions) {                        \
    qt_call(OP, pSrc, nullptr, 0, pDst, nbQuaternions, true, nullptr, "arm_" #NAME "_f32");                      \
  }                                                                                                              \
  arm_status arm_##NAME##_f32_batch(const float32_t* d_src, float32_t* d_dst, uint32_t nbQuaternions,            \
                                    void* stream) {                                                              \
    return qt_call(OP, d_src, nullptr, 0, d_dst, nbQuaternions, false, stream, "arm_" #NAME "_f32_batch");       \
  }
MI355X_QT_1(quaternion_norm, kQtNorm)
MI355X_QT_1(quaternion_inverse, kQtInverse)
MI355X_QT_1(quaternion_conjugate, kQtConjugate)
MI355X_QT_1(quaternion_normalize, kQtNormalize)
MI355X_QT_1(quaternion2rotation, kQtToRotation)
MI355X_QT_1(rotation2quaternion, kQtFromRotation)
#undef MI355X_QT_1

void arm_quaternion_product_f32(const float32_t* qa, const float32_t* qb, float32_t* qr, uint32_t nbQuaternions) {
  qt_call(kQtProduct, qa, qb, 4, qr, nbQuaternions, true, nullptr, "arm_quaternion_product_f32");
}
void arm_quaternion_product_single_f32(const float32_t* qa, const float32_t* qb, float32_t* qr) {
  qt_call(kQtProduct, qa, qb, 4, qr, 1, true, nullptr, "arm_quaternion_product_single_f32");
}
arm_status arm_quaternion_product_f32_batch(const float32_t* d_qa, const float32_t* d_qb, uint32_t bStride,
                                            float32_t* d_qr, uint32_t nbQuaternions, void* stream) {
  return qt_call(kQtProduct, d_qa, d_qb, bStride, d_qr, nbQuaternions, false, stream,
                 "arm_quaternion_product_f32_batch");
}
}  // extern "C"

// ---- interpolation (interp.hip) ----------------------------------------------------------------------------
// interpolation_functions.h.  The linear and bilinear drop-ins take one sample and are computed on the host from a
// host-readable table; their _batch forms, and both forms of the spline, run on the GPU.
namespace {
// a failed scalar drop-in returns 0 (a NaN from the f32 forms) and records the refusal
template <typename T>
T interp_refused(const char* what) {
  set_error(hipErrorInvalidValue, what);
  if (std::is_same<T, float>::value) return (T)__builtin_nanf("");
  return (T)0;
}

// launch(table, x, y, st)
template <typename T, typename X, typename Launch>
arm_status linear_batch(const T* table, uint32_t nValues, const X* x, T* y, uint32_t count, void* stream,
                        const char* what, Launch&& launch) {
  const VecCall c{what, false, stream, 0, 3,
                  {{table, sizeof(T) * (size_t)nValues, kIn}, {x, sizeof(X) * (size_t)count, kIn},
                   {y, sizeof(T) * (size_t)count, kOut}}};
  if (nValues == 0) return ARM_MATH_ARGUMENT_ERROR;
  if (count == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) { return launch((const T*)p[0], (const X*)p[1], (T*)p[2], st); });
}

// launch(table, X, Y, out, st)
template <typename T, typename X, typename Launch>
arm_status bilinear_batch(const T* table, uint32_t rows, uint32_t cols, const X* px, const X* py, T* out,
                          uint32_t count, void* stream, const char* what, Launch&& launch) {
  const VecCall c{what, false, stream, 0, 4,
                  {{table, sizeof(T) * (size_t)rows * cols, kIn}, {px, sizeof(X) * (size_t)count, kIn},
                   {py, sizeof(X) * (size_t)count, kIn}, {out, sizeof(T) * (size_t)count, kOut}}};
  if ((uint64_t)rows * cols >= 0x80000000ull) return ARM_MATH_ARGUMENT_ERROR;
  if (count == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return launch((const T*)p[0], (const X*)p[1], (const X*)p[2], (T*)p[3], st);
  });
}

arm_status spline_init(int type, const float* x, uint32_t xStride, const float* y, uint32_t n, float* coeffs,
                       float* temp, bool sync, uint32_t batch, void* stream, const char* what) {
  const size_t items = batch, xw = batch ? (size_t)xStride * (items - 1) + n : 0;
  const size_t cw = n ? 3 * ((size_t)n - 1) : 0, tw = n ? 2 * (size_t)n - 1 : 0;
  const VecCall c{what, sync, stream, 0, 4,
                  {{x, sizeof(float) * xw, kIn}, {y, sizeof(float) * n * items, kIn},
                   {coeffs, sizeof(float) * cw * items, kOut}, {temp, sizeof(float) * tw * items, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (n < 2 || (type != ARM_SPLINE_NATURAL && type != ARM_SPLINE_PARABOLIC_RUNOUT)) return refuse(sync, what);
  if (xStride != 0 && xStride < n) return refuse(sync, what);
  if (batch == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return spline_init_launch(type, (const float*)p[0], xStride, (const float*)p[1], n, (float*)p[2], (float*)p[3],
                              batch, st);
  });
}

arm_status spline_eval(const float* x, uint32_t xStride, const float* y, const float* coeffs, uint32_t n,
                       const float* xq, uint32_t xqStride, float* dst, uint32_t blockSize, bool sync, uint32_t batch,
                       void* stream, const char* what) {
  const size_t items = batch, xw = batch ? (size_t)xStride * (items - 1) + n : 0;
  const size_t qw = batch ? (size_t)xqStride * (items - 1) + blockSize : 0, cw = n ? 3 * ((size_t)n - 1) : 0;
  const VecCall c{what, sync, stream, 0, 5,
                  {{x, sizeof(float) * xw, kIn}, {y, sizeof(float) * n * items, kIn},
                   {coeffs, sizeof(float) * cw * items, kIn}, {xq, sizeof(float) * qw, kIn},
                   {dst, sizeof(float) * blockSize * items, kOut}}};
  if (c.null_in_sync()) return ARM_MATH_ARGUMENT_ERROR;
  if (n < 2) return refuse(sync, what);
  if ((xStride != 0 && xStride < n) || (xqStride != 0 && xqStride < blockSize)) return refuse(sync, what);
  if (batch == 0 || blockSize == 0) return ARM_MATH_SUCCESS;
  return c.run([&](void* const* p, hipStream_t st) {
    return spline_launch((const float*)p[0], xStride, (const float*)p[1], (const float*)p[2], n, (const float*)p[3],
                         xqStride, (float*)p[4], blockSize, batch, st);
  });
}
}  // namespace

extern "C" {
float32_t arm_linear_interp_f32(const arm_linear_interp_instance_f32* S, float32_t x) {
  if (!S || !S->pYData || S->nValues == 0) return interp_refused<float>("arm_linear_interp_f32");
  return linear_interp_f32_host(S->pYData, S->nValues, S->x1, S->xSpacing, x);
}
q31_t arm_linear_interp_q31(const q31_t* pYData, q31_t x, uint32_t nValues) {
  if (!pYData || nValues == 0) return interp_refused<q31_t>("arm_linear_interp_q31");
  return linear_interp_q31_host(pYData, nValues, x);
}
q15_t arm_linear_interp_q15(const q15_t* pYData, q31_t x, uint32_t nValues) {
  if (!pYData || nValues == 0) return interp_refused<q15_t>("arm_linear_interp_q15");
  return linear_interp_q15_host(pYData, nValues, x);
}
q7_t arm_linear_interp_q7(const q7_t* pYData, q31_t x, uint32_t nValues) {
  if (!pYData || nValues == 0) return interp_refused<q7_t>("arm_linear_interp_q7");
  return linear_interp_q7_host(pYData, nValues, x);
}
arm_status arm_linear_interp_f32_batch(const arm_linear_interp_instance_f32* S, const float32_t* d_x, float32_t* d_y,
                                       uint32_t blockSize, void* stream) {
  if (!S) return ARM_MATH_ARGUMENT_ERROR;
  const uint32_t nValues = S->nValues;
  const float x1 = S->x1, xSpacing = S->xSpacing;
  return linear_batch(S->pYData, nValues, d_x, d_y, blockSize, stream, "arm_linear_interp_f32_batch",
                      [&](const float* t, const float* x, float* y, hipStream_t st) {
                        return linear_interp_f32_launch(t, nValues, x1, xSpacing, x, y, blockSize, st);
                      });
}
#define MI355X_INTERP_Q(T, CT)                                                                                   \
  arm_status arm_linear_interp_##T##_batch(const CT* d_table, uint32_t nValues, const q31_t* d_x, CT* d_y,       \
                                           uint32_t blockSize, void* stream) {                                   \
    return linear_batch(d_table, nValues, d_x, d_y, blockSize, stream, "arm_linear_interp_" #T "_batch",         \
                        [&](const CT* t, const q31_t* x, CT* y, hipStream_t st) {                                \
                          return linear_interp_q_launch<CT>(t, nValues, x, y, blockSize, st);                    \
                        });                                                                                      \
  }                                                                                                              \
  CT arm_bilinear_interp_##T(arm_bilinear_interp_instance_##T* S, q31_t X, q31_t Y) {                            \
    if (!S || !S->pData || (uint64_t)S->numRows * S->numCols >= 0x80000000ull)                                   \
      return interp_refused<CT>("arm_bilinear_interp_" #T);                                                      \
    return bilinear_interp_##T##_host(S->pData, S->numRows, S->numCols, X, Y);                                   \
  }                                                                                                              \
  arm_status arm_bilinear_interp_##T##_batch(const arm_bilinear_interp_instance_##T* S, const q31_t* d_X,        \
                                             const q31_t* d_Y, CT* d_out, uint32_t blockSize, void* stream) {    \
    if (!S) return ARM_MATH_ARGUMENT_ERROR;                                                                      \
    const uint32_t rows = S->numRows, cols = S->numCols;                                                         \
    return bilinear_batch(S->pData, rows, cols, d_X, d_Y, d_out, blockSize, stream,                              \
                          "arm_bilinear_interp_" #T "_batch",                                                    \
                          [&](const CT* t, const q31_t* x, const q31_t* y, CT* o, hipStream_t st) {              \
                            return bilinear_interp_q_launch<CT>(t, rows, cols, x, y, o, blockSize, st);          \
                          });                                                                                    \
  }
MI355X_INTERP_Q(q31, q31_t)
MI355X_INTERP_Q(q15, q15_t)
MI355X_INTERP_Q(q7, q7_t)
#undef MI355X_INTERP_Q

float32_t arm_bilinear_interp_f32(const arm_bilinear_interp_instance_f32* S, float32_t X, float32_t Y) {
  if (!S || !S->pData || (uint64_t)S->numRows * S->numCols >= 0x80000000ull)
    return interp_refused<float>("arm_bilinear_interp_f32");
  return bilinear_interp_f32_host(S->pData, S->numRows, S->numCols, X, Y);
}
arm_status arm_bilinear_interp_f32_batch(const arm_bilinear_interp_instance_f32* S, const float32_t* d_X,
                                         const float32_t* d_Y, float32_t* d_out, uint32_t blockSize, void* stream) {
  if (!S) return ARM_MATH_ARGUMENT_ERROR;
  const uint32_t rows = S->numRows, cols = S->numCols;
  return bilinear_batch(S->pData, rows, cols, d_X, d_Y, d_out, blockSize, stream, "arm_bilinear_interp_f32_batch",
                        [&](const float* t, const float* x, const float* y, float* o, hipStream_t st) {
                          return bilinear_interp_f32_launch(t, rows, cols, x, y, o, blockSize, st);
                        });
}

void arm_spline_init_f32(arm_spline_instance_f32* S, arm_spline_type type, const float32_t* x, const float32_t* y,
                         uint32_t n, float32_t* coeffs, float32_t* tempBuffer) {
  if (!S) { refuse(true, "arm_spline_init_f32"); return; }
  if (spline_init((int)type, x, 0, y, n, coeffs, tempBuffer, true, 1, nullptr, "arm_spline_init_f32") !=
      ARM_MATH_SUCCESS)
    return;
  S->x = x;
  S->y = y;
  S->n_x = n;
  S->coeffs = coeffs;
}
void arm_spline_f32(arm_spline_instance_f32* S, const float32_t* xq, float32_t* pDst, uint32_t blockSize) {
  if (!S) { refuse(true, "arm_spline_f32"); return; }
  spline_eval(S->x, 0, S->y, S->coeffs, S->n_x, xq, 0, pDst, blockSize, true, 1, nullptr, "arm_spline_f32");
}
arm_status arm_spline_init_f32_batch(arm_spline_type type, const float32_t* d_x, uint32_t xStride,
                                     const float32_t* d_y, uint32_t n, float32_t* d_coeffs, float32_t* d_temp,
                                     uint32_t batch, void* stream) {
  return spline_init((int)type, d_x, xStride, d_y, n, d_coeffs, d_temp, false, batch, stream,
                     "arm_spline_init_f32_batch");
}
arm_status arm_spline_f32_batch(const float32_t* d_x, uint32_t xStride, const float32_t* d_y,
                                const float32_t* d_coeffs, uint32_t n, const float32_t* d_xq, uint32_t xqStride,
                                float32_t* d_dst, uint32_t blockSize, uint32_t batch, void* stream) {
  return spline_eval(d_x, xStride, d_y, d_coeffs, n, d_xq, xqStride, d_dst, blockSize, false, batch, stream,
                     "arm_spline_f32_batch");
}
}  // extern "C"
