// C ABI of libcmsisdsp_mi355x.so: the drop-in processing functions of arm_math.h and the
// batched device API of arm_math_mi355x.h.  Every GPU failure is caught here and mapped
// to the reference's status values (or the thread-local error channel for void functions);
// nothing aborts.  There is no CPU fallback: all compute runs in the HIP kernels.
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/arm_math.h"
#include "../../include/arm_math_mi355x.h"
#include "common.hpp"
#include "kernels.hpp"
#include "runtime.hpp"

using namespace mi355x;

namespace {

bool cfft_len_ok(uint32_t n) {
  return n == 16 || n == 32 || n == 64 || n == 128 || n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096;
}

#define MI_CHECK(expr, where)                        \
  do {                                               \
    hipError_t e_ = (expr);                          \
    if (e_ != hipSuccess) { set_error(e_, where); return false; } \
  } while (0)

// status of a batched entry point whose last step returned e; a failure is recorded under `what`
arm_status batch_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return ARM_MATH_SUCCESS;
  set_error(e, what);
  return ARM_MATH_ARGUMENT_ERROR;
}

struct CfftPrep {
  const void* tw = nullptr;
  const uint16_t* perm = nullptr;
  uint32_t flags = 0;
  // a 4-byte-aligned copy of a q15 twiddle table that sits on an odd 2-byte boundary (cfft_prepare),
  // freed in stream order after the launches of the call that holds this
  void* tw_copy = nullptr;
  hipStream_t st = nullptr;
  CfftPrep() = default;
  CfftPrep(const CfftPrep&) = delete;
  CfftPrep& operator=(const CfftPrep&) = delete;
  ~CfftPrep() {
    if (tw_copy) (void)hipFreeAsync(tw_copy, st);
  }
};

// kind: 0 f32, 1 q31, 2 q15; st: the stream the call's launches go to
bool cfft_prepare(uint32_t n, const void* pTwiddle, const uint16_t* pBitRev, uint16_t bitRevLen, int kind,
                  uint8_t ifftFlag, uint8_t bitReverseFlag, hipStream_t st, CfftPrep& out) {
  // twiddle words: f32 N complex (twiddleCoef_N[2N]); fixed-point 3N/4 complex
  // (twiddleCoef_N_q31[3N/2], arm_common_tables.h:61-116)
  const size_t twb = kind == 0 ? 8u * n : (kind == 1 ? 4u * 3u * n / 2u : 2u * 3u * n / 2u);
  out.tw = device_table(pTwiddle, twb);
  if (!out.tw) return false;   // device_table recorded the cause
  // The q15 kernels read a twiddle as one (cos, sin) dword, and the lane-uniform ones (the last
  // pass of cfft_fx_r16_kernel, stage 5 of cfft_q15_4096_pk_kernel) through the scalar cache, which
  // drops the low two address bits.  The library's tables and the cache's copies are at least
  // 4-byte aligned; a q15_t table resident in device memory need not be ("Pointer
  // alignment contract"): it is copied to an aligned buffer on the call's stream, the kernels and
  // the aligned path are untouched.
  if (kind == 2 && ((uintptr_t)out.tw & 3u) != 0) {
    hipError_t e = hipMallocAsync(&out.tw_copy, twb, st);
    if (e != hipSuccess) { out.tw_copy = nullptr; set_error(e, "cfft twiddle copy"); return false; }
    out.st = st;
    e = hipMemcpyAsync(out.tw_copy, out.tw, twb, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) { set_error(e, "cfft twiddle copy"); return false; }
    out.tw = out.tw_copy;
  }
  out.flags = (ifftFlag == 1u ? kIfft : 0u) | (bitReverseFlag ? kBitrev : 0u);   // arm_cfft_f32.c:1252,1282
  if (bitReverseFlag) {
    bool canon = true, ok = true;
    out.perm = device_perm((int)n, pBitRev, bitRevLen, kind == 0 ? 0 : 1, &canon, &ok);
    if (!ok) { set_error(hipErrorInvalidValue, "bit-reversal table"); return false; }
  }
  return true;
}

hipError_t cfft_launch(int kind, uint32_t n, void* d, uint32_t batch, const CfftPrep& pr, hipStream_t st) {
  switch (kind) {
    case 0: return cfft_f32_launch((int)n, (float*)d, batch, (const float*)pr.tw, pr.perm, pr.flags, st);
    case 1: return cfft_q31_launch((int)n, (int32_t*)d, batch, (const int32_t*)pr.tw, pr.perm, pr.flags, st);
    default: return cfft_q15_launch((int)n, (int16_t*)d, batch, (const int16_t*)pr.tw, pr.perm, pr.flags, st);
  }
}

// synchronous single-transform drop-in path (host or device buffer)
template <typename Inst>
void cfft_sync(const Inst* S, void* p1, uint8_t ifftFlag, uint8_t bitReverseFlag, int kind, size_t word) {
  if (!S || !p1 || !cfft_len_ok(S->fftLen)) return;       // reference: silent no-op
  const uint32_t n = S->fftLen;
  hipStream_t st = sync_stream();
  BlobScope hold(st);
  CfftPrep pr;
  if (!cfft_prepare(n, S->pTwiddle, S->pBitRevTable, S->bitRevLength, kind, ifftFlag, bitReverseFlag, st, pr)) return;
  const size_t bytes = 2 * word * n;
  if (is_device_ptr(p1)) {
    hipError_t e = cfft_launch(kind, n, p1, 1, pr, st);
    if (e == hipSuccess) e = wait_stream(st);
    if (e != hipSuccess) set_error(e, "arm_cfft");
    return;
  }
  if (bytes <= kZeroCopyMax) {               // one launch on the coherent pinned copy, no DMA
    HostIO io(st);
    void* z = io.zinout(p1, bytes);
    if (!z) { set_error(hipErrorOutOfMemory, "arm_cfft staging"); return; }
    // N = 1024 f32 (the reference example's shape): the transform's workgroup also writes the
    // completion word, so the call is one launch (runtime.hpp done_slot)
    uint32_t* done = nullptr;
    uint32_t seq = 0;
    if (kind == 0 && n == 1024 && !pr.perm && done_slot(&done, &seq) &&
        cfft_f32_n1024_done_launch((float*)z, 1, (const float*)pr.tw, pr.perm, pr.flags, done, seq, st)) {
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = io.finish(seq);
      if (e != hipSuccess) set_error(e, "arm_cfft");
      return;
    }
    hipError_t e = cfft_launch(kind, n, z, 1, pr, st);
    if (e == hipSuccess) e = io.finish();
    if (e != hipSuccess) set_error(e, "arm_cfft");
    return;
  }
  void* d = scratch(bytes, 0);
  if (!d) { set_error(hipErrorOutOfMemory, "arm_cfft scratch"); return; }
  HostIO io(st);
  hipError_t e = io.in(d, p1, bytes);
  if (e == hipSuccess) e = cfft_launch(kind, n, d, 1, pr, st);
  if (e == hipSuccess) e = io.out(p1, d, bytes);
  if (e == hipSuccess) e = io.finish();
  if (e != hipSuccess) set_error(e, "arm_cfft");
}

template <typename Inst>
arm_status cfft_batch(const Inst* S, void* d_p1, uint32_t batch, uint8_t ifftFlag, uint8_t bitReverseFlag,
                      void* stream, int kind) {
  if (!S || (!d_p1 && batch) || !cfft_len_ok(S->fftLen)) return ARM_MATH_ARGUMENT_ERROR;
  BlobScope hold((hipStream_t)stream);
  CfftPrep pr;
  if (!cfft_prepare(S->fftLen, S->pTwiddle, S->pBitRevTable, S->bitRevLength, kind, ifftFlag, bitReverseFlag,
                    (hipStream_t)stream, pr))
    return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(cfft_launch(kind, S->fftLen, d_p1, batch, pr, (hipStream_t)stream), "arm_cfft_batch");
}

// multi-GPU: validate every shard, launch each on its device's internal stream (one BlobScope per
// shard, so the tables a shard uses stay held until its launches are enqueued), then wait for
// every device that received work.  launch(s, st) enqueues shard s on st (its device current).
template <typename Launch>
arm_status run_multi(uint32_t nshards, const int* devices, const uint32_t* batch, const char* what, Launch&& launch) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }
  for (uint32_t s = 0; s < nshards; ++s)
    if (devices[s] < 0 || devices[s] >= ndev) return ARM_MATH_ARGUMENT_ERROR;
  int prev = 0;
  (void)hipGetDevice(&prev);
  std::vector<int> used;
  arm_status status = ARM_MATH_SUCCESS;
  for (uint32_t s = 0; s < nshards && status == ARM_MATH_SUCCESS; ++s) {
    if (!batch[s]) continue;
    hipError_t e = hipSetDevice(devices[s]);
    if (e != hipSuccess) { set_error(e, what); status = ARM_MATH_ARGUMENT_ERROR; break; }
    if (std::find(used.begin(), used.end(), devices[s]) == used.end()) used.push_back(devices[s]);
    hipStream_t st = sync_stream();
    if (!st) { set_error(hipErrorOutOfMemory, what); status = ARM_MATH_ARGUMENT_ERROR; break; }
    BlobScope hold(st);
    if (!launch(s, st)) status = ARM_MATH_ARGUMENT_ERROR;
  }
  for (int d : used) {   // drain every device that received work, also after a failure
    hipError_t e = hipSetDevice(d);
    if (e == hipSuccess) e = hipStreamSynchronize(sync_stream());
    if (e != hipSuccess) { set_error(e, what); status = ARM_MATH_ARGUMENT_ERROR; }
  }
  (void)hipSetDevice(prev);
  return status;
}

template <typename Inst>
arm_status cfft_batch_multi(const Inst* S, uint32_t nshards, const int* devices, void* const* d_p1,
                            const uint32_t* batch, uint8_t ifftFlag, uint8_t bitReverseFlag, int kind) {
  if (!S || !cfft_len_ok(S->fftLen) || (nshards && (!devices || !d_p1 || !batch))) return ARM_MATH_ARGUMENT_ERROR;
  for (uint32_t s = 0; s < nshards; ++s)
    if (batch[s] && !d_p1[s]) return ARM_MATH_ARGUMENT_ERROR;
  return run_multi(nshards, devices, batch, "arm_cfft_batch_multi", [&](uint32_t s, hipStream_t st) {
    CfftPrep pr;
    if (!cfft_prepare(S->fftLen, S->pTwiddle, S->pBitRevTable, S->bitRevLength, kind, ifftFlag, bitReverseFlag, st, pr))
      return false;
    hipError_t e = cfft_launch(kind, S->fftLen, d_p1[s], batch[s], pr, st);
    if (e != hipSuccess) { set_error(e, "arm_cfft_batch_multi"); return false; }
    return true;
  });
}

bool rfft_len_ok(uint32_t n) { return n >= 32 && n <= 4096 && (n & (n - 1)) == 0; }

// arm_rfft_fast_f32.c:675-699 on `batch` signals; d_p / d_out device pointers
// p_scratch (ARM_MI355X_RFFT_P_SCRATCH): the forward fused kernels skip writing the inner CFFT's
// output back into p (the reference documents p as scratch; the drop-in always writes it).
bool rfft_run(const arm_rfft_fast_instance_f32* S, float* d_p, float* d_out, uint32_t batch, uint8_t ifftFlag,
              hipStream_t st, bool p_scratch = false) {
  const uint32_t n = S->fftLenRFFT, h = S->Sint.fftLen;
  if (h != n / 2 || !cfft_len_ok(h)) { set_error(hipErrorInvalidValue, "rfft instance"); return false; }
  BlobScope hold(st);
  const void* twr = device_table(S->pTwiddleRFFT, sizeof(float) * n);
  if (!twr) return false;
  CfftPrep pr;
  // the inner CFFT receives ifftFlag unchanged and bitReverseFlag = 1 (:689, :694)
  if (!cfft_prepare(h, S->Sint.pTwiddle, S->Sint.pBitRevTable, S->Sint.bitRevLength, 0, ifftFlag, 1, st, pr))
    return false;
  if (!pr.perm && ifftFlag <= 1) {   // the reference's own tables: one fused launch
    // (ifftFlag > 1: merge + a FORWARD inner CFFT, arm_cfft_f32.c:1252 -- unfused path)
    MI_CHECK(rfft_f32_fused_launch((int)n, ifftFlag != 0, d_p, (ifftFlag || p_scratch) ? nullptr : d_p, d_out, batch,
                                   (const float*)pr.tw, (const float*)twr, st),
             "rfft fused");
    return true;
  }
  if (ifftFlag) {
    MI_CHECK(rfft_f32_merge_launch((int)n, d_p, d_out, batch, (const float*)twr, st), "rfft merge");
    MI_CHECK(cfft_f32_launch((int)h, d_out, batch, (const float*)pr.tw, pr.perm, pr.flags, st), "rfft cfft");
  } else {
    MI_CHECK(cfft_f32_launch((int)h, d_p, batch, (const float*)pr.tw, pr.perm, pr.flags, st), "rfft cfft");
    MI_CHECK(rfft_f32_stage_launch((int)n, d_p, d_out, batch, (const float*)twr, st), "rfft stage");
  }
  return true;
}

// ---- RFFT q31 / q15 (arm_rfft_q31.c:148-183, arm_rfft_q15.c): `batch` signals.
// Forward: d_src [batch][N] (overwritten by the inner CFFT, as the reference leaves pSrc),
// d_dst [batch][2N].  Inverse: d_src [batch][2N] spectrum rows (words 0 .. N+1 read),
// d_dst [batch][N]; the final arm_shift(+1) is folded into the inverse CFFT's store.
template <typename T, typename RInst>
bool rfft_fixed_run(const RInst* S, T* d_src, T* d_dst, uint32_t batch, hipStream_t st) {
  constexpr int kind = sizeof(T) == 4 ? 1 : 2;
  const uint32_t n = S->fftLenReal, L = n / 2;
  const auto* in = S->pCfft;
  if (!in || in->fftLen != L || !cfft_len_ok(L) || n > 8192) { set_error(hipErrorInvalidValue, "rfft instance"); return false; }
  BlobScope hold(st);
  const bool inv = S->ifftFlagR == 1u;
  CfftPrep pr;
  if (!cfft_prepare(L, in->pTwiddle, in->pBitRevTable, in->bitRevLength, kind, inv ? 1 : 0, S->bitReverseFlagR, st, pr))
    return false;
  // forward, the reference's own bit reversal, bitReverseFlag 1: the split runs inside the CFFT
  // launch (cfft_fixed.hip L = 4096 from the tables as they are; cfft_fixed_r16.hip L = 256 .. 2048
  // from packed per-bin records)
  const bool fuse = !inv && !pr.perm && (pr.flags & kBitrev) &&
                    (L == 4096 ? (kind == 1 ? MI355X_RFFT_Q31_FUSED : MI355X_RFFT_Q15_FUSED && MI355X_FX_Q15_PACKED)
                               : L >= 256 && L <= 2048 && MI355X_RFFT_FX_R16_FUSED);
  // inverse, same conditions: the merge runs in the CFFT's first pass (cfft_fixed_r16.hip L = 256 ..
  // 2048, cfft_fixed.hip L = 4096 -- q31 there stages half the records, so only for tables whose
  // records are symmetric, as the reference's realCoefAQ31 / BQ31 are)
  bool ifuse = inv && !pr.perm && (pr.flags & kBitrev) &&
               (L == 4096 ? (kind == 1 ? MI355X_RFFT_Q31_INV_FUSED : MI355X_RFFT_Q15_INV_FUSED && MI355X_FX_Q15_PACKED)
                          : L >= 256 && L <= 2048 && MI355X_RFFT_FX_R16_INV_FUSED);
  const void* irec = nullptr;
  if (ifuse) {
    bool sym = false;
    irec = device_split_records(S->pTwiddleAReal, S->pTwiddleBReal, S->twidCoefRModifier, L, (int)sizeof(T), st, &sym);
    if (!irec) return false;
    if (kind == 1 && L == 4096 && !sym) ifuse = false;
  }
  // the split / merge pass reads realCoef[2*mod*k + 1] for k < L: mod * N words cover it
  const T *ta = nullptr, *tb = nullptr;
  if ((!fuse && !ifuse) || (fuse && L == 4096)) {
    const size_t words = std::max<size_t>(2, (size_t)S->twidCoefRModifier * n);
    ta = (const T*)device_table(S->pTwiddleAReal, sizeof(T) * words);
    tb = (const T*)device_table(S->pTwiddleBReal, sizeof(T) * words);
    if (!ta || !tb) return false;
  }
  auto pass = [&](const T* a, T* b) {
    if constexpr (kind == 1)
      return rfft_q31_pass_launch(inv, (int)n, a, b, batch, ta, tb, S->twidCoefRModifier, st);
    else
      return rfft_q15_pass_launch(inv, (int)n, a, b, batch, ta, tb, S->twidCoefRModifier, st);
  };
  if (ifuse) {
    if (L == 4096) {
      MI_CHECK(kind == 1 ? rfft_q31_8192_inv_fused_launch((const int32_t*)d_src, (int32_t*)d_dst, batch, (const int32_t*)pr.tw, irec, st)
                         : rfft_q15_8192_inv_fused_launch((const int16_t*)d_src, (int16_t*)d_dst, batch, (const int16_t*)pr.tw, irec, st),
               "rfft inverse fused 8192");
      return true;
    }
    const bool done = kind == 1
        ? rfft_q31_r16_inv_fused_launch((int)L, (const int32_t*)d_src, (int32_t*)d_dst, batch, (const int32_t*)pr.tw, irec, st)
        : rfft_q15_r16_inv_fused_launch((int)L, (const int16_t*)d_src, (int16_t*)d_dst, batch, (const int16_t*)pr.tw, irec, st);
    if (!done) { set_error(hipErrorInvalidValue, "rfft inverse fused length"); return false; }
    MI_CHECK(hipGetLastError(), "rfft inverse fused");
  } else if (inv) {
    MI_CHECK(pass(d_src, d_dst), "rfft merge");
    pr.flags |= kSatShl1;
    MI_CHECK(cfft_launch(kind, L, d_dst, batch, pr, st), "rfft cfft");
  } else if (fuse) {
    if (L == 4096) {
      MI_CHECK(kind == 1 ? rfft_q31_8192_fused_launch((int32_t*)d_src, (int32_t*)d_dst, batch, (const int32_t*)pr.tw,
                                                      (const int32_t*)ta, (const int32_t*)tb, S->twidCoefRModifier, st)
                         : rfft_q15_8192_fused_launch((int16_t*)d_src, (int16_t*)d_dst, batch, (const int16_t*)pr.tw,
                                                      (const int16_t*)ta, (const int16_t*)tb, S->twidCoefRModifier, st),
               "rfft fused");
    } else {
      const void* rec = device_split_records(S->pTwiddleAReal, S->pTwiddleBReal, S->twidCoefRModifier, L, (int)sizeof(T), st);
      if (!rec) return false;
      const bool done = kind == 1
          ? rfft_q31_r16_fused_launch((int)L, (int32_t*)d_src, (int32_t*)d_dst, batch, (const int32_t*)pr.tw, rec, st)
          : rfft_q15_r16_fused_launch((int)L, (int16_t*)d_src, (int16_t*)d_dst, batch, (const int16_t*)pr.tw, rec, st);
      if (!done) { set_error(hipErrorInvalidValue, "rfft fused length"); return false; }
      MI_CHECK(hipGetLastError(), "rfft fused");
    }
  } else {
    MI_CHECK(cfft_launch(kind, L, d_src, batch, pr, st), "rfft cfft");
    MI_CHECK(pass(d_src, d_dst), "rfft split");
  }
  return true;
}

// drop-in arm_rfft_q31 / _q15: host or device buffers, synchronous
template <typename T, typename RInst>
void rfft_fixed_sync(const RInst* S, T* pSrc, T* pDst) {
  if (!S || !pSrc || !pDst) return;
  const uint32_t n = S->fftLenReal;
  if (n < 32 || n > 8192 || (n & (n - 1))) return;   // reference: lengths of the init switch only
  const bool inv = S->ifftFlagR == 1u;
  // forward: src N words in/out, dst 2N out; inverse: src words 0..N+1 in, dst N out
  const size_t sb = sizeof(T) * (inv ? (size_t)n + 2 : n), db = sizeof(T) * (inv ? n : 2 * (size_t)n);
  hipStream_t st = sync_stream();
  const bool ds = is_device_ptr(pSrc), dd = is_device_ptr(pDst);
  // the batched inverse reads spectrum rows of 2N words: a host row is staged that wide
  T* s = ds ? pSrc : (T*)scratch(sizeof(T) * 2 * (size_t)n, 0);
  T* d = dd ? pDst : (T*)scratch(db, 1);
  if (!s || !d) { set_error(hipErrorOutOfMemory, "arm_rfft scratch"); return; }
  HostIO io(st);
  hipError_t e = hipSuccess;
  if (!ds) e = io.in(s, pSrc, sb);
  if (e != hipSuccess) { set_error(e, "arm_rfft"); return; }
  if (!rfft_fixed_run<T>(S, s, d, 1, st)) { (void)hipStreamSynchronize(st); return; }
  if (!ds && !inv) e = io.out(pSrc, s, sb);   // forward overwrites pSrc
  if (e == hipSuccess && !dd) e = io.out(pDst, d, db);
  if (e == hipSuccess) e = io.finish();
  if (e != hipSuccess) set_error(e, "arm_rfft");
}

template <typename T, typename RInst>
arm_status rfft_fixed_batch(const RInst* S, T* d_src, T* d_dst, uint32_t batch, void* stream) {
  if (!S || (batch && (!d_src || !d_dst))) return ARM_MATH_ARGUMENT_ERROR;
  const uint32_t n = S->fftLenReal;
  if (n < 32 || n > 8192 || (n & (n - 1))) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  return rfft_fixed_run<T>(S, d_src, d_dst, batch, (hipStream_t)stream) ? ARM_MATH_SUCCESS : ARM_MATH_ARGUMENT_ERROR;
}

// ---- MFCC (arm_mfcc_f32.c:83-160): the instance's user tables packed into one
// content-cached device blob: [dct | filter coefs | window | pos | len | coef offsets]
// (T words: f32, or q31 / q15 for the fixed-point instances, which append to it)
template <typename T>
struct MfccDev {
  int total = 0;                   // Mel coefficients (sum of filterLengths)
  const T* dct = nullptr;
  const T* coefs = nullptr;
  const T* win = nullptr;
  const uint32_t* pos = nullptr;
  const uint32_t* len = nullptr;
  const uint32_t* off = nullptr;
};

template <typename T>
bool host_copy(const T* p, size_t count, std::vector<T>& out) {
  out.resize(count);
  if (!count) return true;
  if (!p) return false;
  if (is_device_ptr(p)) return hipMemcpy(out.data(), p, sizeof(T) * count, hipMemcpyDeviceToHost) == hipSuccess;
  memcpy(out.data(), p, sizeof(T) * count);
  return true;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// byte offsets of the blob's parts (dct at 0), each padded to 16 B; end: where a caller may append
struct MfccLayout {
  size_t coefs, win, pos, len, off, end;
  uint64_t total;
};

// Packs the blob above from the instance's (host or device) tables: blob gets lay.end bytes, pos / len
// the filter tables.  bound: the bins a Mel filter may read (pos + len <= bound), `beyond` the error
// a filter past it is reported under.
template <typename T, typename Inst>
bool mfcc_pack(const Inst* S, uint32_t bound, const char* beyond, std::vector<uint8_t>& blob,
               std::vector<uint32_t>& pos, std::vector<uint32_t>& len, MfccLayout& lay) {
  const uint32_t n = S->fftLen, nm = S->nbMelFilters, nd = S->nbDctOutputs;
  if (!host_copy(S->filterPos, nm, pos) || !host_copy(S->filterLengths, nm, len)) {
    set_error(hipErrorInvalidValue, "mfcc filter tables");
    return false;
  }
  std::vector<uint32_t> off(nm);
  uint64_t total = 0;
  for (uint32_t i = 0; i < nm; ++i) {
    if ((uint64_t)pos[i] + len[i] > bound) { set_error(hipErrorInvalidValue, beyond); return false; }
    off[i] = (uint32_t)total;
    total += len[i];
  }
  const size_t b_u = up16(sizeof(uint32_t) * nm);
  lay.total = total;
  lay.coefs = up16(sizeof(T) * nm * nd);
  lay.win = lay.coefs + up16(sizeof(T) * total);
  lay.pos = lay.win + up16(sizeof(T) * n);
  lay.len = lay.pos + b_u;
  lay.off = lay.len + b_u;
  lay.end = lay.off + b_u;
  blob.assign(lay.end, 0);
  std::vector<T> tmp;
  if (!host_copy(S->dctCoefs, (size_t)nm * nd, tmp)) { set_error(hipErrorInvalidValue, "mfcc dct"); return false; }
  memcpy(blob.data(), tmp.data(), sizeof(T) * tmp.size());
  if (!host_copy(S->filterCoefs, (size_t)total, tmp)) { set_error(hipErrorInvalidValue, "mfcc coefs"); return false; }
  memcpy(blob.data() + lay.coefs, tmp.data(), sizeof(T) * tmp.size());
  if (!host_copy(S->windowCoefs, (size_t)n, tmp)) { set_error(hipErrorInvalidValue, "mfcc window"); return false; }
  memcpy(blob.data() + lay.win, tmp.data(), sizeof(T) * tmp.size());
  memcpy(blob.data() + lay.pos, pos.data(), sizeof(uint32_t) * nm);
  memcpy(blob.data() + lay.len, len.data(), sizeof(uint32_t) * nm);
  memcpy(blob.data() + lay.off, off.data(), sizeof(uint32_t) * nm);
  return true;
}

// the device views of the packed parts, dev the blob's device copy
template <typename T>
void mfcc_bind(MfccDev<T>& d, const uint8_t* dev, const MfccLayout& lay) {
  d.total = (int)lay.total;
  d.dct = (const T*)dev;
  d.coefs = (const T*)(dev + lay.coefs);
  d.win = (const T*)(dev + lay.win);
  d.pos = (const uint32_t*)(dev + lay.pos);
  d.len = (const uint32_t*)(dev + lay.len);
  d.off = (const uint32_t*)(dev + lay.off);
}

bool mfcc_prepare(const arm_mfcc_instance_f32* S, MfccDev<float>& d) {
  const uint32_t n = S->fftLen, nm = S->nbMelFilters;
  if (!rfft_len_ok(n) || S->rfft.fftLenRFFT != n) { set_error(hipErrorInvalidValue, "mfcc instance"); return false; }
  if (mfcc_f32_post_lds((int)n, (int)nm) > 65536) { set_error(hipErrorInvalidValue, "mfcc: too many Mel filters"); return false; }
  std::vector<uint8_t> blob;
  std::vector<uint32_t> pos, len;
  MfccLayout lay;
  if (!mfcc_pack<float>(S, n, "mfcc filter beyond fftLen", blob, pos, len, lay)) return false;
  blob.resize(lay.end + 16, 0);
  const uint8_t* dev = (const uint8_t*)device_blob(blob.data(), blob.size());
  if (!dev) return false;
  mfcc_bind(d, dev, lay);
  return true;
}

// x: [batch][n] frames, y: [batch][n] work, dst: [batch][nbDct].  The reference's own
// (canonical) CFFT tables take the fused single-launch kernel (x read once, y unused);
// otherwise three launches, x overwritten and the frame maxima carried in dst[frame][0]
// between the passes (read before the row is written).
bool mfcc_run(const arm_mfcc_instance_f32* S, const MfccDev<float>& d, float* x, float* y, float* dst, uint32_t batch,
              hipStream_t st) {
  const int n = (int)S->fftLen, nd = (int)S->nbDctOutputs, nm = (int)S->nbMelFilters;
  const arm_cfft_instance_f32& in = S->rfft.Sint;
  BlobScope hold(st);
  bool canon = true, ok = true;
  if (in.pBitRevTable) (void)device_perm((int)in.fftLen, in.pBitRevTable, in.bitRevLength, 0, &canon, &ok);
  if (ok && canon && nm <= n / 2 && in.fftLen == (uint32_t)n / 2) {
    const void* tw = device_table(in.pTwiddle, 8u * in.fftLen);
    const void* twr = device_table(S->rfft.pTwiddleRFFT, sizeof(float) * n);
    if (!tw || !twr) return false;
    MI_CHECK(mfcc_f32_fused_launch(n, x, d.win, (const float*)tw, (const float*)twr, nm, d.pos, d.len, d.off,
                                   d.coefs, nd, d.dct, dst, batch, d.total, st),
             "mfcc fused");
    return true;
  }
  MI_CHECK(mfcc_f32_pre_launch(n, x, d.win, x, dst, batch, nd, st), "mfcc pre");
  if (!rfft_run(&S->rfft, x, y, batch, 0, st)) return false;
  MI_CHECK(mfcc_f32_post_launch(n, y, dst, nd, nm, d.pos, d.len, d.off, d.coefs, nd, d.dct, dst, batch, st),
           "mfcc post");
  return true;
}

// ---- MFCC q31 / q15 (arm_mfcc_q31.c:88-225, arm_mfcc_q15.c:96-228): the same content-cached
// blob layout as the f32 instance in q31 / q15 words; the inner RFFT is the bit-exact batched
// fixed-point RFFT.  Mel filters must
// stay within the fftLen/2 + 1 magnitudes (the reference would read its CFFT's leftovers).
template <typename T>
struct MfccFxDev : MfccDev<T> {
  const uint32_t* bf = nullptr;    // flat Mel coefficient g -> bin << 16 | filter
  int kmin = 0, kcnt = 0;          // the bins some Mel filter reads: kmin .. kmin + kcnt - 1
  const int4* tw = nullptr;        // split twiddles per bin k <= fftLen/2: {A[2mk], A[2mk+1], B[2mk], B[2mk+1]}
  const int32_t* lut = nullptr;
};

// the blob: mfcc_pack's parts, then [bf | split twiddle records] (the records' packing is what
// mfcc_fixed_post.hpp reads)
template <typename T, typename Inst>
bool mfcc_prepare(const Inst* S, MfccFxDev<T>& d) {
  const uint32_t n = S->fftLen, nm = S->nbMelFilters;
  if (!rfft_len_ok(n) || S->rfft.fftLenReal != n || S->rfft.ifftFlagR != 0) {
    set_error(hipErrorInvalidValue, "mfcc q31 instance");
    return false;
  }
  if (mfcc_q31_post_lds((int)n, (int)nm) > 65536) { set_error(hipErrorInvalidValue, "mfcc q31: too many Mel filters"); return false; }
  std::vector<uint8_t> blob;
  std::vector<uint32_t> pos, len;
  MfccLayout lay;
  if (!mfcc_pack<T>(S, n / 2 + 1, "mfcc q31 filter beyond fftLen/2", blob, pos, len, lay)) return false;
  const uint64_t total = lay.total;
  if (nm > 0xFFFFu || total > 0x7FFFFFFFull) { set_error(hipErrorInvalidValue, "mfcc: too many Mel coefficients"); return false; }
  {
    uint32_t lo = n, hi = 0;
    for (uint32_t i = 0; i < nm; ++i)
      if (len[i]) { lo = std::min(lo, pos[i]); hi = std::max(hi, pos[i] + len[i]); }
    d.kmin = lo < hi ? (int)lo : 0;
    d.kcnt = lo < hi ? (int)(hi - lo) : 0;
  }
  const size_t b_bf = up16(sizeof(uint32_t) * total), b_tw = up16(sizeof(int4) * (n / 2 + 1));
  blob.resize(lay.end + b_bf + b_tw + 16, 0);
  uint32_t* bfh = reinterpret_cast<uint32_t*>(blob.data() + lay.end);
  for (uint32_t i = 0, g = 0; i < nm; ++i)
    for (uint32_t j = 0; j < len[i]; ++j) bfh[g++] = ((pos[i] + j) << 16) | i;
  {   // the split's twiddle records (arm_rfft_q31.c:293-326 index 2 * modifier * k)
    const uint32_t mod = S->rfft.twidCoefRModifier, words = mod * n;
    std::vector<T> ta, tb;
    if (!host_copy(S->rfft.pTwiddleAReal, words, ta) || !host_copy(S->rfft.pTwiddleBReal, words, tb)) {
      set_error(hipErrorInvalidValue, "mfcc rfft tables");
      return false;
    }
    int4* twh = reinterpret_cast<int4*>(blob.data() + lay.end + b_bf);
    for (uint32_t k = 1; k < n / 2; ++k) {
      const uint32_t c = 2 * mod * k;
      if constexpr (sizeof(T) == 2) {   // q15: packed pairs for v_dot2 (mfcc_fixed_post.hpp mq_split_q15)
        auto p2 = [](int32_t lo, int32_t hi) { return (int32_t)((uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16)); };
        const int32_t a0 = ta[c], a1 = ta[c + 1], b0 = tb[c], b1 = tb[c + 1];
        twh[k] = make_int4(p2(a0, ~a1), p2(b0, b1), p2(b1, ~b0), p2(a1, a0));
      } else {
        twh[k] = make_int4(ta[c], ta[c + 1], tb[c], tb[c + 1]);
      }
    }
  }
  const uint8_t* dev = (const uint8_t*)device_blob(blob.data(), blob.size());
  d.lut = (const int32_t*)device_table(sqrt_initial_lut_q31, sizeof(int32_t) * 32);
  if (!dev || !d.lut) return false;
  mfcc_bind(d, dev, lay);
  d.bf = (const uint32_t*)(dev + lay.end);
  d.tw = (const int4*)(dev + lay.end + b_bf);
  return true;
}

// x: [batch][n] frames (overwritten), y: [batch][2n] spectra, dst: [batch][nbDct]; the frame
// maxima ride in dst[frame][0] between the launches (read before the row is written)
// MFCC q31 / q15 schedule (MI355X_MFCC_FX_MODE, tuning.hpp; fftLen 512..4096 with the reference's
// own CFFT bit reversal): 1 = two launches (default: front end fused into the radix-16 CFFT's load
// phase, then the post kernel), 2 = one launch (round 4: front end, radix-16 CFFT and back end in
// one kernel, the spectra never leave LDS: traffic = the frames once, but 1.30 / 1.09 ms against
// 1.02 / 0.83 ms per 2^18 frames -- the CFFT and back-end phases of a workgroup serialise at two
// workgroups per CU), 0 = three launches (pre, CFFT, post: also every other length
// and custom bit-reversal tables).
template <typename T, typename Inst>
bool mfcc_run(const Inst* S, const MfccFxDev<T>& d, T* x, T* y, T* dst, uint32_t batch, hipStream_t st) {
  const int n = (int)S->fftLen, nd = (int)S->nbDctOutputs, nm = (int)S->nbMelFilters;
  // the forward RFFT's inner CFFT (arm_rfft_q31.c:148-183: cfft(L, fwd, bitReverseFlagR), then
  // arm_split_rfft): its tables and bit-reversal mode
  const auto* in = S->rfft.pCfft;
  const uint32_t L = (uint32_t)n / 2;
  if (!in || in->fftLen != L || !cfft_len_ok(L)) { set_error(hipErrorInvalidValue, "mfcc rfft instance"); return false; }
  BlobScope hold(st);
  CfftPrep pr;
  if (!cfft_prepare(L, in->pTwiddle, in->pBitRevTable, in->bitRevLength, sizeof(T) == 4 ? 1 : 2, 0,
                    S->rfft.bitReverseFlagR, st, pr))
    return false;
  if (MI355X_MFCC_FX_MODE >= 2 && !pr.perm) {    // the whole MFCC in one launch
    hipError_t e;
    if constexpr (sizeof(T) == 4)
      e = mfcc_q31_fused_launch((int)L, x, batch, (const int32_t*)pr.tw, d.win, S->rfft.bitReverseFlagR != 0, d.tw,
                                nm, d.coefs, d.bf, d.total, d.kmin, d.kcnt, nd, d.dct, d.lut, dst, st);
    else
      e = mfcc_q15_fused_launch((int)L, x, batch, (const int16_t*)pr.tw, d.win, S->rfft.bitReverseFlagR != 0, d.tw,
                                nm, d.coefs, d.bf, d.total, d.kmin, d.kcnt, nd, d.dct, d.lut, dst, st);
    if (e != hipErrorNotSupported) {
      MI_CHECK(e, "mfcc fused");
      return true;
    }
  }
  bool front = false;                       // pre + CFFT done by one launch
  if (MI355X_MFCC_FX_MODE >= 1 && !pr.perm) {
    if constexpr (sizeof(T) == 4)
      front = cfft_q31_r16_mfcc_launch((int)L, x, batch, (const int32_t*)pr.tw, d.win, dst, nd,
                                       S->rfft.bitReverseFlagR != 0, st);
    else
      front = cfft_q15_r16_mfcc_launch((int)L, x, batch, (const int16_t*)pr.tw, d.win, dst, nd,
                                       S->rfft.bitReverseFlagR != 0, st);
    if (front) MI_CHECK(hipGetLastError(), "mfcc front");
  }
  if (!front) {
    if constexpr (sizeof(T) == 4) {
      MI_CHECK(mfcc_q31_pre_launch(n, x, d.win, x, dst, batch, nd, st), "mfcc q31 pre");
    } else {
      MI_CHECK(mfcc_q15_pre_launch(n, x, d.win, x, dst, batch, nd, st), "mfcc q15 pre");
    }
    MI_CHECK(cfft_launch(sizeof(T) == 4 ? 1 : 2, L, x, batch, pr, st), "mfcc cfft");
  }
  (void)y;
  if constexpr (sizeof(T) == 4) {
    MI_CHECK(mfcc_q31_post_launch(n, x, d.tw, dst, nd, nm, d.kmin, d.kcnt, d.coefs, d.bf, d.total, nd, d.dct, d.lut, dst,
                                  batch, st),
             "mfcc q31 post");
  } else {
    MI_CHECK(mfcc_q15_post_launch(n, x, d.tw, dst, nd, nm, d.kmin, d.kcnt, d.coefs, d.bf, d.total, nd, d.dct, d.lut, dst,
                                  batch, st),
             "mfcc q15 post");
  }
  return true;
}

// Filter coefficients: device pointers in place, host sets through the content-keyed cache
// (uploaded synchronously once per distinct set, so an asynchronous batch call never
// shares a staging buffer with a later call on another stream).  nullptr: the upload failed,
// recorded as hipErrorOutOfMemory under `what`.
template <typename T>
const T* device_coeffs(const T* c, int n, const char* what) {
  const T* d = (const T*)device_table(c, sizeof(T) * (size_t)n);
  if (!d) set_error(hipErrorOutOfMemory, what);
  return d;
}

bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return bytes && x < y + bytes && y < x + bytes;
}

// ---- drop-in staging of the stateful filters (FIR, multirate, lattice, biquad) ---------------
// One synchronous call: the thread's stream, the scope that holds the coefficient blob, the
// coefficients on the device (nullptr: see device_coeffs) and which of the caller's three buffers
// are device memory.
template <typename T>
struct FilterCall {
  hipStream_t st;
  BlobScope hold;
  const T* dc;
  bool dstate, dsrc, ddst;
  FilterCall(const T* pCoeffs, int ncoef, const void* pState, const void* pSrc, const void* pDst, const char* what)
      : st(sync_stream()), hold(st), dc(device_coeffs(pCoeffs, ncoef, what)), dstate(is_device_ptr(pState)),
        dsrc(is_device_ptr(pSrc)), ddst(is_device_ptr(pDst)) {}
};

// The call's DMA path.  pState (hb bytes of ST words), pSrc (sb bytes) and pDst (ob bytes) lie each
// on the host or the device; host ones are staged through scratch slots 2, 3 and 4: state in, src
// in, run(dc, src, dst, state, st), dst out, state out.
// in_state: the block input is part of the state, [history (hb) ; block (sb)] (FIR, decimator,
// interpolator).  The reference copies each input into pState before it writes pDst
// (arm_fir_f32.c:947-975), so after the call the state holds [new history ; block input], and a
// device pSrc overlapping pDst is filtered from a copy of the input, which also feeds the new
// history and that tail.
// what_scratch: arm_fir names its scratch failure apart from its other errors.
template <typename T, typename ST, typename Run>
void filter_sync(FilterCall<T>& c, ST* pState, size_t hb, const T* pSrc, size_t sb, T* pDst, size_t ob, bool in_state,
                 const char* what, Run&& run, const char* what_scratch = nullptr) {
  hipStream_t st = c.st;
  const bool alias = in_state && c.dsrc && c.ddst && ranges_overlap(pSrc, pDst, std::max(sb, ob));
  ST* dhist = c.dstate ? pState : (ST*)scratch(hb + 16, 2);
  const T* dsr = (c.dsrc && !alias) ? pSrc : (const T*)scratch(sb + 16, 3);
  T* dds = c.ddst ? pDst : (T*)scratch(ob + 16, 4);
  if (!dhist || !dsr || !dds) { set_error(hipErrorOutOfMemory, what_scratch ? what_scratch : what); return; }
  HostIO io(st);
  hipError_t e = hipSuccess;
  if (!c.dstate && hb > 0) e = io.in(dhist, pState, hb);
  if (e == hipSuccess && alias) e = hipMemcpyAsync((void*)dsr, pSrc, sb, hipMemcpyDeviceToDevice, st);
  else if (e == hipSuccess && !c.dsrc) e = io.in((void*)dsr, pSrc, sb);
  if (e == hipSuccess) e = run(c.dc, dsr, dds, dhist, st);
  if (e == hipSuccess && !c.ddst && ob) e = io.out(pDst, dds, ob);
  if (e == hipSuccess && !c.dstate && hb > 0) e = io.out(pState, dhist, hb);
  if (e == hipSuccess && in_state) {
    void* tail = (uint8_t*)pState + hb;
    if (c.dstate) e = hipMemcpyAsync(tail, dsr, sb, hipMemcpyDeviceToDevice, st);
    else if (c.dsrc) e = io.out(tail, dsr, sb);
    else memcpy(tail, pSrc, sb);               // host input, host state: the caller's words
  }
  if (e == hipSuccess) e = io.finish();
  if (e == hipSuccess) c.hold.synced();
  if (e != hipSuccess) set_error(e, what);
}

// the whole call, for the families with no path in front of the DMA one
template <typename T, typename ST, typename Run>
void filter_sync(const T* pCoeffs, int ncoef, ST* pState, size_t hb, const T* pSrc, size_t sb, T* pDst, size_t ob,
                 bool in_state, const char* what, Run&& run) {
  FilterCall<T> c(pCoeffs, ncoef, pState, pSrc, pDst, what);
  if (c.dc) filter_sync(c, pState, hb, pSrc, sb, pDst, ob, in_state, what, run);
}

// drop-in FIR: state = [history(T-1) ; block(B)] on host or device (arm_fir_f32.c:911-1280).
// After the call the state holds [new history ; block input], as the reference leaves it.
template <typename T, typename Inst>
void fir_sync(const Inst* S, const T* pSrc, T* pDst, uint32_t B, int kind) {
  if (!S || !S->pState || !S->pCoeffs || S->numTaps == 0 || B == 0) return;
  const int taps = S->numTaps, T1 = taps - 1;
  FilterCall<T> c(S->pCoeffs, taps, S->pState, pSrc, pDst, "arm_fir coeffs");
  if (!c.dc) return;
  const size_t sb = sizeof(T) * (size_t)B, hb = sizeof(T) * (size_t)T1;
  if (!c.dstate && !c.dsrc && !c.ddst && hb + sb <= kZeroCopyMax) {
    // all host, small: the caller's state buffer itself, [history ; block], staged as one
    // coherent pinned copy the kernels use in place (the filter reads it, the history kernel
    // rewrites its head), so after finish() it holds [new history ; block input] exactly as the
    // reference leaves pState; outputs likewise -- two launches, no DMA
    HostIO io(c.st);
    T* zs = (T*)io.zinout(S->pState, hb + sb);
    T* zd = (T*)io.zout(pDst, sb);
    if (!zs || !zd) { set_error(hipErrorOutOfMemory, "arm_fir staging"); return; }
    memmove(zs + T1, pSrc, sb);                   // pSrc may alias pDst: read before anything
    uint32_t* done = nullptr;
    uint32_t seq = 0;
    bool flagged = false;                         // the filter's workgroup wrote the completion word
    if (!done_slot(&done, &seq)) done = nullptr;
    hipError_t e = fir_run(kind, c.dc, taps, zs + T1, zd, B, 1, zs, c.st, done, seq, &flagged);
    if (e == hipSuccess) e = io.finish(flagged ? seq : 0);
    if (e == hipSuccess) c.hold.synced();
    if (e != hipSuccess) set_error(e, "arm_fir");
    return;
  }
  filter_sync(c, S->pState, hb, pSrc, sb, pDst, sb, true, "arm_fir",
              [&](const T* dc, const T* src, T* dst, T* hist, hipStream_t st) {
                return fir_run(kind, dc, taps, src, dst, B, 1, hist, st);
              },
              "arm_fir scratch");
}

template <typename T, typename Inst>
arm_status fir_batch(const Inst* S, const T* d_src, T* d_dst, uint32_t B, uint32_t batch, T* d_hist, void* stream,
                     int kind) {
  if (!S || !S->pCoeffs || S->numTaps == 0 || (batch && B && (!d_src || !d_dst))) return ARM_MATH_ARGUMENT_ERROR;
  if (S->numTaps > 1 && batch && !d_hist) return ARM_MATH_ARGUMENT_ERROR;
  hipStream_t st = (hipStream_t)stream;
  BlobScope hold(st);
  const T* dc = device_coeffs<T>(S->pCoeffs, S->numTaps, "arm_fir_batch coeffs");
  if (!dc) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(fir_run(kind, dc, S->numTaps, d_src, d_dst, B, batch, d_hist, st), "arm_fir_batch");
}

// multi-GPU FIR (the batch is sliced by filter, each shard's history rows stay on
// its device): shard s = batch[s] filters at d_src[s] / d_dst[s] / d_hist[s] on devices[s].
template <typename T, typename Inst>
arm_status fir_batch_multi(const Inst* S, uint32_t nshards, const int* devices, const T* const* d_src, T* const* d_dst,
                           T* const* d_hist, uint32_t B, const uint32_t* batch, int kind) {
  if (!S || !S->pCoeffs || S->numTaps == 0 || (nshards && (!devices || !batch || !d_src || !d_dst || !d_hist)))
    return ARM_MATH_ARGUMENT_ERROR;
  for (uint32_t s = 0; s < nshards; ++s)
    if (batch[s] && ((B && (!d_src[s] || !d_dst[s])) || (S->numTaps > 1 && !d_hist[s]))) return ARM_MATH_ARGUMENT_ERROR;
  return run_multi(nshards, devices, batch, "arm_fir_batch_multi", [&](uint32_t s, hipStream_t st) {
    const T* dc = device_coeffs<T>(S->pCoeffs, S->numTaps, "arm_fir_batch_multi");   // uploaded once per device
    if (!dc) return false;
    hipError_t e = fir_run(kind, dc, S->numTaps, d_src[s], d_dst[s], B, batch[s], d_hist[s], st);
    if (e != hipSuccess) { set_error(e, "arm_fir_batch_multi"); return false; }
    return true;
  });
}

// zero a host or device buffer (the init functions' memset)
void zero_words(void* p, size_t bytes, const char* what) {
  if (is_device_ptr(p)) {
    hipError_t e = hipMemset(p, 0, bytes);
    if (e != hipSuccess) set_error(e, what);
  } else {
    memset(p, 0, bytes);
  }
}

// ---- multirate FIR (decimator / interpolator) ----------------------------------------
// Drop-in: state = [history (H) ; block (B)] on host or device; after the call it holds
// [new history ; block input], as the reference leaves it (the block is copied into pState
// before the pass, arm_fir_decimate_f32.c / arm_fir_interpolate_f32.c): filter_sync's in_state.
template <typename T, typename Inst>
arm_status decimate_init(Inst* S, uint16_t numTaps, uint8_t M, const T* pCoeffs, T* pState, uint32_t blockSize) {
  if (!S) return ARM_MATH_ARGUMENT_ERROR;
  if (M == 0 || blockSize % M) return ARM_MATH_LENGTH_ERROR;       // arm_fir_decimate_init_f32.c
  S->numTaps = numTaps; S->pCoeffs = pCoeffs; S->pState = pState; S->M = M;
  if (pState) zero_words(pState, sizeof(T) * ((size_t)numTaps + blockSize - 1), "arm_fir_decimate_init");
  return ARM_MATH_SUCCESS;
}
template <typename T, typename Inst>
arm_status interpolate_init(Inst* S, uint8_t L, uint16_t numTaps, const T* pCoeffs, T* pState, uint32_t blockSize) {
  if (!S) return ARM_MATH_ARGUMENT_ERROR;
  if (L == 0 || numTaps % L) return ARM_MATH_LENGTH_ERROR;         // arm_fir_interpolate_init_f32.c
  S->pCoeffs = pCoeffs; S->L = L; S->phaseLength = (uint16_t)(numTaps / L); S->pState = pState;
  if (pState) zero_words(pState, sizeof(T) * ((size_t)blockSize + S->phaseLength - 1), "arm_fir_interpolate_init");
  return ARM_MATH_SUCCESS;
}
template <typename T, typename Inst>
void decimate_sync(const Inst* S, const T* pSrc, T* pDst, uint32_t B, int op, const char* what) {
  if (!S || S->M == 0 || S->numTaps == 0 || !S->pState || !S->pCoeffs || B == 0) return;
  const int M = S->M, taps = S->numTaps;
  filter_sync(S->pCoeffs, taps, S->pState, sizeof(T) * (size_t)(taps - 1), pSrc, sizeof(T) * (size_t)B, pDst,
              sizeof(T) * (size_t)(B / M), true, what,
              [&](const T* dc, const T* src, T* dst, T* hist, hipStream_t st) {
                return fir_decimate_run(op, dc, taps, M, src, dst, B, 1, hist, st);
              });
}
template <typename T, typename Inst>
void interpolate_sync(const Inst* S, const T* pSrc, T* pDst, uint32_t B, int op, const char* what) {
  if (!S || S->L == 0 || S->phaseLength == 0 || !S->pState || !S->pCoeffs || B == 0) return;
  const int L = S->L, P = S->phaseLength;
  filter_sync(S->pCoeffs, L * P, S->pState, sizeof(T) * (size_t)(P - 1), pSrc, sizeof(T) * (size_t)B, pDst,
              sizeof(T) * (size_t)B * L, true, what,
              [&](const T* dc, const T* src, T* dst, T* hist, hipStream_t st) {
                return fir_interpolate_run(op, dc, L, P, src, dst, B, 1, hist, st);
              });
}
template <typename T, typename Inst>
arm_status decimate_batch(const Inst* S, const T* d_src, T* d_dst, uint32_t B, uint32_t batch, T* d_hist,
                          void* stream, int op, const char* what) {
  if (!S || !S->pCoeffs || S->numTaps == 0 || S->M == 0) return ARM_MATH_ARGUMENT_ERROR;
  if (batch && B && (!d_src || (B >= S->M && !d_dst) || (S->numTaps > 1 && !d_hist))) return ARM_MATH_ARGUMENT_ERROR;
  BlobScope hold((hipStream_t)stream);
  const T* dc = device_coeffs<T>(S->pCoeffs, S->numTaps, what);
  if (!dc) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(fir_decimate_run(op, dc, S->numTaps, S->M, d_src, d_dst, B, batch, d_hist, (hipStream_t)stream),
                      what);
}
template <typename T, typename Inst>
arm_status interpolate_batch(const Inst* S, const T* d_src, T* d_dst, uint32_t B, uint32_t batch, T* d_hist,
                             void* stream, int op, const char* what) {
  if (!S || !S->pCoeffs || S->phaseLength == 0 || S->L == 0) return ARM_MATH_ARGUMENT_ERROR;
  if (batch && B && (!d_src || !d_dst || (S->phaseLength > 1 && !d_hist))) return ARM_MATH_ARGUMENT_ERROR;
  BlobScope hold((hipStream_t)stream);
  const T* dc = device_coeffs<T>(S->pCoeffs, (int)S->L * S->phaseLength, what);
  if (!dc) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(fir_interpolate_run(op, dc, S->L, S->phaseLength, d_src, d_dst, B, batch, d_hist,
                                          (hipStream_t)stream),
                      what);
}

// ---- sparse FIR ---------------------------------------------------------------------------
// Drop-in: the reference's circular state (L = maxDelay + blockSize words, host or device) gets
// the block at stateIndex (arm_circularWrite_f32), then one kernel reads every tap straight from
// it at the reference's read indices (arm_fir_sparse_f32.c); pScratchIn / pScratchOut are not
// needed.  Host state + host input: the block is written into the caller's state on the host and
// the state uploaded once (the kernel never modifies it).
template <typename T, typename Inst>
void sparse_init(Inst* S, uint16_t numTaps, const T* pCoeffs, T* pState, int32_t* pTapDelay, uint16_t maxDelay,
                 uint32_t blockSize) {
  if (!S) return;
  S->numTaps = numTaps; S->pCoeffs = pCoeffs; S->pTapDelay = pTapDelay; S->maxDelay = maxDelay;
  S->stateIndex = 0;                                                  // arm_fir_sparse_init_f32.c
  if (pState) zero_words(pState, sizeof(T) * ((size_t)maxDelay + blockSize), "arm_fir_sparse_init");
  S->pState = pState;
}

template <typename T, typename Inst>
void sparse_sync(Inst* S, const T* pSrc, T* pDst, uint32_t B, int op, const char* what) {
  if (!S || !S->pState || !S->pCoeffs || !S->pTapDelay || S->numTaps == 0 || B == 0) return;
  const int taps = S->numTaps;
  const uint32_t L = (uint32_t)S->maxDelay + B;
  hipStream_t st = sync_stream();
  BlobScope hold(st);
  const T* dc = device_coeffs<T>(S->pCoeffs, taps, what);
  const int32_t* dd = device_coeffs<int32_t>(S->pTapDelay, taps, what);
  if (!dc || !dd) return;
  const bool dstate = is_device_ptr(S->pState), dsrc = is_device_ptr(pSrc), ddst = is_device_ptr(pDst);
  // words moved: the circular length, or up to a stateIndex a larger earlier block left past it
  const size_t es = sizeof(T), sb = es * B, lb = es * std::max<size_t>(L, (size_t)S->stateIndex + 1);
  T* ds = dstate ? S->pState : (T*)scratch(lb + 16, 2);
  // a device output overlapping the state would be read by later taps: write to scratch
  const bool dalias = ddst && dstate && ranges_overlap(pDst, S->pState, lb > sb ? lb : sb);
  T* dds = (ddst && !dalias) ? pDst : (T*)scratch(sb + 16, 4);
  if (!ds || !dds) { set_error(hipErrorOutOfMemory, what); return; }
  // arm_circularWrite_f32 position by position: sample i at w, then w + 1 wrapped once at L
  // (a stateIndex left >= L by a larger earlier blockSize writes there first, as the reference
  // does), as contiguous segments
  auto circular_write = [&](auto&& copy) -> hipError_t {
    int64_t w = S->stateIndex;
    for (uint32_t i = 0; i < B;) {
      const uint32_t n = w >= (int64_t)L ? 1u : (B - i < L - (uint32_t)w ? B - i : L - (uint32_t)w);
      hipError_t e = copy((size_t)w, i, n);
      if (e != hipSuccess) return e;
      i += n;
      w += n;
      if (w >= (int64_t)L) w -= L;
    }
    S->stateIndex = (uint16_t)w;
    return hipSuccess;
  };
  const uint16_t prev = S->stateIndex;
  HostIO io(st);
  hipError_t e = hipSuccess;
  if (!dstate && !dsrc) {
    e = circular_write([&](size_t w, uint32_t i, uint32_t n) {
      memcpy(S->pState + w, pSrc + i, es * n);
      return hipSuccess;
    });
    if (e == hipSuccess) e = io.in(ds, S->pState, lb);
  } else {
    if (!dstate) e = io.in(ds, S->pState, lb);
    if (e == hipSuccess)
      e = circular_write([&](size_t w, uint32_t i, uint32_t n) {
        return dsrc ? hipMemcpyAsync(ds + w, pSrc + i, es * n, hipMemcpyDeviceToDevice, st) : io.in(ds + w, pSrc + i, es * n);
      });
  }
  const uint16_t next = S->stateIndex;
  S->stateIndex = prev;                                               // committed on success
  const int r0 = (int32_t)((uint32_t)next - B);                       // arm_fir_sparse_f32.c readIndex
  if (e == hipSuccess) e = fir_sparse_run(op, dc, dd, taps, S->maxDelay, ds, dds, B, 1, nullptr, (int)L, r0, st);
  if (e == hipSuccess && dalias) e = hipMemcpyAsync(pDst, dds, sb, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && !ddst) e = io.out(pDst, dds, sb);
  if (e == hipSuccess && !dstate && dsrc) e = io.out(S->pState, ds, lb);
  if (e == hipSuccess) e = io.finish();
  if (e != hipSuccess) { set_error(e, what); return; }
  S->stateIndex = next;
}

// Batched: `batch` streams with linear histories d_hist[batch][maxDelay] (oldest first,
// updated), delays in [0, maxDelay] (others read 0); stateIndex / pState are not used.
template <typename T, typename Inst>
arm_status sparse_batch(const Inst* S, const T* d_src, T* d_dst, uint32_t B, uint32_t batch, T* d_hist, void* stream,
                        int op, const char* what) {
  if (!S || !S->pCoeffs || !S->pTapDelay || S->numTaps == 0) return ARM_MATH_ARGUMENT_ERROR;
  if (batch && B && (!d_src || !d_dst || (S->maxDelay > 0 && !d_hist))) return ARM_MATH_ARGUMENT_ERROR;
  BlobScope hold((hipStream_t)stream);
  const T* dc = device_coeffs<T>(S->pCoeffs, S->numTaps, what);
  const int32_t* dd = device_coeffs<int32_t>(S->pTapDelay, S->numTaps, what);
  if (!dc || !dd) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(fir_sparse_run(op, dc, dd, S->numTaps, S->maxDelay, d_src, d_dst, B, batch, d_hist, 0, 0,
                                     (hipStream_t)stream),
                      what);
}

// ---- FIR lattice ----------------------------------------------------------------------------
// Drop-in: state (numStages words, host or device) in, filter, state out (arm_fir_lattice_f32.c);
// the kernel reads the old state from its own copy, so in-place device state is fine.
template <typename T, typename Inst>
void lattice_init(Inst* S, uint16_t numStages, const T* pCoeffs, T* pState) {
  if (!S) return;
  S->numStages = numStages; S->pCoeffs = pCoeffs; S->pState = pState;     // arm_fir_lattice_init_f32.c
  if (pState && numStages) zero_words(pState, sizeof(T) * numStages, "arm_fir_lattice_init");
}

template <typename T, typename Inst>
void lattice_sync(const Inst* S, const T* pSrc, T* pDst, uint32_t B, int op, const char* what) {
  if (!S || !S->pState || !S->pCoeffs || S->numStages == 0 || B == 0) return;
  const int M = S->numStages;
  const size_t sb = sizeof(T) * (size_t)B;
  filter_sync(S->pCoeffs, M, S->pState, sizeof(T) * (size_t)M, pSrc, sb, pDst, sb, false, what,
              [&](const T* dc, const T* src, T* dst, T* state, hipStream_t st) {
                return fir_lattice_run(op, dc, M, src, dst, B, 1, state, st);
              });
}

template <typename T, typename Inst>
arm_status lattice_batch(const Inst* S, const T* d_src, T* d_dst, uint32_t B, uint32_t batch, T* d_state,
                         void* stream, int op, const char* what) {
  if (!S || !S->pCoeffs || S->numStages == 0) return ARM_MATH_ARGUMENT_ERROR;
  if (batch && B && (!d_src || !d_dst || !d_state)) return ARM_MATH_ARGUMENT_ERROR;
  BlobScope hold((hipStream_t)stream);
  const T* dc = device_coeffs<T>(S->pCoeffs, S->numStages, what);
  if (!dc) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(fir_lattice_run(op, dc, S->numStages, d_src, d_dst, B, batch, d_state, (hipStream_t)stream), what);
}

// ---- biquad cascades ------------------------------------------------------------------------
// ks state words (of ST) and nc coefficients per stage, ch interleaved channels (biquad.hip).  Drop-in:
// state (host or device) in, filter, state out, as lattice_sync; the inits zero the state as
// arm_biquad_cascade_*_init_*.c do.
template <typename ST, typename Inst, typename CT>
void biquad_init(Inst* S, uint8_t numStages, const CT* pCoeffs, ST* pState, int ks, const char* what) {
  if (!S) return;
  S->numStages = numStages; S->pCoeffs = pCoeffs; S->pState = pState;
  if (pState && numStages) zero_words(pState, sizeof(ST) * (size_t)ks * numStages, what);
}

template <typename T, typename ST, typename Inst>
void biquad_sync(const Inst* S, int ps, const T* pSrc, T* pDst, uint32_t B, int op, int ch, int ks, int nc,
                 const char* what) {
  if (!S || !S->pState || !S->pCoeffs || !pSrc || !pDst || S->numStages <= 0 || B == 0) return;
  const uint32_t M = (uint32_t)S->numStages;
  const size_t sb = sizeof(T) * (size_t)B * ch;
  filter_sync(S->pCoeffs, (int)(M * nc), S->pState, sizeof(ST) * (size_t)M * ks, pSrc, sb, pDst, sb, false, what,
              [&](const T* dc, const T* src, T* dst, ST* state, hipStream_t st) {
                return biquad_run(op, dc, M, ps, src, dst, B, 1, state, st);
              });
}

template <typename T, typename ST, typename Inst>
arm_status biquad_batch(const Inst* S, int ps, const T* d_src, T* d_dst, uint32_t B, uint32_t batch, ST* d_state,
                        void* stream, int op, int nc, const char* what) {
  if (!S || !S->pCoeffs || S->numStages <= 0 || !d_src || !d_dst || !d_state) return ARM_MATH_ARGUMENT_ERROR;
  if (!batch || !B) return ARM_MATH_SUCCESS;
  const uint32_t M = (uint32_t)S->numStages;
  BlobScope hold((hipStream_t)stream);
  const T* dc = device_coeffs<T>(S->pCoeffs, (int)(M * nc), what);
  if (!dc) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(biquad_run(op, dc, M, ps, d_src, d_dst, B, batch, d_state, (hipStream_t)stream), what);
}

// ---- IIR lattice ----------------------------------------------------------------------------
// Drop-in: the live state (the first numStages words of pState, host or device) in, filter, state out,
// as lattice_sync, with a second coefficient set; the reference's blockSize scratch words that follow
// are not touched.  The inits zero numStages + blockSize words (arm_iir_lattice_init_f32.c).
template <typename T, typename Inst>
void iir_lattice_init(Inst* S, uint16_t numStages, T* pkCoeffs, T* pvCoeffs, T* pState, uint32_t blockSize) {
  if (!S) return;
  S->numStages = numStages; S->pkCoeffs = pkCoeffs; S->pvCoeffs = pvCoeffs; S->pState = pState;
  const size_t words = (size_t)numStages + blockSize;
  if (pState && words) zero_words(pState, sizeof(T) * words, "arm_iir_lattice_init");
}

template <typename T, typename Inst>
void iir_lattice_sync(const Inst* S, const T* pSrc, T* pDst, uint32_t B, int op, const char* what) {
  if (!S || B == 0) return;
  if (!S->pState || !S->pkCoeffs || !S->pvCoeffs || !pSrc || !pDst || S->numStages == 0) {
    set_error(hipErrorInvalidValue, what);
    return;
  }
  const int N = S->numStages;
  const size_t sb = sizeof(T) * (size_t)B;
  FilterCall<T> c(S->pkCoeffs, N, S->pState, pSrc, pDst, what);
  const T* dv = c.dc ? device_coeffs<T>(S->pvCoeffs, N + 1, what) : nullptr;
  if (!dv) return;
  filter_sync(c, S->pState, sizeof(T) * (size_t)N, pSrc, sb, pDst, sb, false, what,
              [&](const T* dk, const T* src, T* dst, T* state, hipStream_t st) {
                return iir_lattice_run(op, dk, dv, N, src, dst, B, 1, state, st);
              });
}

template <typename T, typename Inst>
arm_status iir_lattice_batch(const Inst* S, const T* d_src, T* d_dst, uint32_t B, uint32_t batch, T* d_state,
                             void* stream, int op, const char* what) {
  if (!S || !S->pkCoeffs || !S->pvCoeffs || S->numStages == 0 || !d_src || !d_dst || !d_state)
    return ARM_MATH_ARGUMENT_ERROR;
  if (!batch || !B) return ARM_MATH_SUCCESS;
  BlobScope hold((hipStream_t)stream);
  const T* dk = device_coeffs<T>(S->pkCoeffs, S->numStages, what);
  const T* dv = dk ? device_coeffs<T>(S->pvCoeffs, S->numStages + 1, what) : nullptr;
  if (!dv) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(iir_lattice_run(op, dk, dv, S->numStages, d_src, d_dst, B, batch, d_state, (hipStream_t)stream),
                      what);
}

// ---- LMS / normalised LMS -----------------------------------------------------------------
// What a call needs from its instance: the kernel's op, the scalars as the kernel takes them and, for
// the q15 normalised kind, the reciprocal table.  ok: the reference's shift counts stay in 0...31.
struct LmsParams {
  int op;
  bool norm;
  int taps;
  int32_t mu, post_shift;
  const q15_t* recip;
  bool ok;
};
int32_t f32_bits(float32_t v) { int32_t b; memcpy(&b, &v, 4); return b; }
extern "C" const int16_t armRecipTableQ15[64];
LmsParams lms_params(const arm_lms_instance_f32* S) { return {kLmsF32, false, S->numTaps, f32_bits(S->mu), 0, nullptr, true}; }
LmsParams lms_params(const arm_lms_instance_q31* S) {
  return {kLmsQ31, false, S->numTaps, S->mu, (int32_t)S->postShift, nullptr, S->postShift <= 30};
}
LmsParams lms_params(const arm_lms_instance_q15* S) {
  return {kLmsQ15, false, S->numTaps, S->mu, (int32_t)S->postShift, nullptr, S->postShift <= 14};
}
LmsParams lms_params(const arm_lms_norm_instance_f32* S) {
  return {kLmsF32, true, S->numTaps, f32_bits(S->mu), 0, nullptr, true};
}
LmsParams lms_params(const arm_lms_norm_instance_q15* S) {
  return {kLmsQ15, true, S->numTaps, S->mu, S->postShift, S->recipTable ? S->recipTable : armRecipTableQ15,
          S->postShift <= 14};
}

// The inits set the fields and zero numTaps + blockSize - 1 state words (arm_lms_init_f32.c).
template <typename T, typename Inst>
void lms_init(Inst* S, uint16_t numTaps, T* pCoeffs, T* pState, T mu, uint32_t blockSize) {
  S->numTaps = numTaps; S->pCoeffs = pCoeffs; S->pState = pState; S->mu = mu;
  const size_t words = (size_t)numTaps + blockSize - 1;      // numTaps = blockSize = 0: none
  if (pState && (numTaps || blockSize) && words) zero_words(pState, sizeof(T) * words, "arm_lms_init");
}

// Drop-in staging of the adaptive shape: two inputs (pSrc, pRef), two outputs (pOut, pErr), and the
// coefficients, the history (the first numTaps - 1 words of pState) and, normalised, {energy, x0} both
// in and out.  Every buffer lies on the host or the device; host ones go through scratch slots 2...8.
// ex: the instance's {energy, x0} words, or nullptr.
template <typename T>
void adaptive_sync(const LmsParams& p, T* pCoeffs, T* pState, const T* pSrc, const T* pRef, T* pOut, T* pErr, uint32_t B,
                   T* ex, const char* what) {
  if (B == 0) return;
  if (!pCoeffs || !pSrc || !pRef || !pOut || !pErr || p.taps == 0 || (p.taps > 1 && !pState) || !p.ok) {
    set_error(hipErrorInvalidValue, what);
    return;
  }
  hipStream_t st = sync_stream();
  BlobScope hold(st);
  const int16_t* drecip = nullptr;
  if (p.recip) {
    drecip = device_coeffs<int16_t>(p.recip, 64, what);
    if (!drecip) return;
  }
  const size_t sb = sizeof(T) * (size_t)B, cb = sizeof(T) * (size_t)p.taps, hb = cb - sizeof(T), eb = 2 * sizeof(T);
  const bool dco = is_device_ptr(pCoeffs), dst8 = hb && is_device_ptr(pState), dsrc = is_device_ptr(pSrc),
             dref = is_device_ptr(pRef), dout = is_device_ptr(pOut), derr = is_device_ptr(pErr);
  T* dc = dco ? pCoeffs : (T*)scratch(cb + 16, 2);
  T* dh = (dst8 || !hb) ? pState : (T*)scratch(hb + 16, 3);
  const T* dx = dsrc ? pSrc : (const T*)scratch(sb + 16, 4);
  const T* dr = dref ? pRef : (const T*)scratch(sb + 16, 5);
  T* dy = dout ? pOut : (T*)scratch(sb + 16, 6);
  T* de = derr ? pErr : (T*)scratch(sb + 16, 7);
  T* dex = ex ? (T*)scratch(eb + 16, 8) : nullptr;
  if (!dc || (hb && !dh) || !dx || !dr || !dy || !de || (ex && !dex)) { set_error(hipErrorOutOfMemory, what); return; }
  HostIO io(st);
  hipError_t e = hipSuccess;
  if (!dco) e = io.in(dc, pCoeffs, cb);
  if (e == hipSuccess && hb && !dst8) e = io.in(dh, pState, hb);
  if (e == hipSuccess && !dsrc) e = io.in((void*)dx, pSrc, sb);
  if (e == hipSuccess && !dref) e = io.in((void*)dr, pRef, sb);
  if (e == hipSuccess && ex) e = io.in(dex, ex, eb);
  if (e == hipSuccess)
    e = lms_run(p.op, p.norm, dx, dr, dy, de, B, 1, p.taps, dc, hb ? dh : nullptr, dex, p.mu, p.post_shift, drecip, st);
  if (e == hipSuccess && !dout) e = io.out(pOut, dy, sb);
  if (e == hipSuccess && !derr) e = io.out(pErr, de, sb);
  if (e == hipSuccess && !dco) e = io.out(pCoeffs, dc, cb);
  if (e == hipSuccess && hb && !dst8) e = io.out(pState, dh, hb);
  if (e == hipSuccess && ex) e = io.out(ex, dex, eb);
  if (e == hipSuccess) e = io.finish();
  if (e == hipSuccess) hold.synced();
  if (e != hipSuccess) set_error(e, what);
}

template <typename T>
arm_status adaptive_batch(const LmsParams& p, const T* d_src, const T* d_ref, T* d_out, T* d_err, uint32_t B,
                          uint32_t batch, T* d_coeffs, T* d_state, T* d_ex, void* stream, const char* what) {
  if (p.taps == 0 || !p.ok || !d_src || !d_ref || !d_out || !d_err || !d_coeffs || (p.taps > 1 && !d_state) ||
      (p.norm && !d_ex))
    return ARM_MATH_ARGUMENT_ERROR;
  if (!batch || !B) return ARM_MATH_SUCCESS;
  BlobScope hold((hipStream_t)stream);
  const int16_t* drecip = nullptr;
  if (p.recip) {
    drecip = device_coeffs<int16_t>(p.recip, 64, what);
    if (!drecip) return ARM_MATH_ARGUMENT_ERROR;
  }
  return batch_status(lms_run(p.op, p.norm, d_src, d_ref, d_out, d_err, B, batch, p.taps, d_coeffs, d_state, d_ex, p.mu,
                              p.post_shift, drecip, (hipStream_t)stream),
                      what);
}

// ---- convolution / correlation family ------------------------------------------------
// How each reference function maps onto one ConvJob (conv.hip):
//   conv (exact):      x = pSrcA, h = pSrcB, all srcALen + srcBLen - 1 outputs forward;
//   conv (fast q15/q31): x = the longer input (arm_conv_fast_q15.c:83-103);
//   conv_partial:      outputs [firstIndex, firstIndex + numPoints) at pDst[n];
//   correlate (all):   x = the longer input, h = the shorter reversed; forward at
//                      srcALen - srcBLen, or backward from srcALen + srcBLen - 2 when
//                      srcALen < srcBLen (arm_correlate_f32.c:1040-1070).
// Returns the job and the written output range [wlo, whi) of one item.
enum ConvVariant { kVarConv = 0, kVarPartial = 1, kVarCorr = 2 };
ConvJob conv_plan(int op, int variant, const void* a, uint32_t alen, const void* b, uint32_t blen, uint32_t first,
                  uint32_t num, uint64_t* wlo, uint64_t* whi, bool* swapped) {
  ConvJob j{};
  j.op = op;
  j.corr = variant == kVarCorr;
  const bool swap = (variant == kVarCorr || op == kConvFastQ15 || op == kConvFastQ31) && alen < blen;
  *swapped = swap;
  j.x = swap ? b : a; j.A = swap ? blen : alen;
  j.h = swap ? a : b; j.B = swap ? alen : blen;
  const uint32_t L = alen + blen - 1;
  j.ydir = 1; j.yoff = 0; j.first = 0; j.num = L;
  *wlo = 0; *whi = L;
  if (variant == kVarPartial) {
    j.first = first; j.num = num;
    *wlo = first; *whi = (uint64_t)first + num;
  } else if (variant == kVarCorr) {
    if (alen >= blen) { j.yoff = alen - blen; *wlo = alen - blen; *whi = (uint64_t)j.yoff + L; }
    else { j.yoff = L - 1; j.ydir = -1; }
  }
  return j;
}

// drop-in: host or device operands, synchronous
template <typename T>
void conv_family_sync(int op, int variant, const T* a, uint32_t alen, const T* b, uint32_t blen, T* dst,
                      uint32_t first, uint32_t num, const char* what) {
  if (!a || !b || !dst || alen == 0 || blen == 0) return;
  uint64_t wlo, whi;
  bool swapped = false;
  ConvJob j = conv_plan(op, variant, a, alen, b, blen, first, num, &wlo, &whi, &swapped);
  if (j.num == 0) return;
  const size_t ab = sizeof(T) * alen, bb = sizeof(T) * blen;
  hipStream_t st = sync_stream();
  const bool da = is_device_ptr(a), db = is_device_ptr(b), dd = is_device_ptr(dst);
  const T* A = da ? a : (const T*)scratch(ab, 0);
  const T* B = db ? b : (const T*)scratch(bb, 1);
  T* Y = dd ? dst : (T*)scratch(sizeof(T) * whi, 2);
  if (!A || !B || !Y) { set_error(hipErrorOutOfMemory, what); return; }
  HostIO io(st);
  hipError_t e = hipSuccess;
  if (!da) e = io.in((void*)A, a, ab);
  if (e == hipSuccess && !db) e = io.in((void*)B, b, bb);
  j.x = swapped ? (const void*)B : (const void*)A;
  j.h = swapped ? (const void*)A : (const void*)B;
  j.y = Y; j.sx = j.sh = j.sy = 0; j.batch = 1;
  if (e == hipSuccess) e = conv_family_run(j, st);
  // only the words the reference writes are copied back (partial / correlate leave the rest)
  if (e == hipSuccess && !dd) e = io.out(dst + wlo, Y + wlo, sizeof(T) * (whi - wlo));
  if (e == hipSuccess) e = io.finish();
  if (e != hipSuccess) set_error(e, what);
}

// batched device API: item i reads a + i*sa, b + i*sb (0 = shared) and writes y + i*sy at
// the drop-in positions, except conv_partial, which writes its numPoints outputs compactly.
template <typename T>
arm_status conv_family_batch(int op, int variant, const T* a, uint32_t alen, uint32_t sa, const T* b, uint32_t blen,
                             uint32_t sb, T* y, uint32_t first, uint32_t num, uint32_t batch, void* stream,
                             const char* what) {
  if (batch && (!a || !b || !y || alen == 0 || blen == 0)) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  uint64_t wlo, whi;
  bool swapped = false;
  ConvJob j = conv_plan(op, variant, a, alen, b, blen, first, num, &wlo, &whi, &swapped);
  j.sx = swapped ? sb : sa;
  j.sh = swapped ? sa : sb;
  j.y = y; j.batch = batch;
  if (variant == kVarPartial) { j.sy = num; j.yoff = -(int64_t)first; }
  else if (variant == kVarCorr) j.sy = 2ull * (alen > blen ? alen : blen) - 1;
  else j.sy = (uint64_t)alen + blen - 1;
  return batch_status(conv_family_run(j, (hipStream_t)stream), what);
}

bool partial_range_ok(uint32_t alen, uint32_t blen, uint32_t first, uint32_t num) {
  // arm_conv_partial_f32.c:644: (firstIndex + numPoints) > (srcALen + (srcBLen - 1))
  return (uint64_t)first + num <= (uint64_t)alen + blen - 1;
}

template <typename M>
bool mat_shapes_ok(const M* a, const M* b, const M* c) {
  return a->numCols == b->numRows && a->numRows == c->numRows && b->numCols == c->numCols;
}

// multi-GPU matrix multiply: shard s = batch[s] matrices (shapes of the instances) at d_a[s],
// d_b[s], d_c[s] on devices[s].  launch(m, k, n, a, b, c, batch, st) is the per-type launcher.
template <typename T, typename M, typename Launch>
arm_status mat_batch_multi(const M* pSrcA, const M* pSrcB, M* pDst, uint32_t nshards, const int* devices,
                           const T* const* d_a, const T* const* d_b, T* const* d_c, const uint32_t* batch,
                           const char* what, Launch&& launch) {
  if (!pSrcA || !pSrcB || !pDst || (nshards && (!devices || !batch || !d_a || !d_b || !d_c))) return ARM_MATH_ARGUMENT_ERROR;
  if (!mat_shapes_ok(pSrcA, pSrcB, pDst)) return ARM_MATH_SIZE_MISMATCH;
  for (uint32_t s = 0; s < nshards; ++s)
    if (batch[s] && (!d_a[s] || !d_b[s] || !d_c[s])) return ARM_MATH_ARGUMENT_ERROR;
  return run_multi(nshards, devices, batch, what, [&](uint32_t s, hipStream_t st) {
    hipError_t e = launch(pSrcA->numRows, pSrcA->numCols, pSrcB->numCols, d_a[s], d_b[s], d_c[s], batch[s], st);
    if (e != hipSuccess) { set_error(e, what); return false; }
    return true;
  });
}

// drop-in matrix multiply (host or device operands), synchronous; launch as for mat_batch_multi.
// words: T words per element (2: interleaved complex).  bt (complex q15 only, host or device, may
// be null): receives B transposed, the n rows of k complex words that arm_mat_cmplx_mult_q15 leaves
// in pScratch.
template <typename T, typename M, typename Launch>
arm_status mat_mult_sync(const M* pSrcA, const M* pSrcB, M* pDst, const char* what, Launch&& launch, int words = 1,
                         T* bt = nullptr) {
  if (!pSrcA || !pSrcB || !pDst) return ARM_MATH_ARGUMENT_ERROR;
  if (!mat_shapes_ok(pSrcA, pSrcB, pDst)) return ARM_MATH_SIZE_MISMATCH;
  const int m = pSrcA->numRows, k = pSrcA->numCols, n = pSrcB->numCols;
  const size_t ab = sizeof(T) * (size_t)m * k * words, bb = sizeof(T) * (size_t)k * n * words,
               cb = sizeof(T) * (size_t)m * n * words;
  hipStream_t st = sync_stream();
  const bool da = is_device_ptr(pSrcA->pData), db = is_device_ptr(pSrcB->pData), dc = is_device_ptr(pDst->pData);
  T* A = da ? pSrcA->pData : (T*)scratch(ab + 16, 0);
  T* B = db ? pSrcB->pData : (T*)scratch(bb + 16, 1);
  T* Cd = dc ? pDst->pData : (T*)scratch(cb + 16, 2);
  if (!A || !B || !Cd) { set_error(hipErrorOutOfMemory, "arm_mat_mult scratch"); return ARM_MATH_ARGUMENT_ERROR; }
  HostIO io(st);
  hipError_t e = hipSuccess;
  if (!da) e = io.in(A, pSrcA->pData, ab);
  if (e == hipSuccess && !db) e = io.in(B, pSrcB->pData, bb);
  if (e == hipSuccess) e = launch(m, k, n, A, B, Cd, 1, st);
  if (e == hipSuccess && !dc) e = io.out(pDst->pData, Cd, cb);
  if constexpr (sizeof(T) == 2) {
    if (e == hipSuccess && bt && bb) {
      const bool dt = is_device_ptr(bt);
      T* Bt = dt ? bt : (T*)scratch(bb, 3);
      if (!Bt) e = hipErrorOutOfMemory;
      if (e == hipSuccess) e = mat_cmplx_trans_q15_launch(k, n, B, Bt, st);
      if (e == hipSuccess && !dt) e = io.out(bt, Bt, bb);
    }
  }
  if (e == hipSuccess) e = io.finish();
  return batch_status(e, what);
}

// batched device API: `batch` contiguous matrices at the instances' pData
template <typename M, typename Launch>
arm_status mat_batch(const M* pSrcA, const M* pSrcB, M* pDst, uint32_t batch, void* stream, const char* what,
                     Launch&& launch) {
  if (!pSrcA || !pSrcB || !pDst) return ARM_MATH_ARGUMENT_ERROR;
  if (!mat_shapes_ok(pSrcA, pSrcB, pDst)) return ARM_MATH_SIZE_MISMATCH;
  return batch_status(launch(pSrcA->numRows, pSrcA->numCols, pSrcB->numCols, pSrcA->pData, pSrcB->pData, pDst->pData,
                             batch, (hipStream_t)stream),
                      what);
}

// FIR init: zero numTaps + blockSize - 1 state words (arm_fir_init_f32.c:74-95,
// arm_fir_init_q15.c:119-139, the !ARM_MATH_DSP branch: no even-numTaps check).
// The state buffer is caller memory, host or device.
template <typename T, typename Inst>
void fir_init(Inst* S, uint16_t numTaps, const T* pCoeffs, T* pState, uint32_t blockSize) {
  S->numTaps = numTaps;
  S->pCoeffs = pCoeffs;
  S->pState = pState;
  if (pState) zero_words(pState, sizeof(T) * ((size_t)numTaps + blockSize - 1), "arm_fir_init");
}

// ---- MFCC drop-in and batched calls, f32 (Dev = MfccDev<float>) and q31 / q15 (MfccFxDev<T>) ----
// Drop-in: work space lives on the device; the reference's pSrc / pTmp work contents are not
// reproduced.
template <typename Dev, typename T, typename Inst>
arm_status mfcc_sync(const Inst* S, T* pSrc, T* pDst, const char* what) {
  if (!S || !pSrc || !pDst) return ARM_MATH_ARGUMENT_ERROR;
  if (S->nbDctOutputs == 0) return ARM_MATH_SUCCESS;
  hipStream_t st = sync_stream();
  BlobScope hold(st);
  Dev d;
  if (!mfcc_prepare(S, d)) return ARM_MATH_ARGUMENT_ERROR;
  const uint32_t n = S->fftLen, nd = S->nbDctOutputs;
  T* x = (T*)scratch(sizeof(T) * n, 0);
  T* y = (T*)scratch(sizeof(T) * 2 * n, 1);
  const bool ddst = is_device_ptr(pDst);
  T* o = ddst ? pDst : (T*)scratch(sizeof(T) * nd, 2);
  if (!x || !y || !o) { set_error(hipErrorOutOfMemory, what); return ARM_MATH_ARGUMENT_ERROR; }
  HostIO io(st);
  hipError_t e = is_device_ptr(pSrc) ? hipMemcpyAsync(x, pSrc, sizeof(T) * n, hipMemcpyDeviceToDevice, st)
                                     : io.in(x, pSrc, sizeof(T) * n);
  if (e != hipSuccess) { set_error(e, what); return ARM_MATH_ARGUMENT_ERROR; }
  if (!mfcc_run(S, d, x, y, o, 1, st)) { (void)hipStreamSynchronize(st); return ARM_MATH_ARGUMENT_ERROR; }
  if (!ddst) e = io.out(pDst, o, sizeof(T) * nd);
  if (e == hipSuccess) e = io.finish();
  return batch_status(e, what);
}

template <typename Dev, typename T, typename Inst>
arm_status mfcc_batch(const Inst* S, T* d_src, T* d_dst, T* d_tmp, uint32_t batch, void* stream) {
  if (!S || (batch && (!d_src || !d_dst || !d_tmp))) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0 || S->nbDctOutputs == 0) return ARM_MATH_SUCCESS;
  BlobScope hold((hipStream_t)stream);
  Dev d;
  if (!mfcc_prepare(S, d)) return ARM_MATH_ARGUMENT_ERROR;
  return mfcc_run(S, d, d_src, d_tmp, d_dst, batch, (hipStream_t)stream) ? ARM_MATH_SUCCESS : ARM_MATH_ARGUMENT_ERROR;
}
}  // namespace

// ---- inverse, Cholesky, LDLT, triangular solves (f32) ---------------------------------
// matrix_functions.h:659-777; kernels and the reference bodies they restate: mat_solve.hip.  The shape rules
// are those the reference states under ARM_MATH_MATRIX_CHECK, applied always (as mat_shapes_ok is), plus
// a / dst agreement in the solves.
namespace {
using MatF = arm_matrix_instance_f32;

// One operand of a synchronous drop-in call: host words are staged into device scratch (in) and copied
// back after the launch (out); a device pointer is used in place.
struct SolveBuf {
  void* p;
  size_t bytes;
  bool in, out;
  void* d = nullptr;
  bool dev = false;
};

// launch(st) -> hipError_t runs on the staged operands (bufs[i].d) between the copies in and out.
template <typename Launch>
arm_status mat_staged_sync(SolveBuf* bufs, int nb, const char* what, Launch&& launch) {
  hipStream_t st = sync_stream();
  for (int i = 0; i < nb; ++i) {
    SolveBuf& b = bufs[i];
    b.dev = is_device_ptr(b.p);
    b.d = b.dev ? b.p : scratch(b.bytes + 16, i);
    for (int j = 0; j < i; ++j)          // exact alias (add / sub / scale in place): one staged copy
      if (!b.dev && bufs[j].p == b.p && bufs[j].bytes == b.bytes) b.d = bufs[j].d;
    if (!b.d) { set_error(hipErrorOutOfMemory, what); return ARM_MATH_ARGUMENT_ERROR; }
  }
  HostIO io(st);
  hipError_t e = hipSuccess;
  for (int i = 0; i < nb && e == hipSuccess; ++i)
    if (!bufs[i].dev && bufs[i].in) e = io.in(bufs[i].d, bufs[i].p, bufs[i].bytes);
  if (e == hipSuccess) e = launch(st);
  for (int i = 0; i < nb && e == hipSuccess; ++i)
    if (!bufs[i].dev && bufs[i].out) e = io.out(bufs[i].p, bufs[i].d, bufs[i].bytes);
  if (e == hipSuccess) e = io.finish();
  return batch_status(e, what);
}

// launch(st, d_status) -> hipError_t runs one item on the staged operands; returns the item's status, which
// is staged out like one more operand.
template <typename Launch>
arm_status mat_solve_sync(SolveBuf* bufs, int nb, const char* what, Launch&& launch) {
  int32_t status = ARM_MATH_SUCCESS;
  SolveBuf all[5];
  for (int i = 0; i < nb; ++i) all[i] = bufs[i];
  all[nb] = {&status, sizeof(status), false, true};
  const arm_status r = mat_staged_sync(all, nb + 1, what, [&](hipStream_t st) {
    for (int i = 0; i < nb; ++i) bufs[i] = all[i];      // the callers' launches read bufs[i].d
    return launch(st, (int32_t*)all[nb].d);
  });
  return r != ARM_MATH_SUCCESS ? r : (arm_status)status;
}

bool square(const MatF* m) { return m->numRows == m->numCols; }

arm_status solve_tri_sync(bool lower, const MatF* t, const MatF* a, MatF* dst, const char* what) {
  if (!t || !a || !dst || !t->pData || !a->pData || !dst->pData) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(t) || t->numRows != a->numRows || a->numRows != dst->numRows || a->numCols != dst->numCols)
    return ARM_MATH_SIZE_MISMATCH;
  const int n = t->numRows, cols = a->numCols;
  if (n == 0 || cols == 0) return ARM_MATH_SUCCESS;
  // dst is staged in as well: a failing solve leaves most of its words alone
  SolveBuf b[3] = {{t->pData, sizeof(float) * n * n, true, false},
                   {a->pData, sizeof(float) * n * cols, true, false},
                   {dst->pData, sizeof(float) * n * cols, true, true}};
  return mat_solve_sync(b, 3, what, [&](hipStream_t st, int32_t* ds) {
    return mat_solve_tri_f32_launch(lower, n, cols, (const float*)b[0].d, (const float*)b[1].d, (float*)b[2].d, 1, ds,
                                    st);
  });
}

arm_status solve_tri_batch(bool lower, const MatF* t, const MatF* a, MatF* dst, uint32_t batch, int32_t* d_status,
                           void* stream, const char* what) {
  if (!t || !a || !dst) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(t) || t->numRows != a->numRows || a->numRows != dst->numRows || a->numCols != dst->numCols)
    return ARM_MATH_SIZE_MISMATCH;
  if (batch == 0 || t->numRows == 0 || a->numCols == 0) return ARM_MATH_SUCCESS;
  if (!t->pData || !a->pData || !dst->pData) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(mat_solve_tri_f32_launch(lower, t->numRows, a->numCols, t->pData, a->pData, dst->pData, batch,
                                               d_status, (hipStream_t)stream), what);
}

// ---- add / sub / scale, transposes, matrix x vector (mat_basic.hip) ------------------------------
// matrix_functions.h groups MatrixAdd, MatrixSub, MatrixScale, MatrixTrans, MatrixComplexTrans and the
// arm_mat_vec_mult_* of MatrixMult.  The shape rules are the reference's ARM_MATH_MATRIX_CHECK ones, applied
// always.  sync: the drop-in (operands staged as SolveBuf describes); otherwise the batched form on device
// pointers, which only enqueues.

template <typename M>
bool same_shape(const M* a, const M* b) { return a->numRows == b->numRows && a->numCols == b->numCols; }

// op: kMatAdd / kMatSub (b != null) or kMatScale (b == null, scale and shift used).
template <typename T, typename M>
arm_status mat_ew(int op, const M* a, const M* b, M* d, T scale, int32_t shift, bool sync, uint32_t batch,
                  void* stream, const char* what) {
  const bool two = op != kMatScale;
  if (!a || (two && !b) || !d) return ARM_MATH_ARGUMENT_ERROR;
  if (sync && (!a->pData || (two && !b->pData) || !d->pData)) return ARM_MATH_ARGUMENT_ERROR;
  if (!same_shape(a, d) || (two && !same_shape(a, b))) return ARM_MATH_SIZE_MISMATCH;
  if (op == kMatScale && !std::is_same<T, float>::value) {
    // past these the reference shifts by a negative or too large count
    const int lo = sizeof(T) == 4 ? -1 : -16, hi = sizeof(T) == 4 ? 30 : 15;
    if (shift < lo || shift > hi) return ARM_MATH_ARGUMENT_ERROR;
  }
  const size_t n = (size_t)a->numRows * a->numCols;
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  if (!sync) {
    if (!a->pData || (two && !b->pData) || !d->pData) return ARM_MATH_ARGUMENT_ERROR;
    return batch_status(mat_ew_launch<T>(op, (const T*)a->pData, two ? (const T*)b->pData : nullptr, (T*)d->pData,
                                         n * batch, scale, shift, (hipStream_t)stream), what);
  }
  SolveBuf bufs[3] = {{a->pData, sizeof(T) * n, true, false},
                      {d->pData, sizeof(T) * n, false, true},
                      {two ? b->pData : nullptr, sizeof(T) * n, true, false}};
  return mat_staged_sync(bufs, two ? 3 : 2, what, [&](hipStream_t st) {
    return mat_ew_launch<T>(op, (const T*)bufs[0].d, (const T*)bufs[2].d, (T*)bufs[1].d, n, scale, shift, st);
  });
}

// words: T words per element (2: interleaved complex).
template <typename T, typename M>
arm_status mat_trans(const M* s, M* d, int words, bool sync, uint32_t batch, void* stream, const char* what) {
  if (!s || !d) return ARM_MATH_ARGUMENT_ERROR;
  if (sync && (!s->pData || !d->pData)) return ARM_MATH_ARGUMENT_ERROR;
  if (s->numRows != d->numCols || s->numCols != d->numRows) return ARM_MATH_SIZE_MISMATCH;
  const size_t n = (size_t)s->numRows * s->numCols;
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  const int eb = (int)sizeof(T) * words;
  if (!sync) {
    if (!s->pData || !d->pData) return ARM_MATH_ARGUMENT_ERROR;
    return batch_status(mat_trans_launch(eb, s->numRows, s->numCols, s->pData, d->pData, batch, (hipStream_t)stream),
                        what);
  }
  SolveBuf bufs[2] = {{s->pData, eb * n, true, false}, {d->pData, eb * n, false, true}};
  return mat_staged_sync(bufs, 2, what, [&](hipStream_t st) {
    return mat_trans_launch(eb, s->numRows, s->numCols, bufs[0].d, bufs[1].d, 1, st);
  });
}

template <typename T, typename M>
arm_status mat_vec_mult_batch(const M* m, size_t matStride, const T* d_vec, T* d_dst, uint32_t batch, void* stream,
                              const char* what) {
  if (!m) return ARM_MATH_ARGUMENT_ERROR;
  if (matStride != 0 && matStride < (size_t)m->numRows * m->numCols) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0 || m->numRows == 0) return ARM_MATH_SUCCESS;
  if (!m->pData || !d_vec || !d_dst) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(mat_vec_mult_launch<T>(m->numRows, m->numCols, (const T*)m->pData, matStride, d_vec, d_dst,
                                             batch, (hipStream_t)stream), what);
}

template <typename T, typename M>
void mat_vec_mult_sync(const M* m, const T* pVec, T* pDst, const char* what) {
  if (!m || !m->pData || !pVec || !pDst) { set_error(hipErrorInvalidValue, what); return; }
  const size_t rows = m->numRows, cols = m->numCols;
  if (rows == 0) return;
  // numCols == 0: every sum is empty and the outputs are zero, as in the reference; no operand word is read
  SolveBuf bufs[3] = {{m->pData, sizeof(T) * rows * cols, cols != 0, false},
                      {const_cast<T*>(pVec), sizeof(T) * cols, cols != 0, false},
                      {pDst, sizeof(T) * rows, false, true}};
  mat_staged_sync(bufs, 3, what, [&](hipStream_t st) {
    return mat_vec_mult_launch<T>((int)rows, (int)cols, (const T*)bufs[0].d, 0, (const T*)bufs[1].d, (T*)bufs[2].d, 1,
                                  st);
  });
}
// ---- complex math, max / min (cmplx_math.hip) ---------------------------------------------------
// complex_math_functions.h and arm_max_* / arm_min_* of statistics_functions.h.  sync: the void drop-in (operands
// staged as SolveBuf describes, a failure only sets the last error); otherwise the batched form on device
// pointers, which only enqueues.  On device memory dst may be a source exactly where the kernel allows it
// (conj: the source; mult_cmplx: either source; mult_real: the complex source); any other overlap of an output
// with a source is refused.

bool cm_overlaps(const void* d, size_t db, const void* s, size_t sb, bool exactOk) {
  if (!db || !sb || !s) return false;
  if (d == s && db == sb && exactOk) return false;
  const uintptr_t d0 = (uintptr_t)d, s0 = (uintptr_t)s;
  return d0 < s0 + sb && s0 < d0 + db;
}

arm_status cm_null(bool sync, const char* what) {
  if (sync) set_error(hipErrorInvalidValue, what);
  return ARM_MATH_ARGUMENT_ERROR;
}

template <typename T>
arm_status cmplx_ew(int op, const T* a, const T* b, T* d, uint32_t n, bool sync, uint32_t batch, void* stream,
                    const char* what) {
  const int wb = op == kCmMultCmplx ? 2 : op == kCmMultReal ? 1 : 0;
  const int wd = op == kCmMag || op == kCmMagSquared || op == kCmMagFast ? 1 : 2;
  if (sync && (!a || (wb && !b) || !d)) return cm_null(true, what);
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  if (!a || (wb && !b) || !d) return ARM_MATH_ARGUMENT_ERROR;
  const size_t count = (size_t)n * batch;
  const bool lut = op == kCmMag && !std::is_same<T, float>::value;
  auto run = [&](const T* da, const T* db, T* dd, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dd, sizeof(T) * wd * count, da, sizeof(T) * 2 * count, wd == 2) ||
        cm_overlaps(dd, sizeof(T) * wd * count, db, sizeof(T) * wb * count, op == kCmMultCmplx))
      return hipErrorInvalidValue;
    const int32_t* dl = lut ? (const int32_t*)device_table(sqrt_initial_lut_q31, sizeof(int32_t) * 32) : nullptr;
    if (lut && !dl) return hipErrorOutOfMemory;
    return cmplx_ew_launch<T>(op, da, db, dd, count, dl, st);
  };
  if (!sync) return batch_status(run(a, b, d, (hipStream_t)stream), what);
  SolveBuf bufs[3] = {{const_cast<T*>(a), sizeof(T) * 2 * count, true, false},
                      {d, sizeof(T) * wd * count, false, true},
                      {const_cast<T*>(b), sizeof(T) * wb * count, true, false}};
  return mat_staged_sync(bufs, wb ? 3 : 2, what, [&](hipStream_t st) {
    return run((const T*)bufs[0].d, wb ? (const T*)bufs[2].d : nullptr, (T*)bufs[1].d, st);
  });
}

// bStride (complex samples; the drop-in passes n): 0 shares one b, otherwise >= n.
template <typename T, typename R>
arm_status cmplx_dot(const T* a, const T* b, uint32_t bStride, uint32_t n, R* re, R* im, bool sync, uint32_t batch,
                     void* stream, const char* what) {
  if (sync && (!a || !b || !re || !im)) return cm_null(true, what);
  if (bStride != 0 && bStride < n) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  if (!a || !b || !re || !im) return ARM_MATH_ARGUMENT_ERROR;
  const size_t ab = sizeof(T) * 2 * n * batch, ob = sizeof(R) * batch;
  const size_t bb = sizeof(T) * 2 * ((size_t)bStride * (batch - 1) + n);
  auto run = [&](const T* da, const T* db, R* dre, R* dim, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dre, ob, da, ab, false) || cm_overlaps(dre, ob, db, bb, false) ||
        cm_overlaps(dim, ob, da, ab, false) || cm_overlaps(dim, ob, db, bb, false) || cm_overlaps(dre, ob, dim, ob, false))
      return hipErrorInvalidValue;
    return cmplx_dot_launch<T, R>(da, db, bStride, n, dre, dim, batch, st);
  };
  if (!sync) return batch_status(run(a, b, re, im, (hipStream_t)stream), what);
  SolveBuf bufs[4] = {{const_cast<T*>(a), ab, n != 0, false}, {const_cast<T*>(b), bb, n != 0, false},
                      {re, ob, false, true}, {im, ob, false, true}};
  return mat_staged_sync(bufs, 4, what, [&](hipStream_t st) {
    return run((const T*)bufs[0].d, (const T*)bufs[1].d, (R*)bufs[2].d, (R*)bufs[3].d, st);
  });
}

template <typename T>
arm_status cm_search(bool max, const T* src, uint32_t n, T* result, uint32_t* index, bool sync, uint32_t batch,
                     void* stream, const char* what) {
  if (sync && (!src || !result || !index)) return cm_null(true, what);
  if (batch == 0) return ARM_MATH_SUCCESS;
  if (n == 0) return cm_null(sync, what);                  // the reference reads pSrc[0]
  if (!src || !result || !index) return ARM_MATH_ARGUMENT_ERROR;
  const size_t sb = sizeof(T) * n * batch, rb = sizeof(T) * batch, ib = sizeof(uint32_t) * batch;
  auto run = [&](const T* ds, T* dr, uint32_t* di, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dr, rb, ds, sb, false) || cm_overlaps(di, ib, ds, sb, false) || cm_overlaps(dr, rb, di, ib, false))
      return hipErrorInvalidValue;
    return search_launch<T>(max, ds, n, dr, di, batch, st);
  };
  if (!sync) return batch_status(run(src, result, index, (hipStream_t)stream), what);
  SolveBuf bufs[3] = {{const_cast<T*>(src), sb, true, false}, {result, rb, false, true}, {index, ib, false, true}};
  return mat_staged_sync(bufs, 3, what, [&](hipStream_t st) {
    return run((const T*)bufs[0].d, (T*)bufs[1].d, (uint32_t*)bufs[2].d, st);
  });
}

// ---- statistics (statistics.hip) ------------------------------------------------------------------
// The sums and level measures of statistics_functions.h (op: kStMean ... kStAccumulate; b: the second source of
// kStMse) and the abs / no-index searches.  sync and the overlap rule as above.  blockSize == 0: what the
// reference's empty sums give is stored (power, accumulate: 0; mean_f32, mse_f32: 0 / 0; rms_f32: +0.0; var, std:
// 0; max / min_no_idx_f32: their start value); where it would divide an integer by zero or read pSrc[0] the call
// is refused as cm_search refuses it.
template <typename T, typename R>
arm_status st_sum(int op, const T* a, const T* b, uint32_t n, R* result, bool sync, uint32_t batch, void* stream,
                  const char* what) {
  constexpr bool f32 = std::is_same<T, float>::value;
  const bool two = op == kStMse;
  if (sync && (!a || (two && !b) || !result)) return cm_null(true, what);
  if (batch == 0) return ARM_MATH_SUCCESS;
  if (n == 0 && !f32 && (op == kStMean || op == kStRms || op == kStMse)) return cm_null(sync, what);
  if (!a || (two && !b) || !result) return ARM_MATH_ARGUMENT_ERROR;
  const size_t sb = sizeof(T) * n * batch, rb = sizeof(R) * batch;
  const bool lut = std::is_same<T, int32_t>::value && (op == kStRms || op == kStStd);
  auto run = [&](const T* da, const T* db, R* dr, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dr, rb, da, sb, false) || (two && cm_overlaps(dr, rb, db, sb, false))) return hipErrorInvalidValue;
    const int32_t* dl = lut ? (const int32_t*)device_table(sqrt_initial_lut_q31, sizeof(int32_t) * 32) : nullptr;
    if (lut && !dl) return hipErrorOutOfMemory;
    return stat_sum_launch<T, R>(op, da, db, n, dr, batch, dl, st);
  };
  if (!sync) return batch_status(run(a, b, result, (hipStream_t)stream), what);
  SolveBuf bufs[3] = {{const_cast<T*>(a), sb, n != 0, false}, {result, rb, false, true},
                      {const_cast<T*>(b), sb, n != 0, false}};
  return mat_staged_sync(bufs, two ? 3 : 2, what, [&](hipStream_t st) {
    return run((const T*)bufs[0].d, two ? (const T*)bufs[2].d : nullptr, (R*)bufs[1].d, st);
  });
}

// idx false: the _no_idx forms (index unused).
template <typename T>
arm_status st_search(bool max, bool abs, bool idx, const T* src, uint32_t n, T* result, uint32_t* index, bool sync,
                     uint32_t batch, void* stream, const char* what) {
  if (sync && (!src || !result || (idx && !index))) return cm_null(true, what);
  if (batch == 0) return ARM_MATH_SUCCESS;
  const bool fromStart = std::is_same<T, float>::value && !abs && !idx;   // max / min_no_idx_f32 read no pSrc[0]
  if (n == 0 && !fromStart) return cm_null(sync, what);
  if (!src || !result || (idx && !index)) return ARM_MATH_ARGUMENT_ERROR;
  const size_t sb = sizeof(T) * n * batch, rb = sizeof(T) * batch, ib = idx ? sizeof(uint32_t) * batch : 0;
  auto run = [&](const T* ds, T* dr, uint32_t* di, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dr, rb, ds, sb, false) || cm_overlaps(di, ib, ds, sb, false) || cm_overlaps(dr, rb, di, ib, false))
      return hipErrorInvalidValue;
    return stat_search_launch<T>(max, abs, ds, n, dr, di, batch, st);
  };
  if (!sync) return batch_status(run(src, result, idx ? index : nullptr, (hipStream_t)stream), what);
  SolveBuf bufs[3] = {{const_cast<T*>(src), sb, n != 0, false}, {result, rb, false, true}, {index, ib, false, true}};
  return mat_staged_sync(bufs, idx ? 3 : 2, what, [&](hipStream_t st) {
    return run((const T*)bufs[0].d, (T*)bufs[1].d, idx ? (uint32_t*)bufs[2].d : nullptr, st);
  });
}

// ---- basic math (basic_math.hip; the dot products: statistics.hip) ---------------------------------
// basic_math_functions.h.  sync and the null / overlap rules as the complex-math functions: dst may be a source
// exactly, any other overlap of an output with a source is refused.  One scalar (offset, scale and shift, low and
// high) serves the whole call.  shift: the counts at which the reference's C is defined (a count below 32 either way
// on its promoted int operands): arm_shift_* -31 .. 31; arm_scale_q31 -32 .. 30 (kShift = shift + 1), _q15 -16 .. 15
// (kShift = 15 - shift in 0 .. 31), _q7 -24 .. 7 (kShift = 7 - shift); outside the call is refused.
bool bm_two(int op) { return op == kBmAdd || op == kBmSub || op == kBmMult || op == kBmAnd || op == kBmOr || op == kBmXor; }

template <typename T>
arm_status bm_ew(int op, const T* a, const T* b, T* d, uint32_t n, T s0, T s1, int shift, bool sync, uint32_t batch,
                 void* stream, const char* what) {
  const bool two = bm_two(op);
  if (sync && (!a || (two && !b) || !d)) return cm_null(true, what);
  int sh = 0;
  if (op == kBmShift) {
    if (shift < -31 || shift > 31) return cm_null(sync, what);
    sh = shift;
  } else if (op == kBmScale && !std::is_same<T, float>::value) {
    const int lo = sizeof(T) == 4 ? -32 : sizeof(T) == 2 ? -16 : -24, hi = sizeof(T) == 4 ? 30 : sizeof(T) == 2 ? 15 : 7;
    if (shift < lo || shift > hi) return cm_null(sync, what);
    sh = sizeof(T) == 4 ? shift + 1 : hi - shift;
  }
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  if (!a || (two && !b) || !d) return ARM_MATH_ARGUMENT_ERROR;
  const size_t count = (size_t)n * batch, bytes = sizeof(T) * count;
  auto run = [&](const T* da, const T* db, T* dd, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dd, bytes, da, bytes, true) || (two && cm_overlaps(dd, bytes, db, bytes, true)))
      return hipErrorInvalidValue;
    return basic_ew_launch<T>(op, da, db, dd, count, s0, s1, sh, st);
  };
  if (!sync) return batch_status(run(a, b, d, (hipStream_t)stream), what);
  SolveBuf bufs[3] = {{const_cast<T*>(a), bytes, true, false}, {d, bytes, false, true},
                      {const_cast<T*>(b), bytes, true, false}};
  return mat_staged_sync(bufs, two ? 3 : 2, what, [&](hipStream_t st) {
    return run((const T*)bufs[0].d, two ? (const T*)bufs[2].d : nullptr, (T*)bufs[1].d, st);
  });
}

// bStride (words; the drop-in passes n): 0 shares one b, otherwise >= n.  n == 0 stores zeros.
template <typename T, typename R>
arm_status bm_dot(const T* a, const T* b, uint32_t bStride, uint32_t n, R* result, bool sync, uint32_t batch,
                  void* stream, const char* what) {
  if (sync && (!a || !b || !result)) return cm_null(true, what);
  if (bStride != 0 && bStride < n) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  if (!a || !b || !result) return ARM_MATH_ARGUMENT_ERROR;
  const size_t ab = sizeof(T) * n * batch, rb = sizeof(R) * batch;
  const size_t bb = sizeof(T) * ((size_t)bStride * (batch - 1) + n);
  auto run = [&](const T* da, const T* db, R* dr, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dr, rb, da, ab, false) || cm_overlaps(dr, rb, db, bb, false)) return hipErrorInvalidValue;
    return dot_prod_launch<T, R>(da, db, bStride, n, dr, batch, st);
  };
  if (!sync) return batch_status(run(a, b, result, (hipStream_t)stream), what);
  SolveBuf bufs[3] = {{const_cast<T*>(a), ab, n != 0, false}, {const_cast<T*>(b), bb, n != 0, false},
                      {result, rb, false, true}};
  return mat_staged_sync(bufs, 3, what, [&](hipStream_t st) {
    return run((const T*)bufs[0].d, (const T*)bufs[1].d, (R*)bufs[2].d, st);
  });
}

// ---- support functions (support.hip, sort.hip; the weighted average: statistics.hip) --------------
// support_functions.h.  sync and the null / overlap rules as the basic math functions; dst may be src exactly where
// both element widths are equal (float_to_q31, q31_to_float, copy) and in the sorts.
template <typename S, typename D>
arm_status sp_convert(const S* s, D* d, uint32_t n, bool sync, uint32_t batch, void* stream, const char* what) {
  if (sync && (!s || !d)) return cm_null(true, what);
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  if (!s || !d) return ARM_MATH_ARGUMENT_ERROR;
  const size_t count = (size_t)n * batch, sb = sizeof(S) * count, db = sizeof(D) * count;
  auto run = [&](const S* ds, D* dd, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dd, db, ds, sb, sizeof(S) == sizeof(D))) return hipErrorInvalidValue;
    return support_convert_launch<S, D>(ds, dd, count, st);
  };
  if (!sync) return batch_status(run(s, d, (hipStream_t)stream), what);
  SolveBuf bufs[2] = {{const_cast<S*>(s), sb, true, false}, {d, db, false, true}};
  return mat_staged_sync(bufs, 2, what, [&](hipStream_t st) { return run((const S*)bufs[0].d, (D*)bufs[1].d, st); });
}

template <typename T>
arm_status sp_fill(T value, T* d, uint32_t n, bool sync, uint32_t batch, void* stream, const char* what) {
  if (sync && !d) return cm_null(true, what);
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  if (!d) return ARM_MATH_ARGUMENT_ERROR;
  const size_t count = (size_t)n * batch;
  if (!sync) return batch_status(support_fill_launch<T>(value, d, count, (hipStream_t)stream), what);
  SolveBuf bufs[1] = {{d, sizeof(T) * count, false, true}};
  return mat_staged_sync(bufs, 1, what,
                         [&](hipStream_t st) { return support_fill_launch<T>(value, (T*)bufs[0].d, count, st); });
}

// dir: ARM_SORT_DESCENDING (0) or ARM_SORT_ASCENDING (1), anything else is refused.
arm_status sp_sort(int dir, const float* src, float* dst, uint32_t n, bool sync, uint32_t batch, void* stream,
                   const char* what) {
  if (sync && (!src || !dst)) return cm_null(true, what);
  if ((dir != 0 && dir != 1) || n > 0x80000000u) return cm_null(sync, what);
  if (n == 0 || batch == 0) return ARM_MATH_SUCCESS;
  if (!src || !dst) return ARM_MATH_ARGUMENT_ERROR;
  const size_t bytes = sizeof(float) * n * batch;
  auto run = [&](const float* ds, float* dd, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dd, bytes, ds, bytes, true)) return hipErrorInvalidValue;
    return sort_launch((const uint32_t*)ds, (uint32_t*)dd, n, dir == 1, batch, st);
  };
  if (!sync) return batch_status(run(src, dst, (hipStream_t)stream), what);
  SolveBuf bufs[2] = {{const_cast<float*>(src), bytes, true, false}, {dst, bytes, false, true}};
  return mat_staged_sync(bufs, 2, what,
                         [&](hipStream_t st) { return run((const float*)bufs[0].d, (float*)bufs[1].d, st); });
}

// wStride (words; the drop-in passes n): 0 shares one weight vector, otherwise >= n.  n == 0 stores 0 / 0.
arm_status sp_wavg(const float* a, const float* w, uint32_t wStride, uint32_t n, float* result, bool sync,
                   uint32_t batch, void* stream, const char* what) {
  if (sync && (!a || !w || !result)) return cm_null(true, what);
  if (wStride != 0 && wStride < n) return cm_null(sync, what);
  if (batch == 0) return ARM_MATH_SUCCESS;
  if (!a || !w || !result) return ARM_MATH_ARGUMENT_ERROR;
  const size_t ab = sizeof(float) * n * batch, rb = sizeof(float) * batch;
  const size_t wb = sizeof(float) * ((size_t)wStride * (batch - 1) + n);
  auto run = [&](const float* da, const float* dw, float* dr, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dr, rb, da, ab, false) || cm_overlaps(dr, rb, dw, wb, false)) return hipErrorInvalidValue;
    return weighted_average_launch(da, dw, wStride, n, dr, batch, st);
  };
  if (!sync) return batch_status(run(a, w, result, (hipStream_t)stream), what);
  SolveBuf bufs[3] = {{const_cast<float*>(a), ab, n != 0, false}, {const_cast<float*>(w), wb, n != 0, false},
                      {result, rb, false, true}};
  return mat_staged_sync(bufs, 3, what, [&](hipStream_t st) {
    return run((const float*)bufs[0].d, (const float*)bufs[1].d, (float*)bufs[2].d, st);
  });
}

// wStride as sp_wavg against nbVectors.  vecDim == 0 writes nothing; nbVectors == 0 stores 0 / 0.
arm_status sp_barycenter(const float* in, const float* w, uint32_t wStride, float* out, uint32_t nv, uint32_t dim,
                         bool sync, uint32_t batch, void* stream, const char* what) {
  if (sync && (!in || !w || !out)) return cm_null(true, what);
  if (wStride != 0 && wStride < nv) return cm_null(sync, what);
  if (batch == 0 || dim == 0) return ARM_MATH_SUCCESS;
  if (!in || !w || !out) return ARM_MATH_ARGUMENT_ERROR;
  const size_t ib = sizeof(float) * nv * dim * batch, ob = sizeof(float) * dim * batch;
  const size_t wb = sizeof(float) * ((size_t)wStride * (batch - 1) + nv);
  auto run = [&](const float* di, const float* dw, float* dout, hipStream_t st) -> hipError_t {
    if (cm_overlaps(dout, ob, di, ib, false) || cm_overlaps(dout, ob, dw, wb, false)) return hipErrorInvalidValue;
    return barycenter_launch(di, dw, wStride, dout, nv, dim, batch, st);
  };
  if (!sync) return batch_status(run(in, w, out, (hipStream_t)stream), what);
  SolveBuf bufs[3] = {{const_cast<float*>(in), ib, nv != 0, false}, {const_cast<float*>(w), wb, nv != 0, false},
                      {out, ob, false, true}};
  return mat_staged_sync(bufs, 3, what, [&](hipStream_t st) {
    return run((const float*)bufs[0].d, (const float*)bufs[1].d, (float*)bufs[2].d, st);
  });
}
}  // namespace

extern "C" {

#ifndef MI355X_BUILD_DEFS
#define MI355X_BUILD_DEFS ""
#endif
#ifndef MI355X_SRC_ID
#define MI355X_SRC_ID "unknown"
#endif
// "src:" is the sha256-based id of the sources the library was built from (Makefile SRC_ID);
// "[...]" lists the non-default tuning macros of the build (Makefile DEFS, build_variant.sh)
const char* arm_mi355x_version(void) {
  return sizeof(MI355X_BUILD_DEFS) > 1 ? "cmsisdsp-mi355x 0.3.0 gfx950 src:" MI355X_SRC_ID " [" MI355X_BUILD_DEFS "]"
                                       : "cmsisdsp-mi355x 0.3.0 gfx950 src:" MI355X_SRC_ID;
}

void arm_cfft_f32(const arm_cfft_instance_f32* S, float32_t* p1, uint8_t ifftFlag, uint8_t bitReverseFlag) {
  cfft_sync(S, p1, ifftFlag, bitReverseFlag, 0, sizeof(float));
}
void arm_cfft_q31(const arm_cfft_instance_q31* S, q31_t* p1, uint8_t ifftFlag, uint8_t bitReverseFlag) {
  cfft_sync(S, p1, ifftFlag, bitReverseFlag, 1, sizeof(int32_t));
}
void arm_cfft_q15(const arm_cfft_instance_q15* S, q15_t* p1, uint8_t ifftFlag, uint8_t bitReverseFlag) {
  cfft_sync(S, p1, ifftFlag, bitReverseFlag, 2, sizeof(int16_t));
}

arm_status arm_cfft_f32_batch(const arm_cfft_instance_f32* S, float32_t* d_p1, uint32_t batch, uint8_t ifftFlag,
                              uint8_t bitReverseFlag, void* stream) {
  return cfft_batch(S, d_p1, batch, ifftFlag, bitReverseFlag, stream, 0);
}
arm_status arm_cfft_q31_batch(const arm_cfft_instance_q31* S, q31_t* d_p1, uint32_t batch, uint8_t ifftFlag,
                              uint8_t bitReverseFlag, void* stream) {
  return cfft_batch(S, d_p1, batch, ifftFlag, bitReverseFlag, stream, 1);
}
arm_status arm_cfft_q15_batch(const arm_cfft_instance_q15* S, q15_t* d_p1, uint32_t batch, uint8_t ifftFlag,
                              uint8_t bitReverseFlag, void* stream) {
  return cfft_batch(S, d_p1, batch, ifftFlag, bitReverseFlag, stream, 2);
}

arm_status arm_cfft_f32_batch_multi(const arm_cfft_instance_f32* S, uint32_t nshards, const int* devices,
                                    float32_t* const* d_p1, const uint32_t* batch, uint8_t ifftFlag,
                                    uint8_t bitReverseFlag) {
  return cfft_batch_multi(S, nshards, devices, (void* const*)d_p1, batch, ifftFlag, bitReverseFlag, 0);
}
arm_status arm_cfft_q31_batch_multi(const arm_cfft_instance_q31* S, uint32_t nshards, const int* devices,
                                    q31_t* const* d_p1, const uint32_t* batch, uint8_t ifftFlag,
                                    uint8_t bitReverseFlag) {
  return cfft_batch_multi(S, nshards, devices, (void* const*)d_p1, batch, ifftFlag, bitReverseFlag, 1);
}
arm_status arm_cfft_q15_batch_multi(const arm_cfft_instance_q15* S, uint32_t nshards, const int* devices,
                                    q15_t* const* d_p1, const uint32_t* batch, uint8_t ifftFlag,
                                    uint8_t bitReverseFlag) {
  return cfft_batch_multi(S, nshards, devices, (void* const*)d_p1, batch, ifftFlag, bitReverseFlag, 2);
}
int arm_mi355x_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

void arm_rfft_fast_f32(const arm_rfft_fast_instance_f32* S, float32_t* p, float32_t* pOut, uint8_t ifftFlag) {
  if (!S || !p || !pOut || !rfft_len_ok(S->fftLenRFFT)) return;
  const size_t bytes = sizeof(float) * S->fftLenRFFT;
  hipStream_t st = sync_stream();
  const bool dp = is_device_ptr(p), dout = is_device_ptr(pOut);
  float* d_p = dp ? p : (float*)scratch(bytes, 0);
  float* d_o = dout ? pOut : (float*)scratch(bytes, 1);
  if (!d_p || !d_o) { set_error(hipErrorOutOfMemory, "arm_rfft_fast scratch"); return; }
  HostIO io(st);
  hipError_t e = hipSuccess;
  if (!dp) e = io.in(d_p, p, bytes);
  if (e != hipSuccess) { set_error(e, "arm_rfft_fast"); return; }
  if (!rfft_run(S, d_p, d_o, 1, ifftFlag, st)) { (void)hipStreamSynchronize(st); return; }
  if (!dp && !ifftFlag) e = io.out(p, d_p, bytes);   // forward overwrites p
  if (e == hipSuccess && !dout) e = io.out(pOut, d_o, bytes);
  if (e == hipSuccess) e = io.finish();
  if (e != hipSuccess) set_error(e, "arm_rfft_fast");
}

arm_status arm_rfft_fast_f32_batch(const arm_rfft_fast_instance_f32* S, float32_t* d_p, float32_t* d_out,
                                   uint32_t batch, uint8_t ifftFlag, void* stream) {
  if (!S || !rfft_len_ok(S->fftLenRFFT) || (batch && (!d_p || !d_out))) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  return rfft_run(S, d_p, d_out, batch, ifftFlag, (hipStream_t)stream) ? ARM_MATH_SUCCESS : ARM_MATH_ARGUMENT_ERROR;
}
arm_status arm_rfft_fast_f32_batch_ex(const arm_rfft_fast_instance_f32* S, float32_t* d_p, float32_t* d_out,
                                      uint32_t batch, uint8_t ifftFlag, uint32_t flags, void* stream) {
  if (!S || !rfft_len_ok(S->fftLenRFFT) || (batch && (!d_p || !d_out))) return ARM_MATH_ARGUMENT_ERROR;
  if (flags & ~(uint32_t)ARM_MI355X_RFFT_P_SCRATCH) return ARM_MATH_ARGUMENT_ERROR;
  if (batch == 0) return ARM_MATH_SUCCESS;
  return rfft_run(S, d_p, d_out, batch, ifftFlag, (hipStream_t)stream, (flags & ARM_MI355X_RFFT_P_SCRATCH) != 0)
             ? ARM_MATH_SUCCESS
             : ARM_MATH_ARGUMENT_ERROR;
}

void arm_rfft_q31(const arm_rfft_instance_q31* S, q31_t* pSrc, q31_t* pDst) { rfft_fixed_sync<int32_t>(S, pSrc, pDst); }
void arm_rfft_q15(const arm_rfft_instance_q15* S, q15_t* pSrc, q15_t* pDst) { rfft_fixed_sync<int16_t>(S, pSrc, pDst); }
arm_status arm_rfft_q31_batch(const arm_rfft_instance_q31* S, q31_t* d_src, q31_t* d_dst, uint32_t batch,
                              void* stream) {
  return rfft_fixed_batch<int32_t>(S, d_src, d_dst, batch, stream);
}
arm_status arm_rfft_q15_batch(const arm_rfft_instance_q15* S, q15_t* d_src, q15_t* d_dst, uint32_t batch,
                              void* stream) {
  return rfft_fixed_batch<int16_t>(S, d_src, d_dst, batch, stream);
}

void arm_fir_init_f32(arm_fir_instance_f32* S, uint16_t numTaps, const float32_t* pCoeffs, float32_t* pState,
                      uint32_t blockSize) {
  if (S) fir_init<float>(S, numTaps, pCoeffs, pState, blockSize);
}
arm_status arm_fir_init_q15(arm_fir_instance_q15* S, uint16_t numTaps, const q15_t* pCoeffs, q15_t* pState,
                            uint32_t blockSize) {
  if (!S) return ARM_MATH_ARGUMENT_ERROR;
  fir_init<int16_t>(S, numTaps, pCoeffs, pState, blockSize);
  return ARM_MATH_SUCCESS;
}

void arm_fir_init_q31(arm_fir_instance_q31* S, uint16_t numTaps, const q31_t* pCoeffs, q31_t* pState,
                      uint32_t blockSize) {
  if (S) fir_init<int32_t>(S, numTaps, pCoeffs, pState, blockSize);
}

void arm_fir_init_q7(arm_fir_instance_q7* S, uint16_t numTaps, const q7_t* pCoeffs, q7_t* pState,
                     uint32_t blockSize) {
  if (S) fir_init<int8_t>(S, numTaps, pCoeffs, pState, blockSize);
}

void arm_fir_f32(const arm_fir_instance_f32* S, const float32_t* pSrc, float32_t* pDst, uint32_t blockSize) {
  fir_sync<float>(S, pSrc, pDst, blockSize, kFirF32);
}
void arm_fir_q7(const arm_fir_instance_q7* S, const q7_t* pSrc, q7_t* pDst, uint32_t blockSize) {
  fir_sync<int8_t>(S, pSrc, pDst, blockSize, kFirQ7);
}
void arm_fir_q15(const arm_fir_instance_q15* S, const q15_t* pSrc, q15_t* pDst, uint32_t blockSize) {
  fir_sync<int16_t>(S, pSrc, pDst, blockSize, kFirQ15);
}
void arm_fir_fast_q15(const arm_fir_instance_q15* S, const q15_t* pSrc, q15_t* pDst, uint32_t blockSize) {
  fir_sync<int16_t>(S, pSrc, pDst, blockSize, kFirFastQ15);
}
void arm_fir_q31(const arm_fir_instance_q31* S, const q31_t* pSrc, q31_t* pDst, uint32_t blockSize) {
  fir_sync<int32_t>(S, pSrc, pDst, blockSize, kFirQ31);
}
void arm_fir_fast_q31(const arm_fir_instance_q31* S, const q31_t* pSrc, q31_t* pDst, uint32_t blockSize) {
  fir_sync<int32_t>(S, pSrc, pDst, blockSize, kFirFastQ31);
}
arm_status arm_fir_f32_batch(const arm_fir_instance_f32* S, const float32_t* d_src, float32_t* d_dst,
                             uint32_t blockSize, uint32_t batch, float32_t* d_hist, void* stream) {
  return fir_batch<float>(S, d_src, d_dst, blockSize, batch, d_hist, stream, kFirF32);
}
arm_status arm_fir_f32_batch_fma(const arm_fir_instance_f32* S, const float32_t* d_src, float32_t* d_dst,
                                 uint32_t blockSize, uint32_t batch, float32_t* d_hist, void* stream) {
  return fir_batch<float>(S, d_src, d_dst, blockSize, batch, d_hist, stream, kFirF32Fma);
}
arm_status arm_fir_q15_batch(const arm_fir_instance_q15* S, const q15_t* d_src, q15_t* d_dst, uint32_t blockSize,
                             uint32_t batch, q15_t* d_hist, void* stream) {
  return fir_batch<int16_t>(S, d_src, d_dst, blockSize, batch, d_hist, stream, kFirQ15);
}
arm_status arm_fir_fast_q15_batch(const arm_fir_instance_q15* S, const q15_t* d_src, q15_t* d_dst, uint32_t blockSize,
                                  uint32_t batch, q15_t* d_hist, void* stream) {
  return fir_batch<int16_t>(S, d_src, d_dst, blockSize, batch, d_hist, stream, kFirFastQ15);
}
arm_status arm_fir_q31_batch(const arm_fir_instance_q31* S, const q31_t* d_src, q31_t* d_dst, uint32_t blockSize,
                             uint32_t batch, q31_t* d_hist, void* stream) {
  return fir_batch<int32_t>(S, d_src, d_dst, blockSize, batch, d_hist, stream, kFirQ31);
}
arm_status arm_fir_fast_q31_batch(const arm_fir_instance_q31* S, const q31_t* d_src, q31_t* d_dst, uint32_t blockSize,
                                  uint32_t batch, q31_t* d_hist, void* stream) {
  return fir_batch<int32_t>(S, d_src, d_dst, blockSize, batch, d_hist, stream, kFirFastQ31);
}
arm_status arm_fir_q7_batch(const arm_fir_instance_q7* S, const q7_t* d_src, q7_t* d_dst, uint32_t blockSize,
                            uint32_t batch, q7_t* d_hist, void* stream) {
  return fir_batch<int8_t>(S, d_src, d_dst, blockSize, batch, d_hist, stream, kFirQ7);
}

#define MI355X_FIR_MULTI(NAME, INST, T, CT, KIND)                                                          \
  arm_status NAME##_batch_multi(const INST* S, uint32_t nshards, const int* devices, const T* const* d_src, \
                                T* const* d_dst, T* const* d_hist, uint32_t blockSize, const uint32_t* batch) { \
    return fir_batch_multi<CT>(S, nshards, devices, (const CT* const*)d_src, (CT* const*)d_dst,          \
                               (CT* const*)d_hist, blockSize, batch, KIND);                              \
  }
MI355X_FIR_MULTI(arm_fir_f32, arm_fir_instance_f32, float32_t, float, kFirF32)
MI355X_FIR_MULTI(arm_fir_q15, arm_fir_instance_q15, q15_t, int16_t, kFirQ15)
MI355X_FIR_MULTI(arm_fir_fast_q15, arm_fir_instance_q15, q15_t, int16_t, kFirFastQ15)
MI355X_FIR_MULTI(arm_fir_q31, arm_fir_instance_q31, q31_t, int32_t, kFirQ31)
MI355X_FIR_MULTI(arm_fir_fast_q31, arm_fir_instance_q31, q31_t, int32_t, kFirFastQ31)
MI355X_FIR_MULTI(arm_fir_q7, arm_fir_instance_q7, q7_t, int8_t, kFirQ7)
#undef MI355X_FIR_MULTI

arm_status arm_mat_mult_f32_batch_multi(const arm_matrix_instance_f32* pSrcA, const arm_matrix_instance_f32* pSrcB,
                                        arm_matrix_instance_f32* pDst, uint32_t nshards, const int* devices,
                                        const float32_t* const* d_a, const float32_t* const* d_b,
                                        float32_t* const* d_c, const uint32_t* batch) {
  return mat_batch_multi<float>(pSrcA, pSrcB, pDst, nshards, devices, d_a, d_b, d_c, batch,
                                "arm_mat_mult_f32_batch_multi", mat_mult_f32_launch);
}
arm_status arm_mat_mult_q7_batch_multi(const arm_matrix_instance_q7* pSrcA, const arm_matrix_instance_q7* pSrcB,
                                       arm_matrix_instance_q7* pDst, uint32_t nshards, const int* devices,
                                       const q7_t* const* d_a, const q7_t* const* d_b, q7_t* const* d_c,
                                       const uint32_t* batch) {
  return mat_batch_multi<int8_t>(pSrcA, pSrcB, pDst, nshards, devices, d_a, d_b, d_c, batch,
                                 "arm_mat_mult_q7_batch_multi", mat_mult_q7_launch);
}
arm_status arm_mat_mult_q15_batch_multi(const arm_matrix_instance_q15* pSrcA, const arm_matrix_instance_q15* pSrcB,
                                        arm_matrix_instance_q15* pDst, uint32_t nshards, const int* devices,
                                        const q15_t* const* d_a, const q15_t* const* d_b, q15_t* const* d_c,
                                        const uint32_t* batch) {
  return mat_batch_multi<int16_t>(pSrcA, pSrcB, pDst, nshards, devices, d_a, d_b, d_c, batch,
                                  "arm_mat_mult_q15_batch_multi", mat_mult_q15_launch);
}
arm_status arm_mat_mult_q31_batch_multi(const arm_matrix_instance_q31* pSrcA, const arm_matrix_instance_q31* pSrcB,
                                        arm_matrix_instance_q31* pDst, uint32_t nshards, const int* devices,
                                        const q31_t* const* d_a, const q31_t* const* d_b, q31_t* const* d_c,
                                        const uint32_t* batch) {
  return mat_batch_multi<int32_t>(pSrcA, pSrcB, pDst, nshards, devices, d_a, d_b, d_c, batch,
                                  "arm_mat_mult_q31_batch_multi", mat_mult_q31_launch);
}

arm_status arm_mat_mult_f32(const arm_matrix_instance_f32* pSrcA, const arm_matrix_instance_f32* pSrcB,
                            arm_matrix_instance_f32* pDst) {
  return mat_mult_sync<float>(pSrcA, pSrcB, pDst, "arm_mat_mult_f32", mat_mult_f32_launch);
}
arm_status arm_mat_mult_f32_batch(const arm_matrix_instance_f32* pSrcA, const arm_matrix_instance_f32* pSrcB,
                                  arm_matrix_instance_f32* pDst, uint32_t batch, void* stream) {
  return mat_batch(pSrcA, pSrcB, pDst, batch, stream, "arm_mat_mult_f32_batch", mat_mult_f32_launch);
}

// ---- MFCC (drop-in + batched) ------------------------------------------------------
void arm_mfcc_f32(const arm_mfcc_instance_f32* S, float32_t* pSrc, float32_t* pDst, float32_t* pTmp) {
  (void)pTmp;
  (void)mfcc_sync<MfccDev<float>>(S, pSrc, pDst, "arm_mfcc_f32");
}
arm_status arm_mfcc_f32_batch(const arm_mfcc_instance_f32* S, float32_t* d_src, float32_t* d_dst, float32_t* d_tmp,
                              uint32_t batch, void* stream) {
  return mfcc_batch<MfccDev<float>>(S, d_src, d_dst, d_tmp, batch, stream);
}
arm_status arm_mfcc_q31(const arm_mfcc_instance_q31* S, q31_t* pSrc, q31_t* pDst, q31_t* pTmp) {
  (void)pTmp;
  return mfcc_sync<MfccFxDev<int32_t>>(S, pSrc, pDst, "arm_mfcc_q31");
}
arm_status arm_mfcc_q31_batch(const arm_mfcc_instance_q31* S, q31_t* d_src, q31_t* d_dst, q31_t* d_tmp,
                              uint32_t batch, void* stream) {
  return mfcc_batch<MfccFxDev<int32_t>>(S, d_src, d_dst, d_tmp, batch, stream);
}
arm_status arm_mfcc_q15(const arm_mfcc_instance_q15* S, q15_t* pSrc, q15_t* pDst, q31_t* pTmp) {
  (void)pTmp;
  return mfcc_sync<MfccFxDev<int16_t>>(S, pSrc, pDst, "arm_mfcc_q15");
}
arm_status arm_mfcc_q15_batch(const arm_mfcc_instance_q15* S, q15_t* d_src, q15_t* d_dst, q15_t* d_tmp,
                              uint32_t batch, void* stream) {
  return mfcc_batch<MfccFxDev<int16_t>>(S, d_src, d_dst, d_tmp, batch, stream);
}

// ---- matrix multiply q7 / q15 / q31 ---------------------------------------------
// arm_mat_mult_q7.c:689-790 (scalar branch): q31_t sum of exact q7 products (never wraps for
// uint16_t dimensions), (q7)__SSAT(sum >> 7, 8); pState (the Helium/Neon transpose buffer) unused.
arm_status arm_mat_mult_q7(const arm_matrix_instance_q7* pSrcA, const arm_matrix_instance_q7* pSrcB,
                           arm_matrix_instance_q7* pDst, q7_t* pState) {
  (void)pState;
  return mat_mult_sync<int8_t>(pSrcA, pSrcB, pDst, "arm_mat_mult", mat_mult_q7_launch);
}
arm_status arm_mat_mult_q15(const arm_matrix_instance_q15* pSrcA, const arm_matrix_instance_q15* pSrcB,
                            arm_matrix_instance_q15* pDst, q15_t* pState) {
  (void)pState;   // the reference's transpose buffer (ARM_MATH_DSP branch only)
  return mat_mult_sync<int16_t>(pSrcA, pSrcB, pDst, "arm_mat_mult", mat_mult_q15_launch);
}
arm_status arm_mat_mult_q31(const arm_matrix_instance_q31* pSrcA, const arm_matrix_instance_q31* pSrcB,
                            arm_matrix_instance_q31* pDst) {
  return mat_mult_sync<int32_t>(pSrcA, pSrcB, pDst, "arm_mat_mult", mat_mult_q31_launch);
}
// arm_mat_mult_opt_q31.c:648-780 (the host build's scalar branch): the q31 product above; pState
// (the Helium branch's transpose buffer) is unused there too.
arm_status arm_mat_mult_opt_q31(const arm_matrix_instance_q31* pSrcA, const arm_matrix_instance_q31* pSrcB,
                                arm_matrix_instance_q31* pDst, q31_t* pState) {
  (void)pState;
  return arm_mat_mult_q31(pSrcA, pSrcB, pDst);
}
// arm_mat_mult_fast_q15.c:351-401 (!ARM_MATH_DSP: q31_t modular sum, (q15)(sum >> 15)),
// arm_mat_mult_fast_q31.c:152-166 (per-product high word, sum << 1); pState unused (the
// reference's transpose buffer).
arm_status arm_mat_mult_fast_q15(const arm_matrix_instance_q15* pSrcA, const arm_matrix_instance_q15* pSrcB,
                                 arm_matrix_instance_q15* pDst, q15_t* pState) {
  (void)pState;
  return mat_mult_sync<int16_t>(pSrcA, pSrcB, pDst, "arm_mat_mult", mat_mult_fast_q15_launch);
}
arm_status arm_mat_mult_fast_q31(const arm_matrix_instance_q31* pSrcA, const arm_matrix_instance_q31* pSrcB,
                                 arm_matrix_instance_q31* pDst) {
  return mat_mult_sync<int32_t>(pSrcA, pSrcB, pDst, "arm_mat_mult", mat_mult_fast_q31_launch);
}
#define MI355X_MAT_BATCH(NAME, INST, LAUNCH)                                                                \
  arm_status NAME(const INST* pSrcA, const INST* pSrcB, INST* pDst, uint32_t batch, void* stream) {        \
    return mat_batch(pSrcA, pSrcB, pDst, batch, stream, #NAME, LAUNCH);                                    \
  }
MI355X_MAT_BATCH(arm_mat_mult_q7_batch, arm_matrix_instance_q7, mat_mult_q7_launch)
MI355X_MAT_BATCH(arm_mat_mult_q15_batch, arm_matrix_instance_q15, mat_mult_q15_launch)
MI355X_MAT_BATCH(arm_mat_mult_q31_batch, arm_matrix_instance_q31, mat_mult_q31_launch)
MI355X_MAT_BATCH(arm_mat_mult_fast_q15_batch, arm_matrix_instance_q15, mat_mult_fast_q15_launch)
MI355X_MAT_BATCH(arm_mat_mult_fast_q31_batch, arm_matrix_instance_q31, mat_mult_fast_q31_launch)
#undef MI355X_MAT_BATCH

// ---- complex matrix multiply f32 / q31 / q15 ----------------------------------------
// arm_mat_cmplx_mult_f32.c:1225-1392, arm_mat_cmplx_mult_q31.c:836-1057 (scalar branch: wrapping q63
// sums, clip_q63_to_q31(sum >> 31)), arm_mat_cmplx_mult_q15.c:433-582 (!ARM_MATH_DSP: q63 sums,
// __SSAT(sum >> 15, 16); B is first transposed into pScratch, which the call leaves there).
// numRows / numCols count complex elements; pData holds interleaved (re, im) words.
arm_status arm_mat_cmplx_mult_f32(const arm_matrix_instance_f32* pSrcA, const arm_matrix_instance_f32* pSrcB,
                                  arm_matrix_instance_f32* pDst) {
  return mat_mult_sync<float>(pSrcA, pSrcB, pDst, "arm_mat_cmplx_mult_f32", mat_cmplx_mult_f32_launch, 2);
}
arm_status arm_mat_cmplx_mult_q31(const arm_matrix_instance_q31* pSrcA, const arm_matrix_instance_q31* pSrcB,
                                  arm_matrix_instance_q31* pDst) {
  return mat_mult_sync<int32_t>(pSrcA, pSrcB, pDst, "arm_mat_cmplx_mult_q31", mat_cmplx_mult_q31_launch, 2);
}
arm_status arm_mat_cmplx_mult_q15(const arm_matrix_instance_q15* pSrcA, const arm_matrix_instance_q15* pSrcB,
                                  arm_matrix_instance_q15* pDst, q15_t* pScratch) {
  return mat_mult_sync<int16_t>(pSrcA, pSrcB, pDst, "arm_mat_cmplx_mult_q15", mat_cmplx_mult_q15_launch, 2,
                                pScratch);
}
#define MI355X_CMAT(SUF, INST, T, CT)                                                                           \
  arm_status arm_mat_cmplx_mult_##SUF##_batch(const INST* pSrcA, const INST* pSrcB, INST* pDst, uint32_t batch, \
                                              void* stream) {                                                   \
    return mat_batch(pSrcA, pSrcB, pDst, batch, stream, "arm_mat_cmplx_mult_" #SUF "_batch",                    \
                     mat_cmplx_mult_##SUF##_launch);                                                            \
  }                                                                                                             \
  arm_status arm_mat_cmplx_mult_##SUF##_batch_multi(const INST* pSrcA, const INST* pSrcB, INST* pDst,           \
                                                    uint32_t nshards, const int* devices, const T* const* d_a,  \
                                                    const T* const* d_b, T* const* d_c, const uint32_t* batch) { \
    return mat_batch_multi<CT>(pSrcA, pSrcB, pDst, nshards, devices, d_a, d_b, d_c, batch,                      \
                               "arm_mat_cmplx_mult_" #SUF "_batch_multi", mat_cmplx_mult_##SUF##_launch);       \
  }
MI355X_CMAT(f32, arm_matrix_instance_f32, float32_t, float)
MI355X_CMAT(q31, arm_matrix_instance_q31, q31_t, int32_t)
MI355X_CMAT(q15, arm_matrix_instance_q15, q15_t, int16_t)
#undef MI355X_CMAT

// ---- inverse, Cholesky, LDLT, triangular solves (f32); mat_solve_sync and its kin precede the C block ----
arm_status arm_mat_inverse_f32(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pDst) {
  if (!pSrc || !pDst || !pSrc->pData || !pDst->pData) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(pSrc) || !square(pDst) || pSrc->numRows != pDst->numRows) return ARM_MATH_SIZE_MISMATCH;
  const int n = pSrc->numRows;
  if (n == 0) return ARM_MATH_SUCCESS;
  // src is written back: the reference destroys it, and its final words are part of the contract
  SolveBuf b[2] = {{pSrc->pData, sizeof(float) * n * n, true, true}, {pDst->pData, sizeof(float) * n * n, false, true}};
  return mat_solve_sync(b, 2, "arm_mat_inverse_f32", [&](hipStream_t st, int32_t* ds) {
    return mat_inverse_f32_launch(n, (float*)b[0].d, (float*)b[1].d, 1, ds, st);
  });
}

arm_status arm_mat_cholesky_f32(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pDst) {
  if (!pSrc || !pDst || !pSrc->pData || !pDst->pData) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(pSrc) || !square(pDst) || pSrc->numRows != pDst->numRows) return ARM_MATH_SIZE_MISMATCH;
  const int n = pSrc->numRows;
  if (n == 0) return ARM_MATH_SUCCESS;
  // dst is staged in as well: its strict upper triangle, and the columns past a failure, are never written
  SolveBuf b[2] = {{pSrc->pData, sizeof(float) * n * n, true, false}, {pDst->pData, sizeof(float) * n * n, true, true}};
  return mat_solve_sync(b, 2, "arm_mat_cholesky_f32", [&](hipStream_t st, int32_t* ds) {
    return mat_cholesky_f32_launch(n, (const float*)b[0].d, (float*)b[1].d, 1, ds, st);
  });
}

arm_status arm_mat_ldlt_f32(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pl,
                            arm_matrix_instance_f32* pd, uint16_t* pp) {
  if (!pSrc || !pl || !pd || !pp || !pSrc->pData || !pl->pData || !pd->pData) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(pSrc) || !square(pl) || !square(pd) || pl->numRows != pd->numRows || pSrc->numRows != pl->numRows)
    return ARM_MATH_SIZE_MISMATCH;
  const int n = pSrc->numRows;
  if (n == 0) return ARM_MATH_SUCCESS;
  SolveBuf b[4] = {{pSrc->pData, sizeof(float) * n * n, true, false},
                   {pl->pData, sizeof(float) * n * n, false, true},
                   {pd->pData, sizeof(float) * n * n, false, true},
                   {pp, sizeof(uint16_t) * n, false, true}};
  return mat_solve_sync(b, 4, "arm_mat_ldlt_f32", [&](hipStream_t st, int32_t* ds) {
    hipError_t e = hipMemsetAsync(ds, 0, sizeof(int32_t), st);       // the function cannot fail
    if (e == hipSuccess)
      e = mat_ldlt_f32_launch(n, (const float*)b[0].d, (float*)b[1].d, (float*)b[2].d, (uint16_t*)b[3].d, 1, st);
    return e;
  });
}

arm_status arm_mat_solve_lower_triangular_f32(const arm_matrix_instance_f32* lt, const arm_matrix_instance_f32* a,
                                              arm_matrix_instance_f32* dst) {
  return solve_tri_sync(true, lt, a, dst, "arm_mat_solve_lower_triangular_f32");
}
arm_status arm_mat_solve_upper_triangular_f32(const arm_matrix_instance_f32* ut, const arm_matrix_instance_f32* a,
                                              arm_matrix_instance_f32* dst) {
  return solve_tri_sync(false, ut, a, dst, "arm_mat_solve_upper_triangular_f32");
}

arm_status arm_mat_inverse_f32_batch(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pDst,
                                     uint32_t batch, int32_t* d_status, void* stream) {
  if (!pSrc || !pDst) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(pSrc) || !square(pDst) || pSrc->numRows != pDst->numRows) return ARM_MATH_SIZE_MISMATCH;
  if (batch == 0 || pSrc->numRows == 0) return ARM_MATH_SUCCESS;
  if (!pSrc->pData || !pDst->pData) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(mat_inverse_f32_launch(pSrc->numRows, pSrc->pData, pDst->pData, batch, d_status,
                                             (hipStream_t)stream), "arm_mat_inverse_f32_batch");
}

arm_status arm_mat_cholesky_f32_batch(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pDst,
                                      uint32_t batch, int32_t* d_status, void* stream) {
  if (!pSrc || !pDst) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(pSrc) || !square(pDst) || pSrc->numRows != pDst->numRows) return ARM_MATH_SIZE_MISMATCH;
  if (batch == 0 || pSrc->numRows == 0) return ARM_MATH_SUCCESS;
  if (!pSrc->pData || !pDst->pData) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(mat_cholesky_f32_launch(pSrc->numRows, pSrc->pData, pDst->pData, batch, d_status,
                                              (hipStream_t)stream), "arm_mat_cholesky_f32_batch");
}

arm_status arm_mat_ldlt_f32_batch(const arm_matrix_instance_f32* pSrc, arm_matrix_instance_f32* pl,
                                  arm_matrix_instance_f32* pd, uint16_t* d_pp, uint32_t batch, void* stream) {
  if (!pSrc || !pl || !pd) return ARM_MATH_ARGUMENT_ERROR;
  if (!square(pSrc) || !square(pl) || !square(pd) || pl->numRows != pd->numRows || pSrc->numRows != pl->numRows)
    return ARM_MATH_SIZE_MISMATCH;
  if (batch == 0 || pSrc->numRows == 0) return ARM_MATH_SUCCESS;
  if (!pSrc->pData || !pl->pData || !pd->pData || !d_pp) return ARM_MATH_ARGUMENT_ERROR;
  return batch_status(mat_ldlt_f32_launch(pSrc->numRows, pSrc->pData, pl->pData, pd->pData, d_pp, batch,
                                          (hipStream_t)stream), "arm_mat_ldlt_f32_batch");
}

arm_status arm_mat_solve_lower_triangular_f32_batch(const arm_matrix_instance_f32* lt,
                                                    const arm_matrix_instance_f32* a, arm_matrix_instance_f32* dst,
                                                    uint32_t batch, int32_t* d_status, void* stream) {
  return solve_tri_batch(true, lt, a, dst, batch, d_status, stream, "arm_mat_solve_lower_triangular_f32_batch");
}
arm_status arm_mat_solve_upper_triangular_f32_batch(const arm_matrix_instance_f32* ut,
                                                    const arm_matrix_instance_f32* a, arm_matrix_instance_f32* dst,
                                                    uint32_t batch, int32_t* d_status, void* stream) {
  return solve_tri_batch(false, ut, a, dst, batch, d_status, stream, "arm_mat_solve_upper_triangular_f32_batch");
}

// ---- add / sub / scale, transposes, matrix x vector; mat_ew and its kin precede the C block ----
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
    mat_vec_mult_sync<CT>(pSrcMat, (const CT*)pVec, (CT*)pDst, "arm_mat_vec_mult_" #SUF);                        \
  }                                                                                                              \
  arm_status arm_mat_vec_mult_##SUF##_batch(const INST* pSrcMat, uint32_t matStride, const T* d_vec, T* d_dst,   \
                                            uint32_t batch, void* stream) {                                      \
    return mat_vec_mult_batch<CT>(pSrcMat, matStride, (const CT*)d_vec, (CT*)d_dst, batch, stream,               \
                                  "arm_mat_vec_mult_" #SUF "_batch");                                            \
  }
MI355X_MAT_VEC(f32, arm_matrix_instance_f32, float32_t, float)
MI355X_MAT_VEC(q31, arm_matrix_instance_q31, q31_t, int32_t)
MI355X_MAT_VEC(q15, arm_matrix_instance_q15, q15_t, int16_t)
MI355X_MAT_VEC(q7, arm_matrix_instance_q7, q7_t, int8_t)
#undef MI355X_MAT_VEC

// ---- complex math, max / min; cmplx_ew and its kin precede the C block ----
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

#define MI355X_SEARCH(NAME, MAX, SUF, T, CT)                                                                     \
  void arm_##NAME##_##SUF(const T* pSrc, uint32_t blockSize, T* pResult, uint32_t* pIndex) {                     \
    cm_search<CT>(MAX, (const CT*)pSrc, blockSize, (CT*)pResult, pIndex, true, 1, nullptr, "arm_" #NAME "_" #SUF); \
  }                                                                                                              \
  arm_status arm_##NAME##_##SUF##_batch(const T* d_src, uint32_t blockSize, T* d_result, uint32_t* d_index,      \
                                        uint32_t batch, void* stream) {                                          \
    return cm_search<CT>(MAX, (const CT*)d_src, blockSize, (CT*)d_result, d_index, false, batch, stream,         \
                         "arm_" #NAME "_" #SUF "_batch");                                                        \
  }
#define MI355X_SEARCH_TYPE(SUF, T, CT) MI355X_SEARCH(max, true, SUF, T, CT) MI355X_SEARCH(min, false, SUF, T, CT)
MI355X_SEARCH_TYPE(f32, float32_t, float)
MI355X_SEARCH_TYPE(q31, q31_t, int32_t)
MI355X_SEARCH_TYPE(q15, q15_t, int16_t)
MI355X_SEARCH_TYPE(q7, q7_t, int8_t)
#undef MI355X_SEARCH_TYPE
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

// ---- statistics; st_sum and st_search precede the C block ----
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

// abs searches with the index, and the four searches without it
#define MI355X_STAT_SEARCH(NAME, MAX, ABS, SUF, T, CT)                                                           \
  void arm_##NAME##_##SUF(const T* pSrc, uint32_t blockSize, T* pResult, uint32_t* pIndex) {                     \
    st_search<CT>(MAX, ABS, true, (const CT*)pSrc, blockSize, (CT*)pResult, pIndex, true, 1, nullptr,            \
                  "arm_" #NAME "_" #SUF);                                                                        \
  }                                                                                                              \
  arm_status arm_##NAME##_##SUF##_batch(const T* d_src, uint32_t blockSize, T* d_result, uint32_t* d_index,      \
                                        uint32_t batch, void* stream) {                                          \
    return st_search<CT>(MAX, ABS, true, (const CT*)d_src, blockSize, (CT*)d_result, d_index, false, batch,      \
                         stream, "arm_" #NAME "_" #SUF "_batch");                                                \
  }
#define MI355X_STAT_NO_IDX(NAME, MAX, ABS, SUF, T, CT)                                                           \
  void arm_##NAME##_no_idx_##SUF(const T* pSrc, uint32_t blockSize, T* pResult) {                                \
    st_search<CT>(MAX, ABS, false, (const CT*)pSrc, blockSize, (CT*)pResult, nullptr, true, 1, nullptr,          \
                  "arm_" #NAME "_no_idx_" #SUF);                                                                 \
  }                                                                                                              \
  arm_status arm_##NAME##_no_idx_##SUF##_batch(const T* d_src, uint32_t blockSize, T* d_result, uint32_t batch,  \
                                               void* stream) {                                                   \
    return st_search<CT>(MAX, ABS, false, (const CT*)d_src, blockSize, (CT*)d_result, nullptr, false, batch,     \
                         stream, "arm_" #NAME "_no_idx_" #SUF "_batch");                                         \
  }
#define MI355X_STAT_SEARCH_TYPE(SUF, T, CT)             \
  MI355X_STAT_SEARCH(absmax, true, true, SUF, T, CT)    \
  MI355X_STAT_SEARCH(absmin, false, true, SUF, T, CT)   \
  MI355X_STAT_NO_IDX(max, true, false, SUF, T, CT)      \
  MI355X_STAT_NO_IDX(min, false, false, SUF, T, CT)     \
  MI355X_STAT_NO_IDX(absmax, true, true, SUF, T, CT)    \
  MI355X_STAT_NO_IDX(absmin, false, true, SUF, T, CT)
MI355X_STAT_SEARCH_TYPE(f32, float32_t, float)
MI355X_STAT_SEARCH_TYPE(q31, q31_t, int32_t)
MI355X_STAT_SEARCH_TYPE(q15, q15_t, int16_t)
MI355X_STAT_SEARCH_TYPE(q7, q7_t, int8_t)
#undef MI355X_STAT_SEARCH_TYPE
#undef MI355X_STAT_NO_IDX
#undef MI355X_STAT_SEARCH

// ---- basic math; bm_ew and bm_dot precede the C block ----
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

// ---- support functions; sp_convert .. sp_barycenter precede the C block ----
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
  if (!S) { cm_null(true, "arm_sort_f32"); return; }
  if ((int)S->alg < (int)ARM_SORT_BITONIC || (int)S->alg > (int)ARM_SORT_SELECTION) return;
  sp_sort((int)S->dir, pSrc, pDst, blockSize, true, 1, nullptr, "arm_sort_f32");
}
// S->buffer is neither read nor written.
void arm_merge_sort_f32(const arm_merge_sort_instance_f32* S, float32_t* pSrc, float32_t* pDst, uint32_t blockSize) {
  if (!S) { cm_null(true, "arm_merge_sort_f32"); return; }
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

// ---- convolution ------------------------------------------------------------------
#define MI355X_CONV_FULL(NAME, T, CT, OP, VAR)                                                                  \
  void NAME(const T* pSrcA, uint32_t srcALen, const T* pSrcB, uint32_t srcBLen, T* pDst) {                      \
    conv_family_sync<CT>(OP, VAR, (const CT*)pSrcA, srcALen, (const CT*)pSrcB, srcBLen, (CT*)pDst, 0, 0, #NAME); \
  }                                                                                                             \
  arm_status NAME##_batch(const T* d_a, uint32_t srcALen, uint32_t strideA, const T* d_b, uint32_t srcBLen,     \
                          uint32_t strideB, T* d_dst, uint32_t batch, void* stream) {                           \
    return conv_family_batch<CT>(OP, VAR, (const CT*)d_a, srcALen, strideA, (const CT*)d_b, srcBLen, strideB,   \
                                 (CT*)d_dst, 0, 0, batch, stream, #NAME "_batch");                              \
  }
MI355X_CONV_FULL(arm_conv_f32, float32_t, float, kConvF32, kVarConv)
MI355X_CONV_FULL(arm_conv_q15, q15_t, int16_t, kConvQ15, kVarConv)
MI355X_CONV_FULL(arm_conv_q31, q31_t, int32_t, kConvQ31, kVarConv)
MI355X_CONV_FULL(arm_conv_fast_q15, q15_t, int16_t, kConvFastQ15, kVarConv)
MI355X_CONV_FULL(arm_conv_fast_q31, q31_t, int32_t, kConvFastQ31, kVarConv)
MI355X_CONV_FULL(arm_correlate_f32, float32_t, float, kConvF32, kVarCorr)
MI355X_CONV_FULL(arm_correlate_q15, q15_t, int16_t, kConvQ15, kVarCorr)
MI355X_CONV_FULL(arm_correlate_q31, q31_t, int32_t, kConvQ31, kVarCorr)
MI355X_CONV_FULL(arm_correlate_fast_q15, q15_t, int16_t, kConvFastQ15, kVarCorr)
MI355X_CONV_FULL(arm_correlate_fast_q31, q31_t, int32_t, kConvFastQ31, kVarCorr)
MI355X_CONV_FULL(arm_conv_q7, q7_t, int8_t, kConvQ7, kVarConv)
MI355X_CONV_FULL(arm_correlate_q7, q7_t, int8_t, kConvQ7, kVarCorr)
#undef MI355X_CONV_FULL

#define MI355X_CONV_PARTIAL(NAME, T, CT, OP)                                                                       \
  arm_status NAME(const T* pSrcA, uint32_t srcALen, const T* pSrcB, uint32_t srcBLen, T* pDst, uint32_t firstIndex, \
                  uint32_t numPoints) {                                                                            \
    if (!partial_range_ok(srcALen, srcBLen, firstIndex, numPoints)) return ARM_MATH_ARGUMENT_ERROR;                \
    conv_family_sync<CT>(OP, kVarPartial, (const CT*)pSrcA, srcALen, (const CT*)pSrcB, srcBLen, (CT*)pDst,         \
                         firstIndex, numPoints, #NAME);                                                            \
    return ARM_MATH_SUCCESS;                                                                                       \
  }                                                                                                                \
  arm_status NAME##_batch(const T* d_a, uint32_t srcALen, uint32_t strideA, const T* d_b, uint32_t srcBLen,        \
                          uint32_t strideB, T* d_dst, uint32_t firstIndex, uint32_t numPoints, uint32_t batch,     \
                          void* stream) {                                                                          \
    if (!partial_range_ok(srcALen, srcBLen, firstIndex, numPoints)) return ARM_MATH_ARGUMENT_ERROR;                \
    return conv_family_batch<CT>(OP, kVarPartial, (const CT*)d_a, srcALen, strideA, (const CT*)d_b, srcBLen,       \
                                 strideB, (CT*)d_dst, firstIndex, numPoints, batch, stream, #NAME "_batch");       \
  }
MI355X_CONV_PARTIAL(arm_conv_partial_f32, float32_t, float, kConvF32)
MI355X_CONV_PARTIAL(arm_conv_partial_q15, q15_t, int16_t, kConvQ15)
MI355X_CONV_PARTIAL(arm_conv_partial_q31, q31_t, int32_t, kConvQ31)
MI355X_CONV_PARTIAL(arm_conv_partial_q7, q7_t, int8_t, kConvQ7)
// arm_conv_partial_fast_q15 / _q31: outputs firstIndex .. of arm_conv_fast_q15 / _q31.  The
// reference's own bodies (arm_conv_partial_fast_q15.c:110-118 stage sizes) read outside the
// inputs for most ranges (the host build segfaults: tools/probes/conv_family_model.py), so
// the contract is the documented one: the fast convolution's words over the range.
MI355X_CONV_PARTIAL(arm_conv_partial_fast_q15, q15_t, int16_t, kConvFastQ15)
MI355X_CONV_PARTIAL(arm_conv_partial_fast_q31, q31_t, int32_t, kConvFastQ31)
#undef MI355X_CONV_PARTIAL

// The scratch-buffer ("_opt") forms (arm_conv_opt_q15.c, arm_conv_opt_q7.c,
// arm_correlate_opt_q15.c, arm_correlate_opt_q7.c, arm_conv_partial_opt_q15.c, _q7.c): the
// exact sums of the plain functions (tests/test_conv_opt.py pins that on the reference build),
// so they run the same kernels; the fast q15 ones are a modular sum with a saturating output
// (kConvFastOptQ15).  The scratch buffers are not needed.
void arm_conv_opt_q15(const q15_t* pSrcA, uint32_t srcALen, const q15_t* pSrcB, uint32_t srcBLen, q15_t* pDst,
                      q15_t* pScratch1, q15_t* pScratch2) {
  (void)pScratch1; (void)pScratch2;
  arm_conv_q15(pSrcA, srcALen, pSrcB, srcBLen, pDst);
}
void arm_conv_opt_q7(const q7_t* pSrcA, uint32_t srcALen, const q7_t* pSrcB, uint32_t srcBLen, q7_t* pDst,
                     q15_t* pScratch1, q15_t* pScratch2) {
  (void)pScratch1; (void)pScratch2;
  arm_conv_q7(pSrcA, srcALen, pSrcB, srcBLen, pDst);
}
void arm_correlate_opt_q15(const q15_t* pSrcA, uint32_t srcALen, const q15_t* pSrcB, uint32_t srcBLen, q15_t* pDst,
                           q15_t* pScratch) {
  (void)pScratch;
  arm_correlate_q15(pSrcA, srcALen, pSrcB, srcBLen, pDst);
}
void arm_correlate_opt_q7(const q7_t* pSrcA, uint32_t srcALen, const q7_t* pSrcB, uint32_t srcBLen, q7_t* pDst,
                          q15_t* pScratch1, q15_t* pScratch2) {
  (void)pScratch1; (void)pScratch2;
  arm_correlate_q7(pSrcA, srcALen, pSrcB, srcBLen, pDst);
}
arm_status arm_conv_partial_opt_q15(const q15_t* pSrcA, uint32_t srcALen, const q15_t* pSrcB, uint32_t srcBLen,
                                    q15_t* pDst, uint32_t firstIndex, uint32_t numPoints, q15_t* pScratch1,
                                    q15_t* pScratch2) {
  (void)pScratch1; (void)pScratch2;
  return arm_conv_partial_q15(pSrcA, srcALen, pSrcB, srcBLen, pDst, firstIndex, numPoints);
}
arm_status arm_conv_partial_opt_q7(const q7_t* pSrcA, uint32_t srcALen, const q7_t* pSrcB, uint32_t srcBLen,
                                   q7_t* pDst, uint32_t firstIndex, uint32_t numPoints, q15_t* pScratch1,
                                   q15_t* pScratch2) {
  (void)pScratch1; (void)pScratch2;
  return arm_conv_partial_q7(pSrcA, srcALen, pSrcB, srcBLen, pDst, firstIndex, numPoints);
}
void arm_conv_fast_opt_q15(const q15_t* pSrcA, uint32_t srcALen, const q15_t* pSrcB, uint32_t srcBLen, q15_t* pDst,
                           q15_t* pScratch1, q15_t* pScratch2) {
  (void)pScratch1; (void)pScratch2;
  conv_family_sync<int16_t>(kConvFastOptQ15, kVarConv, pSrcA, srcALen, pSrcB, srcBLen, pDst, 0, 0,
                            "arm_conv_fast_opt_q15");
}
void arm_correlate_fast_opt_q15(const q15_t* pSrcA, uint32_t srcALen, const q15_t* pSrcB, uint32_t srcBLen,
                                q15_t* pDst, q15_t* pScratch) {
  (void)pScratch;
  conv_family_sync<int16_t>(kConvFastOptQ15, kVarCorr, pSrcA, srcALen, pSrcB, srcBLen, pDst, 0, 0,
                            "arm_correlate_fast_opt_q15");
}
arm_status arm_conv_partial_fast_opt_q15(const q15_t* pSrcA, uint32_t srcALen, const q15_t* pSrcB, uint32_t srcBLen,
                                         q15_t* pDst, uint32_t firstIndex, uint32_t numPoints, q15_t* pScratch1,
                                         q15_t* pScratch2) {
  (void)pScratch1; (void)pScratch2;
  if (!partial_range_ok(srcALen, srcBLen, firstIndex, numPoints)) return ARM_MATH_ARGUMENT_ERROR;
  conv_family_sync<int16_t>(kConvFastOptQ15, kVarPartial, pSrcA, srcALen, pSrcB, srcBLen, pDst, firstIndex,
                            numPoints, "arm_conv_partial_fast_opt_q15");
  return ARM_MATH_SUCCESS;
}

// ---- multirate FIR ---------------------------------------------------------------------
arm_status arm_fir_decimate_init_f32(arm_fir_decimate_instance_f32* S, uint16_t numTaps, uint8_t M,
                                     const float32_t* pCoeffs, float32_t* pState, uint32_t blockSize) {
  return decimate_init<float>(S, numTaps, M, pCoeffs, pState, blockSize);
}
arm_status arm_fir_decimate_init_q15(arm_fir_decimate_instance_q15* S, uint16_t numTaps, uint8_t M,
                                     const q15_t* pCoeffs, q15_t* pState, uint32_t blockSize) {
  return decimate_init<int16_t>(S, numTaps, M, pCoeffs, pState, blockSize);
}
arm_status arm_fir_decimate_init_q31(arm_fir_decimate_instance_q31* S, uint16_t numTaps, uint8_t M,
                                     const q31_t* pCoeffs, q31_t* pState, uint32_t blockSize) {
  return decimate_init<int32_t>(S, numTaps, M, pCoeffs, pState, blockSize);
}
arm_status arm_fir_interpolate_init_f32(arm_fir_interpolate_instance_f32* S, uint8_t L, uint16_t numTaps,
                                        const float32_t* pCoeffs, float32_t* pState, uint32_t blockSize) {
  return interpolate_init<float>(S, L, numTaps, pCoeffs, pState, blockSize);
}
arm_status arm_fir_interpolate_init_q15(arm_fir_interpolate_instance_q15* S, uint8_t L, uint16_t numTaps,
                                        const q15_t* pCoeffs, q15_t* pState, uint32_t blockSize) {
  return interpolate_init<int16_t>(S, L, numTaps, pCoeffs, pState, blockSize);
}
arm_status arm_fir_interpolate_init_q31(arm_fir_interpolate_instance_q31* S, uint8_t L, uint16_t numTaps,
                                        const q31_t* pCoeffs, q31_t* pState, uint32_t blockSize) {
  return interpolate_init<int32_t>(S, L, numTaps, pCoeffs, pState, blockSize);
}
#define MI355X_DECIM(NAME, INST, T, CT, OP)                                                              \
  void NAME(const INST* S, const T* pSrc, T* pDst, uint32_t blockSize) {                                \
    decimate_sync<CT>(S, (const CT*)pSrc, (CT*)pDst, blockSize, OP, #NAME);                             \
  }                                                                                                     \
  arm_status NAME##_batch(const INST* S, const T* d_src, T* d_dst, uint32_t blockSize, uint32_t batch,  \
                          T* d_hist, void* stream) {                                                    \
    return decimate_batch<CT>(S, (const CT*)d_src, (CT*)d_dst, blockSize, batch, (CT*)d_hist, stream, OP, \
                              #NAME "_batch");                                                          \
  }
MI355X_DECIM(arm_fir_decimate_f32, arm_fir_decimate_instance_f32, float32_t, float, kMrF32)
MI355X_DECIM(arm_fir_decimate_q15, arm_fir_decimate_instance_q15, q15_t, int16_t, kMrQ15)
MI355X_DECIM(arm_fir_decimate_fast_q15, arm_fir_decimate_instance_q15, q15_t, int16_t, kMrFastQ15)
MI355X_DECIM(arm_fir_decimate_q31, arm_fir_decimate_instance_q31, q31_t, int32_t, kMrQ31)
MI355X_DECIM(arm_fir_decimate_fast_q31, arm_fir_decimate_instance_q31, q31_t, int32_t, kMrFastQ31)
#undef MI355X_DECIM
#define MI355X_INTERP(NAME, INST, T, CT, OP)                                                             \
  void NAME(const INST* S, const T* pSrc, T* pDst, uint32_t blockSize) {                                \
    interpolate_sync<CT>(S, (const CT*)pSrc, (CT*)pDst, blockSize, OP, #NAME);                          \
  }                                                                                                     \
  arm_status NAME##_batch(const INST* S, const T* d_src, T* d_dst, uint32_t blockSize, uint32_t batch,  \
                          T* d_hist, void* stream) {                                                    \
    return interpolate_batch<CT>(S, (const CT*)d_src, (CT*)d_dst, blockSize, batch, (CT*)d_hist, stream, OP, \
                                 #NAME "_batch");                                                       \
  }
MI355X_INTERP(arm_fir_interpolate_f32, arm_fir_interpolate_instance_f32, float32_t, float, kMrF32)
MI355X_INTERP(arm_fir_interpolate_q15, arm_fir_interpolate_instance_q15, q15_t, int16_t, kMrQ15)
MI355X_INTERP(arm_fir_interpolate_q31, arm_fir_interpolate_instance_q31, q31_t, int32_t, kMrQ31)
#undef MI355X_INTERP

#define MI355X_SPARSE(T, CT, OP)                                                                        \
  void arm_fir_sparse_init_##T(arm_fir_sparse_instance_##T* S, uint16_t numTaps, const CT* pCoeffs, CT* pState, \
                               int32_t* pTapDelay, uint16_t maxDelay, uint32_t blockSize) {            \
    sparse_init(S, numTaps, pCoeffs, pState, pTapDelay, maxDelay, blockSize);                           \
  }                                                                                                     \
  arm_status arm_fir_sparse_##T##_batch(const arm_fir_sparse_instance_##T* S, const CT* d_src, CT* d_dst, \
                                        uint32_t blockSize, uint32_t batch, CT* d_hist, void* stream) { \
    return sparse_batch(S, d_src, d_dst, blockSize, batch, d_hist, stream, OP, "arm_fir_sparse_" #T "_batch"); \
  }
MI355X_SPARSE(f32, float32_t, kSpF32)
MI355X_SPARSE(q31, q31_t, kSpQ31)
MI355X_SPARSE(q15, q15_t, kSpQ15)
MI355X_SPARSE(q7, q7_t, kSpQ7)
#undef MI355X_SPARSE
#define MI355X_LATTICE(T, CT, OP)                                                                       \
  void arm_fir_lattice_init_##T(arm_fir_lattice_instance_##T* S, uint16_t numStages, const CT* pCoeffs,  \
                                CT* pState) {                                                           \
    lattice_init(S, numStages, pCoeffs, pState);                                                        \
  }                                                                                                     \
  void arm_fir_lattice_##T(const arm_fir_lattice_instance_##T* S, const CT* pSrc, CT* pDst, uint32_t blockSize) { \
    lattice_sync(S, pSrc, pDst, blockSize, OP, "arm_fir_lattice_" #T);                                  \
  }                                                                                                     \
  arm_status arm_fir_lattice_##T##_batch(const arm_fir_lattice_instance_##T* S, const CT* d_src, CT* d_dst, \
                                         uint32_t blockSize, uint32_t batch, CT* d_state, void* stream) { \
    return lattice_batch(S, d_src, d_dst, blockSize, batch, d_state, stream, OP, "arm_fir_lattice_" #T "_batch"); \
  }
MI355X_LATTICE(f32, float32_t, kLatF32)
MI355X_LATTICE(q31, q31_t, kLatQ31)
MI355X_LATTICE(q15, q15_t, kLatQ15)
#undef MI355X_LATTICE
// biquad cascades: NAME the processing function, INST its instance, PS the postShift expression
#define MI355X_BIQUAD(NAME, INST, CT, ST, OP, CH, KS, NC, PS)                                           \
  void NAME(const INST* S, const CT* pSrc, CT* pDst, uint32_t blockSize) {                              \
    biquad_sync<CT, ST>(S, S ? (int)(PS) : 0, pSrc, pDst, blockSize, OP, CH, KS, NC, #NAME);            \
  }                                                                                                     \
  arm_status NAME##_batch(const INST* S, const CT* d_src, CT* d_dst, uint32_t blockSize, uint32_t batch, \
                          ST* d_state, void* stream) {                                                  \
    return biquad_batch<CT, ST>(S, S ? (int)(PS) : 0, d_src, d_dst, blockSize, batch, d_state, stream, OP, NC, \
                                #NAME "_batch");                                                        \
  }
MI355X_BIQUAD(arm_biquad_cascade_df1_f32, arm_biquad_casd_df1_inst_f32, float32_t, float32_t, kBqDf1F32, 1, 4, 5, 0)
MI355X_BIQUAD(arm_biquad_cascade_df1_q31, arm_biquad_casd_df1_inst_q31, q31_t, q31_t, kBqDf1Q31, 1, 4, 5, S->postShift)
MI355X_BIQUAD(arm_biquad_cascade_df1_fast_q31, arm_biquad_casd_df1_inst_q31, q31_t, q31_t, kBqDf1FastQ31, 1, 4, 5,
              S->postShift)
MI355X_BIQUAD(arm_biquad_cascade_df1_q15, arm_biquad_casd_df1_inst_q15, q15_t, q15_t, kBqDf1Q15, 1, 4, 6, S->postShift)
MI355X_BIQUAD(arm_biquad_cascade_df1_fast_q15, arm_biquad_casd_df1_inst_q15, q15_t, q15_t, kBqDf1FastQ15, 1, 4, 6,
              S->postShift)
MI355X_BIQUAD(arm_biquad_cas_df1_32x64_q31, arm_biquad_cas_df1_32x64_ins_q31, q31_t, q63_t, kBq32x64, 1, 4, 5,
              S->postShift)
MI355X_BIQUAD(arm_biquad_cascade_df2T_f32, arm_biquad_cascade_df2T_instance_f32, float32_t, float32_t, kBqDf2TF32, 1, 2,
              5, 0)
MI355X_BIQUAD(arm_biquad_cascade_stereo_df2T_f32, arm_biquad_cascade_stereo_df2T_instance_f32, float32_t, float32_t,
              kBqStereoDf2TF32, 2, 4, 5, 0)
#undef MI355X_BIQUAD
void arm_biquad_cascade_df1_init_f32(arm_biquad_casd_df1_inst_f32* S, uint8_t numStages, const float32_t* pCoeffs,
                                     float32_t* pState) {
  biquad_init(S, numStages, pCoeffs, pState, 4, "arm_biquad_cascade_df1_init_f32");
}
void arm_biquad_cascade_df1_init_q31(arm_biquad_casd_df1_inst_q31* S, uint8_t numStages, const q31_t* pCoeffs,
                                     q31_t* pState, int8_t postShift) {
  biquad_init(S, numStages, pCoeffs, pState, 4, "arm_biquad_cascade_df1_init_q31");
  if (S) S->postShift = (uint8_t)postShift;
}
void arm_biquad_cascade_df1_init_q15(arm_biquad_casd_df1_inst_q15* S, uint8_t numStages, const q15_t* pCoeffs,
                                     q15_t* pState, int8_t postShift) {
  biquad_init(S, numStages, pCoeffs, pState, 4, "arm_biquad_cascade_df1_init_q15");
  if (S) S->postShift = postShift;
}
void arm_biquad_cas_df1_32x64_init_q31(arm_biquad_cas_df1_32x64_ins_q31* S, uint8_t numStages, const q31_t* pCoeffs,
                                       q63_t* pState, uint8_t postShift) {
  biquad_init(S, numStages, pCoeffs, pState, 4, "arm_biquad_cas_df1_32x64_init_q31");
  if (S) S->postShift = postShift;
}
void arm_biquad_cascade_df2T_init_f32(arm_biquad_cascade_df2T_instance_f32* S, uint8_t numStages,
                                      const float32_t* pCoeffs, float32_t* pState) {
  biquad_init(S, numStages, pCoeffs, pState, 2, "arm_biquad_cascade_df2T_init_f32");
}
void arm_biquad_cascade_stereo_df2T_init_f32(arm_biquad_cascade_stereo_df2T_instance_f32* S, uint8_t numStages,
                                             const float32_t* pCoeffs, float32_t* pState) {
  biquad_init(S, numStages, pCoeffs, pState, 4, "arm_biquad_cascade_stereo_df2T_init_f32");
}
// IIR lattice
#define MI355X_IIR_LATTICE(T, CT, OP)                                                                    \
  void arm_iir_lattice_init_##T(arm_iir_lattice_instance_##T* S, uint16_t numStages, CT* pkCoeffs,      \
                                CT* pvCoeffs, CT* pState, uint32_t blockSize) {                         \
    iir_lattice_init(S, numStages, pkCoeffs, pvCoeffs, pState, blockSize);                              \
  }                                                                                                     \
  void arm_iir_lattice_##T(const arm_iir_lattice_instance_##T* S, const CT* pSrc, CT* pDst, uint32_t blockSize) { \
    iir_lattice_sync(S, pSrc, pDst, blockSize, OP, "arm_iir_lattice_" #T);                              \
  }                                                                                                     \
  arm_status arm_iir_lattice_##T##_batch(const arm_iir_lattice_instance_##T* S, const CT* d_src, CT* d_dst, \
                                         uint32_t blockSize, uint32_t batch, CT* d_state, void* stream) { \
    return iir_lattice_batch(S, d_src, d_dst, blockSize, batch, d_state, stream, OP, "arm_iir_lattice_" #T "_batch"); \
  }
MI355X_IIR_LATTICE(f32, float32_t, kIirF32)
MI355X_IIR_LATTICE(q31, q31_t, kIirQ31)
MI355X_IIR_LATTICE(q15, q15_t, kIirQ15)
#undef MI355X_IIR_LATTICE
// Initial values of arm_recip_q15: the mean of the reciprocals of the ends of [1 + i/64, 1 + (i+1)/64]
// in q15 with one integer bit, floor(2^20 (129 + 2 i) / ((64 + i)(65 + i))).
#define MI355X_R1(i) (int16_t)((1048576u * (129u + 2u * (i))) / ((64u + (i)) * (65u + (i))))
#define MI355X_R4(i) MI355X_R1(i), MI355X_R1((i) + 1u), MI355X_R1((i) + 2u), MI355X_R1((i) + 3u)
#define MI355X_R16(i) MI355X_R4(i), MI355X_R4((i) + 4u), MI355X_R4((i) + 8u), MI355X_R4((i) + 12u)
const int16_t armRecipTableQ15[64] = {MI355X_R16(0u), MI355X_R16(16u), MI355X_R16(32u), MI355X_R16(48u)};
#undef MI355X_R16
#undef MI355X_R4
#undef MI355X_R1
// LMS: KIND lms | lms_norm, SC const for the plain kinds, EX the instance's {energy, x0} words
#define MI355X_LMS(KIND, T, CT, SC, EXIN, EXOUT)                                                            \
  void arm_##KIND##_##T(SC arm_##KIND##_instance_##T* S, const CT* pSrc, CT* pRef, CT* pOut, CT* pErr,     \
                        uint32_t blockSize) {                                                               \
    if (!S) return;                                                                                         \
    CT ex[2] = {0, 0};                                                                                      \
    CT* pex = nullptr;                                                                                      \
    EXIN;                                                                                                   \
    adaptive_sync<CT>(lms_params(S), S->pCoeffs, S->pState, pSrc, pRef, pOut, pErr, blockSize, pex,         \
                      "arm_" #KIND "_" #T);                                                                 \
    EXOUT;                                                                                                  \
  }
#define MI355X_EX_IN ex[0] = S->energy; ex[1] = S->x0; pex = ex
#define MI355X_EX_OUT S->energy = ex[0]; S->x0 = ex[1]
MI355X_LMS(lms, f32, float32_t, const, (void)ex, (void)pex)
MI355X_LMS(lms, q31, q31_t, const, (void)ex, (void)pex)
MI355X_LMS(lms, q15, q15_t, const, (void)ex, (void)pex)
MI355X_LMS(lms_norm, f32, float32_t, , MI355X_EX_IN, MI355X_EX_OUT)
MI355X_LMS(lms_norm, q15, q15_t, , MI355X_EX_IN, MI355X_EX_OUT)
#undef MI355X_EX_OUT
#undef MI355X_EX_IN
#undef MI355X_LMS
#define MI355X_LMS_BATCH(KIND, T, CT)                                                                       \
  arm_status arm_##KIND##_##T##_batch(const arm_##KIND##_instance_##T* S, const CT* d_src, const CT* d_ref, \
                                      CT* d_out, CT* d_err, uint32_t blockSize, uint32_t batch, CT* d_coeffs, \
                                      CT* d_state, void* stream) {                                          \
    if (!S) return ARM_MATH_ARGUMENT_ERROR;                                                                 \
    return adaptive_batch<CT>(lms_params(S), d_src, d_ref, d_out, d_err, blockSize, batch, d_coeffs, d_state, \
                              nullptr, stream, "arm_" #KIND "_" #T "_batch");                               \
  }
MI355X_LMS_BATCH(lms, f32, float32_t)
MI355X_LMS_BATCH(lms, q31, q31_t)
MI355X_LMS_BATCH(lms, q15, q15_t)
#undef MI355X_LMS_BATCH
#define MI355X_LMS_NORM_BATCH(T, CT)                                                                        \
  arm_status arm_lms_norm_##T##_batch(const arm_lms_norm_instance_##T* S, const CT* d_src, const CT* d_ref, \
                                      CT* d_out, CT* d_err, uint32_t blockSize, uint32_t batch, CT* d_coeffs, \
                                      CT* d_state, CT* d_energy_x0, void* stream) {                         \
    if (!S) return ARM_MATH_ARGUMENT_ERROR;                                                                 \
    return adaptive_batch<CT>(lms_params(S), d_src, d_ref, d_out, d_err, blockSize, batch, d_coeffs, d_state, \
                              d_energy_x0, stream, "arm_lms_norm_" #T "_batch");                            \
  }
MI355X_LMS_NORM_BATCH(f32, float32_t)
MI355X_LMS_NORM_BATCH(q15, q15_t)
#undef MI355X_LMS_NORM_BATCH
void arm_lms_init_f32(arm_lms_instance_f32* S, uint16_t numTaps, float32_t* pCoeffs, float32_t* pState, float32_t mu,
                      uint32_t blockSize) {
  if (S) lms_init(S, numTaps, pCoeffs, pState, mu, blockSize);
}
void arm_lms_init_q31(arm_lms_instance_q31* S, uint16_t numTaps, q31_t* pCoeffs, q31_t* pState, q31_t mu,
                      uint32_t blockSize, uint32_t postShift) {
  if (!S) return;
  lms_init(S, numTaps, pCoeffs, pState, mu, blockSize);
  S->postShift = postShift;
}
void arm_lms_init_q15(arm_lms_instance_q15* S, uint16_t numTaps, q15_t* pCoeffs, q15_t* pState, q15_t mu,
                      uint32_t blockSize, uint32_t postShift) {
  if (!S) return;
  lms_init(S, numTaps, pCoeffs, pState, mu, blockSize);
  S->postShift = postShift;
}
void arm_lms_norm_init_f32(arm_lms_norm_instance_f32* S, uint16_t numTaps, float32_t* pCoeffs, float32_t* pState,
                           float32_t mu, uint32_t blockSize) {
  if (!S) return;
  lms_init(S, numTaps, pCoeffs, pState, mu, blockSize);
  S->energy = 0.0f;
  S->x0 = 0.0f;
}
void arm_lms_norm_init_q15(arm_lms_norm_instance_q15* S, uint16_t numTaps, q15_t* pCoeffs, q15_t* pState, q15_t mu,
                           uint32_t blockSize, uint8_t postShift) {
  if (!S) return;
  lms_init(S, numTaps, pCoeffs, pState, mu, blockSize);
  S->postShift = postShift;
  S->recipTable = armRecipTableQ15;
  S->energy = 0;
  S->x0 = 0;
}
void arm_fir_sparse_f32(arm_fir_sparse_instance_f32* S, const float32_t* pSrc, float32_t* pDst, float32_t* pScratchIn,
                        uint32_t blockSize) {
  (void)pScratchIn;
  sparse_sync(S, pSrc, pDst, blockSize, kSpF32, "arm_fir_sparse_f32");
}
void arm_fir_sparse_q31(arm_fir_sparse_instance_q31* S, const q31_t* pSrc, q31_t* pDst, q31_t* pScratchIn,
                        uint32_t blockSize) {
  (void)pScratchIn;
  sparse_sync(S, pSrc, pDst, blockSize, kSpQ31, "arm_fir_sparse_q31");
}
void arm_fir_sparse_q15(arm_fir_sparse_instance_q15* S, const q15_t* pSrc, q15_t* pDst, q15_t* pScratchIn,
                        q31_t* pScratchOut, uint32_t blockSize) {
  (void)pScratchIn; (void)pScratchOut;
  sparse_sync(S, pSrc, pDst, blockSize, kSpQ15, "arm_fir_sparse_q15");
}
void arm_fir_sparse_q7(arm_fir_sparse_instance_q7* S, const q7_t* pSrc, q7_t* pDst, q7_t* pScratchIn,
                       q31_t* pScratchOut, uint32_t blockSize) {
  (void)pScratchIn; (void)pScratchOut;
  sparse_sync(S, pSrc, pDst, blockSize, kSpQ7, "arm_fir_sparse_q7");
}

}  // extern "C"
