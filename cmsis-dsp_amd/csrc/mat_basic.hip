// arm_mat_{add,sub,scale}_{f32,q31,q15}, arm_mat_trans_{f32,q31,q15,q7}, arm_mat_cmplx_trans_{f32,q31,q15} and
// arm_mat_vec_mult_{f32,q31,q15,q7} over a batch of contiguous row-major items, bit-exact with the reference's
// scalar branches (Source/MatrixFunctions/arm_mat_add_*.c, arm_mat_sub_*.c, arm_mat_scale_*.c, arm_mat_trans_*.c,
// arm_mat_cmplx_trans_*.c, arm_mat_vec_mult_*.c, the #else of ARM_MATH_MVE* / ARM_MATH_NEON, no ARM_MATH_DSP).
//
//   element-wise   one streaming kernel over the batch's words as one flat array, templated on the operation and
//                  the type: 16-B loads and stores when every pointer is 16-B aligned, four of them in flight
//                  per lane; one element per lane otherwise and for the ragged end.  A lane reads its elements
//                  before it writes them, so dst may be a source exactly.
//   transposes     pure data movement, templated on the element size (1, 2, 4, 8 bytes; a complex element is one
//                  (re, im) pair).  Items above kTransPackMax elements go through a padded LDS tile, one tile per
//                  workgroup; smaller items are packed kTransPackElems / n to a workgroup, which then reads and
//                  writes one contiguous chunk.  Both sides move aligned 4-B words (8-B for the 8-byte element)
//                  wherever a word lies wholly inside the row segment, single elements at its ragged ends.
//   vec_mult       one lane per (row, item); the workgroup stages a tile of matrix rows and the matching piece of
//                  the vectors in LDS with row-segment loads (16-B loads when every row is 16-B aligned), then
//                  every lane walks its own padded LDS row in k order, 16 bytes per read.  With matStride == 0
//                  the matrix tile is loaded once and shared by the workgroup's items.
//                  f32: sum = sum + a * v, product rounded first (arm_mat_vec_mult_f32.c:322-389).  q31: the sum
//                  mod 2^64, >> 31.  q7: an int32 sum, ssat8(sum >> 7).  q15: __SMLALD pairs whose two products
//                  are added in wrapping int32 first (none.h), rows of the 4-row groups pairing (0,1),(2,3),...
//                  and tail rows pairing only inside whole groups of four columns.  q15 and q31 keep the
//                  reference's uint16_t row offset (arm_mat_vec_mult_q15.c:280, _q31.c:277).
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

// ---- element-wise -------------------------------------------------------------------------------------
struct EwParam {
  float fscale;
  int32_t scale;   // scaleFract
  int shift;       // q31: shift + 1 (0..31); q15: 15 - shift (0..31)
};

template <int OP, typename T>
__device__ __forceinline__ T ew_op(T a, T b, const EwParam& p) {
  if constexpr (std::is_same<T, float>::value) {
    return OP == kMatAdd ? a + b : OP == kMatSub ? a - b : a * p.fscale;
  } else if constexpr (std::is_same<T, int32_t>::value) {
    if constexpr (OP == kMatScale) {            // arm_mat_scale_q31.c:173-178
      const int32_t in = mulhi(a, p.scale);
      int32_t out = wshl(in, p.shift);
      if (in != (out >> p.shift)) out = 0x7FFFFFFF ^ (in >> 31);
      return out;
    } else {                                    // __QADD / __QSUB (none.h clip_q63_to_q31)
      const int64_t s = OP == kMatAdd ? (int64_t)a + b : (int64_t)a - b;
      return s > 0x7FFFFFFFLL ? 0x7FFFFFFF : (s < -0x80000000LL ? (int32_t)0x80000000 : (int32_t)s);
    }
  } else {
    if constexpr (OP == kMatScale) return (T)ssat16(((int32_t)a * p.scale) >> p.shift);
    return (T)ssat16(OP == kMatAdd ? (int32_t)a + b : (int32_t)a - b);
  }
}

constexpr int kEwUnroll = 4;   // 16-B packs per lane and tile

// A workgroup takes a tile of kEwUnroll * kBlock consecutive packs (16 KiB per operand); a lane loads its
// kEwUnroll packs, kBlock packs apart, before it stores any of them.  One tile per workgroup (the loop only
// runs again past 2^31 tiles): on 1 GiB this measured faster than 2048 workgroups striding over the tiles and
// than one pack per lane and step.
template <int OP, typename T>
__global__ __launch_bounds__(kBlock) void mat_ew_kernel(const T* a, const T* b, T* d, size_t count, bool vec,
                                                        EwParam p) {
  constexpr int V = 16 / sizeof(T), U = kEwUnroll;
  struct alignas(16) Pack { T v[V]; };
  const size_t packs = vec ? count / V : 0;
  for (size_t tile = blockIdx.x; tile * (U * kBlock) < packs; tile += gridDim.x) {
    const size_t i0 = tile * (U * kBlock) + threadIdx.x;
    Pack x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * kBlock;
      if (i < packs) {
        x[u] = ((const Pack*)a)[i];
        if constexpr (OP != kMatScale) y[u] = ((const Pack*)b)[i]; else y[u] = x[u];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * kBlock;
      if (i < packs) {
        Pack r;
#pragma unroll
        for (int j = 0; j < V; ++j) r.v[j] = ew_op<OP, T>(x[u].v[j], y[u].v[j], p);
        ((Pack*)d)[i] = r;
      }
    }
  }
  // the ragged end, or everything when a pointer is not 16-B aligned: one element per lane
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = packs * V + (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
    const T x = a[i];
    T y = x;
    if constexpr (OP != kMatScale) y = b[i];
    d[i] = ew_op<OP, T>(x, y, p);
  }
}

template <int OP, typename T>
hipError_t ew_launch(const T* a, const T* b, T* d, size_t count, const EwParam& p, hipStream_t st) {
  const bool vec = (((uintptr_t)a | (uintptr_t)(OP == kMatScale ? a : b) | (uintptr_t)d) & 15) == 0;
  constexpr size_t V = 16 / sizeof(T);
  const size_t per = vec ? V * kEwUnroll * kBlock : kBlock;     // elements a workgroup takes per step
  const size_t blocks = (count + per - 1) / per;
  const size_t cap = 0x7fffffff;
  const uint32_t grid = (uint32_t)(blocks < cap ? blocks : cap);
  hipLaunchKernelGGL((mat_ew_kernel<OP, T>), dim3(grid), dim3(kBlock), 0, st, a, b, d, count, vec, p);
  return hipGetLastError();
}

// ---- transposes ----------------------------------------------------------------------------------------
constexpr int kTransPackMax = 256;      // items of at most this many elements are packed
constexpr int kTransPackElems = 1024;   // elements of one packed workgroup

template <int B> struct Elem;
template <> struct Elem<1> { using type = uint8_t; };
template <> struct Elem<2> { using type = uint16_t; };
template <> struct Elem<4> { using type = uint32_t; };
// two words: a complex f32 / q31 element is only 4-byte aligned
struct alignas(4) Elem8 { uint32_t re, im; };
template <> struct Elem<8> { using type = Elem8; };

// One row segment of `len` elements at g (global), moved by the workgroup's lane `w` of the segment in aligned
// words of W = max(4, sizeof(E)) bytes: word w of the segment's aligned cover holds elements [x, x + P) of the
// segment; it moves as one word when all of them lie inside, element by element otherwise.  at(x) is the
// element's LDS slot.
template <typename E, bool LOAD, typename At>
__device__ __forceinline__ void seg_word(E* g, int len, int w, At&& at) {
  constexpr int P = sizeof(E) >= 4 ? 1 : 4 / (int)sizeof(E);
  if constexpr (P == 1) {
    if (w < len) {
      if constexpr (LOAD) at(w) = g[w]; else g[w] = at(w);
    }
  } else {
    const int head = (int)(((uintptr_t)g & 3) / sizeof(E));   // elements of the first word that precede g
    const int x = w * P - head;
    if (x >= len || x + P <= 0) return;
    if (x >= 0 && x + P <= len) {
      uint32_t word;
      if constexpr (LOAD) {
        word = *(const uint32_t*)(g + x);
#pragma unroll
        for (int e = 0; e < P; ++e) at(x + e) = (E)(word >> (8 * sizeof(E) * e));
      } else {
        word = 0;
#pragma unroll
        for (int e = 0; e < P; ++e) word |= (uint32_t)at(x + e) << (8 * sizeof(E) * e);
        *(uint32_t*)(g + x) = word;
      }
    } else {
      for (int e = 0; e < P; ++e) {
        const int xe = x + e;
        if (xe >= 0 && xe < len) {
          if constexpr (LOAD) at(xe) = g[xe]; else g[xe] = at(xe);
        }
      }
    }
  }
}

// Tile path: grid.x = tiles of one item, grid.y strides over the items.  T x T elements, LDS rows padded by
// one word; the tile's source rows are read as row segments, its destination rows (source columns) written
// as row segments, lanes running along the segment on both sides.
template <int B>
__global__ __launch_bounds__(kBlock) void mat_trans_tile_kernel(const void* srcv, void* dstv, int rows, int cols,
                                                                uint32_t batch) {
  using E = typename Elem<B>::type;
  constexpr int T = B <= 2 ? 64 : 32, P = B >= 4 ? 1 : 4 / B, LD = T + P, WPR = T / P + (P > 1 ? 1 : 0);
  __shared__ __align__(16) E tile[T * LD];
  const int tc = (cols + T - 1) / T;
  const int r0 = (int)(blockIdx.x / tc) * T, c0 = (int)(blockIdx.x % tc) * T;
  const int th = min(T, rows - r0), tw = min(T, cols - c0);
  const size_t n = (size_t)rows * cols;
  for (uint32_t item = blockIdx.y; item < batch; item += gridDim.y) {
    const E* s = (const E*)srcv + item * n;
    E* d = (E*)dstv + item * n;
    for (int idx = threadIdx.x; idx < th * WPR; idx += kBlock) {
      const int i = idx / WPR, w = idx - i * WPR;
      seg_word<E, true>(const_cast<E*>(s) + (size_t)(r0 + i) * cols + c0, tw, w,
                        [&](int x) -> E& { return tile[i * LD + x]; });
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < tw * WPR; idx += kBlock) {
      const int j = idx / WPR, w = idx - j * WPR;
      seg_word<E, false>(d + (size_t)(c0 + j) * rows + r0, th, w, [&](int y) -> E& { return tile[y * LD + j]; });
    }
    __syncthreads();
  }
}

// f / x for f < 2^16 and x <= 256 as a multiplication by m = 2^32 / x + 1 (exact: the error term f / 2^32 is
// below 1 / x).
__device__ __forceinline__ int div_by(int f, uint64_t m) { return (int)(((uint64_t)(uint32_t)f * m) >> 32); }
inline uint64_t div_magic(int x) { return (uint64_t(1) << 32) / (uint32_t)x + 1; }

// Packed path (rows * cols <= kTransPackMax): a workgroup owns ipw consecutive items, one contiguous chunk on
// both sides.  LDS keeps each item with an odd row stride.  mn, mc, mr: div_magic of n, cols, rows.
template <int B>
__global__ __launch_bounds__(kBlock) void mat_trans_pack_kernel(const void* srcv, void* dstv, int rows, int cols,
                                                                uint32_t batch, int ipw, uint64_t mn, uint64_t mc,
                                                                uint64_t mr) {
  using E = typename Elem<B>::type;
  constexpr int P = B >= 4 ? 1 : 4 / B;
  __shared__ __align__(16) E lds[2 * kTransPackElems];
  const int n = rows * cols, ld = cols | 1, isz = rows * ld;
  const uint32_t item0 = blockIdx.x * (uint32_t)ipw;
  const int cnt = (int)min((uint32_t)ipw, batch - item0);
  const int len = cnt * n, words = len / P + 2;
  const E* s = (const E*)srcv + (size_t)item0 * n;
  E* d = (E*)dstv + (size_t)item0 * n;
  for (int w = threadIdx.x; w < words; w += kBlock)
    seg_word<E, true>(const_cast<E*>(s), len, w, [&](int f) -> E& {
      const int it = div_by(f, mn), in = f - it * n, r = div_by(in, mc);
      return lds[it * isz + r * ld + (in - r * cols)];
    });
  __syncthreads();
  for (int w = threadIdx.x; w < words; w += kBlock)
    seg_word<E, false>(d, len, w, [&](int f) -> E& {
      const int it = div_by(f, mn), in = f - it * n, c = div_by(in, mr);
      return lds[it * isz + (in - c * rows) * ld + c];
    });
}

template <int B>
hipError_t trans_launch(int rows, int cols, const void* src, void* dst, uint32_t batch, hipStream_t st) {
  const size_t n = (size_t)rows * cols;
  if (n <= kTransPackMax) {
    const int ipw = kTransPackElems / (int)n;
    const uint32_t grid = (uint32_t)(((uint64_t)batch + ipw - 1) / ipw);
    hipLaunchKernelGGL((mat_trans_pack_kernel<B>), dim3(grid), dim3(kBlock), 0, st, src, dst, rows, cols, batch, ipw,
                       div_magic((int)n), div_magic(cols), div_magic(rows));
  } else {
    constexpr int T = B <= 2 ? 64 : 32;
    const uint32_t tiles = (uint32_t)((rows + T - 1) / T) * (uint32_t)((cols + T - 1) / T);
    hipLaunchKernelGGL((mat_trans_tile_kernel<B>), dim3(tiles, batch < 65535u ? batch : 65535u), dim3(kBlock), 0, st,
                       src, dst, rows, cols, batch);
  }
  return hipGetLastError();
}

// ---- matrix x vector ---------------------------------------------------------------------------------
// A row segment is 128 bytes: KT = 128 / sizeof(T) columns per step.  Every lane-row of the LDS tile is
// 128 + 16 bytes: 16-B aligned, and the 16-B reads of 16 consecutive lane-rows cover the 64 banks once.
constexpr int kVmMinRtLog = 2, kVmMaxItems = kBlock >> kVmMinRtLog;   // a workgroup holds at most 64 items
template <typename T> struct VmAcc { using type = int64_t; };
template <> struct VmAcc<float> { using type = float; };
template <> struct VmAcc<int8_t> { using type = int32_t; };

// Element offset of row r inside an item.  WRAP: the reference's uint16_t `i` -- a 4-row group starts at
// (4 g cols) mod 65536 and its rows follow at + cols each, a tail row starts at (r cols) mod 65536.
template <bool WRAP>
__device__ __forceinline__ uint32_t vm_row_offset(uint32_t r, uint32_t rows, uint32_t cols) {
  if constexpr (!WRAP) return r * cols;
  if (r < (rows & ~3u)) return (((r & ~3u) * cols) & 0xFFFFu) + (r & 3u) * cols;
  return (r * cols) & 0xFFFFu;
}

// wide: every row segment and vector is 16-B aligned and cols is a multiple of 16 / sizeof(T), so the tiles are
// staged with 16-B loads (a 16-B piece is then wholly inside the row or wholly outside); else element by element.
template <typename T, bool SHARED>
__global__ __launch_bounds__(kBlock) void mat_vec_mult_kernel(const T* mat, size_t matStride, const T* vec, T* dst,
                                                              int rows, int cols, uint32_t batch, int rtLog,
                                                              bool wide) {
  constexpr int KT = 128 / sizeof(T), KV = 16 / sizeof(T), LD = KT + KV;
  constexpr bool WRAP = std::is_same<T, int16_t>::value || std::is_same<T, int32_t>::value;
  using Acc = typename VmAcc<T>::type;
  struct alignas(16) Piece { T v[KV]; };
  __shared__ __align__(16) T am[kBlock * LD];
  __shared__ __align__(16) T vm[kVmMaxItems * LD];
  const int RT = 1 << rtLog, IT = kBlock >> rtLog;
  const int lr = threadIdx.x & (RT - 1), li = threadIdx.x >> rtLog;
  const uint32_t row0 = blockIdx.y * (uint32_t)RT, item0 = blockIdx.x * (uint32_t)IT;
  const uint32_t row = row0 + lr, item = item0 + li;
  const bool live = row < (uint32_t)rows && item < batch;
  // q15: columns below pairEnd are summed in pairs (arm_mat_vec_mult_q15.c:303-338 / :361-378)
  const int pairEnd = row < ((uint32_t)rows & ~3u) ? (cols & ~1) : (cols & ~3);
  const T* arow = am + (SHARED ? lr : (int)threadIdx.x) * LD;
  const T* vrow = vm + li * LD;
  const int per = wide ? KV : 1;        // columns per load
  Acc sum = 0;
  for (int k0 = 0; k0 < cols; k0 += KT) {
    const int kc = min(KT, cols - k0);
    int cl = 0;                         // loads per row, rounded up to a power of two
    while ((per << cl) < kc) ++cl;
    for (int idx = threadIdx.x; idx < ((SHARED ? RT : kBlock) << cl); idx += kBlock) {
      const int l = idx >> cl, k = (idx & ((1 << cl) - 1)) * per;
      const uint32_t r = row0 + (l & (RT - 1)), it = item0 + (l >> rtLog);
      if (k < kc && r < (uint32_t)rows && it < batch) {
        const T* g = mat + (SHARED ? 0 : it * matStride) + vm_row_offset<WRAP>(r, rows, cols) + k0 + k;
        if (wide) *(Piece*)(am + l * LD + k) = *(const Piece*)g;
        else am[l * LD + k] = *g;
      }
    }
    for (int idx = threadIdx.x; idx < (IT << cl); idx += kBlock) {
      const int l = idx >> cl, k = (idx & ((1 << cl) - 1)) * per;
      const uint32_t it = item0 + l;
      if (k < kc && it < batch) {
        const T* g = vec + (size_t)it * cols + k0 + k;
        if (wide) *(Piece*)(vm + l * LD + k) = *(const Piece*)g;
        else vm[l * LD + k] = *g;
      }
    }
    __syncthreads();
    if (live) {
      // 16-B LDS reads; the words past kc in the last piece are stale and are not used
      for (int k = 0; k < kc; k += KV) {
        const Piece a = *(const Piece*)(arow + k), v = *(const Piece*)(vrow + k);
        if constexpr (std::is_same<T, int16_t>::value) {
          // k0, k and pairEnd are even, so a pair never straddles two pieces
#pragma unroll
          for (int j = 0; j < KV; j += 2) {
            const int32_t p0 = (int32_t)a.v[j] * v.v[j], p1 = (int32_t)a.v[j + 1] * v.v[j + 1];
            if (k0 + k + j < pairEnd) {
              sum += (int64_t)wadd(p0, p1);
            } else {
              if (k + j < kc) sum += (int64_t)p0;
              if (k + j + 1 < kc) sum += (int64_t)p1;
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < KV; ++j) {
            if (k + j < kc) {
              if constexpr (std::is_same<T, float>::value) sum = sum + a.v[j] * v.v[j];
              else if constexpr (std::is_same<T, int32_t>::value)
                sum = (int64_t)((uint64_t)sum + (uint64_t)((int64_t)a.v[j] * v.v[j]));
              else sum += (int32_t)a.v[j] * v.v[j];
            }
          }
        }
      }
    }
    __syncthreads();
  }
  if (live) {
    T out;
    if constexpr (std::is_same<T, float>::value) out = sum;
    else if constexpr (std::is_same<T, int32_t>::value) out = (int32_t)(sum >> 31);
    else if constexpr (std::is_same<T, int8_t>::value) out = (int8_t)ssat8(sum >> 7);
    else {
      const int64_t v = sum >> 15;
      out = (int16_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
    }
    dst[(size_t)item * rows + row] = out;
  }
}

}  // namespace

template <typename T>
hipError_t mat_ew_launch(int op, const T* a, const T* b, T* d, size_t count, T scale, int shift, hipStream_t st) {
  if (count == 0) return hipSuccess;
  EwParam p{0.0f, 0, 0};
  if constexpr (std::is_same<T, float>::value) p.fscale = scale;
  else { p.scale = scale; p.shift = sizeof(T) == 4 ? shift + 1 : 15 - shift; }
  if (op == kMatScale && (p.shift < 0 || p.shift > 31)) return hipErrorInvalidValue;
  switch (op) {
    case kMatAdd: return ew_launch<kMatAdd, T>(a, b, d, count, p, st);
    case kMatSub: return ew_launch<kMatSub, T>(a, b, d, count, p, st);
    case kMatScale: return ew_launch<kMatScale, T>(a, nullptr, d, count, p, st);
  }
  return hipErrorInvalidValue;
}
template hipError_t mat_ew_launch<float>(int, const float*, const float*, float*, size_t, float, int, hipStream_t);
template hipError_t mat_ew_launch<int32_t>(int, const int32_t*, const int32_t*, int32_t*, size_t, int32_t, int,
                                           hipStream_t);
template hipError_t mat_ew_launch<int16_t>(int, const int16_t*, const int16_t*, int16_t*, size_t, int16_t, int,
                                           hipStream_t);

hipError_t mat_trans_launch(int elemBytes, int rows, int cols, const void* src, void* dst, uint32_t batch,
                            hipStream_t st) {
  if (rows <= 0 || cols <= 0 || batch == 0) return hipSuccess;
  switch (elemBytes) {
    case 1: return trans_launch<1>(rows, cols, src, dst, batch, st);
    case 2: return trans_launch<2>(rows, cols, src, dst, batch, st);
    case 4: return trans_launch<4>(rows, cols, src, dst, batch, st);
    case 8: return trans_launch<8>(rows, cols, src, dst, batch, st);
  }
  return hipErrorInvalidValue;
}

template <typename T>
hipError_t mat_vec_mult_launch(int rows, int cols, const T* mat, size_t matStride, const T* vec, T* dst,
                               uint32_t batch, hipStream_t st) {
  if (rows <= 0 || batch == 0) return hipSuccess;
  int rtLog = kVmMinRtLog;
  while (rtLog < 8 && (1 << rtLog) < rows) ++rtLog;
  const uint32_t ipw = kBlock >> rtLog;
  const uint64_t gx = ((uint64_t)batch + ipw - 1) / ipw;
  if (gx > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)gx, (uint32_t)((rows + (1 << rtLog) - 1) >> rtLog));
  const bool wide = cols > 0 && (((uintptr_t)mat | (uintptr_t)vec | (matStride * sizeof(T)) |
                                 ((size_t)cols * sizeof(T))) & 15) == 0;
  if (matStride == 0)
    hipLaunchKernelGGL((mat_vec_mult_kernel<T, true>), grid, dim3(kBlock), 0, st, mat, matStride, vec, dst, rows, cols,
                       batch, rtLog, wide);
  else
    hipLaunchKernelGGL((mat_vec_mult_kernel<T, false>), grid, dim3(kBlock), 0, st, mat, matStride, vec, dst, rows,
                       cols, batch, rtLog, wide);
  return hipGetLastError();
}
template hipError_t mat_vec_mult_launch<float>(int, int, const float*, size_t, const float*, float*, uint32_t,
                                               hipStream_t);
template hipError_t mat_vec_mult_launch<int32_t>(int, int, const int32_t*, size_t, const int32_t*, int32_t*, uint32_t,
                                                 hipStream_t);
template hipError_t mat_vec_mult_launch<int16_t>(int, int, const int16_t*, size_t, const int16_t*, int16_t*, uint32_t,
                                                 hipStream_t);
template hipError_t mat_vec_mult_launch<int8_t>(int, int, const int8_t*, size_t, const int8_t*, int8_t*, uint32_t,
                                                hipStream_t);

}  // namespace mi355x
