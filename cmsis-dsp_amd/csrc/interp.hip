// arm_linear_interp_{f32,q31,q15,q7}, arm_bilinear_interp_{f32,q31,q15,q7}, arm_spline_init_f32 and arm_spline_f32,
// bit-exact with the reference's scalar code (Source/InterpolationFunctions, no FMA contraction).
//
//   The sample functions are written once, __host__ __device__: the drop-ins of arm_math.h take one sample and are
//   computed on the host (interp_*_host below), the _batch forms run the same text with one lane per sample.
//   linear        all samples of a call share one table.  It is staged in LDS where it fits 64 KiB (16384 f32 words;
//                 a fixed-point table reaches at most entry 2048, so it always fits) and read from global memory
//                 otherwise.  A workgroup stages once and then takes every gridDim.x-th tile of 256 samples.
//   bilinear      a gather: four table reads per point from global memory.
//   spline init   each item's forward chain li -> u[i] -> z[i] and backward chain c -> b, d is serial with two
//                 dependent divisions per knot: one lane per item, whatever the batch (lms.hip, iir_lattice.hip).  The
//                 items' arrays are n words apart, so a wave's accesses are not coalesced: untuned.
//   spline        the reference walks xq with a pointer that never goes back: the interval of output k is min(n - 2,
//                 max over j <= k of f(xq[j])), f(v) the first i with v <= x[i + 1], n - 1 where there is none (a NaN
//                 has none).  One wave per item: each lane finds f of its query by the reference's own scan, a wave
//                 scan forms the prefix maximum, and the maximum of a chunk of 64 is carried into the next.
#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

constexpr uint32_t kInterpLdsBytes = 65536;                  // the staged table's limit
constexpr uint32_t kInterpMaxGrid = 2048;                    // workgroups of a linear call

// float -> int32_t as the reference's cast where that is defined: toward zero; saturating by sign outside; NaN: 0
// (the rule of support.hip).
__host__ __device__ __forceinline__ int32_t cast_sat(float p) {
  if (!(p == p)) return 0;
  if (p >= 2147483648.0f) return INT32_MAX;
  if (p <= -2147483648.0f) return INT32_MIN;
  return (int32_t)p;
}
__host__ __device__ __forceinline__ int32_t hd_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__host__ __device__ __forceinline__ int32_t hd_shl(int32_t a, int s) { return (int32_t)((uint32_t)a << s); }
// the 12.20 split: the signed index and the fraction
__host__ __device__ __forceinline__ int32_t q_index(int32_t x) { return (int32_t)(x & (int32_t)0xFFF00000) >> 20; }
__host__ __device__ __forceinline__ int32_t q_fract(int32_t x) { return x & 0x000FFFFF; }

// arm_linear_interp_f32.c; nValues > 0
__host__ __device__ __forceinline__ float linear_f32(const float* tab, uint32_t nValues, float first, float spacing,
                                                     float x) {
  const int32_t i = cast_sat((x - first) / spacing);
  if (x < first) return tab[0];
  if ((uint32_t)i >= nValues - 1) return tab[nValues - 1];
  const float x0 = first + (float)i * spacing;
  const float x1 = first + (float)hd_add(i, 1) * spacing;   // i may be INT32_MAX where nValues - 1 is above it
  const float y0 = tab[i], y1 = tab[(size_t)i + 1];
  return y0 + (x - x0) * ((y1 - y0) / (x1 - x0));
}

// arm_linear_interp_q31.c / _q15.c / _q7.c; nValues > 0
__host__ __device__ __forceinline__ int32_t linear_q(const int32_t* tab, uint32_t nValues, int32_t x) {
  const int32_t index = q_index(x);
  if (index >= (int32_t)(nValues - 1)) return tab[nValues - 1];
  if (index < 0) return tab[0];
  const int32_t fract = hd_shl(q_fract(x), 11);
  const int32_t y0 = tab[index], y1 = tab[index + 1];
  int32_t y = (int32_t)(((int64_t)y0 * (0x7FFFFFFF - fract)) >> 32);
  y = hd_add(y, (int32_t)(((int64_t)y1 * fract) >> 32));
  return hd_shl(y, 1);
}
__host__ __device__ __forceinline__ int16_t linear_q(const int16_t* tab, uint32_t nValues, int32_t x) {
  const int32_t index = q_index(x);
  if (index >= (int32_t)(nValues - 1)) return tab[nValues - 1];
  if (index < 0) return tab[0];
  const int32_t fract = q_fract(x);
  const int16_t y0 = tab[index], y1 = tab[index + 1];
  int64_t y = (int64_t)y0 * (0xFFFFF - fract);
  y += (int64_t)y1 * fract;
  return (int16_t)(y >> 20);
}
__host__ __device__ __forceinline__ int8_t linear_q(const int8_t* tab, uint32_t nValues, int32_t x) {
  if (x < 0) return tab[0];
  const uint32_t index = (uint32_t)(x >> 20) & 0xfff;
  if (index >= nValues - 1) return tab[nValues - 1];
  const int32_t fract = q_fract(x);
  const int8_t y0 = tab[index], y1 = tab[index + 1];
  int32_t y = y0 * (0xFFFFF - fract);
  y += y1 * fract;
  return (int8_t)(y >> 20);
}

// arm_bilinear_interp_f32.c; rows * cols < 2^31
__host__ __device__ __forceinline__ float bilinear_f32(const float* tab, int32_t rows, int32_t cols, float X, float Y) {
  const int32_t xIndex = cast_sat(X), yIndex = cast_sat(Y);
  if (xIndex < 0 || xIndex > cols - 2 || yIndex < 0 || yIndex > rows - 2) return 0.0f;
  const size_t index = (size_t)xIndex + (size_t)yIndex * cols;
  const float f00 = tab[index], f01 = tab[index + 1], f10 = tab[index + cols], f11 = tab[index + cols + 1];
  const float b1 = f00, b2 = f01 - f00, b3 = f10 - f00, b4 = f00 - f01 - f10 + f11;
  const float xdiff = X - (float)xIndex, ydiff = Y - (float)yIndex;
  return b1 + b2 * xdiff + b3 * ydiff + b4 * xdiff * ydiff;
}

// The four table words of a fixed-point point, or false outside the table.  X bounds the column, Y the row, as in
// the reference (which names them rI and cI).
template <typename T>
__host__ __device__ __forceinline__ bool bilinear_words(const T* tab, int32_t rows, int32_t cols, int32_t X, int32_t Y,
                                                        T w[4]) {
  const int32_t rI = q_index(X), cI = q_index(Y);
  if (rI < 0 || rI > cols - 2 || cI < 0 || cI > rows - 2) return false;
  const size_t index = (size_t)rI + (size_t)cols * cI;
  w[0] = tab[index];
  w[1] = tab[index + 1];
  w[2] = tab[index + cols];
  w[3] = tab[index + cols + 1];
  return true;
}
__host__ __device__ __forceinline__ int32_t mul32(int32_t a, int32_t b) { return (int32_t)(((int64_t)a * b) >> 32); }

// arm_bilinear_interp_q31.c / _q15.c / _q7.c
__host__ __device__ __forceinline__ int32_t bilinear_q(const int32_t* tab, int32_t rows, int32_t cols, int32_t X,
                                                       int32_t Y) {
  int32_t w[4];
  if (!bilinear_words(tab, rows, cols, X, Y, w)) return 0;
  const int32_t xfract = hd_shl(q_fract(X), 11), yfract = hd_shl(q_fract(Y), 11);
  int32_t out = mul32(w[0], 0x7FFFFFFF - xfract);
  int32_t acc = mul32(out, 0x7FFFFFFF - yfract);
  out = mul32(w[1], 0x7FFFFFFF - yfract);
  acc = hd_add(acc, mul32(out, xfract));
  out = mul32(w[2], 0x7FFFFFFF - xfract);
  acc = hd_add(acc, mul32(out, yfract));
  out = mul32(w[3], xfract);
  acc = hd_add(acc, mul32(out, yfract));
  return hd_shl(acc, 2);
}
__host__ __device__ __forceinline__ int16_t bilinear_q(const int16_t* tab, int32_t rows, int32_t cols, int32_t X,
                                                       int32_t Y) {
  int16_t w[4];
  if (!bilinear_words(tab, rows, cols, X, Y, w)) return 0;
  const int32_t xfract = q_fract(X), yfract = q_fract(Y);
  int32_t out = (int32_t)(((int64_t)w[0] * (0x0FFFFF - xfract)) >> 4);
  int64_t acc = (int64_t)out * (0x0FFFFF - yfract);
  out = (int32_t)(((int64_t)w[1] * (0x0FFFFF - yfract)) >> 4);
  acc += (int64_t)out * xfract;
  out = (int32_t)(((int64_t)w[2] * (0x0FFFFF - xfract)) >> 4);
  acc += (int64_t)out * yfract;
  out = (int32_t)(((int64_t)w[3] * xfract) >> 4);
  acc += (int64_t)out * yfract;
  return (int16_t)(acc >> 36);
}
__host__ __device__ __forceinline__ int8_t bilinear_q(const int8_t* tab, int32_t rows, int32_t cols, int32_t X,
                                                      int32_t Y) {
  int8_t w[4];
  if (!bilinear_words(tab, rows, cols, X, Y, w)) return 0;
  const int32_t xfract = q_fract(X), yfract = q_fract(Y);
  int32_t out = w[0] * (0xFFFFF - xfract);
  int64_t acc = (int64_t)out * (0xFFFFF - yfract);
  out = w[1] * (0xFFFFF - yfract);
  acc += (int64_t)out * xfract;
  out = w[2] * (0xFFFFF - xfract);
  acc += (int64_t)out * yfract;
  out = w[3] * yfract;
  acc += (int64_t)out * xfract;
  return (int8_t)(acc >> 40);
}

// ---- kernels ---------------------------------------------------------------------------------------------------
// T: the table's and the result's type; X: the sample's (float for f32, int32_t for the fixed-point forms).
template <typename T, typename X>
__device__ __forceinline__ T linear_sample(const T* tab, uint32_t nValues, float first, float spacing, X x) {
  if constexpr (__is_same(X, float)) return linear_f32(tab, nValues, first, spacing, x);
  else return linear_q(tab, nValues, x);
}

template <typename T, typename X>
__global__ __launch_bounds__(kBlock) void linear_kernel(const T* table, uint32_t nValues, float first, float spacing,
                                                        const X* x, T* y, uint32_t count, bool staged) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const T* tab = table;
  if (staged) {                                              // uniform over the grid
    T* lds = (T*)lds_raw;
    for (uint32_t k = threadIdx.x; k < nValues; k += kBlock) lds[k] = table[k];
    __syncthreads();
    tab = lds;
  }
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride)
    y[i] = linear_sample<T, X>(tab, nValues, first, spacing, x[i]);
}

template <typename T, typename X>
__global__ __launch_bounds__(kBlock) void bilinear_kernel(const T* table, int32_t rows, int32_t cols, const X* px,
                                                          const X* py, T* out, uint32_t count) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  if constexpr (__is_same(X, float)) out[i] = bilinear_f32(table, rows, cols, px[i], py[i]);
  else out[i] = bilinear_q(table, rows, cols, px[i], py[i]);
}

// arm_spline_interp_init_f32.c, one lane per item; n >= 2, type 0 (natural) or 1 (parabolic runout).
__global__ __launch_bounds__(kBlock) void spline_init_kernel(int type, const float* px, size_t xStride, const float* py,
                                                             uint32_t n, float* pcoeffs, float* ptemp, uint32_t batch) {
  const size_t item = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (item >= batch) return;
  const float* x = px + item * xStride;
  const float* y = py + item * n;
  float* b = pcoeffs + item * 3 * (n - 1);
  float* c = b + (n - 1);
  float* d = b + 2 * (size_t)(n - 1);
  float* u = ptemp + item * (2 * (size_t)n - 1);
  float* z = u + (n - 1);
  float up = type == 0 ? 0.0f : -1.0f, zp = 0.0f;            // u[i - 1], z[i - 1]
  u[0] = up;
  z[0] = zp;
  float hm1 = x[1] - x[0];
  for (uint32_t i = 1; i + 1 < n; ++i) {
    const float hi = x[i + 1] - x[i];
    const float Bi = 3 * (y[i + 1] - y[i]) / hi - 3 * (y[i] - y[i - 1]) / hm1;
    const float li = 2 * (hi + hm1) - hm1 * up;
    up = hi / li;
    zp = (Bi - hm1 * zp) / li;
    u[i] = up;
    z[i] = zp;
    hm1 = hi;
  }
  float cp1;
  if (type == 0) {
    cp1 = 0.0f;
  } else {
    const float li = 1 + up;                                 // up: u[n - 2], zp: z[n - 2]
    cp1 = zp / li;
  }
  z[n - 1] = cp1;
  for (int64_t i = (int64_t)n - 2; i >= 0; --i) {
    const float ci = z[i] - u[i] * cp1;
    c[i] = ci;
    const float hi = x[i + 1] - x[i];
    b[i] = (y[i + 1] - y[i]) / hi - hi * (cp1 + 2 * ci) / 3;
    d[i] = (cp1 - ci) / (3 * hi);
    cp1 = ci;
  }
}

// arm_spline_interp_f32.c, one wave per item; n >= 2.
__global__ __launch_bounds__(kBlock) void spline_kernel(const float* px, size_t xStride, const float* py,
                                                        const float* pcoeffs, uint32_t n, const float* pxq,
                                                        size_t xqStride, float* pdst, uint32_t blockSize,
                                                        uint32_t batch) {
  const uint32_t lane = threadIdx.x & 63;
  const size_t item = (size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (item >= batch) return;                                 // wave-uniform; the kernel has no barrier
  const float* x = px + item * xStride;
  const float* y = py + item * n;
  const float* b = pcoeffs + item * 3 * (n - 1);
  const float* c = b + (n - 1);
  const float* d = b + 2 * (size_t)(n - 1);
  const float* xq = pxq + item * xqStride;
  float* dst = pdst + item * blockSize;
  uint32_t carry = 0;                                        // the maximum over the chunks before this one
  for (uint32_t k0 = 0; k0 < blockSize; k0 += 64) {          // k0 + lane cannot wrap: k0 <= blockSize - 1
    const uint64_t k = (uint64_t)k0 + lane;
    const bool valid = k < blockSize;
    const float v = valid ? xq[k] : 0.0f;
    uint32_t f = 0;
    if (valid)
      while (f < n - 1 && !(v <= x[f + 1])) ++f;
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t o = __shfl_up(f, s, 64);
      if (lane >= (uint32_t)s && o > f) f = o;
    }
    if (carry > f) f = carry;
    carry = __shfl(f, 63, 64);
    if (valid) {
      const uint32_t i = f < n - 2 ? f : n - 2;
      const float t = v - x[i];
      dst[k] = y[i] + b[i] * t + c[i] * t * t + d[i] * t * t * t;
    }
    if (k0 > 0xffffffffu - 64) break;
  }
}

template <typename T, typename X>
hipError_t linear_run(const T* table, uint32_t nValues, float first, float spacing, const X* x, T* y, uint32_t count,
                      hipStream_t st) {
  if (count == 0) return hipSuccess;
  if (nValues == 0) return hipErrorInvalidValue;
  const bool staged = (uint64_t)nValues * sizeof(T) <= kInterpLdsBytes;
  const uint32_t tiles = (uint32_t)(((uint64_t)count + kBlock - 1) / kBlock);
  const dim3 grid(tiles < kInterpMaxGrid ? tiles : kInterpMaxGrid);
  hipLaunchKernelGGL((linear_kernel<T, X>), grid, dim3(kBlock), staged ? nValues * sizeof(T) : 0, st, table, nValues,
                     first, spacing, x, y, count, staged);
  return hipGetLastError();
}

template <typename T, typename X>
hipError_t bilinear_run(const T* table, uint32_t rows, uint32_t cols, const X* px, const X* py, T* out, uint32_t count,
                        hipStream_t st) {
  if (count == 0) return hipSuccess;
  if ((uint64_t)rows * cols >= 0x80000000ull) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)(((uint64_t)count + kBlock - 1) / kBlock));
  hipLaunchKernelGGL((bilinear_kernel<T, X>), grid, dim3(kBlock), 0, st, table, (int32_t)rows, (int32_t)cols, px, py,
                     out, count);
  return hipGetLastError();
}

}  // namespace

bool linear_interp_staged(uint32_t nValues, uint32_t wordBytes) {
  return (uint64_t)nValues * wordBytes <= kInterpLdsBytes;
}

hipError_t linear_interp_f32_launch(const float* table, uint32_t nValues, float x1, float xSpacing, const float* x,
                                    float* y, uint32_t count, hipStream_t st) {
  return linear_run<float, float>(table, nValues, x1, xSpacing, x, y, count, st);
}
template <typename T>
hipError_t linear_interp_q_launch(const T* table, uint32_t nValues, const int32_t* x, T* y, uint32_t count,
                                  hipStream_t st) {
  return linear_run<T, int32_t>(table, nValues, 0.0f, 0.0f, x, y, count, st);
}
template hipError_t linear_interp_q_launch<int32_t>(const int32_t*, uint32_t, const int32_t*, int32_t*, uint32_t, hipStream_t);
template hipError_t linear_interp_q_launch<int16_t>(const int16_t*, uint32_t, const int32_t*, int16_t*, uint32_t, hipStream_t);
template hipError_t linear_interp_q_launch<int8_t>(const int8_t*, uint32_t, const int32_t*, int8_t*, uint32_t, hipStream_t);

hipError_t bilinear_interp_f32_launch(const float* table, uint32_t rows, uint32_t cols, const float* px,
                                      const float* py, float* out, uint32_t count, hipStream_t st) {
  return bilinear_run<float, float>(table, rows, cols, px, py, out, count, st);
}
template <typename T>
hipError_t bilinear_interp_q_launch(const T* table, uint32_t rows, uint32_t cols, const int32_t* px, const int32_t* py,
                                    T* out, uint32_t count, hipStream_t st) {
  return bilinear_run<T, int32_t>(table, rows, cols, px, py, out, count, st);
}
template hipError_t bilinear_interp_q_launch<int32_t>(const int32_t*, uint32_t, uint32_t, const int32_t*, const int32_t*, int32_t*, uint32_t, hipStream_t);
template hipError_t bilinear_interp_q_launch<int16_t>(const int16_t*, uint32_t, uint32_t, const int32_t*, const int32_t*, int16_t*, uint32_t, hipStream_t);
template hipError_t bilinear_interp_q_launch<int8_t>(const int8_t*, uint32_t, uint32_t, const int32_t*, const int32_t*, int8_t*, uint32_t, hipStream_t);

hipError_t spline_init_launch(int type, const float* x, size_t xStride, const float* y, uint32_t n, float* coeffs,
                              float* temp, uint32_t batch, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if (n < 2 || (type != 0 && type != 1)) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)(((uint64_t)batch + kBlock - 1) / kBlock));
  hipLaunchKernelGGL(spline_init_kernel, grid, dim3(kBlock), 0, st, type, x, xStride, y, n, coeffs, temp, batch);
  return hipGetLastError();
}

hipError_t spline_launch(const float* x, size_t xStride, const float* y, const float* coeffs, uint32_t n,
                         const float* xq, size_t xqStride, float* dst, uint32_t blockSize, uint32_t batch,
                         hipStream_t st) {
  if (batch == 0 || blockSize == 0) return hipSuccess;
  if (n < 2) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)(((uint64_t)batch + kBlock / 64 - 1) / (kBlock / 64)));
  hipLaunchKernelGGL(spline_kernel, grid, dim3(kBlock), 0, st, x, xStride, y, coeffs, n, xq, xqStride, dst, blockSize,
                     batch);
  return hipGetLastError();
}

// The drop-ins' one sample, on the host.
float linear_interp_f32_host(const float* table, uint32_t nValues, float x1, float xSpacing, float x) {
  return linear_f32(table, nValues, x1, xSpacing, x);
}
int32_t linear_interp_q31_host(const int32_t* table, uint32_t nValues, int32_t x) { return linear_q(table, nValues, x); }
int16_t linear_interp_q15_host(const int16_t* table, uint32_t nValues, int32_t x) { return linear_q(table, nValues, x); }
int8_t linear_interp_q7_host(const int8_t* table, uint32_t nValues, int32_t x) { return linear_q(table, nValues, x); }
float bilinear_interp_f32_host(const float* table, uint32_t rows, uint32_t cols, float X, float Y) {
  return bilinear_f32(table, (int32_t)rows, (int32_t)cols, X, Y);
}
int32_t bilinear_interp_q31_host(const int32_t* table, uint32_t rows, uint32_t cols, int32_t X, int32_t Y) {
  return bilinear_q(table, (int32_t)rows, (int32_t)cols, X, Y);
}
int16_t bilinear_interp_q15_host(const int16_t* table, uint32_t rows, uint32_t cols, int32_t X, int32_t Y) {
  return bilinear_q(table, (int32_t)rows, (int32_t)cols, X, Y);
}
int8_t bilinear_interp_q7_host(const int8_t* table, uint32_t rows, uint32_t cols, int32_t X, int32_t Y) {
  return bilinear_q(table, (int32_t)rows, (int32_t)cols, X, Y);
}

}  // namespace mi355x
