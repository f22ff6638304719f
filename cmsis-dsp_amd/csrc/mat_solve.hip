// arm_mat_inverse_f32, arm_mat_cholesky_f32, arm_mat_ldlt_f32 and arm_mat_solve_{lower,upper}_triangular_f32
// over a batch of contiguous row-major items, bit-exact with the reference's scalar branches
// (Source/MatrixFunctions/arm_mat_inverse_f32.c:154-294 with the row macros of matrix_utils.h:460-529,
// arm_mat_cholesky_f32.c:398-431, arm_mat_ldlt_f32.c:345-445, arm_mat_solve_lower_triangular_f32.c:288-325,
// arm_mat_solve_upper_triangular_f32.c:274-310): the same operations in the same association order, products
// rounded before they are subtracted (contraction off), plain `/` and sqrtf (correctly rounded).
//
// Mapping.  A team of L lanes (a power of two, at most the 256 of the workgroup) owns one item, and a
// workgroup holds 256 / L teams, so lanes are busy at n = 4 too.  While a workgroup's items fit the LDS
// (kMatSolveLds) they are staged there and written back once; past that one workgroup of 256 lanes works on
// one item in place in global memory, its phases separated by the same workgroup barriers.  Every loop that
// holds a barrier runs n times in every lane: an item that fails (or lies past the batch) only masks its
// team's work, so all waves of a workgroup meet the same barrier sequence.  The status is one int32 per
// item, stored by the team's lane 0.
//
//   inverse    one lane per column of [src | dst]: row swap, scaling and elimination touch a lane's own column
//              only (conflict-free in LDS), the multiplier src[r][c] is a broadcast read.  Column c itself,
//              which every lane reads, is updated after a barrier, one lane per row.  1 barrier per column.
//   cholesky   one lane per row j >= i of column i; the row stride is odd, so the lanes' row reads spread over
//              the banks.  The unscaled diagonal goes through a per-team word.  2 barriers per column.
//   ldlt       pivot scan by every lane (diagonal reads are broadcasts), row swap one lane per column, column
//              swap one lane per row, trailing update one lane per column x (reads column k, which it does
//              not write), column scaling one lane per row.  4 barriers per step.
//   solves     one lane per right-hand-side column of one item, t and a straight from global memory: the
//              columns are independent and a lane reads back only its own words, so there is no barrier at
//              all.  Up to n = 64 the lane's column of x is kept in LDS as well.
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mi355x {
namespace {

constexpr int kSingular = -5, kDecompositionFailure = -7;      // arm_status values (arm_math.h)

struct Team {
  int sub, lane;          // team within the workgroup, lane within the team
  uint32_t item0, item;   // first item of the workgroup, this team's item
  uint32_t cnt;           // items of this workgroup inside the batch
  bool valid;
};

__device__ __forceinline__ Team team_of(int L, int ipw, uint32_t batch) {
  Team t;
  t.sub = threadIdx.x / L;
  t.lane = threadIdx.x - t.sub * L;
  t.item0 = blockIdx.x * (uint32_t)ipw;
  t.item = t.item0 + t.sub;
  const uint32_t left = batch - t.item0;
  t.cnt = left < (uint32_t)ipw ? left : (uint32_t)ipw;
  t.valid = t.sub < ipw && t.item < batch;
  return t;
}

// The workgroup copies `count` contiguous words; 16-B accesses when the global side is 16-B aligned (the
// LDS side always is).
__device__ __forceinline__ void wg_load(float* lds, const float* g, uint32_t count) {
  if (((uintptr_t)g & 15) == 0) {
    const uint32_t q = count / 4;
    for (uint32_t i = threadIdx.x; i < q; i += kBlock) ((float4*)lds)[i] = ((const float4*)g)[i];
    for (uint32_t i = q * 4 + threadIdx.x; i < count; i += kBlock) lds[i] = g[i];
  } else {
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) lds[i] = g[i];
  }
}
__device__ __forceinline__ void wg_store(float* g, const float* lds, uint32_t count) {
  if (((uintptr_t)g & 15) == 0) {
    const uint32_t q = count / 4;
    for (uint32_t i = threadIdx.x; i < q; i += kBlock) ((float4*)g)[i] = ((const float4*)lds)[i];
    for (uint32_t i = q * 4 + threadIdx.x; i < count; i += kBlock) g[i] = lds[i];
  } else {
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) g[i] = lds[i];
  }
}
// ... into rows of stride ld (> n): `rows` rows of n words.
__device__ __forceinline__ void wg_load_rows(float* lds, const float* g, uint32_t rows, int n, int ld) {
  if (((uintptr_t)g & 15) == 0 && (n & 3) == 0) {
    const uint32_t q = rows * (uint32_t)n / 4, n4 = n / 4;
    for (uint32_t i = threadIdx.x; i < q; i += kBlock) {
      const float4 v = ((const float4*)g)[i];
      const uint32_t r = i / n4;
      float* p = lds + r * ld + (i - r * n4) * 4;
      p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
  } else {
    const uint32_t count = rows * (uint32_t)n;
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
      const uint32_t r = i / n;
      lds[r * ld + (i - r * n)] = g[i];
    }
  }
}

// ---- inverse ---------------------------------------------------------------------------------------
// S, D: the item's src and dst, n x n, stride n (LDS or global).  dst = I, then for every column: pivot =
// first row >= c winning fabsf(new) > fabsf(cur) (a NaN neither wins nor loses); a zero pivot ends the item
// (SINGULAR, both matrices as they stand); swap when the pivot is off the diagonal (src from column c, dst
// whole rows); the pivot row times 1.0f / pivot; every other row x = x - m * p with m = src[r][c] as it was
// before the step.  The reference's all-zero check after the loop (:283-294) cannot fire -- the scaled
// diagonal is pivot * (1 / pivot), never 0 -- and is not built.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void mat_inverse_kernel(float* src, float* dst, int n, uint32_t batch, int L,
                                                            int ipw, int32_t* status) {
  extern __shared__ __align__(16) float ms_lds[];
  using Ix = typename std::conditional<LDS, int, size_t>::type;
  const Team t = team_of(L, ipw, batch);
  const Ix N = n, nn = N * N;
  const uint32_t doff = ((uint32_t)ipw * (uint32_t)nn + 3u) & ~3u;      // LDS: dst block, 16-B aligned
  float *S, *D;
  if (LDS) {
    wg_load(ms_lds, src + (size_t)t.item0 * nn, t.cnt * (uint32_t)nn);
    S = ms_lds + t.sub * nn;
    D = ms_lds + doff + t.sub * nn;
  } else {
    S = src + (size_t)t.item * nn;
    D = dst + (size_t)t.item * nn;
  }
  bool alive = t.valid;
  int st = 0;
  if (alive)
    for (Ix i = t.lane; i < nn; i += L) D[i] = (i % (N + 1)) == 0 ? 1.0f : 0.0f;
  __syncthreads();
  for (int col = 0; col < n; ++col) {
    float piv = 0.0f, vcc = 0.0f, ip = 0.0f;
    int sel = col;
    if (alive) {
      vcc = piv = S[col * N + col];
      for (int r = col + 1; r < n; ++r) {
        const float v = S[r * N + col];
        if (fabsf(v) > fabsf(piv)) { piv = v; sel = r; }
      }
      if (piv == 0.0f) { alive = false; st = kSingular; }
    }
    // every column but `col`, which all lanes are still reading
    if (alive) {
      ip = 1.0f / piv;
      for (int c = t.lane; c < 2 * n; c += L) {
        if (c <= col) continue;                       // src is processed from column col on
        float* X = c < n ? S + c : D + (c - n);
        float p = X[sel * N];
        if (sel != col) X[sel * N] = X[col * N];
        p = p * ip;
        X[col * N] = p;
        // m: row sel now holds the old row col.  From n = 16 on four rows at a time, loads before stores: the
        // compiler cannot tell that the stores to this column leave column col alone, and would wait for each
        // one (n = 32: 30 -> 39, n = 64: 2.3 -> 3.4 M matrices/s; below 16 the plain loop is 9 % faster).
        auto mult = [&](int r) { return r == sel ? vcc : S[r * N + col]; };
        int r = 0;
        for (; n >= 16 && r + 4 <= n; r += 4) {
          const float m0 = mult(r), m1 = mult(r + 1), m2 = mult(r + 2), m3 = mult(r + 3);
          const float x0 = X[r * N], x1 = X[(r + 1) * N], x2 = X[(r + 2) * N], x3 = X[(r + 3) * N];
          X[r * N] = r == col ? x0 : x0 - m0 * p;
          X[(r + 1) * N] = r + 1 == col ? x1 : x1 - m1 * p;
          X[(r + 2) * N] = r + 2 == col ? x2 : x2 - m2 * p;
          X[(r + 3) * N] = r + 3 == col ? x3 : x3 - m3 * p;
        }
        for (; r < n; ++r)
          if (r != col) X[r * N] = X[r * N] - mult(r) * p;
      }
    }
    __syncthreads();
    // column col, one lane per row: the same operations on the words read above
    if (alive) {
      const float p = piv * ip;
      for (int r = t.lane; r < n; r += L) {
        const float old = r == col ? piv : (r == sel ? vcc : S[r * N + col]);
        S[r * N + col] = r == col ? p : old - old * p;
      }
    }
    // no barrier here: nothing reads column col again, and the next step's reads of column col + 1 and its
    // writes of the columns past that one are ordered after this step's first phase by the barrier above
  }
  if (LDS) {
    __syncthreads();
    wg_store(src + (size_t)t.item0 * nn, ms_lds, t.cnt * (uint32_t)nn);
    wg_store(dst + (size_t)t.item0 * nn, ms_lds + doff, t.cnt * (uint32_t)nn);
  }
  if (status && t.valid && t.lane == 0) status[t.item] = st;
}

// ---- Cholesky --------------------------------------------------------------------------------------
// Column i, rows j >= i: g = a[j][i], g = g - G[i][k] * G[j][k] for k ascending; G[i][i] <= 0 ends the item
// (DECOMPOSITION_FAILURE: column i stays unscaled, later columns are not written); else column i from row i
// down times 1.0f / sqrtf(G[i][i]).  The strict upper triangle of dst is never written.
// LDS: the team's matrix is both a and G (stride n | 1), extra[2 sub] the unscaled diagonal, extra[2 sub + 1]
// the number of columns to write back.  Global: a = src, G = dst (which may be the same words), stride n.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void mat_cholesky_kernel(const float* src, float* dst, int n, uint32_t batch,
                                                             int L, int ipw, int32_t* status) {
  extern __shared__ __align__(16) float ms_lds[];
  using Ix = typename std::conditional<LDS, int, size_t>::type;
  const Team t = team_of(L, ipw, batch);
  const Ix N = n, ld = LDS ? (n | 1) : n;
  const size_t nn = (size_t)n * n;
  float* extra = ms_lds + (LDS ? (size_t)ipw * n * (n | 1) : 0);
  const float* A;
  float* G;
  if (LDS) {
    wg_load_rows(ms_lds, src + t.item0 * nn, t.cnt * (uint32_t)n, n, (int)ld);
    G = ms_lds + t.sub * (N * ld);
    A = G;
  } else {
    A = src + t.item * nn;
    G = dst + t.item * nn;
  }
  bool alive = t.valid;
  int st = 0, lim = n;
  if (LDS) __syncthreads();
  for (int i = 0; i < n; ++i) {
    if (alive) {
      for (int j = i + t.lane; j < n; j += L) {
        float g = A[j * ld + i];
        for (int k = 0; k < i; ++k) g = g - G[i * ld + k] * G[j * ld + k];
        G[j * ld + i] = g;
        if (j == i) extra[2 * t.sub] = g;
      }
    }
    __syncthreads();
    if (alive) {
      const float d = extra[2 * t.sub];
      if (d <= 0.0f) {
        alive = false; st = kDecompositionFailure; lim = i + 1;
      } else {
        const float s = 1.0f / sqrtf(d);
        for (int j = i + t.lane; j < n; j += L) G[j * ld + i] = G[j * ld + i] * s;
      }
    }
    __syncthreads();
  }
  if (LDS) {
    if (t.valid && t.lane == 0) ((int*)extra)[2 * t.sub + 1] = lim;
    __syncthreads();
    // the lower triangle of the columns that were reached, flat over the workgroup's items
    const uint32_t count = t.cnt * (uint32_t)nn;
    float* out = dst + t.item0 * nn;
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
      const uint32_t row = i / n, c = i - row * n, it = row / n, r = row - it * n;
      if (c <= r && (int)c < ((const int*)extra)[2 * it + 1]) out[i] = ms_lds[row * ld + c];
    }
  }
  if (status && t.valid && t.lane == 0) status[t.item] = st;
}

// ---- LDLT ------------------------------------------------------------------------------------------
// arm_mat_ldlt_f32 as written.  Step k: pivot j = first diagonal index >= k with the strictly largest value
// above -FLT_MAX; rows then columns k and j swapped over the whole matrix; pp[k] = j; a = A[k][k], and
// fabsf(a) < 1.0e-8f stops the item (rank deficient at k); A[w][x] = A[w][x] - A[w][k] * A[x][k] / a for
// w, x > k (multiply, divide, subtract); column k below the diagonal divided by a.  Then: rank deficient ->
// columns >= k zeroed and diag = k - 1, else diag = n; the strict upper triangle zeroed; d = 0 except
// d[i][i] = A[i][i], l[i][i] = 1.0f for i < diag.  Status is always success, so there is none.
// LDS: the team's working matrix has stride n | 1.  Global: pl is the working matrix.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void mat_ldlt_kernel(const float* src, float* pl, float* pd, uint16_t* pp, int n,
                                                         uint32_t batch, int L, int ipw) {
  extern __shared__ __align__(16) float ms_lds[];
  using Ix = typename std::conditional<LDS, int, size_t>::type;
  const Team t = team_of(L, ipw, batch);
  const Ix N = n, ld = LDS ? (n | 1) : n;
  const size_t nn = (size_t)n * n;
  float* A;
  if (LDS) {
    wg_load_rows(ms_lds, src + t.item0 * nn, t.cnt * (uint32_t)n, n, (int)ld);
    A = ms_lds + t.sub * (N * ld);
  } else {
    A = pl + t.item * nn;
    if (t.valid && A != src + t.item * nn)
      for (size_t i = t.lane; i < nn; i += L) A[i] = src[t.item * nn + i];
  }
  uint16_t* P = pp + (size_t)t.item * n;
  if (t.valid)
    for (int k = t.lane; k < n; k += L) P[k] = (uint16_t)k;
  bool alive = t.valid;
  int stop = n;                           // the step at which the item stopped (n: full rank)
  __syncthreads();
  for (int k = 0; k < n; ++k) {
    int j = k;
    if (alive) {
      float m = -3.402823466e+38f;        // F32_MIN of the reference: -FLT_MAX
      for (int r = k; r < n; ++r) {
        const float v = A[r * ld + r];
        if (v > m) { m = v; j = r; }
      }
    }
    __syncthreads();                      // the row swap writes diagonal words that the scan reads
    if (alive) {
      if (j != k)
        for (int c = t.lane; c < n; c += L) {
          const float x = A[k * ld + c];
          A[k * ld + c] = A[j * ld + c];
          A[j * ld + c] = x;
        }
    }
    __syncthreads();
    if (alive && j != k)
      for (int r = t.lane; r < n; r += L) {
        const float x = A[r * ld + k];
        A[r * ld + k] = A[r * ld + j];
        A[r * ld + j] = x;
      }
    __syncthreads();
    float a = 0.0f;
    if (alive) {
      // k >= 1: ordered after the initial P[k] = k of another lane by the barriers above; k = 0 is lane 0's own
      if (t.lane == 0) P[k] = (uint16_t)j;
      a = A[k * ld + k];
      if (fabsf(a) < 1.0e-8f) { alive = false; stop = k; }
    }
    if (alive)
      for (int x = k + 1 + t.lane; x < n; x += L) {
        const float ax = A[x * ld + k];
        int w = k + 1;
        for (; w + 4 <= n; w += 4) {          // loads before stores, as in the inverse
          const float c0 = A[w * ld + k], c1 = A[(w + 1) * ld + k], c2 = A[(w + 2) * ld + k], c3 = A[(w + 3) * ld + k];
          const float y0 = A[w * ld + x], y1 = A[(w + 1) * ld + x], y2 = A[(w + 2) * ld + x], y3 = A[(w + 3) * ld + x];
          A[w * ld + x] = y0 - c0 * ax / a;
          A[(w + 1) * ld + x] = y1 - c1 * ax / a;
          A[(w + 2) * ld + x] = y2 - c2 * ax / a;
          A[(w + 3) * ld + x] = y3 - c3 * ax / a;
        }
        for (; w < n; ++w) A[w * ld + x] = A[w * ld + x] - A[w * ld + k] * ax / a;
      }
    __syncthreads();
    if (alive)
      for (int w = k + 1 + t.lane; w < n; w += L) A[w * ld + k] = A[w * ld + k] / a;
    // the next step's scan reads the diagonal only; its barrier orders these words before the row swap
  }
  __syncthreads();
  if (t.valid) {
    const int diag = stop < n ? stop - 1 : n;
    float* lo = pl + t.item * nn;
    float* dd = pd + t.item * nn;
    for (size_t i = t.lane; i < nn; i += L) {
      const int r = (int)(i / n), c = (int)(i - (size_t)r * n);
      float v = A[r * ld + c], dv = 0.0f;
      if (c > r || c >= stop) v = 0.0f;
      if (r == c && r < diag) { dv = v; v = 1.0f; }
      lo[i] = v;
      dd[i] = dv;
    }
  }
}

// ---- triangular solves -----------------------------------------------------------------------------
// One lane per (item, right-hand-side column j): tmp = a[i][j], tmp = tmp - t[i][k] * x[k][j] (k ascending
// below i for the lower solve, descending from n - 1 above i for the upper solve), x[i][j] = tmp / t[i][i].
// The reference returns SINGULAR when it reaches a zero diagonal, which is in column 0: only column 0 gets
// the rows before that one, every other word of dst is left alone.  x may be a (a[i][j] is read before
// x[i][j] is written, and a lane touches its own column only).
// XLDS (n <= kSolveLdsMaxN): the lane also keeps its column of x in LDS, word k at k * 256 + lane
// (conflict-free), and the chain reads it there, not through a global store and load of the same word.
constexpr int kSolveLdsMaxN = 64;       // 64 KiB of x per workgroup
template <bool LOWER, bool XLDS>
__global__ __launch_bounds__(kBlock) void mat_solve_tri_kernel(const float* tm, const float* a, float* x, int n,
                                                              int cols, uint64_t total, int32_t* status) {
  extern __shared__ __align__(16) float ms_lds[];
  float* xs = ms_lds + threadIdx.x;
  const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (gid >= total) return;
  const uint64_t item = gid / (uint32_t)cols;
  const int j = (int)(gid - item * (uint32_t)cols);
  const float* T = tm + item * n * n;
  const float* A = a + item * n * cols + j;
  float* X = x + item * n * cols + j;
  const size_t N = n, C = cols;
  int rows = n;                               // rows solved, in the solve's own order
  for (int q = 0; q < n; ++q) {
    const size_t i = LOWER ? q : n - 1 - q;
    if (T[i * N + i] == 0.0f) { rows = q; break; }
  }
  if (rows < n && j != 0) return;
  for (int q = 0; q < rows; ++q) {
    const size_t i = LOWER ? q : n - 1 - q;
    float tmp = A[i * C];
    if (LOWER) {
      for (size_t k = 0; k < i; ++k) tmp = tmp - T[i * N + k] * (XLDS ? xs[k * kBlock] : X[k * C]);
    } else {
      for (size_t k = N - 1; k > i; --k) tmp = tmp - T[i * N + k] * (XLDS ? xs[k * kBlock] : X[k * C]);
    }
    const float v = tmp / T[i * N + i];
    X[i * C] = v;
    if (XLDS) xs[i * kBlock] = v;
  }
  if (status && j == 0) status[item] = rows < n ? kSingular : 0;
}

// ---- launch ----------------------------------------------------------------------------------------
int pow2_at_least(int v) {
  int p = 1;
  while (p < v && p < kBlock) p <<= 1;
  return p;
}

struct Plan { int L, ipw; size_t lds; bool in_lds; };

// width: lanes an item can use; bytes(ipw): the LDS a workgroup of ipw items needs.
template <typename Bytes>
Plan plan_of(int width, Bytes bytes) {
  Plan p;
  p.L = pow2_at_least(width);
  p.ipw = kBlock / p.L;
  while (p.ipw > 1 && bytes(p.ipw) > kMatSolveLds) p.ipw >>= 1;
  p.lds = bytes(p.ipw);
  p.in_lds = p.lds <= kMatSolveLds;
  if (!p.in_lds) { p.L = kBlock; p.ipw = 1; p.lds = 16; }
  return p;
}

template <typename K>
hipError_t allow_lds(K k, size_t lds) {
  if (lds <= 65536) return hipSuccess;
  return hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

size_t inverse_bytes(int n, int ipw) { return 4 * ((((size_t)ipw * n * n + 3) & ~(size_t)3) + (size_t)ipw * n * n); }
size_t padded_bytes(int n, int ipw) { return 4 * ((size_t)ipw * n * (n | 1) + 2 * (size_t)ipw) + 16; }

}  // namespace

hipError_t mat_inverse_f32_launch(int n, float* src, float* dst, uint32_t batch, int32_t* status, hipStream_t st) {
  if (n <= 0 || batch == 0) return hipSuccess;
  const Plan p = plan_of(2 * n, [n](int ipw) { return inverse_bytes(n, ipw); });
  auto k = p.in_lds ? mat_inverse_kernel<true> : mat_inverse_kernel<false>;
  const hipError_t e = allow_lds(k, p.lds);
  if (e != hipSuccess) return e;
  const uint32_t grid = (batch + p.ipw - 1) / p.ipw;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), p.lds, st, src, dst, n, batch, p.L, p.ipw, status);
  return hipGetLastError();
}

hipError_t mat_cholesky_f32_launch(int n, const float* src, float* dst, uint32_t batch, int32_t* status,
                                   hipStream_t st) {
  if (n <= 0 || batch == 0) return hipSuccess;
  const Plan p = plan_of(n, [n](int ipw) { return padded_bytes(n, ipw); });
  auto k = p.in_lds ? mat_cholesky_kernel<true> : mat_cholesky_kernel<false>;
  const hipError_t e = allow_lds(k, p.lds);
  if (e != hipSuccess) return e;
  const uint32_t grid = (batch + p.ipw - 1) / p.ipw;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), p.lds, st, src, dst, n, batch, p.L, p.ipw, status);
  return hipGetLastError();
}

hipError_t mat_ldlt_f32_launch(int n, const float* src, float* pl, float* pd, uint16_t* pp, uint32_t batch,
                               hipStream_t st) {
  if (n <= 0 || batch == 0) return hipSuccess;
  const Plan p = plan_of(n, [n](int ipw) { return padded_bytes(n, ipw); });
  auto k = p.in_lds ? mat_ldlt_kernel<true> : mat_ldlt_kernel<false>;
  const hipError_t e = allow_lds(k, p.lds);
  if (e != hipSuccess) return e;
  const uint32_t grid = (batch + p.ipw - 1) / p.ipw;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), p.lds, st, src, pl, pd, pp, n, batch, p.L, p.ipw);
  return hipGetLastError();
}

hipError_t mat_solve_tri_f32_launch(bool lower, int n, int cols, const float* t, const float* a, float* x,
                                    uint32_t batch, int32_t* status, hipStream_t st) {
  if (n <= 0 || cols <= 0 || batch == 0) return hipSuccess;
  const uint64_t total = (uint64_t)batch * (uint32_t)cols, grid = (total + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  const bool xlds = n <= kSolveLdsMaxN;
  auto k = lower ? (xlds ? mat_solve_tri_kernel<true, true> : mat_solve_tri_kernel<true, false>)
                 : (xlds ? mat_solve_tri_kernel<false, true> : mat_solve_tri_kernel<false, false>);
  const size_t lds = xlds ? sizeof(float) * kBlock * (size_t)n : 0;
  hipLaunchKernelGGL(k, dim3((uint32_t)grid), dim3(kBlock), lds, st, t, a, x, n, cols, total, status);
  return hipGetLastError();
}

}  // namespace mi355x
