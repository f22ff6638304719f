// Batched q15 / q31 matrix multiply on the i8 matrix cores — MI355X, bit-exact.
//
// Replaces the host scalar paths of Source/MatrixFunctions/arm_mat_mult_q15.c (:741-912,
// !ARM_MATH_DSP branch: q63 sum of exact q15 products, __SSAT((sum >> 15), 16)) and
// arm_mat_mult_q31.c (:53-163: q63 sum of exact q31 products, wrapping as gcc's adds do,
// (q31)(sum >> 31)).  Both are plain integer sums, so any evaluation order gives the
// reference's bits.
//
// Byte slicing: a value v of P bytes is v = sum_p 256^p t_p + c0 with every t_p a SIGNED
// byte (the top byte as is, lower bytes offset by -128) and c0 = 128 * sum_{p<P-1} 256^p.
// Then, for C = A*B over K terms,
//   C_ij = sum_{p,q} 256^(p+q) (T^A_p T^B_q)_ij + c0 (rowsum(A)_i + colsum(B)_j) - K c0^2,
// where the P^2 plane products run on v_mfma_i32_32x32x32_i8 (exact int32 accumulation)
// into 2P-1 accumulators by weight class p+q, and the row / column sums are exact integer
// sums gathered while staging.  The result is formed in int64 (mod 2^64, as the reference
// wraps).  Accumulator bound: a class holds at most P pairs of |t t'| <= 2^14 per k, so
// K <= kMatI8MaxK keeps every int32 accumulator exact; longer K uses the VALU kernel.
// Operand maps (verified with exact data, tools/probes/mfma_i8_layout.hip): lane l holds
// A[row l&31][k = 16(l>>5) + j] and B[k = 16(l>>5) + j][col l&31] in byte j.
#include "common.hpp"
#include "kernels.hpp"

namespace mi355x {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef short s2x __attribute__((ext_vector_type(2)));

constexpr int kMatI8MaxK = 32704;

// Plane p of four values given as the low bytes p of four dwords: signed bytes, the lower
// planes offset by -128 (x - 128 = x ^ 0x80 on a byte).
template <int P>
__device__ __forceinline__ uint32_t plane4(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int p) {
  const uint32_t sel = 0x0c0c0400u + 0x0101u * (uint32_t)p;     // [v_lo.byte p, v_hi.byte p, 0, 0]
  const uint32_t lo = __builtin_amdgcn_perm(v1, v0, sel), hi = __builtin_amdgcn_perm(v3, v2, sel);
  const uint32_t w = lo | (hi << 16);
  return p == P - 1 ? w : w ^ 0x80808080u;
}

// ---- both kernels (v2: q15, v3: q31): 128 x 128 (q15) / 128 x 64 (q31) workgroup tiles of 8
// waves (4 x 2), wave tiles 32 x 64 / 32 x 32 (accumulators fit two waves per SIMD, so one wave's
// MFMAs overlap the other's staging), double-buffered LDS planes (one barrier per K step), step
// kt+2's global loads in flight under step kt's MFMAs.  B arrives row-major [k][n]; the MFMA
// wants 16 k-consecutive bytes per column: v2's staging transposes 8 k-rows x 2 columns per
// thread into k-contiguous dwords (v_perm) before the LDS write, v3 stages B as it is and reads
// it transposed.
template <typename T> struct I8Cfg;
template <> struct I8Cfg<int16_t> { static constexpr int BM = 128, BN = 128, WBM = 1, WBN = 2, KT = 64; };
template <> struct I8Cfg<int32_t> { static constexpr int BM = 128, BN = 64, WBM = 1, WBN = 1, KT = 64; };
constexpr int kNT2 = 512, kWavesM = 4, kWavesN = 2;

// LDS plane layout (A in both kernels, B in v2): rows of 64 k-bytes (4 chunks of 16 B) with no
// padding; chunk c of row `row` sits at chunk c ^ ((row >> 2) & 3), and B's column `col` at row
// i8_brow8(col).  Conflict free for the reads and A's writes (MI355X_MICROARCH.md §LDS):
//  * fragment reads (ds_read_b128, 16-lane groups {0-3,12-15,20-27}, ..., banks mod 64): the 16
//    rows of a group hold (row mod 4, swizzled chunk) pairs that are all distinct, i.e. 16
//    distinct 4-bank sets (B's row permutation only swaps rows within such groups);
//  * A staging (ds_write_b128, 8 contiguous lanes, banks mod 32): two consecutive rows x 4
//    chunks -- the rows' parities differ, so the 16-dword halves do.
// (Round 2's 80-byte pitch left both staging writes two-way conflicted: 12.5 M / 54.8 M conflict
// cycles per launch for q15 / q31, profiles/r02/mat_mult_q15|q31/pmc.json.)
__device__ __forceinline__ int i8_chunk(int row, int c) { return (c ^ (row >> 2)) & 3; }
// B staging in v2 (ds_write_b64 of 8 k-bytes, 16-lane groups on consecutive column pairs, banks mod 32):
// flipping the row parity on bit 1 of the column spreads a group over both row parities, the
// most any 16 writes of 8 bytes into 64-byte rows can use (2-way); fragment reads keep each
// aligned row quad, so they stay conflict free.
__device__ __forceinline__ int i8_brow8(int col) { return col ^ ((col >> 1) & 1); }

// plane p of the two q15 values in each of d0, d1: [d0.lo, d0.hi, d1.lo, d1.hi] byte p
template <int P>
__device__ __forceinline__ uint32_t plane_q15(uint32_t d0, uint32_t d1, int p) {
  const uint32_t sel = (uint32_t)p | (uint32_t)(2 + p) << 8 | (uint32_t)(4 + p) << 16 | (uint32_t)(6 + p) << 24;
  const uint32_t w = __builtin_amdgcn_perm(d1, d0, sel);
  return p == P - 1 ? w : w ^ 0x80808080u;
}
// byte o of r0, r1, r2, r3 -> one dword (k-consecutive bytes of one column)
__device__ __forceinline__ uint32_t gather4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, int o) {
  const uint32_t sel = (uint32_t)o | (uint32_t)(4 + o) << 8 | 0x0c0c0000u;
  return __builtin_amdgcn_perm(r1, r0, sel) | (__builtin_amdgcn_perm(r3, r2, sel) << 16);
}

// ---- complex product (CX; arm_mat_cmplx_mult_q15.c:433-582, arm_mat_cmplx_mult_q31.c:836-1057).
// A (M x K/2 complex) is the M x K real matrix it already is in memory; B (K/2 x N/2 complex, i.e.
// K/2 rows of N words (c, d)) is embedded while staging: B' row 2k is the row as loaded, row 2k + 1
// its pair-swapped words (~d, c).  ~d = -d - 1 always fits the type where -d does not (d the
// minimum), and since -b d = b (~d) + b the real outputs (even columns) get the row's sum of A's
// imaginary words added in the int64 epilogue; that sum is gathered while staging A.  Zero-filled
// words outside B become (-1, 0) in the odd rows: they are staged and column-summed as such, so
// the slicing identity still gives sum_k A_ik B'staged_kj, in which A's zero fill removes them;
// columns outside the matrix are never stored.
// clip_q63_to_q31 (none.h:136-141)
__device__ __forceinline__ int32_t clip_q63_q31(int64_t v) {
  return v > 0x7fffffffLL ? 0x7fffffff : (v < -0x80000000LL ? (int32_t)0x80000000 : (int32_t)v);
}

// FULL: M % BM == 0, N % BN == 0, K % 64 == 0 and 16-B aligned rows -- no bounds checks, so the
// K loop is one basic block the scheduler can interleave (loads, staging, MFMAs); otherwise
// every load is guarded and zero-filled.
template <bool FULL, bool CX = false>
__global__ __launch_bounds__(kNT2) void mat_mult_i8v2_kernel(const int16_t* __restrict__ A, const int16_t* __restrict__ B,
                                                             int16_t* __restrict__ C, int M, int K, int N, int fast) {
  using G = I8Cfg<int16_t>;
  constexpr int P = 2, S = 2 * P - 1;            // byte planes, weight classes p + q
  constexpr int64_t C0 = 128;
  constexpr int BM = G::BM, BN = G::BN, WBM = G::WBM, WBN = G::WBN, kKT2 = G::KT, kPitch2 = kKT2;
  static_assert(kKT2 == 64, "the LDS swizzle assumes 4 chunks of 16 k-bytes per row");
  static_assert(BM == kWavesM * 32 * WBM && BN == kWavesN * 32 * WBN, "wave grid covers the tile");
  constexpr int AK = BM * kKT2 / kNT2;           // A elements per staging thread (16)
  constexpr int AKD = AK / 2;                    // ... as dwords
  constexpr int AQ = kKT2 / AK;                  // threads per A row (4)
  constexpr int NQ = kKT2 / 4;                   // rows of the epilogue's column-partial array
  constexpr int BUF = P * (BM + BN) * kPitch2;   // one K step's planes; two buffers
  __shared__ __attribute__((aligned(16))) int8_t lds[2 * BUF];

  // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs, so the linear id is
  // permuted to give each XCD a contiguous run of (matrix, tile) pairs -- the tiles of one
  // matrix then share their A row bands / B column bands in that XCD's L2.
  const int tilesN = (N + BN - 1) / BN, tiles = tilesN * ((M + BM - 1) / BM);
  const uint32_t total = gridDim.x;
  uint32_t lin = blockIdx.x;
  if (total % 8 == 0) lin = (lin % 8) * (total / 8) + lin / 8;
  const int t = (int)(lin % (uint32_t)tiles);
  const int tm = t / tilesN, tn = t % tilesN;
  const size_t bz = lin / (uint32_t)tiles;
  A += bz * (size_t)M * K;
  B += bz * (size_t)(CX ? K / 2 : K) * N;
  C += bz * (size_t)M * N;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int row0 = tm * BM, col0 = tn * BN;

  // staging roles: A row ar, AK k from ak0; B: thread (cp, kb8) stages columns 2cp, 2cp + 1 over
  // k-rows 8 kb8 .. 8 kb8 + 7 (eight coalesced dword loads), i.e. 8 k-bytes per column and plane:
  // one ds_write_b64 each
  const int ar = tid / AQ, ak0 = AK * (tid % AQ);
  const int gr = row0 + ar;
  constexpr int NQB = 8;                         // column-sum partials per column (one per kb8)
  const int cp = tid % 64, kb8 = tid / 64;
  const int gcp = col0 + 2 * cp;
  const bool vecA = FULL || (((K * 2) % 16) == 0 && (((uintptr_t)A) & 15) == 0);
  const bool vecB = FULL || ((N % 2) == 0 && (((uintptr_t)B) & 3) == 0);

  uint32_t ad[AKD], b8[8];
  auto load = [&](int k0) {
    const int ka = k0 + ak0;
    if (FULL || (vecA && gr < M && ka + AK <= K)) {
      const uint4* p = reinterpret_cast<const uint4*>(A + (size_t)gr * K + ka);
#pragma unroll
      for (int i = 0; i < AKD / 4; ++i) {
        const uint4 v = p[i];
        ad[4 * i] = v.x; ad[4 * i + 1] = v.y; ad[4 * i + 2] = v.z; ad[4 * i + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int d = 0; d < AKD; ++d) {
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int k = ka + d * 2 + e;
          const uint32_t v = (gr < M && k < K) ? (uint32_t)A[(size_t)gr * K + k] : 0u;
          w |= (v & 0xffffu) << (16 * e);
        }
        ad[d] = w;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kb = k0 + 8 * kb8 + i;
      if constexpr (CX) {
        if (i & 1) continue;                     // row 2k + 1: formed from row 2k's words in stage()
      }
      if (FULL || (vecB && kb < K && gcp + 2 <= N)) {
        b8[i] = *reinterpret_cast<const uint32_t*>(B + (size_t)(CX ? kb >> 1 : kb) * N + gcp);
      } else {
        const uint32_t lo = (kb < K && gcp < N) ? (uint32_t)(uint16_t)B[(size_t)(CX ? kb >> 1 : kb) * N + gcp] : 0u;
        const uint32_t hi = (kb < K && gcp + 1 < N) ? (uint32_t)(uint16_t)B[(size_t)(CX ? kb >> 1 : kb) * N + gcp + 1] : 0u;
        b8[i] = lo | (hi << 16);
      }
    }
  };

  // this thread's partial row / column sums over the K steps: int32 is exact (at most 16 x 511
  // values of |v| <= 2^15 per partial)
  int32_t my_rsum = 0;
  [[maybe_unused]] int32_t my_isum = 0;          // CX: the sum of this thread's imaginary (odd) words of A
  int32_t bcs[2] = {0, 0};                       // columns 2cp, 2cp + 1 (exact: <= 8 x 511 x 2^15)
  i32x16 acc[S][WBM][WBN];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int i = 0; i < WBM; ++i)
#pragma unroll
      for (int j = 0; j < WBN; ++j) acc[s][i][j] = i32x16{};
  const int wm = wid / kWavesN, wn = wid % kWavesN;
  const int r = lane & 31, h = lane >> 5;

  auto stage = [&](int buf) {
    auto As = reinterpret_cast<int8_t (*)[BM][kPitch2]>(lds + buf * BUF);
    auto Bs = reinterpret_cast<int8_t (*)[BN][kPitch2]>(lds + buf * BUF + P * BM * kPitch2);
    // exact row / column sums of the original values.  CX: b8[0], b8[2], b8[4], b8[6] hold the four
    // complex rows; the odd rows of B' exist only as the byte selectors and complement masks of the
    // plane gather below
    int32_t ra = 0;
#pragma unroll
    for (int d = 0; d < AKD; ++d) ra = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2x, ad[d]), s2x{1, 1}, ra, false);
    my_rsum += ra;
    if constexpr (CX) {
      int32_t ia = 0;
#pragma unroll
      for (int d = 0; d < AKD; ++d) ia = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2x, ad[d]), s2x{0, 1}, ia, false);
      my_isum += ia;
#pragma unroll
      for (int i = 0; i < 8; i += 2) {           // rows (c, d) and (~d, c): c - d - 1 and d + c per complex row
        bcs[0] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2x, b8[i]), s2x{1, -1}, bcs[0], false);
        bcs[1] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2x, b8[i]), s2x{1, 1}, bcs[1], false);
      }
      bcs[0] -= 4;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        bcs[0] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2x, b8[i]), s2x{1, 0}, bcs[0], false);
        bcs[1] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2x, b8[i]), s2x{0, 1}, bcs[1], false);
      }
    }
    // byte planes -> LDS
#pragma unroll
    for (int p = 0; p < P; ++p) {
      uint32_t w[AK / 4];
#pragma unroll
      for (int q = 0; q < AK / 4; ++q) w[q] = plane_q15<P>(ad[2 * q], ad[2 * q + 1], p);
#pragma unroll
      for (int q = 0; q < AK / 16; ++q)
        *reinterpret_cast<uint4*>(&As[p][ar][16 * i8_chunk(ar, ak0 / 16 + q)]) =
            make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int o = 2 * c + p;                // byte of column 2cp + c, plane p, in a dword
        uint32_t g0, g1;
        if constexpr (CX) {
          // k rows (2k, 2k + 1, 2k + 2, 2k + 3) from complex rows (k, k + 1): the odd rows take the pair's
          // other word (byte o ^ 2), complemented in column 0 (~d)
          const uint32_t sel = (uint32_t)o | (uint32_t)(o ^ 2) << 8 | (uint32_t)(4 + o) << 16 | (uint32_t)(4 + (o ^ 2)) << 24;
          const uint32_t xm = (p != P - 1 ? 0x80808080u : 0u) ^ (c == 0 ? 0xff00ff00u : 0u);
          g0 = __builtin_amdgcn_perm(b8[2], b8[0], sel) ^ xm;
          g1 = __builtin_amdgcn_perm(b8[6], b8[4], sel) ^ xm;
        } else {
          g0 = gather4(b8[0], b8[1], b8[2], b8[3], o), g1 = gather4(b8[4], b8[5], b8[6], b8[7], o);
          if (p != P - 1) { g0 ^= 0x80808080u; g1 ^= 0x80808080u; }
        }
        const int row = i8_brow8(2 * cp + c);
        *reinterpret_cast<uint2*>(&Bs[p][row][16 * i8_chunk(row, kb8 >> 1) + 8 * (kb8 & 1)]) = make_uint2(g0, g1);
      }
    }
  };
  // The second MFMA k-step (kk = 1) of K step kt runs at the head of step kt + 1, from registers,
  // while that step's first fragment reads are in flight (the barrier only orders the LDS;
  // register fragments may cross it)
  static_assert(kKT2 / 32 == 2, "two MFMA k-steps per K step");
  i32x4 ga[P][WBM], gb[P][WBN], ha[P][WBM], hb[P][WBN];   // kk = 0 / kk = 1 fragments
  auto frags_kk = [&](int buf, int kk, i32x4 (&FA)[P][WBM], i32x4 (&FB)[P][WBN]) {
    auto As = reinterpret_cast<const int8_t (*)[BM][kPitch2]>(lds + buf * BUF);
    auto Bs = reinterpret_cast<const int8_t (*)[BN][kPitch2]>(lds + buf * BUF + P * BM * kPitch2);
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int i = 0; i < WBM; ++i) {
        const int row = wm * 32 * WBM + i * 32 + r;
        FA[p][i] = *reinterpret_cast<const i32x4*>(&As[p][row][16 * i8_chunk(row, 2 * kk + h)]);
      }
#pragma unroll
      for (int j = 0; j < WBN; ++j) {
        const int row = i8_brow8(wn * 32 * WBN + j * 32 + r);
        FB[p][j] = *reinterpret_cast<const i32x4*>(&Bs[p][row][16 * i8_chunk(row, 2 * kk + h)]);
      }
    }
  };
  auto mma_kk = [&](const i32x4 (&FA)[P][WBM], const i32x4 (&FB)[P][WBN]) {
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < P; ++q)
#pragma unroll
        for (int i = 0; i < WBM; ++i)
#pragma unroll
          for (int j = 0; j < WBN; ++j)
            acc[p + q][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(FA[p][i], FB[q][j], acc[p + q][i][j], 0, 0, 0);
  };

  // Double-buffered K loop: step kt's fragments are read from buffer kt&1 first, then step
  // kt+1's planes are staged into the other buffer and step kt+2's global loads issued, and
  // the MFMAs (register-only) can interleave with that staging work; one barrier per step.
  const int nk = (K + kKT2 - 1) / kKT2;
  load(0);
  stage(0);
  if (nk > 1) load(kKT2);
  __syncthreads();
  frags_kk(0, 0, ga, gb);                      // step 0: nothing outstanding yet
  frags_kk(0, 1, ha, hb);
  if (nk > 1) stage(1);
  if (nk > 2) load(2 * kKT2);
  mma_kk(ga, gb);
  __syncthreads();
  int kt = 1;
  for (; kt + 2 < nk; ++kt) {                  // steady state: one basic block when FULL
    const int cur = kt & 1;
    frags_kk(cur, 0, ga, gb);
    mma_kk(ha, hb);                            // step kt - 1, kk = 1
    frags_kk(cur, 1, ha, hb);
    stage(cur ^ 1);
    load((kt + 2) * kKT2);
    mma_kk(ga, gb);
#pragma unroll
    for (int i = 0; i < 2 * P * P * WBM * WBN; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // one MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 10, 0);   // then up to 10 VALU (DESIGN §4 has the sweep)
    }
    __syncthreads();
  }
  for (; kt < nk; ++kt) {
    const int cur = kt & 1;
    frags_kk(cur, 0, ga, gb);
    mma_kk(ha, hb);
    frags_kk(cur, 1, ha, hb);
    if (kt + 1 < nk) stage(cur ^ 1);
    mma_kk(ga, gb);
    __syncthreads();
  }
  mma_kk(ha, hb);                              // the last step's kk = 1

  // ---- epilogue: exact sums through LDS (reusing the plane buffers), int64 combine.  The
  // partial row / column sums are reduced once (one thread per row, one per column), then every
  // output reads its two final sums; whole tiles are staged in LDS and leave as 16-B stores,
  // 16 threads per 256-B row (the per-element stores issued one 2-byte store per output, 32 lanes
  // covering 64 B).
  int64_t* rs = reinterpret_cast<int64_t*>(lds);            // [AQ][BM] partials
  int64_t* cs = rs + AQ * BM;                               // [NQ][BN], the first NQB rows in use
  int64_t* rfin = cs + NQ * BN;                             // [BM] final row sums
  int64_t* cfin = rfin + BM;                                // [BN] final column sums
  int16_t* ct = reinterpret_cast<int16_t*>(cfin + BN);      // [BM][BN] output tile (FULL)
  int64_t* is = reinterpret_cast<int64_t*>(ct + BM * BN);   // CX: [AQ][BM] partial imaginary sums
  int64_t* ifin = is + AQ * BM;                             // CX: [BM] final ones
  static_assert((AQ * BM + NQ * BN + BM + BN + (CX ? AQ * BM + BM : 0)) * 8 + BM * BN * 2 <= 2 * BUF,
                "epilogue fits the planes");
  rs[(tid % AQ) * BM + ar] = (int64_t)my_rsum;
  if constexpr (CX) is[(tid % AQ) * BM + ar] = (int64_t)my_isum;
  cs[kb8 * BN + 2 * cp] = (int64_t)bcs[0];
  cs[kb8 * BN + 2 * cp + 1] = (int64_t)bcs[1];
  __syncthreads();
  for (int i = tid; i < BM + BN; i += kNT2) {
    int64_t sum = 0;
    if (i < BM) {
#pragma unroll
      for (int q = 0; q < AQ; ++q) sum += rs[q * BM + i];
      rfin[i] = sum;
      if constexpr (CX) {
        int64_t isum = 0;
#pragma unroll
        for (int q = 0; q < AQ; ++q) isum += is[q * BM + i];
        ifin[i] = isum;
      }
    } else {
#pragma unroll
      for (int q = 0; q < NQB; ++q) sum += cs[q * BN + (i - BM)];
      cfin[i - BM] = sum;
    }
  }
  __syncthreads();
  const int64_t kpad = (int64_t)nk * kKT2;   // padded k terms are zeros: the identity holds over kpad
#pragma unroll
  for (int j = 0; j < WBN; ++j) {
    const int cc = wn * 32 * WBN + j * 32 + r;
    const int64_t csum = cfin[cc];
    const int gcol = col0 + cc;
#pragma unroll
    for (int i = 0; i < WBM; ++i) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int rr = wm * 32 * WBM + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const int grow = row0 + rr;
        uint64_t v = (uint64_t)(C0 * (rfin[rr] + csum)) - (uint64_t)kpad * (uint64_t)(C0 * C0);
#pragma unroll
        for (int s = 0; s < S; ++s) v += (uint64_t)(int64_t)acc[s][i][j][reg] << (8 * s);
        if constexpr (CX) {
          if (!(cc & 1)) v += (uint64_t)ifin[rr];             // real outputs: b (~d) + b = -b d
        }
        const int64_t sum = (int64_t)v;
        // fast q15 (arm_mat_mult_fast_q15.c:356-401 host branch): q31_t modular sum, (q15)(sum >> 15)
        const int16_t o = fast ? (int16_t)((int32_t)(uint32_t)v >> 15) : (int16_t)ssat16((int32_t)(sum >> 15));
        if constexpr (FULL) ct[rr * BN + cc] = o;
        else if (grow < M && gcol < N) C[(size_t)grow * N + gcol] = o;
      }
    }
  }
  if constexpr (FULL) {
    __syncthreads();
    constexpr int VPR = BN * 2 / 16;                         // 16-B words per tile row
    static_assert(VPR * 16 == BN * 2, "whole 16-B words per row");
#pragma unroll
    for (int w = tid; w < BM * VPR; w += kNT2) {
      const int rr = w / VPR, cw = w % VPR;
      *reinterpret_cast<uint4*>(C + (size_t)(row0 + rr) * N + col0 + cw * 8) =
          *reinterpret_cast<const uint4*>(ct + rr * BN + cw * 8);
    }
  }
}

// ---- v3 kernel (q31; round 4): the v2 tiling with B staged ROW-major.  B's
// planes are stored as [k][n] byte rows (the global layout) and the MFMA's k-contiguous
// operand is read with ds_read_b64_tr_b8 (gfx950's 8-bit transposed LDS read: per 16-lane group
// an 8-row x 16-column byte block, lane i receiving column i, row q in byte q;
// tools/probes/tr_b8.hip), so the v_perm transpose of v2's staging disappears: a thread stages
// one k-row segment of B (32 bytes) with two 16-B loads and splits it into planes with one
// v_perm per 4 values.  Column sums accumulate per thread over the k-rows it stages (its
// columns are fixed for the whole K loop).
typedef int v2i32_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2i32_t tr_b8(const int8_t* p) {   // p: a generic pointer into LDS
  return __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i32_t*)p);
}

template <bool FULL, bool CX = false>
__global__ __launch_bounds__(kNT2) void mat_mult_i8v3_kernel(const int32_t* __restrict__ A, const int32_t* __restrict__ B,
                                                             int32_t* __restrict__ C, int M, int K, int N, int fast) {
  using G = I8Cfg<int32_t>;
  constexpr int P = 4, S = 2 * P - 1;            // byte planes, weight classes p + q
  constexpr int64_t C0 = 128LL * (1 + 256 + 65536);
  constexpr int BM = G::BM, BN = G::BN, WBM = G::WBM, WBN = G::WBN, kKT2 = G::KT, kPitch2 = kKT2;
  constexpr int EPD = 1;                         // elements per dword (the guarded loads share v2's loop nest)
  constexpr int AK = BM * kKT2 / kNT2, AKD = AK, AQ = kKT2 / AK;   // A elements per staging thread (16), threads per row
  constexpr int EB = kKT2 * BN / kNT2, EBD = EB, TPR = BN / EB;    // B elements per staging thread (8), threads per k-row
  // bytes per B plane row: a multiple of 32 that is an odd multiple of 8 dwords mod 64, so the
  // 8 rows x 8 dwords a 32-lane group of ds_read_b64_tr_b8 touches cover the 64 banks once
  // (BN + 16 measured 8x the v2 conflicts)
  constexpr int BP = 96;
  constexpr int ABUF = P * BM * kPitch2, BBUF = P * kKT2 * BP;
  constexpr int BUF = ABUF + BBUF;
  // the epilogue reuses the plane buffers: partial sums (one column partial per staged k-row),
  // final sums and the output tile
  constexpr int EPI = (AQ * BM + kKT2 * BN + BM + BN + (CX ? AQ * BM + BM : 0)) * 8 + BM * BN * 4;
  __shared__ __attribute__((aligned(16))) int8_t lds[2 * BUF > EPI ? 2 * BUF : EPI];

  const int tilesN = (N + BN - 1) / BN, tiles = tilesN * ((M + BM - 1) / BM);
  const uint32_t total = gridDim.x;
  uint32_t lin = blockIdx.x;
  if (total % 8 == 0) lin = (lin % 8) * (total / 8) + lin / 8;
  const int t = (int)(lin % (uint32_t)tiles);
  const int tm = t / tilesN, tn = t % tilesN;
  const size_t bz = lin / (uint32_t)tiles;
  A += bz * (size_t)M * K;
  B += bz * (size_t)(CX ? K / 2 : K) * N;
  C += bz * (size_t)M * N;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int row0 = tm * BM, col0 = tn * BN;

  // staging roles: A row ar, AK k from ak0 (as v2); B k-row bk, columns bc .. bc + EB - 1
  const int ar = tid / AQ, ak0 = AK * (tid % AQ);
  const int bk = tid / TPR, bc = EB * (tid % TPR);
  const int gr = row0 + ar, gc = col0 + bc;
  const bool vecA = FULL || (((K * 4) % 16) == 0 && (((uintptr_t)A) & 15) == 0);
  const bool vecB = FULL || (((N * 4) % 16) == 0 && (((uintptr_t)B) & 15) == 0);

  uint32_t ad[AKD], bd[EBD];
  auto load = [&](int k0) {
    const int ka = k0 + ak0;
    if (FULL || (vecA && gr < M && ka + AK <= K)) {
      const uint4* p = reinterpret_cast<const uint4*>(A + (size_t)gr * K + ka);
#pragma unroll
      for (int i = 0; i < AKD / 4; ++i) {
        const uint4 v = p[i];
        ad[4 * i] = v.x; ad[4 * i + 1] = v.y; ad[4 * i + 2] = v.z; ad[4 * i + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int d = 0; d < AKD; ++d) {
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < EPD; ++e) {
          const int k = ka + d * EPD + e;
          const uint32_t v = (gr < M && k < K) ? (uint32_t)A[(size_t)gr * K + k] : 0u;
          w |= v << (16 * e);
        }
        ad[d] = w;
      }
    }
    const int kb = k0 + bk;
    if (FULL || (vecB && kb < K && gc + EB <= N)) {
      const uint4* p = reinterpret_cast<const uint4*>(B + (size_t)(CX ? kb >> 1 : kb) * N + gc);
#pragma unroll
      for (int i = 0; i < EBD / 4; ++i) {
        const uint4 v = p[i];
        bd[4 * i] = v.x; bd[4 * i + 1] = v.y; bd[4 * i + 2] = v.z; bd[4 * i + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int d = 0; d < EBD; ++d) {
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < EPD; ++e) {
          const int c = gc + d * EPD + e;
          const uint32_t v = (kb < K && c < N) ? (uint32_t)B[(size_t)(CX ? kb >> 1 : kb) * N + c] : 0u;
          w |= v << (16 * e);
        }
        bd[d] = w;
      }
    }
  };

  int64_t my_rsum = 0;                           // CX: the even (real) words only, the odd ones in my_isum
  [[maybe_unused]] int64_t my_isum = 0;          // CX: the sum of this thread's imaginary (odd) words of A
  // CX: this thread's plane row bk is row 2k (the words as loaded) or row 2k + 1 ((~d, c) per pair) for the
  // whole K loop.  An odd row is never formed in registers: its planes come from the loaded words with the
  // pair-swapping byte selector and the complement mask below, and its column sums from the loaded words'
  // sums at the end (sum of ~d = -(sum of d) - the number of staged rows, zero fill included)
  [[maybe_unused]] const bool odd = CX && (bk & 1);
  // column sums of the k-rows this thread stages (at most K / 64 <= 511 of them)
  int64_t my_csum[EB];
#pragma unroll
  for (int c = 0; c < EB; ++c) my_csum[c] = 0;
  i32x16 acc[S][WBM][WBN];
#pragma unroll
  for (int s2 = 0; s2 < S; ++s2)
#pragma unroll
    for (int i = 0; i < WBM; ++i)
#pragma unroll
      for (int j = 0; j < WBN; ++j) acc[s2][i][j] = i32x16{};
  const int wm = wid / kWavesN, wn = wid % kWavesN;
  const int r = lane & 31, h = lane >> 5;

  auto stage = [&](int buf) {
    auto As = reinterpret_cast<int8_t (*)[BM][kPitch2]>(lds + buf * BUF);
    int8_t* Bs = lds + buf * BUF + ABUF;           // [P][kKT2][BP]
#pragma unroll
    for (int d = 0; d < AKD; ++d) {
      if constexpr (CX) {
        if (d & 1) my_isum += (int32_t)ad[d];
        else my_rsum += (int32_t)ad[d];
      } else {
        my_rsum += (int32_t)ad[d];
      }
    }
#pragma unroll
    for (int d = 0; d < EBD; ++d) my_csum[d] += (int32_t)bd[d];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      uint32_t w[AK / 4];
#pragma unroll
      for (int q = 0; q < AK / 4; ++q) w[q] = plane4<P>(ad[4 * q], ad[4 * q + 1], ad[4 * q + 2], ad[4 * q + 3], p);
#pragma unroll
      for (int q = 0; q < AK / 16; ++q)
        *reinterpret_cast<uint4*>(&As[p][ar][16 * i8_chunk(ar, ak0 / 16 + q)]) =
            make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
      // B: plane p of this thread's EB values, EB contiguous bytes of plane row bk
      uint32_t wb[EB / 4];
      if constexpr (CX) {
        // byte p of the four values of a dword group, the pairs swapped in an odd row; there the first
        // byte of each pair (~d) is complemented on top of the lower planes' -128
        const uint32_t up = (uint32_t)p;
        const uint32_t se = 0x0c0c0400u + 0x0101u * up, so = 0x0c0c0004u + 0x0101u * up;
        const uint32_t sel = odd ? so : se;
        const uint32_t xm = (p != P - 1 ? 0x80808080u : 0u) ^ (odd ? 0x00ff00ffu : 0u);
#pragma unroll
        for (int q = 0; q < EB / 4; ++q)
          wb[q] = (__builtin_amdgcn_perm(bd[4 * q + 1], bd[4 * q], sel) |
                   (__builtin_amdgcn_perm(bd[4 * q + 3], bd[4 * q + 2], sel) << 16)) ^ xm;
      } else {
#pragma unroll
        for (int q = 0; q < EB / 4; ++q) wb[q] = plane4<P>(bd[4 * q], bd[4 * q + 1], bd[4 * q + 2], bd[4 * q + 3], p);
      }
      int8_t* dstb = Bs + (size_t)p * kKT2 * BP + bk * BP + bc;
      static_assert(EB == 8, "one ds_write_b64 per plane");
      *reinterpret_cast<uint2*>(dstb) = make_uint2(wb[0], wb[1]);
    }
  };
  constexpr int KS = kKT2 / 32;
  i32x4 fa[KS][P][WBM], fb[KS][P][WBN];
  // B fragment of column block j, k-step kk: lane l of 16-lane group g = l >> 4 supplies row
  // 16 h + 8 rr + (li >> 1), columns 16 (g & 1) + 8 (li & 1) of the block (li = l & 15), for the
  // two 8-row reads rr = 0, 1 (k bytes 16h .. 16h + 7 and 16h + 8 .. 16h + 15 of its column)
  const int li = lane & 15, gq = (lane >> 4) & 1;
  auto frags = [&](int buf) {
    auto As = reinterpret_cast<const int8_t (*)[BM][kPitch2]>(lds + buf * BUF);
    const int8_t* Bs = lds + buf * BUF + ABUF;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
      for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int i = 0; i < WBM; ++i) {
          const int row = wm * 32 * WBM + i * 32 + r;
          fa[kk][p][i] = *reinterpret_cast<const i32x4*>(&As[p][row][16 * i8_chunk(row, 2 * kk + h)]);
        }
#pragma unroll
        for (int j = 0; j < WBN; ++j) {
          const int col = wn * 32 * WBN + j * 32 + 16 * gq + 8 * (li & 1);
          const int8_t* b0 = Bs + (size_t)p * kKT2 * BP + (32 * kk + 16 * h + (li >> 1)) * BP + col;
          const v2i32_t lo = tr_b8(b0), hi = tr_b8(b0 + 8 * BP);
          fb[kk][p][j] = i32x4{lo.x, lo.y, hi.x, hi.y};
        }
      }
  };
  auto mma = [&]() {
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q < P; ++q)
#pragma unroll
          for (int i = 0; i < WBM; ++i)
#pragma unroll
            for (int j = 0; j < WBN; ++j)
              acc[p + q][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[kk][p][i], fb[kk][q][j], acc[p + q][i][j], 0, 0, 0);
  };

  // (no split of the MFMA k-steps as in v2: with four planes the two fragment sets spill)
  const int nk = (K + kKT2 - 1) / kKT2;
  load(0);
  stage(0);
  if (nk > 1) load(kKT2);
  __syncthreads();
  int kt = 0;
  for (; kt + 2 < nk; ++kt) {
    const int cur = kt & 1;
    frags(cur);
    stage(cur ^ 1);
    load((kt + 2) * kKT2);
    mma();
#pragma unroll
    for (int i = 0; i < KS * P * P * WBM * WBN; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                 // one MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);                 // then up to 6 VALU (DESIGN §4 has the sweep)
    }
    __syncthreads();
  }
  for (; kt < nk; ++kt) {
    const int cur = kt & 1;
    frags(cur);
    if (kt + 1 < nk) stage(cur ^ 1);
    mma();
    __syncthreads();
  }

  // ---- epilogue (as v2): partial sums reduced once, the output tile staged in LDS, 16-B stores
  constexpr int NQB = kKT2;                                 // one column partial per staged k-row
  int64_t* rs = reinterpret_cast<int64_t*>(lds);            // [AQ][BM]
  int64_t* cs = rs + AQ * BM;                               // [64 k-rows][BN]
  int64_t* rfin = cs + NQB * BN;
  int64_t* cfin = rfin + BM;
  int32_t* ct = reinterpret_cast<int32_t*>(cfin + BN);
  int64_t* is = reinterpret_cast<int64_t*>(ct + BM * BN);   // CX: [AQ][BM] partial imaginary sums
  int64_t* ifin = is + AQ * BM;                             // CX: [BM] final ones
  if constexpr (CX) rs[(tid % AQ) * BM + ar] = my_rsum + my_isum;
  else rs[(tid % AQ) * BM + ar] = my_rsum;
  if constexpr (CX) is[(tid % AQ) * BM + ar] = my_isum;
#pragma unroll
  for (int c = 0; c < EB; ++c) {
    if constexpr (CX) {                          // an odd row staged (~d, c): the sums of those words
      int64_t v = (int64_t)my_csum[c];
      if (odd) v = (c & 1) ? (int64_t)my_csum[c - 1] : -(int64_t)my_csum[c + 1] - (int64_t)nk;
      cs[bk * BN + bc + c] = v;
    } else {
      cs[bk * BN + bc + c] = (int64_t)my_csum[c];
    }
  }
  __syncthreads();
  for (int i = tid; i < BM + BN; i += kNT2) {
    int64_t sum = 0;
    if (i < BM) {
#pragma unroll
      for (int q = 0; q < AQ; ++q) sum += rs[q * BM + i];
      rfin[i] = sum;
      if constexpr (CX) {
        int64_t isum = 0;
#pragma unroll
        for (int q = 0; q < AQ; ++q) isum += is[q * BM + i];
        ifin[i] = isum;
      }
    } else {
      for (int q = 0; q < NQB; ++q) sum += cs[q * BN + (i - BM)];
      cfin[i - BM] = sum;
    }
  }
  __syncthreads();
  const int64_t kpad = (int64_t)nk * kKT2;
#pragma unroll
  for (int j = 0; j < WBN; ++j) {
    const int cc = wn * 32 * WBN + j * 32 + r;
    const int64_t csum = cfin[cc];
    const int gcol = col0 + cc;
#pragma unroll
    for (int i = 0; i < WBM; ++i) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int rr = wm * 32 * WBM + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const int grow = row0 + rr;
        uint64_t v = (uint64_t)(C0 * (rfin[rr] + csum)) - (uint64_t)kpad * (uint64_t)(C0 * C0);
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) v += (uint64_t)(int64_t)acc[s2][i][j][reg] << (8 * s2);
        if constexpr (CX) {
          if (!(cc & 1)) v += (uint64_t)ifin[rr];             // real outputs: b (~d) + b = -b d
        }
        const int64_t sum = (int64_t)v;
        int32_t o;
        if constexpr (CX) o = clip_q63_q31(sum >> 31);       // arm_mat_cmplx_mult_q31.c:1029-1030
        else o = (int32_t)(sum >> 31);
        if constexpr (FULL) ct[rr * BN + cc] = o;
        else if (grow < M && gcol < N) C[(size_t)grow * N + gcol] = o;
      }
    }
  }
  if constexpr (FULL) {
    __syncthreads();
    constexpr int VPR = BN * 4 / 16;
#pragma unroll
    for (int w = tid; w < BM * VPR; w += kNT2) {
      const int rr = w / VPR, cw = w % VPR;
      *reinterpret_cast<uint4*>(C + (size_t)(row0 + rr) * N + col0 + cw * 4) =
          *reinterpret_cast<const uint4*>(ct + rr * BN + cw * 4);
    }
  }
}

// K beyond the i8 accumulators' exact range: one thread per output, int64 sum.
template <typename T>
__global__ __launch_bounds__(256) void mat_mult_fixed_valu_kernel(const T* __restrict__ A, const T* __restrict__ B,
                                                                  T* __restrict__ C, int M, int K, int N,
                                                                  int fast) {
  // grid x = batch * M * ceil(N / 256) (grid y / z stop at 65,535)
  const uint32_t nb = (uint32_t)(N + 255) / 256, per = (uint32_t)M * nb, in = blockIdx.x % per;
  const size_t bz = blockIdx.x / per;
  const int i = (int)(in / nb), j = (int)(in % nb) * 256 + threadIdx.x;
  if (j >= N) return;
  const T* a = A + bz * (size_t)M * K + (size_t)i * K;
  const T* b = B + bz * (size_t)K * N + j;
  uint64_t sum = 0;
  for (int k = 0; k < K; ++k) sum += (uint64_t)((int64_t)a[k] * b[(size_t)k * N]);
  const int64_t s = (int64_t)sum;
  if constexpr (sizeof(T) == 2)
    C[bz * (size_t)M * N + (size_t)i * N + j] = fast ? (T)((int32_t)(uint32_t)sum >> 15) : (T)ssat16((int32_t)(s >> 15));
  else C[bz * (size_t)M * N + (size_t)i * N + j] = (T)(int32_t)(s >> 31);
}

// CX beyond that range: one thread per output word (column j = 2n + part), the reference's q63 sum
// (wrapping) over the K/2 complex terms; M, K, N are the embedded real shape.
template <typename T>
__global__ __launch_bounds__(256) void mat_cmplx_mult_fixed_valu_kernel(const T* __restrict__ A,
                                                                        const T* __restrict__ B, T* __restrict__ C,
                                                                        int M, int K, int N) {
  const uint32_t nb = (uint32_t)(N + 255) / 256, per = (uint32_t)M * nb, in = blockIdx.x % per;
  const size_t bz = blockIdx.x / per;
  const int i = (int)(in / nb), j = (int)(in % nb) * 256 + threadIdx.x;
  if (j >= N) return;
  const T* a = A + bz * (size_t)M * K + (size_t)i * K;
  const T* b = B + bz * (size_t)(K / 2) * N + (j & ~1);
  uint64_t sum = 0;
  for (int k = 0; k < K / 2; ++k) {
    const int64_t ar = a[2 * k], ai = a[2 * k + 1], br = b[(size_t)k * N], bi = b[(size_t)k * N + 1];
    if (j & 1) sum += (uint64_t)(ar * bi) + (uint64_t)(ai * br);
    else sum += (uint64_t)(ar * br) - (uint64_t)(ai * bi);
  }
  const int64_t s = (int64_t)sum;
  if constexpr (sizeof(T) == 2) C[bz * (size_t)M * N + (size_t)i * N + j] = (T)ssat16((int32_t)(s >> 15));
  else C[bz * (size_t)M * N + (size_t)i * N + j] = (T)clip_q63_q31(s >> 31);
}

template <typename T, bool CX = false>
static hipError_t launch_fixed(int m, int k, int n, const T* a, const T* b, T* c, uint32_t batch, hipStream_t st,
                               int fast = 0) {
  if (batch == 0 || m == 0 || n == 0) return hipSuccess;
  if (k == 0) return hipMemsetAsync(c, 0, sizeof(T) * (size_t)m * n * batch, st);
  if (k <= kMatI8MaxK) {
    using G = I8Cfg<T>;
    const int tiles = ((m + G::BM - 1) / G::BM) * ((n + G::BN - 1) / G::BN);
    const bool full = m % G::BM == 0 && n % G::BN == 0 && k % G::KT == 0 &&
                      ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0 && (k * sizeof(T)) % 16 == 0 &&
                      (n * sizeof(T)) % 16 == 0 && ((uintptr_t)c & 15) == 0;
    const uint64_t blocks = (uint64_t)tiles * batch;
    if (blocks > kMaxGridX) return grid_limit_error("tiles x batch");
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kNT2), 0, st, a, b, c, m, k, n, fast);
    };
    if constexpr (sizeof(T) == 2) full ? go(mat_mult_i8v2_kernel<true, CX>) : go(mat_mult_i8v2_kernel<false, CX>);
    else full ? go(mat_mult_i8v3_kernel<true, CX>) : go(mat_mult_i8v3_kernel<false, CX>);
  } else {
    const uint64_t blocks = (uint64_t)((n + 255) / 256) * m * batch;
    if (blocks > kMaxGridX) return grid_limit_error("row blocks x batch");
    if (CX)
      hipLaunchKernelGGL(mat_cmplx_mult_fixed_valu_kernel<T>, dim3((uint32_t)blocks), dim3(256), 0, st, a, b, c, m, k, n);
    else
      hipLaunchKernelGGL(mat_mult_fixed_valu_kernel<T>, dim3((uint32_t)blocks), dim3(256), 0, st, a, b, c, m, k, n, fast);
  }
  return hipGetLastError();
}

// ============================================================================================
// arm_mat_mult_fast_q31 (arm_mat_mult_fast_q31.c:152-166 / :215-266, !ARM_MATH_DSP):
// sum = (q31)(((q63)sum << 32 + a*b) >> 32) per product, i.e. sum += (a*b) >> 32 mod 2^32,
// output sum << 1.  Not an exact-product GEMM (every product is floored on its own), so it
// runs on the VALU: one v_mul_hi_i32 + one v_add per MAC, 64 x 64 tiles of 256 threads
// (4 x 4 outputs per thread), 16-deep K steps staged in LDS (A k-major so each thread reads
// its 4 rows as one 16-B word).
constexpr int kFQ_T = 64, kFQ_K = 16;
__global__ __launch_bounds__(256) void mat_mult_fast_q31_kernel(const int32_t* __restrict__ A,
                                                                const int32_t* __restrict__ B,
                                                                int32_t* __restrict__ C, int M, int K, int N,
                                                                int tiles_n) {
  __shared__ __attribute__((aligned(16))) int32_t As[kFQ_K][kFQ_T + 4];
  __shared__ __attribute__((aligned(16))) int32_t Bs[kFQ_K][kFQ_T + 4];
  const int tid = threadIdx.x;
  // grid x = batch * tiles (grid y / z stop at 65,535)
  const uint32_t tiles = (uint32_t)tiles_n * (uint32_t)((M + kFQ_T - 1) / kFQ_T), tile = blockIdx.x % tiles;
  const size_t bz = blockIdx.x / tiles;
  const int row0 = (int)(tile / tiles_n) * kFQ_T, col0 = (int)(tile % tiles_n) * kFQ_T;
  const int32_t* a = A + bz * (size_t)M * K;
  const int32_t* b = B + bz * (size_t)K * N;
  const int tr = (tid / 16) * 4, tc = (tid % 16) * 4;
  uint32_t acc[4][4] = {};
  // loaders: A tile 64 x 16 (thread -> row tid/4, k 4*(tid%4) .. +3), B tile 16 x 64
  const int ar = tid / 4, ak = (tid % 4) * 4;
  const int bk = tid / 16, bc = (tid % 16) * 4;
  for (int k0 = 0; k0 < K; k0 += kFQ_K) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int gr = row0 + ar, gk = k0 + ak + u;
      As[ak + u][ar] = (gr < M && gk < K) ? a[(size_t)gr * K + gk] : 0;
      const int gk2 = k0 + bk, gc = col0 + bc + u;
      Bs[bk][bc + u] = (gk2 < K && gc < N) ? b[(size_t)gk2 * N + gc] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kFQ_K; ++kk) {
      const int4 av = *reinterpret_cast<const int4*>(&As[kk][tr]);
      const int4 bv = *reinterpret_cast<const int4*>(&Bs[kk][tc]);
      const int32_t ar4[4] = {av.x, av.y, av.z, av.w}, bc4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += (uint32_t)mulhi(ar4[i], bc4[j]);
    }
    __syncthreads();
  }
  int32_t* c = C + bz * (size_t)M * N;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gr = row0 + tr + i, gc = col0 + tc + j;
      if (gr < M && gc < N) c[(size_t)gr * N + gc] = (int32_t)(acc[i][j] << 1);
    }
}

hipError_t mat_mult_fast_q31_launch(int m, int k, int n, const int32_t* a, const int32_t* b, int32_t* c,
                                    uint32_t batch, hipStream_t st) {
  if (batch == 0 || m == 0 || n == 0) return hipSuccess;
  const int tn = (n + kFQ_T - 1) / kFQ_T, tm = (m + kFQ_T - 1) / kFQ_T;
  const uint64_t blocks = (uint64_t)tm * tn * batch;
  if (blocks > kMaxGridX) return grid_limit_error("tiles x batch");
  hipLaunchKernelGGL(mat_mult_fast_q31_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, a, b, c, m, k, n, tn);
  return hipGetLastError();
}
hipError_t mat_mult_fast_q15_launch(int m, int k, int n, const int16_t* a, const int16_t* b, int16_t* c,
                                    uint32_t batch, hipStream_t st) {
  return launch_fixed<int16_t>(m, k, n, a, b, c, batch, st, 1);
}

hipError_t mat_mult_q15_launch(int m, int k, int n, const int16_t* a, const int16_t* b, int16_t* c, uint32_t batch,
                               hipStream_t st) {
  return launch_fixed<int16_t>(m, k, n, a, b, c, batch, st);
}
hipError_t mat_mult_q31_launch(int m, int k, int n, const int32_t* a, const int32_t* b, int32_t* c, uint32_t batch,
                               hipStream_t st) {
  return launch_fixed<int32_t>(m, k, n, a, b, c, batch, st);
}

// m, k, n count complex elements (arm_matrix_instance dimensions are uint16_t, so the embedded real
// depth and width fit an int); 2k <= kMatI8MaxK, i.e. k <= 16352, runs on the matrix cores
hipError_t mat_cmplx_mult_q15_launch(int m, int k, int n, const int16_t* a, const int16_t* b, int16_t* c,
                                     uint32_t batch, hipStream_t st) {
  return launch_fixed<int16_t, true>(m, 2 * k, 2 * n, a, b, c, batch, st);
}
hipError_t mat_cmplx_mult_q31_launch(int m, int k, int n, const int32_t* a, const int32_t* b, int32_t* c,
                                     uint32_t batch, hipStream_t st) {
  return launch_fixed<int32_t, true>(m, 2 * k, 2 * n, a, b, c, batch, st);
}

// one thread per complex element; 2-byte accesses (pData need not be 4-byte aligned)
__global__ __launch_bounds__(256) void mat_cmplx_trans_q15_kernel(const int16_t* __restrict__ b,
                                                                  int16_t* __restrict__ bt, int k, int n) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (uint32_t)k * (uint32_t)n) return;
  const uint32_t r = idx / (uint32_t)n, c = idx % (uint32_t)n;
  const size_t o = 2 * ((size_t)c * k + r);
  bt[o] = b[2 * (size_t)idx];
  bt[o + 1] = b[2 * (size_t)idx + 1];
}
hipError_t mat_cmplx_trans_q15_launch(int k, int n, const int16_t* b, int16_t* bt, hipStream_t st) {
  const uint64_t total = (uint64_t)k * n;      // < 2^32 for uint16_t dimensions
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(mat_cmplx_trans_q15_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, b, bt, k, n);
  return hipGetLastError();
}

}  // namespace mi355x
