// arm_sort_f32 / arm_merge_sort_f32 over a batch of contiguous items: a bitonic sorting network on 32-bit keys.
//
//   key       the word's IEEE total-order image, bits ^ ((bits >> 31) & 0x7fffffff) compared as signed (an involution):
//             negative NaNs < -Inf < .. < -0.0 < +0.0 < .. < +Inf < positive NaNs.  Two words with equal keys are the
//             same word, so the sorted output is unique by bits and needs no index tie-break.  Descending sorts the
//             complemented key ascending.
//   network   the all-ascending formulation (as the reference's scalar arm_bitonic_sort_f32 builds it): the merge of
//             two sorted runs of s / 2 opens with the mirrored compare (i against base + s - 1 - k), then half-cleaners
//             of stride s / 4 .. 1.  Every compare-exchange puts the smaller key at the lower index, so positions at
//             or beyond n, which behave as maximal keys, never move: in registers and LDS they are filled with
//             INT32_MAX (a real key of that value is indistinguishable from the filler and ends in the same place),
//             in global memory their compares are skipped.  Any n works in place on dst, without a padded buffer.
//   tiers     by the padded length P (n rounded up to a power of two):
//             P <= kSortWaveMax (256): one wave per item, kBlock / 64 items per workgroup, no barrier.  A lane
//               holds E = P / 64 (1, 2, 4) consecutive keys in registers with static indices; strides below E are
//               compares inside the lane, the others one cross-lane move (__shfl_xor) per key.
//             P <= kSortLdsMax (16384 keys, 64 KiB): one workgroup per item.  Each wave sorts tiles of 256 keys in
//               registers as above and stores them to LDS; then per merge the strides of 256 and more run on LDS
//               with one barrier each, and the strides below 256 again in registers, tile by tile, with one barrier.
//             longer: workgroups sort kSortLdsMax-key chunks as above (sort_lds_kernel, kChunkSort), then per merge
//               the strides of kSortLdsMax and more are global compare-exchange passes (sort_global_kernel, one
//               launch per stride) and the rest of the merge runs per chunk in LDS again (kChunkTail).  Between the
//               launches dst holds keys; the last launch turns them back into words.
#include "common.hpp"
#include "kernels.hpp"

namespace mi355x {
namespace {

constexpr int32_t kPad = INT32_MAX;
constexpr int kTileE = 4, kTile = 64 * kTileE;          // keys per lane and per register tile of the LDS tier

__device__ __forceinline__ int32_t to_key(uint32_t bits, bool asc) {
  const int32_t b = (int32_t)bits, k = b ^ ((b >> 31) & 0x7fffffff);
  return asc ? k : ~k;
}
__device__ __forceinline__ uint32_t from_key(int32_t key, bool asc) {
  const int32_t k = asc ? key : ~key;
  return (uint32_t)(k ^ ((k >> 31) & 0x7fffffff));
}

__device__ __forceinline__ void cmpx(int32_t& lo, int32_t& hi) {
  const int32_t a = lo, b = hi;
  lo = a < b ? a : b;
  hi = a < b ? b : a;
}

// A register tile: lane l holds the keys of positions l * E + e.  The merge step of run length s (a power of two,
// 2 <= s <= 64 * E): the mirrored compare inside every block of s positions.
template <int E>
__device__ __forceinline__ void tile_mirror(int32_t (&key)[E], uint32_t lane, uint32_t s) {
  if (s <= (uint32_t)E) {                                   // inside the lane: e against e ^ (s - 1)
#pragma unroll
    for (int ss = 2; ss <= E; ss <<= 1) {
      if ((uint32_t)ss == s) {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (e < (e ^ (ss - 1))) cmpx(key[e], key[e ^ (ss - 1)]);
      }
    }
  } else {                                                  // lane ^ (s / E - 1), register E - 1 - e
    const uint32_t m = s / E - 1;
    const bool low = (lane & (s / (2 * E))) == 0;
    int32_t other[E];
#pragma unroll
    for (int e = 0; e < E; ++e) other[e] = __shfl_xor(key[E - 1 - e], (int)m, 64);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const bool less = other[e] < key[e];
      key[e] = (low == less) ? other[e] : key[e];           // low keeps the minimum, high the maximum
    }
  }
}

// The half-cleaners of stride h, h / 2, .. 1 (h a power of two below 64 * E, or 0: none).
template <int E>
__device__ __forceinline__ void tile_clean(int32_t (&key)[E], uint32_t lane, uint32_t h) {
  for (; h >= (uint32_t)E && h > 0; h >>= 1) {              // lane ^ (h / E), the same register
    const uint32_t m = h / E;
    const bool low = (lane & m) == 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int32_t other = __shfl_xor(key[e], (int)m, 64);
      const bool less = other < key[e];
      key[e] = (low == less) ? other : key[e];
    }
  }
#pragma unroll
  for (int hh = E / 2; hh >= 1; hh >>= 1) {                 // inside the lane
    if ((uint32_t)hh <= h) {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if ((e & hh) == 0) cmpx(key[e], key[e + hh]);
    }
  }
}

// Sorts every block of p positions of the tile (p a power of two, 1 <= p <= 64 * E).
template <int E>
__device__ __forceinline__ void tile_sort(int32_t (&key)[E], uint32_t lane, uint32_t p) {
  for (uint32_t s = 2; s <= p; s <<= 1) {
    tile_mirror<E>(key, lane, s);
    tile_clean<E>(key, lane, s >> 2);
  }
}

// One wave per item of n <= 64 * E words; p: n rounded up to a power of two.
template <int E>
__global__ __launch_bounds__(kBlock) void sort_wave_kernel(const uint32_t* src, uint32_t* dst, uint32_t n, uint32_t p,
                                                           bool asc, uint32_t batch) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t item = blockIdx.x * (uint32_t)(kBlock / 64) + (threadIdx.x >> 6);
  if (item >= batch) return;                                // wave-uniform; the kernel has no barrier
  const uint32_t* s = src + (size_t)item * n;
  uint32_t* d = dst + (size_t)item * n;
  int32_t key[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t pos = lane * E + e;
    key[e] = pos < n ? to_key(s[pos], asc) : kPad;
  }
  tile_sort<E>(key, lane, p);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t pos = lane * E + e;
    if (pos < n) d[pos] = from_key(key[e], asc);
  }
}

// One workgroup per chunk of c positions (a power of two, 2 * kTile <= c <= kSortLdsMax) of an item of n words; an item
// has `chunks` of them (the last one may be ragged; chunks wholly beyond n are not launched).
//   kChunkSort  sorts the chunk.  wordsIn: src holds words (otherwise keys).
//   kChunkTail  the half-cleaners of stride c / 2 .. 1 on the chunk, the end of a merge whose larger strides ran in
//               global memory; src == dst holds keys.
// wordsOut: dst receives words (otherwise keys).
enum : int { kChunkSort = 0, kChunkTail = 1 };

template <int MODE>
__global__ __launch_bounds__(kBlock) void sort_lds_kernel(const uint32_t* src, uint32_t* dst, uint32_t n, uint32_t c,
                                                          uint32_t chunks, bool asc, bool wordsIn, bool wordsOut) {
  extern __shared__ int32_t lds[];                          // c keys
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t item = blockIdx.x / chunks;
  const uint32_t base = (blockIdx.x % chunks) * c;          // < n
  const uint32_t live = n - base < c ? n - base : c;        // words of the chunk
  const uint32_t* s = src + item * n + base;
  uint32_t* d = dst + item * n + base;
  const uint32_t tiles = c / kTile;
  int32_t key[kTileE];

  auto load_global = [&](uint32_t t) {
#pragma unroll
    for (int e = 0; e < kTileE; ++e) {
      const uint32_t pos = t * kTile + lane * kTileE + e;
      key[e] = pos < live ? (wordsIn ? to_key(s[pos], asc) : (int32_t)s[pos]) : kPad;
    }
  };
  auto store_global = [&](uint32_t t) {
#pragma unroll
    for (int e = 0; e < kTileE; ++e) {
      const uint32_t pos = t * kTile + lane * kTileE + e;
      if (pos < live) d[pos] = wordsOut ? from_key(key[e], asc) : (uint32_t)key[e];
    }
  };
  auto load_lds = [&](uint32_t t) {
#pragma unroll
    for (int e = 0; e < kTileE; ++e) key[e] = lds[t * kTile + lane * kTileE + e];
  };
  auto store_lds = [&](uint32_t t) {
#pragma unroll
    for (int e = 0; e < kTileE; ++e) lds[t * kTile + lane * kTileE + e] = key[e];
  };
  // half-cleaners of stride h >= kTile on LDS, one barrier each
  auto clean_lds = [&](uint32_t h) {
    for (; h >= (uint32_t)kTile; h >>= 1) {
      for (uint32_t t = threadIdx.x; t < c / 2; t += kBlock) {
        const uint32_t i = (t / h) * 2 * h + (t % h);
        const int32_t a = lds[i], b = lds[i + h];
        if (b < a) { lds[i] = b; lds[i + h] = a; }
      }
      __syncthreads();
    }
  };

  if (MODE == kChunkSort) {
    for (uint32_t t = wave; t < tiles; t += kBlock / 64) {
      load_global(t);
      tile_sort<kTileE>(key, lane, kTile);
      store_lds(t);
    }
    __syncthreads();
    for (uint32_t sLen = 2 * kTile; sLen <= c; sLen <<= 1) {
      for (uint32_t t = threadIdx.x; t < c / 2; t += kBlock) {        // the mirrored compare
        const uint32_t half = sLen / 2, b0 = (t / half) * sLen, k = t % half;
        const uint32_t i = b0 + k, j = b0 + sLen - 1 - k;
        const int32_t a = lds[i], b = lds[j];
        if (b < a) { lds[i] = b; lds[j] = a; }
      }
      __syncthreads();
      clean_lds(sLen / 4);
      const bool last = sLen == c;
      for (uint32_t t = wave; t < tiles; t += kBlock / 64) {
        load_lds(t);
        tile_clean<kTileE>(key, lane, kTile / 2);
        if (last) store_global(t);
        else store_lds(t);
      }
      if (!last) __syncthreads();
    }
  } else {
    for (uint32_t t = wave; t < tiles; t += kBlock / 64) {
      load_global(t);
      store_lds(t);
    }
    __syncthreads();
    clean_lds(c / 2);
    for (uint32_t t = wave; t < tiles; t += kBlock / 64) {
      load_lds(t);
      tile_clean<kTileE>(key, lane, kTile / 2);
      store_global(t);
    }
  }
}

// One compare-exchange per lane on keys in global memory: the mirrored compare of run length s (mirror), or the
// half-cleaner of stride s / 2.  pairsLog: log2 of the pairs per item (the padded length / 2).  A pair whose upper
// position is at or beyond n is skipped.
__global__ __launch_bounds__(kBlock) void sort_global_kernel(uint32_t* dst, uint32_t n, uint64_t s, bool mirror,
                                                             int pairsLog, size_t total) {
  const size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const size_t item = idx >> pairsLog;
  const uint64_t t = idx & (((uint64_t)1 << pairsLog) - 1), half = s / 2;
  const uint64_t b0 = (t / half) * s, k = t % half;
  const uint64_t i = b0 + k, j = mirror ? b0 + s - 1 - k : i + half;
  if (j >= n) return;
  int32_t* p = (int32_t*)dst + item * n;
  const int32_t a = p[i], b = p[j];
  if (b < a) { p[i] = b; p[j] = a; }
}

template <int E>
hipError_t wave_run(const uint32_t* src, uint32_t* dst, uint32_t n, uint32_t p, bool asc, uint32_t batch,
                    hipStream_t st) {
  const uint32_t ipw = kBlock / 64;
  const dim3 grid((uint32_t)(((uint64_t)batch + ipw - 1) / ipw));
  hipLaunchKernelGGL((sort_wave_kernel<E>), grid, dim3(kBlock), 0, st, src, dst, n, p, asc, batch);
  return hipGetLastError();
}

}  // namespace

hipError_t sort_launch(const uint32_t* src, uint32_t* dst, uint32_t n, bool asc, uint32_t batch, hipStream_t st) {
  if (batch == 0 || n == 0) return hipSuccess;
  if (n > 0x80000000u) return hipErrorInvalidValue;
  uint64_t p = 1;
  int pLog = 0;
  while (p < n) { p <<= 1; ++pLog; }
  if (p <= 64) return wave_run<1>(src, dst, n, (uint32_t)p, asc, batch, st);
  if (p == 128) return wave_run<2>(src, dst, n, (uint32_t)p, asc, batch, st);
  if (p <= kSortWaveMax) return wave_run<4>(src, dst, n, (uint32_t)p, asc, batch, st);
  const uint32_t c = p < kSortLdsMax ? (uint32_t)p : kSortLdsMax;
  const uint64_t chunks = ((uint64_t)n + c - 1) / c, grid = chunks * batch;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  const size_t ldsBytes = (size_t)c * sizeof(int32_t);
  const bool one = p <= kSortLdsMax;
  hipLaunchKernelGGL((sort_lds_kernel<kChunkSort>), dim3((uint32_t)grid), dim3(kBlock), ldsBytes, st, src, dst, n, c,
                     (uint32_t)chunks, asc, true, one);
  hipError_t e = hipGetLastError();
  if (one || e != hipSuccess) return e;
  const size_t total = (size_t)batch << (pLog - 1);
  const size_t gblocks = (total + kBlock - 1) / kBlock;
  if (gblocks > 0x7fffffffull) return hipErrorInvalidValue;
  for (uint64_t s = 2 * (uint64_t)c; s <= p; s <<= 1) {
    for (uint64_t h = s; h >= 2 * (uint64_t)c; h >>= 1) {   // h == s: the mirrored compare; below: stride h / 2 >= c
      hipLaunchKernelGGL(sort_global_kernel, dim3((uint32_t)gblocks), dim3(kBlock), 0, st, dst, n, h, h == s,
                         pLog - 1, total);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL((sort_lds_kernel<kChunkTail>), dim3((uint32_t)grid), dim3(kBlock), ldsBytes, st, dst, dst, n, c,
                       (uint32_t)chunks, asc, false, s == p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mi355x
