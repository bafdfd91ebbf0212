// What the two HMM scans share (hmm.hip: Viterbi, max-plus over int64; hmm_fb.hip: forward-backward, sum-product
// over scaled fp64): the chunking constants, the sequence-boundary flags and the levels of the grouped scans.
// Everything here has internal linkage: each translation unit gets its own copy.
#pragma once

#include "common.h"

#include <climits>

namespace {

constexpr int HMM_KMAX = 32;
constexpr int HMM_L = 64;        // steps per chunk (default; the launchers take any L >= 1)
constexpr int HMM_G = 32;        // chunks (matrices / maps) per group of the grouped scans
constexpr int HMM_BLOCK = 256;
constexpr int FLAG_START = 1, FLAG_END = 2;

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// flags[t]: bit 0 = a sequence starts at t, bit 1 = a sequence ends at t (zeroed before).  first_end[c] = the
// first sequence that ends inside chunk c (written by that sequence's lane; chunks without an end keep 0).
__global__ __launch_bounds__(HMM_BLOCK) void hmm_flags_kernel(const int64_t* __restrict__ off, int64_t S, int64_t T, int L,
                                                              uint8_t* __restrict__ flags, int32_t* __restrict__ first_end) {
  const int64_t s = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  if (s >= S) return;
  const int64_t b = off[s], e = off[s + 1] - 1;
  if (b < 0 || e < b || e >= T) return;  // (the host validated the offsets: keeps the stores in range)
  if (b == e) {
    flags[b] = FLAG_START | FLAG_END;
  } else {
    flags[b] = FLAG_START;
    flags[e] = FLAG_END;
  }
  const int64_t c = e / L;
  if (s == 0 || (b - 1) / L != c) first_end[c] = (int32_t)s;
}

inline int hmm_kp(int K) {
  int kp = 2;
  while (kp < K) kp <<= 1;
  return kp;
}

inline unsigned blocks(int64_t threads) { return (unsigned)((threads + HMM_BLOCK - 1) / HMM_BLOCK); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The levels of a grouped scan over C chunks: n[0] = C, n[l + 1] = ceil(n[l] / G) while n[l] > G.
struct HmmLevels {
  static constexpr int MAXLV = 8;  // 2^31 steps / 32^7 < 1
  int64_t C = 0;
  int nlv = 0;
  int64_t n[MAXLV] = {};
  bool ok = false;
};

inline HmmLevels hmm_levels(int64_t T, int K, int64_t S, int L) {
  HmmLevels p;
  if (T < 1 || T > (int64_t)INT_MAX || K < 1 || K > HMM_KMAX || S < 1 || S > T || L < 1) return p;
  p.C = (T + L - 1) / L;
  p.n[0] = p.C;
  p.nlv = 1;
  while (p.n[p.nlv - 1] > HMM_G) {
    if (p.nlv == HmmLevels::MAXLV) return p;
    p.n[p.nlv] = (p.n[p.nlv - 1] + HMM_G - 1) / HMM_G;
    ++p.nlv;
  }
  p.ok = true;
  return p;
}

}  // namespace
