// Exact parallel Viterbi decoding of a concatenated batch of sequences (har/ops/hmm.py holds the definition).
//
// Scores are integers (int32 quanta of 2^-20, accumulated in int64), so the max-plus products below are exact
// and associative: the chunked decode equals the sequential recurrence bit for bit, ties included.
//
// The batch is ONE scan over T steps.  The step matrix is M_t(i, j) = A(i, j) + E_t(j), or the reset
// pi(j) + E_t(j) (every i) where a sequence starts; the running vector then carries a constant offset across
// a boundary, which changes no argmax, and a sequence's score is the difference of consecutive end maxima.
//
//   1. chunk matrices   the max-plus product of each chunk of L step matrices (one lane per matrix row)
//   2. chunk scan       incoming score vector of every chunk: group products up, vector expansion down
//   3. forward          each chunk again from its true incoming vector: psi [T][K] uint8, the chunk's
//                       backtrace map (state at its last step -> state at the step before its first), end maxima
//   4. map scan         state at every chunk's last step: map compositions up, expansion down
//   5. backtrace        one lane per chunk walks psi backwards and writes path
//   6. scores           score[s] = endmax[s] - endmax[s - 1]
//
// psi_t(j) is the lowest i attaining max_i d_{t-1}(i) + A(i, j); at a step that starts a sequence it is the
// constant lowest argmax of d_{t-1} (the previous sequence's last state), so the backtrace needs no special
// case at a boundary.  No atomics, no device -> host read; every output element has exactly one writer.
#include "hmm_common.h"
#include "../har_kernels.h"

namespace {

__device__ __forceinline__ int64_t shfl64(int64_t v, int src, int width) {
  return (int64_t)__shfl((long long)v, src, width);
}

// Phase 1, K <= 8.  KP lanes per chunk, lane i holds row i of the running product in registers; A (int64) and pi
// sit in LDS at stride KP so every index below is an immediate (the compiler keeps the KP^2 values of A in
// registers across the step loop: 128 VGPRs at KP = 8, which is why wider K takes the kernel after this one).
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void hmm_chunk_mat_kernel(const int32_t* __restrict__ E, const int32_t* __restrict__ A,
                                                                  const int32_t* __restrict__ pi,
                                                                  const uint8_t* __restrict__ flags, int64_t T, int K, int L,
                                                                  int64_t C, int64_t* __restrict__ mats) {
  __shared__ int64_t sA[KP * KP];
  __shared__ int64_t sPi[KP];
  for (int x = threadIdx.x; x < KP * KP; x += HMM_BLOCK) {
    const int r = x / KP, q = x % KP;
    sA[x] = (r < K && q < K) ? (int64_t)A[r * K + q] : 0;
  }
  if (threadIdx.x < KP) sPi[threadIdx.x] = threadIdx.x < K ? (int64_t)pi[threadIdx.x] : 0;
  __syncthreads();
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  const int64_t c = gid / KP;
  const int i = (int)(gid % KP);
  if (c >= C || i >= K) return;
  const int64_t t0 = c * L, t1 = min64(T, t0 + L);
  int64_t P[KP];
  {
    const bool start = flags[t0] & FLAG_START;
    const int32_t* e = E + t0 * K;
#pragma unroll
    for (int j = 0; j < KP; ++j) P[j] = j < K ? (start ? sPi[j] : sA[i * KP + j]) + e[j] : 0;
  }
  for (int64_t t = t0 + 1; t < t1; ++t) {
    const int32_t* e = E + t * K;
    if (flags[t] & FLAG_START) {
      int64_t mx = P[0];
#pragma unroll
      for (int k = 1; k < KP; ++k)
        if (k < K) mx = max64(mx, P[k]);
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < K) P[j] = mx + sPi[j] + e[j];
    } else {
      int64_t N[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        if (j < K) {
          int64_t m = P[0] + sA[j];
#pragma unroll
          for (int k = 1; k < KP; ++k)
            if (k < K) m = max64(m, P[k] + sA[k * KP + j]);
          N[j] = m + e[j];
        }
      }
#pragma unroll
      for (int j = 0; j < KP; ++j)
        if (j < K) P[j] = N[j];
    }
  }
  int64_t* o = mats + (c * K + i) * K;
#pragma unroll
  for (int j = 0; j < KP; ++j)
    if (j < K) o[j] = P[j];
}

// Phase 1, K > 8.  One workgroup of KP^2 lanes per chunk, lane (i, j) holds P(i, j) and column j of A; row i of
// the running product goes through LDS (double buffered: one barrier per step).
template <int KP>
__global__ __launch_bounds__(KP * KP) void hmm_chunk_mat_wide_kernel(const int32_t* __restrict__ E,
                                                                     const int32_t* __restrict__ A,
                                                                     const int32_t* __restrict__ pi,
                                                                     const uint8_t* __restrict__ flags, int64_t T, int K,
                                                                     int L, int64_t C, int64_t* __restrict__ mats) {
  __shared__ int64_t sP[2][KP * KP];
  const int tid = threadIdx.x, i = tid / KP, j = tid % KP;
  const int64_t c = blockIdx.x;
  if (c >= C) return;  // (block-uniform)
  const bool ok = i < K && j < K;
  int64_t a[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) a[k] = (k < K && j < K) ? (int64_t)A[k * K + j] : 0;
  const int64_t pj = j < K ? (int64_t)pi[j] : 0;
  const int64_t t0 = c * L, t1 = min64(T, t0 + L);
  int64_t p = 0;
  if (ok) p = ((flags[t0] & FLAG_START) ? pj : (int64_t)A[i * K + j]) + E[t0 * K + j];
  int buf = 0;
  for (int64_t t = t0 + 1; t < t1; ++t) {
    sP[buf][tid] = p;
    __syncthreads();
    const int64_t* row = &sP[buf][i * KP];
    const int64_t e = ok ? (int64_t)E[t * K + j] : 0;
    int64_t m;
    if (flags[t] & FLAG_START) {  // block-uniform
      m = row[0];
#pragma unroll
      for (int k = 1; k < KP; ++k)
        if (k < K) m = max64(m, row[k]);
      m += pj;
    } else {
      m = row[0] + a[0];
#pragma unroll
      for (int k = 1; k < KP; ++k)
        if (k < K) m = max64(m, row[k] + a[k]);
    }
    p = ok ? m + e : 0;
    buf ^= 1;
  }
  if (ok) mats[(c * K + i) * K + j] = p;
}

// Phase 2 up: out[g] = in[g G] (x) in[g G + 1] (x) ... (max-plus), lane i holds row i.
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void hmm_mat_reduce_kernel(const int64_t* __restrict__ in, int64_t n, int K, int G,
                                                                   int64_t ng, int64_t* __restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  const int64_t g = gid / KP;
  const int i = (int)(gid % KP);
  if (g >= ng || i >= K) return;
  const int64_t c0 = g * G, c1 = min64(n, c0 + G);
  int64_t P[KP];
  {
    const int64_t* m = in + (c0 * K + i) * K;
#pragma unroll
    for (int j = 0; j < KP; ++j) P[j] = j < K ? m[j] : 0;
  }
  for (int64_t c = c0 + 1; c < c1; ++c) {
    const int64_t* m = in + c * K * K;
    int64_t N[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      if (j < K) {
        int64_t v = P[0] + m[j];
#pragma unroll
        for (int k = 1; k < KP; ++k)
          if (k < K) v = max64(v, P[k] + m[k * K + j]);
        N[j] = v;
      }
    }
#pragma unroll
    for (int j = 0; j < KP; ++j)
      if (j < K) P[j] = N[j];
  }
  int64_t* o = out + (g * K + i) * K;
#pragma unroll
  for (int j = 0; j < KP; ++j)
    if (j < K) o[j] = P[j];
}

// Phase 2 down: vout[c] = the vector entering matrix c, from the vector entering its group (null = zeros).
// KP lanes per group, lane j holds v(j); the other lanes' values come by shuffles inside the group.
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void hmm_vec_expand_kernel(const int64_t* __restrict__ mats,
                                                                   const int64_t* __restrict__ vin, int64_t n, int K, int G,
                                                                   int64_t ng, int64_t* __restrict__ vout) {
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  const int64_t g = gid / KP;
  const int j = (int)(gid % KP);
  if (g >= ng) return;  // whole groups leave: the shuffles below stay inside a group
  const bool ok = j < K;
  const int64_t c0 = g * G, c1 = min64(n, c0 + G);
  int64_t v = (ok && vin != nullptr) ? vin[g * K + j] : 0;
  for (int64_t c = c0; c < c1; ++c) {
    if (ok) vout[c * K + j] = v;
    if (c + 1 == c1) break;
    const int64_t* m = mats + c * K * K;
    int64_t nv = LLONG_MIN;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      if (i < K) {
        const int64_t vi = shfl64(v, i, KP);
        if (ok) nv = max64(nv, vi + m[i * K + j]);
      }
    }
    v = nv;
  }
}

// Phase 3.  KP lanes per chunk, lane j holds d(j) and column j of A.
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void hmm_forward_kernel(const int32_t* __restrict__ E, const int32_t* __restrict__ A,
                                                                const int32_t* __restrict__ pi,
                                                                const uint8_t* __restrict__ flags,
                                                                const int64_t* __restrict__ vin,
                                                                const int32_t* __restrict__ first_end, int64_t T, int64_t S, int K,
                                                                int L, int64_t C, uint8_t* __restrict__ psi, uint8_t* __restrict__ maps,
                                                                int64_t* __restrict__ endmax, uint8_t* __restrict__ final_state) {
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  const int64_t c = gid / KP;
  const int j = (int)(gid % KP);
  if (c >= C) return;  // whole groups leave
  const bool ok = j < K;
  int64_t a[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) a[i] = (ok && i < K) ? (int64_t)A[i * K + j] : 0;
  const int64_t pj = ok ? (int64_t)pi[j] : 0;
  int64_t d = ok ? vin[c * K + j] : 0;
  const int64_t t0 = c * L, t1 = min64(T, t0 + L);
  int64_t sidx = first_end[c];
  int m = 0;
  for (int64_t t = t0; t < t1; ++t) {
    const int f = flags[t];
    const bool start = f & FLAG_START;
    int64_t best = LLONG_MIN;
    int arg = 0;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      if (i < K) {
        const int64_t cand = shfl64(d, i, KP) + (start ? 0 : a[i]);
        if (cand > best) {  // strict: the lowest i of equal candidates stays
          best = cand;
          arg = i;
        }
      }
    }
    d = best + (start ? pj : 0) + (ok ? (int64_t)E[t * K + j] : 0);
    if (ok) psi[t * K + j] = (uint8_t)arg;
    // backtrace map: m(x) = the state at t0 - 1 given state x at t
    const int mm = __shfl(m, arg, KP);
    m = t == t0 ? arg : mm;
    if (f & FLAG_END) {  // uniform inside the group
      int64_t mx = LLONG_MIN;
#pragma unroll
      for (int i = 0; i < KP; ++i)
        if (i < K) mx = max64(mx, shfl64(d, i, KP));
      if (j == 0 && sidx < S) endmax[sidx] = mx;
      ++sidx;
    }
  }
  if (ok) maps[c * K + j] = (uint8_t)m;
  if (c == C - 1) {
    int64_t best = LLONG_MIN;
    int arg = 0;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      if (i < K) {
        const int64_t v = shfl64(d, i, KP);
        if (v > best) {
          best = v;
          arg = i;
        }
      }
    }
    if (j == 0) final_state[0] = (uint8_t)arg;
  }
}

// Phase 4 up: out[g](x) = maps[g G]( ... maps[g G + G - 1](x)): one lane per (group, x).
__global__ __launch_bounds__(HMM_BLOCK) void hmm_map_reduce_kernel(const uint8_t* __restrict__ maps, int64_t n, int K, int G,
                                                                   int64_t ng, uint8_t* __restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  if (gid >= ng * K) return;
  const int64_t g = gid / K;
  int cur = (int)(gid % K);
  const int64_t c0 = g * G, c1 = min64(n, c0 + G);
  for (int64_t c = c1 - 1; c >= c0; --c) cur = min((int)maps[c * K + cur], K - 1);
  out[gid] = (uint8_t)cur;
}

// Phase 4 down: rout[c] = the state at the last step of chunk c, from the state at the last step of its group.
__global__ __launch_bounds__(HMM_BLOCK) void hmm_map_expand_kernel(const uint8_t* __restrict__ maps,
                                                                   const uint8_t* __restrict__ rin, int64_t n, int K, int G,
                                                                   int64_t ng, uint8_t* __restrict__ rout) {
  const int64_t g = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  if (g >= ng) return;
  const int64_t c0 = g * G, c1 = min64(n, c0 + G);
  int cur = min((int)rin[g], K - 1);
  for (int64_t c = c1 - 1; c >= c0; --c) {
    rout[c] = (uint8_t)cur;
    cur = min((int)maps[c * K + cur], K - 1);
  }
}

// Phase 5: one lane per chunk.
__global__ __launch_bounds__(HMM_BLOCK) void hmm_backtrace_kernel(const uint8_t* __restrict__ psi,
                                                                  const uint8_t* __restrict__ last, int64_t T, int K, int L,
                                                                  int64_t C, int32_t* __restrict__ path) {
  const int64_t c = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  if (c >= C) return;
  const int64_t t0 = c * L, t1 = min64(T, t0 + L);
  int cur = min((int)last[c], K - 1);
  for (int64_t t = t1 - 1; t >= t0; --t) {
    path[t] = cur;
    cur = min((int)psi[t * K + cur], K - 1);
  }
}

__global__ __launch_bounds__(HMM_BLOCK) void hmm_score_kernel(const int64_t* __restrict__ endmax, int64_t S,
                                                              int64_t* __restrict__ score) {
  const int64_t s = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  if (s >= S) return;
  score[s] = endmax[s] - (s > 0 ? endmax[s - 1] : 0);
}

// The workspace: every buffer of a decode, 256-byte aligned.  levels: n[0] = C chunks, n[l + 1] =
// ceil(n[l] / G) while n[l] > G.
struct HmmPlan {
  static constexpr int MAXLV = HmmLevels::MAXLV;
  int64_t C = 0;
  int nlv = 0;
  int64_t n[MAXLV] = {};
  size_t flags = 0, psi = 0, first_end = 0, endmax = 0, final_state = 0;
  size_t mats[MAXLV] = {}, vecs[MAXLV] = {}, maps[MAXLV] = {}, last[MAXLV] = {};
  size_t bytes = 0;
  bool ok = false;
};

HmmPlan hmm_plan(int64_t T, int K, int64_t S, int L) {
  HmmPlan p;
  const HmmLevels lv = hmm_levels(T, K, S, L);
  if (!lv.ok) return p;
  p.C = lv.C;
  p.nlv = lv.nlv;
  for (int l = 0; l < lv.nlv; ++l) p.n[l] = lv.n[l];
  size_t o = 0;
  auto take = [&o](size_t b) {
    const size_t at = o;
    o += align256(b);
    return at;
  };
  p.flags = take((size_t)T);
  p.psi = take((size_t)T * K);
  p.first_end = take((size_t)p.C * sizeof(int32_t));
  p.endmax = take((size_t)S * sizeof(int64_t));
  p.final_state = take(1);
  for (int l = 0; l < p.nlv; ++l) {
    p.mats[l] = take((size_t)p.n[l] * K * K * sizeof(int64_t));
    p.vecs[l] = take((size_t)p.n[l] * K * sizeof(int64_t));
    p.maps[l] = take((size_t)p.n[l] * K);
    p.last[l] = take((size_t)p.n[l]);
  }
  p.bytes = o;
  p.ok = true;
  return p;
}

template <int KP>
int hmm_run(const HmmPlan& p, const int32_t* E, const int32_t* A, const int32_t* pi, const int64_t* off, int64_t T, int K,
            int64_t S, int L, uint8_t* ws, int32_t* path, int64_t* score, int lo, int hi, hipStream_t s) {
  uint8_t* flags = ws + p.flags;
  uint8_t* psi = ws + p.psi;
  int32_t* first_end = reinterpret_cast<int32_t*>(ws + p.first_end);
  int64_t* endmax = reinterpret_cast<int64_t*>(ws + p.endmax);
  uint8_t* final_state = ws + p.final_state;
  auto mats = [&](int l) { return reinterpret_cast<int64_t*>(ws + p.mats[l]); };
  auto vecs = [&](int l) { return reinterpret_cast<int64_t*>(ws + p.vecs[l]); };
  auto maps = [&](int l) { return ws + p.maps[l]; };
  auto last = [&](int l) { return ws + p.last[l]; };
  const int top = p.nlv - 1;
  const int64_t C = p.C;
  auto on = [lo, hi](int ph) { return lo <= ph && ph <= hi; };
  if (on(0)) {
    hipError_t e = hipMemsetAsync(flags, 0, (size_t)T, s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(first_end, 0, (size_t)C * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    hmm_flags_kernel<<<blocks(S), HMM_BLOCK, 0, s>>>(off, S, T, L, flags, first_end);
    HAR_CHECK_LAUNCH();
  }
  if (on(1)) {
    if constexpr (KP <= 8)
      hmm_chunk_mat_kernel<KP><<<blocks(C * KP), HMM_BLOCK, 0, s>>>(E, A, pi, flags, T, K, L, C, mats(0));
    else
      hmm_chunk_mat_wide_kernel<KP><<<(unsigned)C, KP * KP, 0, s>>>(E, A, pi, flags, T, K, L, C, mats(0));
    HAR_CHECK_LAUNCH();
  }
  if (on(2)) {
    for (int l = 0; l < top; ++l) {
      hmm_mat_reduce_kernel<KP><<<blocks(p.n[l + 1] * KP), HMM_BLOCK, 0, s>>>(mats(l), p.n[l], K, HMM_G, p.n[l + 1], mats(l + 1));
      HAR_CHECK_LAUNCH();
    }
    // the top level is one group of n[top] <= G matrices entered by the zero vector (step 0 is a reset)
    hmm_vec_expand_kernel<KP><<<blocks(KP), HMM_BLOCK, 0, s>>>(mats(top), nullptr, p.n[top], K, HMM_G, 1, vecs(top));
    HAR_CHECK_LAUNCH();
    for (int l = top - 1; l >= 0; --l) {
      hmm_vec_expand_kernel<KP><<<blocks(p.n[l + 1] * KP), HMM_BLOCK, 0, s>>>(mats(l), vecs(l + 1), p.n[l], K, HMM_G, p.n[l + 1],
                                                                              vecs(l));
      HAR_CHECK_LAUNCH();
    }
  }
  if (on(3)) {
    hmm_forward_kernel<KP><<<blocks(C * KP), HMM_BLOCK, 0, s>>>(E, A, pi, flags, vecs(0), first_end, T, S, K, L, C, psi, maps(0),
                                                                endmax, final_state);
    HAR_CHECK_LAUNCH();
  }
  if (on(4)) {
    for (int l = 0; l < top; ++l) {
      hmm_map_reduce_kernel<<<blocks(p.n[l + 1] * K), HMM_BLOCK, 0, s>>>(maps(l), p.n[l], K, HMM_G, p.n[l + 1], maps(l + 1));
      HAR_CHECK_LAUNCH();
    }
    hmm_map_expand_kernel<<<1, HMM_BLOCK, 0, s>>>(maps(top), final_state, p.n[top], K, HMM_G, 1, last(top));
    HAR_CHECK_LAUNCH();
    for (int l = top - 1; l >= 0; --l) {
      hmm_map_expand_kernel<<<blocks(p.n[l + 1]), HMM_BLOCK, 0, s>>>(maps(l), last(l + 1), p.n[l], K, HMM_G, p.n[l + 1], last(l));
      HAR_CHECK_LAUNCH();
    }
  }
  if (on(5)) {
    hmm_backtrace_kernel<<<blocks(C), HMM_BLOCK, 0, s>>>(psi, last(0), T, K, L, C, path);
    HAR_CHECK_LAUNCH();
  }
  if (on(6)) {
    hmm_score_kernel<<<blocks(S), HMM_BLOCK, 0, s>>>(endmax, S, score);
    HAR_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int har_hmm_chunk_len() { return HMM_L; }
extern "C" int har_hmm_scan_group() { return HMM_G; }

extern "C" int64_t har_hmm_workspace_bytes(int64_t T, int K, int64_t S, int L) {
  const HmmPlan p = hmm_plan(T, K, S, L);
  return p.ok ? (int64_t)p.bytes : -1;
}

extern "C" int har_hmm_viterbi(const int32_t* E, const int32_t* A, const int32_t* pi, const int64_t* seq_offsets, int64_t T,
                               int K, int64_t S, int L, void* ws, int64_t ws_bytes, int32_t* path, int64_t* score,
                               int phase_lo, int phase_hi, hipStream_t s) {
  if (T == 0) return 0;
  const HmmPlan p = hmm_plan(T, K, S, L);
  if (!p.ok || ws_bytes < (int64_t)p.bytes) return -2;
  if (E == nullptr || A == nullptr || pi == nullptr || seq_offsets == nullptr || ws == nullptr || path == nullptr ||
      score == nullptr)
    return -4;
  uint8_t* w = static_cast<uint8_t*>(ws);
  switch (hmm_kp(K)) {
    case 2: return hmm_run<2>(p, E, A, pi, seq_offsets, T, K, S, L, w, path, score, phase_lo, phase_hi, s);
    case 4: return hmm_run<4>(p, E, A, pi, seq_offsets, T, K, S, L, w, path, score, phase_lo, phase_hi, s);
    case 8: return hmm_run<8>(p, E, A, pi, seq_offsets, T, K, S, L, w, path, score, phase_lo, phase_hi, s);
    case 16: return hmm_run<16>(p, E, A, pi, seq_offsets, T, K, S, L, w, path, score, phase_lo, phase_hi, s);
    default: return hmm_run<32>(p, E, A, pi, seq_offsets, T, K, S, L, w, path, score, phase_lo, phase_hi, s);
  }
}
