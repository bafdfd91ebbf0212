// Parallel forward-backward over a concatenated batch of sequences (har/ops/hmm.py holds the definition):
// per-step state posteriors gamma, per-sequence log-likelihoods and the summed pairwise posteriors xi that
// Baum-Welch needs.  The structure is hmm.hip's — ONE scan over T steps in chunks of L, grouped scans over the
// chunk products — with the semiring changed from (max, +) over integers to (+, x) over positive fp64 values.
//
// The step matrix is M_t(i, j) = P(i, j) B_t(j), or the rank-one reset p0(j) B_t(j) (every i) where a sequence
// starts.  A reset forgets the direction of the incoming vector and keeps its mass, so the running forward
// vector carries the product of the likelihoods of all sequences so far and a sequence's likelihood is the ratio
// of consecutive end masses; seen from the left a reset makes beta constant over i, so a sequence end needs no
// special case either.
//
//   0. flags            hmm_flags_kernel (hmm_common.h)
//   1. chunk products   the scaled product of each chunk's L step matrices
//                         K <= 8: one lane per matrix row, P in registers
//                         K  > 8: one lane per (i, j) through double-buffered LDS, or v_mfma_f64_16x16x4_f64
//   2. prefix scan      group products up, then the forward vector entering every chunk (entries, exponent)
//   3. suffix scan      the same group products, then the backward vector leaving every chunk
//   4. chunk pass       each chunk again from its true incoming vector: alpha_t kept in LDS, backward from the
//                       chunk's beta, gamma written from LDS with 16-byte stores, the chunk's xi partial, the
//                       cumulative mass at every sequence end; no [T][K] intermediate goes to global memory
//   5. reductions       loglik[s] = log(m_s / m_{s-1}) + (e_s - e_{s-1}) ln 2; xi = a strided sum then a tree
//
// Scaling.  Nothing takes a logarithm or an exponential of a per-step quantity.  Every running matrix or vector
// is kept with its largest entry in [1, 2) plus an integer binary exponent (int64): the rescale multiplies by a
// power of two, which is exact and adds no rounding.  Precondition (the caller's contract, ops/hmm.py builds its
// inputs so): B in [2^-93, 1] with a 1 in every row, P and p0 in [2^-52, 1].  Then, in any partial product R of
// step matrices, two entries of one row differ by a factor >= 2^-145 (the last factor's columns: a ratio of two
// P-weighted sums of the same positive numbers, >= 2^-52, times a ratio of two B entries, >= 2^-93), and two
// entries of one column by >= 2^-52 (the first factor's rows, the same argument with P alone; a reset's rows are
// equal).  So every entry of R lies within 2^-197 of the largest, every scaled entry in [2^-197, 2), and no
// product of two entries (>= 2^-394), nor the four-factor xi term alpha P B beta (>= 2^-342), underflows.  The
// (i, j)-lane kernel applies a step's scale one step late (its running maximum then lies in [2^-52, 64)), which
// the same bounds cover.
//
// No atomics, no device -> host read; every output element has exactly one writer and every reduction a fixed
// order, so two runs are bitwise equal.
#include "hmm_common.h"
#include "../har_kernels.h"

#include <cstdint>

namespace {

constexpr int FB_LDS_BYTES = 64 * 1024;  // phase 4: the alpha rows of a workgroup's chunks
// phase 1 at K > 8: 1 = (i, j) lanes, 2 = MFMA.  Measured on the MI355X at K = 32, 1,000,000 steps: 8.89 ms
// against 1.42 ms (profiles/r12/hmm_fb_probe.txt), so the matrix cores are the default.
constexpr int FB_WIDE_DEFAULT = 2;

typedef double double4_t __attribute__((ext_vector_type(4)));

// the binary exponent of a positive normal double, and 2^e for e in [-1022, 1023]
__device__ __forceinline__ int exp_of(double m) { return (int)((__double_as_longlong(m) >> 52) & 0x7ff) - 1023; }
__device__ __forceinline__ double pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }

template <int W>
__device__ __forceinline__ double gmax(double v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, W));
  return v;
}
// butterfly sum: addition commutes, so every lane of the group ends with the same bits
template <int W>
__device__ __forceinline__ double gsum(double v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}

// Phase 1, K <= 8.  KP lanes per chunk, lane i holds row i of the running product; P sits in LDS at stride KP so
// every index is an immediate (the compiler keeps it in registers across the step loop).  Lanes i >= K stay for
// the group reductions and hold zeros.
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void fb_chunk_mat_kernel(const double* __restrict__ B, const double* __restrict__ P,
                                                                 const double* __restrict__ p0,
                                                                 const uint8_t* __restrict__ flags, int64_t T, int K, int L,
                                                                 int64_t C, double* __restrict__ mats, int64_t* __restrict__ mexp) {
  __shared__ double sP[KP * KP];
  __shared__ double sP0[KP];
  for (int x = threadIdx.x; x < KP * KP; x += HMM_BLOCK) {
    const int r = x / KP, q = x % KP;
    sP[x] = (r < K && q < K) ? P[r * K + q] : 0.0;
  }
  if (threadIdx.x < KP) sP0[threadIdx.x] = threadIdx.x < K ? p0[threadIdx.x] : 0.0;
  __syncthreads();
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  const int64_t c = gid / KP;
  const int i = (int)(gid % KP);
  if (c >= C) return;  // whole groups leave
  const bool ok = i < K;
  const int64_t t0 = c * L, t1 = min64(T, t0 + L);
  double R[KP];
  int64_t ex = 0;
  for (int64_t t = t0; t < t1; ++t) {
    const double* b = B + t * K;
    const bool start = flags[t] & FLAG_START;
    double N[KP];
    if (t == t0) {
#pragma unroll
      for (int j = 0; j < KP; ++j) N[j] = (ok && j < K) ? (start ? sP0[j] : sP[i * KP + j]) * b[j] : 0.0;
    } else if (start) {
      double s = R[0];
#pragma unroll
      for (int k = 1; k < KP; ++k) s += R[k];
#pragma unroll
      for (int j = 0; j < KP; ++j) N[j] = j < K ? s * sP0[j] * b[j] : 0.0;
    } else {
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        double v = R[0] * sP[j];
#pragma unroll
        for (int k = 1; k < KP; ++k) v += R[k] * sP[k * KP + j];
        N[j] = j < K ? v * b[j] : 0.0;
      }
    }
    double m = N[0];
#pragma unroll
    for (int j = 1; j < KP; ++j) m = fmax(m, N[j]);
    const int e = exp_of(gmax<KP>(m));
    const double sc = pow2(-e);
    ex += e;
#pragma unroll
    for (int j = 0; j < KP; ++j) R[j] = N[j] * sc;
  }
  if (ok) {
    double* o = mats + (c * K + i) * K;
#pragma unroll
    for (int j = 0; j < KP; ++j)
      if (j < K) o[j] = R[j];
  }
  if (i == 0) mexp[c] = ex;
}

// Phase 1, K > 8, lanes.  One workgroup of KP^2 lanes per chunk, lane (i, j) holds R(i, j) and column j of P; row i
// of the running product goes through LDS (double buffered: one barrier per step).  Each wave leaves the maximum
// of its entries beside the buffer, so the step that reads a buffer also knows its scale.
template <int KP>
__global__ __launch_bounds__(KP * KP) void fb_chunk_mat_wide_kernel(const double* __restrict__ B, const double* __restrict__ P,
                                                                    const double* __restrict__ p0,
                                                                    const uint8_t* __restrict__ flags, int64_t T, int K,
                                                                    int L, int64_t C, double* __restrict__ mats,
                                                                    int64_t* __restrict__ mexp) {
  constexpr int NW = KP * KP / 64;
  __shared__ double sR[2][KP * KP];
  __shared__ double sMax[2][NW];
  const int tid = threadIdx.x, i = tid / KP, j = tid % KP;
  const int64_t c = blockIdx.x;
  if (c >= C) return;  // (block-uniform)
  const bool ok = i < K && j < K;
  double a[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) a[k] = (k < K && j < K) ? P[k * K + j] : 0.0;
  const double pj = j < K ? p0[j] : 0.0;
  const int64_t t0 = c * L, t1 = min64(T, t0 + L);
  double p = 0.0;
  if (ok) p = ((flags[t0] & FLAG_START) ? pj : P[i * K + j]) * B[t0 * K + j];
  int64_t ex = 0;
  int buf = 0;
  for (int64_t t = t0 + 1; t <= t1; ++t) {  // the pass t = t1 only scales the last product
    sR[buf][tid] = p;
    const double wm = gmax<64>(p);
    if ((tid & 63) == 0) sMax[buf][tid >> 6] = wm;
    __syncthreads();
    double m = sMax[buf][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmax(m, sMax[buf][w]);
    const int e = exp_of(m);
    const double sc = pow2(-e);
    ex += e;
    if (t == t1) {
      p *= sc;
      break;
    }
    const double* row = &sR[buf][i * KP];
    const double bt = ok ? B[t * K + j] : 0.0;
    double v;
    if (flags[t] & FLAG_START) {  // block-uniform
      v = row[0];
#pragma unroll
      for (int k = 1; k < KP; ++k) v += row[k];
      v *= pj;
    } else {
      v = row[0] * a[0];
#pragma unroll
      for (int k = 1; k < KP; ++k) v += row[k] * a[k];
    }
    p = ok ? v * bt * sc : 0.0;
    buf ^= 1;
  }
  if (ok) mats[(c * K + i) * K + j] = p;
  if (tid == 0) mexp[c] = ex;
}

// Phase 1, K > 8, matrix cores.  One wave per chunk keeps X = R^T in v_mfma_f64_16x16x4_f64's C/D layout
// (col = lane & 15, row = (lane >> 4) + 4 reg): register r of tile (jt, ct) holds rows 16 jt + 4 r .. + 3, which is
// exactly the B operand (k = lane >> 4, col = lane & 15) of k-block 4 jt + r.  So X' = M_t^T X needs no lane
// movement and no LDS: the A operand is P^T (or p0 broadcast over k for a reset), held in registers for the whole
// chunk, and B_t scales the result's rows.  K is padded to KP = 16 or 32 with zeros.
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void fb_chunk_mat_mfma_kernel(const double* __restrict__ B, const double* __restrict__ P,
                                                                      const double* __restrict__ p0,
                                                                      const uint8_t* __restrict__ flags, int64_t T, int K,
                                                                      int L, int64_t C, double* __restrict__ mats,
                                                                      int64_t* __restrict__ mexp) {
  constexpr int NT = KP / 16, NK = KP / 4;
  const int lane = threadIdx.x & 63, lo = lane & 15, hi = lane >> 4;
  const int64_t c = (int64_t)blockIdx.x * (HMM_BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= C) return;  // whole waves leave
  double pa[NT][NK], pa0[NT];
#pragma unroll
  for (int jt = 0; jt < NT; ++jt) {
    const int j = 16 * jt + lo;
    pa0[jt] = j < K ? p0[j] : 0.0;
#pragma unroll
    for (int kb = 0; kb < NK; ++kb) {
      const int i = 4 * kb + hi;
      pa[jt][kb] = (i < K && j < K) ? P[i * K + j] : 0.0;
    }
  }
  const int64_t t0 = c * L, t1 = min64(T, t0 + L);
  double4_t X[NT][NT];
  int64_t ex = 0;
  for (int64_t t = t0; t < t1; ++t) {
    const bool start = flags[t] & FLAG_START;  // wave-uniform
    double4_t N[NT][NT];
    if (t == t0) {
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = 16 * jt + hi + 4 * r, i = 16 * ct + lo;
            N[jt][ct][r] = (i < K && j < K) ? (start ? p0[j] : P[i * K + j]) : 0.0;
          }
    } else {
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int kb = 0; kb < NK; ++kb)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(start ? pa0[jt] : pa[jt][kb], X[kb / 4][ct][kb % 4], acc, 0, 0, 0);
          N[jt][ct] = acc;
        }
    }
    double m = 0.0;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * jt + hi + 4 * r;
        const double bt = j < K ? B[t * K + j] : 0.0;
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          N[jt][ct][r] *= bt;
          m = fmax(m, N[jt][ct][r]);
        }
      }
    const int e = exp_of(gmax<64>(m));
    const double sc = pow2(-e);
    ex += e;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) X[jt][ct] = N[jt][ct] * sc;
  }
#pragma unroll
  for (int jt = 0; jt < NT; ++jt)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * jt + hi + 4 * r, i = 16 * ct + lo;
        if (i < K && j < K) mats[(c * K + i) * K + j] = X[jt][ct][r];
      }
  if (lane == 0) mexp[c] = ex;
}

// Phases 2 and 3, up: out[g] = in[g G] in[g G + 1] ... (scaled), lane i holds row i.
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void fb_mat_reduce_kernel(const double* __restrict__ in, const int64_t* __restrict__ inexp,
                                                                  int64_t n, int K, int G, int64_t ng, double* __restrict__ out,
                                                                  int64_t* __restrict__ outexp) {
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  const int64_t g = gid / KP;
  const int i = (int)(gid % KP);
  if (g >= ng) return;  // whole groups leave
  const bool ok = i < K;
  const int64_t c0 = g * G, c1 = min64(n, c0 + G);
  double R[KP];
  {
    const double* m = in + (c0 * K + i) * K;
#pragma unroll
    for (int j = 0; j < KP; ++j) R[j] = (ok && j < K) ? m[j] : 0.0;
  }
  int64_t ex = inexp[c0];
  for (int64_t c = c0 + 1; c < c1; ++c) {
    const double* m = in + c * K * K;
    double N[KP];
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      double v = 0.0;
      if (j < K) {
        v = R[0] * m[j];
#pragma unroll
        for (int k = 1; k < KP; ++k)
          if (k < K) v += R[k] * m[k * K + j];
      }
      N[j] = v;
      mx = fmax(mx, v);
    }
    const int e = exp_of(gmax<KP>(mx));
    const double sc = pow2(-e);
    ex += inexp[c] + e;
#pragma unroll
    for (int j = 0; j < KP; ++j) R[j] = N[j] * sc;
  }
  if (ok) {
    double* o = out + (g * K + i) * K;
#pragma unroll
    for (int j = 0; j < KP; ++j)
      if (j < K) o[j] = R[j];
  }
  if (i == 0) outexp[g] = ex;
}

// Phase 2, down: vout[c] = the forward (row) vector entering matrix c, from the vector entering its group
// (null = the unit vector e_0 with exponent 0: step 0 is a reset, which keeps only the mass 1).  KP lanes per
// group, lane j holds v(j).
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void fb_prefix_kernel(const double* __restrict__ mats, const int64_t* __restrict__ mexp,
                                                              const double* __restrict__ vin, const int64_t* __restrict__ vinexp,
                                                              int64_t n, int K, int G, int64_t ng, double* __restrict__ vout,
                                                              int64_t* __restrict__ voutexp) {
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  const int64_t g = gid / KP;
  const int j = (int)(gid % KP);
  if (g >= ng) return;  // whole groups leave: the shuffles below stay inside a group
  const bool ok = j < K;
  const int64_t c0 = g * G, c1 = min64(n, c0 + G);
  double v = vin != nullptr ? (ok ? vin[g * K + j] : 0.0) : (j == 0 ? 1.0 : 0.0);
  int64_t ex = vin != nullptr ? vinexp[g] : 0;
  for (int64_t c = c0; c < c1; ++c) {
    if (ok) vout[c * K + j] = v;
    if (j == 0) voutexp[c] = ex;
    if (c + 1 == c1) break;
    const double* m = mats + c * K * K;
    double nv = 0.0;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      if (i < K) {
        const double vi = __shfl(v, i, KP);
        if (ok) nv += vi * m[i * K + j];
      }
    }
    const int e = exp_of(gmax<KP>(nv));
    v = nv * pow2(-e);
    ex += mexp[c] + e;
  }
}

// Phase 3, down: bout[c] = the backward (column) vector leaving matrix c, from the vector leaving its group
// (null = ones: nothing follows the last step).  Lane i holds b(i); the exponent of a beta is never needed.
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void fb_suffix_kernel(const double* __restrict__ mats, const double* __restrict__ vin,
                                                              int64_t n, int K, int G, int64_t ng, double* __restrict__ bout) {
  const int64_t gid = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  const int64_t g = gid / KP;
  const int i = (int)(gid % KP);
  if (g >= ng) return;  // whole groups leave
  const bool ok = i < K;
  const int64_t c0 = g * G, c1 = min64(n, c0 + G);
  double b = ok ? (vin != nullptr ? vin[g * K + i] : 1.0) : 0.0;
  for (int64_t c = c1 - 1; c >= c0; --c) {
    if (ok) bout[c * K + i] = b;
    if (c == c0) break;
    const double* m = mats + (c * K + i) * K;
    double nb = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (k < K) {
        const double bk = __shfl(b, k, KP);
        if (ok) nb += m[k] * bk;
      }
    }
    b = nb * pow2(-exp_of(gmax<KP>(nb)));
  }
}

// Phase 4.  KP lanes per chunk, cpb chunks per workgroup; lane j holds alpha(j) / beta(j), column j of P (forward,
// xi) and row j of P (backward).  The chunk's scaled alpha rows live in LDS at stride K (a lane reads back only
// what it wrote), become gamma in place during the backward sweep and leave as one contiguous copy.
template <int KP>
__global__ __launch_bounds__(HMM_BLOCK) void fb_chunk_pass_kernel(
    const double* __restrict__ B, const double* __restrict__ P, const double* __restrict__ p0, const uint8_t* __restrict__ flags,
    const double* __restrict__ vin, const int64_t* __restrict__ vinexp, const double* __restrict__ bin,
    const int32_t* __restrict__ first_end, int64_t T, int64_t S, int K, int L, int64_t C, int cpb, double* __restrict__ gamma,
    double* __restrict__ endm, int64_t* __restrict__ ende, double* __restrict__ xipart) {
  extern __shared__ double fb_lds[];
  const int grp = threadIdx.x / KP, j = threadIdx.x % KP;
  const int64_t c = (int64_t)blockIdx.x * cpb + grp;
  if (c >= C) return;  // whole groups leave
  const bool ok = j < K;
  double* al = fb_lds + (size_t)grp * L * K;
  double col[KP], row[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    col[i] = (ok && i < K) ? P[i * K + j] : 0.0;
    row[i] = (ok && i < K) ? P[j * K + i] : 0.0;
  }
  const double pj = ok ? p0[j] : 0.0;
  const int64_t t0 = c * L, t1 = min64(T, t0 + L);
  const double ain = ok ? vin[c * K + j] : 0.0;
  double a = ain;
  int64_t ex = vinexp[c];
  int64_t sidx = first_end[c];
  for (int64_t t = t0; t < t1; ++t) {
    const int f = flags[t];
    const double bt = ok ? B[t * K + j] : 0.0;
    double v = 0.0;
    if (f & FLAG_START) {  // uniform inside the group
#pragma unroll
      for (int i = 0; i < KP; ++i)
        if (i < K) v += __shfl(a, i, KP);
      v *= pj;
    } else {
#pragma unroll
      for (int i = 0; i < KP; ++i)
        if (i < K) v += __shfl(a, i, KP) * col[i];
    }
    v *= bt;
    const int e = exp_of(gmax<KP>(v));
    a = v * pow2(-e);
    ex += e;
    if (ok) al[(t - t0) * K + j] = a;
    if (f & FLAG_END) {
      const double mass = gsum<KP>(a);
      if (j == 0 && sidx < S) {
        endm[sidx] = mass;
        ende[sidx] = ex;
      }
      ++sidx;
    }
  }
  double b = ok ? bin[c * K + j] : 0.0;
  double xa[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) xa[i] = 0.0;
  for (int64_t t = t1 - 1; t >= t0; --t) {
    const bool start = flags[t] & FLAG_START;
    const double at = ok ? al[(t - t0) * K + j] : 0.0;
    const double gm = at * b;
    const double tot = gsum<KP>(gm);
    if (ok) al[(t - t0) * K + j] = gm / tot;
    const double w = (ok ? B[t * K + j] : 0.0) * b;
    if (xipart != nullptr && !start) {
      const double ap = t > t0 ? (ok ? al[(t - 1 - t0) * K + j] : 0.0) : ain;
      double u[KP];
      double cs = 0.0;
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        u[i] = i < K ? __shfl(ap, i, KP) * col[i] : 0.0;
        cs += u[i];
      }
      const double r = w / gsum<KP>(cs * w);
#pragma unroll
      for (int i = 0; i < KP; ++i) xa[i] += u[i] * r;
    }
    if (t == t0) break;
    double nb = 0.0;
    if (start) {
      const double cst = gsum<KP>(pj * w);  // the same for every i
      nb = ok ? cst : 0.0;
    } else {
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) nb += row[k] * __shfl(w, k, KP);
    }
    b = nb * pow2(-exp_of(gmax<KP>(nb)));
  }
  if (xipart != nullptr && ok) {
    double* o = xipart + c * K * K + j;
#pragma unroll
    for (int i = 0; i < KP; ++i)
      if (i < K) o[i * K] = xa[i];
  }
  // the group's lanes run in one wave: order its LDS writes before the other lanes' reads
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int n = (int)(t1 - t0) * K;
  double* dst = gamma + t0 * K;
  const int head = (reinterpret_cast<uintptr_t>(dst) & 15) ? 1 : 0;  // n >= 1
  if (head && j == 0) dst[0] = al[0];
  const int npair = (n - head) / 2;
  for (int q = j; q < npair; q += KP) {
    const double2 v = make_double2(al[head + 2 * q], al[head + 2 * q + 1]);
    *reinterpret_cast<double2*>(dst + head + 2 * q) = v;
  }
  if (((n - head) & 1) && j == 0) dst[n - 1] = al[n - 1];
}

// Phase 5.
__global__ __launch_bounds__(HMM_BLOCK) void fb_loglik_kernel(const double* __restrict__ endm, const int64_t* __restrict__ ende,
                                                              int64_t S, double* __restrict__ loglik) {
  const int64_t s = (int64_t)blockIdx.x * HMM_BLOCK + threadIdx.x;
  if (s >= S) return;
  const double m0 = s > 0 ? endm[s - 1] : 1.0;
  const int64_t e0 = s > 0 ? ende[s - 1] : 0;
  loglik[s] = log(endm[s] / m0) + (double)(ende[s] - e0) * 0.69314718055994530942;
}

// One workgroup per entry of xi: a strided sum over the chunks' partials, then a tree (both in a fixed order).
__global__ __launch_bounds__(HMM_BLOCK) void fb_xi_reduce_kernel(const double* __restrict__ xipart, int64_t C, int KK,
                                                                 double* __restrict__ xi) {
  __shared__ double sh[HMM_BLOCK];
  const int x = blockIdx.x;
  double s = 0.0;
  for (int64_t c = threadIdx.x; c < C; c += HMM_BLOCK) s += xipart[c * KK + x];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = HMM_BLOCK / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) xi[x] = sh[0];
}

// The workspace: every buffer of a run, 256-byte aligned.
struct FbPlan {
  static constexpr int MAXLV = HmmLevels::MAXLV;
  HmmLevels lv;
  int cpb = 0;  // phase 4: chunks per workgroup
  size_t flags = 0, first_end = 0, endm = 0, ende = 0, xipart = 0;
  size_t mats[MAXLV] = {}, mexp[MAXLV] = {}, fvec[MAXLV] = {}, fexp[MAXLV] = {}, bvec[MAXLV] = {};
  size_t bytes = 0;
  bool ok = false;
};

FbPlan fb_plan(int64_t T, int K, int64_t S, int L, bool want_xi) {
  FbPlan p;
  p.lv = hmm_levels(T, K, S, L);
  if (!p.lv.ok) return p;
  const int64_t chunk_bytes = (int64_t)L * K * (int64_t)sizeof(double);
  if (chunk_bytes > FB_LDS_BYTES) return p;  // a chunk's alpha rows must fit the workgroup's LDS
  const int kp = hmm_kp(K);
  p.cpb = (int)(FB_LDS_BYTES / chunk_bytes);
  if (p.cpb > HMM_BLOCK / kp) p.cpb = HMM_BLOCK / kp;
  size_t o = 0;
  auto take = [&o](size_t b) {
    const size_t at = o;
    o += align256(b);
    return at;
  };
  const int64_t C = p.lv.C;
  p.flags = take((size_t)T);
  p.first_end = take((size_t)C * sizeof(int32_t));
  p.endm = take((size_t)S * sizeof(double));
  p.ende = take((size_t)S * sizeof(int64_t));
  p.xipart = take(want_xi ? (size_t)C * K * K * sizeof(double) : 0);
  for (int l = 0; l < p.lv.nlv; ++l) {
    const size_t n = (size_t)p.lv.n[l];
    p.mats[l] = take(n * K * K * sizeof(double));
    p.mexp[l] = take(n * sizeof(int64_t));
    p.fvec[l] = take(n * K * sizeof(double));
    p.fexp[l] = take(n * sizeof(int64_t));
    p.bvec[l] = take(n * K * sizeof(double));
  }
  p.bytes = o;
  p.ok = true;
  return p;
}

template <int KP>
int fb_run(const FbPlan& p, const double* B, const double* P, const double* p0, const int64_t* off, int64_t T, int K, int64_t S,
           int L, uint8_t* ws, double* gamma, double* loglik, double* xi, int lo, int hi, int variant, hipStream_t s) {
  uint8_t* flags = ws + p.flags;
  int32_t* first_end = reinterpret_cast<int32_t*>(ws + p.first_end);
  double* endm = reinterpret_cast<double*>(ws + p.endm);
  int64_t* ende = reinterpret_cast<int64_t*>(ws + p.ende);
  double* xipart = xi != nullptr ? reinterpret_cast<double*>(ws + p.xipart) : nullptr;
  auto mats = [&](int l) { return reinterpret_cast<double*>(ws + p.mats[l]); };
  auto mexp = [&](int l) { return reinterpret_cast<int64_t*>(ws + p.mexp[l]); };
  auto fvec = [&](int l) { return reinterpret_cast<double*>(ws + p.fvec[l]); };
  auto fexp = [&](int l) { return reinterpret_cast<int64_t*>(ws + p.fexp[l]); };
  auto bvec = [&](int l) { return reinterpret_cast<double*>(ws + p.bvec[l]); };
  const int64_t* n = p.lv.n;
  const int top = p.lv.nlv - 1;
  const int64_t C = p.lv.C;
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
    if constexpr (KP <= 8) {
      fb_chunk_mat_kernel<KP><<<blocks(C * KP), HMM_BLOCK, 0, s>>>(B, P, p0, flags, T, K, L, C, mats(0), mexp(0));
    } else {
      if ((variant == 0 ? FB_WIDE_DEFAULT : variant) == 2)
        fb_chunk_mat_mfma_kernel<KP><<<blocks(C * 64), HMM_BLOCK, 0, s>>>(B, P, p0, flags, T, K, L, C, mats(0), mexp(0));
      else
        fb_chunk_mat_wide_kernel<KP><<<(unsigned)C, KP * KP, 0, s>>>(B, P, p0, flags, T, K, L, C, mats(0), mexp(0));
    }
    HAR_CHECK_LAUNCH();
  }
  if (on(2)) {
    for (int l = 0; l < top; ++l) {
      fb_mat_reduce_kernel<KP><<<blocks(n[l + 1] * KP), HMM_BLOCK, 0, s>>>(mats(l), mexp(l), n[l], K, HMM_G, n[l + 1], mats(l + 1),
                                                                          mexp(l + 1));
      HAR_CHECK_LAUNCH();
    }
    // the top level is one group of n[top] <= G matrices
    fb_prefix_kernel<KP><<<blocks(KP), HMM_BLOCK, 0, s>>>(mats(top), mexp(top), nullptr, nullptr, n[top], K, HMM_G, 1, fvec(top),
                                                          fexp(top));
    HAR_CHECK_LAUNCH();
    for (int l = top - 1; l >= 0; --l) {
      fb_prefix_kernel<KP><<<blocks(n[l + 1] * KP), HMM_BLOCK, 0, s>>>(mats(l), mexp(l), fvec(l + 1), fexp(l + 1), n[l], K, HMM_G,
                                                                      n[l + 1], fvec(l), fexp(l));
      HAR_CHECK_LAUNCH();
    }
  }
  if (on(3)) {
    fb_suffix_kernel<KP><<<blocks(KP), HMM_BLOCK, 0, s>>>(mats(top), nullptr, n[top], K, HMM_G, 1, bvec(top));
    HAR_CHECK_LAUNCH();
    for (int l = top - 1; l >= 0; --l) {
      fb_suffix_kernel<KP><<<blocks(n[l + 1] * KP), HMM_BLOCK, 0, s>>>(mats(l), bvec(l + 1), n[l], K, HMM_G, n[l + 1], bvec(l));
      HAR_CHECK_LAUNCH();
    }
  }
  if (on(4)) {
    const unsigned grid = (unsigned)((C + p.cpb - 1) / p.cpb);
    const size_t lds = (size_t)p.cpb * L * K * sizeof(double);
    fb_chunk_pass_kernel<KP><<<grid, p.cpb * KP, lds, s>>>(B, P, p0, flags, fvec(0), fexp(0), bvec(0), first_end, T, S, K, L, C,
                                                          p.cpb, gamma, endm, ende, xipart);
    HAR_CHECK_LAUNCH();
  }
  if (on(5)) {
    fb_loglik_kernel<<<blocks(S), HMM_BLOCK, 0, s>>>(endm, ende, S, loglik);
    HAR_CHECK_LAUNCH();
    if (xi != nullptr) {
      fb_xi_reduce_kernel<<<K * K, HMM_BLOCK, 0, s>>>(xipart, C, K * K, xi);
      HAR_CHECK_LAUNCH();
    }
  }
  return 0;
}

}  // namespace

extern "C" int64_t har_hmm_fb_workspace_bytes(int64_t T, int K, int64_t S, int L, int want_xi) {
  const FbPlan p = fb_plan(T, K, S, L, want_xi != 0);
  return p.ok ? (int64_t)p.bytes : -1;
}

extern "C" int har_hmm_forward_backward(const double* B, const double* P, const double* p0, const int64_t* seq_offsets, int64_t T,
                                        int K, int64_t S, int L, void* ws, int64_t ws_bytes, double* gamma, double* loglik,
                                        double* xi, int phase_lo, int phase_hi, int variant, hipStream_t s) {
  if (T == 0) return 0;
  const FbPlan p = fb_plan(T, K, S, L, xi != nullptr);
  if (!p.ok || ws_bytes < (int64_t)p.bytes || variant < 0 || variant > 2) return -2;
  if (B == nullptr || P == nullptr || p0 == nullptr || seq_offsets == nullptr || ws == nullptr || gamma == nullptr ||
      loglik == nullptr)
    return -4;
  uint8_t* w = static_cast<uint8_t*>(ws);
  switch (hmm_kp(K)) {
    case 2: return fb_run<2>(p, B, P, p0, seq_offsets, T, K, S, L, w, gamma, loglik, xi, phase_lo, phase_hi, variant, s);
    case 4: return fb_run<4>(p, B, P, p0, seq_offsets, T, K, S, L, w, gamma, loglik, xi, phase_lo, phase_hi, variant, s);
    case 8: return fb_run<8>(p, B, P, p0, seq_offsets, T, K, S, L, w, gamma, loglik, xi, phase_lo, phase_hi, variant, s);
    case 16: return fb_run<16>(p, B, P, p0, seq_offsets, T, K, S, L, w, gamma, loglik, xi, phase_lo, phase_hi, variant, s);
    default: return fb_run<32>(p, B, P, p0, seq_offsets, T, K, S, L, w, gamma, loglik, xi, phase_lo, phase_hi, variant, s);
  }
}
