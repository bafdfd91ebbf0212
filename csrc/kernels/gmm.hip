// Gaussian mixtures (full-covariance EM): the fused E-step + moments kernel on the exact-fp32 matrix
// cores, a per-component finish kernel (fp64 Cholesky and triangular inverse in LDS) and a one-workgroup
// control kernel that keeps the whole fit on the device.
//
// Definitions (har/ops/gmm.py states them once more as PyTorch code; the kernels compare to it):
//   * working rows Z [N][D] fp32 (standardised by the caller); component k has mu_k [D], the upper
//     triangular W_k = L_k^{-T} [D][D] (Sigma_k = L_k L_k^T) and c_k = log pi_k - D/2 log 2pi - sum log L_ii.
//   * d = z - mu_k (one fp32 subtract), y = d W_k, q[n][k] = sum_j y_j^2, t = c_k - q / 2,
//     m = max_k t, e_k = exp(t_k - m), s = sum_k e_k, lse = m + log s, r_k = e_k / s,
//     pred = the first argmax of r.
//   * moments about the OLD mean with wr = w[n] r[n][k]: N_k = sum wr, S1_k = sum wr d, S2_k = sum wr d d^T.
//   * loglik partial of a workgroup = sum of w lse over its rows in a fixed order (fp64).
//
// gmm_estep.  A persistent grid: workgroup b of G takes the 64-row tiles b, b + G, ...  Four waves, 16
// rows each.  Per tile the rows are staged once (row stride D16 + 2 floats: the 32 lanes of an A read
// hit 32 banks, as in kmeans.hip).  Sweep 1 visits the components in order: W_k (entries below the
// diagonal staged as zeros, row stride = 16 mod 64 floats so the four k-phases of a B read take four
// bank groups) and mu_k go through LDS, the A element is z - mu, v_mfma_f32_16x16x4_f32 runs against the
// column tiles at or right of the diagonal block, and the squares are row-summed on the C layout (col =
// lane & 15 = j, row = 4 (lane >> 4) + reg) with one 16-lane DPP reduction per row.  The softmax epilogue
// takes four lanes per row.  Sweep 2 forms (wr o d)^T d per component on the matrix cores, upper
// triangle tiles only, into accumulators the workgroup KEEPS IN LDS across its tiles (per component
// N_k | S1 [Dp] | one 16 x 16 C image per tile pair; a lane reads and writes only its own words, so there
// are no atomics and the result does not depend on timing).  The slab [K][1 + Dp + Dp Dp] is stored ONCE,
// after the workgroup's last tile.  When the accumulators of all K components do not fit beside the
// staging buffers (large K D^2), the components are taken in groups of `grp`: the workgroup passes over
// its tiles once per group.  The first pass runs sweep 1 and the epilogue, writes the outputs and keeps
// w r in a scratch [N][K] in global memory; the later passes stage the rows again and read their
// components' w r back (written by this same workgroup), so no product is repeated.  gmm_finish sums
// the slabs in order in fp64.
#include <math.h>

#include "common.h"
#include "wave_ops.h"
#include "../har_kernels.h"

namespace {

constexpr int GM_ROWS = 64;  // rows per tile
constexpr int GM_THREADS = 256;
constexpr int GM_MAXK = 64, GM_MAXD = 128;
constexpr int GM_MAX_BLOCKS = 512;                    // persistent grid
constexpr int64_t GM_SLAB_BYTES = (int64_t)256 << 20;  // all slabs of a launch stay below this
constexpr int GM_TMAX = GM_MAXD / 16;
constexpr int64_t GM_LDS_MAX = 160 * 1024;

struct GmPlan {
  int Dp, D16, T, ldz, ldw, ldt, npairs, slab, accsz, grp;
  int64_t bytes;
};

bool gm_plan(int D, int K, bool want_mom, GmPlan& p) {
  if (D < 1 || D > GM_MAXD || K < 1 || K > GM_MAXK) return false;
  p.Dp = (D + 3) & ~3;
  p.D16 = (D + 15) & ~15;
  p.T = p.D16 >> 4;
  p.ldz = p.D16 + 2;
  p.ldw = ((p.D16 - 16 + 63) / 64) * 64 + 16;  // the smallest >= D16 that is 16 mod 64
  p.ldt = K + 1;
  p.npairs = p.T * (p.T + 1) / 2;
  p.slab = 1 + p.Dp + p.Dp * p.Dp;
  // [red double 64][zt 64 ldz][ws Dp ldw][mus D16][tl 64 ldt][wl 64]
  p.bytes = 64 * 8 + 4 * ((int64_t)GM_ROWS * p.ldz + (int64_t)p.Dp * p.ldw + p.D16 + (int64_t)GM_ROWS * p.ldt + GM_ROWS);
  // + [acc grp accsz]: the moment accumulators of a group of components
  p.accsz = 1 + p.Dp + p.npairs * 256;
  p.grp = K;
  if (want_mom) {
    const int64_t fit = (GM_LDS_MAX - p.bytes) / ((int64_t)p.accsz * 4);
    if (fit < 1) return false;
    p.grp = (int)(fit < K ? fit : K);
    p.bytes += (int64_t)p.grp * p.accsz * 4;
  }
  return true;
}

int gm_grid(int64_t N, const GmPlan& p, int K, int max_blocks) {
  const int64_t ntiles = (N + GM_ROWS - 1) / GM_ROWS;
  int64_t g = GM_SLAB_BYTES / ((int64_t)K * p.slab * 4);
  if (g > GM_MAX_BLOCKS) g = GM_MAX_BLOCKS;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  if (g > ntiles) g = ntiles;
  return g < 1 ? 1 : (int)g;
}

__global__ __launch_bounds__(GM_THREADS) void gmm_estep_kernel(GmmEstepArgs a, GmPlan p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gm_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  const int D = a.D, K = a.K, Dp = p.Dp, D16 = p.D16, T = p.T, ldz = p.ldz, ldw = p.ldw, ldt = p.ldt;
  double* const red = reinterpret_cast<double*>(gm_lds);
  float* const zt = reinterpret_cast<float*>(red + GM_ROWS);
  float* const ws = zt + GM_ROWS * ldz;
  float* const mus = ws + Dp * ldw;
  float* const tl = mus + D16;
  float* const wl = tl + GM_ROWS * ldt;
  float* const accl = wl + GM_ROWS;
  // a moments-only step of a fit that has converged (or used its iterations) has nothing to do
  if (a.state && !(a.state[1] == 0 && a.state[0] < a.max_iter)) return;  // (uniform)
  const int64_t ntiles = (a.N + GM_ROWS - 1) / GM_ROWS;
  float* const slab = a.slabs ? a.slabs + (int64_t)blockIdx.x * K * p.slab : nullptr;
  double part = 0.0;  // (thread 0)

  for (int g0 = 0; g0 < (slab ? K : 1); g0 += p.grp) {
  const bool pass0 = g0 == 0;  // the outputs are written on the first pass
  const int g1 = min(K, g0 + p.grp);
  if (slab)
    for (int j = tid; j < (g1 - g0) * p.accsz; j += GM_THREADS) accl[j] = 0.f;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * GM_ROWS;
    const int nrows = (int)min<int64_t>(GM_ROWS, a.N - row0);
    __syncthreads();  // the previous tile is consumed
    for (int r = wave; r < GM_ROWS; r += 4) {
      const bool ok = r < nrows;
      const float* src = a.Z + (row0 + r) * D;
      for (int f = lane; f < ldz; f += 64) zt[r * ldz + f] = ok && f < D ? src[f] : 0.f;
    }
    if (tid < GM_ROWS) wl[tid] = tid < nrows ? (a.w ? a.w[row0 + tid] : 1.f) : 0.f;

    if (pass0) {
    // ---- sweep 1: q and t of every component ----
    const float* za = zt + (16 * wave + col) * ldz + q;
    for (int k = 0; k < K; ++k) {
      __syncthreads();  // the rows are staged / the previous component is consumed
      const float* Wk = a.W + (int64_t)k * D * D;
      for (int d = wave; d < Dp; d += 4)
        for (int j = lane; j < D16; j += 64) ws[d * ldw + j] = d < D && j < D && d <= j ? Wk[d * D + j] : 0.f;
      for (int f = tid; f < D16; f += GM_THREADS) mus[f] = f < D ? a.mu[(int64_t)k * D + f] : 0.f;
      __syncthreads();
      f32x4_t acc[GM_TMAX];
#pragma unroll
      for (int u = 0; u < GM_TMAX; ++u) acc[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      for (int d0 = 0; d0 < Dp; d0 += 4) {
        const float av = za[d0] - mus[d0 + q];
        const float* wb = ws + (d0 + q) * ldw + col;
        const int ulo = d0 >> 4;  // column tiles left of the diagonal block hold zeros
#pragma unroll
        for (int u = 0; u < GM_TMAX; ++u)
          if (u >= ulo && u < T) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wb[16 * u], acc[u], 0, 0, 0);
      }
      const float ck = a.c[k];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float sq = 0.f;
#pragma unroll
        for (int u = 0; u < GM_TMAX; ++u)
          if (u < T) sq = fmaf(acc[u][g], acc[u][g], sq);
        sq = wops::row16_sum(sq);
        if (col == g) {
          const int r = 16 * wave + 4 * q + g;
          tl[r * ldt + k] = ck - 0.5f * sq;
          if (a.q && pass0 && r < nrows) a.q[(row0 + r) * K + k] = sq;
        }
      }
    }
    __syncthreads();

    // ---- the softmax epilogue: four lanes per row ----
    {
      const int r = tid >> 2, sub = tid & 3;
      float* tr = tl + r * ldt;
      const bool valid = r < nrows;
      float m = -INFINITY;
      for (int k = sub; k < K; k += 4) m = fmaxf(m, tr[k]);
      m = fmaxf(m, __shfl_xor(m, 1, 64));
      m = fmaxf(m, __shfl_xor(m, 2, 64));
      float s = 0.f;
      for (int k = sub; k < K; k += 4) {
        const float e = expf(tr[k] - m);
        tr[k] = e;
        s += e;
      }
      s += __shfl_xor(s, 1, 64);  // (s0 + s1) + (s2 + s3) in every lane: the adds commute
      s += __shfl_xor(s, 2, 64);
      const float lse = m + logf(s), wv = wl[r];
      float best = -1.f;
      int bi = 0;
      for (int k = sub; k < K; k += 4) {
        const float rv = tr[k] / s;
        if (rv > best) {  // strict: the lane's index only grows
          best = rv;
          bi = k;
        }
        tr[k] = wv * rv;
        if (a.wr && valid) a.wr[(row0 + r) * K + k] = wv * rv;
        if (a.resp && pass0 && valid) a.resp[(row0 + r) * K + k] = rv;
      }
#pragma unroll
      for (int o = 1; o <= 2; o <<= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        const bool take = ob > best || (ob == best && oi < bi);
        best = take ? ob : best;
        bi = take ? oi : bi;
      }
      if (sub == 0) {
        if (valid && pass0) {
          if (a.lse) a.lse[row0 + r] = lse;
          if (a.pred) a.pred[row0 + r] = bi;
        }
        red[r] = valid ? (double)wv * (double)lse : 0.0;
      }
    }
    __syncthreads();
    if (wave == 0) {
      const double v = wops::wave_sum_d_dpp(red[lane]);
      if (lane == 0 && pass0) part += v;
    }
    } else {
      // a later component group: the weighted responsibilities this workgroup stored on its first pass
      __syncthreads();
      for (int j = tid; j < GM_ROWS * (g1 - g0); j += GM_THREADS) {
        const int r = j / (g1 - g0), k = g0 + j - r * (g1 - g0);
        tl[r * ldt + k] = r < nrows ? a.wr[(row0 + r) * K + k] : 0.f;
      }
    }
    if (!slab) continue;

    // ---- sweep 2: the moments about mu_k of the group's components, into the LDS accumulators ----
    for (int k = g0; k < g1; ++k) {
      __syncthreads();  // the previous component's mu is consumed
      for (int f = tid; f < D16; f += GM_THREADS) mus[f] = f < D ? a.mu[(int64_t)k * D + f] : 0.f;
      __syncthreads();
      float* ak = accl + (k - g0) * p.accsz;
      if (tid < Dp) {
        const float mv = mus[tid];
        float s1 = 0.f;
        for (int n = 0; n < GM_ROWS; ++n) s1 = fmaf(tl[n * ldt + k], zt[n * ldz + tid] - mv, s1);
        ak[1 + tid] += s1;
      } else if (tid == GM_THREADS - 1) {
        float nk = 0.f;
        for (int n = 0; n < GM_ROWS; ++n) nk += tl[n * ldt + k];
        ak[0] += nk;
      }
      int ti = 0, tj = 0;  // pair index -> (ti <= tj), row-major over the upper triangle
      for (int pr = 0; pr < p.npairs; ++pr) {
        if ((pr & 3) == wave) {
          const float mi = mus[16 * ti + col], mj = mus[16 * tj + col];
          const float* zi = zt + q * ldz + 16 * ti + col;
          const float* zj = zt + q * ldz + 16 * tj + col;
          const float* wr = tl + q * ldt + k;
          float* pa = ak + 1 + Dp + pr * 256 + lane;  // the lane's own four words of the pair's C image
          f32x4_t acc = {pa[0], pa[64], pa[128], pa[192]};
#pragma unroll 4
          for (int n0 = 0; n0 < GM_ROWS; n0 += 4)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[n0 * ldt] * (zi[n0 * ldz] - mi), zj[n0 * ldz] - mj, acc, 0, 0, 0);
#pragma unroll
          for (int g = 0; g < 4; ++g) pa[64 * g] = acc[g];
        }
        if (++tj == T) {
          ++ti;
          tj = ti;
        }
      }
    }
  }
  if (!slab) break;
  // ---- the group's slab rows, once: every thread stores the words it accumulated ----
  __syncthreads();
  for (int k = g0; k < g1; ++k) {
    const float* ak = accl + (k - g0) * p.accsz;
    float* sk = slab + (int64_t)k * p.slab;
    if (tid < Dp) sk[1 + tid] = ak[1 + tid];
    else if (tid == GM_THREADS - 1) sk[0] = ak[0];
    int ti = 0, tj = 0;
    for (int pr = 0; pr < p.npairs; ++pr) {
      if ((pr & 3) == wave) {
        const float* pa = ak + 1 + Dp + pr * 256 + lane;
        const int j = 16 * tj + col;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int i = 16 * ti + 4 * q + g;
          if (i < Dp && j < Dp) sk[1 + Dp + i * Dp + j] = pa[64 * g];
        }
      }
      if (++tj == T) {
        ++ti;
        tj = ti;
      }
    }
  }
  __syncthreads();  // the accumulators are stored before the next group zeroes them
  }
  if (a.part && tid == 0) a.part[blockIdx.x] = part;
}

// One workgroup per component; see har_kernels.h.  LDS: A [D][D] fp64 | delta [D] | dinv [D].
__global__ __launch_bounds__(256) void gmm_finish_kernel(GmmFinishArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gf_lds[];
  __shared__ double nks[GM_MAXK];
  __shared__ int bad;
  const int tid = (int)threadIdx.x, k = (int)blockIdx.x, K = a.K, D = a.D, Dp = (D + 3) & ~3;
  if (a.state && !(a.state[1] == 0 && a.state[0] < a.max_iter)) return;  // (uniform)
  double* const A = reinterpret_cast<double*>(gf_lds);
  double* const delta = A + D * D;
  double* const dinv = delta + D;
  const int64_t sz = 1 + Dp + Dp * Dp;
  auto slab_sum = [&](int comp, int off) {
    double s = 0.0;
    for (int b = 0; b < a.nslab; ++b) s += (double)a.slabs[((int64_t)b * K + comp) * sz + off];
    return s;
  };
  if (tid < K) nks[tid] = slab_sum(tid, 0);
  if (tid == 0) bad = 0;
  __syncthreads();
  double ntot = 0.0;
  for (int j = 0; j < K; ++j) ntot += nks[j];
  const double nk = nks[k];
  const double pi = ntot > 0.0 ? nk / ntot : 0.0;
  const bool empty = !(nk > 0.0);
  float* const Wk = a.W + (int64_t)k * D * D;
  if (!empty) {
    for (int i = tid; i < D; i += 256) delta[i] = slab_sum(k, 1 + i) / nk;
    __syncthreads();
    for (int e = tid; e < D * D; e += 256) {
      const int i = e / D, j = e - i * D, lo = min(i, j), hi = max(i, j);
      double v = 0.0;
      if (i == j || !a.diag) v = slab_sum(k, 1 + Dp + lo * Dp + hi) / nk - delta[i] * delta[j];
      if (i == j) v += a.reg;
      A[e] = v;
    }
    __syncthreads();
    // right-looking Cholesky on the lower triangle
    const int ty = tid >> 4, tx = tid & 15;
    for (int j = 0; j < D; ++j) {
      if (tid == 0) {
        const double pv = A[j * D + j];
        if (!(pv > 0.0) || !isfinite(pv)) bad = 1;
        else A[j * D + j] = sqrt(pv);
      }
      __syncthreads();
      if (bad) break;
      const double ljj = A[j * D + j];
      for (int i = j + 1 + tid; i < D; i += 256) A[i * D + j] /= ljj;
      __syncthreads();
      for (int i = j + 1 + ty; i < D; i += 16) {
        const double lij = A[i * D + j];
        for (int l = j + 1 + tx; l <= i; l += 16) A[i * D + l] -= lij * A[l * D + j];
      }
      __syncthreads();
    }
  }
  const bool keep = empty || bad;  // (uniform: bad is read after a barrier)
  if (!keep) {
    for (int i = tid; i < D; i += 256) dinv[i] = 1.0 / A[i * D + i];
    __syncthreads();
    // column c of L^-1 by forward substitution, kept in row c of the upper triangle: it is row c of W
    for (int c = tid; c < D; c += 256) {
      for (int i = c + 1; i < D; ++i) {
        double s = A[i * D + c] * dinv[c];
        for (int l = c + 1; l < i; ++l) s += A[i * D + l] * A[c * D + l];
        A[c * D + i] = -s * dinv[i];
      }
    }
    __syncthreads();
    for (int e = tid; e < D * D; e += 256) {
      const int i = e / D, j = e - i * D;
      Wk[e] = i < j ? (float)A[e] : i == j ? (float)dinv[i] : 0.f;
    }
    for (int i = tid; i < D; i += 256) a.mu[(int64_t)k * D + i] = (float)((double)a.mu[(int64_t)k * D + i] + delta[i]);
  }
  if (tid == 0) {
    double logdet = 0.0;  // sum log L_ii; a kept factor gives it back from its own diagonal
    for (int i = 0; i < D; ++i) logdet += keep ? -log((double)Wk[i * D + i]) : log(A[i * D + i]);
    a.c[k] = (float)(log(pi) - 0.5 * D * 1.8378770664093453 - logdet);
    a.Nk[k] = nk;
    a.pi[k] = pi;
  }
}

// One workgroup: the log-likelihood in the fixed order of kmeans_update's cost, the history, the
// converged flag and the iteration counter.  state = {iterations, converged}.
__global__ __launch_bounds__(256) void gmm_control_kernel(GmmControlArgs a) {
  __shared__ double red[256];
  const int tid = (int)threadIdx.x;
  const bool live = a.state[1] == 0 && a.state[0] < a.max_iter;
  if (!live) return;
  double c = 0.0;
  for (int j = tid; j < a.npart; j += 256) c = __dadd_rn(c, a.part[j]);
  red[tid] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = __dadd_rn(red[tid], red[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    const int it = a.state[0];
    const double ll = red[0];
    a.hist[it] = ll;
    a.state[0] = it + 1;
    a.state[1] = it > 0 && fabs(ll - a.hist[it - 1]) <= a.tol ? 1 : 0;
  }
}

}  // namespace

extern "C" int har_gmm_rows_per_block() { return GM_ROWS; }

extern "C" int har_gmm_group(int D, int K) {
  GmPlan p;
  if (!gm_plan(D, K, true, p)) return -2;
  return p.grp;
}

extern "C" int har_gmm_grid(int64_t N, int D, int K, int max_blocks) {
  GmPlan p;
  if (N < 0 || !gm_plan(D, K, true, p)) return -2;
  return gm_grid(N, p, K, max_blocks);
}

extern "C" int har_gmm_estep(const GmmEstepArgs* args, hipStream_t s) {
  if (!args) return -4;
  const GmmEstepArgs& a = *args;
  GmPlan p;
  if (a.N < 0 || a.N > ((int64_t)1 << 31) - GM_ROWS || a.max_blocks < 0 || !gm_plan(a.D, a.K, a.slabs != nullptr, p))
    return -2;
  if (a.state && a.max_iter < 1) return -2;
  if (a.slabs && p.grp < a.K && !a.wr) return -4;
  if (!a.Z || !a.mu || !a.W || !a.c) return -4;
  if (a.N == 0) return 0;
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&gmm_estep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024) == hipSuccess;
  }();
  if (!attr) return -4;
  gmm_estep_kernel<<<(unsigned)gm_grid(a.N, p, a.K, a.max_blocks), GM_THREADS, (size_t)p.bytes, s>>>(a, p);
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_gmm_finish(const GmmFinishArgs* args, hipStream_t s) {
  if (!args) return -4;
  const GmmFinishArgs& a = *args;
  if (a.K < 1 || a.K > GM_MAXK || a.D < 1 || a.D > GM_MAXD || a.nslab < 1 || !(a.reg >= 0.0)) return -2;
  if (a.state && a.max_iter < 1) return -2;
  if (!a.slabs || !a.mu || !a.W || !a.c || !a.Nk || !a.pi) return -4;
  static bool attr = [] {
    // (the factor at D = 128 takes 130 KB; the static arrays share the 160 KB)
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&gmm_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               144 * 1024) == hipSuccess;
  }();
  if (!attr) return -4;
  const size_t bytes = ((size_t)a.D * a.D + 2 * (size_t)a.D) * sizeof(double);
  gmm_finish_kernel<<<(unsigned)a.K, 256, bytes, s>>>(a);
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_gmm_control(const GmmControlArgs* args, hipStream_t s) {
  if (!args) return -4;
  const GmmControlArgs& a = *args;
  if (a.npart < 0 || a.max_iter < 1 || !(a.tol >= 0.0)) return -2;
  if (!a.state || !a.hist || (a.npart && !a.part)) return -4;
  gmm_control_kernel<<<1, 256, 0, s>>>(a);
  HAR_CHECK_LAUNCH();
  return 0;
}
