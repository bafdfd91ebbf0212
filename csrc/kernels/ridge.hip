// Ridge classifier: per-fold Gram moments on the exact-fp32 matrix cores, then a batch of bordered systems
// factored by a blocked Cholesky in fp64 (trailing update on v_mfma_f64_16x16x4_f64) and back-solved.
//
// Definitions (har/ops/ridge.py states them once more as PyTorch code; the kernels compare to it):
//   * augmented row a = [z | T | 1], Dq = D + K + 1 columns, z = fl32(fl32(x - mean) * inv_std) (two roundings,
//     no contraction), T[c] = +1 when y == c else -1.
//   * moments of fold f: A_f = sum over the fold's rows of a a^T.  The rows are taken in list order and cut
//     into chunks of RG_R rows from the fold's start; a chunk entry is ONE fp32 fma chain from zero in row order
//     (what v_mfma_f32_16x16x4_f32 computes: the reduction dimension is the rows), chunk results are added in
//     fp64.  A workgroup adds the chunks of its run in ascending order, ridge_gram_reduce adds the runs of a fold
//     in ascending order and the folds in ascending order into A_all.  No atomics anywhere.
//   * system (f, alpha), u = A_all - A_f entrywise (f = "all": u = A_all), q = D + K the column of ones, n = u[q][q]:
//     entry (r, c) = (u[c][r] - (u[c][q] * u[r][q]) / n) (+ alpha on the diagonal), one rounding per operation.
//     Rows r < D are M (lower triangle), rows D .. D + K - 1 the border Bc^T.
//   * M = L L^T by panels of RS_PANEL columns: factor the diagonal block in LDS, solve the rows below it (the
//     border rows included) against L_jj^T, update the trailing lower triangle.  After the last panel the border
//     rows hold (L^-1 Bc)^T.  A pivot that is not positive and finite sets info = 1 + its column; every later
//     step of that system returns at once and its W and b are zero.
//   * L^T W = Y per (system, class) by blocks of 64 from the last one, b = (t - W^T s) / n.
//
// ridge_gram tile: 64 x 64 entries of A per workgroup, four waves of 32 x 32 (2 x 2 MFMA tiles).  The LDS image
// of a tile is [row of the slab][column] fp32 with a row pitch of 80 floats: lane (i = lane & 15, k = lane >> 4)
// of both MFMA operands reads [4 step + k][column base + i], so a ds_read_b32 lane group {0-31} touches the banks
// (80 k + i) mod 32 = 16 k + i, k in {0, 1}: all 32 different, no transposing read.  A diagonal tile stages one
// image.  The fp64 panels use a pitch of 34 doubles: (34 i + k) mod 32 = 2 i + k, conflict-free for ds_read_b64.
#include <math.h>

#include "common.h"
#include "../har_kernels.h"

typedef __attribute__((ext_vector_type(4))) double f64x4_t;

namespace {

constexpr int RG_R = 256;       // rows per fp32 chain
constexpr int RG_T = 64;        // tile edge
constexpr int RG_SUB = 64;      // rows staged at a time (a chain runs over RG_R / RG_SUB stagings)
constexpr int RG_LD = 80;
constexpr int RG_THREADS = 256;
constexpr int RS_PANEL = 64;
constexpr int RS_LDP = 65;      // potrf / trsm images: one lane per row
constexpr int RS_LDU = 34;      // update images: MFMA operand reads
constexpr int RS_MAXDIM = 10240;
constexpr int RS_MAXK = 32, RS_MAXALPHA = 16;
constexpr int64_t RG_MAXROWS = ((int64_t)1 << 31) - 256;

__host__ __device__ inline int up64(int v) { return (v + 63) & ~63; }

// pair p of the upper triangle of an nt x nt tile grid, rows first: (0,0) (0,1) .. (0,nt-1) (1,1) ..
__device__ __forceinline__ void pair_of(int p, int nt, int& ti, int& tj) {
  ti = 0;
  while (p >= nt - ti) {
    p -= nt - ti;
    ++ti;
  }
  tj = ti + p;
}

__device__ __forceinline__ float rg_entry(const RidgeGramArgs& a, int64_t row, int yv, int g, float mu, float is) {
  if (g < a.D) return __fmul_rn(__fsub_rn(a.X[row * a.ldx + g], mu), is);
  if (g < a.D + a.K) return yv == g - a.D ? 1.f : -1.f;
  return g == a.D + a.K ? 1.f : 0.f;
}

__global__ __launch_bounds__(RG_THREADS) void ridge_gram_kernel(RidgeGramArgs a, int nt, int pairs, int smax) {
  __shared__ float img[2][RG_SUB * RG_LD];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  const int wi = wave >> 1, wj = wave & 1;
  const int f = (int)blockIdx.y / smax, sp = (int)blockIdx.y % smax;
  const int64_t f0 = a.off[f], nf = a.off[f + 1] - f0;
  const int64_t chunks = (nf + RG_R - 1) / RG_R;
  const int64_t c0 = (int64_t)sp * a.cps;
  if (c0 >= chunks) return;  // (uniform: before any barrier)
  const int64_t c1 = c0 + a.cps < chunks ? c0 + a.cps : chunks;
  int ti, tj;
  pair_of((int)blockIdx.x, nt, ti, tj);
  const bool diag = ti == tj;

  // staging: thread (column sc, row group wave) fills rows wave, wave + 4, ... of both images
  const int sc = tid & 63;
  const int gi = RG_T * ti + sc, gj = RG_T * tj + sc;
  const float mi = gi < a.D ? a.mean[gi] : 0.f, si = gi < a.D ? a.inv_std[gi] : 0.f;
  const float mj = gj < a.D ? a.mean[gj] : 0.f, sj = gj < a.D ? a.inv_std[gj] : 0.f;

  f64x4_t acc64[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc64[u][v] = f64x4_t{0.0, 0.0, 0.0, 0.0};

  const float* ia = img[0] + q * RG_LD + 32 * wi + col;
  const float* jb = img[diag ? 0 : 1] + q * RG_LD + 32 * wj + col;
  for (int64_t c = c0; c < c1; ++c) {
    f32x4_t acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int sub = 0; sub < RG_R / RG_SUB; ++sub) {
      const int64_t r0 = c * RG_R + (int64_t)sub * RG_SUB;
      if (r0 >= nf) break;  // (uniform)
      __syncthreads();      // every wave is done with the previous staging
      for (int r = wave; r < RG_SUB; r += 4) {
        const int64_t fr = r0 + r;
        float vi = 0.f, vj = 0.f;  // a row past the fold's end: exact zeros at the end of the chain
        if (fr < nf) {
          const int64_t row = a.rows[f0 + fr];
          const int yv = a.y[row];
          vi = rg_entry(a, row, yv, gi, mi, si);
          if (!diag) vj = rg_entry(a, row, yv, gj, mj, sj);
        }
        img[0][r * RG_LD + sc] = vi;
        if (!diag) img[1][r * RG_LD + sc] = vj;
      }
      __syncthreads();
#pragma unroll 4
      for (int ks = 0; ks < RG_SUB / 4; ++ks) {
        const float a0 = ia[4 * ks * RG_LD], a1 = ia[4 * ks * RG_LD + 16];
        const float b0 = jb[4 * ks * RG_LD], b1 = jb[4 * ks * RG_LD + 16];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc64[u][v][g] += (double)acc[u][v][g];
  }

  // fp32 C layout: column = lane & 15, row = 4 (lane >> 4) + register
  double* slab = a.slabs + (((int64_t)f * smax + sp) * pairs + blockIdx.x) * (RG_T * RG_T);
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        slab[(32 * wi + 16 * u + 4 * q + g) * RG_T + 32 * wj + 16 * v + col] = acc64[u][v][g];
}

__global__ __launch_bounds__(RG_THREADS) void ridge_gram_reduce_kernel(RidgeGramArgs a, int nt, int pairs, int smax,
                                                                       int ldq) {
  int ti, tj;
  pair_of((int)blockIdx.x, nt, ti, tj);
  const int e = (int)blockIdx.y * RG_THREADS + (int)threadIdx.x;  // < 4096
  const int i = RG_T * ti + e / RG_T, j = RG_T * tj + e % RG_T;
  if (i > j) return;
  double all = 0.0;
  for (int f = 0; f < a.F; ++f) {
    const int64_t nf = a.off[f + 1] - a.off[f];
    const int64_t chunks = (nf + RG_R - 1) / RG_R;
    const int ns = (int)((chunks + a.cps - 1) / a.cps);
    double sum = 0.0;
    for (int sp = 0; sp < ns; ++sp) sum += a.slabs[(((int64_t)f * smax + sp) * pairs + blockIdx.x) * (RG_T * RG_T) + e];
    if (a.Af) a.Af[((int64_t)f * ldq + i) * ldq + j] = sum;
    all += sum;
  }
  a.Aall[(int64_t)i * ldq + j] = all;
}

// ------------------------------------------------------------------ systems
__global__ __launch_bounds__(256) void ridge_systems_kernel(RidgeSolveArgs a, int ldq, int ldn) {
  __shared__ double t[16][17];
  const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
  const int s = a.sys0 + (int)blockIdx.z;
  const int fi = s / a.nalpha, ai = s % a.nalpha;
  const bool all = a.F == 1 || fi == a.F;
  const double* Af = all ? nullptr : a.Af + (int64_t)fi * ldq * ldq;
  const int qc = a.D + a.K;
  const int r = (int)blockIdx.y * 16 + ty, c = (int)blockIdx.x * 16 + tx;
  {  // u[c'][r'] with c' = 16 bx + ty, r' = 16 by + tx: rows of the upper triangle, read along r
    const int64_t o = (int64_t)((int)blockIdx.x * 16 + ty) * ldq + (int)blockIdx.y * 16 + tx;
    t[ty][tx] = Af ? __dsub_rn(a.Aall[o], Af[o]) : a.Aall[o];
  }
  __syncthreads();
  double val = 0.0;
  if (c <= r && c < a.D && r < qc) {
    const int64_t oc = (int64_t)c * ldq + qc, orr = (int64_t)r * ldq + qc, on = (int64_t)qc * ldq + qc;
    const double ucq = Af ? __dsub_rn(a.Aall[oc], Af[oc]) : a.Aall[oc];
    const double urq = Af ? __dsub_rn(a.Aall[orr], Af[orr]) : a.Aall[orr];
    const double n = Af ? __dsub_rn(a.Aall[on], Af[on]) : a.Aall[on];
    const double ct = n > 0.0 ? __ddiv_rn(__dmul_rn(ucq, urq), n) : 0.0;
    val = __dsub_rn(t[tx][ty], ct);
    if (r == c) val = __dadd_rn(val, a.alphas[ai]);
  }
  a.Sys[((int64_t)blockIdx.z * ldn + r) * ldn + c] = val;
}

// ------------------------------------------------------------------ Cholesky
// the diagonal block [j0, j0 + pw) of every system, one workgroup each
__global__ __launch_bounds__(256) void ridge_potrf_kernel(RidgeSolveArgs a, int ldn, int j0, int pw) {
  __shared__ double Ld[RS_PANEL * RS_LDP];
  const int tid = (int)threadIdx.x;
  const int s = a.sys0 + (int)blockIdx.x;
  if (a.info[s] != 0) return;
  double* A = a.Sys + (int64_t)blockIdx.x * ldn * ldn;
  for (int e = tid; e < RS_PANEL * RS_PANEL; e += 256) {
    const int i = e >> 6, c = e & 63;
    Ld[i * RS_LDP + c] = (i < pw && c <= i) ? A[(int64_t)(j0 + i) * ldn + j0 + c] : 0.0;
  }
  __syncthreads();
  for (int j = 0; j < pw; ++j) {
    const double d = Ld[j * RS_LDP + j];
    if (!(d > 0.0) || !isfinite(d)) {  // (uniform: every thread read the same word)
      if (tid == 0) a.info[s] = j0 + j + 1;
      return;
    }
    const double rt = __dsqrt_rn(d);
    __syncthreads();  // every thread has read the pivot
    if (tid == 0) Ld[j * RS_LDP + j] = rt;
    for (int i = j + 1 + tid; i < pw; i += 256) Ld[i * RS_LDP + j] = __ddiv_rn(Ld[i * RS_LDP + j], rt);
    __syncthreads();
    const int m = pw - j - 1;
    for (int e = tid; e < m * m; e += 256) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) Ld[i * RS_LDP + c] -= Ld[i * RS_LDP + j] * Ld[c * RS_LDP + j];
    }
    __syncthreads();
  }
  for (int e = tid; e < RS_PANEL * RS_PANEL; e += 256) {
    const int i = e >> 6, c = e & 63;
    if (i < pw && c <= i) A[(int64_t)(j0 + i) * ldn + j0 + c] = Ld[i * RS_LDP + c];
  }
}

// rows [j0 + pw + 64 rb, + 64) of the panel: X L_jj^T = B, one lane per row
__global__ __launch_bounds__(64) void ridge_trsm_kernel(RidgeSolveArgs a, int ldn, int nrow, int j0, int pw) {
  __shared__ double Lp[RS_PANEL * (RS_PANEL + 1) / 2];  // packed lower triangle: (c, k) at c (c + 1) / 2 + k
  __shared__ double B[RS_PANEL * RS_LDP];
  const int tid = (int)threadIdx.x;
  const int s = a.sys0 + (int)blockIdx.y;
  if (a.info[s] != 0) return;
  double* A = a.Sys + (int64_t)blockIdx.y * ldn * ldn;
  const int rs = j0 + pw + RS_PANEL * (int)blockIdx.x;
  for (int i = 0; i < RS_PANEL; ++i) {  // lane = column: coalesced rows
    if (tid <= i) Lp[i * (i + 1) / 2 + tid] = i < pw ? A[(int64_t)(j0 + i) * ldn + j0 + tid] : 0.0;
    B[i * RS_LDP + tid] = (rs + i < nrow && tid < pw) ? A[(int64_t)(rs + i) * ldn + j0 + tid] : 0.0;
  }
  __syncthreads();
  double* b = B + tid * RS_LDP;
  for (int c = 0; c < pw; ++c) {
    double v = b[c];
    const double* lc = Lp + c * (c + 1) / 2;
    for (int k = 0; k < c; ++k) v -= b[k] * lc[k];
    b[c] = __ddiv_rn(v, lc[c]);
  }
  __syncthreads();
  for (int i = 0; i < RS_PANEL; ++i)
    if (rs + i < nrow && tid < pw) A[(int64_t)(rs + i) * ldn + j0 + tid] = B[i * RS_LDP + tid];
}

// trailing update after a full panel at j0: A[r][c] -= sum_k P[r][k] P[c][k] over the 64 panel columns, for
// the 64 x 64 tiles (rt >= ct) of the columns [j0 + 64, D) and the rows up to nrow.  pair index: column tiles
// first, (ct0, ct0) (ct0 + 1, ct0) .. (nrt - 1, ct0) (ct0 + 1, ct0 + 1) ..
__global__ __launch_bounds__(256) void ridge_update_kernel(RidgeSolveArgs a, int ldn, int nrow, int j0, int ct0,
                                                           int nrt) {
  __shared__ double Pr[RS_PANEL * RS_LDU];
  __shared__ double Pc[RS_PANEL * RS_LDU];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  const int wi = wave >> 1, wj = wave & 1;
  const int s = a.sys0 + (int)blockIdx.y;
  if (a.info[s] != 0) return;
  double* A = a.Sys + (int64_t)blockIdx.y * ldn * ldn;
  int ct = ct0, p = (int)blockIdx.x;
  while (p >= nrt - ct) {
    p -= nrt - ct;
    ++ct;
  }
  const int rt = ct + p;
  const bool diag = rt == ct;

  f64x4_t acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  const double* pa = Pr + (32 * wi + col) * RS_LDU + q;
  const double* pb = (diag ? Pr : Pc) + (32 * wj + col) * RS_LDU + q;
  for (int kh = 0; kh < 2; ++kh) {
    __syncthreads();
    for (int e = tid; e < RS_PANEL * 32; e += 256) {
      const int i = e >> 5, k = e & 31;
      Pr[i * RS_LDU + k] = A[(int64_t)(RS_PANEL * rt + i) * ldn + j0 + 32 * kh + k];
      if (!diag) Pc[i * RS_LDU + k] = A[(int64_t)(RS_PANEL * ct + i) * ldn + j0 + 32 * kh + k];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const double a0 = pa[4 * ks], a1 = pa[16 * RS_LDU + 4 * ks];
      const double b0 = pb[4 * ks], b1 = pb[16 * RS_LDU + 4 * ks];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // fp64 C layout: column = lane & 15, row = (lane >> 4) + 4 register
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r = RS_PANEL * rt + 32 * wi + 16 * u + q + 4 * g;
        const int c = RS_PANEL * ct + 32 * wj + 16 * v + col;
        if (c < a.D && r >= c && r < nrow) {
          double* dst = A + (int64_t)r * ldn + c;
          *dst = *dst - acc[u][v][g];
        }
      }
}

// ------------------------------------------------------------------ back substitution
// one workgroup per (class, system): w in LDS [ldn], then the diagonal block image and the partial sums
__global__ __launch_bounds__(256) void ridge_backsolve_kernel(RidgeSolveArgs a, int ldq, int ldn, int ntot) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
  double* const w = reinterpret_cast<double*>(rs_lds);
  double* const Ld = w + ldn;
  double* const red = Ld + RS_PANEL * RS_LDP;  // [256]
  const int tid = (int)threadIdx.x, jl = tid & 63, g = tid >> 6;
  const int cls = (int)blockIdx.x;
  const int s = a.sys0 + (int)blockIdx.y;
  const int D = a.D;
  double* W64 = a.W64 + ((int64_t)s * a.K + cls) * ldn;
  float* W = a.W ? a.W + ((int64_t)s * a.K + cls) * D : nullptr;
  if (a.info[s] != 0) {
    for (int j = tid; j < ldn; j += 256) W64[j] = 0.0;
    if (W)
      for (int j = tid; j < D; j += 256) W[j] = 0.f;
    if (a.b && tid == 0) a.b[(int64_t)s * a.K + cls] = 0.f;
    return;
  }
  const double* A = a.Sys + (int64_t)blockIdx.y * ldn * ldn;
  const double* yrow = A + (int64_t)(D + cls) * ldn;
  for (int j = tid; j < ldn; j += 256) w[j] = 0.0;
  const int nb = (D + RS_PANEL - 1) / RS_PANEL;
  for (int jb = nb - 1; jb >= 0; --jb) {
    const int j0 = RS_PANEL * jb, pw = D - j0 < RS_PANEL ? D - j0 : RS_PANEL, jend = j0 + pw;
    __syncthreads();  // w of the later blocks is written; Ld and red are free
    double part = 0.0;
    if (jl < pw)
      for (int i = jend + g; i < D; i += 4) part = fma(A[(int64_t)i * ldn + j0 + jl], w[i], part);
    red[tid] = part;
    for (int e = tid; e < RS_PANEL * RS_PANEL; e += 256) {
      const int i = e >> 6, c = e & 63;
      Ld[i * RS_LDP + c] = (i < pw && c <= i) ? A[(int64_t)(j0 + i) * ldn + j0 + c] : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
      double rhs = 0.0, sol = 0.0;
      if (jl < pw) rhs = yrow[j0 + jl] - (((red[jl] + red[64 + jl]) + red[128 + jl]) + red[192 + jl]);
      for (int jj = pw - 1; jj >= 0; --jj) {
        const double wv = __ddiv_rn(__shfl(rhs, jj, 64), Ld[jj * RS_LDP + jj]);
        if (jl < jj) rhs -= Ld[jj * RS_LDP + jl] * wv;
        if (jl == jj) sol = wv;
      }
      if (jl < pw) w[j0 + jl] = sol;
    }
  }
  __syncthreads();
  for (int j = tid; j < ldn; j += 256) W64[j] = w[j];
  if (W)
    for (int j = tid; j < D; j += 256) W[j] = (float)w[j];
  if (!a.b) return;  // (uniform)
  // intercept: (t - <w, s>) / n from the moments, partial sums by thread then a fixed tree
  const int fi = s / a.nalpha;
  const bool all = a.F == 1 || fi == a.F;
  const double* Af = all ? nullptr : a.Af + (int64_t)fi * ldq * ldq;
  const int qc = D + a.K;
  auto u_at = [&](int i) {
    const int64_t o = (int64_t)i * ldq + qc;
    return Af ? __dsub_rn(a.Aall[o], Af[o]) : a.Aall[o];
  };
  double part = 0.0;
  for (int j = tid; j < D; j += 256) part = fma(w[j], u_at(j), part);
  __syncthreads();
  red[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double n = u_at(qc);
    a.b[(int64_t)s * a.K + cls] = n > 0.0 ? (float)__ddiv_rn(u_at(D + cls) - red[0], n) : 0.f;
  }
}

struct RgPlan {
  int nt, pairs, smax, ldq;
};

int rg_plan(const RidgeGramArgs& a, RgPlan& p) {
  if (a.D < 1 || a.K < 2 || a.K > RS_MAXK || a.F < 1 || a.F > HAR_RIDGE_MAX_FOLDS || a.cps < 1 || a.ldx < a.D) return -2;
  const int dq = a.D + a.K + 1;
  if (dq > RS_MAXDIM) return -2;
  if (a.off[0] != 0) return -2;
  int64_t cmax = 0;
  for (int f = 0; f < a.F; ++f) {
    const int64_t nf = a.off[f + 1] - a.off[f];
    if (nf < 0) return -2;
    const int64_t ch = (nf + RG_R - 1) / RG_R;
    cmax = ch > cmax ? ch : cmax;
  }
  if (a.off[a.F] > RG_MAXROWS) return -2;
  p.ldq = up64(dq);
  p.nt = p.ldq / RG_T;
  p.pairs = p.nt * (p.nt + 1) / 2;
  const int64_t smax = (cmax + a.cps - 1) / a.cps;
  if ((int64_t)a.F * smax > 65535) return -2;
  p.smax = (int)(smax < 1 ? 1 : smax);
  return 0;
}

int rs_check(const RidgeSolveArgs& a, bool moments) {
  if (a.D < 1 || a.K < 0 || a.K > RS_MAXK || a.F < 1 || a.F > HAR_RIDGE_MAX_FOLDS || a.nalpha < 1 ||
      a.nalpha > RS_MAXALPHA)
    return -2;
  if (a.D + a.K + 1 > RS_MAXDIM) return -2;
  const int total = (a.F > 1 ? a.F + 1 : 1) * a.nalpha;
  if (a.sys0 < 0 || a.nsys < 1 || a.sys0 + a.nsys > total) return -2;
  if (!a.Sys || !a.info) return -4;
  if (moments && (a.K < 2 || !a.Aall || !a.alphas || (a.F > 1 && !a.Af))) return a.K < 2 ? -2 : -4;
  return 0;
}

}  // namespace

extern "C" int har_ridge_chunk_rows() { return RG_R; }
extern "C" int har_ridge_panel() { return RS_PANEL; }
extern "C" int har_ridge_max_dim() { return RS_MAXDIM; }

extern "C" int har_ridge_gram(const RidgeGramArgs* args, hipStream_t s) {
  if (!args) return -4;
  const RidgeGramArgs& a = *args;
  RgPlan p;
  const int rc = rg_plan(a, p);
  if (rc) return rc;
  if (!a.X || !a.y || !a.rows || !a.mean || !a.inv_std || !a.slabs) return -4;
  if (a.off[a.F] == 0) return 0;
  ridge_gram_kernel<<<dim3((unsigned)p.pairs, (unsigned)(a.F * p.smax)), RG_THREADS, 0, s>>>(a, p.nt, p.pairs, p.smax);
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_ridge_gram_reduce(const RidgeGramArgs* args, hipStream_t s) {
  if (!args) return -4;
  const RidgeGramArgs& a = *args;
  RgPlan p;
  const int rc = rg_plan(a, p);
  if (rc) return rc;
  if (!a.slabs || !a.Aall || (a.F > 1 && !a.Af)) return -4;
  ridge_gram_reduce_kernel<<<dim3((unsigned)p.pairs, RG_T * RG_T / RG_THREADS), RG_THREADS, 0, s>>>(a, p.nt, p.pairs,
                                                                                                 p.smax, p.ldq);
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_ridge_systems(const RidgeSolveArgs* args, hipStream_t s) {
  if (!args) return -4;
  const RidgeSolveArgs& a = *args;
  const int rc = rs_check(a, true);
  if (rc) return rc;
  const int ldq = up64(a.D + a.K + 1), ldn = up64(a.D + a.K);
  ridge_systems_kernel<<<dim3((unsigned)(ldn / 16), (unsigned)(ldn / 16), (unsigned)a.nsys), dim3(16, 16), 0, s>>>(
      a, ldq, ldn);
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_ridge_cholesky(const RidgeSolveArgs* args, hipStream_t s) {
  if (!args) return -4;
  const RidgeSolveArgs& a = *args;
  const int rc = rs_check(a, false);
  if (rc) return rc;
  const int ldn = up64(a.D + a.K), nrow = a.D + a.K;
  const int nct = (a.D + RS_PANEL - 1) / RS_PANEL, nrt = (nrow + RS_PANEL - 1) / RS_PANEL;
  for (int j0 = 0; j0 < a.D; j0 += RS_PANEL) {
    const int pw = a.D - j0 < RS_PANEL ? a.D - j0 : RS_PANEL;
    ridge_potrf_kernel<<<(unsigned)a.nsys, 256, 0, s>>>(a, ldn, j0, pw);
    HAR_CHECK_LAUNCH();
    const int below = nrow - (j0 + pw);
    if (below > 0) {
      ridge_trsm_kernel<<<dim3((unsigned)((below + RS_PANEL - 1) / RS_PANEL), (unsigned)a.nsys), 64, 0, s>>>(a, ldn, nrow,
                                                                                                        j0, pw);
      HAR_CHECK_LAUNCH();
    }
    const int ct0 = j0 / RS_PANEL + 1;
    if (pw == RS_PANEL && ct0 < nct) {
      int pairs = 0;
      for (int ct = ct0; ct < nct; ++ct) pairs += nrt - ct;
      ridge_update_kernel<<<dim3((unsigned)pairs, (unsigned)a.nsys), 256, 0, s>>>(a, ldn, nrow, j0, ct0, nrt);
      HAR_CHECK_LAUNCH();
    }
  }
  return 0;
}

extern "C" int har_ridge_backsolve(const RidgeSolveArgs* args, hipStream_t s) {
  if (!args) return -4;
  const RidgeSolveArgs& a = *args;
  const int rc = rs_check(a, false);
  if (rc) return rc;
  if (a.K < 1) return -2;
  if (!a.W64) return -4;
  if (a.b && (!a.Aall || (a.F > 1 && !a.Af))) return -4;
  const int ldq = up64(a.D + a.K + 1), ldn = up64(a.D + a.K);
  const size_t bytes = ((size_t)ldn + RS_PANEL * RS_LDP + 256) * sizeof(double);
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&ridge_backsolve_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
  }();
  if (!attr || bytes > 160 * 1024) return -4;
  const int total = (a.F > 1 ? a.F + 1 : 1) * a.nalpha;
  ridge_backsolve_kernel<<<dim3((unsigned)a.K, (unsigned)a.nsys), 256, bytes, s>>>(a, ldq, ldn, total);
  HAR_CHECK_LAUNCH();
  return 0;
}
