// Gradient-boosted trees (multinomial softmax log-loss, Newton boosting): the per-round kernels.
//
// Every derivative is rounded to an int32 multiple of 2^-20 BEFORE anything is summed, so the level
// histograms, the node totals and the prefix sums of the split search are exact integer sums: their
// value does not depend on the order of the adds (LDS atomics, global atomics across workgroups), a
// fit is bitwise reproducible, and the kernels compare equal — not close — to the PyTorch definitions
// in har/ops/gbt.py.  The gain is evaluated in fp64 from those integers with a fixed operation order
// and explicit round-to-nearest intrinsics (no fused multiply-add).
//
// Layout: trees in heap order (children of n are 2n + 1 and 2n + 2; level d = nodes [2^d - 1, 2^(d+1) - 1)),
// K class trees per round in lock step, bins uint8 feature-major [F][N], qgh [K][N][2], node_of [K][N].
#include "common.h"
#include "wave_ops.h"
#include "../har_kernels.h"

#include <math.h>

#include <algorithm>
#include <climits>

namespace {

constexpr int GBT_KMAX = 32, GBT_MAX_DEPTH = 6, GBT_MAX_BINS = 64;
constexpr double GBT_Q = 1048576.0, GBT_INV_Q = 1.0 / 1048576.0;  // 2^20 quanta per unit
constexpr int64_t GBT_MAX_ROWS = ((int64_t)1 << 26) - 1024;  // <= 65,535 histogram row chunks (grid.y)
constexpr int HIST_ROWS = 1024;        // rows per histogram workgroup (4 per thread)
static_assert((GBT_MAX_ROWS + HIST_ROWS - 1) / HIST_ROWS <= 65535, "row chunks must fit grid.y");
constexpr int HIST_FC = 16;            // features per chunk (fewer when the level's LDS histogram is large)
constexpr int HIST_LDS = 64 * 1024;    // bytes of LDS histogram per workgroup
constexpr int HCH = 3;                 // channels per bin: g, h, rows of nonzero weight

// all-reduce over aligned groups of KP lanes (KP = 2 .. 32) on the VALU: quad permutes, the half-row
// and row mirrors, then the row swap.  Each step adds / maxes the lane's value with one partner's, the
// partners of a step hold the same pair of operands, so every lane of a group ends with the same bits.
template <int KP>
__device__ __forceinline__ double group_sum(double v, const wops::LaneSwap& sw) {
  if (KP >= 2) v += wops::dpp_d<0xb1>(v);   // quad_perm [1,0,3,2]
  if (KP >= 4) v += wops::dpp_d<0x4e>(v);   // quad_perm [2,3,0,1]
  if (KP >= 8) v += wops::dpp_d<0x141>(v);  // row_half_mirror
  if (KP >= 16) v += wops::dpp_d<0x140>(v); // row_mirror
  if (KP >= 32) v += sw.x16d(v);
  return v;
}
template <int KP>
__device__ __forceinline__ double group_max(double v, const wops::LaneSwap& sw) {
  if (KP >= 2) v = fmax(v, wops::dpp_d<0xb1>(v));
  if (KP >= 4) v = fmax(v, wops::dpp_d<0x4e>(v));
  if (KP >= 8) v = fmax(v, wops::dpp_d<0x141>(v));
  if (KP >= 16) v = fmax(v, wops::dpp_d<0x140>(v));
  if (KP >= 32) v = fmax(v, sw.x16d(v));
  return v;
}

// One lane per (row, class), KP = K rounded up to a power of two lanes per row.  fp64 softmax (the
// margins are fp32; +-100 stays finite: exp(m - max) <= 1), g = w (p - [y = k]), h = w max(p (1 - p), 1e-16),
// both rounded to 2^-20 quanta.  The loss partial of a workgroup sums -log p_y over its rows in a fixed
// order (wave butterfly, then the four waves in order): deterministic.
template <int KP>
__global__ __launch_bounds__(256) void gbt_grad_kernel(const float* __restrict__ margins, const int32_t* __restrict__ y,
                                                       const int32_t* __restrict__ w, int64_t N, int K,
                                                       int32_t* __restrict__ qgh, double* __restrict__ block_loss) {
  constexpr int RPB = 256 / KP;
  __shared__ double wl[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int k = tid % KP;
  const int64_t i = (int64_t)blockIdx.x * RPB + tid / KP;
  const bool row_ok = i < N, ok = row_ok && k < K;
  const wops::LaneSwap sw(lane);
  // lanes past K hold -inf (exp = 0); rows past N hold 0 everywhere (finite, discarded)
  const double m = ok ? (double)margins[i * K + k] : (row_ok ? -INFINITY : 0.0);
  const double mx = group_max<KP>(m, sw);
  const double e = exp(m - mx);
  const double se = group_sum<KP>(e, sw);
  const double p = e / se;
  const int yi = row_ok ? y[i] : -1;
  const bool wi = row_ok && (w == nullptr || w[i] != 0);
  if (ok && qgh != nullptr) {
    const double g = wi ? p - (k == yi ? 1.0 : 0.0) : 0.0;
    const double h = wi ? fmax(p * (1.0 - p), 1e-16) : 0.0;
    int2 q;
    q.x = (int)rint(g * GBT_Q);
    q.y = (int)rint(h * GBT_Q);
    reinterpret_cast<int2*>(qgh)[(int64_t)k * N + i] = q;
  }
  double l = (ok && k == yi) ? (log(se) + mx) - m : 0.0;
  l = wops::wave_sum_d_dpp(l);
  if (lane == 0) wl[tid >> 6] = l;
  __syncthreads();
  if (tid == 0) block_loss[blockIdx.x] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
}

// Level histograms.  Grid (feature chunk, row chunk, class); the workgroup's HIST_ROWS rows add their
// (g, h, 1) into an int32 LDS histogram [nodes][fc][maxb][3] at (node, feature, bin) and the nonzero cells
// are then merged into the int64 global histogram with integer atomics.
//
// No overflow: a row adds to ONE cell per feature, so an LDS cell receives at most HIST_ROWS = 2^10 adds
// of |q| <= 2^20 (the contract; |g| <= 1 and h <= 1/4 by construction) -> |cell| <= 2^30 < 2^31, and the
// count channel <= 2^10.  A global cell receives every row at most once: |total| <= N 2^20 <= 2^46 < 2^63
// for the N <= 2^26 - 1024 the launcher accepts.  Integer adds commute, so neither the LDS nor the global
// atomics' arrival order changes a bit of the result.
__global__ __launch_bounds__(256) void gbt_hist_kernel(const uint8_t* __restrict__ bins, const int32_t* __restrict__ qgh,
                                                       const int32_t* __restrict__ w,
                                                       const int32_t* __restrict__ node_of, int64_t N, int F, int maxb,
                                                       int first, int nodes, int fc,
                                                       unsigned long long* __restrict__ hist) {
  extern __shared__ int32_t lh[];
  const int tid = threadIdx.x;
  const int f0 = blockIdx.x * fc;
  const int nf = min(fc, F - f0);
  const int k = blockIdx.z;
  const int64_t r0 = (int64_t)blockIdx.y * HIST_ROWS;
  const int cell = maxb * HCH;
  const int total = nodes * fc * cell;
  for (int j = tid; j < total; j += 256) lh[j] = 0;
  __syncthreads();
  for (int r = 0; r < HIST_ROWS / 256; ++r) {
    const int64_t i = r0 + r * 256 + tid;
    if (i >= N) continue;
    const int nd = node_of[(int64_t)k * N + i] - first;
    if ((unsigned)nd >= (unsigned)nodes) continue;  // the row rests in a leaf of an earlier level
    const int2 q = reinterpret_cast<const int2*>(qgh)[(int64_t)k * N + i];
    const int c = (w == nullptr || w[i] != 0) ? 1 : 0;
    for (int fl = 0; fl < nf; ++fl) {
      const int b = bins[(int64_t)(f0 + fl) * N + i];
      if (b >= maxb) continue;  // (never for bins made with these thresholds: keeps the LDS index in range)
      int32_t* p = lh + (nd * fc + fl) * cell + b * HCH;
      if (q.x) atomicAdd(p, q.x);
      if (q.y) atomicAdd(p + 1, q.y);
      if (c) atomicAdd(p + 2, c);
    }
  }
  __syncthreads();
  for (int j = tid; j < total; j += 256) {
    const int v = lh[j];
    if (v == 0) continue;
    const int rest = j % cell, t = j / cell;
    const int fl = t % fc, nd = t / fc;
    if (fl >= nf) continue;
    const int64_t idx = (((int64_t)k * nodes + nd) * F + f0 + fl) * cell + rest;
    atomicAdd(hist + idx, (unsigned long long)(long long)v);  // two's complement: a signed add
  }
}

__device__ __forceinline__ long long wave_scan_ll(long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// G^2 / (H + lambda) of integer sums, in units: (G 2^-20)^2 / (H 2^-20 + lambda); 0 when the denominator is
// not positive.  Explicitly rounded operations: no contraction into a fused multiply-add.
__device__ __forceinline__ double gbt_score(long long G, long long H, double lambda, bool& pos) {
  const double g = __dmul_rn((double)G, GBT_INV_Q);
  const double d = __dadd_rn(__dmul_rn((double)H, GBT_INV_Q), lambda);
  pos = d > 0.0;
  return pos ? __ddiv_rn(__dmul_rn(g, g), d) : 0.0;
}
__device__ __forceinline__ float gbt_leaf(long long G, long long H, double lambda, double step) {
  const double g = __dmul_rn((double)G, GBT_INV_Q);
  const double d = __dadd_rn(__dmul_rn((double)H, GBT_INV_Q), lambda);
  return d > 0.0 ? (float)(-__dmul_rn(step, __ddiv_rn(g, d))) : 0.f;
}

// One workgroup per (node of the level, class tree); wave v searches features v, v + 4, ..., one lane per
// bin.  Node totals (G, H, C) are the sums over the bins of feature 0 (every row sits in exactly one bin of
// every feature).  A cut "bin <= b" (b < nbins[f] - 1) is valid when both children hold >= min_inst rows of
// nonzero weight, both H + lambda are positive and gain > min_gain.  Index f * 64 + b orders the ties.
__global__ __launch_bounds__(256) void gbt_split_kernel(GbtSplitArgs a, int first, int nodes) {
  __shared__ double sg[4];
  __shared__ int si[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nd = blockIdx.x, k = blockIdx.y;
  const int cell = a.maxb * HCH;
  const long long* h = reinterpret_cast<const long long*>(a.hist) + ((int64_t)k * nodes + nd) * a.F * cell;
  const wops::LaneSwap sw(lane);
  const int nb0 = min(max(a.nbins[0], 1), a.maxb);
  const bool in0 = lane < nb0;
  const long long G = wave_sum_ll(in0 ? h[lane * HCH] : 0), H = wave_sum_ll(in0 ? h[lane * HCH + 1] : 0),
                  C = wave_sum_ll(in0 ? h[lane * HCH + 2] : 0);
  bool ppos;
  const double parent = gbt_score(G, H, a.lambda, ppos);
  double bg = -INFINITY;
  int bidx = INT_MAX;
  for (int f = wave; f < a.F; f += 4) {
    const int nb = min(max(a.nbins[f], 1), a.maxb);
    const long long* hf = h + (int64_t)f * cell;
    const bool in = lane < nb;
    const long long GL = wave_scan_ll(in ? hf[lane * HCH] : 0, lane), HL = wave_scan_ll(in ? hf[lane * HCH + 1] : 0, lane),
                    CL = wave_scan_ll(in ? hf[lane * HCH + 2] : 0, lane);
    bool lpos, rpos;
    const double sl = gbt_score(GL, HL, a.lambda, lpos), sr = gbt_score(G - GL, H - HL, a.lambda, rpos);
    const double gain = __dmul_rn(0.5, __dadd_rn(__dadd_rn(sl, sr), -parent));
    const bool valid = lane < nb - 1 && CL >= a.min_inst && C - CL >= a.min_inst && lpos && rpos && gain > a.min_gain;
    if (valid) wops::argmax_combine(bg, bidx, gain, f * 64 + lane);
  }
  wops::wave_argmax(bg, bidx, sw);
  if (lane == 0) {
    sg[wave] = bg;
    si[wave] = bidx;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int v = 1; v < 4; ++v) wops::argmax_combine(bg, bidx, sg[v], si[v]);
  const bool split = bidx != INT_MAX;
  const int f = split ? bidx >> 6 : -1, b = split ? bidx & 63 : 0;
  long long GL = 0, HL = 0, CL = 0;
  if (split) {
    const long long* hf = h + (int64_t)f * cell;
    for (int j = 0; j <= b; ++j) {
      GL += hf[j * HCH];
      HL += hf[j * HCH + 1];
      CL += hf[j * HCH + 2];
    }
  }
  const int64_t o = (int64_t)k * nodes + nd;
  a.o_feat[o] = f;
  a.o_bin[o] = b;
  a.o_gain[o] = split ? bg : -INFINITY;
  int64_t* os = a.o_sums + o * 6;
  os[0] = GL; os[1] = HL; os[2] = CL; os[3] = G; os[4] = H; os[5] = C;
  // commit: the node, and — of a split — both children's leaf values (a child that splits at the next
  // level keeps its value unused); the root's own value at level 0
  const int n = first + nd;
  const int64_t base = (int64_t)(a.tree0 + k) * a.maxn;
  if (first == 0) {
    const float v = gbt_leaf(G, H, a.lambda, a.step);
    a.value[base] = v;
    a.stats[base * a.K + k] = v;
  }
  a.feature[base + n] = f;
  a.split_bin[base + n] = b;
  a.thresh[base + n] = split ? a.thr_mat[(int64_t)f * a.ldthr + b] : 0.f;
  a.left[base + n] = split ? 2 * n + 1 : 0;
  a.right[base + n] = split ? 2 * n + 2 : 0;
  a.gains[base + n] = split ? (float)bg : 0.f;
  if (split) {
    const float vl = gbt_leaf(GL, HL, a.lambda, a.step), vr = gbt_leaf(G - GL, H - HL, a.lambda, a.step);
    a.value[base + 2 * n + 1] = vl;
    a.value[base + 2 * n + 2] = vr;
    a.stats[(base + 2 * n + 1) * a.K + k] = vl;
    a.stats[(base + 2 * n + 2) * a.K + k] = vr;
  }
}

__global__ __launch_bounds__(256) void gbt_partition_kernel(int32_t* __restrict__ node_of, const uint8_t* __restrict__ bins,
                                                            const int32_t* __restrict__ feature,
                                                            const int32_t* __restrict__ split_bin, int64_t N, int F,
                                                            int first, int nodes, int tree0, int maxn) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  if (i >= N) return;
  const int n = node_of[(int64_t)k * N + i];
  if (n < first || n >= first + nodes) return;
  const int64_t base = (int64_t)(tree0 + k) * maxn;
  const int f = feature[base + n];
  if (f < 0 || f >= F) return;  // a leaf: the row stays
  const int b = bins[(int64_t)f * N + i];
  node_of[(int64_t)k * N + i] = 2 * n + 1 + (b > split_bin[base + n] ? 1 : 0);
}

__global__ __launch_bounds__(256) void gbt_update_kernel(float* __restrict__ margins, const int32_t* __restrict__ node_of,
                                                         const float* __restrict__ value, int64_t N, int K, int tree0,
                                                         int maxn) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= N * K) return;
  const int64_t i = j / K;
  const int k = (int)(j - i * K);
  const int n = node_of[(int64_t)k * N + i];
  if ((unsigned)n >= (unsigned)maxn) return;
  margins[j] += value[(int64_t)(tree0 + k) * maxn + n];
}

int grad_kp(int K) {
  int kp = 2;
  while (kp < K) kp <<= 1;
  return kp;
}

int hist_fc(int F, int nodes, int maxb) {
  const int per_feature = nodes * maxb * HCH * (int)sizeof(int32_t);
  return std::max(1, std::min(std::min(HIST_FC, F), HIST_LDS / per_feature));
}

}  // namespace

extern "C" int har_gbt_grad_blocks(int64_t N, int K) {
  if (N <= 0 || K < 2 || K > GBT_KMAX) return 0;
  const int rpb = 256 / grad_kp(K);
  return (int)((N + rpb - 1) / rpb);
}

extern "C" int har_gbt_grad(const float* margins, const int32_t* y, const int32_t* w, int64_t N, int K, int32_t* qgh,
                            double* block_loss, hipStream_t s) {
  if (K < 2 || K > GBT_KMAX || N < 0 || N > GBT_MAX_ROWS) return -2;
  if (N == 0) return 0;
  if (margins == nullptr || y == nullptr || block_loss == nullptr) return -4;
  const int kp = grad_kp(K);
  const int grid = har_gbt_grad_blocks(N, K);
  switch (kp) {
    case 2: gbt_grad_kernel<2><<<grid, 256, 0, s>>>(margins, y, w, N, K, qgh, block_loss); break;
    case 4: gbt_grad_kernel<4><<<grid, 256, 0, s>>>(margins, y, w, N, K, qgh, block_loss); break;
    case 8: gbt_grad_kernel<8><<<grid, 256, 0, s>>>(margins, y, w, N, K, qgh, block_loss); break;
    case 16: gbt_grad_kernel<16><<<grid, 256, 0, s>>>(margins, y, w, N, K, qgh, block_loss); break;
    default: gbt_grad_kernel<32><<<grid, 256, 0, s>>>(margins, y, w, N, K, qgh, block_loss); break;
  }
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_gbt_hist_rows_per_block() { return HIST_ROWS; }

extern "C" int har_gbt_hist(const uint8_t* bins, const int32_t* qgh, const int32_t* w, const int32_t* node_of, int64_t N,
                            int F, int K, int maxb, int level, int64_t* hist, hipStream_t s) {
  if (K < 1 || K > GBT_KMAX || level < 0 || level >= GBT_MAX_DEPTH || maxb < 2 || maxb > GBT_MAX_BINS || F < 1 ||
      F > 65535 || N < 0 || N > GBT_MAX_ROWS)
    return -2;
  if (bins == nullptr || qgh == nullptr || node_of == nullptr || hist == nullptr) return -4;
  const int nodes = 1 << level;
  const size_t bytes = (size_t)K * nodes * F * maxb * HCH * sizeof(int64_t);
  hipError_t e = hipMemsetAsync(hist, 0, bytes, s);
  if (e != hipSuccess) return (int)e;
  if (N == 0) return 0;
  const int fc = hist_fc(F, nodes, maxb);
  const dim3 grid((unsigned)((F + fc - 1) / fc), (unsigned)((N + HIST_ROWS - 1) / HIST_ROWS), (unsigned)K);
  const size_t lds = (size_t)nodes * fc * maxb * HCH * sizeof(int32_t);
  gbt_hist_kernel<<<grid, 256, lds, s>>>(bins, qgh, w, node_of, N, F, maxb, nodes - 1, nodes, fc,
                                         reinterpret_cast<unsigned long long*>(hist));
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_gbt_split(const GbtSplitArgs* a, hipStream_t s) {
  if (a == nullptr) return -4;
  if (a->K < 1 || a->K > GBT_KMAX || a->level < 0 || a->level >= GBT_MAX_DEPTH || a->maxb < 2 || a->maxb > GBT_MAX_BINS ||
      a->F < 1 || a->F > 65535 || a->ldthr < a->maxb - 1 || a->tree0 < 0 || a->min_inst < 1)
    return -2;
  // the level's nodes and their children must fit the heap arrays
  if (a->maxn < (1 << (a->level + 2)) - 1) return -2;
  if (a->hist == nullptr || a->nbins == nullptr || a->thr_mat == nullptr || a->o_feat == nullptr || a->o_bin == nullptr ||
      a->o_gain == nullptr || a->o_sums == nullptr || a->feature == nullptr || a->split_bin == nullptr ||
      a->thresh == nullptr || a->left == nullptr || a->right == nullptr || a->gains == nullptr || a->value == nullptr ||
      a->stats == nullptr)
    return -4;
  const int nodes = 1 << a->level;
  gbt_split_kernel<<<dim3((unsigned)nodes, (unsigned)a->K), 256, 0, s>>>(*a, nodes - 1, nodes);
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_gbt_partition(int32_t* node_of, const uint8_t* bins, const int32_t* feature, const int32_t* split_bin,
                                 int64_t N, int F, int K, int level, int tree0, int maxn, hipStream_t s) {
  if (K < 1 || K > GBT_KMAX || level < 0 || level >= GBT_MAX_DEPTH || F < 1 || N < 0 || N > GBT_MAX_ROWS || tree0 < 0 ||
      maxn < (1 << (level + 2)) - 1)
    return -2;
  if (node_of == nullptr || bins == nullptr || feature == nullptr || split_bin == nullptr) return -4;
  if (N == 0) return 0;
  const int nodes = 1 << level;
  gbt_partition_kernel<<<dim3((unsigned)((N + 255) / 256), (unsigned)K), 256, 0, s>>>(node_of, bins, feature, split_bin, N,
                                                                                      F, nodes - 1, nodes, tree0, maxn);
  HAR_CHECK_LAUNCH();
  return 0;
}

extern "C" int har_gbt_update(float* margins, const int32_t* node_of, const float* value, int64_t N, int K, int tree0,
                              int maxn, hipStream_t s) {
  if (K < 1 || K > GBT_KMAX || N < 0 || N > GBT_MAX_ROWS || tree0 < 0 || maxn < 1 || maxn > (1 << (GBT_MAX_DEPTH + 1)) - 1)
    return -2;
  if (margins == nullptr || node_of == nullptr || value == nullptr) return -4;
  if (N == 0) return 0;
  gbt_update_kernel<<<(unsigned)((N * K + 255) / 256), 256, 0, s>>>(margins, node_of, value, N, K, tree0, maxn);
  HAR_CHECK_LAUNCH();
  return 0;
}
