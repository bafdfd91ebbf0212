// Banded dynamic time warping between raw windows: the cost of a (query, reference) pair on one lane,
// as a pairwise matrix (dtw_cost) or fused with a running top-k per query (dtw_search), and the merge of
// the reference splits' lists (dtw_merge).
//
// Definitions (har/ops/dtw.py states them once more as PyTorch code; the kernels compare to it):
//   * windows Q [N][W][A], R [M][W][A] fp32, time-major, finite; Sakoe-Chiba radius 0 <= radius <= W - 1.
//   * c(i, j) = sum_a (q[i][a] - r[j][a])^2 for |i - j| <= radius: d * d for a = 0, then one fma per axis
//     in ascending order.  D(0, 0) = c(0, 0), D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1))
//     over the predecessors inside the band and the grid: ONE add per cell.  dtw = D(W-1, W-1).
//   * neighbours: the k smallest PAIRS (dtw, m) in lexicographic order, ascending; a pair is skipped when
//     qgroup[n] >= 0 and qgroup[n] == rgroup[m]; missing entries: index -1, cost +inf (knn.hip's rule).
//
// Mapping: one lane per pair.  A wave takes ONE query against the DT_SLAB = 64 references of a slab, a
// workgroup DT_QROWS = 4 queries (one per wave) against the same slab.  The sweep goes over the REFERENCE
// samples j: a lane's own sample r[j] is A registers, read from an LDS chunk [sample][axis][lane] (lane
// stride 65: the transposing writes and the reads are both conflict free) that the workgroup stages
// DT_TJ samples at a time.  The band of column j lives in 2 RC + 1 registers indexed by e = i - j:
//     band[e] <- c(j + e, j) + min3(band[e - 1] (new: (i-1, j)), band[e + 1] (old: (i, j-1)), band[e] (old: (i-1, j-1)))
// for e ascending, in place; all register indices are static (RC, the radius cap, and AC, the axis cap,
// are template parameters).  The query samples q[j + e] are wave uniform: every wave stages the window
// q[j0 - RC, j0 + TJ + RC) of its query beside the chunk and reads it back as LDS broadcasts (as scalar
// loads the 3 (2 RC + 1) operands of a column did not fit the scalar registers: the compiler spilled).
// A virtual D(-1, -1) = 0 in band[0] starts the recurrence, cells outside the band or the grid are
// skipped (their slots hold +inf or values no admissible cell reads).  Columns whose cells are all
// admissible (radius == RC, RC <= j < W - RC) take a copy of the column without the tests.
//
// A pair's cost is this one operation sequence whatever slab, split, block or lane it sits in, and zero
// padded axes (A < AC) add fma(0, 0, c) = c: the lists are bitwise independent of the launch plan.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../har_kernels.h"

namespace {

constexpr int DT_WAVES = 4, DT_THREADS = 64 * DT_WAVES;
constexpr int DT_QROWS = DT_WAVES;  // queries per workgroup
constexpr int DT_SLAB = 64;         // references per slab: one per lane
constexpr int DT_TJ = 16;           // reference samples per staged chunk (both LDS images: 58 KiB at the largest caps)
constexpr int DT_LD = 65;           // lane stride of the chunk
constexpr int DT_MAXW = 512, DT_MAXR = 64, DT_MAXA = 9, DT_MAXK = 64, DT_MAXSPLITS = 1024;
constexpr int64_t DT_MAXROWS = ((int64_t)1 << 31) - 256;

// compiled radius / axis caps: the request rounds up to the next one
constexpr int DT_RC[] = {0, 1, 2, 4, 8, 12, 16, 20, 32, 48, 64};
constexpr int DT_AC[] = {1, 2, 3, 4, 6, 9};

int dt_rc(int R) {
  for (int v : DT_RC)
    if (v >= R) return v;
  return -1;
}

int dt_ac(int A) {
  for (int v : DT_AC)
    if (v >= A) return v;
  return -1;
}

struct DtPlan {
  int64_t N, M, nslabs;
  int W, A, radius, k, splits, search;
};

// entry (es, ei) precedes the candidate (cs, cm) in the (cost, index) order
__device__ __forceinline__ bool dt_before(float es, int ei, float cs, int cm) {
  return es < cs || (es == cs && ei < cm);
}

// The whole wave inserts the pair (cs, cm) into a sorted list of k entries, lane j holding entry j (lanes
// >= k: +inf, -1).  Returns false when the pair is not among the k smallest (nothing changes).
__device__ __forceinline__ bool dt_insert(float& es, int& ei, float cs, int cm, int k, int lane) {
  const int pos = __popcll(__ballot(lane < k && dt_before(es, ei, cs, cm)));  // the list is sorted: a prefix
  if (pos >= k) return false;
  const float us = __shfl_up(es, 1, 64);
  const int ui = __shfl_up(ei, 1, 64);
  if (lane < k && lane >= pos) {
    es = lane == pos ? cs : us;
    ei = lane == pos ? cm : ui;
  }
  return true;
}

// Column j of the pair's dynamic program (see the head of the file).  CHECK: test every cell against the
// band and the grid.
template <int RC, int AC, bool CHECK>
__device__ __forceinline__ void dt_column(float (&band)[2 * RC + 1], const float (&rv)[AC], const float* qw, int j,
                                          int W, int R) {
#pragma unroll
  for (int e = -RC; e <= RC; ++e) {
    const int i = j + e;
    const bool ok = !CHECK || (e >= -R && e <= R && i >= 0 && i < W);
    if (ok) {
      const float* qi = qw + (e + RC) * AC;  // q[i] in the staged window
      float d = __fsub_rn(qi[0], rv[0]);
      float c = __fmul_rn(d, d);
#pragma unroll
      for (int x = 1; x < AC; ++x) {
        d = __fsub_rn(qi[x], rv[x]);
        c = __fmaf_rn(d, d, c);
      }
      float best = band[e + RC];                              // (i - 1, j - 1)
      if (e > -RC) best = fminf(best, band[e - 1 + RC]);      // (i - 1, j), this column
      if (e < RC) best = fminf(best, band[e + 1 + RC]);       // (i, j - 1), the column before
      band[e + RC] = __fadd_rn(c, best);
    }
  }
}

template <int RC, int AC>
__global__ __launch_bounds__(DT_THREADS) void dtw_kernel(const float* __restrict__ Q, const float* __restrict__ Rf,
                                                         const int32_t* __restrict__ qgroup,
                                                         const int32_t* __restrict__ rgroup, float* __restrict__ cost,
                                                         float* __restrict__ ps, int32_t* __restrict__ pi, DtPlan p) {
  constexpr int TJ = DT_TJ, QW = (TJ + 2 * RC) * AC;
  __shared__ float rs[TJ * AC * DT_LD];
  __shared__ float qs[DT_WAVES * QW];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = p.W, A = p.A, R = p.radius, k = p.k;
  const int64_t n = (int64_t)blockIdx.x * DT_QROWS + wave;
  const bool qok = n < p.N;  // (wave uniform)
  const float* __restrict__ q = Q + (qok ? n : 0) * (int64_t)W * A;
  const int qg = qok && qgroup ? qgroup[n] : -1;
  float es = INFINITY;  // lane j: entry j of the query's list
  int ei = -1;

  // split t takes the slabs [t nslabs / splits, (t + 1) nslabs / splits): at least one each
  const int64_t s0 = (int64_t)blockIdx.y * p.nslabs / p.splits, s1 = (int64_t)(blockIdx.y + 1) * p.nslabs / p.splits;
  for (int64_t sl = s0; sl < s1; ++sl) {
    const int64_t m0 = sl * DT_SLAB, m = m0 + lane;
    float band[2 * RC + 1];
#pragma unroll
    for (int e = 0; e < 2 * RC + 1; ++e) band[e] = INFINITY;
    band[RC] = 0.f;  // D(-1, -1)
    for (int j0 = 0; j0 < W; j0 += TJ) {
      __syncthreads();  // every wave is done with the chunk before
      for (int t = lane; t < QW; t += 64) {  // the wave's query window q[j0 - RC, j0 + TJ + RC), zeros outside
        const int i = j0 - RC + t / AC, x = t % AC;
        qs[wave * QW + t] = qok && i >= 0 && i < W && x < A ? q[(int64_t)i * A + x] : 0.f;
      }
      for (int t = tid; t < DT_SLAB * TJ * AC; t += DT_THREADS) {
        const int ref = t / (TJ * AC), fl = t % (TJ * AC), jj = fl / AC, x = fl % AC;
        const int64_t mm = m0 + ref;
        float v = 0.f;
        if (mm < p.M && j0 + jj < W && x < A) v = Rf[(mm * W + (j0 + jj)) * A + x];
        rs[fl * DT_LD + ref] = v;
      }
      __syncthreads();
      if (qok) {
        const int jn = min(TJ, W - j0);
        for (int jj = 0; jj < jn; ++jj) {
          const int j = j0 + jj;
          float rv[AC];
#pragma unroll
          for (int x = 0; x < AC; ++x) rv[x] = rs[(jj * AC + x) * DT_LD + lane];
          const float* qw = qs + wave * QW + jj * AC;
          if (R == RC && j >= RC && j + RC < W) dt_column<RC, AC, false>(band, rv, qw, j, W, R);
          else dt_column<RC, AC, true>(band, rv, qw, j, W, R);
        }
      }
    }
    if (!qok) continue;
    const float c = band[RC];  // D(W - 1, W - 1)
    if (!p.search) {
      if (m < p.M) cost[n * p.M + m] = c;
      continue;
    }
    const int rg = m < p.M && rgroup ? rgroup[m] : -1;
    const float ts = __shfl(es, k - 1, 64);
    const int tm = __shfl(ei, k - 1, 64);
    // the current k-th pair (an empty entry is (+inf, -1)) does not precede the candidate
    bool want = m < p.M && !(qg >= 0 && qg == rg) && c < INFINITY && !dt_before(ts, tm, c, (int)m);
    unsigned long long mask;
    while ((mask = __ballot(want)) != 0ull) {
      const int src = __ffsll((long long)mask) - 1;
      dt_insert(es, ei, __shfl(c, src, 64), __shfl((int)m, src, 64), k, lane);
      if (lane == src) want = false;
    }
  }
  if (p.search && qok && lane < k) {
    const int64_t o = ((int64_t)blockIdx.y * p.N + n) * k + lane;
    ps[o] = es;
    pi[o] = ei;
  }
}

// A wave per query, lane j = list entry j: the k smallest pairs of the splits' sorted lists (split 0 is the
// start, the others are inserted in order; a list is left at its first entry that does not enter).
__global__ __launch_bounds__(256) void dtw_merge_kernel(DtwMergeArgs a) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * 4 + wave;
  if (n >= a.N) return;  // (no workgroup barrier below)
  const int k = a.k;
  float es = INFINITY;
  int ei = -1;
  if (lane < k) {
    es = a.ps[n * k + lane];
    ei = a.pi[n * k + lane];
  }
  for (int t = 1; t < a.splits; ++t) {
    const float* ps = a.ps + ((int64_t)t * a.N + n) * k;
    const int* pi = a.pi + ((int64_t)t * a.N + n) * k;
    for (int j = 0; j < k; ++j) {
      const int cm = pi[j];
      if (cm < 0 || !dt_insert(es, ei, ps[j], cm, k, lane)) break;  // (wave uniform)
    }
  }
  if (lane < k) {
    a.idx[n * k + lane] = ei;
    a.d2[n * k + lane] = ei >= 0 ? es : INFINITY;
  }
}

template <int RC, int AC>
int dt_launch(const DtwArgs& a, const DtPlan& p, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + DT_QROWS - 1) / DT_QROWS), (unsigned)p.splits);
  dtw_kernel<RC, AC><<<grid, DT_THREADS, 0, s>>>(a.Q, a.R, a.qgroup, a.rgroup, a.cost, a.ps, a.pi, p);
  HAR_CHECK_LAUNCH();
  return 0;
}

template <int RC>
int dt_dispatch_axes(int ac, const DtwArgs& a, const DtPlan& p, hipStream_t s) {
  switch (ac) {
    case 1: return dt_launch<RC, 1>(a, p, s);
    case 2: return dt_launch<RC, 2>(a, p, s);
    case 3: return dt_launch<RC, 3>(a, p, s);
    case 4: return dt_launch<RC, 4>(a, p, s);
    case 6: return dt_launch<RC, 6>(a, p, s);
    case 9: return dt_launch<RC, 9>(a, p, s);
  }
  return -2;
}

int dt_dispatch(const DtwArgs& a, const DtPlan& p, hipStream_t s) {
  const int ac = dt_ac(a.A);
  switch (dt_rc(a.radius)) {
    case 0: return dt_dispatch_axes<0>(ac, a, p, s);
    case 1: return dt_dispatch_axes<1>(ac, a, p, s);
    case 2: return dt_dispatch_axes<2>(ac, a, p, s);
    case 4: return dt_dispatch_axes<4>(ac, a, p, s);
    case 8: return dt_dispatch_axes<8>(ac, a, p, s);
    case 12: return dt_dispatch_axes<12>(ac, a, p, s);
    case 16: return dt_dispatch_axes<16>(ac, a, p, s);
    case 20: return dt_dispatch_axes<20>(ac, a, p, s);
    case 32: return dt_dispatch_axes<32>(ac, a, p, s);
    case 48: return dt_dispatch_axes<48>(ac, a, p, s);
    case 64: return dt_dispatch_axes<64>(ac, a, p, s);
  }
  return -2;
}

// the shape rules both entry points share
int dt_check(const DtwArgs& a) {
  if (a.N < 0 || a.N > DT_MAXROWS || a.M < 1 || a.M > DT_MAXROWS) return -2;
  if (a.W < 1 || a.W > DT_MAXW || a.A < 1 || a.A > DT_MAXA) return -2;
  if (a.radius < 0 || a.radius > DT_MAXR || a.radius > a.W - 1) return -2;
  if (!a.Q || !a.R) return -4;
  return 0;
}

}  // namespace

extern "C" int har_dtw_query_rows() { return DT_QROWS; }
extern "C" int har_dtw_slab_rows() { return DT_SLAB; }
extern "C" int har_dtw_max_w() { return DT_MAXW; }
extern "C" int har_dtw_max_radius() { return DT_MAXR; }
extern "C" int har_dtw_max_axes() { return DT_MAXA; }
extern "C" int har_dtw_max_k() { return DT_MAXK; }
extern "C" int har_dtw_max_splits() { return DT_MAXSPLITS; }

extern "C" int har_dtw_auto_splits(int64_t N, int64_t M) {
  if (N < 1 || M < 1) return -2;
  const int64_t nslabs = (M + DT_SLAB - 1) / DT_SLAB, qb = (N + DT_QROWS - 1) / DT_QROWS;
  // four workgroups of four waves per CU of the 256: small query counts split the references instead
  int64_t s = (1024 + qb - 1) / qb;
  s = s < nslabs ? s : nslabs;
  s = s < DT_MAXSPLITS ? s : DT_MAXSPLITS;
  return (int)(s < 1 ? 1 : s);
}

extern "C" int har_dtw_cost(const DtwArgs* args, hipStream_t s) {
  if (!args) return -4;
  const DtwArgs& a = *args;
  const int rc = dt_check(a);
  if (rc) return rc;
  if (!a.cost) return -4;
  DtPlan p{a.N, a.M, (a.M + DT_SLAB - 1) / DT_SLAB, a.W, a.A, a.radius, 1, 0, 0};
  if (p.nslabs > 65535) return -2;  // one workgroup row per slab (grid.y)
  p.splits = (int)p.nslabs;
  if (a.N == 0) return 0;
  return dt_dispatch(a, p, s);
}

extern "C" int har_dtw_search(const DtwArgs* args, hipStream_t s) {
  if (!args) return -4;
  const DtwArgs& a = *args;
  const int rc = dt_check(a);
  if (rc) return rc;
  if (a.k < 1 || a.k > DT_MAXK) return -2;
  DtPlan p{a.N, a.M, (a.M + DT_SLAB - 1) / DT_SLAB, a.W, a.A, a.radius, a.k, a.splits, 1};
  if (p.splits < 1 || p.splits > DT_MAXSPLITS || p.splits > p.nslabs) return -2;
  if ((a.qgroup == nullptr) != (a.rgroup == nullptr)) return -2;
  if (!a.ps || !a.pi) return -4;
  if (a.N == 0) return 0;
  return dt_dispatch(a, p, s);
}

extern "C" int har_dtw_merge(const DtwMergeArgs* args, hipStream_t s) {
  if (!args) return -4;
  const DtwMergeArgs& a = *args;
  if (a.N < 0 || a.N > DT_MAXROWS || a.k < 1 || a.k > DT_MAXK || a.splits < 1 || a.splits > DT_MAXSPLITS) return -2;
  if (!a.ps || !a.pi || !a.idx || !a.d2) return -4;
  if (a.N == 0) return 0;
  dtw_merge_kernel<<<(unsigned)((a.N + 3) / 4), 256, 0, s>>>(a);
  HAR_CHECK_LAUNCH();
  return 0;
}
