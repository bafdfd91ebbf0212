// K-means (Lloyd iterations) and the squared-Euclidean silhouette: a rows-by-centres product on the
// exact-fp32 matrix cores with the argmin / silhouette epilogue on the C layout, fixed-point cluster
// sums, and a one-workgroup update kernel that keeps the whole fit on the device.
//
// Definitions (har/ops/kmeans.py states them once more as PyTorch code; the kernels compare to it):
//   * working rows X [N][D] are already centred; centres C [K][D], h[k] = ||C[k]||^2 / 2.
//   * score s[n][k] = h[k] - <X[n], C[k]>, assignment = argmin over k, the LOWEST k among equal scores.
//   * nrm[n] = (p0 + p1) + (p2 + p3), p_j = the fp64 sum of X[n][f]^2 over f = j, j + 4, ... in that order
//     (a square of an fp32 is exact in fp64, so a fused multiply-add gives the same bits).
//   * d2[n] = float(max(0, nrm + 2 s)) evaluated in fp64 from the fp32 score.
//   * accumulators: one flat int64 buffer [K D sums | K counts | K norms]; row n of weight w adds
//     w rint(X[n][f] 2^e[f]), w and w rint(nrm 2^q) to its cluster.  Integer adds commute: LDS atomics,
//     global atomics and any number of workgroups give the same bits.
//   * cost partial of a workgroup = sum of w d2 over its rows in a fixed order (fp64).
//
// The product.  A workgroup of four waves owns KM_CHUNK = 256 consecutive rows, 64 per wave as four
// 16-row tiles.  It stages a slab of centres (all of them when they fit) and their h in LDS, rows
// padded to a multiple of 4 in D and the slab to a multiple of 16 in K (padding centres: zeros, h = +inf:
// never chosen).  Each wave stages its 16-row tile and runs v_mfma_f32_16x16x4_f32 against every
// 16-centre tile, NCT tiles per sweep of D so one A read feeds NCT MFMAs.  Both images have a row
// stride of Dp + 2 floats: the 32 lanes of a ds_read_b32 group (16 rows x 2 k-phases) then hit 32
// different banks.  On the C layout (col = lane & 15 = centre, row = 4 (lane >> 4) + reg) each lane keeps a
// running (min, argmin) of its four rows — strict <, and a lane's centre index only grows, so the
// lower index survives — and one 16-lane DPP reduction per row joins them.  Slabs are visited in
// ascending order and merged with strict < as well.
#include <math.h>

#include <type_traits>

#include "common.h"
#include "wave_ops.h"
#include "../har_kernels.h"

namespace {

constexpr int KM_CHUNK = 256;            // rows per workgroup
constexpr int KM_THREADS = 256;
constexpr int KM_TILES = KM_CHUNK / 64;  // 16-row tiles per wave
constexpr int KM_MAXK = 256, KM_MAXD = 256;
constexpr int NCT = 4;                   // centre tiles per sweep of D
constexpr int64_t KM_LDS_MAX = 160 * 1024;
constexpr int64_t KM_ACC_LDS = 48 * 1024;  // the int64 accumulators go through LDS up to this size

enum { MODE_ASSIGN = 0, MODE_SIL = 1 };

__host__ __device__ constexpr int km_ld(int D) { return ((D + 3) & ~3) + 2; }

// LDS image (bytes): [rn double 256][acc int64 nacc][rmin float 256][rarg int 256][raux float 256]
//                    [hs float kt][cs float kt * ld][xt float 4 * 16 * ld]
struct KmPlan {
  int ld, kt, npass, lds_acc;
  int64_t bytes;
};

bool km_plan(int D, int K, bool want_acc, KmPlan& p) {
  if (D < 1 || D > KM_MAXD || K < 1 || K > KM_MAXK) return false;
  p.ld = km_ld(D);
  const int Kp = (K + 15) & ~15;
  const int64_t fixed = 256 * 8 + 3 * 256 * 4 + (int64_t)4 * 16 * p.ld * 4;
  const int64_t acc = (int64_t)K * (D + 2) * 8;
  p.lds_acc = want_acc && acc <= KM_ACC_LDS ? 1 : 0;
  const int64_t left = KM_LDS_MAX - fixed - (p.lds_acc ? acc : 0);
  int kt = (int)(left / ((int64_t)(p.ld + 1) * 4));
  kt = kt & ~15;
  if (kt < 16) return false;
  if (kt > Kp) kt = Kp;
  p.kt = kt;
  p.npass = (Kp + kt - 1) / kt;
  p.bytes = fixed + (p.lds_acc ? acc : 0) + (int64_t)kt * (p.ld + 1) * 4;
  return true;
}

// (min, lowest index) over the 16 lanes of a DPP row; every lane ends with the winner
__device__ __forceinline__ void row16_argmin(float& v, int& i) {
  auto comb = [&](float ov, int oi) {
    const bool take = ov < v || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
  };
  comb(wops::dpp_f<wops::DPP_ROR8>(v), wops::dpp_i<wops::DPP_ROR8>(i));
  comb(wops::dpp_f<wops::DPP_ROR4>(v), wops::dpp_i<wops::DPP_ROR4>(i));
  comb(wops::dpp_f<wops::DPP_ROR2>(v), wops::dpp_i<wops::DPP_ROR2>(i));
  comb(wops::dpp_f<wops::DPP_ROR1>(v), wops::dpp_i<wops::DPP_ROR1>(i));
}
__device__ __forceinline__ float row16_minf(float v) {
  v = fminf(v, wops::dpp_f<wops::DPP_ROR8>(v));
  v = fminf(v, wops::dpp_f<wops::DPP_ROR4>(v));
  v = fminf(v, wops::dpp_f<wops::DPP_ROR2>(v));
  return fminf(v, wops::dpp_f<wops::DPP_ROR1>(v));
}

// Scores of one staged 16-row tile against NT centre tiles starting at tile ct0 of the slab: the shared
// product of the assignment and the silhouette.  acc[u][g] = <row 4 q + g, centre 16 (ct0 + u) + col>.
template <int NT>
__device__ __forceinline__ void km_product(const float* __restrict__ xa, const float* __restrict__ cb, int ld, int Dp,
                                           f32x4_t (&acc)[NT]) {
#pragma unroll
  for (int u = 0; u < NT; ++u) acc[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int d0 = 0; d0 < Dp; d0 += 4) {
    const float a = xa[d0];
#pragma unroll
    for (int u = 0; u < NT; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, cb[u * 16 * ld + d0], acc[u], 0, 0, 0);
  }
}

template <int MODE>
__global__ __launch_bounds__(KM_THREADS) void kmeans_kernel(KMeansArgs a, KmPlan p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  const int D = a.D, K = a.K, ld = p.ld, Dp = ld - 2;
  const int nacc = p.lds_acc ? K * (D + 2) : 0;
  double* const rn = reinterpret_cast<double*>(km_lds);
  unsigned long long* const lacc = reinterpret_cast<unsigned long long*>(rn + KM_CHUNK);
  float* const rmin = reinterpret_cast<float*>(lacc + nacc);
  int* const rarg = reinterpret_cast<int*>(rmin + KM_CHUNK);
  float* const raux = reinterpret_cast<float*>(rarg + KM_CHUNK);
  float* const hs = raux + KM_CHUNK;
  float* const cs = hs + p.kt;
  float* const xt = cs + (int64_t)p.kt * ld + wave * 16 * ld;
  const int64_t row0 = (int64_t)blockIdx.x * KM_CHUNK;
  const int nrows = (int)min<int64_t>(KM_CHUNK, a.N - row0);
  // given labels (assignment mode): no product, the accumulators take the caller's clusters
  const bool given = MODE == MODE_ASSIGN && a.labels != nullptr;
  const int npass = given ? 0 : p.npass;

  for (int j = tid; j < nacc; j += KM_THREADS) lacc[j] = 0ull;
  rmin[tid] = INFINITY;
  rarg[tid] = 0;
  raux[tid] = INFINITY;

  for (int pass = 0; pass < (given ? 1 : npass); ++pass) {
    const int k0 = pass * p.kt;
    if (!given) {
      if (pass) __syncthreads();  // every wave is done with the previous slab
      for (int kl = wave; kl < p.kt; kl += 4) {
        const int k = k0 + kl;
        const bool ok = k < K;
        for (int f = lane; f < ld; f += 64) cs[kl * ld + f] = ok && f < D ? a.C[(int64_t)k * D + f] : 0.f;
        if (lane == 0) {
          float hv = INFINITY;
          if (ok) {
            hv = a.h[k];
            // silhouette: an empty cluster (size 0) is no neighbour
            if (MODE == MODE_SIL && !(a.cnt[k] > 0.0)) hv = INFINITY;
          }
          hs[kl] = hv;
        }
      }
    }
    const int ktiles = min(p.kt, ((K + 15) & ~15) - k0) >> 4;
    for (int t = 0; t < KM_TILES; ++t) {
      const int tr0 = 64 * wave + 16 * t;  // first row of the tile within the chunk
      __syncthreads();                     // the slab is staged / the wave's previous tile is consumed
      for (int r = 0; r < 16; ++r) {
        const bool ok = tr0 + r < nrows;
        const float* src = a.X + (row0 + tr0 + r) * D;
        for (int f = lane; f < ld; f += 64) xt[r * ld + f] = ok && f < D ? src[f] : 0.f;
      }
      __syncthreads();
      const float* xa = xt + col * ld + q;
      if (pass == 0) {
        // the row norms, from the A fragments: lane (col, q) sums f = q, q + 4, ... of row col
        double pn = 0.0;
        for (int d0 = 0; d0 < Dp; d0 += 4) {
          const double x = (double)xa[d0];
          pn = fma(x, x, pn);
        }
        pn += __shfl_xor(pn, 16, 64);  // p0 + p1 | p2 + p3
        pn += __shfl_xor(pn, 32, 64);  // (p0 + p1) + (p2 + p3), the same bits in either operand order
        if (q == 0) rn[tr0 + col] = pn;
      }
      if (given) continue;
      float best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
      int bidx[4] = {0, 0, 0, 0};
      float own[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
      int lab[4] = {-1, -1, -1, -1};
      if (MODE == MODE_SIL) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int r = tr0 + 4 * q + g;
          lab[g] = r < nrows ? a.labels[row0 + r] : -1;
        }
      }
      auto sweep = [&](auto nt_c, int ct0) {
        constexpr int NT = decltype(nt_c)::value;
        f32x4_t acc[NT];
        km_product<NT>(xa, cs + (16 * ct0 + col) * ld + q, ld, Dp, acc);
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          const int kl = 16 * (ct0 + u) + col;
          const float hv = hs[kl];
          const int kidx = k0 + kl;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float s = hv - acc[u][g];
            if (MODE == MODE_ASSIGN) {
              const bool up = s < best[g];  // strict: the lane's index only grows, ties keep the lowest
              best[g] = up ? s : best[g];
              bidx[g] = up ? kidx : bidx[g];
            } else {
              const bool mine = kidx == lab[g];
              own[g] = mine ? s : own[g];
              best[g] = mine ? best[g] : fminf(best[g], s);
            }
          }
        }
      };
      for (int ct0 = 0; ct0 < ktiles; ct0 += NCT) {
        const int ntl = min(NCT, ktiles - ct0);
        if (ntl == 4) sweep(std::integral_constant<int, 4>{}, ct0);
        else if (ntl == 3) sweep(std::integral_constant<int, 3>{}, ct0);
        else if (ntl == 2) sweep(std::integral_constant<int, 2>{}, ct0);
        else sweep(std::integral_constant<int, 1>{}, ct0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r = tr0 + 4 * q + g;
        if (MODE == MODE_ASSIGN) {
          float v = best[g];
          int i = bidx[g];
          row16_argmin(v, i);
          if (col == g && v < rmin[r]) {  // strict: an earlier slab holds the lower indices
            rmin[r] = v;
            rarg[r] = i;
          }
        } else {
          const float b = row16_minf(best[g]), o = row16_minf(own[g]);
          if (col == g) {
            rmin[r] = fminf(rmin[r], b);
            raux[r] = fminf(raux[r], o);
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- one thread per row ----
  const bool valid = tid < nrows;
  const int64_t row = row0 + tid;
  double part = 0.0;
  if (MODE == MODE_ASSIGN) {
    int k = given ? (valid ? a.labels[row] : 0) : rarg[tid];
    const bool kok = (unsigned)k < (unsigned)K;
    k = kok ? k : 0;
    if (given) rarg[tid] = kok ? k : -1;
    const int wv = valid && kok ? (a.w ? a.w[row] : 1) : 0;
    const double nrm = rn[tid];
    if (!given && valid) {
      const float d2 = (float)fmax(0.0, nrm + 2.0 * (double)rmin[tid]);
      if (a.assign) a.assign[row] = k;
      if (a.d2) a.d2[row] = d2;
      part = (double)wv * (double)d2;
    }
    if (a.acc && wv != 0) {
      unsigned long long* dst = p.lds_acc ? lacc : reinterpret_cast<unsigned long long*>(a.acc);
      atomicAdd(dst + (int64_t)K * D + k, (unsigned long long)(long long)wv);
      const long long qn = (long long)wv * llrint(nrm * a.norm_scale[0]);
      if (qn) atomicAdd(dst + (int64_t)K * D + K + k, (unsigned long long)qn);
    }
  } else if (valid) {
    const int k = a.labels[row];
    double sil = 0.0;
    if ((unsigned)k < (unsigned)K) {
      const double nrm = rn[tid], na = a.cnt[k];
      const double b = fmax(0.0, nrm + 2.0 * (double)rmin[tid]);
      if (na > 1.0 && isfinite(b) && isfinite(raux[tid])) {
        const double av = fmax(0.0, nrm + 2.0 * (double)raux[tid]) * na / (na - 1.0);
        const double mx = fmax(av, b);
        sil = mx > 0.0 ? (b - av) / mx : 0.0;
      }
    }
    if (a.sil) a.sil[row] = (float)sil;
    part = sil;
  }
  __syncthreads();  // rn is read; it now carries the per-row partials
  rn[tid] = part;
  __syncthreads();
  if (a.part && wave == 0) {
    double v = ((rn[lane] + rn[lane + 64]) + rn[lane + 128]) + rn[lane + 192];
    v = wops::wave_sum_d_dpp(v);
    if (lane == 0) a.part[blockIdx.x] = v;
  }
  if (MODE != MODE_ASSIGN || !a.acc) return;

  // ---- cluster sums: a wave per row, a lane per feature ----
  unsigned long long* dst = p.lds_acc ? lacc : reinterpret_cast<unsigned long long*>(a.acc);
  for (int r = wave; r < nrows; r += 4) {
    const int k = rarg[r];
    const int wv = k < 0 ? 0 : (a.w ? a.w[row0 + r] : 1);
    if (wv == 0) continue;  // (wave-uniform)
    const float* src = a.X + (row0 + r) * D;
    for (int f = lane; f < D; f += 64) {
      const long long v = (long long)wv * (long long)__float2int_rn(src[f] * a.scale[f]);
      if (v) atomicAdd(dst + (int64_t)k * D + f, (unsigned long long)v);  // two's complement: a signed add
    }
  }
  if (!p.lds_acc) return;
  __syncthreads();
  unsigned long long* g = reinterpret_cast<unsigned long long*>(a.acc);
  for (int j = tid; j < nacc; j += KM_THREADS) {
    const unsigned long long v = lacc[j];
    if (v) atomicAdd(g + j, v);
  }
}

template <int MODE>
int km_launch(const KMeansArgs& a, const KmPlan& p, hipStream_t s) {
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&kmeans_kernel<MODE>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)KM_LDS_MAX) == hipSuccess;
  }();
  if (!attr) return -4;
  const int64_t nblk = (a.N + KM_CHUNK - 1) / KM_CHUNK;
  if (nblk > 0x7fffffff) return -2;
  kmeans_kernel<MODE><<<(unsigned)nblk, KM_THREADS, (size_t)p.bytes, s>>>(a, p);
  HAR_CHECK_LAUNCH();
  return 0;
}

// One workgroup.  Not converged at entry: centres from the integer sums (an empty cluster keeps its
// centre), h, moved = max_k ||C_new[k] - C[k]||^2 (fp64, explicitly rounded, features in order), the
// iteration counter, the cost history and the converged flag.  Always: the accumulators are zeroed for
// the next assignment.  state = {iterations, converged}.
__global__ __launch_bounds__(256) void kmeans_update_kernel(KMeansUpdateArgs a) {
  __shared__ double red[256];
  __shared__ double cost_s;
  const int tid = (int)threadIdx.x, K = a.K, D = a.D;
  const int nacc = K * (D + 2);
  const bool live = a.state[1] == 0 && a.state[0] < a.max_iter;  // (read before anyone writes: one workgroup)
  const long long* sums = reinterpret_cast<const long long*>(a.acc);
  const long long* counts = sums + (int64_t)K * D;
  if (live) {
    for (int j = tid; j < K * D; j += 256) {
      const int k = j / D, f = j - k * D;
      const long long c = counts[k];
      float v = a.C[j];
      if (c > 0) v = (float)__ddiv_rn(__dmul_rn((double)sums[j], __ddiv_rn(1.0, (double)a.scale[f])), (double)c);
      a.Cnew[j] = v;
    }
  }
  {
    // the cost in a fixed order: thread t sums partials t, t + 256, ... in order, then the halving tree
    double c = 0.0;
    if (live)
      for (int j = tid; j < a.ncost; j += 256) c = __dadd_rn(c, a.cost[j]);
    red[tid] = c;
    __syncthreads();  // (also orders the workgroup's own global writes of Cnew before the reads below)
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] = __dadd_rn(red[tid], red[tid + o]);
      __syncthreads();
    }
    if (tid == 0) cost_s = red[0];
    __syncthreads();
  }
  double mv = 0.0;
  if (live) {
    for (int k = tid; k < K; k += 256) {
      double m2 = 0.0, h2 = 0.0;
      for (int f = 0; f < D; ++f) {
        const double cn = (double)a.Cnew[(int64_t)k * D + f];
        const double d = __dadd_rn(cn, -(double)a.C[(int64_t)k * D + f]);
        m2 = __dadd_rn(m2, __dmul_rn(d, d));
        h2 = __dadd_rn(h2, __dmul_rn(cn, cn));
      }
      a.h[k] = (float)__dmul_rn(0.5, h2);
      if (a.sizes) a.sizes[k] = counts[k];
      mv = fmax(mv, m2);
    }
  }
  red[tid] = mv;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  if (live) {
    for (int j = tid; j < K * D; j += 256) a.C[j] = a.Cnew[j];
    if (tid == 0) {
      const int it = a.state[0];
      a.cost_hist[it] = cost_s;
      a.state[0] = it + 1;
      a.state[1] = red[0] <= a.tol2 ? 1 : 0;
      if (a.moved) *a.moved = red[0];
    }
  }
  for (int j = tid; j < nacc; j += 256) a.acc[j] = 0;
}

bool km_args_ok(const KMeansArgs& a) {
  return a.X && a.N >= 0 && a.N <= ((int64_t)1 << 31) - KM_CHUNK && a.D >= 1 && a.D <= KM_MAXD && a.K >= 1 &&
         a.K <= KM_MAXK;
}

}  // namespace

extern "C" int har_kmeans_rows_per_block() { return KM_CHUNK; }
extern "C" int har_kmeans_max_k() { return KM_MAXK; }
extern "C" int har_kmeans_max_d() { return KM_MAXD; }

extern "C" int har_kmeans_plan(int D, int K, int* out4) {
  KmPlan p;
  if (!out4) return -4;
  if (!km_plan(D, K, true, p)) return -2;
  out4[0] = p.kt;
  out4[1] = p.npass;
  out4[2] = p.lds_acc;
  out4[3] = (int)p.bytes;
  return 0;
}

extern "C" int har_kmeans_assign(const KMeansArgs* args, hipStream_t s) {
  if (!args) return -4;
  const KMeansArgs& a = *args;
  if (!km_args_ok(a)) return -2;
  if (a.labels) {
    if (a.assign || a.d2 || a.part || !a.acc) return -2;  // given labels: accumulation only
  } else if (!a.C || !a.h) {
    return -4;
  }
  if (a.acc && (!a.scale || !a.norm_scale)) return -4;
  KmPlan p;
  if (!km_plan(a.D, a.K, a.acc != nullptr, p)) return -2;
  if (a.N == 0) return 0;
  return km_launch<MODE_ASSIGN>(a, p, s);
}

extern "C" int har_kmeans_silhouette(const KMeansArgs* args, hipStream_t s) {
  if (!args) return -4;
  const KMeansArgs& a = *args;
  if (!km_args_ok(a)) return -2;
  if (!a.C || !a.h || !a.labels || !a.cnt || (!a.part && !a.sil)) return -4;
  KmPlan p;
  if (!km_plan(a.D, a.K, false, p)) return -2;
  if (a.N == 0) return 0;
  return km_launch<MODE_SIL>(a, p, s);
}

extern "C" int har_kmeans_update(const KMeansUpdateArgs* args, hipStream_t s) {
  if (!args) return -4;
  const KMeansUpdateArgs& a = *args;
  if (a.K < 1 || a.K > KM_MAXK || a.D < 1 || a.D > KM_MAXD || a.ncost < 0 || a.max_iter < 1) return -2;
  if (!a.acc || !a.scale || !a.C || !a.Cnew || !a.h || !a.state || !a.cost_hist || (a.ncost && !a.cost)) return -4;
  kmeans_update_kernel<<<1, 256, 0, s>>>(a);
  HAR_CHECK_LAUNCH();
  return 0;
}
