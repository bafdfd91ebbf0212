// Exact k-nearest neighbours: a queries-by-references product on the exact-fp32 matrix cores fused
// with a running top-k, so the N x M scores never reach global memory; then a merge + vote kernel.
//
// Definitions (har/ops/knn.py states them once more as PyTorch code; the kernels compare to it):
//   * working rows Q [N][D], R [M][D] fp32 (centred / standardised by the caller), h[m] = ||R[m]||^2 / 2.
//   * score s[n][m] = h[m] - <Q[n], R[m]>.  The neighbours of row n are the k smallest PAIRS (s, m) in
//     lexicographic order (ties: the lower reference index), ascending.  A pair is skipped when
//     qgroup[n] >= 0 and qgroup[n] == rgroup[m].  Missing entries: index -1, score / d2 = +inf.
//   * d2 = float(max(0, nrm[n] + 2 s)) in fp64, nrm as in kmeans.hip: (p0 + p1) + (p2 + p3), p_j the
//     in-order fp64 sum of Q[n][f]^2 over f = j, j + 4, ...
//   * vote: class weight c[j] = the in-order sum of w_i over the valid neighbours of class j; uniform
//     w = 1; distance w = 1 / sqrt(d2) in fp64, and when some valid neighbour has d2 == 0 those get 1 and
//     the others 0.  probability = c / sum_j c (1 / C without a valid neighbour), prediction = first argmax.
//
// knn_search, grid (query blocks, reference splits).  Four waves own KN_QROWS = 64 query rows, 16 per
// wave; the wave's A operand of v_mfma_f32_16x16x4_f32 (lane (col, q) holds Q[row col][4 i + q]) stays in
// NQ registers for the whole sweep.  NQ is the smallest of a few compiled sizes that covers D / 4: the
// zero padding adds exact zeros to the end of the chain.  Reference rows stream through LDS in
// double-buffered slabs with kmeans.hip's row stride (4 NQ + 2 floats), padding rows carry h = +inf.
// A score is ONE chain of NQ MFMAs from a zero accumulator over d ascending, whatever tile, slab, split
// or batch the pair sits in: the same bits everywhere, which is what makes the result independent of
// the split and of the query batching.  On the C layout (col = lane & 15 = reference, row = 4 (lane >> 4) +
// reg) every lane holds the current k-th pair of its four rows in registers; a candidate that does not
// beat it is dropped by one compare, the others are inserted one at a time by the whole wave into the
// row's sorted list in LDS (lane j owns entry j; k <= 64).  The total order on pairs makes the list
// independent of the insertion order.
#include <limits.h>
#include <math.h>

#include <type_traits>

#include "common.h"
#include "../har_kernels.h"

namespace {

constexpr int KN_THREADS = 256;
constexpr int KN_QROWS = 64;   // query rows per workgroup
constexpr int KN_MAXK = 64, KN_MAXD = 256, KN_MAXC = 32;
constexpr int KN_NCT = 4;      // reference tiles per sweep
constexpr int KN_MAXSLAB = 128;
constexpr int KN_MAXSPLITS = 1024;
constexpr int64_t KN_MAXROWS = ((int64_t)1 << 31) - 256;
constexpr int64_t KN_LDS_MAX = 160 * 1024;
constexpr int64_t KN_LIST_BYTES = (int64_t)KN_QROWS * KN_MAXK * 8;

// compiled A-fragment sizes (registers per lane); D / 4 rounds up to the next one
constexpr int KN_NQ[] = {1, 2, 4, 8, 11, 16, 24, 32, 43, 48, 64};

int kn_nq(int D) {
  const int need = (D + 3) / 4;
  for (int v : KN_NQ)
    if (v >= need) return v;
  return 0;
}

// reference rows per slab: two buffers of (row, h, group) beside the lists of the largest k; a shape of a
// few dozen features keeps two or three workgroups on a CU
int kn_slab(int D) {
  const int nq = kn_nq(D);
  if (!nq) return 0;
  const int ld = 4 * nq + 2;
  int slab = (int)((KN_LDS_MAX - KN_LIST_BYTES) / ((int64_t)2 * (ld + 2) * 4));
  slab &= ~15;
  return slab > KN_MAXSLAB ? KN_MAXSLAB : slab;
}

struct KnPlan {
  int slab, splits;
  int64_t nslabs, bytes;
};

// entry (es, ei) precedes the candidate (cs, cm) in the (score, index) order
__device__ __forceinline__ bool kn_before(float es, int ei, float cs, int cm) {
  return es < cs || (es == cs && ei < cm);
}

// The whole wave inserts the pair (cs, cm) into a sorted list of k entries, lane j holding entry j (lanes
// >= k: +inf, -1).  Returns false when the pair is not among the k smallest (nothing changes).
__device__ __forceinline__ bool kn_insert(float& es, int& ei, float cs, int cm, int k, int lane, int& pos) {
  pos = __popcll(__ballot(lane < k && kn_before(es, ei, cs, cm)));  // the list is sorted: a prefix
  if (pos >= k) return false;
  const float us = __shfl_up(es, 1, 64);
  const int ui = __shfl_up(ei, 1, 64);
  if (lane < k && lane >= pos) {
    es = lane == pos ? cs : us;
    ei = lane == pos ? cm : ui;
  }
  return true;
}

template <int NQ>
__global__ __launch_bounds__(KN_THREADS) void knn_search_kernel(KnnSearchArgs a, KnPlan p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kn_lds[];
  constexpr int ld = 4 * NQ + 2;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  const int D = a.D, k = a.k, slab = p.slab;
  // LDS image: [ls float 64 k][li int 64 k][hs float 2 slab][gs int 2 slab][rs float 2 slab ld]
  float* const ls = reinterpret_cast<float*>(kn_lds) + 16 * wave * k;  // the wave's 16 lists
  int* const li = reinterpret_cast<int*>(kn_lds) + KN_QROWS * k + 16 * wave * k;
  float* const hs = reinterpret_cast<float*>(kn_lds) + 2 * KN_QROWS * k;
  int* const gs = reinterpret_cast<int*>(hs + 2 * slab);
  float* const rs = reinterpret_cast<float*>(gs + 2 * slab);
  const int64_t row0 = (int64_t)blockIdx.x * KN_QROWS + 16 * wave;

  float av[NQ];
  {
    const int64_t n = row0 + col;
    const bool ok = n < a.N;
    const float* src = a.Q + (ok ? n : 0) * D;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int f = 4 * i + q;
      av[i] = ok && f < D ? src[f] : 0.f;
    }
  }
  // the rows 4 q + g of this lane on the C layout: group, and the current k-th pair (a row past N: -inf,
  // nothing enters)
  int qg[4], tm[4];
  float ts[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int64_t n = row0 + 4 * q + g;
    const bool ok = n < a.N;
    qg[g] = ok && a.qgroup ? a.qgroup[n] : -1;
    ts[g] = ok ? INFINITY : -INFINITY;
    tm[g] = INT_MAX;
  }
  for (int e = lane; e < 16 * k; e += 64) {
    ls[e] = INFINITY;
    li[e] = -1;
  }

  auto stage = [&](int64_t sl, int b) {
    const int64_t m0 = sl * slab;
    float* dst = rs + (int64_t)b * slab * ld;
    for (int kl = wave; kl < slab; kl += 4) {
      const int64_t m = m0 + kl;
      const bool ok = m < a.M;
      const float* src = a.R + (ok ? m : 0) * D;
      for (int f = lane; f < ld; f += 64) dst[kl * ld + f] = ok && f < D ? src[f] : 0.f;
      if (lane == 0) {
        hs[b * slab + kl] = ok ? a.h[m] : INFINITY;
        gs[b * slab + kl] = ok && a.rgroup ? a.rgroup[m] : -1;
      }
    }
  };

  // split t takes the slabs [t nslabs / splits, (t + 1) nslabs / splits): at least one each
  const int64_t s0 = (int64_t)blockIdx.y * p.nslabs / p.splits, s1 = (int64_t)(blockIdx.y + 1) * p.nslabs / p.splits;
  stage(s0, 0);
  for (int64_t sl = s0; sl < s1; ++sl) {
    const int b = (int)((sl - s0) & 1);
    __syncthreads();  // slab sl is staged; every wave is done with the buffer the next one goes to
    if (sl + 1 < s1) stage(sl + 1, b ^ 1);
    const int64_t m0 = sl * slab;
    const int ktiles = (int)(min<int64_t>(slab, ((a.M - m0) + 15) & ~(int64_t)15) >> 4);
    const float* cb = rs + (int64_t)b * slab * ld + col * ld + q;
    const float* hb = hs + b * slab;
    const int* gb = gs + b * slab;

    auto sweep = [&](auto nt_c, int ct0) {
      constexpr int NT = decltype(nt_c)::value;
      f32x4_t acc[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u) acc[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const float* c0 = cb + 16 * ct0 * ld;
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
#pragma unroll
        for (int u = 0; u < NT; ++u)
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], c0[u * 16 * ld + 4 * i], acc[u], 0, 0, 0);
      }
      float sv[NT][4];
      bool any = false;
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        const int kl = 16 * (ct0 + u) + col;
        const float hv = hb[kl];
        const int rg = gb[kl];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float s = hv - acc[u][g];
          s = (qg[g] >= 0 && qg[g] == rg) ? INFINITY : s;
          sv[u][g] = s;
          any |= s <= ts[g] && s < INFINITY;
        }
      }
      if (__ballot(any) == 0) return;  // the common case once the lists are warm
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        const int m = (int)(m0 + 16 * (ct0 + u) + col);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float s = sv[u][g];
          bool want = s < INFINITY && kn_before(s, m, ts[g], tm[g]);
          unsigned long long mask;
          while ((mask = __ballot(want)) != 0ull) {
            const int src = __ffsll((long long)mask) - 1;
            const float cs = __shfl(s, src, 64);
            const int cm = __shfl(m, src, 64);
            const int r = 4 * (src >> 4) + g;  // the wave's row
            float es = INFINITY;
            int ei = -1;
            if (lane < k) {
              es = ls[r * k + lane];
              ei = li[r * k + lane];
            }
            int pos;
            if (kn_insert(es, ei, cs, cm, k, lane, pos) && lane < k && lane >= pos) {
              ls[r * k + lane] = es;
              li[r * k + lane] = ei;
            }
            __builtin_amdgcn_wave_barrier();
            const float nts = __shfl(es, k - 1, 64);
            const int ntm = __shfl(ei, k - 1, 64);
            if (q == (src >> 4)) {
              ts[g] = nts;
              tm[g] = ntm;
            }
            want = lane != src && want && kn_before(s, m, ts[g], tm[g]);
          }
        }
      }
    };
    for (int ct0 = 0; ct0 < ktiles; ct0 += KN_NCT) {
      const int ntl = min(KN_NCT, ktiles - ct0);
      if (ntl == 4) sweep(std::integral_constant<int, 4>{}, ct0);
      else if (ntl == 3) sweep(std::integral_constant<int, 3>{}, ct0);
      else if (ntl == 2) sweep(std::integral_constant<int, 2>{}, ct0);
      else sweep(std::integral_constant<int, 1>{}, ct0);
    }
  }

  // the wave's sorted partial lists
  __builtin_amdgcn_wave_barrier();
  if (lane < k) {
    for (int r = 0; r < 16; ++r) {
      const int64_t n = row0 + r;
      if (n >= a.N) break;
      const int64_t o = ((int64_t)blockIdx.y * a.N + n) * k + lane;
      a.ps[o] = ls[r * k + lane];
      a.pi[o] = li[r * k + lane];
    }
  }
}

template <int NQ>
int kn_launch(const KnnSearchArgs& a, const KnPlan& p, hipStream_t s) {
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_search_kernel<NQ>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)KN_LDS_MAX) == hipSuccess;
  }();
  if (!attr) return -4;
  const dim3 grid((unsigned)((a.N + KN_QROWS - 1) / KN_QROWS), (unsigned)p.splits);
  knn_search_kernel<NQ><<<grid, KN_THREADS, (size_t)p.bytes, s>>>(a, p);
  HAR_CHECK_LAUNCH();
  return 0;
}

// A wave per query row, lane j = list entry j.  With partial lists (ps): the k smallest pairs of the
// splits' lists (split 0 is the start, the others are inserted in order; a sorted partial list is left
// at its first entry that does not enter), then idx and d2.  Without: idx and d2 are read ([N][ldk], the
// first k of every row).  With labels: the vote.
__global__ __launch_bounds__(KN_THREADS) void knn_vote_kernel(KnnVoteArgs a) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * 4 + wave;
  if (n >= a.N) return;  // (no workgroup barrier below)
  const int k = a.k;
  int ei = -1;
  float d2 = INFINITY;
  if (a.ps) {
    float es = INFINITY;
    if (lane < k) {
      es = a.ps[n * k + lane];
      ei = a.pi[n * k + lane];
    }
    for (int t = 1; t < a.splits; ++t) {
      const float* ps = a.ps + ((int64_t)t * a.N + n) * k;
      const int* pi = a.pi + ((int64_t)t * a.N + n) * k;
      for (int j = 0; j < k; ++j) {
        const int cm = pi[j];
        int pos;
        if (cm < 0 || !kn_insert(es, ei, ps[j], cm, k, lane, pos)) break;  // (wave-uniform)
      }
    }
    double pn = 0.0;
    if (lane < 4) {
      const float* src = a.Q + n * a.D;
      for (int f = lane; f < a.D; f += 4) {
        const double x = (double)src[f];
        pn = fma(x, x, pn);
      }
    }
    pn += __shfl_xor(pn, 1, 64);  // p0 + p1 | p2 + p3
    pn += __shfl_xor(pn, 2, 64);  // (p0 + p1) + (p2 + p3)
    const double nrm = __shfl(pn, 0, 64);
    if (ei >= 0) d2 = (float)fmax(0.0, nrm + 2.0 * (double)es);
    if (lane < k) {
      a.idx[n * a.ldk + lane] = ei;
      a.d2[n * a.ldk + lane] = d2;
    }
  } else if (lane < k) {
    ei = a.idx[n * a.ldk + lane];
    d2 = a.d2[n * a.ldk + lane];
  }
  if (!a.y) return;

  const int C = a.C;
  const bool valid = lane < k && ei >= 0 && (int64_t)ei < a.M;
  const int cls = valid ? a.y[ei] : -1;
  double w = valid ? 1.0 : 0.0;
  if (a.weights == 1) {
    const bool zero = valid && d2 == 0.f;
    if (__ballot(zero) != 0ull) w = zero ? 1.0 : 0.0;
    else if (valid) w = __ddiv_rn(1.0, __dsqrt_rn((double)d2));
  }
  double c = 0.0;  // lane j < C: class j
  for (int i = 0; i < k; ++i) {
    const double wi = __shfl(w, i, 64);
    const int ci = __shfl(cls, i, 64);
    if (ci == lane) c = __dadd_rn(c, wi);
  }
  double tot = 0.0, best = -1.0;
  int bi = 0;
  for (int j = 0; j < C; ++j) {
    const double cj = __shfl(c, j, 64);
    tot = __dadd_rn(tot, cj);
    if (cj > best) {  // strict: the first maximum
      best = cj;
      bi = j;
    }
  }
  if (lane < C) {
    if (a.raw) a.raw[n * C + lane] = c;
    if (a.prob) a.prob[n * C + lane] = tot > 0.0 ? __ddiv_rn(c, tot) : __ddiv_rn(1.0, (double)C);
  }
  if (lane == 0 && a.pred) a.pred[n] = bi;
}

}  // namespace

extern "C" int har_knn_query_rows() { return KN_QROWS; }
extern "C" int har_knn_max_k() { return KN_MAXK; }
extern "C" int har_knn_max_d() { return KN_MAXD; }
extern "C" int har_knn_max_classes() { return KN_MAXC; }
extern "C" int har_knn_max_splits() { return KN_MAXSPLITS; }
extern "C" int har_knn_slab_rows(int D) { return D >= 1 && D <= KN_MAXD ? kn_slab(D) : -2; }

extern "C" int har_knn_auto_splits(int64_t N, int64_t M, int D) {
  if (N < 1 || M < 1 || D < 1 || D > KN_MAXD) return -2;
  const int64_t slab = kn_slab(D), nslabs = (M + slab - 1) / slab, qb = (N + KN_QROWS - 1) / KN_QROWS;
  // two workgroups' worth per CU of the 256: small query counts split the references instead
  int64_t s = (512 + qb - 1) / qb;
  s = s < nslabs ? s : nslabs;
  s = s < KN_MAXSPLITS ? s : KN_MAXSPLITS;
  return (int)(s < 1 ? 1 : s);
}

extern "C" int har_knn_search(const KnnSearchArgs* args, hipStream_t s) {
  if (!args) return -4;
  const KnnSearchArgs& a = *args;
  if (a.N < 0 || a.N > KN_MAXROWS || a.M < 1 || a.M > KN_MAXROWS || a.D < 1 || a.D > KN_MAXD || a.k < 1 ||
      a.k > KN_MAXK)
    return -2;
  if (!a.Q || !a.R || !a.h || !a.ps || !a.pi) return -4;
  KnPlan p;
  p.slab = kn_slab(a.D);
  p.nslabs = (a.M + p.slab - 1) / p.slab;
  p.splits = a.splits;
  if (p.splits < 1 || p.splits > KN_MAXSPLITS || p.splits > p.nslabs) return -2;
  const int nq = kn_nq(a.D), ld = 4 * nq + 2;
  p.bytes = (int64_t)KN_QROWS * a.k * 8 + (int64_t)2 * p.slab * (ld + 2) * 4;
  if (p.bytes > KN_LDS_MAX) return -2;
  if (a.N == 0) return 0;
  switch (nq) {
    case 1: return kn_launch<1>(a, p, s);
    case 2: return kn_launch<2>(a, p, s);
    case 4: return kn_launch<4>(a, p, s);
    case 8: return kn_launch<8>(a, p, s);
    case 11: return kn_launch<11>(a, p, s);
    case 16: return kn_launch<16>(a, p, s);
    case 24: return kn_launch<24>(a, p, s);
    case 32: return kn_launch<32>(a, p, s);
    case 43: return kn_launch<43>(a, p, s);
    case 48: return kn_launch<48>(a, p, s);
    case 64: return kn_launch<64>(a, p, s);
  }
  return -2;
}

extern "C" int har_knn_merge_vote(const KnnVoteArgs* args, hipStream_t s) {
  if (!args) return -4;
  const KnnVoteArgs& a = *args;
  if (a.N < 0 || a.N > KN_MAXROWS || a.k < 1 || a.k > KN_MAXK || a.ldk < a.k) return -2;
  if (!a.idx || !a.d2) return -4;
  if (a.ps) {
    if (a.splits < 1 || a.splits > KN_MAXSPLITS || a.D < 1 || a.D > KN_MAXD) return -2;
    if (!a.pi || !a.Q) return -4;
  }
  if (a.y) {
    if (a.C < 1 || a.C > KN_MAXC || a.M < 1 || a.M > KN_MAXROWS || a.weights < 0 || a.weights > 1) return -2;
    if (!a.raw && !a.prob && !a.pred) return -4;
  } else if (!a.ps) {
    return -2;  // nothing to do
  }
  if (a.N == 0) return 0;
  knn_vote_kernel<<<(unsigned)((a.N + 3) / 4), KN_THREADS, 0, s>>>(a);
  HAR_CHECK_LAUNCH();
  return 0;
}
