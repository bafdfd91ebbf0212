// IIR filtering of raw [S][A] fp32 streams by cascaded second-order sections (har/ops/sosfilt.py holds the
// definition): a chunked scan of the affine maps z -> M^n z + u over fixed global chunks of L samples.
//
// A recursive filter is a linear recurrence in its 2 x sections states z.  Time is cut into chunks of L samples
// in SCAN order (tau = t, or S - 1 - t with `reverse`: an index mapping, never a copy of the stream), one lane
// per (chunk, axis):
//
//   0. chunk state   every lane runs its chunk from a zero state in fp64 and stores the chunk's final state u,
//                    plus a reset flag when a segment starts inside the chunk: from the last such start on the
//                    state is absolute (set from x[start] or to zero), so the incoming carry is discarded
//   1. carry scan    the incoming state of every chunk: a grouped prefix scan over the maps
//                    z -> (reset ? 0 : P z) + u.  Inside a group of level l the transition is the constant
//                    P_l = M^(L G^l): the host hands over P_l, P_l^2, ..., P_l^G in fp64.  Up: one lane per
//                    (group, axis) leaves every element's exclusive prefix in place and the group's total one
//                    level up; down: one lane per (element, axis) adds P_l^k times its group's incoming state
//   2. apply         every lane runs its chunk again from its incoming state and writes y as fp32 — or, in the
//                    same pass, [x - y | y] into an [S][2A] output, or x - y alone
//
// Separate launches order the phases; no kernel waits on another workgroup.  No atomics, no device -> host read,
// every output element has exactly one writer: two runs give the same bits.  Only the last element of a level
// can be short (fewer samples, fewer chunks) and its map is never anyone's predecessor, so the constant
// transitions hold everywhere they are used.
//
// Memory access.  The stream is sample-major and axis-interleaved while a lane walks L consecutive samples of
// one axis, so a workgroup stages the contiguous span of its chunks through LDS: 16-byte global loads and
// stores (scalar for the at most 3 + 3 words around an unaligned span), 4-byte LDS accesses.  The LDS image
// keeps the stream's own order — word (sample m, axis a) of chunk q at q * pitch + (m - q L) * A + a — and
// only the chunk pitch is padded, to pitch = A (mod 32).  Lane (q, a) = lane index q A + a then starts at bank
// q * pitch + a = q A + a = its own lane index (mod 32) and all lanes advance by the same A words per step, so
// the 32 lanes of a ds_read_b32 / ds_write_b32 group always sit on 32 different banks.  (A transposed image, lane
// stride L + 1, is conflict free too but needs a division by A per staged word and forbids 16-byte global access
// of whole words; padding every sample would break the 16-byte global transfers as well.)  The [S][2A] output
// of the split mode has an image of its own with the same pitch rule.
// That argument covers the walks only.  The STAGING accesses are not conflict free: a lane moves its 16-byte
// global vector as four 4-byte LDS accesses at words 4 tid + j, a word stride of 4 across the lanes, i.e. a
// 4-way bank conflict on each of them (16 LDS cycles per wave and vector where a 16-byte LDS access would take
// about 13 for a store and 4 for a load).  16-byte LDS accesses need a pitch that is a multiple of 4 words,
// which the bank rule pitch = A (mod 32) excludes for most A.  Counted per lane, staging moves as many LDS
// words as the walk does (L in, L out), so with the conflict it may well take more LDS cycles than the walk;
// its share of a block's time is not measured (PARITY.md gives the phase times only).
//
// Numerics.  States, coefficients and carries are fp64; coefficients and the step-response states travel as
// kernel arguments (scalar registers).  A lane holds its 2 x sections states in registers: 16 VGPRs at four
// sections.  Compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see PARITY.md, "StreamFilter".
#include "common.h"
#include "../har_kernels.h"

#include <climits>

namespace {

constexpr int SOS_BLOCK = 256;
constexpr int SOS_L = 64;            // samples per chunk (default)
constexpr int SOS_G = 32;            // elements per group of the carry scan (default)
constexpr int SOS_MAX_SEC = 4;
constexpr int SOS_MAX_AXES = 9;
constexpr int SOS_MAX_L = 256;
constexpr int SOS_MAX_G = 64;
constexpr int SOS_MAXLV = 32;        // G >= 2: 2^31 chunks take at most 31 levels
constexpr int SOS_LDS_WORDS = 16384; // 64 KiB of dynamic LDS per workgroup
constexpr int64_t SOS_MAX_SAMPLES = ((int64_t)1 << 31) - 256;

struct SosCoef {
  double b0[SOS_MAX_SEC], b1[SOS_MAX_SEC], b2[SOS_MAX_SEC], a1[SOS_MAX_SEC], a2[SOS_MAX_SEC];
  double z1[SOS_MAX_SEC], z2[SOS_MAX_SEC];  // step-response states per unit input
};

// An LDS image of a block's span: cw words per chunk in stream order, chunk q at q * pitch; dq / dr = quotient /
// remainder of the staging loop's stride (4 SOS_BLOCK words) by cw.
struct SosImage {
  int cw, pitch, dq, dr;
};

struct SosChunkArgs {
  const float* x;
  const float* xc;      // complement source (null: x)
  float* y;
  const int64_t* seg;   // [nseg + 1] (null: one segment)
  int64_t S, nseg, C;
  int A, OA, L, cpb, reverse, init_step, mode;
  SosImage in, out;
  int out_off, xc_off;  // LDS word offsets of the output / complement images
  double* state;        // [C][A][2 NS]: phase 0 writes u, phase 2 reads the incoming state
  uint8_t* flag;        // [C]
  SosCoef k;
};

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// scan-order position of the i-th segment start, i in [0, nseg)
__device__ __forceinline__ int64_t sos_start(const SosChunkArgs& p, int64_t i) {
  if (p.seg == nullptr) return 0;
  return p.reverse ? p.S - p.seg[p.nseg - i] : p.seg[i];
}

// Image words [w_lo, w_hi) <-> global words base[off + w] (off + w_lo >= 0; off itself may be negative).
template <bool LOAD>
__device__ __forceinline__ void sos_stage(float* img, const SosImage im, float* base, int64_t off, int w_lo, int w_hi) {
  const int tid = threadIdx.x;
  float* g = base + (off + w_lo);  // first word touched
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) >> 2);
  if (head > w_hi - w_lo) head = w_hi - w_lo;
  const int wv = w_lo + head;
  const int nvec = (w_hi - wv) >> 2;
  const int wt = wv + 4 * nvec;
  if (tid < head + (w_hi - wt)) {  // the unaligned ends, at most 3 + 3 words
    const int w = tid < head ? w_lo + tid : wt + (tid - head);
    const int q = w / im.cw, r = w - q * im.cw;
    if (LOAD) img[q * im.pitch + r] = g[w - w_lo];
    else g[w - w_lo] = img[q * im.pitch + r];
  }
  int w = wv + 4 * tid;
  int q = w / im.cw, r = w - q * im.cw;
  for (int i = tid; i < nvec; i += SOS_BLOCK) {
    float4* gv = reinterpret_cast<float4*>(g + (w - w_lo));
    float e[4];
    if (LOAD) {
      const float4 v = *gv;
      e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
    }
    int qi = q, ri = r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (LOAD) img[qi * im.pitch + ri] = e[j];
      else e[j] = img[qi * im.pitch + ri];
      if (++ri == im.cw) ri = 0, ++qi;
    }
    if (!LOAD) *gv = make_float4(e[0], e[1], e[2], e[3]);
    w += 4 * SOS_BLOCK;
    q += im.dq;
    r += im.dr;
    if (r >= im.cw) r -= im.cw, ++q;
  }
}

// One sample through the cascade (direct form II transposed), the definition's operation order.
template <int NS>
__device__ __forceinline__ double sos_step(const SosCoef& k, double (&s1)[NS], double (&s2)[NS], double x) {
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const double y = k.b0[j] * x + s1[j];
    s1[j] = (k.b1[j] * x - k.a1[j] * y) + s2[j];
    s2[j] = k.b2[j] * x - k.a2[j] * y;
    x = y;
  }
  return x;
}

// Phases 0 and 2.  Block b owns the chunks [b cpb, (b + 1) cpb) in scan order; its image holds their samples in
// STREAM order: image sample m is t = t_base + m.  Lane (q, a) walks image chunk q — forwards that is chunk
// b cpb + q, ascending; reversed it is chunk b cpb + cpb - 1 - q, descending — so the bank argument of the
// header holds in both directions.
template <int NS, bool APPLY>
__global__ __launch_bounds__(SOS_BLOCK) void sos_chunk_kernel(const SosChunkArgs p) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int64_t k0 = (int64_t)blockIdx.x * p.cpb;
  const int span = p.cpb * p.L;
  const int64_t t_base = p.reverse ? p.S - (k0 + p.cpb) * (int64_t)p.L : k0 * (int64_t)p.L;
  const int m_lo = t_base < 0 ? (int)(-t_base) : 0;            // samples before the stream (reversed, last block)
  const int m_hi = (int)min64(span, p.S - t_base);             // samples past the stream (forwards, last block)
  sos_stage<true>(lds, p.in, const_cast<float*>(p.x), t_base * p.A, m_lo * p.A, m_hi * p.A);
  const bool own_comp = APPLY && p.xc != nullptr;
  if (own_comp) sos_stage<true>(lds + p.xc_off, p.in, const_cast<float*>(p.xc), t_base * p.A, m_lo * p.A, m_hi * p.A);
  __syncthreads();
  if (tid < p.cpb * p.A) {
    const int q = tid / p.A, a = tid - q * p.A;
    const int64_t k = p.reverse ? k0 + (p.cpb - 1 - q) : k0 + q;
    if (k < p.C) {
      const int64_t tau0 = k * p.L;
      const int n = (int)min64(p.L, p.S - tau0);
      // the first segment start at or after tau0 (start 0 is 0: chunk 0 always begins with a reset)
      int64_t lo = 0, hi = p.nseg;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sos_start(p, mid) < tau0) lo = mid + 1;
        else hi = mid;
      }
      int64_t si = lo;
      int64_t next = si < p.nseg ? sos_start(p, si) : LLONG_MAX;
      double s1[NS], s2[NS];
      double* st = p.state + (k * p.A + a) * (2 * NS);
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        s1[j] = APPLY ? st[2 * j] : 0.0;
        s2[j] = APPLY ? st[2 * j + 1] : 0.0;
      }
      bool reset = false;
      const float* in = lds + q * p.in.pitch + a;
      const float* cin = own_comp ? in + p.xc_off : in;
      float* outp = lds + p.out_off + q * p.out.pitch + a;
      for (int i = 0; i < n; ++i) {
        const int m = p.reverse ? p.L - 1 - i : i;
        const float xf = in[m * p.A];
        const double x = (double)xf;
        if (tau0 + i == next) {
          reset = true;
#pragma unroll
          for (int j = 0; j < NS; ++j) {
            s1[j] = p.init_step ? p.k.z1[j] * x : 0.0;
            s2[j] = p.init_step ? p.k.z2[j] * x : 0.0;
          }
          ++si;
          next = si < p.nseg ? sos_start(p, si) : LLONG_MAX;
        }
        const double y = sos_step<NS>(p.k, s1, s2, x);
        if (APPLY) {
          const float yf = (float)y;
          if (p.mode == 0) {
            outp[m * p.A] = yf;                       // in place: out_off = 0, out = in
          } else {
            const float body = cin[m * p.A] - yf;
            if (p.mode == 2) {
              outp[m * p.A] = body;                   // in place
            } else {
              outp[m * p.OA] = body;
              outp[m * p.OA + p.A] = yf;
            }
          }
        }
      }
      if (!APPLY) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          st[2 * j] = s1[j];
          st[2 * j + 1] = s2[j];
        }
        if (a == 0) p.flag[k] = reset ? 1 : 0;
      }
    }
  }
  if (APPLY) {
    __syncthreads();
    sos_stage<false>(lds + p.out_off, p.out, p.y, t_base * p.OA, m_lo * p.OA, m_hi * p.OA);
  }
}

// Phase 1 up.  One lane per (group, axis) of a level's n elements: st[c] <- the exclusive prefix of the group's
// maps before c (pf[c] = a reset lies among them), the group's total to st_up / fl_up (null at the top level).
template <int NST>
__global__ __launch_bounds__(SOS_BLOCK) void sos_scan_up_kernel(double* __restrict__ st, const uint8_t* __restrict__ fl,
                                                                uint8_t* __restrict__ pf, int64_t n, int A, int G, int64_t ng,
                                                                const double* __restrict__ P, double* __restrict__ st_up,
                                                                uint8_t* __restrict__ fl_up) {
  __shared__ double sP[NST * NST];
  for (int i = threadIdx.x; i < NST * NST; i += SOS_BLOCK) sP[i] = P[i];
  __syncthreads();
  const int64_t gid = (int64_t)blockIdx.x * SOS_BLOCK + threadIdx.x;
  const int64_t g = gid / A;
  const int a = (int)(gid - g * A);
  if (g >= ng) return;
  const int64_t c0 = g * G, c1 = min64(n, c0 + G);
  double U[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) U[i] = 0.0;
  bool R = false;
  for (int64_t c = c0; c < c1; ++c) {
    double* s = st + (c * A + a) * NST;
    double u[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) u[i] = s[i];
    const bool r = fl[c] != 0;
#pragma unroll
    for (int i = 0; i < NST; ++i) s[i] = U[i];
    if (a == 0) pf[c] = R ? 1 : 0;
    if (r) {
#pragma unroll
      for (int i = 0; i < NST; ++i) U[i] = u[i];
      R = true;
    } else {
      double N[NST];
#pragma unroll
      for (int i = 0; i < NST; ++i) {
        double v = u[i];
#pragma unroll
        for (int j = 0; j < NST; ++j) v += sP[i * NST + j] * U[j];
        N[i] = v;
      }
#pragma unroll
      for (int i = 0; i < NST; ++i) U[i] = N[i];
    }
  }
  if (st_up != nullptr) {
    double* o = st_up + (g * A + a) * NST;
#pragma unroll
    for (int i = 0; i < NST; ++i) o[i] = U[i];
    if (a == 0) fl_up[g] = R ? 1 : 0;
  }
}

// Phase 1 down.  One lane per (element, axis): st[c] <- P^k zin_up[group] + st[c] for the k-th element of its
// group, unless a reset precedes it inside the group.  Pw [G][NST][NST] = P, P^2, ..., P^G; the powers 1 .. G - 1
// sit in LDS at a pitch of NST^2 + 1 doubles, so lanes on different powers read different banks.
template <int NST>
__global__ __launch_bounds__(SOS_BLOCK) void sos_scan_down_kernel(double* __restrict__ st, const uint8_t* __restrict__ pf, int64_t n,
                                                                  int A, int G, const double* __restrict__ Pw,
                                                                  const double* __restrict__ zin_up) {
  extern __shared__ double sPw[];
  constexpr int PP = NST * NST + 1;
  for (int i = threadIdx.x; i < (G - 1) * NST * NST; i += SOS_BLOCK) {
    const int k = i / (NST * NST);
    sPw[k * PP + (i - k * NST * NST)] = Pw[i];
  }
  __syncthreads();
  const int64_t gid = (int64_t)blockIdx.x * SOS_BLOCK + threadIdx.x;
  const int64_t c = gid / A;
  const int a = (int)(gid - c * A);
  if (c >= n) return;
  const int64_t g = c / G;
  const int k = (int)(c - g * G);
  if (pf[c]) return;  // absolute already
  const double* zg = zin_up + (g * A + a) * NST;
  double* s = st + (c * A + a) * NST;
  double z[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) z[i] = zg[i];
  if (k == 0) {  // the group's first element: the incoming state itself (its prefix is zero)
#pragma unroll
    for (int i = 0; i < NST; ++i) s[i] = z[i];
    return;
  }
  const double* Pk = sPw + (k - 1) * PP;
#pragma unroll
  for (int i = 0; i < NST; ++i) {
    double v = s[i];
#pragma unroll
    for (int j = 0; j < NST; ++j) v += Pk[i * NST + j] * z[j];
    s[i] = v;
  }
}

inline unsigned sos_blocks(int64_t threads) { return (unsigned)((threads + SOS_BLOCK - 1) / SOS_BLOCK); }
inline size_t sos_align(size_t x) { return (x + 255) & ~(size_t)255; }

// The workspace: per level l the states [n_l][A][2 ns] fp64, the reset flags [n_l] and the prefix flags [n_l].
struct SosPlan {
  int nlv = 0;
  int64_t n[SOS_MAXLV] = {};
  size_t st[SOS_MAXLV] = {}, fl[SOS_MAXLV] = {}, pf[SOS_MAXLV] = {};
  size_t bytes = 0;
  bool ok = false;
};

SosPlan sos_plan(int64_t S, int A, int ns, int L, int G) {
  SosPlan p;
  if (S < 1 || S >= SOS_MAX_SAMPLES || A < 1 || A > SOS_MAX_AXES || ns < 1 || ns > SOS_MAX_SEC || L < 1 || L > SOS_MAX_L ||
      G < 2 || G > SOS_MAX_G)
    return p;
  p.n[0] = (S + L - 1) / L;
  p.nlv = 1;
  while (p.n[p.nlv - 1] > G) {
    if (p.nlv == SOS_MAXLV) return p;
    p.n[p.nlv] = (p.n[p.nlv - 1] + G - 1) / G;
    ++p.nlv;
  }
  size_t o = 0;
  for (int l = 0; l < p.nlv; ++l) {
    p.st[l] = o;
    o += sos_align((size_t)p.n[l] * A * 2 * ns * sizeof(double));
    p.fl[l] = o;
    o += sos_align((size_t)p.n[l]);
    p.pf[l] = o;
    o += sos_align((size_t)p.n[l]);
  }
  p.bytes = o;
  p.ok = true;
  return p;
}

SosImage sos_image(int words_per_sample, int L, int A) {
  SosImage im;
  im.cw = words_per_sample * L;
  im.pitch = im.cw + (((A - im.cw) % 32) + 32) % 32;  // pitch = A (mod 32)
  im.dq = (4 * SOS_BLOCK) / im.cw;
  im.dr = (4 * SOS_BLOCK) % im.cw;
  return im;
}

template <int NS>
int sos_run(const SosPlan& pl, const SosFilterArgs& a, hipStream_t s) {
  uint8_t* ws = static_cast<uint8_t*>(a.ws);
  auto st = [&](int l) { return reinterpret_cast<double*>(ws + pl.st[l]); };
  auto fl = [&](int l) { return ws + pl.fl[l]; };
  auto pf = [&](int l) { return ws + pl.pf[l]; };
  constexpr int NST = 2 * NS;
  const int A = a.axes, L = a.L, G = a.G;
  const int64_t C = pl.n[0];
  auto on = [&](int ph) { return a.phase_lo <= ph && ph <= a.phase_hi; };

  SosChunkArgs k;
  k.x = a.x, k.xc = a.xc, k.y = a.y, k.seg = a.n_seg > 1 ? a.seg : nullptr;
  k.S = a.n_samples, k.nseg = a.n_seg, k.C = C;
  k.A = A, k.OA = a.mode == 1 ? 2 * A : A, k.L = L;
  k.reverse = a.reverse, k.init_step = a.init_step, k.mode = a.mode;
  k.in = sos_image(A, L, A);
  k.state = st(0), k.flag = fl(0);
  for (int j = 0; j < SOS_MAX_SEC; ++j) {
    const bool in = j < NS;
    k.k.b0[j] = in ? a.sos[j][0] : 0.0, k.k.b1[j] = in ? a.sos[j][1] : 0.0, k.k.b2[j] = in ? a.sos[j][2] : 0.0;
    k.k.a1[j] = in ? a.sos[j][3] : 0.0, k.k.a2[j] = in ? a.sos[j][4] : 0.0;
    k.k.z1[j] = in ? a.zi[j][0] : 0.0, k.k.z2[j] = in ? a.zi[j][1] : 0.0;
  }
  const int lanes_max = SOS_BLOCK / A;
  if (on(0)) {
    SosChunkArgs p = k;
    p.xc = nullptr, p.mode = 0, p.OA = A;
    p.out = p.in, p.out_off = 0, p.xc_off = 0;
    int cpb = SOS_LDS_WORDS / p.in.pitch;
    if (cpb > lanes_max) cpb = lanes_max;
    if ((int64_t)cpb > C) cpb = (int)C;
    if (cpb < 1) return -2;
    p.cpb = cpb;
    sos_chunk_kernel<NS, false><<<(unsigned)((C + cpb - 1) / cpb), SOS_BLOCK, (size_t)cpb * p.in.pitch * sizeof(float), s>>>(p);
    HAR_CHECK_LAUNCH();
  }
  if (on(1)) {
    const int top = pl.nlv - 1;
    const double* pw = a.powers;
    const size_t lvl = (size_t)G * NST * NST;
    for (int l = 0; l <= top; ++l) {
      const int64_t ng = l < top ? pl.n[l + 1] : 1;
      sos_scan_up_kernel<NST><<<sos_blocks(ng * A), SOS_BLOCK, 0, s>>>(st(l), fl(l), pf(l), pl.n[l], A, G, ng, pw + l * lvl,
                                                                        l < top ? st(l + 1) : nullptr,
                                                                        l < top ? fl(l + 1) : nullptr);
      HAR_CHECK_LAUNCH();
    }
    for (int l = top - 1; l >= 0; --l) {
      sos_scan_down_kernel<NST><<<sos_blocks(pl.n[l] * A), SOS_BLOCK, (size_t)(G - 1) * (NST * NST + 1) * sizeof(double), s>>>(
          st(l), pf(l), pl.n[l], A, G, pw + l * lvl, st(l + 1));
      HAR_CHECK_LAUNCH();
    }
  }
  if (on(2)) {
    SosChunkArgs p = k;
    int per_chunk = p.in.pitch;
    p.out = p.in, p.out_off = 0, p.xc_off = 0;
    if (p.xc != nullptr) per_chunk += p.in.pitch;
    if (p.mode == 1) {
      p.out = sos_image(2 * A, L, A);
      per_chunk += p.out.pitch;
    }
    int cpb = SOS_LDS_WORDS / per_chunk;
    if (cpb > lanes_max) cpb = lanes_max;
    if ((int64_t)cpb > C) cpb = (int)C;
    if (cpb < 1) return -2;
    p.cpb = cpb;
    int o = cpb * p.in.pitch;
    if (p.xc != nullptr) p.xc_off = o, o += cpb * p.in.pitch;
    if (p.mode == 1) p.out_off = o, o += cpb * p.out.pitch;
    sos_chunk_kernel<NS, true><<<(unsigned)((C + cpb - 1) / cpb), SOS_BLOCK, (size_t)o * sizeof(float), s>>>(p);
    HAR_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int har_sosfilt_chunk_len() { return SOS_L; }
extern "C" int har_sosfilt_scan_group() { return SOS_G; }

extern "C" int har_sosfilt_levels(int64_t n_samples, int L, int G) {
  const SosPlan p = sos_plan(n_samples, 1, 1, L, G);
  return p.ok ? p.nlv : -1;
}

extern "C" int64_t har_sosfilt_workspace_bytes(int64_t n_samples, int axes, int sections, int L, int G) {
  const SosPlan p = sos_plan(n_samples, axes, sections, L, G);
  return p.ok ? (int64_t)p.bytes : -1;
}

extern "C" int har_sosfilt(const SosFilterArgs* a, hipStream_t s) {
  if (a == nullptr) return -4;
  if (a->n_samples == 0) return 0;
  const SosPlan p = sos_plan(a->n_samples, a->axes, a->sections, a->L, a->G);
  if (!p.ok || a->ws_bytes < (int64_t)p.bytes || a->levels != p.nlv || a->n_seg < 1 || a->n_seg > a->n_samples ||
      a->mode < 0 || a->mode > 2 || (a->xc != nullptr && a->mode == 0))
    return -2;
  if (a->x == nullptr || a->y == nullptr || a->ws == nullptr || a->powers == nullptr || (a->n_seg > 1 && a->seg == nullptr))
    return -4;
  switch (a->sections) {
    case 1: return sos_run<1>(p, *a, s);
    case 2: return sos_run<2>(p, *a, s);
    case 3: return sos_run<3>(p, *a, s);
    default: return sos_run<4>(p, *a, s);
  }
}
