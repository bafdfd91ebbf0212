// Spectral window features over raw IMU streams: the real DFT of every (window, axis)
// as an exact-fp32 GEMM on the matrix cores, with the whole feature epilogue fused behind it — the
// spectrum never goes to memory.
//
// Per window and axis, from the raw samples x[0..W) (no taper), bins k = 1..K, K = W / 2 (DC excluded,
// the Nyquist bin as is):  X_k = sum_n x[n] e^{-2 pi i k n / W},  P_k = |X_k|^2,  f_k = k hz / W.
// Output per axis (11 floats): 8 band fractions (band of bin k: ((k - 1) * 8) / K), the dominant
// frequency (largest P_k, lowest k among equals), the centroid sum f_k P_k / total and the entropy
// -sum p_k ln p_k / ln K.  A constant axis-window (max == min) or total == 0 gives 11 zeros — the rule
// window.hip applies to a constant axis, so rounding noise never becomes a spectrum.
// Row layout for A axes: [A x 8 band fractions][dominant Hz: A][centroid Hz: A][entropy: A].
//
// The GEMM: rows are (window, axis) pairs, the K dimension is the window's samples, the columns are the
// cos / sin twiddles of the bins.
//   * A block owns `wpb` whole windows = wpb * A rows, 16 rows (one MFMA row block) per wave.  It stages
//     the contiguous sample span of its windows in LDS (overlapping windows read each sample once, as in
//     window.hip) next to the twiddle table.
//   * The twiddle table holds W pairs (cos, sin)(2 pi j / W), computed in float64 on the host, rounded
//     once to fp32 and cached on the device per (device, W).  The B operand of bin k at sample n is entry
//     (k n) mod W, kept as a running integer index (+ 4 k mod W per step of 4 samples): no sinf / cosf in
//     the loop, and no angle that loses bits as k n grows.
//   * A wave sweeps the samples once per NBT = 4 bin tiles (16 bins each), with a cos and a sin
//     accumulator tile per bin tile: one A-fragment read from LDS feeds eight v_mfma_f32_16x16x4_f32, and
//     the operands of the next step are read ahead of the current step's MFMAs.  The A fragment is x[n] - x[0] (any pivot leaves the bins k >= 1 unchanged; this one keeps the
//     products small when the signal rides on gravity).  The n >= W tail of W % 4 != 0 is a zero operand,
//     the columns k > K of the last bin tile are dropped in the epilogue.
//   * LDS banks (ds_read_b32: 32 banks, conflicts within a 32-lane half): the 16 lanes of a sample read 16
//     rows `A` or `stride A` floats apart — for 3 axes and stride 200 that is 2-way (windows 0 and 4 of a
//     row block are 2,400 floats = 0 mod 32 apart).  With one A read per eight MFMAs (256 issue cycles)
//     the conflicts do not show; the span is therefore staged unpadded, with 16-byte copies.
//   * Epilogue on the C layout (col = lane & 15 = bin, row = 4 (lane >> 4) + reg): re and im of a bin sit
//     in the same lane and register, so P_k is lane-local.  Every lane keeps running band sums, sum P,
//     sum k P, sum P ln P and (max P, lowest k) for its four rows; ONE 16-lane DPP reduction per row at
//     the end.  P is prescaled by 2 / (W * W var) (Parseval: total ~ 1), so ln(total) - sum P ln P / total
//     of a near-pure tone is a difference of small numbers.  The row's min / max (constant rule) and
//     variance come from the A fragments of the first sweep.
//   * No atomics; every output element is written once by one lane: bitwise reproducible.
#include <cmath>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"
#include "wave_ops.h"
#include "../har_kernels.h"

namespace {

constexpr int MAXA = 9;
constexpr int NBANDS = 8;
constexpr int NFA = NBANDS + 3;       // features per axis
constexpr int MAXW = 2048;            // har_spectral_max_window(): the twiddle table and one 9-axis window fit the LDS
constexpr int NBT = 4;                // bin tiles (of 16 bins) per sweep of the samples
constexpr int64_t LDS_MAX = 160 * 1024;

typedef float v4f __attribute__((ext_vector_type(4)));

// floats of the twiddle table in LDS (W float2, rounded up so the span behind it is 16-byte aligned)
__host__ __device__ constexpr int tab_floats(int W) { return (2 * W + 3) & ~3; }

struct SpecOut {
  float* out;            // fp32 rows (MLP = false)
  uint16_t* outb;        // bf16 rows (MLP = true)
  const float* mean;     // [11 A] (MLP)
  const float* inv_std;  // [11 A] (MLP)
  int ld, col0;
};

// per-lane running statistics of the lane's four C rows (reg = 0..3) over the bins it has seen
struct RowAcc {
  float band[4][NBANDS], sP[4], skP[4], sPl[4], mx[4];
  int mk[4];
};

// x mod W for 0 <= x < 4 W
__device__ __forceinline__ int mod4(int x, int W) {
  x -= x >= 2 * W ? 2 * W : 0;
  return x - (x >= W ? W : 0);
}

template <bool MLP>
__global__ __launch_bounds__(256) void spectral_kernel(const float* __restrict__ stream,
                                                       const float2* __restrict__ tw, int A, int W, int stride,
                                                       int64_t n_windows, float hz, int wpb, SpecOut o) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int nt = (int)blockDim.x, tid = (int)threadIdx.x;
  float2* const tab = reinterpret_cast<float2*>(lds);
  float* const span = lds + tab_floats(W);
  const int64_t w0 = (int64_t)blockIdx.x * wpb;
  const int nwin = (int)min<int64_t>(wpb, n_windows - w0);

  // ---- stage the twiddle table and the span: samples [w0 stride, (w0 + nwin - 1) stride + W), A floats each ----
  for (int i = tid; i < W; i += nt) tab[i] = tw[i];
  {
    const float* src = stream + w0 * stride * A;
    const int nspan = ((nwin - 1) * stride + W) * A;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      const int n4 = nspan >> 2;
      const v4f* s4 = reinterpret_cast<const v4f*>(src);
      v4f* d4 = reinterpret_cast<v4f*>(span);
      // SU unconditional (clamped) 16-byte loads in flight per thread, as window.hip stages its span: one
      // load per trip was one HBM latency per 4 KB of a ~50 KB span (a clamped slot rewrites the last float4)
      constexpr int SU = 8;
      for (int f0 = tid; f0 < n4; f0 += SU * nt) {
        v4f r[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) r[u] = s4[min(f0 + u * nt, n4 - 1)];
#pragma unroll
        for (int u = 0; u < SU; ++u) d4[min(f0 + u * nt, n4 - 1)] = r[u];
      }
      done = n4 * 4;
    }
    for (int e = done + tid; e < nspan; e += nt) span[e] = src[e];
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  const int nrows = nwin * A;
  if (16 * wave >= nrows) return;  // (wave-uniform, after the only barrier)
  const int K = W >> 1, ntiles = (K + 15) >> 4;

  // the A-operand row of this lane: row 16 wave + col of the block = (window, axis); rows past the block's
  // windows compute row 0 again and are never written
  const float* xr;
  {
    const int r = 16 * wave + col, rr = r < nrows ? r : 0, wi = rr / A;
    xr = span + wi * stride * A + (rr - wi * A);
  }
  const float pivot = xr[0];
  float s1 = 0.f, s2 = 0.f, lo = pivot, hi = pivot;

  RowAcc a;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int b = 0; b < NBANDS; ++b) a.band[g][b] = 0.f;
    a.sP[g] = 0.f; a.skP[g] = 0.f; a.sPl[g] = 0.f; a.mx[g] = 0.f; a.mk[g] = 1;
  }
  float scale[4] = {1.f, 1.f, 1.f, 1.f};
  bool flat[4] = {false, false, false, false};
  // band of bin k = ((k - 1) * 8) / K as a multiply-high: exact for (k - 1) * 8 * K < 2^32
  const uint32_t bmagic = K == 1 ? 0xffffffffu : 0xffffffffu / (uint32_t)K + 1u;

  // one sweep of the samples for NT bin tiles starting at tile t0, then their epilogue
  auto sweep = [&](auto nt_c, int t0) {
    constexpr int NT = decltype(nt_c)::value;
    f32x4_t ac[NT], as[NT];
    int idx[NT], inc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int k = 1 + 16 * (t0 + u) + col;  // k <= K + 15 < W for W >= 32
      const int kk = W >= 32 ? k : k % W;
      idx[u] = mod4(kk * q, W);
      inc[u] = mod4(4 * kk, W);
      ac[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      as[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const bool first = t0 == 0;
    // Software-pipelined: the operands of step s + 1 (one sample, NT twiddle pairs) are read from LDS before
    // the MFMAs of step s issue, so the reads' latency hides behind 2 NT MFMAs (read and used back to back,
    // every step paid NT + 1 LDS round trips).  Samples n >= W (the W % 4 tail, and the read ahead of the
    // last step) take the address of sample W - 1 and enter as zero operands.
    float xn;
    bool okn;
    float2 tn[NT];
    auto fetch = [&](int n) {
      okn = n < W;
      xn = xr[__mul24(okn ? n : W - 1, A)];
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        tn[u] = tab[idx[u]];
        idx[u] += inc[u];
        idx[u] -= idx[u] >= W ? W : 0;
      }
    };
    fetch(q);
    for (int n0 = 0; n0 < W; n0 += 4) {
      const float x = xn, d = okn ? xn - pivot : 0.f;
      float2 t[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u) t[u] = tn[u];
      fetch(n0 + 4 + q);
      if (first) {  // (uniform) the row's sums, min and max from the A fragments of the first sweep
        s1 += d; s2 = fmaf(d, d, s2); lo = fminf(lo, x); hi = fmaxf(hi, x);
      }
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        ac[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(d, t[u].x, ac[u], 0, 0, 0);
        as[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(d, t[u].y, as[u], 0, 0, 0);
      }
    }
    if (first) {
      // the four sample phases (lanes l, l ^ 16, l ^ 32) of a row, then C row 4 q + reg from lane 4 q + reg
      for (int m = 16; m <= 32; m <<= 1) {
        s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64);
        lo = fminf(lo, __shfl_xor(lo, m, 64)); hi = fmaxf(hi, __shfl_xor(hi, m, 64));
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int srcl = 4 * q + g;
        const float t1 = __shfl(s1, srcl, 64), t2 = __shfl(s2, srcl, 64);
        const float l = __shfl(lo, srcl, 64), h = __shfl(hi, srcl, 64);
        flat[g] = !(h > l);
        // W var = sum d^2 - (sum d)^2 / W, floored against cancellation (it is a scale, not a result)
        const float wv = fmaxf(t2 - t1 * t1 / (float)W, 1e-4f * t2);
        scale[g] = wv > 0.f ? 2.f / ((float)W * wv) : 1.f;
      }
    }
    // ---- epilogue of the NT tiles ----
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int k = 1 + 16 * (t0 + u) + col;
      const bool valid = k <= K;
      const float fk = (float)k;
      const int b = (int)__umulhi((uint32_t)(k - 1) * NBANDS, bmagic);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float re = ac[u][g], im = as[u][g];
        const float P = valid ? fmaf(re, re, im * im) * scale[g] : 0.f;
        a.sP[g] += P;
        a.skP[g] = fmaf(fk, P, a.skP[g]);
        a.sPl[g] += P > 0.f ? P * __logf(P) : 0.f;
        const bool up = P > a.mx[g];  // strict: a lane's k only grows, so ties keep the lowest
        a.mx[g] = up ? P : a.mx[g];
        a.mk[g] = up ? k : a.mk[g];
#pragma unroll
        for (int bb = 0; bb < NBANDS; ++bb) a.band[g][bb] += b == bb ? P : 0.f;
      }
    }
  };

  for (int t0 = 0; t0 < ntiles; t0 += NBT) {
    const int ntl = min(NBT, ntiles - t0);
    if (ntl == 4) sweep(std::integral_constant<int, 4>{}, t0);
    else if (ntl == 3) sweep(std::integral_constant<int, 3>{}, t0);
    else if (ntl == 2) sweep(std::integral_constant<int, 2>{}, t0);
    else sweep(std::integral_constant<int, 1>{}, t0);
  }

  // ---- one 16-lane reduction per row, then lane `col` < 11 writes feature `col` of its four rows ----
  const float fscale = hz / (float)W;
  const float inv_lnK = K > 1 ? 1.f / logf((float)K) : 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float tot = wops::row16_sum(a.sP[g]);
    const float skP = wops::row16_sum(a.skP[g]), sPl = wops::row16_sum(a.sPl[g]);
    float mx = a.mx[g];
    int mk = a.mk[g];
    auto comb = [&](float om, int ok) {
      const bool take = om > mx || (om == mx && ok < mk);
      mx = take ? om : mx;
      mk = take ? ok : mk;
    };
    comb(wops::dpp_f<wops::DPP_ROR8>(mx), wops::dpp_i<wops::DPP_ROR8>(mk));
    comb(wops::dpp_f<wops::DPP_ROR4>(mx), wops::dpp_i<wops::DPP_ROR4>(mk));
    comb(wops::dpp_f<wops::DPP_ROR2>(mx), wops::dpp_i<wops::DPP_ROR2>(mk));
    comb(wops::dpp_f<wops::DPP_ROR1>(mx), wops::dpp_i<wops::DPP_ROR1>(mk));
    float bsel = 0.f;
#pragma unroll
    for (int bb = 0; bb < NBANDS; ++bb) {
      const float bs = wops::row16_sum(a.band[g][bb]);
      bsel = col == bb ? bs : bsel;
    }
    const bool zero = flat[g] || !(tot > 0.f);
    const float inv = zero ? 0.f : 1.f / tot;
    const float ent = fmaxf((__logf(zero ? 1.f : tot) - sPl * inv) * inv_lnK, 0.f);
    float v = bsel * inv;
    v = col == NBANDS ? (float)mk * hz / (float)W : v;
    v = col == NBANDS + 1 ? skP * inv * fscale : v;
    v = col == NBANDS + 2 ? ent : v;
    v = zero ? 0.f : v;
    const int r = 16 * wave + 4 * q + g;
    if (col < NFA && r < nrows) {
      const int wi = r / A, ax = r - wi * A;
      const int f = col < NBANDS ? ax * NBANDS + col : col * A + ax;  // [A x 8 bands][dom A][centroid A][entropy A]
      const int64_t at = (w0 + wi) * (int64_t)o.ld + o.col0 + f;
      if constexpr (MLP) o.outb[at] = f2bf((v - o.mean[f]) * o.inv_std[f]);
      else o.out[at] = v;
    }
  }
}

// The block shape for one launch: windows per block (whole windows, 16 rows per wave) whose span and
// twiddle table fit the LDS — the most waves (4, 2, 1) within 64 KB (two or more blocks per CU), else
// within the 160 KB; then fewer windows than one wave's 16 rows hold.  false: not even one window fits.
struct Plan {
  int wpb, waves;
  size_t bytes;
};
bool make_plan(int A, int W, int stride, int64_t n_windows, Plan& p) {
  auto bytes = [&](int wpb) -> int64_t {
    return ((int64_t)tab_floats(W) + ((int64_t)(wpb - 1) * stride + W) * A + 4) * (int64_t)sizeof(float);
  };
  auto take = [&](int wpb) {
    p.wpb = wpb;
    p.waves = (wpb * A + 15) / 16;
    p.bytes = (size_t)bytes(wpb);
    return true;
  };
  const int64_t budgets[2] = {64 * 1024, LDS_MAX};
  for (int64_t budget : budgets)
    for (int waves = 4; waves >= 1; waves >>= 1) {
      const int wpb = (int)std::min<int64_t>(16 * waves / A, std::max<int64_t>(n_windows, 1));
      if (bytes(wpb) <= budget) return take(wpb);
    }
  for (int wpb = 16 / A - 1; wpb >= 1; --wpb)
    if (bytes(wpb) <= LDS_MAX) return take(wpb);
  return false;
}

// (cos, sin)(2 pi j / W), j = 0..W-1: float64 on the host, rounded once to fp32, one device copy per
// (device, W) kept for the life of the process (at most 16 KB each).  The first call for a W allocates and
// copies synchronously, so it must not happen inside a stream capture.
int twiddles(int W, const float2** out) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, float2*> cache;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find({dev, W});
  if (it == cache.end()) {
    std::vector<float2> h((size_t)W);
    const double step = 2.0 * M_PI / (double)W;
    for (int j = 0; j < W; ++j) h[(size_t)j] = float2{(float)std::cos(step * j), (float)std::sin(step * j)};
    float2* d = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(float2) * (size_t)W);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(d, h.data(), sizeof(float2) * (size_t)W, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return (int)e;
    }
    it = cache.emplace(std::make_pair(dev, W), d).first;
  }
  *out = it->second;
  return 0;
}

int contract(const float* stream, int64_t n_samples, int axes, int window, int stride, int64_t n_windows, float hz,
             const void* out, int ld_out, int col0, Plan& p) {
  if (axes <= 0 || axes > MAXA || axes % 3 || window < 3 || stride <= 0 || n_windows < 0 || col0 < 0 || !(hz > 0.f))
    return -2;
  if (n_windows > 0 && (n_windows - 1) * (int64_t)stride + window > n_samples) return -3;  // every window in bounds
  if (!stream || !out || (int64_t)ld_out < (int64_t)col0 + NFA * axes) return -4;
  if (window > MAXW || !make_plan(axes, window, stride, n_windows, p)) return -5;
  return 0;
}

template <bool MLP>
int launch(const float* stream, int axes, int window, int stride, int64_t n_windows, float hz, const Plan& p,
           const SpecOut& o, hipStream_t s) {
  const float2* tw = nullptr;
  if (const int rc = twiddles(window, &tw)) return rc;
  const int64_t nblk = (n_windows + p.wpb - 1) / p.wpb;
  if (nblk > 0x7fffffff) return -2;
  spectral_kernel<MLP><<<(unsigned)nblk, 64 * p.waves, p.bytes, s>>>(stream, tw, axes, window, stride, n_windows, hz,
                                                                     p.wpb, o);
  HAR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int har_spectral_max_window() { return MAXW; }

extern "C" int har_spectral_features(const float* stream, int64_t n_samples, int axes, int window, int stride,
                                     int64_t n_windows, float hz, float* out, int ld_out, int col0, hipStream_t s) {
  Plan p;
  if (const int rc = contract(stream, n_samples, axes, window, stride, n_windows, hz, out, ld_out, col0, p)) return rc;
  if (n_windows == 0) return 0;
  return launch<false>(stream, axes, window, stride, n_windows, hz, p, SpecOut{out, nullptr, nullptr, nullptr, ld_out, col0},
                       s);
}

extern "C" int har_spectral_features_mlp(const float* stream, int64_t n_samples, int axes, int window, int stride,
                                         int64_t n_windows, float hz, const float* mean, const float* inv_std,
                                         uint16_t* out, int ld_out, int col0, hipStream_t s) {
  Plan p;
  if (const int rc = contract(stream, n_samples, axes, window, stride, n_windows, hz, out, ld_out, col0, p)) return rc;
  if (!mean || !inv_std) return -4;
  if (n_windows == 0) return 0;
  return launch<true>(stream, axes, window, stride, n_windows, hz, p, SpecOut{nullptr, out, mean, inv_std, ld_out, col0},
                      s);
}
