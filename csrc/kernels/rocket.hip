// MiniRocket-style convolutional window features over raw IMU streams: a fixed bank of 84 dilated
// 9-tap kernels, pooled to PPV (the proportion of positions whose convolution exceeds a bias).
//
// Per window (W >= 9 samples x_c[t], A axes), dilation d_e = 2^e (e < n_dil) and kernel k (the k-th
// 3-subset {a < b < c} of {0..8} in lexicographic order; taps 2 on the subset, -1 elsewhere):
//   C[t] = sum_{c in mask[e,k]} sum_j w_k[j] x_c[t + (j - 4) d]          (samples outside [0, W) are 0)
//   count[e,k,i] = #{t in range : C[t] > bias[e,k,i]},  range = [0, W) for (e + k) even, [4d, W - 4d) else
//   feature = fp32(count) / fp32(range length), column (e * 84 + k) * q + i.
// The weights are integers, so on integer-valued samples every sum is exact and the counts equal the
// float64 definition (ops/rocket.py) bit for bit.
//
// The kernel:
//   * A block of four waves owns `wpb` whole windows.  Each is staged in LDS axis-major with 4 d_max zeros
//     on both sides of every axis row: a tap address is base + t + (j - 4) d with no bounds test, and the
//     padding contributes exact zeros.  Lanes are positions, so consecutive lanes read consecutive
//     dwords: no bank conflicts.
//   * A wave task is (window, dilation, group of NCH 64-position chunks); NCH * A = 12 (4 chunks at 3
//     axes, 2 at 6) or 9 (1 chunk at 9 axes), so the task's 9 A taps per chunk sit in at most 108 VGPRs
//     and are read from LDS once for all 84 kernels.
//   * The 84 kernels are a compile-time list.  With alpha_c = -sum_j T_c,j (once per task and axis),
//     kernel k costs alpha_c + 3 (T_c,a + T_c,b + T_c,c) per axis: two adds and one FMA, then one FMA
//     with the axis's 0/1 factor.  The axis mask and the biases are wave-uniform (scalar loads, SGPR
//     factors): no per-lane select.
//   * Each bias is one compare; its 64-bit result is ANDed with the chunk's valid-position mask and
//     popcounted on the scalar unit.  The count of (kernel, bias) is a scalar; one lane adds it to the
//     window's integer count table in LDS (windows longer than one group meet there).
//   * After a barrier the block turns the table into features with coalesced stores.  Integer counts only:
//     no float atomics, no cross-lane reduction, and a window's row does not depend on the block it is in.
// Samples must be finite (a 0 factor does not silence a NaN of an unselected axis).
#include <type_traits>
#include <utility>

#include "common.h"
#include "../har_kernels.h"

namespace {

constexpr int NK = 84;                     // kernels: 3-subsets of 9 taps
constexpr int64_t LDS_MAX = 160 * 1024;    // bytes of LDS a block may take
constexpr int64_t IMG_MAX = 96 * 1024;     // ... of which one window's padded image (har_rocket_max_window)
constexpr int64_t LDS_SHARED = 64 * 1024;  // preferred: two or more blocks per CU

struct Combs {
  int a[NK], b[NK], c[NK];
};
constexpr Combs make_combs() {
  Combs t{};
  int k = 0;
  for (int a = 0; a < 9; ++a)
    for (int b = a + 1; b < 9; ++b)
      for (int c = b + 1; c < 9; ++c) {
        t.a[k] = a; t.b[k] = b; t.c[k] = c;
        ++k;
      }
  return t;
}
constexpr Combs COMBS = make_combs();

template <class F, int... Is>
__device__ __forceinline__ void for_each_kernel(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}

__host__ __device__ constexpr int chunks_per_task(int A) { return A == 3 ? 4 : A == 6 ? 2 : 1; }

struct RocketArgs {
  const float* stream;   // [S, A]
  const int* masks;      // [n_dil, 84] axis bit sets
  const float* biases;   // [n_dil, 84, q]
  float* out;            // rows [n_windows][ld], columns [col0, col0 + F)
  int* counts;           // [n_windows, F] or null
  int64_t n_windows;
  int W, stride, n_dil, q, ld, col0, wpb, pad, wp, F;
};

template <int A>
__global__ __launch_bounds__(256) void rocket_kernel(RocketArgs p) {
  constexpr int NCH = chunks_per_task(A);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int W = p.W, wp = p.wp, pad = p.pad, F = p.F, q = p.q;
  const int img = A * wp;                                      // floats of one window's image
  const int64_t w0 = (int64_t)blockIdx.x * p.wpb;
  const int nwin = (int)min<int64_t>(p.wpb, p.n_windows - w0);
  float* const image = lds;                                    // [wpb][A][wp]
  int* const table = reinterpret_cast<int*>(lds + p.wpb * img);  // [wpb][F]

  // ---- stage: axis-major rows with `pad` zeros on both sides, and a zeroed count table ----
  for (int wi = 0; wi < nwin; ++wi) {
    const float* src = p.stream + (w0 + wi) * (int64_t)p.stride * A;
    float* dst = image + wi * img;
    for (int i = tid; i < img; i += nt) {
      const int c = i / wp, t = i - c * wp - pad;
      dst[i] = (t >= 0 && t < W) ? src[t * A + c] : 0.f;
    }
  }
  for (int i = tid; i < nwin * F; i += nt) table[i] = 0;
  __syncthreads();

  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nt >> 6;
  const int ngroups = (W + 64 * NCH - 1) / (64 * NCH);
  const int per_win = p.n_dil * ngroups, ntasks = nwin * per_win;

  for (int task = wave; task < ntasks; task += nwaves) {
    const int wi = task / per_win, r = task - wi * per_win;
    const int e = r / ngroups, g = r - e * ngroups;
    const int d = 1 << e;
    const float* const row0 = image + wi * img + pad;
    int* const cnt = table + wi * F + e * NK * q;
    const int* const mrow = p.masks + e * NK;
    const float* const brow = p.biases + (int64_t)e * NK * q;

    // the task's taps, alpha and valid-position masks
    float T[NCH][A][9], alpha[NCH][A];
    unsigned long long vpad[NCH], vval[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int t = (g * NCH + ch) * 64 + lane;
      const int tl = min(t, W - 1);  // lanes past the window read its last position and are never counted
      vpad[ch] = __ballot(t < W);
      vval[ch] = __ballot(t >= 4 * d && t < W - 4 * d);
#pragma unroll
      for (int c = 0; c < A; ++c) {
        const float* x = row0 + c * wp + tl;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          T[ch][c][j] = x[(j - 4) * d];
          s += T[ch][c][j];
        }
        alpha[ch][c] = -s;
      }
    }

    for_each_kernel(
        [&](auto kc) {
          constexpr int k = decltype(kc)::value;
          constexpr int ta = COMBS.a[k], tb = COMBS.b[k], tc = COMBS.c[k];
          const int m = mrow[k];
          float f[A];
#pragma unroll
          for (int c = 0; c < A; ++c) f[c] = (m >> c) & 1 ? 1.f : 0.f;
          float C[NCH];
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < A; ++c) {
              const float s3 = (T[ch][c][ta] + T[ch][c][tb]) + T[ch][c][tc];
              acc = fmaf(f[c], fmaf(3.f, s3, alpha[ch][c]), acc);
            }
            C[ch] = acc;
          }
          const bool padded = ((e + k) & 1) == 0;
          for (int i = 0; i < q; ++i) {
            const float b = brow[k * q + i];
            int n = 0;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
              n += __popcll(__ballot(C[ch] > b) & (padded ? vpad[ch] : vval[ch]));
            if (lane == 0 && n) atomicAdd(&cnt[k * q + i], n);
          }
        },
        std::make_integer_sequence<int, NK>{});
  }
  __syncthreads();

  // ---- counts -> features: fp32(count) / fp32(L), one correctly rounded division ----
  const int per_e = NK * q;
  for (int i = tid; i < nwin * F; i += nt) {
    const int wi = i / F, fi = i - wi * F;
    const int e = fi / per_e, k = (fi - e * per_e) / q;
    const int L = ((e + k) & 1) ? W - (8 << e) : W;
    const int n = table[i];
    p.out[(w0 + wi) * (int64_t)p.ld + p.col0 + fi] = (float)n / (float)L;
    if (p.counts) p.counts[(w0 + wi) * (int64_t)F + fi] = n;
  }
}

// dilations of a window: d_e = 2^e, e = 0 .. floor(log2((W - 1) / 8))
int n_dilations(int W) {
  int n = 0;
  while ((8 << n) <= W - 1) ++n;
  return n;
}

int64_t image_bytes(int A, int W) {
  const int pad = 4 << (n_dilations(W) - 1);
  return (int64_t)A * (W + 2 * pad) * (int64_t)sizeof(float);
}

}  // namespace

extern "C" int har_rocket_max_window(int axes) {
  if (axes != 3 && axes != 6 && axes != 9) return 0;
  int W = 9;
  while (image_bytes(axes, W + 1) <= IMG_MAX) ++W;
  return W;
}

extern "C" int har_rocket_features(const float* stream, int64_t n_samples, int axes, int window, int stride,
                                   int64_t n_windows, int n_dil, int q, const int* masks, const float* biases,
                                   float* out, int ld_out, int col0, int* counts, hipStream_t s) {
  if ((axes != 3 && axes != 6 && axes != 9) || window < 9 || stride <= 0 || n_windows < 0 || col0 < 0 || q < 1 ||
      n_dil != n_dilations(window))
    return -2;
  if (n_windows > 0 && (n_windows - 1) * (int64_t)stride + window > n_samples) return -3;  // every window in bounds
  const int64_t F = (int64_t)NK * n_dil * q;
  if (!stream || !masks || !biases || !out || (int64_t)ld_out < (int64_t)col0 + F) return -4;
  const int64_t per_window = image_bytes(axes, window) + F * (int64_t)sizeof(int);
  if (window > har_rocket_max_window(axes) || per_window > LDS_MAX) return -5;
  if (n_windows == 0) return 0;

  // windows per block: up to 4 (tasks spread evenly over the four waves) within 64 KB, else one
  int wpb = 1;
  for (int w = 4; w > 1; w >>= 1)
    if (w * per_window <= LDS_SHARED) {
      wpb = w;
      break;
    }
  const int64_t nblk = (n_windows + wpb - 1) / wpb;
  if (nblk > 0x7fffffff) return -2;
  RocketArgs p;
  p.stream = stream; p.masks = masks; p.biases = biases; p.out = out; p.counts = counts;
  p.n_windows = n_windows;
  p.W = window; p.stride = stride; p.n_dil = n_dil; p.q = q; p.ld = ld_out; p.col0 = col0; p.wpb = wpb;
  p.pad = 4 << (n_dil - 1);
  p.wp = window + 2 * p.pad;
  p.F = (int)F;
  const size_t bytes = (size_t)(wpb * per_window);
  if (axes == 3) rocket_kernel<3><<<(unsigned)nblk, 256, bytes, s>>>(p);
  else if (axes == 6) rocket_kernel<6><<<(unsigned)nblk, 256, bytes, s>>>(p);
  else rocket_kernel<9><<<(unsigned)nblk, 256, bytes, s>>>(p);
  HAR_CHECK_LAUNCH();
  return 0;
}
