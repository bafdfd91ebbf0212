// C ABI of the har HIP kernels (gfx950).  Every launcher takes raw device
// pointers plus the HIP stream to enqueue on, never allocates or synchronizes
// (so every launch can be captured into a hipGraph), and returns 0 or a
// hipError_t / negative contract-violation code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct GemmParams {
  const void* A;
  const void* B;
  void* C;
  const float* bias;      // EPI_BIAS*, may be null
  const void* mask;       // EPI_RELU_GRAD: bf16 activations of the forward pass
  float* rowsum;          // optional fused sum_k A(m,k) (bias gradient of a weight-grad product)
  int M, N, K;
  int lda, ldb, ldc, ldmask;
  int k_split;            // EPI_F32_ATOMIC / EPI_F32_SLAB: K range per grid.z slice (multiple of 32)
  int tile;               // -1 = automatic tile choice, else tile id (gemm.hip)
  int64_t slab_stride;    // EPI_F32_SLAB: elements between the C slabs of consecutive splits
  int64_t slab_stride_rowsum;  // elements between rowsum slabs
  float alpha;
} GemmParams;

int har_gemm_bf16(const GemmParams* p, int layout, int epi, hipStream_t s);
int har_gemm_f32(const GemmParams* p, int layout, int epi, hipStream_t s);

// Fused classifier head: logits = H . W^T + b (C <= 32 classes, W padded to 32 rows),
// softmax, cross-entropy, dlogits = (p - onehot) * scale (bf16, 32 columns).
// Per-workgroup partial CE sums / correct counts go to block_loss[blockIdx] /
// block_correct[blockIdx] (no same-address atomics; the host sums them lazily).
// Returns the number of workgroups through *nblocks_out if non-null.
int har_softmax_ce_head(const uint16_t* H, const uint16_t* W, const float* bias, const int32_t* labels,
                        int B, int Hdim, int C, float scale, uint16_t* dlogits, float* block_loss,
                        int32_t* block_correct, float* logits_out, hipStream_t s);
int har_softmax_ce_head_blocks(int B);

// Fused Adam(W) over a flat fp32 parameter buffer; also writes the bf16 compute copy.
// Gradient = grad[i] (if slabs == null) or sum_s slabs[s*n + i] (fused split-K reduction).
// The step counter (*step, device int32) is incremented on the stream before the update
// (by this call when tick != 0, else by an earlier kernel such as har_reduce_slabs_grouped).
// Flat-gradient reduction (+ Adam) of the MLP step (mlp.hip): mode bits 1 = reduce the regions' slabs,
// 2 = store G, 4 = Adam with t = *step (tick != 0: *step += 1 first, in its own launch).  Regions:
// sorted, disjoint, 4-aligned [start, start + len), S slabs at src + s * lds.
// MFMA-fragment-ordered bf16 copies of the step's W0 / W1 (mlp.hip frag_pos): dst = [W0 frag (H*K0) |
// W1 frag (H*H) | W1^T frag (H*H)], refreshed by every Adam update that is given the spec.
typedef struct MlpFragSpec {
  uint16_t* dst;
  int64_t w0_off, w1_off;  // flat offsets of W0 [H][K0] and W1 [H][H]
  int K0, H;
  int w1t;                 // the Adam update also writes the W1^T copy (paths with no step forward)
} MlpFragSpec;
// Small-batch step (mlp_small.hip): the whole forward + backward of a 32-row tile per workgroup (B / 32
// of them, B <= har_mlp_small_step_max_batch()), each writing its partial gradient to slab blockIdx.x in
// the flat parameter layout (segment offsets off_*), loss / #correct per workgroup; `tick` (optional)
// advances Adam's step counter.  Wf: the MlpFragSpec fragment copies (W0 | W1 | W1^T, all read).
typedef struct MlpSmallStepArgs {
  const uint16_t* X;        // [B][K0] bf16 (padded inputs)
  const uint16_t* Wf;       // fragment copies
  const float* b0;
  const float* b1;
  const uint16_t* Wo;       // [16][H] bf16
  const float* bo;          // [16]
  const int32_t* labels;    // [B]
  int B, C;
  float scale;              // 1 / global batch
  float* slab;              // [B / 32][total]
  int64_t total, off_w0, off_b0, off_w1, off_b1, off_wo, off_bo;
  float* block_loss;        // [B / 32]
  int32_t* block_correct;   // [B / 32]
  int32_t* tick;
} MlpSmallStepArgs;
int har_mlp_small_step(const MlpSmallStepArgs* args, int K0, int H, hipStream_t s);
int har_mlp_small_step_max_batch();
int har_grad_reduce_adam(int nreg, const float* const* src, const int64_t* start, const int64_t* len,
                         const int64_t* lds, const int* S, int64_t n, float* G, float* param, float* m, float* v,
                         uint16_t* pb, float lr, float b1, float b2, float eps, float wd, int32_t* step, int tick,
                         int mode, const MlpFragSpec* frag, hipStream_t s, const void* pf = nullptr,
                         int64_t pf_bytes = 0, uint32_t* pf_sink = nullptr, const void* pf1 = nullptr,
                         int64_t pf1_bytes = 0);
int har_mlp_pack_frag(const uint16_t* pb, const MlpFragSpec* f, hipStream_t s);
int har_adam_step(float* param, const float* grad, const float* slabs, int nslabs, float* m, float* v,
                  uint16_t* param_bf16, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, float grad_scale, int32_t* step, int tick, hipStream_t s);

// Fused head + last hidden layer's data gradient: logits/softmax/CE/dlogits as above plus
// dH = (dlogits . Wout) * (H > 0) written as bf16 [B][D].  Per-workgroup partials (64 rows each).
int har_head_fused(const uint16_t* H, const uint16_t* W, const float* bias, const int32_t* labels, int B, int D,
                   int C, float scale, uint16_t* dlogits, uint16_t* dH, float* block_loss, int32_t* block_correct,
                   hipStream_t s);
int har_head_fused_blocks(int B);

// Fused 2-hidden-layer MLP forward + head + head weight gradient (mlp_fused.hip):
// X [B][K0] bf16 (K0 = 32/64), W0 [H][K0], W1 [H][H], Wo [>=16][H] bf16 (H = 128/256),
// fp32 biases, C <= 16 classes, B % 16 == 0.  Writes h1 and dact2 = (dz . Wo) * (h2 > 0)
// ([B][H] bf16), per-workgroup slabs of pitch 16*H + 16 + H floats (dWout rows 0..15, dbout 0..15;
// the last H floats of a slab are not written) and per-workgroup loss / #correct.  Grid size:
// har_mlp_fwd_head_grid(B).
int har_mlp_fwd_head(const uint16_t* X, int K0, const uint16_t* W0, const float* b0, const uint16_t* W1,
                     const float* b1, int H, const uint16_t* Wo, const float* bo, const int32_t* labels, int B,
                     int C, float scale, uint16_t* h1, uint16_t* dact, float* slab, float* block_loss,
                     int32_t* block_correct, hipStream_t s);
int har_mlp_fwd_head_grid(int B);
// Fused training step of the H = 256 MLP (mlp_step.hip; K0 = 32/64, C <= 16, B % 64 == 0):
// har_mlp_step_fwd writes dact2 [B][256] bf16 (the layer-2 gradient (dz . Wout) * relu'(h2), 16-byte
// chunks of rows with bit 2 set swapped in pairs), per workgroup slabs
// [har_mlp_step_grid(B)][har_mlp_step_fwd_slab_width(H)] (dWout rows 0..15, dbout) and per-workgroup
// loss / #correct; har_mlp_step_bwd reads dact2 and X and writes per row slice
// s < har_mlp_step_slices(B) the partials of dW1, dW0, db0, db1 at gw1 / gw0 / gb0 / gb1 + s * slab_stride
// (h1 recomputed from X).
// Wf: the MlpFragSpec::dst fragment copies of W0 / W1 (the step's weight operands); the forward
// (re)writes the W1^T part from its W1 registers, the backward of the same step reads it.
int har_mlp_step_fwd(const uint16_t* X, int K0, uint16_t* Wf, const float* b0, const float* b1, int H,
                     const uint16_t* Wo, const float* bo, const int32_t* labels, int B, int C, float scale,
                     uint16_t* dact2, float* slab, float* block_loss, int32_t* block_correct, hipStream_t s);
// serving forward on the same pipeline: logits [B][C] fp32 + argmax [B] (B % 64 == 0, H == 256)
int har_mlp_step_fwd_infer(const uint16_t* X, int K0, const uint16_t* Wf, const float* b0, const float* b1, int H,
                           const uint16_t* Wo, const float* bo, int B, int C, float* logits, int32_t* pred,
                           hipStream_t s);
int har_mlp_step_bwd(const uint16_t* dact2, const uint16_t* X, int K0, const uint16_t* Wf, int H, const float* b0,
                     int B, float* gw1, float* gw0, float* gb0, float* gb1, int64_t slab_stride, int32_t* tick,
                     const float* fslab, int fslab_w, float* gwo, float* gbo, hipStream_t s);
int har_mlp_step_grid(int B);
int har_mlp_step_slices(int B);
int har_mlp_step_fwd_slab_width(int H);
// diagnostic phase stamps of the step kernels (nullptr = off); see mlp_step.hip
void har_mlp_set_stamps(uint64_t* p);
// Serving variant of the same kernel: logits [B][C] fp32 + argmax class [B] int32, nothing else.
int har_mlp_fwd_infer_f32(const float* X, int ldx, int F, int K0, const uint16_t* W0, const float* b0,
                          const uint16_t* W1, const float* b1, int H, const uint16_t* Wo, const float* bo, int B, int C,
                          float* logits, int32_t* pred, hipStream_t s);
int har_mlp_fwd_infer(const uint16_t* X, int K0, const uint16_t* W0, const float* b0, const uint16_t* W1,
                      const float* b1, int H, const uint16_t* Wo, const float* bo, int B, int C, float* logits,
                      int32_t* pred, hipStream_t s);

// dst[g*n + i] = sum of slabs[s*n + i] over the g-th group of ceil(S/G) slabs (deterministic).
// A non-null tick is incremented once by the first workgroup (the optimizer step counter).
// Up to 4 independent grouped slab reductions in one launch (per-segment slabs / S / n / lds / dst / ldd).
int har_reduce_slabs_multi(int nseg, const float* const* slabs, const int* S, const int64_t* n, const int64_t* lds,
                           float* const* dst, const int64_t* ldd, int G, int32_t* tick, hipStream_t s);
int har_reduce_slabs_grouped(const float* slabs, int S, int64_t n, int64_t lds, float* dst, int G, int64_t ldd,
                             int32_t* tick, hipStream_t s);

// dst[i] = sum_s slabs[s*n + i]  (deterministic split-K reduction)
int har_reduce_slabs(const float* slabs, int nslabs, int64_t n, float* dst, hipStream_t s);

// fp32 -> bf16 cast with row padding: out[r][0:cols_out] = in[r][0:cols_in], zero fill.
int har_cast_pad_bf16(const float* in, int rows, int cols_in, int ld_in, uint16_t* out, int cols_out,
                      hipStream_t s);

// ---- randomness (Philox4x32-10 keyed by global row id) ----
int har_philox_buckets(uint64_t seed, uint32_t stream, int64_t row0, int64_t n, const uint32_t* thr,
                       int nthr, int32_t* out, hipStream_t s);
// Per-fit init (tree.hip): W [T][N] = bootstrap draw from the CDF table (or 1) x optional rw [T][N]; node_of [T][N]
// = 0 / -1 (zero weight); root class counts added into stats + t * stats_tree_stride; *bad |= 1 on a
// label outside [0, K), *bad |= 2 on a weight W that is not a non-negative integer below 2^24 (the
// integer-weight contract of the level kernels, see "trees" below).
// cdf: HOST array of ncdf (<= 16) uint32 bootstrap CDF thresholds (ncdf = 0: every weight 1).
int har_tree_init(uint64_t seed, int tree0, int ntrees, int64_t row0, int64_t n, const uint32_t* cdf, int ncdf,
                  const float* rw, const int32_t* y, int K, float* W, int32_t* node_of, float* stats,
                  int64_t stats_tree_stride, int32_t* bad, hipStream_t s);
// findSplits cut points from the per-feature sorted sample [F][n] (NaN last), n <= 16384, ns <= 63:
// out [F][ns + 1] = thresholds then their count.
int har_find_splits_post_sort(const float* sorted, int F, int n, int ns, float* out, hipStream_t s);
// findSplits sample sort: columns of the row-major X [n][ld] (F of them) -> out [F][n] ascending, NaN
// last (n <= 16384: one LDS bitonic sort per column).
int har_sort_columns(const float* X, int n, int F, int ld, float* out, hipStream_t s);
int har_poisson_bootstrap(uint64_t seed, int tree0, int ntrees, int64_t row0, int64_t n, uint8_t* out,
                          hipStream_t s);

// ---- statistics / metrics ----
// Column count/sum/sumsq/min/max (optional row weights, NaN skipped) -> stats[5][ncols] (double);
// workspace: har_column_stats_workspace(n, ncols) doubles.
int har_column_stats(const float* X, int64_t n, int ncols, int ld, const float* w, double* stats,
                     double* workspace, hipStream_t s);
int har_column_stats_f64(const double* X, int64_t n, int ncols, const double* center, double* stats,
                         double* workspace, hipStream_t s);
int64_t har_column_stats_workspace(int64_t n, int ncols);
// bins[f][i] = #{b < nthr[f] : thr[f][b] < X[i][f]}  (uint8, feature-major)
int har_bin_features(const float* X, int64_t n, int F, int ld, const float* thr, int maxb, const int32_t* nthr,
                     uint8_t* bins, hipStream_t s);
// counts of codes in [0, V) (V <= 32768; -1 / out-of-range ignored) into out[V] (zeroed here)
int har_value_counts(const int64_t* codes, int64_t n, int V, int64_t* out, hipStream_t s);
int har_value_counts_max_v();  // largest V the launcher accepts on the current device
int har_confusion_matrix(const int32_t* label, const int32_t* pred, int64_t n, int K, int64_t* cm,
                         hipStream_t s);
int har_regression_moments(const float* y, const float* yhat, int64_t n, double* out6, hipStream_t s);
// B models' confusion matrices over masked rows: pred / mask [B][n] (mask != 0 = scored), cm [B][K][K]
// (zeroed here)
// DP forest level wire format (tree_dp.hip): per-node present classes / field widths packed into
// int32 words (sum-exact), and the owner's unpack back to an fp32 [n][mb][K] store
int har_tree_dp_pack(const float* store, int A, int64_t slot, int mb, int K, const int32_t* cls, const int32_t* kp,
                     const int32_t* bw, const int64_t* woff, int32_t* out, hipStream_t s);
int har_tree_dp_unpack(const int32_t* in, int a0, int n, int64_t slot, int mb, int K, const int32_t* cls,
                       const int32_t* kp, const int32_t* bw, const int64_t* woff, int64_t base, float* local,
                       hipStream_t s);
int har_confusion_matrix_batched(const int32_t* label, const int32_t* pred, const uint8_t* mask, int64_t n, int B,
                                 int K, int64_t* cm, hipStream_t s);
// scores sorted descending, labels permuted alike (positive iff > 0.5):
// out4 = {sum dFP (TP + TP_prev), sum dTP (prec + prec_prev), P, N} over tie-group end points
int har_roc_pr_sums(const float* sorted_scores, const float* labels, int64_t n, double* out4, hipStream_t s);
int har_roc_pr_sums_batched(const float* sorted_scores, const float* labels, const int32_t* ns, int B, int64_t ld,
                            double* out, hipStream_t s);

// ---- logistic regression (batched over B models, K classes padded to 8) ----
// ---- device logistic regression + batched L-BFGS / OWL-QN (logreg_qn.hip) ----
typedef struct LogregEvalArgs {
  const float* dense;       // [N][ldd] dense feature columns (Fd used)
  int64_t ldd;
  int Fd;
  const int32_t* dense_cols;  // [Fd] global column id of each dense column
  const int32_t* cat;       // [N][C] global column id of each row's one-hot entry, -1 = none
  int C;
  const int32_t* y;         // [N] labels (mode 0)
  const float* rw;          // [S][N] row weights per spec (null = 1)
  const float* inv_wsum;    // [S]
  const float* W;           // [n_trial_models][F+1][KP] effective weights (row F = intercept)
  int64_t N;
  int F, K, T, tstride;     // model bt = model0 + blockIdx.y * tstride, spec = bt / T
  int model0;               // first model of the launch (R holds one [N][KP] slot per launched model)
  int mode;                 // 0 = loss/gradient, 1 = margins into R
  float* R;                 // [n_trial_models][N][KP] residuals (mode 0, needed when C > 0) / margins
  float* slab;              // [n_trial_models][tiles][Fd*KP + KP + 1]
} LogregEvalArgs;

typedef struct LogregGradArgs {
  const float* slab;
  const float* R;
  const int32_t* col_map;   // [F+1]: >= 0 dense index, -1 intercept, <= -2 one-hot (CSC rows)
  const int32_t* csc_rows;  // row ids of the one-hot columns, column-major, ascending per column
  const int32_t* csc_off;   // [F+2] CSC offsets of every column
  const int32_t* col_slice; // [F+2] first row slice of each column (har_logreg_col_slices)
  int SL;                   // rows per slice
  const float* inv_std;     // [S][F]
  const float* pmask;       // [S][K][F+1]
  int64_t N;
  int F, Fd, K, T, tstride, ntiles;
  int model0;               // as LogregEvalArgs: model bt = model0 + blockIdx.y * tstride, R slot blockIdx.y
  float* G;                 // [n_trial_models][K][F+1]
  double* loss;             // [n_trial_models] (loss_fx == null)
  float* loss_fx;           // [n_trial_models][5] fixed-point loss pieces for the DP bucket, or null
  const int32_t* col_blk;   // [nblk][4] column blocks (c0, c1, first slice, end slice): <= 256 columns and
  int nblk;                 // <= 256 slices each (a lone heavier column excepted); grid.x of the launch
  const int32_t* srow;      // [slices + 1] first CSC row of every slice
} LogregGradArgs;

typedef struct QnArgs {
  int B, T, K, F, m, head, filled, init, nch;
  int fin_it;               // phase 2: hist row of the objective it leaves (0 for the init update)
  int64_t D;                // K * (F + 1)
  float* x;                 // [B][D] standardized parameters
  float* g;                 // [B][D] smooth gradient at x
  double* fobj;             // [B] objective at x (smooth + regularization)
  const float* l1;          // [B][D] per-element L1 weights (null = pure L-BFGS)
  const float* l2;          // [B][D] per-element L2 weights
  const float* pmask;       // [B][D]
  const float* inv_std;     // [B][F]
  float* S;                 // [m][B][D]
  float* Y;                 // [m][B][D]
  double* rho;              // [m][B] (0 = empty / rejected slot)
  double* SY;               // [B][m][m] history Gram matrix s_i . y_j
  double* YY;               // [B][m][m] history Gram matrix y_i . y_j
  double* P1;               // [B][nch][2m+1] chunk partials of the next direction's dots (phase 2)
  double* P2;               // [B][nch][3T+2] chunk partials (phase 1)
  double* P3;               // [B][nch][5+3m] chunk partials (phase 2)
  float* xtrial;            // [B*T][D]
  float* weff;              // [B*T][F+1][KP]
  double* reg;              // [B*T]
  double* decr;             // [B*T]
  const float* G;           // [B*T][D] data gradient of each trial (masked, scaled)
  const double* loss;       // [B*T] data loss of each trial
  float* step_scale;        // [B]
  int32_t* active;          // [B]
  int32_t* fails;           // [B]
  int32_t* iters;           // [B]
  int32_t* steep;           // [B] steepest descent this iteration (the last direction was not descent)
  int32_t* pick;            // [B] trial taken by the last phase 2 (-1 none, -2 non-descent)
  double* hist;             // [max_iter + 1][B] objective per iteration (nullable)
  int32_t* done;            // [B] phase-2 chunks done (zeroed; the last chunk resets it)
  double c1, tol;
} QnArgs;

int har_logreg_eval(const LogregEvalArgs* a, int KP, int n_models, hipStream_t s);
int har_logreg_eval_tiles(int64_t n);
int har_logreg_grad(const LogregGradArgs* a, int KP, int n_models, hipStream_t s);
typedef struct LogregSummaryArgs {
  const float* dense;       // [N][ldd] dense feature columns
  int64_t ldd;
  int Fd;
  const int32_t* y;         // [N]
  const float* rw;          // [S][N] row weights (null = 1)
  int64_t N;
  int F, K, S;
  const int32_t* col_map;   // [F+1] (HybridMatrix.col_map)
  const int32_t* csc_rows;
  const int32_t* csc_off;   // [F+2]
  const int32_t* col_slice; // [F+2] (har_logreg_col_slices)
  int SL;
  int ntiles;               // har_logreg_summary_tiles(N)
  const int32_t* srow;      // [slices + 1] first CSC row of every slice, or null (search the slice's column)
  double* part;             // [S][ntiles][2 Fd + K + 1] tile partials
  double* summ;             // [S][1 + 2F + K] (sum w, sum w x, sum w x^2, class sums)
} LogregSummaryArgs;

typedef struct LogregPrepareArgs {
  const double* summ;       // [B][1 + 2F + K] (all-reduced in data-parallel fits)
  const float* reg;         // [B] regParam
  const float* alpha;       // [B] elasticNetParam
  int B, F, K, Kp;
  int standardization, fit_intercept, binomial;
  float* inv_std;           // [B][F]
  float* inv_wsum;          // [B]
  float* pmask;             // [B][Kp][F+1]
  float* l2;                // [B][Kp (F+1)]
  float* l1;                // [B][Kp (F+1)] or null (no L1 term)
  float* x0;                // [B][Kp][F+1]
} LogregPrepareArgs;

// phase 0: tile partials, phase 1: column sums
int har_logreg_summary(const LogregSummaryArgs* a, int phase, hipStream_t s);
int har_logreg_summary_tiles(int64_t n);
int har_logreg_prepare(const LogregPrepareArgs* a, hipStream_t s);
int har_logreg_col_slices(const int32_t* csc_off, int F, int SL, int32_t* col_slice, hipStream_t s);
int har_logreg_loss_decode(const float* fx, double* loss, int n, hipStream_t s);
int har_qn_chunks(int64_t D, int B);
int har_lbfgs_phase(const QnArgs* a, int KP, int phase, hipStream_t s);
// diagnostic phase stamps of the evaluation / direction / update kernels (tools/lr_stamps.py); null = off
void har_lr_set_stamps(uint64_t* ev, uint64_t* dir, uint64_t* upd, uint64_t* grd);



// ---- windowed feature extraction over raw [S, A] streams ----
// Training-input variant: bf16 ((isnan(v) ? nan_value : v) - mean) * inv_std rows, zero-padded to ld_out.
int har_window_features_mlp(const float* stream, int64_t n_samples, int axes, int window, int stride,
                            int64_t n_windows, float hz, const float* mean, const float* inv_std, float nan_value,
                            uint16_t* out, int ld_out, hipStream_t s);
int har_window_features(const float* stream, int64_t n_samples, int axes, int window, int stride,
                        int64_t n_windows, float hz, int nbins, float* out, int ld_out, hipStream_t s);

// ---- spectral window features (spectral.hip): the DFT of every (window, axis) on the matrix cores ----
// 11 features per axis — 8 band fractions, dominant frequency, centroid, entropy — laid out
// [A x 8 bands][dominant Hz: A][centroid Hz: A][entropy: A], written as fp32 into columns
// [col0, col0 + 11 A) of rows [n_windows][ld_out].  Contract codes as har_window_features: -2 bad shape,
// -3 windows past the stream, -4 null pointer or row too narrow, -5 window longer than
// har_spectral_max_window() (or a span that does not fit the LDS).
int har_spectral_features(const float* stream, int64_t n_samples, int axes, int window, int stride,
                          int64_t n_windows, float hz, float* out, int ld_out, int col0, hipStream_t s);
// Training-input variant: bf16 ((v - mean[f]) * inv_std[f]), f in [0, 11 A), into columns [col0, col0 + 11 A)
// of an existing bf16 row buffer (the features are never NaN: no fill value).
int har_spectral_features_mlp(const float* stream, int64_t n_samples, int axes, int window, int stride,
                              int64_t n_windows, float hz, const float* mean, const float* inv_std, uint16_t* out,
                              int ld_out, int col0, hipStream_t s);
int har_spectral_max_window();

// ---- MiniRocket-style convolutional window features (rocket.hip) ----
// 84 dilated 9-tap kernels (the 3-subsets of the taps, weight 2 on the subset and -1 elsewhere) at the
// n_dil dilations 2^e of the window, an axis bit set masks[e][k] and q biases[e][k][i] per combination.
// Feature (e * 84 + k) * q + i = fp32(count) / fp32(L): the share of the combination's counted positions
// (all of [0, W) when e + k is even, [4 d, W - 4 d) otherwise) whose convolution exceeds the bias, written
// as fp32 into columns [col0, col0 + 84 n_dil q) of rows [n_windows][ld_out]; `counts` (nullable) receives
// the raw int32 counts [n_windows][84 n_dil q].  Contract codes as har_window_features: -2 bad shape (axes
// not 3, 6 or 9, window < 9, n_dil not the window's), -3 windows past the stream, -4 null pointer or row too
// narrow, -5 the zero-padded window image (or the count table) does not fit the LDS.
int har_rocket_features(const float* stream, int64_t n_samples, int axes, int window, int stride,
                        int64_t n_windows, int n_dil, int q, const int* masks, const float* biases, float* out,
                        int ld_out, int col0, int* counts, hipStream_t s);
// the longest window whose padded image fits the kernel's LDS budget (0: unsupported axis count)
int har_rocket_max_window(int axes);

// ---- trees ----
// Fused per-level histogram + best split; grid (feature chunks, active nodes).
// rows/row_w list each node's rows contiguously (node_start/node_count); feats [A][m].
// Outputs per (node, chunk): gain (-inf = none), global feature, bin, left class counts [K];
// out_total [A][K] = node class counts.  mode 0 fused; 1 histogram only -> ghist [A][m][maxbins][K];
// 2 split search from ghist (after a cross-rank reduction).  row_chunks > 1 (mode 1 only): each node's
// rows are split over that many workgroups that atomically merge into a ZEROED ghist.
// Integer-weight contract: every row_w is a non-negative integer and every class sum stays below 2^24.
// The histograms accumulate the weights as uint32 (a fractional weight would be truncated), and the
// order-free merges, sibling subtraction and the packed DP wire rely on the sums being exact.
// One-hot-aware histograms (tree.hip SPARSE): cat [N][ncat] int32 = the global column of each row's 1 in
// every one-hot block (-1 none), onehot [F] uint8 = 1 for the one-hot columns; F = the feature count.
typedef struct TreeSparse {
  const int32_t* cat;
  int ncat;
  const uint8_t* onehot;
  int F;
} TreeSparse;
// bins [F][n] of a hybrid matrix (numeric block dense [n][Fd] at columns dense_cols, one-hot entries cat)
// findSplits of a hybrid matrix (its sampled rows: cat [n][ncat]; colmap [F] = numeric index or < 0 for
// one-hot; dthr [Fd][ns + 1] = find_splits_post_sort of the numeric block) -> thr_mat [F][maxb], nbins [F]
int har_tree_thresholds_hybrid(const int32_t* cat, int64_t n, int ncat, int F, const int32_t* colmap, const float* dthr,
                               int ns, int maxb, int32_t* ones, float* thr_mat, int32_t* nbins, hipStream_t s);
int har_tree_bins_hybrid(const float* dense, int64_t n, int Fd, const int32_t* dense_cols, const int32_t* cat, int ncat,
                         int F, const float* thr, int maxb, const int32_t* nbins, uint8_t* bins, hipStream_t s);
int har_tree_hist_split(const uint8_t* bins, int64_t N, int F, int row_major, const int32_t* nbins_feat, const int32_t* rows,
                        const float* row_w, const int32_t* node_start, const int32_t* node_count, int A,
                        const int32_t* feats, int m, int fc, const int32_t* label, int K, int maxbins,
                        float min_inst, float min_gain, int impurity, float* out_gain, int32_t* out_feat,
                        int32_t* out_bin, float* out_left, float* out_total, int mode, float* ghist,
                        int row_chunks, const TreeSparse* sparse, hipStream_t s);
// Device-count convention of the level kernels below: a non-null a_dev / p_dev / s_dev points at the
// level's real count on the device and the host's A / P / S is then only an upper bound (grid size
// and array stride), so a whole fit can be enqueued without reading counts back per level.
// Load-balanced level (tree.hip): har_tree_plan builds the work plan from the node row counts
// (nodes of > prows rows become ceil(count / prows) chunk items with a merged-histogram slot, zeroed
// here for at most max_big slots of slot_elems floats); then har_tree_hist_split_planned mode 3
// (grid.y = an upper bound of the items: fused small nodes + chunk histograms) and mode 4 (grid.y
// = max_big: split search of the merged big nodes).  by_node = 1 keeps every node's histogram in
// ghist = a per-node store [A][m][bins][K]; mode 5 then derives the nodes marked derive_from[a] >= 0
// (sibling subtraction, parents in hprev, frontier-provided parent_of / derive_from).
int har_tree_plan(const int32_t* counts, int A, int prows, int32_t* plan, int64_t slot_elems, float* ghist,
                  int max_big, int by_node, const int32_t* a_dev, hipStream_t s);
int har_tree_hist_split_planned(const uint8_t* bins, int64_t N, int F, int row_major, const int32_t* nbins_feat,
                                const int32_t* rows, const float* row_w, const int32_t* node_start,
                                const int32_t* node_count, int A, const int32_t* feats, int m, int fc,
                                const int32_t* label, int K, int maxbins, float min_inst, float min_gain, int impurity,
                                float* out_gain, int32_t* out_feat, int32_t* out_bin, float* out_left,
                                float* out_total, int mode, float* ghist, int row_chunks, const int32_t* plan,
                                int prows, int bound, int by_node, const float* hprev, const int32_t* derive_from,
                                const int32_t* parent_of, const TreeSparse* sparse, hipStream_t s);
// Sum over trees of (normalized) leaf statistics; trees as SoA [T][maxn] arrays, feature < 0 = leaf.
// Level bookkeeping of the forest builder (tree_level.hip): Floyd feature subsets per (tree, node)
// (bit-identical to har/ops/rng.py), per-(tree,row) candidate keys, and the row -> child partition.
int har_tree_feature_subsets(uint64_t seed, const int32_t* trees, const int32_t* nodes, int64_t P, int F, int m,
                             int32_t* out, const int32_t* p_dev, hipStream_t s);
int har_tree_level_keys(const int32_t* node_of, const int32_t* cand_idx, int T, int64_t N, int maxn, int32_t* key,
                        hipStream_t s);
// Stable grouping of the level's (tree, row) pairs by candidate node (no sort); cnt_ws holds
// har_tree_level_group_chunks(N) x A ints.  -4: a tree has more than 4096 candidates.
int har_tree_level_group(const int32_t* node_of, const int32_t* cand_idx, const int32_t* tree_lo, const float* W,
                         int T, int64_t N, int maxn, int A, int nt_max, int32_t* cnt_ws, int32_t* counts,
                         int32_t* starts, int32_t* rows, float* row_w, const int32_t* a_dev, hipStream_t s);
int har_tree_level_group_chunks(int64_t N);
// Commit the level's splits (feature / bin / threshold / children / gain / child stats) in one launch,
// then move rows with the committed arrays (no per-level temporaries).
int har_tree_commit_level(int S, const int64_t* ti, const int64_t* ni, const int64_t* cl, const int64_t* dsi,
                          const int32_t* rfeat, const int32_t* rbin, const float* rgain, const float* rleft,
                          const float* rtotal, int K, const float* thr_mat, int ldthr, int maxn, int32_t* feature,
                          int32_t* split_bin, float* thresh, int32_t* left, int32_t* right, float* gains,
                          float* stats, const int32_t* s_dev, hipStream_t s);
int har_tree_partition_split(int32_t* node_of, const int32_t* feature, const int32_t* split_bin, const int32_t* left,
                             const uint8_t* bins, int T, int64_t N, int maxn, hipStream_t s);
int har_tree_level_decide(int A, const float* gain, const float* left, const float* total, int K, int impurity,
                          float min2, float* out, const int32_t* a_dev, hipStream_t s);
// Device-resident frontier update from the level decisions (see tree_level.hip): commit records
// ti/ni/cl/dsi [<= A], next candidates ct/cn [<= 2A], tree starts [Tn + 1], cand_idx entries, and
// scal = [splits, next candidates, max per tree, max weight float bits] (the level's one D2H).
int har_tree_frontier(int A, int Tn, int maxn, const int32_t* ct, const int32_t* cn, const int32_t* tlo,
                      const float* dec, const int32_t* n_nodes, int32_t* n_nodes_next, int32_t* pos_ws, int64_t* ti,
                      int64_t* ni, int64_t* cl, int64_t* dsi, float* front, int32_t* q_ws, int32_t* ct_next,
                      int32_t* cn_next, int32_t* tlo_next, int32_t* cand_idx, int32_t* scal, const int32_t* a_dev,
                      int32_t* parent_of, int32_t* derive_from, hipStream_t s);
// Root frontier (candidate roots, tree starts, cand_idx, scal = [0, A, 1, max weight bits]) from the
// root class counts stats[t * tree_stride .. + K), on the device.
int har_tree_root_frontier(const float* stats, int Tn, int K, int64_t tree_stride, int impurity, float min2,
                           int maxn, int32_t* ct, int32_t* cn, int32_t* tlo, int32_t* cand_idx, int32_t* scal,
                           hipStream_t s);
int har_tree_partition(int32_t* node_of, const int32_t* lvl_feat, const int32_t* lvl_bin, const int32_t* lvl_left,
                       const uint8_t* bins, int T, int64_t N, int maxn, hipStream_t s);
int har_forest_predict(const float* X, int64_t n, int F, int ld, const int32_t* feat, const float* thr,
                       const int32_t* left, const int32_t* right, const float* leaf, int ntrees, int maxn, int K,
                       int max_depth, int normalize, float* raw_out, hipStream_t s);

// ---- gradient-boosted trees (gbt.hip): multinomial Newton boosting on fixed-point derivatives ----
// Round m grows K regression trees (one per class) in lock step on the shared uint8 feature-major bins.
// Derivatives are int32 multiples of 2^-20 (rint), so every histogram / node total is an exact integer sum
// and a fit is bitwise reproducible.  Trees use the heap layout (children of n: 2n+1, 2n+2); level d holds
// nodes [2^d - 1, 2^(d+1) - 1).  Contract codes: -2 bad shape (K > 32, depth > 6, bins > 64, sizes), -4 null
// pointer.
// margins [N][K] fp32, labels [N], w [N] 0/1 subsample weights (null = 1) -> qgh [K][N][2] int32 (g, h;
// null = loss only) and block_loss[har_gbt_grad_blocks(N, K)] = per-workgroup sums of -log p_y over ALL rows.
int har_gbt_grad(const float* margins, const int32_t* y, const int32_t* w, int64_t N, int K, int32_t* qgh,
                 double* block_loss, hipStream_t s);
int har_gbt_grad_blocks(int64_t N, int K);
// Level histograms of all K trees: hist [K][2^level][F][maxb][3] int64 = sums of (g, h, nonzero-weight
// rows) per (class, node, feature, bin); zeroed here.  |g|, |h| <= 2^20 per row is the caller's contract
// (har_gbt_grad's outputs satisfy it); N <= 2^26 - 1024
// (65,535 row chunks of 1,024 rows).
int har_gbt_hist(const uint8_t* bins, const int32_t* qgh, const int32_t* w, const int32_t* node_of, int64_t N, int F,
                 int K, int maxb, int level, int64_t* hist, hipStream_t s);
int har_gbt_hist_rows_per_block();
typedef struct GbtSplitArgs {
  const int64_t* hist;     // [K][2^level][F][maxb][3]
  const int32_t* nbins;    // [F] bins per feature (cuts b in [0, nbins - 2])
  const float* thr_mat;    // [F][ldthr] thresholds (x <= thr[f][b] goes left)
  int F, K, maxb, ldthr, level;
  int tree0, maxn;         // class k writes tree tree0 + k of the [T][maxn] node arrays
  double lambda, step, min_gain;
  int64_t min_inst;
  // the level's decisions [K][2^level]: feature (-1 = leaf), bin, gain, sums = GL, HL, CL, G, H, C
  int32_t* o_feat;
  int32_t* o_bin;
  double* o_gain;
  int64_t* o_sums;         // [K][2^level][6]
  // committed node arrays [T][maxn] (stats [T][maxn][K], nonzero only at class k)
  int32_t* feature;
  int32_t* split_bin;
  float* thresh;
  int32_t* left;
  int32_t* right;
  float* gains;
  float* value;
  float* stats;
} GbtSplitArgs;
// One workgroup per (class tree, node): prefix scan over the bins of every feature, Newton gain in fp64
// from the exact integers (no contraction), argmax with ties to the lowest feature, then the lowest bin.
int har_gbt_split(const GbtSplitArgs* a, hipStream_t s);
// node_of [K][N] of the rows sitting in the level's split nodes moves to the child (weight-0 rows too)
int har_gbt_partition(int32_t* node_of, const uint8_t* bins, const int32_t* feature, const int32_t* split_bin,
                      int64_t N, int F, int K, int level, int tree0, int maxn, hipStream_t s);
// margins[i][k] += value[tree0 + k][node_of[k][i]]
int har_gbt_update(float* margins, const int32_t* node_of, const float* value, int64_t N, int K, int tree0, int maxn,
                   hipStream_t s);

// ---- HMM smoothing (hmm.hip): exact parallel Viterbi over a concatenated batch of sequences ----
// E [T][K], A [K][K], pi [K] int32 quanta of 2^-20 (|v| <= 2^25, the caller's contract), seq_offsets [S+1] int64
// on the device (0 = first, T = last, strictly increasing: validated by the caller on the host) -> path [T]
// int32, score [S] int64 (quanta).  All accumulation is int64 and every max-plus product exact, so the result
// equals the sequential recurrence bit for bit (lowest-index ties).  L = steps per chunk (har_hmm_chunk_len()
// is the default); ws = har_hmm_workspace_bytes(T, K, S, L) bytes of device scratch (-1 = bad shape).  Phases
// phase_lo..phase_hi of 0..6 run (0 flags, 1 chunk matrices, 2 chunk scan, 3 forward, 4 map scan, 5 backtrace,
// 6 scores; a probe times them one by one over the same workspace).  T = 0 launches nothing.  Contract codes:
// -2 bad shape (K outside 1..32, T >= 2^31, S outside 1..T, L < 1, workspace too small), -4 null pointer.
int har_hmm_chunk_len();
int har_hmm_scan_group();   // chunks per group of the two-level scans: more chunks than this take a second level
int64_t har_hmm_workspace_bytes(int64_t T, int K, int64_t S, int L);
int har_hmm_viterbi(const int32_t* E, const int32_t* A, const int32_t* pi, const int64_t* seq_offsets, int64_t T, int K,
                    int64_t S, int L, void* ws, int64_t ws_bytes, int32_t* path, int64_t* score, int phase_lo,
                    int phase_hi, hipStream_t s);

// ---- HMM posteriors (hmm_fb.hip): parallel forward-backward over the same concatenated batch ----
// B [T][K] emission likelihoods, P [K][K] transition probabilities, p0 [K] start probabilities, all fp64 in the
// probability domain (the caller's contract: B in [2^-93, 1] with a 1 in every row, P and p0 in [2^-52, 1]) ->
// gamma [T][K] state posteriors (rows sum to 1), loglik [S] per-sequence log-likelihoods, xi [K][K] the summed
// pairwise posteriors of every step that does not start a sequence (null = not wanted).  Running products are
// rescaled by powers of two (exact); no atomics, one writer per output element, two runs bitwise equal.
// ws = har_hmm_fb_workspace_bytes(T, K, S, L, want_xi) bytes of device scratch (-1 = bad shape).  Phases
// phase_lo..phase_hi of 0..5 run (0 flags, 1 chunk products, 2 prefix scan, 3 suffix scan, 4 chunk pass,
// 5 reductions).  variant picks phase 1's kernel at K > 8: 0 = the default, 1 = (i, j) lanes through LDS,
// 2 = v_mfma_f64_16x16x4_f64.  T = 0 launches nothing.  Contract codes: -2 bad shape (as har_hmm_viterbi; also
// L * K * 8 bytes above the 64 KiB a workgroup keeps a chunk's alpha rows in, a variant outside 0..2, workspace
// too small), -4 null pointer.
int64_t har_hmm_fb_workspace_bytes(int64_t T, int K, int64_t S, int L, int want_xi);
int har_hmm_forward_backward(const double* B, const double* P, const double* p0, const int64_t* seq_offsets, int64_t T,
                             int K, int64_t S, int L, void* ws, int64_t ws_bytes, double* gamma, double* loglik,
                             double* xi, int phase_lo, int phase_hi, int variant, hipStream_t s);

// ---- IIR stream filters (sosfilt.hip): cascaded second-order sections as a chunked scan over samples ----
// x [S][A] fp32 -> y: mode 0 the filtered stream [S][A], 1 [x - y | y] as [S][2A], 2 x - y [S][A] (xc, nullable,
// replaces x in the complement); every axis on its own, direct form II transposed in fp64, rounded once to fp32
// (har/ops/sosfilt.py).  sos[j] = (b0, b1, b2, a1, a2) of section j, zi[j] = its (s1, s2) per unit step input.
// seg [n_seg + 1] int64 on the device (0 first, S last, strictly increasing: validated by the caller on the host;
// unread when n_seg == 1): the state restarts at every segment start, from zi * x[start] (init_step) or zero.
// reverse runs every segment from its last sample to its first.  L = samples per chunk, G = elements per group of
// the carry scan, levels = har_sosfilt_levels(S, L, G); powers [levels][G][2 sections][2 sections] fp64 on the
// device, entry (l, k) = (M^(L G^l))^(k + 1) for the cascade's transition matrix M.  ws =
// har_sosfilt_workspace_bytes(...) bytes of device scratch (-1 = bad shape).  Phases phase_lo..phase_hi of 0..2
// run (0 chunk states, 1 carry scan, 2 apply).  S = 0 launches nothing.  Contract codes: -2 bad shape (A outside
// 1..9, sections outside 1..4, S >= 2^31 - 256, L outside 1..256, G outside 2..64, levels, mode, workspace too
// small), -4 null pointer.
typedef struct SosFilterArgs {
  const float* x;
  const float* xc;
  float* y;
  const int64_t* seg;
  int64_t n_samples, n_seg;
  int axes, sections, L, G;
  int reverse, init_step, mode;
  double sos[4][5];
  double zi[4][2];
  const double* powers;
  int levels;
  void* ws;
  int64_t ws_bytes;
  int phase_lo, phase_hi;
} SosFilterArgs;
int har_sosfilt_chunk_len();
int har_sosfilt_scan_group();
int har_sosfilt_levels(int64_t n_samples, int L, int G);
int64_t har_sosfilt_workspace_bytes(int64_t n_samples, int axes, int sections, int L, int G);
int har_sosfilt(const SosFilterArgs* a, hipStream_t s);

// ---- K-means and the silhouette (kmeans.hip): rows x centres on the fp32 matrix cores ----
// Working rows X [N][D] fp32 (centred by the caller), operand rows C [K][D] with h [K]: the score is
// s[n][k] = h[k] - <X[n], C[k]> (assignment: C = centres, h = ||C||^2 / 2; silhouette: C = cluster means,
// h = mean ||x||^2 of the cluster / 2).  K and D in 1..har_kmeans_max_k() / har_kmeans_max_d().
// Contract codes: -2 bad shape or a combination of outputs the mode does not have, -4 null pointer.
typedef struct KMeansArgs {
  const float* X;
  int64_t N;
  int D, K;
  const float* C;         // [K][D]
  const float* h;         // [K]
  const int32_t* w;       // assignment: integer row weights >= 0 (null = 1; 0 = the row is ignored)
  const int32_t* labels;  // assignment: given clusters [N] — no product, accumulation only (assign, d2, part
                          // must be null; a label outside [0, K) is ignored); silhouette: the rows' clusters
  const float* scale;     // [D] 2^e[f] (with acc)
  const double* norm_scale;  // [1] on the device: 2^q of the norm channel (with acc)
  int32_t* assign;        // [N] argmin_k s, lowest k among equals (nullable)
  float* d2;              // [N] float(max(0, ||x||^2 + 2 s)) (nullable)
  int64_t* acc;           // [K D sums | K counts | K norms], ADDED to (the caller or har_kmeans_update zeroes it)
  double* part;           // [ceil(N / har_kmeans_rows_per_block())] per-workgroup sums of w d2 / of the silhouettes
  const double* cnt;      // silhouette: cluster sizes [K]
  float* sil;             // silhouette: per row (nullable)
} KMeansArgs;
int har_kmeans_assign(const KMeansArgs* a, hipStream_t s);
int har_kmeans_silhouette(const KMeansArgs* a, hipStream_t s);
int har_kmeans_rows_per_block();
int har_kmeans_max_k();
int har_kmeans_max_d();
// out4 = {centres per LDS slab, slabs, 1 if the accumulators go through LDS, LDS bytes}
int har_kmeans_plan(int D, int K, int* out4);
// One Lloyd update in one launch.  state = {iterations, converged} (device).  When not converged and
// iterations < max_iter: C_new[k][f] = float(double(sum) * 2^-e[f] / count[k]) (an empty cluster keeps its
// centre), h, moved = max_k ||C_new[k] - C[k]||^2, cost_hist[iterations] = the sum of cost[0 .. ncost) in
// order, sizes = the counts, iterations += 1, converged = moved <= tol2.  Otherwise none of those change.
// In both cases acc is zeroed for the next assignment.
typedef struct KMeansUpdateArgs {
  int64_t* acc;           // [K D | K | K]
  const float* scale;     // [D] 2^e[f]
  int K, D, ncost, max_iter;
  const double* cost;     // [ncost] cost partials of the assignment that filled acc
  double tol2;
  float* C;               // [K][D]
  float* Cnew;            // [K][D] scratch
  float* h;               // [K]
  int32_t* state;         // [2]
  double* cost_hist;      // [max_iter]
  double* moved;          // [1] (nullable)
  int64_t* sizes;         // [K] (nullable)
} KMeansUpdateArgs;
int har_kmeans_update(const KMeansUpdateArgs* a, hipStream_t s);

// ---- Exact k-nearest neighbours (knn.hip): queries x references on the fp32 matrix cores, fused top-k ----
// Working rows Q [N][D], R [M][D] fp32, h [M] = ||R[m]||^2 / 2; the score is s[n][m] = h[m] - <Q[n], R[m]>.
// The neighbours of a row are its k smallest pairs (s, m) in lexicographic order; a pair with
// qgroup[n] >= 0 and qgroup[n] == rgroup[m] is skipped; missing entries are (+inf, -1).  Split t of
// `splits` takes the slabs [t S / splits, (t + 1) S / splits) of the S = ceil(M / har_knn_slab_rows(D))
// slabs of references and writes its sorted lists to ps / pi [splits][N][k].  1 <= splits <= min(S,
// har_knn_max_splits()).  Contract codes: -2 bad shape, -4 null pointer.
typedef struct KnnSearchArgs {
  const float* Q;
  int64_t N;
  const float* R;
  const float* h;
  int64_t M;
  int D, k, splits;
  const int32_t* qgroup;  // [N] (nullable: nothing is excluded)
  const int32_t* rgroup;  // [M] (nullable)
  float* ps;              // [splits][N][k] scores, ascending
  int32_t* pi;            // [splits][N][k] reference indices
} KnnSearchArgs;
int har_knn_search(const KnnSearchArgs* a, hipStream_t s);
int har_knn_query_rows();
int har_knn_max_k();
int har_knn_max_d();
int har_knn_max_classes();
int har_knn_max_splits();
int har_knn_slab_rows(int D);
// the number of splits the front-end takes when the caller names none: enough workgroups for the 256 CUs
int har_knn_auto_splits(int64_t N, int64_t M, int D);
// Per query row.  With ps: the k smallest pairs of the splits' lists -> idx, d2 = float(max(0, ||q||^2 +
// 2 s)) ([N][ldk], the first k of a row are written); without: idx / d2 are inputs.  With y (labels of the
// references, classes 0 .. C - 1): class weights over the first k entries (weights 0 = uniform, 1 =
// 1 / sqrt(d2) with the zero-distance rule) -> raw, prob [N][C] fp64 and pred [N] (each nullable).
typedef struct KnnVoteArgs {
  const float* ps;
  const int32_t* pi;
  int splits;
  const float* Q;  // [N][D] (with ps)
  int D;
  int64_t N;
  int k, ldk;
  int32_t* idx;
  float* d2;
  const int32_t* y;  // [M] (nullable: no vote)
  int64_t M;
  int C, weights;
  double* raw;
  double* prob;
  int32_t* pred;
} KnnVoteArgs;
int har_knn_merge_vote(const KnnVoteArgs* a, hipStream_t s);

// ---- Banded dynamic time warping (dtw.hip): one lane per (query, reference) pair of raw windows ----
// Windows Q [N][W][A], R [M][W][A] fp32, time-major; Sakoe-Chiba radius 0 <= radius <= min(W - 1,
// har_dtw_max_radius()); the cost of a pair is the squared-cost DTW of har/ops/dtw.py, one fixed fp32 operation
// sequence.  dtw_cost writes cost [N][M].  dtw_search keeps the k smallest pairs (cost, m) of every query
// (knn.hip's order, exclusion and missing entries) over the slabs [t S / splits, (t + 1) S / splits) of the S =
// ceil(M / har_dtw_slab_rows()) slabs of references and writes the sorted lists ps / pi [splits][N][k]; 1 <=
// splits <= min(S, har_dtw_max_splits()).  dtw_merge takes the k smallest pairs of the splits' lists -> idx, d2
// [N][k].  Contract codes: -2 bad shape, -4 null pointer.
typedef struct DtwArgs {
  const float* Q;
  int64_t N;
  const float* R;
  int64_t M;
  int W, A, radius;
  int k, splits;          // dtw_search
  const int32_t* qgroup;  // [N] (nullable, with rgroup: nothing is excluded)
  const int32_t* rgroup;  // [M]
  float* cost;            // [N][M] (dtw_cost)
  float* ps;              // [splits][N][k] costs, ascending (dtw_search)
  int32_t* pi;            // [splits][N][k] reference indices
} DtwArgs;
int har_dtw_cost(const DtwArgs* a, hipStream_t s);
int har_dtw_search(const DtwArgs* a, hipStream_t s);
typedef struct DtwMergeArgs {
  const float* ps;
  const int32_t* pi;
  int splits;
  int64_t N;
  int k;
  int32_t* idx;  // [N][k]
  float* d2;     // [N][k]
} DtwMergeArgs;
int har_dtw_merge(const DtwMergeArgs* a, hipStream_t s);
int har_dtw_query_rows();
int har_dtw_slab_rows();
int har_dtw_max_w();
int har_dtw_max_radius();
int har_dtw_max_axes();
int har_dtw_max_k();
int har_dtw_max_splits();
// the number of splits the front-end takes when the caller names none
int har_dtw_auto_splits(int64_t N, int64_t M);

// ---- Ridge classifier (ridge.hip): per-fold Gram moments on the fp32 matrix cores, batched fp64 Cholesky ----
// Augmented row a = [z | T | 1] (Dq = D + K + 1 columns): z = fl32(fl32(x - mean) * inv_std), T[c] = +1 when
// y == c else -1.  rows [n_total] lists the table rows grouped by fold; fold f owns rows[off[f] .. off[f + 1]).
// A fold's rows are cut into chunks of har_ridge_chunk_rows() rows from the fold's start; a chunk is one fp32 fma
// chain per entry in row order, chunk results are added in fp64.  Workgroup (pair, f, split) takes the chunks
// [split * cps, (split + 1) * cps) of fold f for one 64 x 64 tile pair (ti <= tj) and stores one fp64 slab
// slabs[((f * smax + split) * pairs + pair)][64][64]; smax = max_f ceil(chunks_f / cps).  ridge_gram_reduce sums
// the slabs of a fold in split order into Af [F][ldq][ldq] (entries i <= j, ldq = Dq rounded up to 64) and the
// folds in order into Aall [ldq][ldq].  Contract codes: -2 bad shape, -4 null pointer.
#define HAR_RIDGE_MAX_FOLDS 16
typedef struct RidgeGramArgs {
  const float* X;         // [N][ldx]
  int64_t ldx;
  const int32_t* y;       // [N]
  const int32_t* rows;    // [off[F]] row indices (< N) grouped by fold
  const float* mean;      // [D]
  const float* inv_std;   // [D]
  int64_t off[HAR_RIDGE_MAX_FOLDS + 1];
  int D, K, F;
  int cps;                // chunks per workgroup (>= 1)
  double* slabs;
  double* Af;
  double* Aall;
} RidgeGramArgs;
int har_ridge_chunk_rows();
int har_ridge_panel();
int har_ridge_max_dim();
int har_ridge_gram(const RidgeGramArgs* a, hipStream_t s);
int har_ridge_gram_reduce(const RidgeGramArgs* a, hipStream_t s);
// Systems sys0 .. sys0 + nsys - 1 of the fit's (F > 1 ? F + 1 : 1) * nalpha (system s: fold s / nalpha, the
// last one or F == 1 meaning "all rows"; alpha s % nalpha).  With n = n_all - n_f and u = A_all - A_f entrywise,
// entry (r, c), c <= r, c < D, r < D + K of system s is (u[c][r] - (u[c][q] * u[r][q]) / n) (+ alpha when r == c),
// q = D + K the column of ones; one rounding per operation, the quotient is 0 when n == 0.  Rows r < D are the
// lower triangle of M, rows D .. D + K - 1 the border Bc^T.  Sys [nsys][ldn][ldn] row-major, ldn = D + K rounded
// up to 64; everything else of a system's matrix is written as zero.
typedef struct RidgeSolveArgs {
  const double* Af;       // [F][ldq][ldq] (null when F == 1)
  const double* Aall;     // [ldq][ldq]
  const double* alphas;   // [nalpha]
  int D, K, F, nalpha;
  int sys0, nsys;
  double* Sys;            // [nsys][ldn][ldn]
  int32_t* info;          // [total systems]: 0, or 1 + the column whose pivot was not positive and finite
  double* W64;            // [total systems][K][ldn]: the solution before rounding
  float* W;               // [total systems][K][D]
  float* b;               // [total systems][K]
} RidgeSolveArgs;
int har_ridge_systems(const RidgeSolveArgs* a, hipStream_t s);
// Blocked right-looking Cholesky of the leading D columns of every system (panel width har_ridge_panel()); the
// border rows are carried through the triangular solves and end as (L^-1 Bc)^T.  info must be zero on entry.
int har_ridge_cholesky(const RidgeSolveArgs* a, hipStream_t s);
// L^T W = Y per (system, class), then b = (t - W^T s) / n; a system with info != 0 gets W = 0, b = 0.
int har_ridge_backsolve(const RidgeSolveArgs* a, hipStream_t s);

// ---- Gaussian mixtures (gmm.hip): full-covariance EM on the fp32 matrix cores ----
// Working rows Z [N][D] fp32 (standardised by the caller).  Component k: mu [K][D], the upper triangular
// W_k = L_k^{-T} [K][D][D] (Sigma_k = L_k L_k^T; the kernel reads entries on and above the diagonal only)
// and c [K] = log pi_k - D/2 log 2pi - sum_i log L_k[i][i] (-inf: the component is never chosen, r = 0).
// q[n][k] = |(z_n - mu_k) W_k|^2, t = c_k - q / 2, lse = logsumexp_k t, r = exp(t - lse), pred = the first
// argmax of r.  K in 1..har_gmm_max_k(), D in 1..har_gmm_max_d().  Contract codes as above (-2, -4).
// The grid is persistent: har_gmm_grid(N, D, K, max_blocks) workgroups (independent of N beyond one per
// har_gmm_rows_per_block() rows; max_blocks > 0 lowers the cap), each looping over row tiles, keeping
// its moment accumulators in LDS across the tiles and storing ONE moment slab [K][1 + Dp + Dp Dp] (Dp = D
// rounded up to 4) at its end: N_k | S1_k [Dp] | S2_k [Dp][Dp], moments of w r about mu_k, S2 valid for
// i <= j only (the upper triangle), and one fp64 partial of sum_n w lse.  Components whose accumulators
// do not fit the LDS together are taken har_gmm_group(D, K) at a time, one pass over the tiles per group;
// the passes after the first read w r back from the scratch wr, which is then required.
// No atomics: two launches give the same bits.
typedef struct GmmEstepArgs {
  const float* Z;
  int64_t N;
  int D, K;
  const float* mu;
  const float* W;
  const float* c;
  const float* w;   // [N] row weights >= 0 (nullable: 1)
  float* resp;      // [N][K] (nullable)
  float* lse;       // [N] (nullable)
  int32_t* pred;    // [N] (nullable)
  float* q;         // [N][K] (nullable)
  float* slabs;     // [grid][K][1 + Dp + Dp Dp], overwritten (nullable: no moments)
  float* wr;        // [N][K] scratch for w r (needed with slabs when har_gmm_group(D, K) < K, else nullable)
  double* part;     // [grid] (nullable)
  int max_blocks;   // 0: the default cap
  const int* state; // [2] iterations, converged (nullable): no work when converged or iterations >= max_iter
  int max_iter;
} GmmEstepArgs;
int har_gmm_estep(const GmmEstepArgs* a, hipStream_t s);
int har_gmm_rows_per_block();
int har_gmm_group(int D, int K);
int har_gmm_grid(int64_t N, int D, int K, int max_blocks);
// One workgroup per component, nothing when state (nullable) says converged or iterations >= max_iter.
// Sums the slabs in order in fp64; delta = S1 / N_k, mu += delta, Sigma = S2 / N_k - delta delta^T + reg I
// (diag: off-diagonal entries zeroed), pi_k = N_k / sum N, then the Cholesky factor, W = L^{-T} and c, all
// in fp64 in LDS, written as fp32.  N_k = 0 or a non-positive / non-finite pivot: mu and W stay, c is
// rebuilt from the kept factor's diagonal and the new weight.
typedef struct GmmFinishArgs {
  const float* slabs;
  int nslab, K, D, diag, max_iter;
  double reg;
  float* mu;
  float* W;
  float* c;
  double* Nk;        // [K]
  double* pi;        // [K]
  const int* state;  // [2] iterations, converged (nullable: always run)
} GmmFinishArgs;
int har_gmm_finish(const GmmFinishArgs* a, hipStream_t s);
// One workgroup.  When not converged and iterations < max_iter: hist[iterations] = the sum of part[0 ..
// npart) in the fixed order of har_kmeans_update's cost, converged = iterations > 0 and |loglik -
// hist[iterations - 1]| <= tol, iterations += 1.  Otherwise nothing changes.
typedef struct GmmControlArgs {
  const double* part;
  int npart, max_iter;
  double tol;
  int* state;
  double* hist;  // [max_iter]
} GmmControlArgs;
int har_gmm_control(const GmmControlArgs* a, hipStream_t s);

// ---- CSV on device (4 KiB chunks per workgroup) ----
int har_csv_count_newlines(const uint8_t* buf, int64_t n, int32_t* counts, hipStream_t s);
int har_csv_newline_pos(const uint8_t* buf, int64_t n, const int64_t* block_off, int64_t* pos, hipStream_t s);
// Per (col, row) outputs ([ncols][nrows]): fp64 value (NaN if not numeric), FNV-1a hash,
// flags (bit0 present, bit1 int literal, bit2 float literal, bit3 quoted), byte span.
int har_csv_parse_rows(const uint8_t* buf, const int64_t* starts, const int64_t* ends, int64_t nrows, int ncols,
                       double* vals, uint64_t* hashes, uint8_t* flags, int64_t* fstart, int32_t* flen,
                       hipStream_t s);

#ifdef __cplusplus
}
#endif
