// pybind11 module `_har_native`: host runtime (CSV parser) + kernel launchers.
//
// Launchers take device pointers and the HIP stream as integers (the Python
// side passes `tensor.data_ptr()` and `torch.cuda.current_stream().cuda_stream`),
// so this translation unit needs neither torch nor HIP device headers and the
// kernels stay capturable into hipGraphs.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "har_kernels.h"
#include "host/csv_parser.h"

namespace py = pybind11;
using u = uintptr_t;

template <typename T>
static T* P(u x) { return reinterpret_cast<T*>(x); }
static hipStream_t S(u x) { return reinterpret_cast<hipStream_t>(x); }

static void check(int rc, const char* what) {
  if (rc != 0) {
    std::string msg = std::string(what) + " failed: ";
    if (rc > 0) msg += hipGetErrorString((hipError_t)rc);
    else msg += "contract violation code " + std::to_string(rc);
    throw std::runtime_error(msg);
  }
}

static py::dict csv_parse(py::bytes data, bool header, int threads) {
  std::string_view sv;
  char* ptr;
  Py_ssize_t len;
  PyBytes_AsStringAndSize(data.ptr(), &ptr, &len);
  har::CsvResult r;
  {
    py::gil_scoped_release nogil;
    r = har::parse_csv(ptr, (size_t)len, header, threads);
  }
  py::dict out;
  out["names"] = r.names;
  out["kinds"] = r.kinds;
  py::list dbl, ints, miss, strs;
  for (int j = 0; j < r.ncols; ++j) {
    py::array_t<double> d(r.nrows);
    std::memcpy(d.mutable_data(), r.doubles[j].data(), sizeof(double) * r.nrows);
    py::array_t<int64_t> i(r.nrows);
    std::memcpy(i.mutable_data(), r.ints[j].data(), sizeof(int64_t) * r.nrows);
    py::array_t<bool> m(r.nrows);
    auto* mp = m.mutable_data();
    for (int64_t k = 0; k < r.nrows; ++k) mp[k] = r.missing[j][k] != 0;
    dbl.append(d);
    ints.append(i);
    miss.append(m);
    py::list s;
    if (r.kinds[j] == "string") {
      for (int64_t k = 0; k < r.nrows; ++k) {
        if (r.missing[j][k]) s.append(py::none());
        else s.append(py::str(r.field(j, k)));
      }
    }
    strs.append(s);
  }
  out["doubles"] = dbl;
  out["ints"] = ints;
  out["missing"] = miss;
  out["strings"] = strs;
  out["nrows"] = r.nrows;
  return out;
}

static GemmParams make_gemm(u A, u B, u C, u bias, u mask, u rowsum, int M, int N, int K, int lda, int ldb,
                            int ldc, int ldmask, int k_split, int tile, int64_t slab_stride,
                            int64_t slab_stride_rowsum, float alpha) {
  GemmParams p;
  p.A = P<const void>(A);
  p.B = P<const void>(B);
  p.C = P<void>(C);
  p.bias = P<const float>(bias);
  p.mask = P<const void>(mask);
  p.rowsum = P<float>(rowsum);
  p.M = M; p.N = N; p.K = K;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ldmask = ldmask;
  p.k_split = k_split;
  p.tile = tile;
  p.slab_stride = slab_stride;
  p.slab_stride_rowsum = slab_stride_rowsum;
  p.alpha = alpha;
  return p;
}

#ifndef HAR_SOURCE_HASH
#define HAR_SOURCE_HASH "unknown"
#endif

static QnArgs qn_args_from_dict(py::dict d) {
  auto I = [&](const char* k) { return d[k].cast<int64_t>(); };
  auto U = [&](const char* k) { return d[k].cast<u>(); };
  QnArgs a;
  a.B = (int)I("B");
  a.T = (int)I("T");
  a.K = (int)I("K");
  a.F = (int)I("F");
  a.m = (int)I("m");
  a.head = (int)I("head");
  a.filled = (int)I("filled");
  a.init = (int)I("init");
  a.nch = (int)I("nch");
  a.fin_it = (int)I("fin_it");
  a.D = I("D");
  a.x = P<float>(U("x"));
  a.g = P<float>(U("g"));
  a.fobj = P<double>(U("fobj"));
  a.l1 = P<const float>(U("l1"));
  a.l2 = P<const float>(U("l2"));
  a.pmask = P<const float>(U("pmask"));
  a.inv_std = P<const float>(U("inv_std"));
  a.S = P<float>(U("S"));
  a.Y = P<float>(U("Y"));
  a.rho = P<double>(U("rho"));
  a.SY = P<double>(U("SY"));
  a.YY = P<double>(U("YY"));
  a.P1 = P<double>(U("P1"));
  a.P2 = P<double>(U("P2"));
  a.P3 = P<double>(U("P3"));
  a.xtrial = P<float>(U("xtrial"));
  a.weff = P<float>(U("weff"));
  a.reg = P<double>(U("reg"));
  a.decr = P<double>(U("decr"));
  a.G = P<const float>(U("G"));
  a.loss = P<const double>(U("loss"));
  a.step_scale = P<float>(U("step_scale"));
  a.active = P<int32_t>(U("active"));
  a.fails = P<int32_t>(U("fails"));
  a.iters = P<int32_t>(U("iters"));
  a.steep = P<int32_t>(U("steep"));
  a.pick = P<int32_t>(U("pick"));
  a.hist = P<double>(U("hist"));
  a.done = P<int32_t>(U("done"));
  a.c1 = d["c1"].cast<double>();
  a.tol = d["tol"].cast<double>();
  return a;
}

// The pointer / shape fields of a solve's L-BFGS arguments, converted from the Python dict ONCE per
// solve; each phase launch then passes only the iteration scalars (a dict conversion per launch cost
// ~20 us of host time, three launches per iteration).
struct QnArgsHolder {
  QnArgs a;
};

// The evaluate / gradient launches' arguments as ops/logreg.py holds them: one tuple per launch, in
// the order below, ending (evaluate) or followed (gradient: before the column blocks) by KP and the
// number of models.  Every entry point converts through these two.
static LogregEvalArgs eval_args(py::tuple e, int& KP, int& n_models) {
  if (e.size() != 21) throw std::runtime_error("logreg evaluate arguments: 21 fields expected");
  auto U = [&](int i) { return e[i].cast<u>(); };
  auto I = [&](int i) { return e[i].cast<int64_t>(); };
  LogregEvalArgs a;
  a.dense = P<const float>(U(0));
  a.ldd = I(1);
  a.Fd = (int)I(2);
  a.dense_cols = P<const int32_t>(U(3));
  a.cat = P<const int32_t>(U(4));
  a.C = (int)I(5);
  a.y = P<const int32_t>(U(6));
  a.rw = P<const float>(U(7));
  a.inv_wsum = P<const float>(U(8));
  a.W = P<const float>(U(9));
  a.N = I(10);
  a.F = (int)I(11);
  a.K = (int)I(12);
  a.T = (int)I(13);
  a.tstride = (int)I(14);
  a.model0 = (int)I(15);
  a.mode = (int)I(16);
  a.R = P<float>(U(17));
  a.slab = P<float>(U(18));
  KP = (int)I(19);
  n_models = (int)I(20);
  return a;
}

static LogregGradArgs grad_args(py::tuple g, int& KP, int& n_models) {
  if (g.size() != 25) throw std::runtime_error("logreg gradient arguments: 25 fields expected");
  auto U = [&](int i) { return g[i].cast<u>(); };
  auto I = [&](int i) { return g[i].cast<int64_t>(); };
  LogregGradArgs a;
  a.slab = P<const float>(U(0));
  a.R = P<const float>(U(1));
  a.col_map = P<const int32_t>(U(2));
  a.csc_rows = P<const int32_t>(U(3));
  a.csc_off = P<const int32_t>(U(4));
  a.col_slice = P<const int32_t>(U(5));
  a.SL = (int)I(6);
  a.inv_std = P<const float>(U(7));
  a.pmask = P<const float>(U(8));
  a.N = I(9);
  a.F = (int)I(10);
  a.Fd = (int)I(11);
  a.K = (int)I(12);
  a.T = (int)I(13);
  a.tstride = (int)I(14);
  a.model0 = (int)I(15);
  a.ntiles = (int)I(16);
  a.G = P<float>(U(17));
  a.loss = P<double>(U(18));
  a.loss_fx = P<float>(U(19));
  KP = (int)I(20);
  n_models = (int)I(21);
  a.col_blk = P<const int32_t>(U(22));
  a.nblk = (int)I(23);
  a.srow = P<const int32_t>(U(24));
  return a;
}

// One launch chunk of a LogisticRegression objective evaluation: the evaluate + gradient kernels'
// arguments (pointers fixed for the life of a DeviceLogregSolver).
struct LogregEvalChunk {
  LogregEvalArgs ev;
  LogregGradArgs gr;
  int KP, n_models;
};

// The whole device L-BFGS / OWL-QN solve of a fit as ONE host call (no convergence poll, no
// collective): the same launch sequence as ops/logreg.py DeviceLogregSolver.solve enqueues from
// Python, minus ~60 pybind round trips per fit (the host, not the GPU, bounded a WISDM fit).
struct LogregSolvePlan {
  QnArgs q;
  std::vector<LogregEvalChunk> evT, ev1;  // evaluations of the T trials (first) / 1 per model
  int KP = 8;
};

static void logreg_solve_run(LogregSolvePlan& p, int max_iter, int m, hipStream_t s) {
  auto phase = [&](int ph, int head, int filled, int init, int fin_it) {
    QnArgs a = p.q;
    a.head = head;
    a.filled = filled;
    a.init = init;
    a.fin_it = fin_it;
    check(har_lbfgs_phase(&a, p.KP, ph, s), "lbfgs_phase");
  };
  auto evaluate = [&](const std::vector<LogregEvalChunk>& v) {
    for (const auto& c : v) {
      check(har_logreg_eval(&c.ev, c.KP, c.n_models, s), "logreg_eval");
      check(har_logreg_grad(&c.gr, c.KP, c.n_models, s), "logreg_grad");
    }
  };
  phase(1, 0, 0, 1, 0);
  evaluate(p.evT);
  phase(2, 0, 0, 1, 0);
  int head = 0, filled = 0;
  for (int it = 0; it < max_iter; ++it) {
    phase(1, head, filled, 0, 0);
    evaluate(p.ev1);
    phase(2, head, filled, 0, it + 1);
    head = (head + 1) % m;
    filled = filled + 1 < m ? filled + 1 : m;
  }
}

// The flagship MLP training step as ONE host call: the buffers of an engine never move, so their
// pointers, the gradient-reduction regions and the Adam hyper-parameters are fixed once per (engine,
// batch size) and run() enqueues mlp_step_fwd -> mlp_step_bwd -> grad_reduce_adam with only the batch
// pointers changing (three pybind calls with ~20 arguments each and a region list rebuilt in Python
// every step were ~10 us of host time per 70 us step: enough to starve the GPU when not graph-captured).
struct MlpStepPlan {
  u Wf, b0, b1, Wo, bo, dact2, fslab, bloss, bcorr, gw1, gw0, gb0, gb1, step, G, Pw, m, v, Pb;
  int K0, H, C, fslab_w;
  MlpFragSpec frag;
  u gwo, gbo;
  int64_t stride, n;
  float lr, b1c, b2c, eps, wd;
  std::vector<const float*> src;
  std::vector<int64_t> start, len, lds;
  std::vector<int> S;
  u pf_sink = 0;  // 4-byte scratch word of the prefetch workgroups (set once by the engine)
  // mode: 1 reduce + Adam (N = 1), 2 reduce + store G (DP, before the all-reduce), 4 Adam from G;
  // pf / pf_bytes (and pf1 / pf1_bytes): the next step's input rows (and labels), read by the reduction
  // launch's prefetch workgroups
  void run(u X, u y, int B, float scale, int mode, u stream, u pf, int64_t pf_bytes, u pf1, int64_t pf1_bytes) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mode & 3) {
      check(har_mlp_step_fwd(P<const uint16_t>(X), K0, P<uint16_t>(Wf), P<const float>(b0), P<const float>(b1), H,
                             P<const uint16_t>(Wo), P<const float>(bo), P<const int32_t>(y), B, C, scale,
                             P<uint16_t>(dact2), P<float>(fslab), P<float>(bloss), P<int32_t>(bcorr), s),
            "mlp_step_fwd");
      check(har_mlp_step_bwd(P<const uint16_t>(dact2), P<const uint16_t>(X), K0, P<const uint16_t>(Wf), H,
                             P<const float>(b0), B, P<float>(gw1), P<float>(gw0), P<float>(gb0), P<float>(gb1),
                             stride, P<int32_t>(step), P<const float>(fslab), fslab_w, P<float>(gwo), P<float>(gbo), s),
            "mlp_step_bwd");
    }
    const int gm = mode == 1 ? 1 | 4 : mode == 2 ? 1 | 2 : 4;  // GR_REDUCE 1, GR_STORE 2, GR_ADAM 4
    const int k = (gm & 1) ? (int)src.size() : 0;
    check(har_grad_reduce_adam(k, src.data(), start.data(), len.data(), lds.data(), S.data(), n, P<float>(G),
                               P<float>(Pw), P<float>(m), P<float>(v), P<uint16_t>(Pb), lr, b1c, b2c, eps, wd,
                               P<int32_t>(step), 0, gm, &frag, s, pf && pf_sink ? P<const void>(pf) : nullptr,
                               pf_bytes, P<uint32_t>(pf_sink), P<const void>(pf1), pf1_bytes),
          "grad_reduce_adam");
  }
};

PYBIND11_MODULE(_har_native, m) {
  m.doc() = "har native runtime: host CSV parser + gfx950 HIP kernel launchers";
  // content hash of every source / header / flag the library was built from (tools/build_native.py);
  // ops/_native.py refuses a library whose hash differs from the tree it is imported from
  m.def("source_hash", []() { return std::string(HAR_SOURCE_HASH); });
  m.def("csv_parse", &csv_parse, py::arg("data"), py::arg("header") = true, py::arg("threads") = 0);

  m.def("gemm", [](bool bf16, int layout, int epi, u A, u B, u C, u bias, u mask, u rowsum, int M, int N, int K,
                   int lda, int ldb, int ldc, int ldmask, int k_split, int tile, int64_t slab_stride,
                   int64_t slab_stride_rowsum, float alpha, u stream) {
    GemmParams p = make_gemm(A, B, C, bias, mask, rowsum, M, N, K, lda, ldb, ldc, ldmask, k_split, tile, slab_stride,
                             slab_stride_rowsum, alpha);
    check(bf16 ? har_gemm_bf16(&p, layout, epi, S(stream)) : har_gemm_f32(&p, layout, epi, S(stream)), "gemm");
  });

  m.def("softmax_ce_head_blocks", &har_softmax_ce_head_blocks);
  m.def("softmax_ce_head", [](u H, u W, u bias, u labels, int B, int D, int C, float scale, u dlogits,
                              u block_loss, u block_correct, u logits_out, u stream) {
    check(har_softmax_ce_head(P<const uint16_t>(H), P<const uint16_t>(W), P<const float>(bias),
                              P<const int32_t>(labels), B, D, C, scale, P<uint16_t>(dlogits), P<float>(block_loss),
                              P<int32_t>(block_correct), P<float>(logits_out), S(stream)),
          "softmax_ce_head");
  });

  m.def("adam_step", [](u param, u grad, u slabs, int nslabs, u mm, u vv, u pb, int64_t n, float lr, float b1,
                        float b2, float eps, float wd, float gs, u step, u stream, int tick) {
    check(har_adam_step(P<float>(param), P<const float>(grad), P<const float>(slabs), nslabs, P<float>(mm),
                        P<float>(vv), P<uint16_t>(pb), n, lr, b1, b2, eps, wd, gs, P<int32_t>(step), tick, S(stream)),
          "adam_step");
  });

  m.def("reduce_slabs", [](u slabs, int nslabs, int64_t n, u dst, u stream) {
    check(har_reduce_slabs(P<const float>(slabs), nslabs, n, P<float>(dst), S(stream)), "reduce_slabs");
  });

  m.def("logreg_eval_tiles", &har_logreg_eval_tiles);
  m.def("logreg_eval", [](py::tuple e, u stream) {
    int KP, n_models;
    const LogregEvalArgs a = eval_args(e, KP, n_models);
    check(har_logreg_eval(&a, KP, n_models, S(stream)), "logreg_eval");
  });
  // argument holder for logreg_solve_plan: one launch chunk's evaluate + gradient tuples
  py::class_<LogregEvalChunk>(m, "LogregEvalChunk");
  m.def("logreg_eval_chunk", [](py::tuple e, py::tuple g) {
    LogregEvalChunk c{};
    int KP, n_models;
    c.ev = eval_args(e, c.KP, c.n_models);
    c.gr = grad_args(g, KP, n_models);
    if (KP != c.KP || n_models != c.n_models) throw std::runtime_error("logreg_eval_chunk: KP / n mismatch");
    return c;
  });
  py::class_<LogregSolvePlan>(m, "LogregSolvePlan");
  m.def("logreg_solve_plan", [](const QnArgsHolder& h, std::vector<LogregEvalChunk> evT,
                                std::vector<LogregEvalChunk> ev1, int KP) {
    LogregSolvePlan p;
    p.q = h.a;
    p.evT = std::move(evT);
    p.ev1 = std::move(ev1);
    p.KP = KP;
    return p;
  });
  m.def("logreg_solve", [](LogregSolvePlan& p, int max_iter, int m, u stream) {
    logreg_solve_run(p, max_iter, m, S(stream));
  });
  m.def("lr_set_stamps", [](uint64_t ev, uint64_t dir, uint64_t upd, uint64_t grd) {
    har_lr_set_stamps(reinterpret_cast<uint64_t*>(ev), reinterpret_cast<uint64_t*>(dir), reinterpret_cast<uint64_t*>(upd),
                      reinterpret_cast<uint64_t*>(grd));
  });
  m.def("logreg_grad", [](py::tuple g, u stream) {
    int KP, n_models;
    const LogregGradArgs a = grad_args(g, KP, n_models);
    check(har_logreg_grad(&a, KP, n_models, S(stream)), "logreg_grad");
  });
  m.def("logreg_col_slices", [](u csc_off, int F, int SL, u col_slice, u stream) {
    check(har_logreg_col_slices(P<const int32_t>(csc_off), F, SL, P<int32_t>(col_slice), S(stream)),
          "logreg_col_slices");
  });
  m.def("logreg_summary_tiles", &har_logreg_summary_tiles);
  m.def("logreg_summary", [](int phase, u dense, int64_t ldd, int Fd, u y, u rw, int64_t N, int F, int K, int nspec,
                             u col_map, u csc_rows, u csc_off, u col_slice, int SL, int ntiles, u part, u summ,
                             u srow, u stream) {
    LogregSummaryArgs a;
    a.srow = P<const int32_t>(srow);
    a.dense = P<const float>(dense);
    a.ldd = ldd;
    a.Fd = Fd;
    a.y = P<const int32_t>(y);
    a.rw = P<const float>(rw);
    a.N = N;
    a.F = F;
    a.K = K;
    a.S = nspec;
    a.col_map = P<const int32_t>(col_map);
    a.csc_rows = P<const int32_t>(csc_rows);
    a.csc_off = P<const int32_t>(csc_off);
    a.col_slice = P<const int32_t>(col_slice);
    a.SL = SL;
    a.ntiles = ntiles;
    a.part = P<double>(part);
    a.summ = P<double>(summ);
    check(har_logreg_summary(&a, phase, S(stream)), "logreg_summary");
  });
  m.def("logreg_prepare", [](u summ, u reg, u alpha, int B, int F, int K, int Kp, int standardization,
                             int fit_intercept, int binomial, u inv_std, u inv_wsum, u pmask, u l2, u l1, u x0,
                             u stream) {
    LogregPrepareArgs a;
    a.summ = P<const double>(summ);
    a.reg = P<const float>(reg);
    a.alpha = P<const float>(alpha);
    a.B = B;
    a.F = F;
    a.K = K;
    a.Kp = Kp;
    a.standardization = standardization;
    a.fit_intercept = fit_intercept;
    a.binomial = binomial;
    a.inv_std = P<float>(inv_std);
    a.inv_wsum = P<float>(inv_wsum);
    a.pmask = P<float>(pmask);
    a.l2 = P<float>(l2);
    a.l1 = P<float>(l1);
    a.x0 = P<float>(x0);
    check(har_logreg_prepare(&a, S(stream)), "logreg_prepare");
  });
  m.def("logreg_loss_decode", [](u fx, u loss, int n, u stream) {
    check(har_logreg_loss_decode(P<const float>(fx), P<double>(loss), n, S(stream)), "logreg_loss_decode");
  });
  // one L-BFGS phase (logreg_qn.hip: 1 direction + trials, 2 pick + history + the next direction's
  // dots, finalized by the model's last chunk); the QnArgs fields come from a dict of ints / floats /
  // device pointers
  m.def("qn_chunks", &har_qn_chunks);
  m.def("lbfgs_phase", [](int phase, py::dict d, int KP, u stream) {
    QnArgs a = qn_args_from_dict(d);
    check(har_lbfgs_phase(&a, KP, phase, S(stream)), "lbfgs_phase");
  });
  py::class_<QnArgsHolder>(m, "QnArgs");
  m.def("qn_args", [](py::dict d) { return QnArgsHolder{qn_args_from_dict(d)}; });
  m.def("lbfgs_phase_h", [](const QnArgsHolder& h, int phase, int head, int filled, int init, int fin_it, int KP,
                            u stream) {
    QnArgs a = h.a;
    a.head = head;
    a.filled = filled;
    a.init = init;
    a.fin_it = fin_it;
    check(har_lbfgs_phase(&a, KP, phase, S(stream)), "lbfgs_phase");
  });

  m.def("value_counts_max_v", &har_value_counts_max_v);
  m.def("value_counts", [](u codes, int64_t n, int V, u out, u stream) {
    check(har_value_counts(P<const int64_t>(codes), n, V, P<int64_t>(out), S(stream)), "value_counts");
  });
  m.def("confusion_matrix", [](u label, u pred, int64_t n, int K, u cm, u stream) {
    check(har_confusion_matrix(P<const int32_t>(label), P<const int32_t>(pred), n, K, P<int64_t>(cm), S(stream)),
          "confusion_matrix");
  });

  m.def("regression_moments", [](u y, u yh, int64_t n, u out, u stream) {
    check(har_regression_moments(P<const float>(y), P<const float>(yh), n, P<double>(out), S(stream)),
          "regression_moments");
  });

  m.def("tree_dp_pack", [](u store, int A, int64_t slot, int mb, int K, u cls, u kp, u bw, u woff, u out, u stream) {
    check(har_tree_dp_pack(P<const float>(store), A, slot, mb, K, P<const int32_t>(cls), P<const int32_t>(kp),
                           P<const int32_t>(bw), P<const int64_t>(woff), P<int32_t>(out), S(stream)),
          "tree_dp_pack");
  });
  m.def("tree_dp_unpack", [](u in, int a0, int n, int64_t slot, int mb, int K, u cls, u kp, u bw, u woff,
                             int64_t base, u local, u stream) {
    check(har_tree_dp_unpack(P<const int32_t>(in), a0, n, slot, mb, K, P<const int32_t>(cls), P<const int32_t>(kp),
                             P<const int32_t>(bw), P<const int64_t>(woff), base, P<float>(local), S(stream)),
          "tree_dp_unpack");
  });
  m.def("confusion_matrix_batched", [](u label, u pred, u mask, int64_t n, int B, int K, u cm, u stream) {
    check(har_confusion_matrix_batched(P<const int32_t>(label), P<const int32_t>(pred), P<const uint8_t>(mask), n, B,
                                       K, P<int64_t>(cm), S(stream)),
          "confusion_matrix_batched");
  });
  m.def("roc_pr_sums_batched", [](u s, u y, u ns, int B, int64_t ld, u out, u stream) {
    check(har_roc_pr_sums_batched(P<const float>(s), P<const float>(y), P<const int32_t>(ns), B, ld, P<double>(out),
                                  S(stream)),
          "roc_pr_sums_batched");
  });
  m.def("roc_pr_sums", [](u s, u y, int64_t n, u out, u stream) {
    check(har_roc_pr_sums(P<const float>(s), P<const float>(y), n, P<double>(out), S(stream)), "roc_pr_sums");
  });

  m.def("tree_hist_split", [](u bins, int64_t N, int F, int row_major, u nbins, u rows, u row_w, u node_start, u node_count, int A,
                              u feats, int m, int fc, u label, int K, int maxbins, float min_inst, float min_gain,
                              int impurity, u gain, u feat, u bin, u left, u total, int mode, u ghist, int row_chunks,
                              u cat, int ncat, u onehot, u stream) {
    const TreeSparse sp{P<const int32_t>(cat), ncat, P<const uint8_t>(onehot), F};
    check(har_tree_hist_split(P<const uint8_t>(bins), N, F, row_major, P<const int32_t>(nbins), P<const int32_t>(rows),
                              P<const float>(row_w), P<const int32_t>(node_start), P<const int32_t>(node_count), A,
                              P<const int32_t>(feats), m, fc, P<const int32_t>(label), K, maxbins, min_inst, min_gain,
                              impurity, P<float>(gain), P<int32_t>(feat), P<int32_t>(bin), P<float>(left),
                              P<float>(total), mode, P<float>(ghist), row_chunks, cat ? &sp : nullptr, S(stream)),
          "tree_hist_split");
  });

  m.def("tree_plan", [](u counts, int A, int prows, u plan, int64_t slot_elems, u ghist, int max_big, int by_node,
                        u a_dev, u stream) {
    check(har_tree_plan(P<const int32_t>(counts), A, prows, P<int32_t>(plan), slot_elems, P<float>(ghist), max_big,
                        by_node, P<const int32_t>(a_dev), S(stream)),
          "tree_plan");
  });
  m.def("tree_hist_split_planned", [](u bins, int64_t N, int F, int row_major, u nbins, u rows, u row_w, u node_start,
                                      u node_count, int A, u feats, int m, int fc, u label, int K, int maxbins,
                                      float min_inst, float min_gain, int impurity, u gain, u feat, u bin, u left,
                                      u total, int mode, u ghist, u plan, int prows, int bound, int by_node,
                                      u hprev, u derive_from, u parent_of, u cat, int ncat, u onehot, u stream) {
    const TreeSparse sp{P<const int32_t>(cat), ncat, P<const uint8_t>(onehot), F};
    check(har_tree_hist_split_planned(P<const uint8_t>(bins), N, F, row_major, P<const int32_t>(nbins),
                                      P<const int32_t>(rows), P<const float>(row_w), P<const int32_t>(node_start),
                                      P<const int32_t>(node_count), A, P<const int32_t>(feats), m, fc,
                                      P<const int32_t>(label), K, maxbins, min_inst, min_gain, impurity,
                                      P<float>(gain), P<int32_t>(feat), P<int32_t>(bin), P<float>(left),
                                      P<float>(total), mode, P<float>(ghist), 1, P<const int32_t>(plan), prows, bound,
                                      by_node, P<const float>(hprev), P<const int32_t>(derive_from),
                                      P<const int32_t>(parent_of), cat ? &sp : nullptr, S(stream)),
          "tree_hist_split_planned");
  });

  m.def("forest_predict", [](u X, int64_t n, int F, int ld, u feat, u thr, u left, u right, u leaf, int T, int maxn,
                             int K, int max_depth, int normalize, u out, u stream) {
    check(har_forest_predict(P<const float>(X), n, F, ld, P<const int32_t>(feat), P<const float>(thr),
                             P<const int32_t>(left), P<const int32_t>(right), P<const float>(leaf), T, maxn, K,
                             max_depth, normalize, P<float>(out), S(stream)),
          "forest_predict");
  });

  m.def("tree_init", [](uint64_t seed, int tree0, int ntrees, int64_t row0, int64_t n, std::vector<uint32_t> cdf,
                        u rw, u y, int K, u W, u node_of, u stats, int64_t stride, u bad, u stream) {
    check(har_tree_init(seed, tree0, ntrees, row0, n, cdf.data(), (int)cdf.size(), P<const float>(rw),
                        P<const int32_t>(y), K, P<float>(W), P<int32_t>(node_of), P<float>(stats), stride,
                        P<int32_t>(bad), S(stream)),
          "tree_init");
  });
  m.def("sort_columns", [](u X, int n, int F, int ld, u out, u stream) {
    check(har_sort_columns(P<const float>(X), n, F, ld, P<float>(out), S(stream)), "sort_columns");
  });
  m.def("find_splits_post_sort", [](u sorted, int F, int n, int ns, u out, u stream) {
    check(har_find_splits_post_sort(P<const float>(sorted), F, n, ns, P<float>(out), S(stream)),
          "find_splits_post_sort");
  });
  m.def("poisson_bootstrap", [](uint64_t seed, int tree0, int ntrees, int64_t row0, int64_t n, u out, u stream) {
    check(har_poisson_bootstrap(seed, tree0, ntrees, row0, n, P<uint8_t>(out), S(stream)), "poisson_bootstrap");
  });

  m.def("philox_buckets", [](uint64_t seed, uint32_t stream_id, int64_t row0, int64_t n, u thr, int nthr, u out,
                             u stream) {
    check(har_philox_buckets(seed, stream_id, row0, n, P<const uint32_t>(thr), nthr, P<int32_t>(out), S(stream)),
          "philox_buckets");
  });

  m.def("window_features_mlp", [](u stream, int64_t n_samples, int axes, int window, int stride, int64_t n_windows,
                                  float hz, u mean, u inv_std, float nan_value, u out, int ld_out, u stream_) {
    check(har_window_features_mlp(P<const float>(stream), n_samples, axes, window, stride, n_windows, hz,
                                  P<const float>(mean), P<const float>(inv_std), nan_value, P<uint16_t>(out), ld_out,
                                  S(stream_)),
          "window_features_mlp");
  });
  m.def("window_features", [](u stream, int64_t n_samples, int axes, int window, int stride, int64_t n_windows,
                              float hz, int nbins, u out, int ld_out, u st) {
    check(har_window_features(P<const float>(stream), n_samples, axes, window, stride, n_windows, hz, nbins,
                              P<float>(out), ld_out, S(st)),
          "window_features");
  });
  m.def("spectral_features", [](u stream, int64_t n_samples, int axes, int window, int stride, int64_t n_windows,
                                float hz, u out, int ld_out, int col0, u st) {
    check(har_spectral_features(P<const float>(stream), n_samples, axes, window, stride, n_windows, hz, P<float>(out),
                                ld_out, col0, S(st)),
          "spectral_features");
  });
  m.def("spectral_features_mlp", [](u stream, int64_t n_samples, int axes, int window, int stride, int64_t n_windows,
                                    float hz, u mean, u inv_std, u out, int ld_out, int col0, u st) {
    check(har_spectral_features_mlp(P<const float>(stream), n_samples, axes, window, stride, n_windows, hz,
                                    P<const float>(mean), P<const float>(inv_std), P<uint16_t>(out), ld_out, col0,
                                    S(st)),
          "spectral_features_mlp");
  });
  m.def("spectral_max_window", []() { return har_spectral_max_window(); });
  m.def("rocket_features", [](u stream, int64_t n_samples, int axes, int window, int stride, int64_t n_windows,
                              int n_dil, int q, u masks, u biases, u out, int ld_out, int col0, u counts, u st) {
    check(har_rocket_features(P<const float>(stream), n_samples, axes, window, stride, n_windows, n_dil, q,
                              P<const int>(masks), P<const float>(biases), P<float>(out), ld_out, col0,
                              P<int>(counts), S(st)),
          "rocket_features");
  });
  m.def("rocket_max_window", [](int axes) { return har_rocket_max_window(axes); });

  // gradient-boosted trees (gbt.hip)
  m.def("gbt_grad", [](u margins, u y, u w, int64_t N, int K, u qgh, u block_loss, u st) {
    check(har_gbt_grad(P<const float>(margins), P<const int32_t>(y), P<const int32_t>(w), N, K, P<int32_t>(qgh),
                       P<double>(block_loss), S(st)),
          "gbt_grad");
  });
  m.def("gbt_grad_blocks", [](int64_t N, int K) { return har_gbt_grad_blocks(N, K); });
  m.def("gbt_hist", [](u bins, u qgh, u w, u node_of, int64_t N, int F, int K, int maxb, int level, u hist, u st) {
    check(har_gbt_hist(P<const uint8_t>(bins), P<const int32_t>(qgh), P<const int32_t>(w), P<const int32_t>(node_of), N,
                       F, K, maxb, level, P<int64_t>(hist), S(st)),
          "gbt_hist");
  });
  m.def("gbt_hist_rows_per_block", []() { return har_gbt_hist_rows_per_block(); });
  m.def("gbt_split", [](u hist, u nbins, u thr_mat, int F, int K, int maxb, int ldthr, int level, int tree0, int maxn,
                        double lambda, double step, double min_gain, int64_t min_inst, u o_feat, u o_bin, u o_gain,
                        u o_sums, u feature, u split_bin, u thresh, u left, u right, u gains, u value, u stats, u st) {
    GbtSplitArgs a{};
    a.hist = P<const int64_t>(hist);
    a.nbins = P<const int32_t>(nbins);
    a.thr_mat = P<const float>(thr_mat);
    a.F = F; a.K = K; a.maxb = maxb; a.ldthr = ldthr; a.level = level; a.tree0 = tree0; a.maxn = maxn;
    a.lambda = lambda; a.step = step; a.min_gain = min_gain; a.min_inst = min_inst;
    a.o_feat = P<int32_t>(o_feat); a.o_bin = P<int32_t>(o_bin); a.o_gain = P<double>(o_gain);
    a.o_sums = P<int64_t>(o_sums);
    a.feature = P<int32_t>(feature); a.split_bin = P<int32_t>(split_bin); a.thresh = P<float>(thresh);
    a.left = P<int32_t>(left); a.right = P<int32_t>(right); a.gains = P<float>(gains); a.value = P<float>(value);
    a.stats = P<float>(stats);
    check(har_gbt_split(&a, S(st)), "gbt_split");
  });
  m.def("gbt_partition", [](u node_of, u bins, u feature, u split_bin, int64_t N, int F, int K, int level, int tree0,
                            int maxn, u st) {
    check(har_gbt_partition(P<int32_t>(node_of), P<const uint8_t>(bins), P<const int32_t>(feature),
                            P<const int32_t>(split_bin), N, F, K, level, tree0, maxn, S(st)),
          "gbt_partition");
  });
  m.def("gbt_update", [](u margins, u node_of, u value, int64_t N, int K, int tree0, int maxn, u st) {
    check(har_gbt_update(P<float>(margins), P<const int32_t>(node_of), P<const float>(value), N, K, tree0, maxn, S(st)),
          "gbt_update");
  });

  // HMM smoothing (hmm.hip)
  m.def("hmm_chunk_len", []() { return har_hmm_chunk_len(); });
  m.def("hmm_scan_group", []() { return har_hmm_scan_group(); });
  m.def("hmm_workspace_bytes", [](int64_t T, int K, int64_t S, int L) { return har_hmm_workspace_bytes(T, K, S, L); });
  m.def("hmm_viterbi", [](u E, u A, u pi, u off, int64_t T, int K, int64_t nseq, int L, u ws, int64_t ws_bytes, u path,
                          u score, int phase_lo, int phase_hi, u st) {
    check(har_hmm_viterbi(P<const int32_t>(E), P<const int32_t>(A), P<const int32_t>(pi), P<const int64_t>(off), T, K, nseq,
                          L, P<void>(ws), ws_bytes, P<int32_t>(path), P<int64_t>(score), phase_lo, phase_hi, S(st)),
          "hmm_viterbi");
  });
  m.def("hmm_fb_workspace_bytes", [](int64_t T, int K, int64_t S, int L, bool want_xi) {
    return har_hmm_fb_workspace_bytes(T, K, S, L, want_xi ? 1 : 0);
  });
  m.def("hmm_forward_backward", [](u B, u Pm, u p0, u off, int64_t T, int K, int64_t nseq, int L, u ws, int64_t ws_bytes,
                                   u gamma, u loglik, u xi, int phase_lo, int phase_hi, int variant, u st) {
    check(har_hmm_forward_backward(P<const double>(B), P<const double>(Pm), P<const double>(p0), P<const int64_t>(off), T, K,
                                   nseq, L, P<void>(ws), ws_bytes, P<double>(gamma), P<double>(loglik), P<double>(xi),
                                   phase_lo, phase_hi, variant, S(st)),
          "hmm_forward_backward");
  });

  // IIR stream filters (sosfilt.hip)
  m.def("sosfilt_chunk_len", []() { return har_sosfilt_chunk_len(); });
  m.def("sosfilt_scan_group", []() { return har_sosfilt_scan_group(); });
  m.def("sosfilt_levels", [](int64_t S, int L, int G) { return har_sosfilt_levels(S, L, G); });
  m.def("sosfilt_workspace_bytes", [](int64_t S, int A, int ns, int L, int G) {
    return har_sosfilt_workspace_bytes(S, A, ns, L, G);
  });
  m.def("sosfilt", [](u x, u xc, u y, u seg, int64_t n, int64_t nseg, int A, int ns, int L, int G, int reverse,
                      int init_step, int mode, std::vector<double> sos, std::vector<double> zi, u powers, int levels, u ws,
                      int64_t ws_bytes, int phase_lo, int phase_hi, u st) {
    if (ns < 1 || ns > 4 || sos.size() != (size_t)ns * 5 || zi.size() != (size_t)ns * 2)
      throw std::runtime_error("sosfilt: sos must hold 5 and zi 2 values per section, 1..4 sections");
    SosFilterArgs a{};
    a.x = P<const float>(x);
    a.xc = P<const float>(xc);
    a.y = P<float>(y);
    a.seg = P<const int64_t>(seg);
    a.n_samples = n;
    a.n_seg = nseg;
    a.axes = A;
    a.sections = ns;
    a.L = L;
    a.G = G;
    a.reverse = reverse;
    a.init_step = init_step;
    a.mode = mode;
    for (int j = 0; j < ns; ++j) {
      for (int i = 0; i < 5; ++i) a.sos[j][i] = sos[j * 5 + i];
      for (int i = 0; i < 2; ++i) a.zi[j][i] = zi[j * 2 + i];
    }
    a.powers = P<const double>(powers);
    a.levels = levels;
    a.ws = P<void>(ws);
    a.ws_bytes = ws_bytes;
    a.phase_lo = phase_lo;
    a.phase_hi = phase_hi;
    check(har_sosfilt(&a, S(st)), "sosfilt");
  });

  // K-means and the silhouette (kmeans.hip)
  m.def("kmeans_rows_per_block", []() { return har_kmeans_rows_per_block(); });
  m.def("kmeans_max_k", []() { return har_kmeans_max_k(); });
  m.def("kmeans_max_d", []() { return har_kmeans_max_d(); });
  m.def("kmeans_plan", [](int D, int K) {
    int o[4] = {0, 0, 0, 0};
    check(har_kmeans_plan(D, K, o), "kmeans_plan");
    return std::vector<int>{o[0], o[1], o[2], o[3]};
  });
  m.def("kmeans_assign", [](u X, int64_t N, int D, int K, u C, u h, u w, u labels, u scale, u norm_scale, u assign,
                            u d2, u acc, u part, u st) {
    KMeansArgs a{};
    a.X = P<const float>(X);
    a.N = N;
    a.D = D;
    a.K = K;
    a.C = P<const float>(C);
    a.h = P<const float>(h);
    a.w = P<const int32_t>(w);
    a.labels = P<const int32_t>(labels);
    a.scale = P<const float>(scale);
    a.norm_scale = P<const double>(norm_scale);
    a.assign = P<int32_t>(assign);
    a.d2 = P<float>(d2);
    a.acc = P<int64_t>(acc);
    a.part = P<double>(part);
    check(har_kmeans_assign(&a, S(st)), "kmeans_assign");
  });
  m.def("kmeans_silhouette", [](u X, int64_t N, int D, int K, u M, u h, u labels, u cnt, u sil, u part, u st) {
    KMeansArgs a{};
    a.X = P<const float>(X);
    a.N = N;
    a.D = D;
    a.K = K;
    a.C = P<const float>(M);
    a.h = P<const float>(h);
    a.labels = P<const int32_t>(labels);
    a.cnt = P<const double>(cnt);
    a.sil = P<float>(sil);
    a.part = P<double>(part);
    check(har_kmeans_silhouette(&a, S(st)), "kmeans_silhouette");
  });
  m.def("kmeans_update", [](u acc, u scale, int K, int D, u cost, int ncost, int max_iter, double tol2, u C, u Cnew, u h,
                            u state, u cost_hist, u moved, u sizes, u st) {
    KMeansUpdateArgs a{};
    a.acc = P<int64_t>(acc);
    a.scale = P<const float>(scale);
    a.K = K;
    a.D = D;
    a.cost = P<const double>(cost);
    a.ncost = ncost;
    a.max_iter = max_iter;
    a.tol2 = tol2;
    a.C = P<float>(C);
    a.Cnew = P<float>(Cnew);
    a.h = P<float>(h);
    a.state = P<int32_t>(state);
    a.cost_hist = P<double>(cost_hist);
    a.moved = P<double>(moved);
    a.sizes = P<int64_t>(sizes);
    check(har_kmeans_update(&a, S(st)), "kmeans_update");
  });

  // Ridge classifier (ridge.hip)
  m.def("ridge_chunk_rows", []() { return har_ridge_chunk_rows(); });
  m.def("ridge_panel", []() { return har_ridge_panel(); });
  m.def("ridge_max_dim", []() { return har_ridge_max_dim(); });
  m.def("ridge_gram", [](u X, int64_t ldx, u y, u rows, u mean, u inv_std, std::vector<int64_t> off, int D, int K, int cps,
                         u slabs, u Af, u Aall, bool reduce, u st) {
    RidgeGramArgs a{};
    const int F = (int)off.size() - 1;
    if (F < 1 || F > HAR_RIDGE_MAX_FOLDS) check(-2, "ridge_gram");
    a.X = P<const float>(X);
    a.ldx = ldx;
    a.y = P<const int32_t>(y);
    a.rows = P<const int32_t>(rows);
    a.mean = P<const float>(mean);
    a.inv_std = P<const float>(inv_std);
    for (int f = 0; f <= F; ++f) a.off[f] = off[f];
    a.D = D;
    a.K = K;
    a.F = F;
    a.cps = cps;
    a.slabs = P<double>(slabs);
    a.Af = P<double>(Af);
    a.Aall = P<double>(Aall);
    if (reduce) check(har_ridge_gram_reduce(&a, S(st)), "ridge_gram_reduce");
    else check(har_ridge_gram(&a, S(st)), "ridge_gram");
  });
  m.def("ridge_solve", [](int step, u Af, u Aall, u alphas, int D, int K, int F, int nalpha, int sys0, int nsys, u Sys,
                          u info, u W64, u W, u b, u st) {
    RidgeSolveArgs a{};
    a.Af = P<const double>(Af);
    a.Aall = P<const double>(Aall);
    a.alphas = P<const double>(alphas);
    a.D = D;
    a.K = K;
    a.F = F;
    a.nalpha = nalpha;
    a.sys0 = sys0;
    a.nsys = nsys;
    a.Sys = P<double>(Sys);
    a.info = P<int32_t>(info);
    a.W64 = P<double>(W64);
    a.W = P<float>(W);
    a.b = P<float>(b);
    if (step == 0) check(har_ridge_systems(&a, S(st)), "ridge_systems");
    else if (step == 1) check(har_ridge_cholesky(&a, S(st)), "ridge_cholesky");
    else if (step == 2) check(har_ridge_backsolve(&a, S(st)), "ridge_backsolve");
    else check(-2, "ridge_solve");
  });

  // Exact k-nearest neighbours (knn.hip)
  m.def("knn_query_rows", []() { return har_knn_query_rows(); });
  m.def("knn_max_k", []() { return har_knn_max_k(); });
  m.def("knn_max_d", []() { return har_knn_max_d(); });
  m.def("knn_max_classes", []() { return har_knn_max_classes(); });
  m.def("knn_max_splits", []() { return har_knn_max_splits(); });
  m.def("knn_slab_rows", [](int D) {
    const int r = har_knn_slab_rows(D);
    check(r < 0 ? r : 0, "knn_slab_rows");
    return r;
  });
  m.def("knn_auto_splits", [](int64_t N, int64_t M, int D) {
    const int r = har_knn_auto_splits(N, M, D);
    check(r < 0 ? r : 0, "knn_auto_splits");
    return r;
  });
  m.def("knn_search", [](u Q, int64_t N, u R, u h, int64_t M, int D, int k, int splits, u qgroup, u rgroup, u ps, u pi,
                         u st) {
    KnnSearchArgs a{};
    a.Q = P<const float>(Q);
    a.N = N;
    a.R = P<const float>(R);
    a.h = P<const float>(h);
    a.M = M;
    a.D = D;
    a.k = k;
    a.splits = splits;
    a.qgroup = P<const int32_t>(qgroup);
    a.rgroup = P<const int32_t>(rgroup);
    a.ps = P<float>(ps);
    a.pi = P<int32_t>(pi);
    check(har_knn_search(&a, S(st)), "knn_search");
  });
  m.def("knn_merge_vote", [](u ps, u pi, int splits, u Q, int D, int64_t N, int k, int ldk, u idx, u d2, u y, int64_t M,
                             int C, int weights, u raw, u prob, u pred, u st) {
    KnnVoteArgs a{};
    a.ps = P<const float>(ps);
    a.pi = P<const int32_t>(pi);
    a.splits = splits;
    a.Q = P<const float>(Q);
    a.D = D;
    a.N = N;
    a.k = k;
    a.ldk = ldk;
    a.idx = P<int32_t>(idx);
    a.d2 = P<float>(d2);
    a.y = P<const int32_t>(y);
    a.M = M;
    a.C = C;
    a.weights = weights;
    a.raw = P<double>(raw);
    a.prob = P<double>(prob);
    a.pred = P<int32_t>(pred);
    check(har_knn_merge_vote(&a, S(st)), "knn_merge_vote");
  });

  // Banded dynamic time warping (dtw.hip)
  m.def("dtw_query_rows", []() { return har_dtw_query_rows(); });
  m.def("dtw_slab_rows", []() { return har_dtw_slab_rows(); });
  m.def("dtw_max_w", []() { return har_dtw_max_w(); });
  m.def("dtw_max_radius", []() { return har_dtw_max_radius(); });
  m.def("dtw_max_axes", []() { return har_dtw_max_axes(); });
  m.def("dtw_max_k", []() { return har_dtw_max_k(); });
  m.def("dtw_max_splits", []() { return har_dtw_max_splits(); });
  m.def("dtw_auto_splits", [](int64_t N, int64_t M) {
    const int r = har_dtw_auto_splits(N, M);
    check(r < 0 ? r : 0, "dtw_auto_splits");
    return r;
  });
  m.def("dtw_cost", [](u Q, int64_t N, u R, int64_t M, int W, int A, int radius, u cost, u st) {
    DtwArgs a{};
    a.Q = P<const float>(Q);
    a.N = N;
    a.R = P<const float>(R);
    a.M = M;
    a.W = W;
    a.A = A;
    a.radius = radius;
    a.cost = P<float>(cost);
    check(har_dtw_cost(&a, S(st)), "dtw_cost");
  });
  m.def("dtw_search", [](u Q, int64_t N, u R, int64_t M, int W, int A, int radius, int k, int splits, u qgroup, u rgroup,
                         u ps, u pi, u st) {
    DtwArgs a{};
    a.Q = P<const float>(Q);
    a.N = N;
    a.R = P<const float>(R);
    a.M = M;
    a.W = W;
    a.A = A;
    a.radius = radius;
    a.k = k;
    a.splits = splits;
    a.qgroup = P<const int32_t>(qgroup);
    a.rgroup = P<const int32_t>(rgroup);
    a.ps = P<float>(ps);
    a.pi = P<int32_t>(pi);
    check(har_dtw_search(&a, S(st)), "dtw_search");
  });
  m.def("dtw_merge", [](u ps, u pi, int splits, int64_t N, int k, u idx, u d2, u st) {
    DtwMergeArgs a{};
    a.ps = P<const float>(ps);
    a.pi = P<const int32_t>(pi);
    a.splits = splits;
    a.N = N;
    a.k = k;
    a.idx = P<int32_t>(idx);
    a.d2 = P<float>(d2);
    check(har_dtw_merge(&a, S(st)), "dtw_merge");
  });

  // Gaussian mixtures (gmm.hip)
  m.def("gmm_rows_per_block", []() { return har_gmm_rows_per_block(); });
  m.def("gmm_group", [](int D, int K) {
    const int g = har_gmm_group(D, K);
    if (g < 0) check(g, "gmm_group");
    return g;
  });
  m.def("gmm_grid", [](int64_t N, int D, int K, int max_blocks) {
    const int g = har_gmm_grid(N, D, K, max_blocks);
    if (g < 0) check(g, "gmm_grid");
    return g;
  });
  m.def("gmm_estep", [](u Z, int64_t N, int D, int K, u mu, u W, u c, u w, u resp, u lse, u pred, u q, u slabs, u part,
                        int max_blocks, u state, int max_iter, u wr, u st) {
    GmmEstepArgs a{};
    a.Z = P<const float>(Z);
    a.N = N;
    a.D = D;
    a.K = K;
    a.mu = P<const float>(mu);
    a.W = P<const float>(W);
    a.c = P<const float>(c);
    a.w = P<const float>(w);
    a.resp = P<float>(resp);
    a.lse = P<float>(lse);
    a.pred = P<int32_t>(pred);
    a.q = P<float>(q);
    a.slabs = P<float>(slabs);
    a.part = P<double>(part);
    a.max_blocks = max_blocks;
    a.state = P<const int>(state);
    a.max_iter = max_iter;
    a.wr = P<float>(wr);
    check(har_gmm_estep(&a, S(st)), "gmm_estep");
  });
  m.def("gmm_finish", [](u slabs, int nslab, int K, int D, int diag, int max_iter, double reg, u mu, u W, u c, u Nk, u pi,
                         u state, u st) {
    GmmFinishArgs a{};
    a.slabs = P<const float>(slabs);
    a.nslab = nslab;
    a.K = K;
    a.D = D;
    a.diag = diag;
    a.max_iter = max_iter;
    a.reg = reg;
    a.mu = P<float>(mu);
    a.W = P<float>(W);
    a.c = P<float>(c);
    a.Nk = P<double>(Nk);
    a.pi = P<double>(pi);
    a.state = P<const int>(state);
    check(har_gmm_finish(&a, S(st)), "gmm_finish");
  });
  m.def("gmm_control", [](u part, int npart, int max_iter, double tol, u state, u hist, u st) {
    GmmControlArgs a{};
    a.part = P<const double>(part);
    a.npart = npart;
    a.max_iter = max_iter;
    a.tol = tol;
    a.state = P<int>(state);
    a.hist = P<double>(hist);
    check(har_gmm_control(&a, S(st)), "gmm_control");
  });

  m.def("grad_reduce_adam", [](std::vector<u> src, std::vector<int64_t> start, std::vector<int64_t> len,
                               std::vector<int64_t> lds, std::vector<int> nsl, int64_t n, u G, u param, u mm, u vv,
                               u pb, float lr, float b1, float b2, float eps, float wd, u step, int tick, int mode,
                               u stream, u frag_dst, int64_t w0_off, int64_t w1_off, int fK0, int fH, int fw1t) {
    const MlpFragSpec frag{P<uint16_t>(frag_dst), w0_off, w1_off, fK0, fH, fw1t};
    const int k = (int)src.size();
    if ((int)start.size() != k || (int)len.size() != k || (int)lds.size() != k || (int)nsl.size() != k)
      throw std::runtime_error("grad_reduce_adam: region lists differ in length");
    std::vector<const float*> sp(k);
    for (int i = 0; i < k; ++i) sp[i] = P<const float>(src[i]);
    check(har_grad_reduce_adam(k, sp.data(), start.data(), len.data(), lds.data(), nsl.data(), n, P<float>(G),
                               P<float>(param), P<float>(mm), P<float>(vv), P<uint16_t>(pb), lr, b1, b2, eps, wd,
                               P<int32_t>(step), tick, mode, frag_dst ? &frag : nullptr, S(stream)),
          "grad_reduce_adam");
  }, py::arg("src"), py::arg("start"), py::arg("len"), py::arg("lds"), py::arg("nsl"), py::arg("n"), py::arg("G"),
     py::arg("param"), py::arg("m"), py::arg("v"), py::arg("pb"), py::arg("lr"), py::arg("b1"), py::arg("b2"),
     py::arg("eps"), py::arg("wd"), py::arg("step"), py::arg("tick"), py::arg("mode"), py::arg("stream"),
     py::arg("frag_dst") = 0, py::arg("w0_off") = 0, py::arg("w1_off") = 0, py::arg("fK0") = 0, py::arg("fH") = 0,
     py::arg("fw1t") = 0);
  // small-batch step: the fused tile kernel, then ONE region reduction of its B / 32 slabs + Adam that
  // refreshes Pb and all three fragment copies (mlp_small.hip)
  m.def("mlp_small_step_max_batch", &har_mlp_small_step_max_batch);
  m.def("mlp_small_step", [](u X, int K0, u Wf, u b0, u b1, int H, u Wo, u bo, u labels, int B, int C, float scale,
                             u slab, int64_t total, int64_t off_w0, int64_t off_b0, int64_t off_w1, int64_t off_b1,
                             int64_t off_wo, int64_t off_bo, u block_loss, u block_correct, u tick, u G, u param,
                             u mm, u vv, u pb, float lr, float b1c, float b2c, float eps, float wd, u step,
                             u stream) {
    const MlpSmallStepArgs a{P<const uint16_t>(X), P<const uint16_t>(Wf), P<const float>(b0), P<const float>(b1),
                             P<const uint16_t>(Wo), P<const float>(bo), P<const int32_t>(labels), B, C, scale,
                             P<float>(slab), total, off_w0, off_b0, off_w1, off_b1, off_wo, off_bo,
                             P<float>(block_loss), P<int32_t>(block_correct), P<int32_t>(tick)};
    check(har_mlp_small_step(&a, K0, H, S(stream)), "mlp_small_step");
    const float* src = P<const float>(slab);
    const int64_t start = 0;
    const int nsl = B / 32;
    const MlpFragSpec frag{P<uint16_t>(Wf), off_w0, off_w1, K0, H, 1};
    check(har_grad_reduce_adam(1, &src, &start, &total, &total, &nsl, total, P<float>(G), P<float>(param),
                               P<float>(mm), P<float>(vv), P<uint16_t>(pb), lr, b1c, b2c, eps, wd, P<int32_t>(step),
                               0, 1 | 4, &frag, S(stream)),
          "mlp_small_step reduce+adam");
  });
  m.def("mlp_pack_frag", [](u pb, u dst, int64_t w0_off, int64_t w1_off, int K0, int H, u stream) {
    const MlpFragSpec f{P<uint16_t>(dst), w0_off, w1_off, K0, H};
    check(har_mlp_pack_frag(P<const uint16_t>(pb), &f, S(stream)), "mlp_pack_frag");
  });
  m.def("reduce_slabs_multi", [](std::vector<u> slabs, std::vector<int> nsl, std::vector<int64_t> n,
                                 std::vector<int64_t> lds, std::vector<u> dst, std::vector<int64_t> ldd, int G,
                                 u tick, u stream) {
    const int k = (int)slabs.size();
    if ((int)nsl.size() != k || (int)n.size() != k || (int)lds.size() != k || (int)dst.size() != k ||
        (int)ldd.size() != k)
      throw std::runtime_error("reduce_slabs_multi: segment lists differ in length");
    std::vector<const float*> sp(k);
    std::vector<float*> dp(k);
    for (int i = 0; i < k; ++i) { sp[i] = P<const float>(slabs[i]); dp[i] = P<float>(dst[i]); }
    check(har_reduce_slabs_multi(k, sp.data(), nsl.data(), n.data(), lds.data(), dp.data(), ldd.data(), G,
                                 P<int32_t>(tick), S(stream)),
          "reduce_slabs_multi");
  });
  m.def("head_fused_blocks", &har_head_fused_blocks);
  m.def("mlp_fwd_head_grid", &har_mlp_fwd_head_grid);
  m.def("mlp_set_stamps", [](u p) { har_mlp_set_stamps(P<uint64_t>(p)); });
  py::class_<MlpStepPlan>(m, "MlpStepPlan")
      .def(py::init([](py::dict d) {
        MlpStepPlan p;
        for (const char* k : {"Wf", "b0", "b1", "Wo", "bo", "dact2", "fslab", "bloss", "bcorr", "gw1", "gw0",
                              "gb0", "gb1", "step", "G", "P", "m", "v", "Pb"}) {
          const u x = d[k].cast<u>();
          if (!strcmp(k, "Wf")) p.Wf = x; else if (!strcmp(k, "b0")) p.b0 = x;
          else if (!strcmp(k, "b1")) p.b1 = x; else if (!strcmp(k, "Wo")) p.Wo = x; else if (!strcmp(k, "bo")) p.bo = x;
          else if (!strcmp(k, "dact2")) p.dact2 = x;
          else if (!strcmp(k, "fslab")) p.fslab = x; else if (!strcmp(k, "bloss")) p.bloss = x;
          else if (!strcmp(k, "bcorr")) p.bcorr = x; else if (!strcmp(k, "gw1")) p.gw1 = x;
          else if (!strcmp(k, "gw0")) p.gw0 = x; else if (!strcmp(k, "gb0")) p.gb0 = x; else if (!strcmp(k, "gb1")) p.gb1 = x;
          else if (!strcmp(k, "step")) p.step = x; else if (!strcmp(k, "G")) p.G = x; else if (!strcmp(k, "P")) p.Pw = x;
          else if (!strcmp(k, "m")) p.m = x; else if (!strcmp(k, "v")) p.v = x; else p.Pb = x;
        }
        p.K0 = d["K0"].cast<int>();
        p.fslab_w = d["fslab_w"].cast<int>();
        p.gwo = d["gwo"].cast<u>();
        p.gbo = d["gbo"].cast<u>();
        p.H = d["H"].cast<int>();
        p.C = d["C"].cast<int>();
        p.stride = d["stride"].cast<int64_t>();
        p.n = d["n"].cast<int64_t>();
        p.lr = d["lr"].cast<float>();
        p.b1c = d["beta1"].cast<float>();
        p.b2c = d["beta2"].cast<float>();
        p.eps = d["eps"].cast<float>();
        p.wd = d["wd"].cast<float>();
        p.frag = MlpFragSpec{P<uint16_t>(p.Wf), d["w0_off"].cast<int64_t>(), d["w1_off"].cast<int64_t>(), p.K0, p.H};
        for (auto r : d["regions"].cast<py::list>()) {  // (start, end, src pointer, #slabs, slab stride)
          auto t = r.cast<py::tuple>();
          const int64_t a = t[0].cast<int64_t>(), e = t[1].cast<int64_t>();
          p.start.push_back(a);
          p.len.push_back(e - a);
          p.src.push_back(P<const float>(t[2].cast<u>()));
          p.S.push_back(t[3].cast<int>());
          p.lds.push_back(t[4].cast<int64_t>());
        }
        return p;
      }))
      .def("run", &MlpStepPlan::run, py::arg("X"), py::arg("y"), py::arg("B"), py::arg("scale"), py::arg("mode"),
           py::arg("stream"), py::arg("pf") = 0, py::arg("pf_bytes") = 0, py::arg("pf1") = 0, py::arg("pf1_bytes") = 0)
      .def_readwrite("pf_sink", &MlpStepPlan::pf_sink);
  m.def("mlp_step_grid", &har_mlp_step_grid);
  m.def("mlp_step_slices", &har_mlp_step_slices);
  m.def("mlp_step_fwd_slab_width", &har_mlp_step_fwd_slab_width);
  m.def("mlp_step_fwd", [](u X, int K0, u Wf, u b0, u b1, int H, u Wo, u bo, u labels, int B, int C, float scale,
                           u dact2, u slab, u block_loss, u block_correct, u stream) {
    check(har_mlp_step_fwd(P<const uint16_t>(X), K0, P<uint16_t>(Wf), P<const float>(b0), P<const float>(b1), H,
                           P<const uint16_t>(Wo), P<const float>(bo), P<const int32_t>(labels), B, C, scale,
                           P<uint16_t>(dact2), P<float>(slab), P<float>(block_loss), P<int32_t>(block_correct),
                           S(stream)),
          "mlp_step_fwd");
  });
  m.def("mlp_step_fwd_infer", [](u X, int K0, u Wf, u b0, u b1, int H, u Wo, u bo, int B, int C, u logits, u pred,
                                 u stream) {
    check(har_mlp_step_fwd_infer(P<const uint16_t>(X), K0, P<const uint16_t>(Wf), P<const float>(b0),
                                 P<const float>(b1), H, P<const uint16_t>(Wo), P<const float>(bo), B, C,
                                 P<float>(logits), P<int32_t>(pred), S(stream)),
          "mlp_step_fwd_infer");
  });
  m.def("mlp_step_bwd", [](u dact2, u X, int K0, u Wf, int H, u b0, int B, u gw1, u gw0, u gb0, u gb1,
                           int64_t stride, u tick, u fslab, int fslab_w, u gwo, u gbo, u stream) {
    check(har_mlp_step_bwd(P<const uint16_t>(dact2), P<const uint16_t>(X), K0, P<const uint16_t>(Wf), H,
                           P<const float>(b0), B, P<float>(gw1), P<float>(gw0), P<float>(gb0), P<float>(gb1), stride,
                           P<int32_t>(tick), P<const float>(fslab), fslab_w, P<float>(gwo), P<float>(gbo), S(stream)),
          "mlp_step_bwd");
  });
  m.def("mlp_fwd_head", [](u X, int K0, u W0, u b0, u W1, u b1, int H, u Wo, u bo, u labels, int B, int C,
                           float scale, u h1, u dact, u slab, u block_loss, u block_correct, u stream) {
    check(har_mlp_fwd_head(P<const uint16_t>(X), K0, P<const uint16_t>(W0), P<const float>(b0),
                           P<const uint16_t>(W1), P<const float>(b1), H, P<const uint16_t>(Wo), P<const float>(bo),
                           P<const int32_t>(labels), B, C, scale, P<uint16_t>(h1), P<uint16_t>(dact), P<float>(slab),
                           P<float>(block_loss), P<int32_t>(block_correct), S(stream)),
          "mlp_fwd_head");
  });
  m.def("mlp_fwd_infer_f32", [](u X, int ldx, int F, int K0, u W0, u b0, u W1, u b1, int H, u Wo, u bo, int B,
                                int C, u logits, u pred, u stream) {
    check(har_mlp_fwd_infer_f32(P<const float>(X), ldx, F, K0, P<const uint16_t>(W0), P<const float>(b0),
                                P<const uint16_t>(W1), P<const float>(b1), H, P<const uint16_t>(Wo), P<const float>(bo),
                                B, C, P<float>(logits), P<int32_t>(pred), S(stream)),
          "mlp_fwd_infer_f32");
  });
  m.def("mlp_fwd_infer", [](u X, int K0, u W0, u b0, u W1, u b1, int H, u Wo, u bo, int B, int C, u logits, u pred,
                            u stream) {
    check(har_mlp_fwd_infer(P<const uint16_t>(X), K0, P<const uint16_t>(W0), P<const float>(b0),
                            P<const uint16_t>(W1), P<const float>(b1), H, P<const uint16_t>(Wo), P<const float>(bo), B,
                            C, P<float>(logits), P<int32_t>(pred), S(stream)),
          "mlp_fwd_infer");
  });
  m.def("head_fused", [](u H, u W, u bias, u labels, int B, int D, int C, float scale, u dlogits, u dH, u block_loss,
                         u block_correct, u stream) {
    check(har_head_fused(P<const uint16_t>(H), P<const uint16_t>(W), P<const float>(bias), P<const int32_t>(labels),
                         B, D, C, scale, P<uint16_t>(dlogits), P<uint16_t>(dH), P<float>(block_loss),
                         P<int32_t>(block_correct), S(stream)),
          "head_fused");
  });

  m.def(
      "reduce_slabs_grouped",
      [](u slabs, int S_, int64_t n, u dst, int G, u stream, u tick, int64_t lds, int64_t ldd) {
        check(har_reduce_slabs_grouped(P<const float>(slabs), S_, n, lds < 0 ? n : lds, P<float>(dst), G,
                                       ldd < 0 ? n : ldd, P<int32_t>(tick), S(stream)),
              "reduce_slabs_grouped");
      },
      py::arg("slabs"), py::arg("S"), py::arg("n"), py::arg("dst"), py::arg("G"), py::arg("stream"),
      py::arg("tick"), py::arg("lds") = -1, py::arg("ldd") = -1);

  m.def("column_stats_workspace", &har_column_stats_workspace);
  m.def("column_stats_f64", [](u X, int64_t n, int ncols, u center, u stats, u ws, u stream) {
    check(har_column_stats_f64(P<const double>(X), n, ncols, P<const double>(center), P<double>(stats),
                               P<double>(ws), S(stream)),
          "column_stats_f64");
  });
  m.def("column_stats", [](u X, int64_t n, int ncols, int ld, u w, u stats, u ws, u stream) {
    check(har_column_stats(P<const float>(X), n, ncols, ld, P<const float>(w), P<double>(stats), P<double>(ws),
                           S(stream)),
          "column_stats");
  });
  m.def("tree_thresholds_hybrid", [](u cat, int64_t n, int ncat, int F, u colmap, u dthr, int ns, int maxb, u ones,
                                     u thr_mat, u nbins, u stream) {
    check(har_tree_thresholds_hybrid(P<const int32_t>(cat), n, ncat, F, P<const int32_t>(colmap), P<const float>(dthr),
                                     ns, maxb, P<int32_t>(ones), P<float>(thr_mat), P<int32_t>(nbins), S(stream)),
          "tree_thresholds_hybrid");
  });
  m.def("tree_bins_hybrid", [](u dense, int64_t n, int Fd, u dense_cols, u cat, int ncat, int F, u thr, int maxb,
                               u nbins, u bins, u stream) {
    check(har_tree_bins_hybrid(P<const float>(dense), n, Fd, P<const int32_t>(dense_cols), P<const int32_t>(cat), ncat,
                               F, P<const float>(thr), maxb, P<const int32_t>(nbins), P<uint8_t>(bins), S(stream)),
          "tree_bins_hybrid");
  });
  m.def("bin_features", [](u X, int64_t n, int F, int ld, u thr, int maxb, u nthr, u bins, u stream) {
    check(har_bin_features(P<const float>(X), n, F, ld, P<const float>(thr), maxb, P<const int32_t>(nthr),
                           P<uint8_t>(bins), S(stream)),
          "bin_features");
  });

  m.def("tree_feature_subsets", [](uint64_t seed, u trees, u nodes, int64_t npairs, int F, int m_, u out, u p_dev,
                                   u stream) {
    check(har_tree_feature_subsets(seed, P<const int32_t>(trees), P<const int32_t>(nodes), npairs, F, m_,
                                   P<int32_t>(out), P<const int32_t>(p_dev), S(stream)),
          "tree_feature_subsets");
  });
  m.def("tree_level_keys", [](u node_of, u cand_idx, int T, int64_t N, int maxn, u key, u stream) {
    check(har_tree_level_keys(P<const int32_t>(node_of), P<const int32_t>(cand_idx), T, N, maxn, P<int32_t>(key),
                              S(stream)),
          "tree_level_keys");
  });
  m.def("tree_level_group", [](u node_of, u cand_idx, u tree_lo, u W, int T, int64_t N, int maxn, int A, int nt_max,
                               u cnt_ws, u counts, u starts, u rows, u row_w, u a_dev, u stream) {
    check(har_tree_level_group(P<const int32_t>(node_of), P<const int32_t>(cand_idx), P<const int32_t>(tree_lo),
                               P<const float>(W), T, N, maxn, A, nt_max, P<int32_t>(cnt_ws), P<int32_t>(counts),
                               P<int32_t>(starts), P<int32_t>(rows), P<float>(row_w), P<const int32_t>(a_dev),
                               S(stream)),
          "tree_level_group");
  });
  m.def("tree_level_group_chunks", [](int64_t N) { return har_tree_level_group_chunks(N); });
  m.def("tree_commit_level", [](int nsplit, u ti, u ni, u cl, u dsi, u rfeat, u rbin, u rgain, u rleft, u rtotal, int K,
                                u thr_mat, int ldthr, int maxn, u feature, u split_bin, u thresh, u left, u right,
                                u gains, u stats, u s_dev, u stream) {
    check(har_tree_commit_level(nsplit, P<const int64_t>(ti), P<const int64_t>(ni), P<const int64_t>(cl),
                                P<const int64_t>(dsi), P<const int32_t>(rfeat), P<const int32_t>(rbin),
                                P<const float>(rgain), P<const float>(rleft), P<const float>(rtotal), K,
                                P<const float>(thr_mat), ldthr, maxn, P<int32_t>(feature), P<int32_t>(split_bin),
                                P<float>(thresh), P<int32_t>(left), P<int32_t>(right), P<float>(gains),
                                P<float>(stats), P<const int32_t>(s_dev), S(stream)),
          "tree_commit_level");
  });
  m.def("tree_partition_split", [](u node_of, u feature, u split_bin, u left, u bins, int T, int64_t N, int maxn,
                                   u stream) {
    check(har_tree_partition_split(P<int32_t>(node_of), P<const int32_t>(feature), P<const int32_t>(split_bin),
                                   P<const int32_t>(left), P<const uint8_t>(bins), T, N, maxn, S(stream)),
          "tree_partition_split");
  });
  m.def("tree_level_decide", [](int A, u gain, u left, u total, int K, int impurity, float min2, u out, u a_dev,
                                u stream) {
    check(har_tree_level_decide(A, P<const float>(gain), P<const float>(left), P<const float>(total), K, impurity, min2,
                                P<float>(out), P<const int32_t>(a_dev), S(stream)),
          "tree_level_decide");
  });
  m.def("tree_frontier", [](int A, int Tn, int maxn, u ct, u cn, u tlo, u dec, u n_nodes, u n_nodes_next, u pos_ws,
                            u ti, u ni, u cl, u dsi, u front, u q_ws, u ct_next, u cn_next, u tlo_next, u cand_idx,
                            u scal, u a_dev, u parent_of, u derive_from, u stream) {
    check(har_tree_frontier(A, Tn, maxn, P<const int32_t>(ct), P<const int32_t>(cn), P<const int32_t>(tlo),
                            P<const float>(dec), P<const int32_t>(n_nodes), P<int32_t>(n_nodes_next),
                            P<int32_t>(pos_ws), P<int64_t>(ti), P<int64_t>(ni), P<int64_t>(cl), P<int64_t>(dsi),
                            P<float>(front), P<int32_t>(q_ws), P<int32_t>(ct_next), P<int32_t>(cn_next),
                            P<int32_t>(tlo_next), P<int32_t>(cand_idx), P<int32_t>(scal), P<const int32_t>(a_dev),
                            P<int32_t>(parent_of), P<int32_t>(derive_from), S(stream)),
          "tree_frontier");
  });
  m.def("tree_root_frontier", [](u stats, int Tn, int K, int64_t tree_stride, int impurity, float min2, int maxn, u ct,
                                 u cn, u tlo, u cand_idx, u scal, u stream) {
    check(har_tree_root_frontier(P<const float>(stats), Tn, K, tree_stride, impurity, min2, maxn, P<int32_t>(ct),
                                 P<int32_t>(cn), P<int32_t>(tlo), P<int32_t>(cand_idx), P<int32_t>(scal), S(stream)),
          "tree_root_frontier");
  });
  m.def("tree_partition", [](u node_of, u lvl_feat, u lvl_bin, u lvl_left, u bins, int T, int64_t N, int maxn,
                             u stream) {
    check(har_tree_partition(P<int32_t>(node_of), P<const int32_t>(lvl_feat), P<const int32_t>(lvl_bin),
                             P<const int32_t>(lvl_left), P<const uint8_t>(bins), T, N, maxn, S(stream)),
          "tree_partition");
  });
  m.def("csv_count_newlines", [](u buf, int64_t n, u counts, u stream) {
    check(har_csv_count_newlines(P<const uint8_t>(buf), n, P<int32_t>(counts), S(stream)), "csv_count_newlines");
  });
  m.def("csv_newline_pos", [](u buf, int64_t n, u block_off, u pos, u stream) {
    check(har_csv_newline_pos(P<const uint8_t>(buf), n, P<const int64_t>(block_off), P<int64_t>(pos), S(stream)),
          "csv_newline_pos");
  });
  m.def("csv_parse_rows", [](u buf, u starts, u ends, int64_t nrows, int ncols, u vals, u hashes, u flags, u fstart,
                             u flen, u stream) {
    check(har_csv_parse_rows(P<const uint8_t>(buf), P<const int64_t>(starts), P<const int64_t>(ends), nrows, ncols,
                             P<double>(vals), P<uint64_t>(hashes), P<uint8_t>(flags), P<int64_t>(fstart),
                             P<int32_t>(flen), S(stream)),
          "csv_parse_rows");
  });

  m.def("cast_pad_bf16", [](u in, int rows, int cin, int ldin, u out, int cout, u stream) {
    check(har_cast_pad_bf16(P<const float>(in), rows, cin, ldin, P<uint16_t>(out), cout, S(stream)), "cast_pad_bf16");
  });
}
