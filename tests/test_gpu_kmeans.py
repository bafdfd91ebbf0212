"""The K-means kernels (csrc/kernels/kmeans.hip) against their PyTorch definitions in har/ops/kmeans.py.

The scores run on the fp32 matrix cores, so assignments are compared under the derived tie rule of
tests/_kmeans_util.py (clear rows EQUAL the fp64 oracle; the excluded share is a condition, guarded on the
CPU in tests/test_kmeans.py).  Everything downstream of an assignment is fixed point or explicitly rounded
fp64 and must EQUAL the definitions."""
import csv
import os

import numpy as np
import pytest
import torch

from _kmeans_util import ASSIGN_SHAPES, CHUNK, assign_case, blobs, gen, mixture, tie_rule
from har.evaluation.evaluators import ClusteringEvaluator
from har.models.kmeans import KMeans
from har.ops import kmeans as KM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_size_and_plan(cuda):
    assert KM.rows_per_block() == CHUNK
    assert KM.native_plan(43, 6)[2] and KM.native_plan(43, 6)[1] == 1       # LDS accumulators, one slab
    assert not KM.native_plan(43, 256)[2]                                    # global atomics
    assert KM.native_plan(130, 256)[1] == 2 and KM.native_plan(256, 256)[1] > 1


# ------------------------------------------------------------------ assignment
@pytest.mark.parametrize("N,D,K", ASSIGN_SHAPES)
def test_assign_against_fp64_oracle(cuda, N, D, K):
    Xc, C, h = assign_case(N, D, K)
    a_ref, clear, d2_ref, atol = tie_rule(Xc, C, h)
    r = KM.assign_native(Xc.to(cuda), C.to(cuda), h.to(cuda))
    torch.cuda.synchronize()
    a, d2 = r.assign.cpu(), r.d2.cpu()
    excluded = 1.0 - clear.double().mean().item()
    err = (d2.double() - d2_ref).abs()
    worst = (err / atol.clamp_min(1e-300)).max().item()
    print(f"kmeans_assign N={N} D={D} K={K}: excluded share {excluded:.6f}, "
          f"equal share {(a == a_ref).double().mean().item():.6f}, worst d2 error / atol {worst:.4f}")
    assert excluded <= 0.01
    assert int(a.min()) >= 0 and int(a.max()) < K
    assert torch.equal(a[clear], a_ref[clear])
    assert bool((err <= atol).all())
    torch.testing.assert_close(KM.reduce_cost(r.part.cpu()), d2.double().sum(), rtol=1e-12, atol=0)


def test_exact_ties_and_padding(cuda):
    g = gen(5)
    # duplicated centres: the lower index wins (also across the 16-centre tiles and lanes)
    Xc, _ = mixture(300, 43, 21)
    base = Xc[:10].clone()
    C = torch.cat([base, base, base, base[:3]], 0).contiguous()          # K = 33: duplicates 10 and 20 and 30 apart
    r = KM.assign_native(Xc.to(cuda), C.to(cuda), KM.center_h(C).to(cuda))
    assert int(r.assign.max()) < 10
    ref = KM.assign_torch(Xc, base, KM.center_h(base)).assign
    _, clear, _, _ = tie_rule(Xc, base, KM.center_h(base))
    assert torch.equal(r.assign.cpu()[clear], ref[clear])
    # a zero row between +c and -c: equal scores, index 0 wins
    c = torch.randn(1, 5, generator=g)
    C2 = torch.cat([c, -c], 0).contiguous()
    Z = torch.zeros(40, 5)
    r = KM.assign_native(Z.to(cuda), C2.to(cuda), KM.center_h(C2).to(cuda))
    assert int(r.assign.abs().sum()) == 0
    C2r = torch.cat([-c, c], 0).contiguous()
    r = KM.assign_native(Z.to(cuda), C2r.to(cuda), KM.center_h(C2r).to(cuda))
    assert int(r.assign.abs().sum()) == 0
    # padding centres (zeros) are never chosen, though the rows sit at the origin: K = 1 and K = 17
    for K in (1, 17):
        Cf = (torch.randn(K, 5, generator=g) + 5.0).contiguous()
        Zs = torch.randn(70, 5, generator=g) * 1e-3
        r = KM.assign_native(Zs.to(cuda), Cf.to(cuda), KM.center_h(Cf).to(cuda))
        assert int(r.assign.min()) >= 0 and int(r.assign.max()) < K


# ------------------------------------------------------------------ accumulation
def _accumulate_case(cuda, Xc, C, w):
    N, D = Xc.shape
    K = C.shape[0]
    h = KM.center_h(C)
    scale = KM.feature_scales(Xc)
    nscale = KM.norm_scale(KM.row_norms(Xc))
    acc = torch.zeros(KM.acc_size(K, D), dtype=torch.int64, device=cuda)
    r = KM.assign_native(Xc.to(cuda), C.to(cuda), h.to(cuda), w=None if w is None else w.to(cuda),
                         scale=scale.to(cuda), nscale=nscale.to(cuda), acc=acc)
    torch.cuda.synchronize()
    ref = KM.accumulate_torch(Xc, r.assign.cpu(), w, scale, nscale, K)
    assert torch.equal(acc.cpu(), ref)
    # the given-labels mode of the kernel adds the same integers
    acc2 = KM.accumulate_native(Xc.to(cuda), r.assign, None if w is None else w.to(cuda), scale.to(cuda),
                                nscale.to(cuda), K)
    assert torch.equal(acc2.cpu(), ref)
    wd = torch.ones(N, dtype=torch.float64) if w is None else w.double()
    torch.testing.assert_close(KM.reduce_cost(r.part.cpu()), (wd * r.d2.cpu().double()).sum(), rtol=1e-12, atol=0)
    return ref


@pytest.mark.parametrize("N,D,K,weighted", [(2 * CHUNK + 1, 43, 6, False), (2 * CHUNK + 1, 43, 6, True),
                                            (CHUNK + 1, 5, 17, True), (2 * CHUNK + 1, 43, 256, True),
                                            (CHUNK - 1, 130, 255, False)])
def test_accumulators_equal_oracle(cuda, N, D, K, weighted):
    Xc, C, _ = assign_case(N, D, K)
    w = None
    if weighted:
        w = torch.randint(0, 4, (N,), generator=gen(N + K)).to(torch.int32)   # zeros included
        assert int((w == 0).sum()) > 0
    assert KM.native_plan(D, K)[2] == (K * (D + 2) * 8 <= 48 * 1024)
    _accumulate_case(cuda, Xc, C, w)


def test_accumulators_at_the_quantization_limit(cuda):
    # every row in ONE cluster, every value at the 2^30 limit, two full chunks: the total needs > 32 bits
    N, D = 2 * CHUNK, 7
    Xc = torch.full((N, D), 1.0 - 2.0 ** -24)
    Xc[:, 1] = -(1.0 - 2.0 ** -24)
    C = torch.stack([Xc[0], -Xc[0] * 3.0], 0).contiguous()
    ref = _accumulate_case(cuda, Xc, C, None)
    sums, counts, _ = KM.acc_views(ref, 2, D)
    assert int(counts[0]) == N and int(sums[0, 0]) == N * ((1 << 30) - 64) and int(sums[0, 0]) > (1 << 32)
    assert int(sums[0, 1]) == -int(sums[0, 0])


# ------------------------------------------------------------------ update
def _state_tuple(st):
    return st.C.cpu(), st.h.cpu(), st.state.cpu(), st.cost_hist.cpu(), st.moved.cpu(), st.sizes.cpu(), st.acc.cpu()


@pytest.mark.parametrize("N,D,K", [(500, 43, 6), (300, 5, 17), (600, 130, 255)])
def test_update_equals_definition(cuda, N, D, K):
    Xc, C, h = assign_case(N, D, K)
    C[K - 1] = 1e3                                             # a centre far from every row: an empty cluster
    scale, nscale = KM.feature_scales(Xc), KM.norm_scale(KM.row_norms(Xc))
    ref = KM.FitState.alloc(C, 4)
    r = KM.assign_torch(Xc, ref.C, ref.h, scale=scale, nscale=nscale, acc=ref.acc)
    assert int(KM.acc_views(ref.acc, K, D)[1][K - 1]) == 0
    cost = torch.rand(2 * CHUNK + 3, dtype=torch.float64, generator=gen(K))
    dev = KM.FitState.alloc(C.to(cuda), 4)
    dev.acc.copy_(ref.acc)
    for tol2 in (-1.0, -1.0, 1e30, 1e30):                      # two live updates, the third converges, the fourth is frozen
        KM.update_torch(ref, scale, cost, tol2, 4)
        KM.update_native(dev, scale.to(cuda), cost.to(cuda), tol2, 4)
        torch.cuda.synchronize()
        for x, y in zip(_state_tuple(dev), _state_tuple(ref)):
            assert torch.equal(x, y)
        assert torch.equal(ref.C[K - 1], C[K - 1])             # the empty cluster kept its centre
        ref.acc.copy_(KM.accumulate_torch(Xc, r.assign, None, scale, nscale, K))
        dev.acc.copy_(ref.acc)
    assert ref.state.tolist() == [3, 1]                        # the already-converged call changed nothing


# ------------------------------------------------------------------ fits
@pytest.fixture(scope="module")
def blob_problem():
    return blobs()


@pytest.mark.parametrize("k", [6, 16])
def test_teacher_forced_fit(cuda, blob_problem, k):
    X, y, _ = blob_problem
    init = X[torch.randperm(X.shape[0], generator=gen(k))[:k]].clone()
    est = KMeans(k=k, maxIter=12, tol=1e-4, seed=1)
    m1 = est._fit_tensors(X.to(cuda), initial_centers=init)
    m2 = est._fit_tensors(X.to(cuda), initial_centers=init)
    assert torch.equal(m1._Cw, m2._Cw) and torch.equal(m1.summary.predictions, m2.summary.predictions)
    assert m1.summary.costHistory == m2.summary.costHistory and m1.summary.numIter == m2.summary.numIter
    # each device iteration against one oracle iteration from the device's previous centres
    mean = KM.column_means(X)
    Xc = (X - mean.view(1, -1)).contiguous()
    scale, nscale = KM.feature_scales(Xc), KM.norm_scale(KM.row_norms(Xc))
    st = KM.FitState.alloc((init - mean.view(1, -1)).to(cuda).contiguous(), 12)
    Xg = Xc.to(cuda)
    for it in range(4):
        Cprev, hprev = st.C.cpu().clone(), st.h.cpu().clone()
        r = KM.assign_native(Xg, st.C, st.h, scale=scale.to(cuda), nscale=nscale.to(cuda), acc=st.acc)
        a_ref, clear, _, _ = tie_rule(Xc, Cprev, hprev)
        assert torch.equal(r.assign.cpu()[clear], a_ref[clear])
        KM.update_native(st, scale.to(cuda), r.part, -1.0, 12)
        if bool(clear.all()):
            ref = KM.FitState.alloc(Cprev, 12)
            KM.assign_torch(Xc, ref.C, ref.h, scale=scale, nscale=nscale, acc=ref.acc)
            KM.update_torch(ref, scale, r.part.cpu(), -1.0, 12)
            assert torch.equal(st.C.cpu(), ref.C) and torch.equal(st.h.cpu(), ref.h)
    # the oracle's own fit converges to the same partition
    mc = est._fit_tensors(X, initial_centers=init)
    print(f"teacher-forced k={k}: device cost {m1.summary.trainingCost:.6f} oracle {mc.summary.trainingCost:.6f} "
          f"iterations {m1.summary.numIter} / {mc.summary.numIter}")
    assert m1.summary.trainingCost == pytest.approx(mc.summary.trainingCost, rel=1e-5)


def test_kmeans_pp_on_device(cuda, blob_problem):
    X, y, _ = blob_problem
    Xg = X.to(cuda)
    est = KMeans(k=6, maxIter=0, initMode="k-means++", seed=4)
    c1 = est.fit_tensors(Xg).clusterCenters().cpu()
    c2 = est.fit_tensors(Xg).clusterCenters().cpu()
    assert torch.equal(c1, c2)
    assert len({tuple(r.tolist()) for r in c1}) == 6
    # every chosen centre is a row (up to the rounding of centre + mean)
    assert float(torch.cdist(c1.double(), X.double()).min(dim=1).values.max()) < 1e-4
    pp = KMeans(k=6, maxIter=20, initMode="k-means++", seed=4).fit_tensors(Xg)
    rnd = KMeans(k=6, maxIter=20, initMode="random", seed=4).fit_tensors(Xg)
    print(f"k-means++ cost {pp.summary.trainingCost:.4f} random cost {rnd.summary.trainingCost:.4f}")
    assert pp.summary.trainingCost <= rnd.summary.trainingCost * (1 + 1e-12)
    cm, maj, purity = pp.label_map(pp.predict(Xg), y.to(cuda), 6)
    assert int(cm.sum()) == X.shape[0] and purity >= 0.95


# ------------------------------------------------------------------ silhouette
@pytest.mark.parametrize("N,D,K,singleton", [(257, 5, 3, False), (2049, 43, 6, False), (1025, 130, 33, False),
                                             (300, 43, 5, True)])
def test_silhouette_kernel(cuda, N, D, K, singleton):
    Xc, comp = mixture(N, D, 3 * N + K, comps=min(K, 6))
    lab = torch.randint(0, K, (N,), generator=gen(N)) if K > 6 else comp.clone()
    lab[:K] = torch.arange(K)                                    # every cluster non-empty
    if singleton:
        lab[lab == K - 1] = 0
        lab[17] = K - 1                                          # one singleton cluster, and cluster K - 2 emptied
        lab[lab == K - 2] = 1
    ref_rows = KM.silhouette_rows_torch(Xc, lab, K)
    rows = torch.empty(N, dtype=torch.float32, device=cuda)
    got = KM.silhouette_native(Xc.to(cuda), lab.to(cuda), K, rows_out=rows)
    torch.cuda.synchronize()
    print(f"silhouette N={N} D={D} K={K}: kernel {float(got):.8f} fp64 definition {float(ref_rows.mean()):.8f}")
    assert float(got) == pytest.approx(float(ref_rows.mean()), rel=1e-5)
    if singleton:
        assert float(rows[17]) == 0.0


def test_clustering_evaluator_on_device_table(cuda, blob_problem):
    from har.data.table import Column, Table

    X, y, _ = blob_problem
    model = KMeans(k=6, seed=2, device=cuda).fit_tensors(X.to(cuda))
    t = Table([Column("features", "vector", X.double().numpy())])
    out = model.transform(t)
    s = ClusteringEvaluator(device=cuda).evaluate(out)
    ref = float(KM.silhouette(X, torch.as_tensor(out["prediction"].data).long(), 6, native=False))
    assert s == pytest.approx(ref, rel=1e-5) and s > 0.5


# ------------------------------------------------------------------ no host read inside a fit's loop
def test_fit_loop_issues_no_host_read(cuda, blob_problem):
    X, _, mu = blob_problem
    mean = KM.column_means(X)
    Xc = (X - mean.view(1, -1)).contiguous().to(cuda)
    scale, nscale = KM.feature_scales(Xc), KM.norm_scale(KM.row_norms(Xc))
    st = KM.FitState.alloc((mu - mean.view(1, -1)).to(cuda), 8)     # from the blob means: converges in a few iterations
    part = torch.zeros(-(-Xc.shape[0] // CHUNK), dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # a synchronizing call (any device -> host read) raises
    try:
        for _ in range(8):
            r = KM.assign_native(Xc, st.C, st.h, scale=scale, nscale=nscale, acc=st.acc, want_assign=False,
                                 part_out=part)
            KM.update_native(st, scale, r.part, 1e-8, 8)
        KM.assign_native(Xc, st.C, st.h, scale=scale, nscale=nscale, acc=st.acc, part_out=part)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    it, conv = st.state.tolist()
    assert conv == 1 and 1 <= it < 8 and int(KM.acc_views(st.acc, 6, X.shape[1])[1].sum()) == X.shape[0]


# ------------------------------------------------------------------ command line
def test_main_and_predict_on_device(cuda, tmp_path):
    import main
    import predict
    from har.features.raw import raw_to_table, write_synthetic_raw
    from har.models.kmeans import KMeansModel
    from har.utils import persist

    p = str(tmp_path / "raw.csv")
    write_synthetic_raw(p, n_windows=120, users=4)
    mdir = tmp_path / "models"
    s = main.run(main.config_from_args(["--raw", p, "--out-dir", str(tmp_path / "out"), "--device", "cuda:0", "--preset",
                                        "all-numeric", "--kmeans", "6", "--save-models", str(mdir)]))
    assert s["kmeans"]["k"] == 6 and sum(s["kmeans"]["cluster_sizes"]) == s["n_train"]
    assert "device_warmup" in s["phases_s"] and "fit:kmeans" in s["phases_s"]
    assert "Silhouette (test)" in open(tmp_path / "out" / "result.txt").read()
    m = persist.load(str(mdir / "kmeans"), device="cuda:0")
    assert isinstance(m, KMeansModel) and m._Cw.is_cuda and m.majority_labels is not None
    t = raw_to_table(p)
    tab = tmp_path / "windows.csv"
    with open(tab, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(t.columns)
        cols = [t[c].data for c in t.columns]
        for i in range(t.count()):
            w.writerow([c[i] for c in cols])
    rec = predict.main(["--models", str(mdir), "--model", "kmeans", "--data", str(tab), "--device", "cuda:0", "--out",
                        str(tmp_path / "pred.csv")])
    assert rec["rows"] == 120 and 1 <= rec["clusters_used"] <= 6
    with open(tmp_path / "pred.csv") as f:
        assert len(list(csv.reader(f))) == 121
