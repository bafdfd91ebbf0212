"""GBTClassifier on the CPU: the PyTorch definitions of har/ops/gbt.py (the oracle of the HIP
kernels) against autograd / closed forms, the tie and edge rules, determinism, the loss history,
WISDM accuracy against a single tree, persistence, the CLI and CrossValidator."""
import csv
import math

import numpy as np
import pytest
import torch

from har.models.gbt import GBTClassificationModel, GBTClassifier
from har.ops import gbt as G


def _blobs(N=600, F=8, K=4, seed=0, spread=1.5):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(K, F, generator=g) * 2.0
    y = torch.randint(0, K, (N,), generator=g)
    X = mu[y] + spread * torch.randn(N, F, generator=g)
    return X, y


def test_oracle_gradient_equals_autograd():
    g = torch.Generator().manual_seed(1)
    N, K = 257, 6
    m32 = (torch.randn(N, K, generator=g) * 3).float()
    y = torch.randint(0, K, (N,), generator=g)
    gf, hf, loss = G.grad_float(m32, y)
    m = m32.double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(m, y, reduction="sum")
    (ag,) = torch.autograd.grad(ce, m)
    torch.testing.assert_close(gf.t(), ag, rtol=1e-10, atol=0)
    p = torch.softmax(m32.double(), dim=1)
    torch.testing.assert_close(hf.t(), (p * (1 - p)).clamp_min(1e-16), rtol=1e-10, atol=0)
    torch.testing.assert_close(loss, ce.detach(), rtol=1e-12, atol=0)
    # +-100 margins: finite, and weight 0 rows carry nothing
    big = torch.tensor([[100.0, -100.0, 0.0], [-100.0, 100.0, 100.0]])
    q, l = G.grad_torch(big, torch.tensor([1, 0]), torch.tensor([1, 0], dtype=torch.int32))
    assert torch.isfinite(l).all() and (q[:, 1] == 0).all()
    assert q[0, 0, 0].item() == 1 << 20 and q[1, 0, 0].item() == -(1 << 20)


# 8 rows, 2 features.  Feature 0 separates the classes at x0 <= 3.5 | > 3.5; feature 1 is constant.
_HAND_X = torch.tensor([[0.0, 7.0], [1.0, 7.0], [2.0, 7.0], [3.0, 7.0], [4.0, 7.0], [5.0, 7.0], [6.0, 7.0], [7.0, 7.0]])
_HAND_Y = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1])


def test_one_tree_on_hand_made_data():
    """K = 2, priors 1/2: p = 1/2 everywhere, so for class 0 g = -1/2 on rows 0-3 and +1/2 on rows 4-7,
    h = 1/4.  With minInstancesPerNode = 4 the only valid cut is bin 3 of feature 0 (4 | 4 rows), gain
    = 1/2 [2^2 / (1 + 1) + 2^2 / (1 + 1) - 0] = 2, leaves -0.1 * (-+2) / (1 + 1) = +-0.1."""
    est = GBTClassifier(maxIter=1, maxDepth=2, minInstancesPerNode=4, stepSize=0.1, regLambda=1.0)
    m = est.fit_tensors(_HAND_X, _HAND_Y, 2)
    a = m.arrs
    assert a.feature.shape == (2, 7) and m.getNumTrees == 2
    for t, sign in ((0, 1.0), (1, -1.0)):
        assert a.feature[t].tolist() == [0, -1, -1, -1, -1, -1, -1]
        assert a.threshold[t, 0].item() == 3.5 and (a.left[t, 0].item(), a.right[t, 0].item()) == (1, 2)
        assert a.gain[t, 0].item() == 2.0
        # root value 0 (G = 0); left leaf: G = -+2, H = 1 -> -0.1 * G / 2
        np.testing.assert_allclose(a.stats[t, :3, t].tolist(), [0.0, sign * 0.1, -sign * 0.1], rtol=1e-7, atol=0)
        assert a.stats[t, :, 1 - t].abs().sum().item() == 0
    assert list(m.arrs.n_nodes) == [3, 3] and m.totalNumNodes == 6
    raw = m.predict_raw(_HAND_X)
    np.testing.assert_allclose(raw[0].tolist(), [math.log(0.5) + 0.1, math.log(0.5) - 0.1], rtol=1e-6)
    assert m.predict(_HAND_X).tolist() == _HAND_Y.tolist()
    imp = m.featureImportances
    assert imp.tolist() == [1.0, 0.0]


def test_tie_rule_lowest_feature_then_lowest_bin():
    X, y = _blobs(200, 1, 2, seed=3)
    X2 = torch.cat([X, X, X], dim=1)  # identical columns: every gain ties
    m = GBTClassifier(maxIter=3, maxDepth=3).fit_tensors(X2, y, 2)
    f = m.arrs.feature
    assert (f[f >= 0] == 0).all() and (f >= 0).any()
    # exact ties inside a histogram: features 1 and 2 are duplicates whose cuts 1 and 2 are the same cut (bin 2 is
    # empty) and whose cut 0 is invalid (no row left of it); feature 0 has a single bin and holds the totals
    q, hh = 1 << 20, 1 << 18
    hist = torch.zeros(1, 1, 3, 4, 3, dtype=torch.int64)
    hist[0, 0, 0, 0] = torch.tensor([0, 2 * hh, 2])
    for f in (1, 2):
        hist[0, 0, f, 1] = torch.tensor([-q, hh, 1])
        hist[0, 0, f, 3] = torch.tensor([q, hh, 1])
    r = G.split_torch(hist, torch.tensor([1, 4, 4], dtype=torch.int32), 1.0, 1, 0.0)
    assert (r.feat.item(), r.bin.item()) == (1, 1)
    assert r.gain.item() == 0.5 * ((1.0 / 1.25 + 1.0 / 1.25) - 0.0) and r.sums[0, 0].tolist() == [-q, hh, 1, 0, 2 * hh, 2]
    # no valid cut at minInstancesPerNode = 2: a leaf
    r = G.split_torch(hist, torch.tensor([1, 4, 4], dtype=torch.int32), 1.0, 2, 0.0)
    assert r.feat.item() == -1 and r.gain.item() == float("-inf")


def test_edges_constant_feature_min_instances_k2_n1_absent_class():
    X, y = _blobs(300, 5, 3, seed=4)
    X[:, 2] = 1.25  # constant: one bin, never split
    est = GBTClassifier(maxIter=4, maxDepth=4, minInstancesPerNode=7)
    m = est.fit_tensors(X, y, 3)
    assert not (m.arrs.feature == 2).any()
    # every committed split: both children hold >= 7 rows (replay the partition of the training rows)
    from har.ops import tree as T
    from har.ops.stats import bin_features

    tt = T.ThresholdTable.from_any(T.thresholds_for(X, 32, seed=0))
    bins = bin_features(X, tt)
    for t in range(m.getNumTrees):
        node = torch.zeros(X.shape[0], dtype=torch.long)
        for _ in range(4):
            f = m.arrs.feature[t][node].long()
            go = X[torch.arange(X.shape[0]), f.clamp_min(0)] <= m.arrs.threshold[t][node]
            nxt = torch.where(go, m.arrs.left[t][node], m.arrs.right[t][node]).long()
            node = torch.where(f >= 0, nxt, node)
        cnt = torch.bincount(node, minlength=31)
        internal = (m.arrs.feature[t] >= 0).nonzero().flatten().tolist()
        for n in range(1, 31):
            parent = (n - 1) // 2
            if parent in internal and m.arrs.feature[t, n] < 0:
                assert cnt[n] >= 7, (t, n, cnt[n])
    assert bins.shape[0] == 5
    # K = 2
    Xb, yb = _blobs(200, 4, 2, seed=5)
    mb = GBTClassifier(maxIter=5, maxDepth=3).fit_tensors(Xb, yb, 2)
    assert (mb.predict(Xb) == yb).float().mean() > 0.9
    # N = 1: no thresholds, root leaves only
    m1 = GBTClassifier(maxIter=2, maxDepth=3).fit_tensors(torch.tensor([[1.0, 2.0]]), torch.tensor([1]), 2)
    assert m1.totalNumNodes == 4 and m1.predict(torch.tensor([[1.0, 2.0]])).tolist() == [1]
    assert all(math.isfinite(v) for v in m1.trainLossHistory)
    # a class with no training rows: its log prior is clamped, never predicted, everything finite
    ya = yb.clone()
    ma = GBTClassifier(maxIter=3, maxDepth=3).fit_tensors(Xb, ya, 3)
    assert ma.init[2].item() == pytest.approx(math.log(1e-12), rel=1e-6)
    raw, prob, pred = ma.predict_all(Xb)
    assert torch.isfinite(raw).all() and (pred != 2).all() and all(math.isfinite(v) for v in ma.trainLossHistory)
    # parameters outside the native range raise, on every device
    for kw in ({"maxDepth": 7}, {"maxDepth": 0}, {"maxBins": 65}, {"maxBins": 1}):
        with pytest.raises(ValueError):
            GBTClassifier(maxIter=1, **kw).fit_tensors(Xb, yb, 2)


def _arrays(m):
    a = m.arrs
    return [a.feature, a.threshold, a.left, a.right, a.stats, a.gain, m.init]


def test_determinism_and_subsampling_seeds():
    X, y = _blobs(500, 8, 4, seed=6)
    a = GBTClassifier(maxIter=5, maxDepth=4, subsamplingRate=0.5, seed=7).fit_tensors(X, y, 4)
    b = GBTClassifier(maxIter=5, maxDepth=4, subsamplingRate=0.5, seed=7).fit_tensors(X, y, 4)
    c = GBTClassifier(maxIter=5, maxDepth=4, subsamplingRate=0.5, seed=8).fit_tensors(X, y, 4)
    assert all(torch.equal(u, v) for u, v in zip(_arrays(a), _arrays(b)))
    assert a.trainLossHistory == b.trainLossHistory
    assert not all(torch.equal(u, v) for u, v in zip(_arrays(a), _arrays(c)))
    # the round weights are the Philox row stream: keyed by round, about half the rows
    w0, w1 = G.round_weights(7, 0, 500, 0.5, "cpu"), G.round_weights(7, 1, 500, 0.5, "cpu")
    assert not torch.equal(w0, w1) and 180 < int(w0.sum()) < 320 and set(w0.tolist()) == {0, 1}
    assert G.round_weights(7, 0, 500, 1.0, "cpu") is None


def test_loss_history_starts_at_prior_entropy_and_falls():
    X, y = _blobs(400, 6, 3, seed=9)
    m = GBTClassifier(maxIter=8, maxDepth=3).fit_tensors(X, y, 3)
    p = torch.bincount(y, minlength=3).double() / 400
    ent = -(p * torch.log(p)).sum().item()
    h = m.trainLossHistory
    assert len(h) == 9
    assert h[0] == pytest.approx(ent, rel=1e-6)  # (the margins are fp32 logs of the priors)
    assert h[-1] < h[0] and all(b < a for a, b in zip(h, h[1:]))


def test_wisdm_accuracy_not_below_a_single_tree(wisdm_csv):
    from har.models.base import features_tensor, labels_tensor
    from har.models.tree import DecisionTreeClassifier
    from har.suite import load_wisdm

    train, test, _ = load_wisdm(wisdm_csv, "numeric43", 2018)
    Xt, yt = features_tensor(test, "features", "cpu"), labels_tensor(test, "label", "cpu")
    gbt = GBTClassifier(maxIter=20, maxDepth=4, device="cpu").fit(train)
    dt = DecisionTreeClassifier(maxDepth=5, device="cpu").fit(train)
    acc_gbt = (gbt.predict(Xt) == yt).double().mean().item()
    acc_dt = (dt.predict(Xt) == yt).double().mean().item()
    print(f"WISDM numeric43 test accuracy: GBT(20 rounds, depth 4) {acc_gbt:.4f}, DecisionTree(depth 5) {acc_dt:.4f}")
    assert acc_gbt >= acc_dt


def test_persist_round_trip_is_bitwise(tmp_path):
    from har.utils import persist

    X, y = _blobs(300, 6, 3, seed=10)
    m = GBTClassifier(maxIter=4, maxDepth=3).fit_tensors(X, y, 3)
    persist.save(m, str(tmp_path / "gbt"))
    r = persist.load(str(tmp_path / "gbt"), device="cpu")
    assert isinstance(r, GBTClassificationModel) and r.getNumTrees == 12
    for u, v in zip(m.predict_all(X), r.predict_all(X)):
        assert torch.equal(u, v)
    assert r.trainLossHistory == m.trainLossHistory and torch.equal(r.featureImportances, m.featureImportances)


def test_cli_preset_gbt_then_predict_on_synthetic_raw(tmp_path):
    import main
    import predict
    from har.features.raw import raw_to_table, write_synthetic_raw

    p = str(tmp_path / "raw.csv")
    write_synthetic_raw(p, n_windows=120, users=4)
    mdir = tmp_path / "models"
    s = main.run(main.config_from_args(["--raw", p, "--out-dir", str(tmp_path / "out"), "--device", "cpu", "--preset",
                                        "gbt", "--gbt-max-iter", "5", "--gbt-max-depth", "3", "--gbt-step-size", "0.2",
                                        "--save-models", str(mdir)]))
    assert set(s["models"]) == {"gbt"} and s["models"]["gbt"]["accuracy"] > 0.5
    assert "GBTClassificationModel" in s["models"]["gbt"]["model"]  # 5 rounds x the stream's classes
    # the windowed table of the same raw rows, as the CSV predict.py reads
    t = raw_to_table(p)
    tab = tmp_path / "windows.csv"
    with open(tab, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(t.columns)
        cols = [t[c].data for c in t.columns]
        for i in range(t.count()):
            w.writerow([c[i] for c in cols])
    out = tmp_path / "pred.csv"
    rec = predict.main(["--models", str(mdir), "--model", "gbt", "--data", str(tab), "--device", "cpu", "--out",
                        str(out)])
    assert rec["rows"] == 120 and rec["accuracy"] > 0.5
    with open(out) as f:
        rows = list(csv.reader(f))
    assert len(rows) == 121 and rows[0][-3:] == ["prediction", "label_name", "probability"]


def test_cross_validator_over_max_depth():
    from har.data.table import Column, Table
    from har.evaluation.evaluators import MulticlassClassificationEvaluator
    from har.tuning.crossval import CrossValidator, ParamGridBuilder

    X, y = _blobs(240, 5, 3, seed=11)
    table = Table([Column("features", "vector", X.double().numpy()), Column("label", "double", y.double().numpy())])
    est = GBTClassifier(maxIter=3, device="cpu")
    grid = ParamGridBuilder().addGrid("maxDepth", [2, 3]).build()
    cv = CrossValidator(estimator=est, estimatorParamMaps=grid, numFolds=2, seed=1,
                        evaluator=MulticlassClassificationEvaluator(labelCol="label", predictionCol="prediction",
                                                                    metricName="accuracy"))
    m = cv.fit(table)
    assert isinstance(m.bestModel, GBTClassificationModel) and len(m.avgMetrics) == 2
    assert m.bestModel.arrs.max_depth in (2, 3) and max(m.avgMetrics) > 0.8


# The device prediction test (tests/test_gpu_gbt.py) compares margins ELEMENTWISE at rtol 1e-5 with the torch
# forest oracle, which sums the same fp32 terms in another order.  Two fp32 orders of one margin (the prior plus
# <= 10 nonzero leaf values, partial sums below 4 in magnitude: at most 11 roundings of <= 2^-23 each per order)
# differ by at most 2 * 11 * 2^-23 = 2.7e-6, so the bound is one that arithmetic can meet only while every margin
# stays at least 0.5 away from zero (2.7e-6 / 0.5 = 5.3e-6 < 1e-5).  The problem, the step size and the seed
# below are chosen so; these checks guard that choice, and the 2 % cap of the tie rule, on the oracle alone.
PREDICT_SHAPE = (2000, 43, 6)


def predict_problem():
    from har.ops import tree as T

    N, F, K = PREDICT_SHAPE
    g = torch.Generator().manual_seed(2024)
    mu = torch.randn(K, F, generator=g)
    y = torch.randint(0, K, (N,), generator=g)
    X = mu[y] + 2.5 * torch.randn(N, F, generator=g)
    return X, y, T.ThresholdTable.from_any(T.thresholds_for(X, 32, seed=0))


def predict_estimator():
    return GBTClassifier(maxIter=10, maxDepth=4, stepSize=0.02, seed=0)


def test_predict_problem_margins_clear_of_zero_and_ties():
    X, y, tt = predict_problem()
    m = predict_estimator().fit_tensors(X, y, PREDICT_SHAPE[2], thresholds=tt)
    raw = m.predict_raw(X)
    top = raw.topk(2, dim=1).values
    excluded = int(((top[:, 0] - top[:, 1]) <= 1e-4).sum())
    print(f"predict problem: |margin| in [{raw.abs().min().item():.4f}, {raw.abs().max().item():.4f}], "
          f"{excluded} of {PREDICT_SHAPE[0]} rows within 1e-4 of a tie")
    assert raw.abs().min().item() >= 0.5 and raw.abs().max().item() < 4.0
    assert excluded <= 0.02 * PREDICT_SHAPE[0]
    assert m.getNumTrees == 60 and (m.predict(X) == y).double().mean() > 0.7
