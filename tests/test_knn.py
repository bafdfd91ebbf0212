"""KNNClassifier on the CPU: the PyTorch definitions of har/ops/knn.py (the oracle of csrc/kernels/knn.hip)
against a plain Python sort, their structural properties, the vote rules, and the model / CrossValidator /
command-line layers."""
import csv

import numpy as np
import pytest
import torch

from _kmeans_util import blobs, gen
from _knn_util import RANK_SHAPES, integer_case, near_tie_share, python_neighbors, rank_consistency, real_case, table_of
from har.evaluation.evaluators import MulticlassClassificationEvaluator
from har.models.knn import KNNClassificationModel, KNNClassifier
from har.ops import kmeans as KM
from har.ops import knn as KN
from har.tuning.crossval import CrossValidator, ParamGridBuilder


# ------------------------------------------------------------------ the search definition
@pytest.mark.parametrize("seed", range(6))
def test_neighbors_against_python_sort(seed):
    N, M, D = [(12, 11, 3), (1, 12, 1), (7, 1, 2), (12, 12, 2), (5, 9, 3), (11, 4, 1)][seed]
    grouped = seed % 2 == 1
    Q, R, h, qg, rg = integer_case(N, D, M, seed, amax=2, groups=grouped)      # many exact ties
    for k in (1, 3, 7, 13):                                                     # k > M included
        wi, ws = python_neighbors(Q, R, h, k, qg, rg)
        idx, d2 = KN.neighbors_torch(Q, R, h, k, qg, rg)
        assert torch.equal(idx, wi)
        want_d = torch.where(wi >= 0, (KM.row_norms(Q).view(-1, 1) + 2.0 * ws).clamp_min(0.0).float(),
                             torch.full((N, k), float("inf")))
        assert torch.equal(d2, want_d)
        # on integer rows d2 is the exact squared distance
        direct = ((Q.double()[:, None, :] - R.double()[None, :, :]) ** 2).sum(-1)
        assert torch.equal(d2[wi >= 0].double(), direct.gather(1, wi.clamp_min(0).long())[wi >= 0])


def test_prefix_property():
    Q, R, h, qg, rg = integer_case(12, 3, 40, 21, amax=2, groups=True)
    i7, d7 = KN.neighbors_torch(Q, R, h, 7, qg, rg)
    i3, d3 = KN.neighbors_torch(Q, R, h, 3, qg, rg)
    assert torch.equal(i3, i7[:, :3]) and torch.equal(d3, d7[:, :3])


def test_reference_split_merge_equals_the_whole_search():
    Q, R, h, qg, rg = integer_case(12, 3, 40, 9, amax=2, groups=True)
    for cuts in ([(0, 40)], [(0, 13), (13, 14), (14, 40)], [(0, 3), (3, 20), (20, 21), (21, 39), (39, 40)]):
        parts = [KN.partial_torch(Q, R[a:b], h[a:b], 7, qg, rg[a:b], offset=a) for a, b in cuts]
        s, i = KN.merge_torch(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), 7)
        wi, wd = KN.neighbors_torch(Q, R, h, 7, qg, rg)
        assert torch.equal(i, wi) and torch.equal(KN.finish_torch(Q, s, i), wd)


def test_rank_rule_holds_for_the_oracle_and_exact_order_would_not():
    """The fp64 oracle meets the rank-consistency requirements with zero error, and the share of rows an
    exact-order rule would have to exclude is what rules that rule out."""
    shares = {}
    for (N, D, M, k) in RANK_SHAPES:
        Q, R, h, qg, rg = real_case(N, D, M, 1000 * N + 10 * D + k, groups=(N % 2 == 1))
        idx, d2 = KN.neighbors_torch(Q, R, h, k, qg, rg)
        worst, S, t = rank_consistency(idx, d2, Q, R, h, k, qg, rg)
        assert worst <= 0.0
        shares[(N, D, M, k)] = near_tie_share(S, k, t)
    print("near-tie shares:", {k: round(v, 3) for k, v in shares.items()})
    assert shares[(64, 130, 513, 64)] > 0.9 and shares[(129, 43, 4097, 64)] > 0.9


# ------------------------------------------------------------------ the vote
def test_vote_rules():
    y = torch.tensor([0, 1, 1, 2, 2, 2], dtype=torch.int32)
    idx = torch.tensor([[0, 1, 2, 3], [3, 4, 0, -1], [-1, -1, -1, -1], [0, 1, 3, -1], [1, 0, 5, 4]], dtype=torch.int32)
    d2 = torch.tensor([[1.0, 4.0, 4.0, 16.0], [0.0, 0.0, 1.0, float("inf")], [float("inf")] * 4,
                       [1.0, 1.0, 1.0, float("inf")], [0.25, 0.25, 1.0, 1.0]])
    u = KN.vote_torch(idx, d2, y, 3, "uniform")
    assert u.raw.tolist() == [[1, 2, 1], [1, 0, 2], [0, 0, 0], [1, 1, 1], [1, 1, 2]]
    assert u.pred.tolist() == [1, 2, 0, 0, 2]                       # the first argmax wins the 1-1-1 tie
    assert u.prob[2].tolist() == [1 / 3] * 3                        # no valid neighbour: uniform
    assert torch.equal(u.prob[0], torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64))
    d = KN.vote_torch(idx, d2, y, 3, "distance")
    assert d.raw[0].tolist() == [1.0, 1.0, 0.25]                    # 1 / sqrt(d2)
    assert d.pred[0] == 0                                           # tie 1.0 - 1.0: the first
    assert d.raw[1].tolist() == [0.0, 0.0, 2.0]                     # the zero-distance rule: zeros 1, others 0
    assert d.raw[2].tolist() == [0.0, 0.0, 0.0] and d.pred[2] == 0
    assert d.raw[4].tolist() == [2.0, 2.0, 2.0] and d.pred[4] == 0
    # the prefix vote
    p = KN.vote_torch(idx, d2, y, 3, "uniform", k=2)
    assert p.raw.tolist() == [[1, 1, 0], [0, 0, 2], [0, 0, 0], [1, 1, 0], [1, 1, 0]]


def test_range_errors_on_the_cpu():
    Q, R, h, _, _ = integer_case(4, 3, 9, 1)
    for k in (0, 65):
        with pytest.raises(ValueError):
            KN.neighbors(Q, R, h, k)
    with pytest.raises(ValueError):
        KN.neighbors(torch.zeros(2, 257), torch.zeros(3, 257), torch.zeros(3), 1)
    y = torch.zeros(9, dtype=torch.int32)
    for C in (0, 33):
        with pytest.raises(ValueError):
            KN.search(Q, R, h, 2, y=y, C=C)
    with pytest.raises(ValueError):
        KN.search(Q, R, h, 2, y=y, C=3, weights="rank")
    with pytest.raises(ValueError):
        KNNClassifier(k=65, device="cpu").fit_tensors(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int64), 2)


def test_working_rows_and_constant_column():
    X = torch.tensor([[1.0, 5.0, 2.0], [3.0, 5.0, 6.0], [5.0, 5.0, 1.0]])
    mean, std = KN.standardizer(X)
    assert mean.tolist() == [3.0, 5.0, 3.0] and std[1] == 1.0
    assert std[0].item() == pytest.approx((8.0 / 3.0) ** 0.5, rel=1e-7)
    mean0, std0 = KN.standardizer(X, standardize=False)
    assert torch.equal(mean0, mean) and std0.tolist() == [1.0, 1.0, 1.0]
    assert torch.equal(KN.working_rows(X, mean0, std0), X - mean)


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def blob_problem():
    return blobs(2000, 43, 6)


def test_blobs_accuracy_equals_brute_force(blob_problem):
    X, y, _ = blob_problem
    Xtr, ytr, Xte, yte = X[:1400], y[:1400], X[1400:], y[1400:]
    m = KNNClassifier(k=5, device="cpu").fit_tensors(Xtr, ytr, 6)
    pred = m.predict(Xte)
    # brute force in fp64, from the model's definition of the working rows but none of its code
    mu = Xtr.double().mean(0)
    sd = ((Xtr.double() - mu) ** 2).mean(0).sqrt()
    Ztr, Zte = ((Xtr.double() - mu) / sd), ((Xte.double() - mu) / sd)
    nn = torch.cdist(Zte, Ztr).topk(5, dim=1, largest=False).indices
    votes = torch.nn.functional.one_hot(ytr[nn], 6).sum(1)
    top = votes.topk(2, dim=1).values
    assert int((top[:, 0] == top[:, 1]).sum()) == 0
    want = votes.argmax(1)
    assert torch.equal(pred, want)
    acc = (pred == yte).double().mean().item()
    assert acc == (want == yte).double().mean().item() == 1.0


def test_kneighbors_and_exclusion(blob_problem):
    X, y, _ = blob_problem
    m = KNNClassifier(k=3, device="cpu").fit_tensors(X[:300], y[:300], 6)
    idx, d2 = m.kneighbors(X[:300])
    assert torch.equal(idx[:, 0], torch.arange(300, dtype=torch.int32))         # a training row finds itself
    g = torch.arange(300, dtype=torch.int32)
    idx2, d22 = m.kneighbors(X[:300], k=2, exclude=(g, g))
    assert torch.equal(idx2, idx[:, 1:]) and torch.equal(d22, d2[:, 1:])


def test_wisdm_accuracy_above_majority_share(wisdm_csv):
    from har.models.base import features_tensor, labels_tensor
    from har.suite import load_wisdm

    train, test, _ = load_wisdm(wisdm_csv, "numeric43", 2018)
    Xt, yt = features_tensor(test, "features", "cpu"), labels_tensor(test, "label", "cpu")
    m = KNNClassifier(k=5, device="cpu").fit(train)
    acc = (m.predict(Xt) == yt).double().mean().item()
    majority = torch.bincount(yt).max().item() / yt.numel()
    print(f"WISDM numeric43 test accuracy: KNN(k=5, standardised) {acc:.4f}; majority-class share {majority:.4f} "
          f"({train.count()} training rows, {test.count()} test rows)")
    assert acc > majority


def test_leave_group_out_equals_refitting_without_each_group(blob_problem):
    X, y, _ = blob_problem
    X, y = X[:240], y[:240]
    groups = torch.randint(0, 7, (240,), generator=gen(3)).numpy()
    t = table_of(X, y, {"subject": groups})
    est = KNNClassifier(k=5, standardize=False, device="cpu")
    got = est.leave_group_out(t, "subject")
    want = torch.empty(240, dtype=torch.int64)
    for g in range(7):
        tr, te = np.nonzero(groups != g)[0], np.nonzero(groups == g)[0]
        want[te] = est.fit(t.take_rows(tr)).predict(X[te])
    assert torch.equal(got, want)
    loo = est.leave_group_out(t)
    for n in (0, 17, 239):
        keep = np.array([i for i in range(240) if i != n])
        assert int(loo[n]) == int(est.fit(t.take_rows(keep)).predict(X[n:n + 1])[0])


def test_cross_validator_one_search_equals_the_generic_loop(blob_problem):
    X, y, _ = blob_problem
    X, y = X[:400] * torch.linspace(0.5, 3.0, 43).view(1, -1), y[:400]        # mixed scales: standardising matters
    grid = ParamGridBuilder().addGrid("k", [1, 5, 9]).build()
    ev = MulticlassClassificationEvaluator(metricName="accuracy")

    class Plain(KNNClassifier):
        """The same estimator without the one-search branch: CrossValidator's generic take_rows loop."""
        cv_predictions = None

        def __getattribute__(self, name):
            if name == "cv_predictions":
                raise AttributeError(name)
            return super().__getattribute__(name)

    t = table_of(X, y)
    one = CrossValidator(KNNClassifier(standardize=False, device="cpu"), grid, ev, numFolds=4, seed=5).fit(t)
    loop = CrossValidator(Plain(standardize=False, device="cpu"), grid, ev, numFolds=4, seed=5).fit(t)
    assert not hasattr(Plain(), "cv_predictions")
    assert one.avgMetrics == pytest.approx(loop.avgMetrics, rel=0, abs=1e-12)   # exact counts over the fold sizes
    # standardize=True: the branch's moments are the whole table's
    mean, std = KN.standardizer(X)
    tz = table_of(KN.working_rows(X, mean, std), y)
    one = CrossValidator(KNNClassifier(standardize=True, device="cpu"), grid, ev, numFolds=4, seed=5).fit(t)
    loop = CrossValidator(Plain(standardize=False, device="cpu"), grid, ev, numFolds=4, seed=5).fit(tz)
    assert one.avgMetrics == pytest.approx(loop.avgMetrics, rel=0, abs=1e-12)
    assert one.bestModel.k in (1, 5, 9) and max(one.avgMetrics) > 0.9
    # a map outside {k, weights} keeps the generic loop
    other = CrossValidator(KNNClassifier(device="cpu"), [{"standardize": False}, {"standardize": True}], ev, numFolds=3,
                           seed=5).fit(t)
    assert len(other.avgMetrics) == 2


def test_persist_round_trip_is_bitwise(tmp_path, blob_problem):
    from har.utils import persist

    X, y, _ = blob_problem
    m = KNNClassifier(k=7, weights="distance", device="cpu").fit_tensors(X[:300], y[:300], 6)
    persist.save(m, str(tmp_path / "knn"))
    r = persist.load(str(tmp_path / "knn"), device="cpu")
    assert isinstance(r, KNNClassificationModel) and (r.k, r.weights, r.standardize) == (7, "distance", True)
    for u, v in zip(m.predict_all(X[300:500]), r.predict_all(X[300:500])):
        assert torch.equal(u, v)
    for u, v in zip(m.kneighbors(X[300:320]), r.kneighbors(X[300:320])):
        assert torch.equal(u, v)


def test_cli_preset_knn_then_predict_on_synthetic_raw(tmp_path):
    import main
    import predict
    from har.features.raw import raw_to_table, write_synthetic_raw

    p = str(tmp_path / "raw.csv")
    write_synthetic_raw(p, n_windows=120, users=4)
    mdir = tmp_path / "models"
    s = main.run(main.config_from_args(["--raw", p, "--out-dir", str(tmp_path / "out"), "--device", "cpu", "--preset",
                                        "knn", "--knn-k", "3", "--knn-weights", "distance", "--knn-group-col", "UID",
                                        "--save-models", str(mdir)]))
    rec = s["models"]["knn"]
    assert set(s["models"]) == {"knn"} and rec["accuracy"] > 0.5 and "KNNClassificationModel" in rec["model"]
    assert 0.0 <= rec["leave_group_out_accuracy"] <= 1.0 and rec["leave_group_out_groups"] >= 1
    with open(tmp_path / "out" / "result.txt") as f:
        text = f.read()
    assert "Leave-one-UID-out Accuracy" in text and "with k=3" in text
    t = raw_to_table(p)
    tab = tmp_path / "windows.csv"
    with open(tab, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(t.columns)
        cols = [t[c].data for c in t.columns]
        for i in range(t.count()):
            w.writerow([c[i] for c in cols])
    out = tmp_path / "pred.csv"
    got = predict.main(["--models", str(mdir), "--model", "knn", "--data", str(tab), "--device", "cpu", "--out",
                        str(out)])
    assert got["rows"] == 120 and got["accuracy"] > 0.5
    # without the switches nothing of the new classifier shows
    s2 = main.run(main.config_from_args(["--raw", p, "--out-dir", str(tmp_path / "out2"), "--device", "cpu",
                                         "--classifiers", "nb", "--encoding", "numeric43"]))
    with open(tmp_path / "out2" / "result.txt") as f:
        text2 = f.read()
    assert set(s2["models"]) == {"nb"} and "KNN" not in text2 and "Leave-one" not in text2
    assert "knn" not in main.config_from_args([]).classifiers
