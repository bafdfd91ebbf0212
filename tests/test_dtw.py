"""Banded dynamic time warping (har/ops/dtw.py), the DTWClassifier and the raw-sample plumbing, on the CPU.

Integer-valued windows make every fp64 sum exact, so the definition is held to equality: against a brute-force
enumeration of every admissible warping path, and against closed forms."""
import csv

import numpy as np
import pytest
import torch

from _dtw_util import brute_force, groups, integer_windows, pulse_problem, table_of
from har.models.dtw import DTWClassificationModel, DTWClassifier
from har.ops import dtw as DT
from har.utils import persist


# ------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("W", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("A", [1, 3])
def test_cost_equals_brute_force_path_enumeration(W, A):
    Q, R = integer_windows(3, W, A, 10 * W + A, amax=4), integer_windows(4, W, A, 77 * W + A, amax=4)
    for radius in sorted({0, min(1, W - 1), W - 1}):
        got = DT.cost_torch(Q, R, radius)
        assert got.dtype == torch.float64 and tuple(got.shape) == (3, 4)
        want = torch.tensor([[brute_force(q, r, radius) for r in R] for q in Q], dtype=torch.float64)
        assert torch.equal(got, want), (W, A, radius)


def test_closed_forms():
    W, A = 12, 3
    Q, R = integer_windows(5, W, A, 1), integer_windows(6, W, A, 2)
    sq = ((Q.double()[:, None] - R.double()[None]) ** 2).sum(dim=(2, 3))
    assert torch.equal(DT.cost_torch(Q, R, 0), sq)                                  # R = 0: squared Euclidean
    a, b = torch.full((1, W, A), 3.0), torch.full((1, W, A), -2.0)
    for radius in (0, 2, W - 1):
        assert float(DT.cost_torch(a, b, radius)) == W * A * 25.0                   # two constant windows
        assert torch.equal(DT.cost_torch(Q, R, radius), DT.cost_torch(R, Q, radius).t())   # symmetry
    costs = [DT.cost_torch(Q, R, radius) for radius in range(W)]
    for lo, hi in zip(costs, costs[1:]):
        assert bool((hi <= lo).all())                                               # non-increasing in R
    assert bool((costs[-1] < costs[0]).any())


def test_shifted_pattern_costs_zero_inside_the_band():
    W, s_max, radius = 24, 5, 3
    base = torch.zeros(W, 2)
    base[s_max:W - s_max] = integer_windows(1, W - 2 * s_max, 2, 5, lo=1)[0]        # >= s zero samples on both ends
    for s in range(-s_max, s_max + 1):
        c = float(DT.cost_torch(base[None], torch.roll(base, s, dims=0)[None], radius))
        assert (c == 0.0) if abs(s) <= radius else (c > 0.0), (s, c)


# ------------------------------------------------------------------ 2. neighbour rules
def test_neighbour_rules():
    W, A, radius = 9, 2, 2
    Q, R = integer_windows(7, W, A, 3), integer_windows(11, W, A, 4)
    R = torch.cat([R, R[:4]], 0)                                                    # duplicates: 11..14 == 0..3
    cost = DT.cost_torch(Q, R, radius)
    idx, d2 = DT.neighbors_torch(Q, R, 15, radius)
    for n in range(7):
        pairs = sorted((float(cost[n, m]), m) for m in range(15))
        assert idx[n].tolist() == [m for _, m in pairs] and d2[n].tolist() == [c for c, _ in pairs]
        pos = {m: i for i, m in enumerate(idx[n].tolist())}
        assert all(pos[m] < pos[m + 11] for m in range(4))                          # the lower index first
    for kp in (1, 4):
        i2, e2 = DT.neighbors_torch(Q, R, kp, radius)
        assert torch.equal(i2, idx[:, :kp]) and torch.equal(e2, d2[:, :kp])         # k prefixes
    qg, rg = groups(7, 15, 9, ngroups=3)
    gi, gd = DT.neighbors_torch(Q, R, 15, radius, qg, rg)
    for n in range(7):
        ok = [m for m in range(15) if not (int(qg[n]) >= 0 and int(qg[n]) == int(rg[m]))]
        assert [m for m in gi[n].tolist() if m >= 0] == [m for m in idx[n].tolist() if m in ok]
        assert gi[n, len(ok):].tolist() == [-1] * (15 - len(ok)) and bool(torch.isinf(gd[n, len(ok):]).all())
    i3, e3 = DT.neighbors_torch(Q, R[:3], 5, radius)                                # M < k
    assert bool((i3[:, 3:] == -1).all()) and bool(torch.isinf(e3[:, 3:]).all()) and bool((i3[:, :3] >= 0).all())


def test_zscore_and_radius_resolution():
    X = integer_windows(4, 10, 3, 6)
    X[:, :, 1] = 5.0                                                                # a constant axis keeps scale 1
    Z = DT.zscore(X)
    assert torch.allclose(Z[:, :, 0].double().mean(1), torch.zeros(4, dtype=torch.float64), atol=1e-6)
    assert torch.allclose(Z[:, :, 0].double().pow(2).mean(1), torch.ones(4, dtype=torch.float64), atol=1e-5)
    assert bool((Z[:, :, 1] == 0).all())
    m = DTWClassifier(band=0.1, axes=3, device="cpu").fit_tensors(X.reshape(4, -1), torch.tensor([0, 1, 0, 1]), 2)
    assert m.radius == 1 and m.window == 10 and m.axes == 3
    assert DTWClassifier(radius=4, band=0.5, axes=3, device="cpu").fit_tensors(
        X.reshape(4, -1), torch.tensor([0, 1, 0, 1]), 2).radius == 4


# ------------------------------------------------------------------ 3. the classifier
def test_pulse_problem_is_solved_exactly_and_round_trips(tmp_path):
    W, R, C = 48, 6, 4
    Xtr, ytr = pulse_problem(6, C, W, R, 1)
    Xte, yte = pulse_problem(5, C, W, R, 2)
    acc = {}
    for radius in (R, 0):
        m = DTWClassifier(k=1, radius=radius, axes=1, device="cpu").fit(table_of(Xtr, ytr))
        raw, prob, pred = m.predict_all(Xte.reshape(Xte.shape[0], -1))
        acc[radius] = float((pred == yte).double().mean())
        if radius == R:
            idx, d2 = m.kneighbors(Xte.reshape(Xte.shape[0], -1), k=1)
            assert bool((d2 == 0).all()) and torch.equal(ytr[idx[:, 0].long()], yte)
            persist.save(m, str(tmp_path / "dtw"))
            again = persist.load(str(tmp_path / "dtw"), device="cpu")
            assert isinstance(again, DTWClassificationModel) and again.radius == R
            for a, b in zip(again.predict_all(Xte.reshape(Xte.shape[0], -1)), (raw, prob, pred)):
                assert torch.equal(a, b)
    print(f"pulse problem, 1-NN accuracy: DTW radius {R}: {acc[R]:.4f}, radius 0 (Euclidean): {acc[0]:.4f}")
    assert acc[R] == 1.0


def test_leave_group_out_and_cv_branch_equal_refitting():
    from har.evaluation.evaluators import MulticlassClassificationEvaluator
    from har.tuning.crossval import CrossValidator, ParamGridBuilder

    X, y = pulse_problem(6, 3, 40, 4, 3)
    X = X + integer_windows(18, 40, 1, 8, amax=1)
    user = np.arange(18) % 4
    t = table_of(X, y, {"USER": user})
    est = DTWClassifier(k=3, radius=4, axes=1, weights="distance", device="cpu")
    lgo = est.leave_group_out(t, "USER")
    for u in range(4):
        tr, te = np.nonzero(user != u)[0], np.nonzero(user == u)[0]
        m = est.fit(table_of(X[tr], y[tr]))
        assert torch.equal(m.predict_all(X[te].reshape(len(te), -1))[2], lgo[te])
    grid = ParamGridBuilder().addGrid("k", [1, 3]).addGrid("weights", ["uniform", "distance"]).build()
    cv = CrossValidator(estimator=est, estimatorParamMaps=grid, evaluator=MulticlassClassificationEvaluator(
        metricName="accuracy"), numFolds=3, seed=7)
    model = cv.fit(t)
    assert len(model.avgMetrics) == 4 and all(0.0 <= v <= 1.0 for v in model.avgMetrics)


def test_range_errors():
    Q, R = integer_windows(2, 8, 3, 1), integer_windows(3, 8, 3, 2)
    with pytest.raises(ValueError, match="k in"):
        DT.neighbors_torch(Q, R, 0, 1)
    with pytest.raises(ValueError, match="k in"):
        DT.neighbors_torch(Q, R, DT.MAX_K + 1, 1)
    with pytest.raises(ValueError, match="samples"):
        DT.cost_torch(torch.zeros(1, DT.MAX_W + 1, 1), torch.zeros(1, DT.MAX_W + 1, 1), 0)
    with pytest.raises(ValueError, match="axes"):
        DT.cost_torch(torch.zeros(1, 4, 10), torch.zeros(1, 4, 10), 0)
    with pytest.raises(ValueError, match="radius"):
        DT.cost_torch(Q, R, -1)
    with pytest.raises(ValueError, match="W - 1"):
        DT.cost_torch(Q, R, 8)
    with pytest.raises(ValueError, match="radius"):
        DT.cost_torch(torch.zeros(1, 100, 1), torch.zeros(1, 100, 1), DT.MAX_RADIUS + 1)
    with pytest.raises(ValueError, match="differ"):
        DT.cost_torch(Q, integer_windows(3, 9, 3, 2), 1)
    with pytest.raises(ValueError, match="classes"):
        DT.search_torch(Q, R, 1, 1, y=torch.zeros(3, dtype=torch.int64), C=DT.MAX_CLASSES + 1)
    with pytest.raises(ValueError, match="weights"):
        DT.search_torch(Q, R, 1, 1, y=torch.zeros(3, dtype=torch.int64), C=2, weights="gaussian")
    with pytest.raises(ValueError, match="both"):
        DT.neighbors_torch(Q, R, 1, 1, qgroup=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="normalize"):
        DTWClassifier(normalize="minmax", axes=3, device="cpu").fit_tensors(Q.reshape(2, -1), torch.tensor([0, 1]), 2)
    with pytest.raises(ValueError, match="axes"):
        DTWClassifier(axes=5, device="cpu").fit_tensors(Q.reshape(2, -1), torch.tensor([0, 1]), 2)
    m = DTWClassifier(radius=1, axes=3, device="cpu").fit_tensors(Q.reshape(2, -1), torch.tensor([0, 1]), 2)
    with pytest.raises(ValueError, match="rows"):
        m.predict_all(torch.zeros(2, 27))


# ------------------------------------------------------------------ 4. raw samples through the table and the command lines
def test_raw_sample_columns_and_cli_end_to_end(tmp_path):
    import main
    import predict
    from har.data.split import split_ids
    from har.features.raw import ACTIVITIES, WISDM43, raw_to_table, read_raw, sample_cols, write_synthetic_raw

    p = str(tmp_path / "raw.csv")
    info = write_synthetic_raw(p, n_windows=96, users=4, hz=10.0, window_sec=4.0)
    W = info["window"]
    plain = raw_to_table(p, hz=10.0, window_sec=4.0)
    t = raw_to_table(p, hz=10.0, window_sec=4.0, samples=True)
    assert plain.columns == ["UID", "USER"] + WISDM43 + ["ACTIVITY"]               # switch off: the table as it was
    assert t.columns == plain.columns + sample_cols(W) and t.count() == 96
    assert sample_cols(W)[:4] == ["RAW0_X", "RAW0_Y", "RAW0_Z", "RAW1_X"]          # time-major
    xyz = read_raw(p)[3]
    S = np.stack([np.asarray(t[c].data) for c in sample_cols(W)], 1)
    assert np.array_equal(S, xyz.reshape(96, W * 3).astype(np.float64))
    for c in plain.columns:
        assert np.array_equal(np.asarray(t[c].data), np.asarray(plain[c].data))

    with pytest.raises(SystemExit):
        main.config_from_args(["--preset", "dtw"])                                  # needs --raw
    out, mdir = tmp_path / "out", tmp_path / "models"
    s = main.run(main.config_from_args(["--raw", p, "--hz", "10", "--window-sec", "4", "--preset", "dtw",
                                        "--dtw-group-col", "USER", "--out-dir", str(out), "--device", "cpu",
                                        "--save-models", str(mdir)]))
    assert s["encoding"] == "raw" and s["n_train"] + s["n_test"] == 96 and set(s["models"]) == {"dtw"}
    rec = s["models"]["dtw"]
    text = (out / "result.txt").read_text()
    assert "MultiClass Accuracy -------------------------: %g" % rec["accuracy"] in text
    assert "Leave-one-USER-out Accuracy = %g  (4 groups" % rec["leave_group_out_accuracy"] in text
    assert rec["accuracy"] > 0.5
    print(f"synthetic stream (96 windows of {W} x 3): DTW 1-NN accuracy {rec['accuracy']:.4f}, "
          f"leave-one-USER-out {rec['leave_group_out_accuracy']:.4f}")
    r = predict.main(["--models", str(mdir), "--model", "dtw", "--raw", p, "--device", "cpu", "--out",
                      str(tmp_path / "p.csv")])
    assert r["rows"] == 96
    with open(tmp_path / "p.csv") as f:
        rows = list(csv.reader(f))[1:]
    pred = np.array([row[3] for row in rows])
    truth = np.array([ACTIVITIES[int(v)] for v in info["labels"]])
    test = split_ids(96, [0.7, 0.3], 2018) == 1
    assert int(test.sum()) == s["n_test"]
    assert float((pred[test] == truth[test]).mean()) == pytest.approx(rec["accuracy"], abs=1e-12)
