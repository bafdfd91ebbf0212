"""RidgeClassifier on the CPU: the definitions of har/ops/ridge.py against explicit refits, the selection rule,
persistence and the command lines, the accuracy on the rocket columns, and the properties of the fixtures that
tests/test_gpu_ridge.py relies on (asserted on the oracle alone)."""
import csv

import numpy as np
import pytest
import torch

from _ridge_util import EXCLUDED_CAP, FIT_ALPHAS, FIT_CASES, R, exact_case, excluded_rows, fit_case, gen
from har.models.ridge import RidgeClassificationModel, RidgeClassifier
from har.ops import ridge as RD
from har.utils import persist


# ------------------------------------------------------------------ 1. fold identity
def test_fold_systems_equal_explicit_refits():
    """N = 300, D = 7, K = 3, F = 4: every (fold, alpha) model of the one-pass oracle equals an fp64 solve on the
    centred training rows of that fold (the same whole-table scaling), rtol 1e-9; fold rows never enter their
    own system."""
    N, D, K, F = 300, 7, 3, 4
    g = gen(1)
    X = torch.randn(N, D, generator=g) * 2.0 + 1.0
    y = torch.randint(0, K, (N,), generator=g)
    fold = torch.randint(0, F, (N,), generator=g).numpy()
    alphas = [0.1, 1.0, 10.0]
    mean, inv_std = RD.standardizer(X)
    o = RD.fit_torch(X, y, fold, F, alphas, mean, inv_std, K)
    assert o.info == [0] * ((F + 1) * len(alphas))
    Z = RD.working_rows(X, mean, inv_std).double()
    T = RD.augment(Z.float(), y, K)[:, D:D + K].double()
    rows, off = RD.fold_order(fold, F)
    for f in list(range(F)) + [F]:
        tr = np.ones(N, dtype=bool) if f == F else fold != f
        if f < F:
            own = set(rows[off[f]:off[f + 1]].tolist())
            assert own == set(np.nonzero(fold == f)[0].tolist()) and not own & set(np.nonzero(tr)[0].tolist())
        Zt, Tt = Z[tr], T[tr]
        zm, tm = Zt.mean(0), Tt.mean(0)
        Zc = Zt - zm
        for ai, alpha in enumerate(alphas):
            W = torch.linalg.solve(Zc.T @ Zc + alpha * torch.eye(D, dtype=torch.float64), Zc.T @ (Tt - tm))
            b = tm - zm @ W
            s = f * len(alphas) + ai
            torch.testing.assert_close(o.W64[s], W.T, rtol=1e-9, atol=1e-12)
            torch.testing.assert_close(o.b_all[s].double(), b, rtol=1e-6, atol=1e-7)   # b is kept in fp32
    # a perturbed held-out row changes nothing in its own fold's systems
    X2 = X.clone()
    i = int(np.nonzero(fold == 2)[0][0])
    X2[i] += 1000.0
    o2 = RD.fit_torch(X2, y, fold, F, alphas, mean, inv_std, K)
    sl = slice(2 * len(alphas), 3 * len(alphas))
    torch.testing.assert_close(o2.W64[sl], o.W64[sl], rtol=1e-9, atol=1e-12)
    assert not torch.allclose(o2.W64[:len(alphas)], o.W64[:len(alphas)], rtol=1e-3)


def test_fp32_chain_emulation():
    """The chunked chains are exact on the exact-arithmetic fixture and an honest fp32 chain elsewhere."""
    X, y, rows, off, mean, inv_std = exact_case(17, 2, R + 1, 2)
    a32 = RD.moments_torch(X, y, rows, off, mean, inv_std, 2, "fp32")
    a64 = RD.moments_torch(X, y, rows, off, mean, inv_std, 2, "fp64")
    assert torch.equal(a32[0], a64[0]) and torch.equal(a32[1], a64[1])
    acc = torch.tensor([1.0], dtype=torch.float32)
    p = torch.tensor([2.0 ** -24 + 2.0 ** -60], dtype=torch.float64)       # above the tie: fmaf rounds up
    assert float(RD._fma32(acc, p)) == 1.0 + 2.0 ** -23
    assert float(RD._fma32(acc, torch.tensor([2.0 ** -24], dtype=torch.float64))) == 1.0   # the tie: to even


# ------------------------------------------------------------------ 2. selection
def test_selection_rule_and_range():
    a = torch.tensor([0.1, 10.0, 1.0], dtype=torch.float64)
    assert int(RD.choose_alpha(torch.tensor([5, 5, 5]), a)) == 1            # ties: the larger alpha
    assert int(RD.choose_alpha(torch.tensor([5, 4, 5]), a)) == 2
    assert int(RD.choose_alpha(torch.tensor([6, 5, 5]), a)) == 0
    g = gen(2)
    X, y = torch.randn(50, 3, generator=g), torch.randint(0, 2, (50,), generator=g)
    mean, inv_std = RD.standardizer(X)
    o = RD.fit_torch(X, y, np.zeros(50, dtype=np.int64), 1, [0.5, 2.0], mean, inv_std, 2)
    assert o.cvCorrect == [0, 0] and o.chosen == 1 and o.fold_pred is None and len(o.info) == 2   # F = 1: no selection
    m = RidgeClassifier(alphas=[3.0], numFolds=5).fit_tensors(X, y, 2)
    assert m.alpha == 3.0 and m.summary.numFolds == 1                       # one alpha: no folds
    for bad in (dict(D=RD.MAX_DIM, K=2), dict(D=3, K=1), dict(D=3, K=33), dict(D=3, K=2, F=17),
                dict(D=3, K=2, alphas=[0.0]), dict(D=3, K=2, alphas=[1.0] * 17), dict(D=3, K=2, alphas=[])):
        with pytest.raises(ValueError):
            RD.check_range(**bad)
    with pytest.raises(ValueError):
        RidgeClassifier(alphas=[-1.0]).fit_tensors(X, y, 2)
    raw, prob, pred = m.predict_all(X)
    assert torch.equal(pred, RD.first_argmax(raw)) and torch.allclose(prob.sum(1), torch.ones(50, dtype=torch.float64))
    assert int(RD.first_argmax(torch.tensor([[1.0, 2.0, 2.0]]))) == 1


def test_fold_column_and_cross_validator(tmp_path):
    from har.data.table import Column, Table
    from har.evaluation.evaluators import MulticlassClassificationEvaluator
    from har.tuning.crossval import CrossValidator, ParamGridBuilder

    g = gen(3)
    y = torch.randint(0, 3, (240,), generator=g)
    X = torch.randn(3, 5, generator=g)[y] * 2 + torch.randn(240, 5, generator=g)
    subj = np.array(["s%d" % (i % 4) for i in range(240)], dtype=object)
    t = Table([Column("features", "vector", X.double().numpy()), Column("label", "double", y.double().numpy()),
               Column("SUBJ", "string", subj)])
    m = RidgeClassifier(alphas=[0.1, 10.0], foldCol="SUBJ", device="cpu").fit(t)
    assert m.summary.numFolds == 4 and len(m.summary.info) == 10 and sum(m.summary.cvCorrect) > 240
    est = RidgeClassifier(alphas=[1.0], device="cpu")
    grid = ParamGridBuilder().addGrid("alphas", [[0.1], [100.0]]).build()
    cv = CrossValidator(estimator=est, estimatorParamMaps=grid, evaluator=MulticlassClassificationEvaluator(metricName="accuracy"),
                        numFolds=3, seed=1).fit(t)
    assert isinstance(cv.bestModel, RidgeClassificationModel) and len(cv.avgMetrics) == 2


# ------------------------------------------------------------------ 3. persistence and the command lines
def test_persist_round_trip_and_cli(tmp_path):
    import main
    import predict
    from har.features.raw import write_synthetic_raw

    p = str(tmp_path / "raw.csv")
    write_synthetic_raw(p, n_windows=160, users=5)
    out, mdir = tmp_path / "out", tmp_path / "models"
    s = main.run(main.config_from_args(["--raw", p, "--preset", "rocket-ridge", "--rocket", "420", "--ridge-folds", "3",
                                        "--ridge-alphas", "1,100", "--out-dir", str(out), "--device", "cpu",
                                        "--save-models", str(mdir)]))
    assert s["encoding"] == "rocket" and set(s["models"]) == {"ridge"} and s["models"]["ridge"]["accuracy"] > 0.5
    m = persist.load(str(mdir / "ridge"), device="cpu")
    assert isinstance(m, RidgeClassificationModel) and m.num_features == 420 and m.summary.numFolds == 3
    assert m.summary.alphas == [1.0, 100.0] and m.alpha in (1.0, 100.0) and len(m.summary.cvCorrect) == 2
    persist.save(m, str(tmp_path / "again"))
    r = persist.load(str(tmp_path / "again"), device="cpu")
    X = torch.rand(9, 420, generator=gen(4))
    assert torch.equal(r.predict_raw(X), m.predict_raw(X)) and r.summary == m.summary
    rec = predict.main(["--models", str(mdir), "--model", "ridge", "--raw", p, "--device", "cpu", "--out",
                        str(tmp_path / "p.csv")])
    assert rec["rows"] == 160
    with open(tmp_path / "p.csv") as f:
        assert len(list(csv.reader(f))) == 161
    cfg = main.config_from_args(["--raw", p, "--preset", "rocket-ridge"])
    assert cfg.rocket == 1680 and cfg.classifiers == ["ridge"] and len(cfg.ridge_alphas) == 10 and cfg.ridge_folds == 5
    assert np.allclose(cfg.ridge_alphas, RD.default_alphas())


# ------------------------------------------------------------------ 4. accuracy on the rocket columns
def test_ridge_on_rocket_columns_beats_lr_on_the_window_features():
    """StreamSpec() fixture of test_rocket.py, 2,000 training and the next 2,000 held-out windows: RidgeClassifier
    (default alphas, 5 folds) on the 1,680 rocket columns against LogisticRegression (the rocket test's
    parameters) on the 43 window features.  Measured: ridge 0.9265 (PARITY.md), window features 0.8795."""
    from har.data.table import Column, Table
    from har.features.rocket import RocketFeaturizer
    from har.features.window import window_features_torch
    from har.models.logreg import LogisticRegression
    from test_rocket import _fixture

    s, y = _fixture()
    W = 200
    y = torch.as_tensor(y).long()
    Xr = RocketFeaturizer().fit(s[: 2000 * W]).transform(s).float()
    Xw = torch.nan_to_num(window_features_torch(s, W, W, 20.0)[:, :43].double(), nan=-1.0)
    m = RidgeClassifier(device="cpu", seed=0).fit_tensors(Xr[:2000], y[:2000], int(y.max()) + 1)
    ridge = float((m.predict_all(Xr[2000:])[2].long() == y[2000:]).double().mean())
    train = Table([Column("features", "vector", Xw[:2000].numpy()),
                   Column("label", "double", y[:2000].numpy().astype(np.float64))])
    lr = LogisticRegression(maxIter=100, regParam=0.01, elasticNetParam=0.0, lineSearch="wolfe", device="cpu").fit(train)
    base = float((lr.predict_all(Xw[2000:].float())[2].long().cpu() == y[2000:]).double().mean())
    print(f"held-out accuracy: ridge on rocket {ridge:.4f} (alpha {m.alpha:g}, cvCorrect {m.summary.cvCorrect}), "
          f"LR on 43 window features {base:.4f}")
    assert m.summary.info == [0] * 60
    assert ridge > base


# ------------------------------------------------------------------ 5. fixture guards
@pytest.mark.parametrize("D", FIT_CASES)
def test_fit_fixture_guards(D):
    """What test_gpu_ridge.py::test_fit_end_to_end relies on: the oracle's own share of near-tie rows is far below
    the 2 % cap, and its best and second-best correct counts differ by more than the excluded row count."""
    c = fit_case(D)
    ex = excluded_rows(c)
    print(f"D = {D}: fp64 vs fp32-chain oracle difference {c['diff']:.3e}, tolerance {c['tol']:.3e}, excluded rows "
          f"{int(ex.sum())} of {ex.numel()}, cvCorrect {c['o64'].cvCorrect}")
    assert float(ex.double().mean()) < EXCLUDED_CAP / 10
    cnt = sorted(c["o64"].cvCorrect)
    assert cnt[-1] - cnt[-2] > int(ex.sum())
    assert c["o64"].chosen == c["o32"].chosen and c["o64"].info == [0] * (6 * len(FIT_ALPHAS))
    assert c["tol"] < 1e-3
