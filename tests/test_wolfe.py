"""Breeze-semantics line searches for LogisticRegression (``lineSearch="wolfe"``):
the batched strong-Wolfe L-BFGS / backtracking OWL-QN of ``optim.lbfgs.minimize_wolfe`` (the CPU
oracle of the device path: the same function, the objective from the evaluation kernels)."""
import numpy as np
import pytest
import torch

from har.optim.lbfgs import minimize_trials, minimize_wolfe

N, F, K = 1500, 10, 4


def _problem(seed=0):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(K, F, generator=g)
    y = torch.randint(0, K, (N,), generator=g)
    X = (mu[y] + 1.5 * torch.randn(N, F, generator=g)).double()

    def data(x):  # the softmax cross entropy (mean) of B weight tables x [B, K (F + 1)] and its gradient
        B = x.shape[0]
        W = x.double().view(B, K, F + 1)
        z = torch.einsum("nf,bkf->bnk", X, W[:, :, :F]) + W[:, None, :, F]
        loss = torch.nn.functional.cross_entropy(z.reshape(-1, K), y.repeat(B), reduction="none").view(B, N).mean(1)
        p = torch.softmax(z, -1)
        p[:, torch.arange(N), y] -= 1
        p /= N
        G = torch.cat([torch.einsum("bnk,nf->bkf", p, X), p.sum(1)[:, :, None]], 2).reshape(B, -1)
        return loss, G.float()

    return data


def _reg(l2, l1):
    notb = torch.ones(K, F + 1)
    notb[:, F] = 0  # the intercept is not regularized
    l2v = (torch.tensor(l2)[:, None] * notb.reshape(1, -1)).float()
    l1v = (torch.tensor(l1)[:, None] * notb.reshape(1, -1)).float()
    return l2v, l1v


def test_wolfe_lbfgs_reaches_the_scipy_optimum():
    import scipy.optimize as so

    data = _problem()
    l2v, l1v = _reg([0.1, 0.01], [0.0, 0.0])
    r = minimize_wolfe(data, torch.zeros(2, K * (F + 1)), l2v, None, max_iter=300, tol=1e-12)
    for b in range(2):
        def fg(w):
            wt = torch.tensor(w)
            loss, G = data(wt[None])
            reg = l2v[b].double()
            return float(loss[0]) + 0.5 * float((reg * wt * wt).sum()), (G[0].double() + reg * wt).numpy()

        ref = so.minimize(fg, np.zeros(K * (F + 1)), jac=True, method="L-BFGS-B",
                          options=dict(maxiter=2000, gtol=1e-12, ftol=1e-15))
        assert abs(float(r.f[b]) - ref.fun) <= 1e-9 * max(1.0, abs(ref.fun)), (b, float(r.f[b]), ref.fun)


def test_wolfe_steps_satisfy_their_conditions_and_decrease():
    """Every accepted L-BFGS step satisfies the strong Wolfe conditions (Armijo, |phi'(t)| <= 0.9
    |phi'(0)|) and every accepted OWL-QN step Armijo + the weak curvature condition (phi'(t) >= 0.9
    phi'(0), phi' along the pseudo-gradient), on the line searches' own recorded values, which are
    tied to the path: phi(0) / phi(t) of consecutive steps are the objective history, and phi(t) is
    the objective recomputed at the accepted point.  The histories decrease; OWL-QN ends at the
    optimum a long Armijo-trial solve reaches."""
    data = _problem(1)
    l2v, l1v = _reg([0.05, 0.02], [0.0, 0.03])
    trace = []
    r = minimize_wolfe(data, torch.zeros(2, K * (F + 1)), l2v, l1v, max_iter=25, tol=1e-9, trace=trace)
    c1, c2 = 1e-4, 0.9
    for b in range(2):
        h = r.history_per_model[b]
        assert all(b2 <= a2 + 1e-12 for a2, b2 in zip(h, h[1:])), h
        steps = [s for s in trace if s["model"] == b]
        assert len(steps) == int(r.iterations[b]) >= 5, (b, len(steps))
        assert steps[0]["owl"] == (b == 1)
        for i, s in enumerate(steps):
            assert s["iter"] == i and s["t"] > 0
            assert s["d0"] < 0, s                                      # a descent direction
            assert s["ft"] <= s["f0"] + c1 * s["t"] * s["d0"], s       # Armijo (sufficient decrease)
            if b == 0:
                assert abs(s["dt"]) <= c2 * abs(s["d0"]), s           # strong curvature
            else:
                assert s["dt"] >= c2 * s["d0"], s                     # weak curvature
            assert s["f0"] == h[i] and s["ft"] == h[i + 1]           # the recorded values are the path's
    # phi(t) of the last accepted step is the objective at the solution, recomputed independently
    for b in range(2):
        loss, _ = data(r.x[b:b + 1])
        x = r.x[b].double()
        obj = float(loss[0]) + 0.5 * float((l2v[b].double() * x * x).sum()) + float((l1v[b].double() * x.abs()).sum())
        assert abs(obj - [s for s in trace if s["model"] == b][-1]["ft"]) <= 1e-9 * max(1.0, abs(obj))
    long = minimize_trials(data, torch.zeros(2, K * (F + 1)), l2v, l1v, max_iter=400, tol=1e-12)
    r2 = minimize_wolfe(data, torch.zeros(2, K * (F + 1)), l2v, l1v, max_iter=400, tol=1e-12)
    np.testing.assert_allclose(r2.f.numpy(), long.f.numpy(), rtol=1e-9)


def test_wolfe_batch_equals_single_model_solves():
    """Models advance their own line-search state machines: a batched solve of three models equals
    the three single-model solves (the same trial points, iterations and objective histories)."""
    data = _problem(2)
    l2v, l1v = _reg([0.1, 0.3, 0.05], [0.0, 0.0, 0.01])
    x0 = torch.zeros(3, K * (F + 1))
    rb = minimize_wolfe(data, x0, l2v, l1v, max_iter=20, tol=1e-6)
    for b in range(3):
        rs = minimize_wolfe(data, x0[b:b + 1], l2v[b:b + 1], l1v[b:b + 1] if l1v[b].any() else None,
                            max_iter=20, tol=1e-6)
        assert torch.equal(rs.x[0], rb.x[b]), b
        assert rs.iterations.tolist() == [int(rb.iterations[b])]
        n = len(rs.history_per_model[0])
        assert rs.history_per_model[0] == rb.history_per_model[b][:n]


MAX_ZOOM = 10  # minimize_wolfe's default zoom budget


class _FailOneSearch:
    """``evaluate`` with one sabotaged line search: from batched evaluation ``first_call`` on (0 = the initial
    one), for ``1 + MAX_ZOOM`` calls, model 0's loss is 10 above the true one — above phi(0) at every trial
    point, so its strong-Wolfe search goes bracket -> zoom and spends the zoom budget (one bracketing trial,
    ``MAX_ZOOM`` zoom trials) and fails.  The gradient and every other model are untouched; afterwards the
    wrapper is the plain callable."""

    def __init__(self, evaluate, first_call):
        self.evaluate, self.first, self.calls = evaluate, first_call, 0

    def __call__(self, x):
        loss, G = self.evaluate(x)
        if self.first <= self.calls < self.first + 1 + MAX_ZOOM:
            loss = loss.clone()
            loss[0] += 10.0
        self.calls += 1
        return loss, G


def _first_call_of_iteration(rounds_per_iter, k):
    """Index of the batched evaluation that is the first trial of batch iteration ``k``."""
    return 1 + sum(rounds_per_iter[:k])


def _check_history_is_the_path(h, iterations):
    assert len(h) == iterations + 1, (len(h), iterations)
    assert all(a != b for a, b in zip(h, h[1:])), h    # no value twice in a row: no row of a failed search


def test_wolfe_history_skips_a_failed_line_search():
    """A model whose line search fails once (history reset, retry from steepest descent) and then goes on:
    its ``history_per_model`` is the start objective plus one entry per step it TOOK — the failed batch
    iteration, which moves nothing, adds no row — while the other model of the batch is untouched."""
    data = _problem(3)
    l2v, l1v = _reg([0.05, 0.02], [0.0, 0.03])
    x0 = torch.zeros(2, K * (F + 1))
    kw = dict(max_iter=12, tol=1e-12, max_zoom=MAX_ZOOM)
    clean = minimize_wolfe(data, x0, l2v, l1v, **kw)
    assert clean.iterations.tolist() == [12, 12]
    k = 2  # the third batch iteration fails for model 0
    wrapped = _FailOneSearch(data, _first_call_of_iteration(clean.rounds_per_iter, k))
    trace = []
    r = minimize_wolfe(wrapped, x0, l2v, l1v, trace=trace, **kw)
    assert wrapped.calls > wrapped.first + 1 + MAX_ZOOM
    assert r.rounds_per_iter[:k] == clean.rounds_per_iter[:k] and r.rounds_per_iter[k] >= 1 + MAX_ZOOM
    # model 0 lost exactly that iteration, recovered, and went on
    assert r.iterations.tolist() == [11, 12] and int(r.iterations[0]) >= 3
    h = r.history_per_model[0]
    steps = [s for s in trace if s["model"] == 0]
    assert len(steps) == int(r.iterations[0])
    for i, s in enumerate(steps):
        assert s["iter"] == i
        assert h[i] == s["f0"] and h[i + 1] == s["ft"], (i, h[i], s["f0"], h[i + 1], s["ft"])
    _check_history_is_the_path(h, int(r.iterations[0]))
    assert h[:k + 1] == clean.history_per_model[0][:k + 1]          # the same path up to the failure
    assert all(b <= a for a, b in zip(h, h[1:])) and h[-1] == float(r.f[0])
    # model 1: bit-equal to the unwrapped solve
    assert r.history_per_model[1] == clean.history_per_model[1]
    assert torch.equal(r.x[1], clean.x[1]) and float(r.f[1]) == float(clean.f[1])
    _check_history_is_the_path(r.history_per_model[1], 12)
    assert len(r.history) == 13  # (the batch mean keeps one row per batch iteration)


def test_logistic_regression_wolfe_history_after_a_failed_search(monkeypatch):
    """``LogisticRegression(lineSearch="wolfe")`` through the same wrapper: the summaries' objectiveHistory is
    ``minimize_wolfe``'s ``history_per_model`` of that run — one owner of the history, no second cut."""
    from har.models import logreg as lr_mod
    from har.models.logreg import FitSpec, LogisticRegression

    g = torch.Generator().manual_seed(4)
    mu = torch.randn(K, F, generator=g)
    y = torch.randint(0, K, (N,), generator=g)
    X = mu[y] + 1.5 * torch.randn(N, F, generator=g)
    specs = [FitSpec(None, 0.05, 0.0), FitSpec(None, 0.02, 0.0)]
    est = lambda: LogisticRegression(maxIter=10, tol=1e-12, lineSearch="wolfe")  # noqa: E731
    clean = est().fit_many(X, y, specs, K)
    rounds = clean[0].summary["lineSearchRounds"]
    assert [m.summary["iterations"] for m in clean] == [10, 10]
    real = lr_mod.lbfgs.minimize_wolfe
    seen = {}

    def shim(evaluate, *a, **kw):
        seen["wrapper"] = w = _FailOneSearch(evaluate, _first_call_of_iteration(rounds, 2))
        seen["res"] = res = real(w, *a, **kw)
        return res

    monkeypatch.setattr(lr_mod.lbfgs, "minimize_wolfe", shim)
    ms = est().fit_many(X, y, specs, K)
    res = seen["res"]
    assert seen["wrapper"].calls > seen["wrapper"].first + 1 + MAX_ZOOM
    assert res.iterations.tolist() == [9, 10]
    for b, m in enumerate(ms):
        h = m.summary["objectiveHistory"]
        assert h == res.history_per_model[b]
        assert m.summary["iterations"] == int(res.iterations[b])
        _check_history_is_the_path(h, m.summary["iterations"])
        assert h[-1] == m.summary["objective"]
    assert ms[1].summary["objectiveHistory"] == clean[1].summary["objectiveHistory"]
    assert torch.equal(ms[1].coefficientMatrix, clean[1].coefficientMatrix)


def test_logistic_regression_wolfe_on_wisdm(wisdm_csv):
    """The reference's LR (maxIter 20, regParam 0.3) and an OWL-QN grid point with lineSearch="wolfe":
    accuracy at least the reference's (0.6148, result.txt:167), one objectiveHistory entry per
    iteration (+ the start), decreasing."""
    from har.data.csv_io import read_csv
    from har.data.split import random_split
    from har.features import wisdm
    from har.models.logreg import LogisticRegression

    _, _, df = wisdm.prepare(read_csv(wisdm_csv), "reference")
    train, test = random_split(df, [0.7, 0.3], 2018)
    for reg, a in ((0.3, 0.0), (0.1, 0.2)):
        m = LogisticRegression(maxIter=20, regParam=reg, elasticNetParam=a, lineSearch="wolfe").fit(train)
        s = m.summary
        h = s["objectiveHistory"]
        assert s["lineSearch"] == "wolfe" and len(h) == s["iterations"] + 1, (len(h), s["iterations"])
        assert all(b <= a2 + 1e-12 for a2, b in zip(h, h[1:]))
        assert len(s["lineSearchRounds"]) >= s["iterations"]
        out = m.transform(test)
        acc = float((out["prediction"].data == out["label"].data).mean())
        assert acc >= 0.61, (reg, a, acc)


def test_line_search_param_validated():
    from har.models.logreg import LogisticRegression

    with pytest.raises(ValueError):
        LogisticRegression(lineSearch="more-thuente")
