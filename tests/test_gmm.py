"""GaussianMixture on the CPU: the PyTorch definitions of har/ops/gmm.py against closed forms, a hand-written
scalar implementation and the properties of EM, then the model surface and the command line."""
import csv
import math
import os
import re

import numpy as np
import pytest
import torch

from _gmm_util import ESTEP_SHAPES, clear_rows, em_history, gen, operands_case, q_reference, row_weights, small_problem
from _kmeans_util import blobs
from har.data.table import Column, Table
from har.models.gmm import GaussianMixture, GaussianMixtureModel
from har.ops import gmm as GM

F64 = torch.float64


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("weighted", [False, True])
def test_k1_step_is_the_sample_mean_and_covariance(weighted):
    g = gen(4)
    Z = (torch.randn(300, 5, generator=g) @ (torch.randn(5, 5, generator=g) * 0.5 + torch.eye(5))).contiguous()
    w = row_weights(300, 9) if weighted else None
    assert w is None or bool((w == 0).any())
    mu0 = torch.randn(1, 5, generator=g)                       # any start
    W0 = torch.triu(torch.randn(1, 5, 5, generator=g) * 0.2, 1) + torch.diag_embed(0.5 + torch.rand(1, 5, generator=g))
    c0 = torch.zeros(1)
    e = GM.estep_torch(Z, mu0, W0, c0, w)
    assert torch.equal(e.resp, torch.ones(300, 1, dtype=F64))
    f = GM.finish_torch(e.Nk, e.S1, e.S2, mu0, W0, 1e-6)
    aw = None if w is None else w.double()
    wsum = 300.0 if w is None else float(aw.sum())
    mean = Z.double().mean(dim=0) if w is None else (Z.double() * aw.view(-1, 1)).sum(dim=0) / wsum
    cov = torch.cov(Z.double().t(), correction=0, aweights=aw)
    torch.testing.assert_close(f.mu64[0], mean, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(f.Sigma[0], cov + 1e-6 * torch.eye(5, dtype=F64), rtol=1e-10, atol=1e-12)
    assert float(f.pi[0]) == 1.0 and float(f.Nk[0]) == pytest.approx(wsum, rel=1e-12)
    # the factor: W^T Sigma W = I, W upper triangular, c from its diagonal
    Wd = f.W64[0]
    torch.testing.assert_close(Wd.t() @ f.Sigma[0] @ Wd, torch.eye(5, dtype=F64), rtol=0, atol=1e-10)
    assert float(torch.tril(Wd, -1).abs().max()) == 0.0
    logdet = 0.5 * torch.logdet(f.Sigma[0])
    assert float(f.c[0]) == pytest.approx(float(-2.5 * math.log(2 * math.pi) - logdet), rel=1e-6)


def test_enumeration_k2_d1_n6():
    """r, lse and one M-step against scalar arithmetic written out by hand."""
    z = [-1.5, -0.25, 0.0, 0.75, 2.0, 3.5]
    mu, sd, pi = [-0.5, 2.5], [0.75, 1.25], [0.375, 0.625]
    Z = torch.tensor(z, dtype=torch.float32).view(6, 1)
    mut = torch.tensor(mu, dtype=torch.float32).view(2, 1)
    W = torch.tensor([1.0 / s for s in sd], dtype=torch.float32).view(2, 1, 1)
    c = torch.tensor([math.log(p) - 0.5 * math.log(2 * math.pi) - math.log(s) for p, s in zip(pi, sd)], dtype=torch.float32)
    e = GM.estep_torch(Z, mut, W, c)
    cf, wf = [float(v) for v in c.double()], [float(v) for v in W.double().view(-1)]   # the fp32 operands, exactly
    r_ref, lse_ref = [], []
    for x in z:
        t = [cf[k] - 0.5 * ((x - mu[k]) * wf[k]) ** 2 for k in range(2)]
        m = max(t)
        l = m + math.log(sum(math.exp(v - m) for v in t))
        lse_ref.append(l)
        r_ref.append([math.exp(v - l) for v in t])
    torch.testing.assert_close(e.resp, torch.tensor(r_ref, dtype=F64), rtol=1e-12, atol=0)
    torch.testing.assert_close(e.lse, torch.tensor(lse_ref, dtype=F64), rtol=1e-12, atol=0)
    assert float(e.loglik) == pytest.approx(sum(lse_ref), rel=1e-12)
    assert e.pred.tolist() == [0 if a >= b else 1 for a, b in r_ref]
    f = GM.finish_torch(e.Nk, e.S1, e.S2, mut, W, 1e-6)
    for k in range(2):
        nk = sum(r[k] for r in r_ref)
        m1 = sum(r[k] * x for r, x in zip(r_ref, z)) / nk
        var = sum(r[k] * (x - m1) ** 2 for r, x in zip(r_ref, z)) / nk + 1e-6
        assert float(f.Nk[k]) == pytest.approx(nk, rel=1e-12)
        assert float(f.pi[k]) == pytest.approx(nk / 6.0, rel=1e-12)
        assert float(f.mu64[k, 0]) == pytest.approx(m1, rel=1e-12)
        assert float(f.Sigma[k, 0, 0]) == pytest.approx(var, rel=1e-12)
        assert float(f.W64[k, 0, 0]) == pytest.approx(var ** -0.5, rel=1e-12)
        assert float(f.c[k]) == pytest.approx(math.log(nk / 6.0) - 0.5 * math.log(2 * math.pi) - 0.5 * math.log(var), rel=1e-6)


def test_finish_keeps_empty_and_singular_components():
    g = gen(8)
    Z = torch.randn(200, 3, generator=g)
    Z[:, 2] = Z[:, 0]                                   # rank deficient
    mu = Z[:3].clone()
    W = torch.diag_embed(0.5 + torch.rand(3, 3, generator=g))
    r = torch.softmax(torch.randn(200, 3, generator=g), dim=1).double()
    r[:, 1] = 0.0
    Nk, S1, S2 = GM.moments_torch(Z, mu, r)
    f = GM.finish_torch(Nk, S1, S2, mu, W, 0.0)
    assert f.updated.tolist() == [False, False, False] or not bool(f.updated[1])
    assert torch.equal(f.W[1], W[1]) and torch.equal(f.mu[1], mu[1]) and float(f.pi[1]) == 0.0
    assert float(f.c[1]) == float("-inf")
    torch.testing.assert_close(f.pi.sum(), torch.tensor(1.0, dtype=F64))
    f = GM.finish_torch(Nk, S1, S2, mu, W, 1e-3)        # regCovar rescues the rank-deficient components
    assert f.updated.tolist() == [True, False, True] and bool(torch.isfinite(f.W).all())
    d = GM.finish_torch(Nk, S1, S2, mu, W, 1e-3, diag=True)
    assert float((d.Sigma[0] - torch.diag(torch.diagonal(d.Sigma[0]))).abs().max()) == 0.0
    torch.testing.assert_close(torch.diagonal(d.Sigma[0]), torch.diagonal(f.Sigma[0]))


# ------------------------------------------------------------------ EM
@pytest.fixture(scope="module")
def blob_problem():
    return blobs(2000, 43, 6)


def _working(X):
    mean, std, inv = GM.standardizer(X)
    return GM.working_rows(X, mean, inv), mean, std, inv


def test_em_never_decreases_the_log_likelihood(blob_problem):
    X, _, _ = blob_problem
    Z, mean, _, inv = _working(X)
    h, _ = em_history(Z, ((X[:6] - mean) * inv).contiguous(), 8)
    Xs, _, mus, _ = small_problem()
    Zs, means, _, invs = _working(Xs)
    hs, _ = em_history(Zs, ((Xs[:3] - means) * invs).contiguous(), 8)
    hw, _ = em_history(Zs, ((Xs[:3] - means) * invs).contiguous(), 8, w=row_weights(513, 2))
    for hist in (h, hs, hw):
        assert hist.numel() == 8 and bool(torch.isfinite(hist).all())
        for a, b in zip(hist[:-1].tolist(), hist[1:].tolist()):
            assert b >= a - 1e-9 * abs(a)
    assert float(h[-1]) > float(h[0])


def test_standardizer_and_constant_columns():
    g = gen(2)
    X = torch.randn(50, 4, generator=g) * torch.tensor([1.0, 100.0, 1e-3, 1.0]) + torch.tensor([0.0, 5.0, -2.0, 7.0])
    X[:, 3] = 7.0
    mean, std, inv = GM.standardizer(X)
    assert float(std[3]) == 1.0 and float(inv[3]) == 1.0
    Z = GM.working_rows(X, mean, inv)
    torch.testing.assert_close(Z[:, :3].double().std(dim=0, unbiased=False), torch.ones(3, dtype=F64), rtol=1e-5, atol=0)
    assert float(Z[:, 3].abs().max()) == 0.0
    assert sorted(GM.random_init_rows(3, 5, 50).tolist()) != sorted(GM.random_init_rows(4, 5, 50).tolist())
    assert len(set(GM.random_init_rows(3, 5, 50).tolist())) == 5


@pytest.mark.parametrize("N,D,K", ESTEP_SHAPES)
def test_excluded_share_of_the_gpu_tie_rule(N, D, K):
    """The condition the GPU suite's prediction test rests on, from the fp64 oracle alone, same seeds."""
    Z, mu, W, c = operands_case(N, D, K)
    q, b = q_reference(Z, mu, W)
    pred, clear = clear_rows(q, b, c)
    assert 1.0 - clear.double().mean().item() <= 0.01
    assert torch.equal(pred, GM.estep_torch(Z, mu, W, c, want_moments=False).pred)


# ------------------------------------------------------------------ recovery
def _match(est_means, true_means):
    cost = torch.cdist(est_means.double(), true_means.double())
    import itertools

    best = min(itertools.permutations(range(true_means.shape[0])), key=lambda p: sum(cost[i, p[i]] for i in range(len(p))))
    return list(best)


def test_recovers_three_full_covariance_gaussians():
    g = gen(12)
    K, D, N = 3, 5, 3000
    mu = torch.tensor([[0.0, 0, 0, 0, 0], [6.0, 3, -2, 1, 0], [-4.0, 5, 3, -3, 2]])
    A = torch.randn(K, D, D, generator=g) * 0.45 + torch.eye(D) * torch.tensor([1.0, 0.7, 1.4]).view(K, 1, 1)
    pi = torch.tensor([0.5, 0.3, 0.2])
    y = torch.multinomial(pi, N, replacement=True, generator=g)
    X = (mu[y] + torch.einsum("nd,nde->ne", torch.randn(N, D, generator=g), A[y])).contiguous()
    Sig = A.transpose(1, 2) @ A
    model = GaussianMixture(k=3, maxIter=50, tol=1e-3, seed=1).fit_tensors(X)
    means, covs = model.gaussians()
    perm = _match(means, mu)
    for i, j in enumerate(perm):
        assert float((means[i] - mu[j].double()).abs().max()) <= 0.15
        assert abs(float(model.weights[i]) - float(pi[j])) <= 0.03
        rel = torch.linalg.matrix_norm(covs[i] - Sig[j].double()) / torch.linalg.matrix_norm(Sig[j].double())
        assert float(rel) <= 0.25
    assert model.summary.converged and sum(model.summary.clusterSizes) == N
    acc = float((torch.tensor(perm)[model.predict(X)] == y).double().mean())
    assert acc > 0.97


def test_diag_recovers_axis_aligned_gaussians():
    g = gen(13)
    K, D, N = 3, 5, 3000
    mu = torch.tensor([[0.0, 0, 0, 0, 0], [5.0, 3, -2, 1, 0], [-4.0, 5, 3, -3, 2]])
    # sd <= 1.5: the sample mean of ~1,000 rows then has a standard error <= 0.048, so the 0.15 below is > 3 sigma
    sd = 0.5 + 1.0 * torch.rand(K, D, generator=g)
    y = torch.randint(0, K, (N,), generator=g)
    X = (mu[y] + torch.randn(N, D, generator=g) * sd[y]).contiguous()
    model = GaussianMixture(k=3, maxIter=50, tol=1e-3, seed=1, covarianceType="diag").fit_tensors(X)
    means, covs = model.gaussians()
    for i, j in enumerate(_match(means, mu)):
        assert float((means[i] - mu[j].double()).abs().max()) <= 0.15
        assert abs(float(model.weights[i]) - 1.0 / 3.0) <= 0.03
        true = torch.diag(sd[j].double() ** 2)
        assert float(torch.linalg.matrix_norm(covs[i] - true) / torch.linalg.matrix_norm(true)) <= 0.25
        off = covs[i] - torch.diag(torch.diagonal(covs[i]))
        assert float(off.abs().max()) <= 1e-9


# ------------------------------------------------------------------ model surface
def test_gaussians_map_back_to_the_original_coordinates():
    X, _, _, _ = small_problem()
    a = torch.tensor([2.0, 0.5, 10.0, 1.0, 3.0])
    b = torch.tensor([1.0, -20.0, 0.0, 4.0, 100.0])
    init = X[:3].clone()
    m1 = GaussianMixture(k=3, maxIter=10, tol=0.0)._fit_tensors(X, initial_means=init)
    m2 = GaussianMixture(k=3, maxIter=10, tol=0.0)._fit_tensors(X * a + b, initial_means=init * a + b)
    mu1, S1 = m1.gaussians()
    mu2, S2 = m2.gaussians()
    torch.testing.assert_close(mu2, mu1 * a.double() + b.double(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(S2, S1 * a.double().view(1, -1, 1) * a.double().view(1, 1, -1), rtol=2e-3, atol=1e-5)
    torch.testing.assert_close(m2.weights, m1.weights, rtol=1e-4, atol=1e-6)
    # the density transforms with the Jacobian
    torch.testing.assert_close(m2.score_samples(X * a + b), m1.score_samples(X) - float(torch.log(a.double()).sum()),
                               rtol=0, atol=2e-3)


def test_score_samples_integrates_to_one():
    g = gen(21)
    y = torch.randint(0, 2, (800,), generator=g)
    X = (torch.where(y == 0, -30.0, 50.0) + torch.randn(800, generator=g) * torch.where(y == 0, 4.0, 9.0)).view(-1, 1)
    model = GaussianMixture(k=2, maxIter=30, seed=0).fit_tensors(X)
    grid = torch.linspace(-130.0, 190.0, 64001, dtype=F64).view(-1, 1)
    dens = torch.exp(model.score_samples(grid))
    assert float(dens.sum() * (320.0 / 64000)) == pytest.approx(1.0, abs=1e-4)
    p = model.predictProbability(X)
    torch.testing.assert_close(p.sum(dim=1), torch.ones(800, dtype=p.dtype), rtol=0, atol=1e-12)
    assert torch.equal(model.predict(X), p.argmax(dim=1))


def test_persist_round_trip_and_native_range(tmp_path):
    from har.utils import persist

    X, y, _, _ = small_problem()
    model = GaussianMixture(k=3, maxIter=15, seed=3, probabilityCol="p").fit(Table([Column("features", "vector", X.double().numpy())]))
    model.label_map(model.predict(X), y, 3)
    persist.save(model, str(tmp_path / "gmm"), labels=list("abc"))
    back = persist.load(str(tmp_path / "gmm"), device="cpu")
    assert isinstance(back, GaussianMixtureModel) and back.uid == model.uid and back.probabilityCol == "p"
    assert torch.equal(back.predict(X), model.predict(X)) and torch.equal(back.score_samples(X), model.score_samples(X))
    assert torch.equal(back.weights, model.weights) and back.majority_labels == model.majority_labels
    assert back.summary.as_dict() == model.summary.as_dict()
    s = model.summary
    assert s.k == 3 and len(s.logLikelihoodHistory) == s.numIter <= 15 and sum(s.clusterSizes) == 513
    # the native range holds on the CPU too
    with pytest.raises(ValueError):
        GaussianMixture(k=65).fit_tensors(torch.randn(100, 4))
    with pytest.raises(ValueError):
        GaussianMixture(k=2).fit_tensors(torch.randn(100, 129))
    with pytest.raises(ValueError):
        GaussianMixture(k=0).fit_tensors(torch.randn(100, 4))
    with pytest.raises(ValueError):
        GaussianMixture(k=2, covarianceType="tied").fit_tensors(torch.randn(100, 4))
    with pytest.raises(ValueError):
        GaussianMixture(k=2, initMode="k-means++").fit_tensors(torch.randn(100, 4))
    r = GaussianMixture(k=4, initMode="random", maxIter=5, seed=5).fit_tensors(X)
    assert r.k == 4 and sum(r.summary.clusterSizes) == 513


# ------------------------------------------------------------------ composition with the HMM smoother
def test_mixture_probabilities_feed_the_hmm_smoother():
    from har.data.synth import StreamSpec, generate_stream
    from har.features.window import window_features_torch
    from har.models.hmm import HMMSmoother
    from har.ops import hmm as H

    spec, n = StreamSpec(), 2000
    xs, _ = generate_stream(2 * n, spec)
    F = window_features_torch(xs, spec.window, spec.window, spec.hz)[:, :43]
    F = torch.nan_to_num(F.float(), nan=0.0, posinf=0.0, neginf=0.0)
    train = Table([Column("features", "vector", F[:n].double().numpy())])
    test = Table([Column("features", "vector", F[n:].double().numpy())])
    out = GaussianMixture(6).fit(train).transform(test)
    prob = torch.as_tensor(out["probability"].data)
    assert prob.shape == (n, 6)
    smoother = HMMSmoother(stay=0.9, numClasses=6).fit(out)
    one = torch.tensor([0, n], dtype=torch.int64)
    path, _ = smoother.decode(prob, one)
    raw = torch.as_tensor(out["prediction"].data).to(torch.int32)
    segs, raw_segs = H.count_segments(path, one), H.count_segments(raw, one)
    print(f"mixture -> HMM: {raw_segs} raw segments -> {segs} smoothed")
    assert segs < raw_segs


# ------------------------------------------------------------------ command line
def _stable(text):
    keep = [l for l in text.splitlines() if "seconds" not in l]
    return [re.sub(r"_[0-9a-f]{20}", "_<uid>", l) for l in keep]


def test_main_and_predict_end_to_end(tmp_path, wisdm_csv):
    import main
    import predict

    with open(wisdm_csv) as f:
        lines = f.read().splitlines()
    data = tmp_path / "small.csv"
    data.write_text("\n".join(lines[:901]) + "\n")
    common = ["--data", str(data), "--device", "cpu", "--preset", "all-numeric", "--classifiers", "dt"]
    off = main.run(main.config_from_args(common + ["--out-dir", str(tmp_path / "off"), "--save-models", str(tmp_path / "m_off")]))
    off2 = main.run(main.config_from_args(common + ["--out-dir", str(tmp_path / "off2")]))
    on = main.run(main.config_from_args(common + ["--out-dir", str(tmp_path / "on"), "--save-models", str(tmp_path / "m_on"),
                                                  "--gmm", "6", "--gmm-max-iter", "15", "--gmm-cov", "diag",
                                                  "--gmm-init", "random"]))
    txt_off, txt_off2 = (tmp_path / "off" / "result.txt").read_text(), (tmp_path / "off2" / "result.txt").read_text()
    txt_on = (tmp_path / "on" / "result.txt").read_text()
    assert "GaussianMixture" not in txt_off and "gmm" not in off and not (tmp_path / "m_off" / "gmm").exists()
    assert _stable(txt_off) == _stable(txt_off2)            # the flag off: what the same command writes
    assert sorted(os.listdir(tmp_path / "m_off") + ["gmm"]) == sorted(os.listdir(tmp_path / "m_on"))
    cut = txt_on.index("GaussianMixture")
    assert _stable(txt_on[:cut])[:-2] == _stable(txt_off)[:len(_stable(txt_on[:cut])) - 2]
    for key in ("Weights", "Cluster Sizes", "Log-Likelihood", "Iterations", "Mean LL / row (test)", "Silhouette (test)",
                "Purity (train)", "Cluster x label"):
        assert key in txt_on[cut:], key
    rec = on["gmm"]
    assert rec["k"] == 6 and sum(rec["cluster_sizes"]) == on["n_train"] and 1 <= rec["num_iter"] <= 15
    assert abs(sum(rec["weights"]) - 1.0) < 1e-9 and 0.0 < rec["purity"] <= 1.0 and -1.0 <= rec["silhouette"] <= 1.0
    assert math.isfinite(rec["test_mean_log_likelihood"]) and len(rec["contingency"]) == 6
    from har.config import RunConfig

    c = RunConfig()
    assert (c.gmm, c.gmm_max_iter, c.gmm_cov, c.gmm_init) == (0, 100, "full", "k-means")
    out = tmp_path / "pred.csv"
    p = predict.main(["--models", str(tmp_path / "m_on"), "--model", "gmm", "--data", str(data), "--device", "cpu",
                      "--out", str(out)])
    assert p["rows"] == 900 and 1 <= p["clusters_used"] <= 6 and math.isfinite(p["mean_log_likelihood"])
    assert 0.0 <= p["majority_label_accuracy"] <= 1.0
    with open(out) as f:
        rows = list(csv.reader(f))
    assert rows[0][-5:] == ["cluster", "majority_label", "label_name", "probability", "log_likelihood"]
    assert len(rows) == 901 and all(0 <= int(r[-5]) < 6 and 0.0 < float(r[-2]) <= 1.0 and math.isfinite(float(r[-1]))
                                    for r in rows[1:])
