"""HMMSmoother posteriors on the CPU: the sequential forward-backward definition
(``har.ops.hmm.forward_backward_torch``) against enumeration of all paths, its invariants and edge cases,
Baum-Welch, the model layer, persistence and the two entry points.

The bound of every comparison between two implementations is ``eta(T, K) = 16 (K + 4) T 2^-53`` (T = the batch
length): K + 2 roundings per step and component, four quantities (alpha, beta, their product, its sum), two
implementations, a factor 2 for higher-order terms.  It is relative and has no absolute term."""
import csv
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

from har.data.table import Column, Table
from har.models import hmm as M
from har.models.hmm import HMMSmoother, HMMSmootherModel
from har.ops import hmm as H

F64 = torch.float64


def eta(T, K):
    return 16.0 * (K + 4) * max(T, 1) * 2.0 ** -53


def _one(T):
    return torch.tensor([0, T], dtype=torch.int64)


def _off(lens):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)


def random_model(rng, T, K, spread=8.0):
    """(E int32 [T, K], B, P, p0) through the module's own helpers."""
    E = H.quantize_logprob(torch.as_tensor(-spread * rng.random((T, K))))
    qA = H.quantize_logprob(torch.as_tensor(-spread * rng.random((K, K))))
    qpi = H.quantize_logprob(torch.as_tensor(-spread * rng.random(K)))
    return E, H.emission_likelihoods(E), H.transition_probs(qA), H.start_probs(qpi)


def enumerate_paths(B, P, p0):
    """gamma, xi, loglik of ONE sequence from all K^T paths (numpy fp64)."""
    B, P, p0 = B.numpy(), P.numpy(), p0.numpy()
    T, K = B.shape
    gamma, xi, Z = np.zeros((T, K)), np.zeros((K, K)), 0.0
    for p in itertools.product(range(K), repeat=T):
        w = p0[p[0]] * B[0, p[0]]
        for t in range(1, T):
            w *= P[p[t - 1], p[t]] * B[t, p[t]]
        Z += w
        for t in range(T):
            gamma[t, p[t]] += w
        for t in range(1, T):
            xi[p[t - 1], p[t]] += w
    return gamma / Z, xi / Z, math.log(Z)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_forward_backward_equals_enumeration(K, T):
    rng = np.random.default_rng(100 * K + T)
    for _ in range(4):
        _, B, P, p0 = random_model(rng, T, K)
        gamma, ll, xi = H.forward_backward_torch(B, P, p0, _one(T), want_xi=True)
        g, x, z = enumerate_paths(B, P, p0)
        assert gamma.dtype == F64 and ll.dtype == F64 and xi.dtype == F64
        np.testing.assert_allclose(gamma.numpy(), g, rtol=1e-12, atol=0)
        np.testing.assert_allclose(xi.numpy(), x, rtol=1e-12, atol=0)
        np.testing.assert_allclose(ll.numpy(), [z], rtol=1e-12, atol=0)
    # two sequences in one batch: each is its own enumeration, xi is their sum
    T2 = max(1, T // 2)
    _, B, P, p0 = random_model(rng, T + T2, K)
    gamma, ll, xi = H.forward_backward_torch(B, P, p0, _off([T, T2]), want_xi=True)
    g1, x1, z1 = enumerate_paths(B[:T], P, p0)
    g2, x2, z2 = enumerate_paths(B[T:], P, p0)
    np.testing.assert_allclose(gamma.numpy(), np.concatenate([g1, g2]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(xi.numpy(), x1 + x2, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(ll.numpy(), [z1, z2], rtol=1e-12, atol=0)
    assert H.forward_backward_torch(B, P, p0, _off([T, T2]))[2] is None


def test_invariants():
    rng = np.random.default_rng(3)
    K, lens = 5, [1, 9, 2, 1, 30, 5, 1]
    off = _off(lens)
    T, S = int(off[-1]), len(lens)
    _, B, P, p0 = random_model(rng, T, K)
    gamma, ll, xi = H.forward_backward_torch(B, P, p0, off, want_xi=True)
    tol = eta(T, K)
    assert torch.allclose(gamma.sum(1), torch.ones(T, dtype=F64), rtol=tol, atol=0)
    assert abs(float(xi.sum()) - (T - S)) <= tol * (T - S)
    is_start, is_end = torch.zeros(T, dtype=torch.bool), torch.zeros(T, dtype=torch.bool)
    is_start[off[:-1]] = True
    is_end[off[1:] - 1] = True
    assert torch.allclose(xi.sum(1), gamma[~is_end].sum(0), rtol=tol * T, atol=0)
    assert torch.allclose(xi.sum(0), gamma[~is_start].sum(0), rtol=tol * T, atol=0)
    assert (ll < 0).all()   # B <= 1 and probabilities: every sequence's likelihood is below 1
    # a batch equals per-sequence calls
    for s, (a, b) in enumerate(zip(off[:-1].tolist(), off[1:].tolist())):
        g1, l1, x1 = H.forward_backward_torch(B[a:b], P, p0, _one(b - a), want_xi=True)
        assert ((gamma[a:b] - g1).abs() <= tol * g1).all()
        assert abs(float(ll[s] - l1[0])) <= tol * (1 + abs(float(l1[0])))
        xi = xi - x1
    assert (xi.abs() <= tol * T).all()


def adversarial(T, K, seed=0):
    """Emission rows at the floor except one entry (which moves), transitions with forbidden entries."""
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << 25), 1 << 25
    E = torch.full((T, K), lo, dtype=torch.int32)
    E[torch.arange(T), torch.as_tensor(rng.integers(0, K, T))] = hi
    logA = torch.as_tensor(np.log(rng.random((K, K)) + 0.05))
    logA[torch.as_tensor(rng.random((K, K)) < 0.4)] = float("-inf")   # forbidden: floored at -32
    logpi = torch.full((K,), float("-inf"), dtype=F64)
    logpi[K - 1] = 0.0
    return E, H.emission_likelihoods(E), H.transition_probs(H.quantize_logprob(logA)), H.start_probs(H.quantize_logprob(logpi))


@pytest.mark.parametrize("K", [6, 32])
def test_adversarial_ranges_stay_finite_and_positive(K):
    T = 2049
    E, B, P, p0 = adversarial(T, K)
    assert float(B.max(1).values.min()) == 1.0 and float(B.min()) >= math.exp(-64) * (1 - 1e-12) > 2.0 ** -93
    assert float(P.min()) > 2.0 ** -52 and float(p0.min()) > 2.0 ** -52
    gamma, ll, xi = H.forward_backward_torch(B, P, p0, _off([1000, 1, 1048]), want_xi=True)
    for x in (gamma, ll, xi):
        assert torch.isfinite(x).all()
    assert (gamma > 0).all() and (xi > 0).all()
    assert torch.allclose(gamma.sum(1), torch.ones(T, dtype=F64), rtol=eta(T, K), atol=0)
    full = H.loglik_of_scores(ll, E, _off([1000, 1, 1048]))
    assert torch.isfinite(full).all() and (full > ll).all()   # every row's maximum is +32 here


def test_helpers_and_ranges():
    E = torch.tensor([[0, -(1 << 20), -(1 << 25)], [1 << 25, -(1 << 25), 5]], dtype=torch.int32)
    B = H.emission_likelihoods(E)
    assert B.dtype == F64 and B.max(1).values.tolist() == [1.0, 1.0]
    assert B[0, 1].item() == pytest.approx(math.exp(-1.0), rel=1e-15) and B[1, 1].item() == pytest.approx(math.exp(-64.0), rel=1e-14)
    q = torch.tensor([[0, -(1 << 25)], [-(1 << 20), -(1 << 20)]], dtype=torch.int32)
    P = H.transition_probs(q)
    assert torch.allclose(P.sum(1), torch.ones(2, dtype=F64)) and P[1].tolist() == [0.5, 0.5]
    assert P[0, 1].item() == pytest.approx(math.exp(-32.0) / (1 + math.exp(-32.0)), rel=1e-14)
    assert H.start_probs(q[1]).tolist() == [0.5, 0.5]
    ll = torch.tensor([-1.0], dtype=F64)
    assert H.loglik_of_scores(ll, E, _one(2)).item() == pytest.approx(-1.0 + 32.0, rel=1e-15)


def test_single_state_single_step_empty_and_limits():
    o = lambda *s: torch.ones(*s, dtype=F64)
    gamma, ll, xi = H.forward_backward(o(3, 1) * 0.5, o(1, 1), o(1), _one(3), want_xi=True)
    assert gamma.tolist() == [[1.0]] * 3 and xi.tolist() == [[2.0]] and ll.item() == pytest.approx(3 * math.log(0.5), rel=1e-15)
    B = torch.tensor([[0.25, 1.0, 0.5]], dtype=F64)
    p0 = torch.tensor([0.5, 0.25, 0.25], dtype=F64)
    gamma, ll, xi = H.forward_backward(B, o(3, 3) / 3, p0, _one(1), want_xi=True)
    assert torch.allclose(gamma, (B * p0) / (B * p0).sum(), rtol=1e-15, atol=0)
    assert ll.item() == pytest.approx(math.log(0.5), rel=1e-15) and float(xi.sum()) == 0.0
    gamma, ll, xi = H.forward_backward(o(0, 4), o(4, 4) / 4, o(4) / 4, torch.tensor([0], dtype=torch.int64), want_xi=True)
    assert gamma.shape == (0, 4) and ll.shape == (0,) and xi.shape == (4, 4) and float(xi.sum()) == 0.0
    assert H.emission_likelihoods(torch.zeros(0, 4, dtype=torch.int32)).shape == (0, 4)
    with pytest.raises(ValueError):
        H.forward_backward(o(5, 33), o(33, 33), o(33), _one(5))
    with pytest.raises(ValueError):
        H.forward_backward(o(5, 0), o(0, 0), o(0), _one(5))
    for bad in ([0, 3, 3, 5], [0, 4, 2, 5], [1, 5], [0, 4], [0, 6]):
        with pytest.raises(ValueError):
            H.forward_backward(o(5, 2), o(2, 2), o(2), torch.tensor(bad, dtype=torch.int64))
    with pytest.raises(ValueError):
        H.forward_backward(o(5, 2).float(), o(2, 2), o(2), _one(5))
    with pytest.raises(ValueError):
        H.forward_backward(o(5, 2), o(2, 3), o(2), _one(5))
    with pytest.raises(ValueError):
        H.forward_backward(o(5, 2), o(2, 2), o(3), _one(5))
    with pytest.raises(ValueError):
        H.forward_backward_native(o(5, 2), o(2, 2), o(2), _one(5))   # host tensors


# ------------------------------------------------------------------ the synthetic stream
@pytest.fixture(scope="module")
def stream():
    """The recipe of ``tests/test_hmm.py::stream``: 2,000 train windows, the next 2,000 as test, Gaussian
    NaiveBayes on the 43 window features; (train labels, test labels, test probabilities, predictions)."""
    from har.data.synth import StreamSpec, generate_stream
    from har.features.window import window_features_torch
    from har.models.naive_bayes import NaiveBayes

    spec, n = StreamSpec(), 2000
    xs, ys = generate_stream(2 * n, spec)
    F = window_features_torch(xs, spec.window, spec.window, spec.hz)[:, :43]
    F = torch.nan_to_num(F.float(), nan=0.0, posinf=0.0, neginf=0.0)
    nb = NaiveBayes(modelType="gaussian").fit_tensors(F[:n], ys[:n], spec.num_classes)
    _, prob, pred = nb.predict_all(F[n:])
    return ys[:n], ys[n:], prob, pred


def _acc(a, y):
    return float((a.long() == y).double().mean())


def test_stream_posterior_beats_per_window_labels(stream):
    ytr, yte, prob, pred = stream
    n = yte.numel()
    raw = _acc(pred, yte)
    for name, model in (("label counts", HMMSmoother().fit_labels(ytr, _one(ytr.numel()), 6)),
                        ("stay=0.9", HMMSmoother(stay=0.9).fit_stay(6))):
        gamma, ll = model.posterior(prob, _one(n))
        path, _ = model.decode(prob, _one(n))
        post = _acc(H._lowest_argmax(gamma, 1)[1], yte)
        print(f"{name}: per-window {raw:.4f}, Viterbi {_acc(path, yte):.4f}, posterior argmax {post:.4f}, "
              f"loglik {float(ll[0]):.1f}, smallest gamma {float(gamma.min()):.3g}")
        assert post > raw
        assert torch.allclose(gamma.sum(1), torch.ones(n, dtype=F64), rtol=eta(n, 6), atol=0)


@pytest.fixture(scope="module")
def em_model(stream):
    _, yte, prob, _ = stream
    tab = Table([Column("probability", "vector", prob.double().numpy())])
    return HMMSmoother(stay=0.5, numClasses=6, emIter=10, emTol=0.0, smoothing=1.0).fit(tab)


def test_baum_welch_raises_the_penalised_objective(stream, em_model):
    _, yte, prob, pred = stream
    n, K = yte.numel(), 6
    init = HMMSmoother(stay=0.5).fit_stay(K)
    # the same iterations step by step: the penalised objective is what EM cannot lower
    E = init.emission_scores(prob)
    B = H.emission_likelihoods(E)
    base = float(H.loglik_of_scores(torch.zeros(1, dtype=F64), E, _one(n))[0])
    P, p0, objs, raws = init.P, init.p0, [], []
    for _ in range(10):
        nP, np0, ll = M.baum_welch_step(B, P, p0, _one(n), 1.0)
        raws.append(float(ll) + base)
        objs.append(raws[-1] + float(M.penalty(P, p0, 1.0)))
        # the floor never binds on this input: the update is the plain normalised pseudo-count
        _, _, xi = H.forward_backward(B, P, p0, _one(n), want_xi=True)
        plain = (xi + 1.0) / (xi + 1.0).sum(1, keepdim=True)
        assert float(plain.min()) > M.EM_FLOOR and torch.equal(nP, M._floored(xi + 1.0, 1))
        assert torch.allclose(nP, plain, rtol=1e-15, atol=0) and float(np0.min()) > M.EM_FLOOR
        P, p0 = nP, np0
    print("penalised objective:", " ".join(f"{o:.2f}" for o in objs))
    print("raw log-likelihood: ", " ".join(f"{r:.2f}" for r in raws))
    for a, b in zip(objs, objs[1:]):
        assert b - a >= -eta(n, K) * abs(a)
    assert em_model.emIterations == 10 and len(em_model.objectiveHistory) == 10
    np.testing.assert_allclose(em_model.objectiveHistory, objs, rtol=1e-12)
    ll0, ll1 = float(init.posterior(prob, _one(n))[1][0]), float(em_model.posterior(prob, _one(n))[1][0])
    raw = _acc(pred, yte)
    a0 = _acc(H._lowest_argmax(init.posterior(prob, _one(n))[0], 1)[1], yte)
    a1 = _acc(H._lowest_argmax(em_model.posterior(prob, _one(n))[0], 1)[1], yte)
    print(f"log-likelihood {ll0:.1f} -> {ll1:.1f}; posterior accuracy {a0:.4f} -> {a1:.4f} (per-window {raw:.4f})")
    assert ll1 > ll0 and a1 > raw
    assert torch.allclose(em_model.P.sum(1), torch.ones(K, dtype=F64)) and em_model.P[0, 0] > 0.5


def test_em_tolerance_and_arguments(stream):
    _, _, prob, _ = stream
    tab = Table([Column("probability", "vector", prob[:300].double().numpy())])
    m = HMMSmoother(stay=0.5, numClasses=6, emIter=50, emTol=1e-3).fit(tab)
    assert 1 <= m.emIterations < 50 and len(m.objectiveHistory) == m.emIterations + 1
    h = m.objectiveHistory
    assert h[-1] - h[-2] < 1e-3 * abs(h[-2])
    plain = HMMSmoother(stay=0.5, numClasses=6).fit(tab)
    assert plain.emIterations == 0 and plain.objectiveHistory == [] and "emIterations" not in plain.state()
    with pytest.raises(ValueError):
        HMMSmoother(stay=0.5, numClasses=6, emIter=2).fit(Table([Column("label", "double", np.zeros(4))]))
    with pytest.raises(ValueError):
        HMMSmoother(emIter=-1)


def test_persist_round_trip_of_an_em_model(tmp_path, stream, em_model):
    from har.utils import persist

    _, _, prob, _ = stream
    persist.save(em_model, str(tmp_path / "hmm"), labels=list("abcdef"))
    back = persist.load(str(tmp_path / "hmm"), device="cpu")
    assert isinstance(back, HMMSmootherModel) and back.uid == em_model.uid
    assert back.emIterations == 10 and back.objectiveHistory == em_model.objectiveHistory
    assert torch.equal(back.qA, em_model.qA) and torch.equal(back.P, em_model.P) and torch.equal(back.p0, em_model.p0)
    off = torch.tensor([0, 700, 2000])
    a, b = em_model.posterior(prob, off), back.posterior(prob, off)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a model saved without the record (every model before Baum-Welch existed) loads with an empty one
    with open(tmp_path / "hmm" / "metadata.json") as f:
        md = json.load(f)
    del md["state"]["emIterations"], md["state"]["objectiveHistory"]
    with open(tmp_path / "hmm" / "metadata.json", "w") as f:
        json.dump(md, f)
    old = persist.load(str(tmp_path / "hmm"), device="cpu")
    assert old.emIterations == 0 and old.objectiveHistory == [] and torch.equal(old.qA, em_model.qA)


def test_transform_posterior_columns():
    tab = Table([Column("USER", "int", np.asarray([1, 1, 1, 2, 2, 1])),
                 Column("label", "double", np.asarray([0.0, 0.0, 1.0, 1.0, 0.0, 1.0]))])
    m = HMMSmoother(smoothing=1.0).fit(tab)
    prob = np.asarray([[0.9, 0.1], [0.4, 0.6], [0.9, 0.1], [0.2, 0.8], [0.3, 0.7], [0.6, 0.4]])
    tab = tab.with_column(Column("probability", "vector", prob))
    out = m.transform(tab, method="posterior")
    gamma, _ = m.posterior(torch.as_tensor(prob), torch.tensor([0, 3, 5, 6]))
    assert out.columns[-2:] == ["smoothedProbability", "smoothedPrediction"]
    assert np.array_equal(np.asarray(out["smoothedProbability"].data), gamma.numpy())
    assert out["smoothedPrediction"].data.tolist() == H._lowest_argmax(gamma, 1)[1].double().tolist()
    # the default is the Viterbi path, as before
    assert m.transform(tab)["smoothedPrediction"].data.tolist() == m.transform(tab, method="viterbi")["smoothedPrediction"].data.tolist()
    assert "smoothedProbability" not in m.transform(tab)
    with pytest.raises(ValueError):
        m.transform(tab, method="map")
    # an exact tie takes the lowest state
    tie = HMMSmoother(stay=0.5).fit_stay(2)
    t2 = Table([Column("probability", "vector", np.full((3, 2), 0.5))])
    assert tie.transform(t2, method="posterior")["smoothedPrediction"].data.tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ entry points
def _small_table(path, wisdm_csv, n=900):
    with open(wisdm_csv) as f:
        lines = f.read().splitlines()
    path.write_text("\n".join(lines[:n + 1]) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, wisdm_csv):
    """main.py on one small table: flags off, --hmm, --hmm-posterior, --hmm-posterior --hmm-em 3."""
    import main

    d = tmp_path_factory.mktemp("hmm_post_runs")
    data = _small_table(d / "small.csv", wisdm_csv)
    common = ["--data", data, "--device", "cpu", "--preset", "all-numeric", "--classifiers", "dt,nb"]
    out = {}
    for name, extra in (("off", []), ("hmm", ["--hmm"]), ("post", ["--hmm-posterior"]),
                        ("em", ["--hmm-posterior", "--hmm-em", "3"])):
        out[name] = main.run(main.config_from_args(common + ["--out-dir", str(d / name), "--save-models", str(d / ("m_" + name))] + extra))
    return d, data, out


def _stable(text, drop=()):
    import re

    keep = [l for l in text.splitlines() if "seconds" not in l and not any(l.startswith(p) for p in drop)]
    return [re.sub(r"_[0-9a-f]{20}", "_<uid>", l) for l in keep]


def test_main_posterior_flags(runs):
    d, _, out = runs
    txt = {k: (d / k / "result.txt").read_text() for k in out}
    # off: nothing of the smoother; --hmm alone: what it wrote before, no posterior line or field
    assert "HMM" not in txt["off"] and not (d / "m_off" / "hmm").exists()
    assert "HMM posterior" not in txt["hmm"] and txt["hmm"].count("HMM smoothed Accuracy = ") == 2
    for name in ("dt", "nb"):
        assert not any(k.startswith("posterior") for k in out["hmm"]["models"][name])
        assert not any(k in out["off"]["models"][name] for k in ("smoothed_accuracy", "posterior_accuracy"))
    # --hmm-posterior implies --hmm and only ADDS its line and fields
    assert txt["post"].count("HMM smoothed Accuracy = ") == 2 and txt["post"].count("HMM posterior Accuracy = ") == 2
    assert _stable(txt["post"], ("HMM posterior",)) == _stable(txt["hmm"])
    assert _stable(txt["hmm"], ("HMM smoothed",)) == _stable(txt["off"])
    for name in ("dt", "nb"):
        rec = out["post"]["models"][name]
        assert 0.0 <= rec["posterior_accuracy"] <= 1.0 and math.isfinite(rec["posterior_log_likelihood"])
        assert rec["smoothed_accuracy"] == out["hmm"]["models"][name]["smoothed_accuracy"]
    # the artefacts of a flags-off run are byte for byte those of any other run's shared files
    for f in sorted(os.listdir(d / "off")):
        if f.endswith(".csv") and "param" not in f:
            assert (d / "off" / f).read_bytes() == (d / "post" / f).read_bytes(), f
    # --hmm-em refines on the first classifier's training predictions and is saved with its record
    from har.utils import persist

    m = persist.load(str(d / "m_em" / "hmm"), device="cpu")
    assert 1 <= m.emIterations <= 3 and len(m.objectiveHistory) >= m.emIterations
    assert persist.load(str(d / "m_post" / "hmm"), device="cpu").emIterations == 0
    assert "HMM Baum-Welch" in txt["em"]
    from har.config import RunConfig

    assert RunConfig().hmm_posterior is False and RunConfig().hmm_em_iter == 0


def test_predict_smooth_hmm_posterior_end_to_end(runs, tmp_path):
    import predict

    d, data, _ = runs
    base = ["--models", str(d / "m_post"), "--model", "nb", "--data", data, "--device", "cpu"]
    predict.main(base + ["--out", str(tmp_path / "plain.csv")])
    rec = predict.main(base + ["--out", str(tmp_path / "post.csv"), "--smooth", "hmm-posterior",
                               "--segments-out", str(tmp_path / "segs.csv")])
    assert rec["rows"] == 900 and rec["smooth_s"] >= 0 and 0.0 <= rec["smoothed_accuracy"] <= 1.0
    assert math.isfinite(rec["smoothed_log_likelihood"]) and rec["segments"] >= 1
    with open(tmp_path / "plain.csv") as f, open(tmp_path / "post.csv") as g:
        plain, post = list(csv.reader(f)), list(csv.reader(g))
    assert post[0] == plain[0] + ["smoothed_prediction", "smoothed_label_name", "smoothed_confidence"]
    assert [r[:len(plain[0])] for r in post] == plain
    conf = np.asarray([float(r[-1]) for r in post[1:]])
    assert ((conf >= 0.5 / 6) & (conf <= 1.0 + 1e-12)).all()
    with open(tmp_path / "segs.csv") as f:
        segs = list(csv.reader(f))
    assert len(segs) - 1 == rec["segments"]
    nxt = 0
    for q, a, b, k, name in segs[1:]:
        a, b = int(a), int(b)
        assert a == nxt and all(r[-3] == k and r[-2] == name for r in post[1 + a:2 + b])
        nxt = b + 1
    assert nxt == 900
    # --smooth hmm is what it was: two added columns
    predict.main(base + ["--out", str(tmp_path / "vit.csv"), "--smooth", "hmm"])
    with open(tmp_path / "vit.csv") as f:
        assert next(csv.reader(f)) == plain[0] + ["smoothed_prediction", "smoothed_label_name"]
    with pytest.raises(ValueError):
        predict.main(base + ["--smooth", "kalman"])
