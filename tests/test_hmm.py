"""HMMSmoother on the CPU: the sequential Viterbi definition (``har.ops.hmm.viterbi_torch``) against
brute-force enumeration, its edge cases, the estimator / model, persistence and the two entry points."""
import csv
import itertools
import json
import os

import numpy as np
import pytest
import torch

from har.data.table import Column, Table
from har.models.hmm import HMMSmoother, HMMSmootherModel, sequence_offsets
from har.ops import hmm as H

I32 = torch.int32


def _t(a, dtype=I32):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def _one(T):
    return torch.tensor([0, T], dtype=torch.int64)


def brute_force(E, A, pi):
    """Best score over all K^T paths and, among the best, the path that is smallest when compared from
    the last position backwards."""
    T, K = E.shape
    best, arg = None, None
    for p in itertools.product(range(K), repeat=T):
        s = int(pi[p[0]]) + int(E[0, p[0]])
        for t in range(1, T):
            s += int(A[p[t - 1], p[t]]) + int(E[t, p[t]])
        key = tuple(reversed(p))
        if best is None or s > best or (s == best and key < arg):
            best, arg = s, key
    return np.asarray(list(reversed(arg))), best


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_viterbi_equals_brute_force(K, T):
    rng = np.random.default_rng(100 * K + T)
    for trial in range(12):
        if trial % 2 == 0:   # coarse integer scores: many exact ties
            draw = lambda shape: rng.integers(-2, 1, size=shape)
        else:                # quantised log-probabilities
            draw = lambda shape: H.quantize_logprob(torch.log(torch.as_tensor(rng.random(shape)))).numpy()
        E, A, pi = draw((T, K)), draw((K, K)), draw((K,))
        path, score = H.viterbi_torch(_t(E), _t(A), _t(pi), _one(T))
        want, best = brute_force(E, A, pi)
        assert path.dtype == torch.int32 and score.dtype == torch.int64
        assert path.tolist() == want.tolist(), (E, A, pi)
        assert int(score[0]) == best


def test_single_state_and_single_step():
    E = _t([[-5], [-7], [-1]])
    path, score = H.viterbi_torch(E, _t([[-2]]), _t([-3]), _one(3))
    assert path.tolist() == [0, 0, 0] and int(score[0]) == -3 - 5 - 2 - 7 - 2 - 1
    path, score = H.viterbi_torch(_t([[-4, -1, -1]]), _t(np.zeros((3, 3))), _t([0, -1, -1]), _one(1))
    assert path.tolist() == [1] and int(score[0]) == -2   # states 1 and 2 tie at -2 (state 0: -4): the lowest wins


def test_all_equal_scores_give_the_zero_path():
    T, K = 37, 5
    z = lambda *s: torch.zeros(*s, dtype=I32)
    path, score = H.viterbi_torch(z(T, K), z(K, K), z(K), torch.tensor([0, 10, 11, T]))
    assert path.tolist() == [0] * T and score.tolist() == [0, 0, 0]


def test_empty_input_and_limits():
    z = lambda *s: torch.zeros(*s, dtype=I32)
    path, score = H.viterbi(z(0, 4), z(4, 4), z(4), torch.tensor([0], dtype=torch.int64))
    assert path.shape == (0,) and score.shape == (0,) and H.segments(path, torch.tensor([0])) == []
    with pytest.raises(ValueError):
        H.viterbi(z(5, 33), z(33, 33), z(33), _one(5))
    with pytest.raises(ValueError):
        H.viterbi(z(5, 0), z(0, 0), z(0), _one(5))
    for bad in ([0, 3, 3, 5], [0, 4, 2, 5], [1, 5], [0, 4], [0, 6]):
        with pytest.raises(ValueError):
            H.viterbi(z(5, 2), z(2, 2), z(2), torch.tensor(bad, dtype=torch.int64))
    with pytest.raises(ValueError):
        H.viterbi(z(5, 2).long(), z(2, 2), z(2), _one(5))
    with pytest.raises(ValueError):
        H.viterbi(z(5, 2), z(2, 3), z(2), _one(5))


def test_quantize_logprob():
    x = torch.tensor([0.0, -1.0, -32.0, -40.0, float("-inf"), 2.5e-7, 40.0], dtype=torch.float64)
    q = H.quantize_logprob(x)
    assert q.dtype == torch.int32
    assert q.tolist() == [0, -(1 << 20), -(1 << 25), -(1 << 25), -(1 << 25), 0, 1 << 25]
    p = torch.tensor([[0.5, 0.25, 0.25, 0.0]], dtype=torch.float64)
    prior = torch.tensor([0.5, 0.125, 0.25, 0.125], dtype=torch.float64)
    assert H.emission_scores(p, None, "posterior").tolist() == [[-726817, -1453635, -1453635, -(1 << 25)]]
    assert H.emission_scores(p, prior, "scaled").tolist() == [[0, 726817, 0, -(1 << 25)]]
    with pytest.raises(ValueError):
        H.emission_scores(p, None, "scaled")
    with pytest.raises(ValueError):
        H.emission_scores(p, prior, "likelihood")


def test_batch_equals_per_sequence_calls():
    rng = np.random.default_rng(7)
    K = 4
    lens = [1, 9, 2, 1, 30, 5, 1]
    off = np.concatenate([[0], np.cumsum(lens)])
    T = int(off[-1])
    E, A, pi = _t(rng.integers(-3, 1, (T, K))), _t(rng.integers(-3, 1, (K, K))), _t(rng.integers(-3, 1, K))
    path, score = H.viterbi_torch(E, A, pi, _t(off, torch.int64))
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        p1, s1 = H.viterbi_torch(E[a:b], A, pi, _one(b - a))
        assert torch.equal(path[a:b], p1) and int(score[s]) == int(s1[0])
    segs = H.segments(path, _t(off, torch.int64))
    assert [s[0] for s in segs] == sorted(s[0] for s in segs) and segs[0][1] == 0 and segs[-1][2] == T - 1
    assert all(path[a:b + 1].unique().tolist() == [k] for _, a, b, k in segs)
    assert all(off[q] <= a and b < off[q + 1] for q, a, b, _ in segs)
    # maximal runs: a neighbouring segment is another sequence or another state
    assert all(x[0] != y[0] or x[3] != y[3] for x, y in zip(segs, segs[1:]))


# ------------------------------------------------------------------ the synthetic stream
@pytest.fixture(scope="module")
def stream():
    """``StreamSpec()``: 2,000 train windows, the next 2,000 as test, the project's Gaussian NaiveBayes on
    the 43 window features; returns (train labels, test labels, test probabilities)."""
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


def test_stream_smoothing_beats_per_window_labels(stream):
    ytr, yte, prob, pred = stream
    n = yte.numel()
    model = HMMSmoother().fit_labels(ytr, _one(ytr.numel()), 6)
    assert torch.allclose(model.logA.exp().sum(1), torch.ones(6, dtype=torch.float64))
    path, score = model.decode(prob, _one(n))
    raw_acc = float((pred == yte).double().mean())
    acc = float((path.long() == yte).double().mean())
    raw_segs = H.count_segments(pred.to(torch.int32), _one(n))
    segs = H.count_segments(path, _one(n))
    print(f"per-window accuracy {raw_acc:.4f} ({raw_segs} segments) -> Viterbi {acc:.4f} ({segs} segments)")
    assert acc > raw_acc
    assert segs < raw_segs
    # the score is the decoded path's own score
    E, p = model.emission_scores(prob).long(), path.long()
    own = model.qpi[p[0]].long() + E[torch.arange(n), p].sum() + model.qA[p[:-1], p[1:]].long().sum()
    assert score.tolist() == [int(own)]


def test_stay_model_needs_no_labels(stream):
    _, yte, prob, pred = stream
    n = yte.numel()
    model = HMMSmoother(stay=0.9, numClasses=6).fit(Table([Column("probability", "vector", prob.double().numpy())]))
    A = model.logA.exp()
    assert torch.allclose(A.diagonal(), torch.full((6,), 0.9, dtype=torch.float64))
    assert torch.allclose(A[0, 1:], torch.full((5,), 0.02, dtype=torch.float64))
    assert torch.allclose(model.prior, torch.full((6,), 1 / 6, dtype=torch.float64))
    path, _ = model.decode(prob, _one(n))
    print(f"stay=0.9: per-window {float((pred == yte).double().mean()):.4f} -> {float((path.long() == yte).double().mean()):.4f}")
    assert float((path.long() == yte).double().mean()) > float((pred == yte).double().mean())
    assert H.count_segments(path, _one(n)) < H.count_segments(pred.to(torch.int32), _one(n))
    one = HMMSmoother(stay=0.9).fit_stay(1)
    assert one.logA.exp().tolist() == [[1.0]]
    assert one.decode(torch.ones(3, 1), _one(3))[0].tolist() == [0, 0, 0]


def test_fit_counts_transitions_inside_sequences_only():
    # users 1, 1, 1 | 2, 2 | 1: three sequences; labels 0 0 1 | 1 0 | 1
    tab = Table([Column("USER", "int", np.asarray([1, 1, 1, 2, 2, 1])),
                 Column("label", "double", np.asarray([0.0, 0.0, 1.0, 1.0, 0.0, 1.0]))])
    assert sequence_offsets(tab, "USER").tolist() == [0, 3, 5, 6]
    assert sequence_offsets(tab, "absent").tolist() == [0, 6]
    m = HMMSmoother(smoothing=1.0).fit(tab)
    counts = torch.tensor([[1.0, 1.0], [1.0, 0.0]]) + 1.0          # 0->0, 0->1, 1->0; nothing across users
    assert torch.allclose(m.logA.exp(), (counts / counts.sum(1, keepdim=True)).double())
    assert torch.allclose(m.logpi.exp(), torch.tensor([2 / 5, 3 / 5], dtype=torch.float64))   # starts 0, 1, 1
    assert torch.allclose(m.prior, torch.tensor([4 / 8, 4 / 8], dtype=torch.float64))
    prob = np.asarray([[0.9, 0.1], [0.4, 0.6], [0.9, 0.1], [0.2, 0.8], [0.3, 0.7], [0.6, 0.4]])
    out = m.transform(tab.with_column(Column("probability", "vector", prob)))
    assert out["smoothedPrediction"].data.tolist() == m.decode(torch.as_tensor(prob), torch.tensor([0, 3, 5, 6]))[0].tolist()
    assert out.columns[-1] == "smoothedPrediction" and len(out["smoothedPrediction"].data) == 6


def test_persist_round_trip(tmp_path, stream):
    from har.utils import persist

    ytr, yte, prob, _ = stream
    model = HMMSmoother(sequenceCol="recording", emission="posterior").fit_labels(ytr, _one(ytr.numel()), 6)
    persist.save(model, str(tmp_path / "hmm"), labels=list("abcdef"))
    back = persist.load(str(tmp_path / "hmm"), device="cpu")
    assert isinstance(back, HMMSmootherModel) and back.uid == model.uid
    assert back.sequenceCol == "recording" and back.emission == "posterior" and back.num_classes == 6
    assert torch.equal(back.qA, model.qA) and torch.equal(back.qpi, model.qpi) and torch.equal(back.prior, model.prior)
    off = torch.tensor([0, 700, 2000])
    a, b = model.decode(prob, off), back.decode(prob, off)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ entry points
def _small_table(path, wisdm_csv, n=900):
    with open(wisdm_csv) as f:
        lines = f.read().splitlines()
    path.write_text("\n".join(lines[:n + 1]) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, wisdm_csv):
    """main.py twice on the same small table: --hmm off, then --hmm on (with --save-models)."""
    import main

    d = tmp_path_factory.mktemp("hmm_runs")
    data = _small_table(d / "small.csv", wisdm_csv)
    common = ["--data", data, "--device", "cpu", "--preset", "all-numeric", "--classifiers", "dt,nb"]
    off = main.run(main.config_from_args(common + ["--out-dir", str(d / "off"), "--save-models", str(d / "m_off")]))
    on = main.run(main.config_from_args(common + ["--out-dir", str(d / "on"), "--save-models", str(d / "m_on"), "--hmm"]))
    return d, data, off, on


def _stable(text):
    """result.txt without the lines that differ between any two runs (timings, random uids)."""
    import re

    keep = [l for l in text.splitlines() if "seconds" not in l and not l.startswith("HMM smoothed")]
    return [re.sub(r"_[0-9a-f]{20}", "_<uid>", l) for l in keep]


def test_main_hmm_off_leaves_the_artefacts_unchanged(runs):
    d, _, off, on = runs
    txt_off, txt_on = (d / "off" / "result.txt").read_text(), (d / "on" / "result.txt").read_text()
    assert "HMM" not in txt_off and not (d / "m_off" / "hmm").exists()
    assert sorted(os.listdir(d / "off")) == sorted(os.listdir(d / "on"))
    assert sorted(os.listdir(d / "m_off") + ["hmm"]) == sorted(os.listdir(d / "m_on"))
    # the smoother only ADDS its line: everything else of the run is what --hmm off writes
    assert _stable(txt_off) == _stable(txt_on)
    assert txt_on.count("HMM smoothed Accuracy = ") == 2
    for name in ("dt", "nb"):
        assert "smoothed_accuracy" not in off["models"][name] and "segments" not in off["models"][name]
        rec = on["models"][name]
        assert 0.0 <= rec["smoothed_accuracy"] <= 1.0 and 1 <= rec["segments"] <= on["n_test"]
        assert {k: v for k, v in rec.items() if k in ("accuracy", "f1", "count_total", "correct")} == \
               {k: v for k, v in off["models"][name].items() if k in ("accuracy", "f1", "count_total", "correct")}
    with open(d / "off" / "additional_param.csv") as f, open(d / "on" / "additional_param.csv") as g:
        a, b = list(csv.reader(f)), list(csv.reader(g))
    drop = [a[0].index("Training Time"), a[0].index("Testing Time"), a[0].index("Classifier")]
    strip = lambda rows: [[c for j, c in enumerate(r) if j not in drop] for r in rows]
    assert strip(a) == strip(b)
    from har.config import RunConfig

    assert RunConfig().hmm is False and RunConfig().hmm_sequence_col == "USER" and RunConfig().hmm_emission == "scaled"


def test_predict_smooth_hmm_end_to_end(runs, tmp_path):
    import predict

    d, data, _, _ = runs
    base = ["--models", str(d / "m_on"), "--model", "nb", "--data", data, "--device", "cpu"]
    rec0 = predict.main(base + ["--out", str(tmp_path / "plain.csv")])
    # without --smooth the saved hmm model changes nothing: same bytes as from the models saved without it
    predict.main(["--models", str(d / "m_off")] + base[2:] + ["--out", str(tmp_path / "plain_off.csv")])
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "plain_off.csv").read_bytes()
    assert "smooth_s" not in rec0 and "segments" not in rec0
    rec = predict.main(base + ["--out", str(tmp_path / "smooth.csv"), "--smooth", "hmm",
                               "--segments-out", str(tmp_path / "segs.csv")])
    assert rec["rows"] == 900 and rec["smooth_s"] >= 0 and 0.0 <= rec["smoothed_accuracy"] <= 1.0
    with open(tmp_path / "plain.csv") as f, open(tmp_path / "smooth.csv") as g:
        plain, smooth = list(csv.reader(f)), list(csv.reader(g))
    assert smooth[0] == plain[0] + ["smoothed_prediction", "smoothed_label_name"]
    assert [r[:len(plain[0])] for r in smooth] == plain          # the existing columns are untouched
    with open(tmp_path / "segs.csv") as f:
        segs = list(csv.reader(f))
    assert segs[0] == ["sequence", "first_row", "last_row", "state", "label_name"] and len(segs) - 1 == rec["segments"]
    # the segments tile the rows and spell the smoothed column; a sequence is a run of one USER
    hdr = open(data).readline().strip().split(",")
    users = [l.split(",")[hdr.index("USER")] for l in open(data).read().splitlines()[1:]]
    nxt = 0
    for q, a, b, k, name in segs[1:]:
        a, b = int(a), int(b)
        assert a == nxt and b >= a
        nxt = b + 1
        assert all(r[-2] == k and r[-1] == name for r in smooth[1 + a:2 + b])
        assert len(set(users[a:b + 1])) == 1
    assert nxt == 900
    assert int(segs[-1][0]) + 1 == sum(1 for x, y in zip(users, users[1:]) if x != y) + 1
    with open(d / "m_on" / "hmm" / "metadata.json") as f:
        md = json.load(f)
    assert md["class"] == "HMMSmootherModel" and md["params"]["sequenceCol"] == "USER" and md["numClasses"] == len(md["labels"])
    # one sequence for the whole table when the column is overridden to an absent one
    rec1 = predict.main(base + ["--smooth", "hmm", "--sequence-col", "nothing"])
    assert rec1["segments"] >= 1 and "smooth_s" in rec1
    with pytest.raises(FileNotFoundError):
        predict.main(["--models", str(d / "m_off")] + base[2:] + ["--smooth", "hmm"])
