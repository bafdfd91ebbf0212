"""RocketFeaturizer on the CPU: the definition (``ops.rocket``) against a naive loop, the fit, persistence,
the raw-stream plumbing and command lines, and the accuracy against the 43 window features."""
import csv
import functools
import itertools

import numpy as np
import pytest
import torch

from _rocket_util import REAL_CASES, ambiguity, hand_params, int_stream, real_case
from har.data.synth import StreamSpec, generate_stream
from har.features.rocket import RocketFeaturizer, RocketModel
from har.ops.rocket import (N_KERNELS, RocketParams, rocket_conv_torch, rocket_counts_torch, rocket_dilations,
                            rocket_features_torch, rocket_kernels, rocket_names)
from har.utils import persist


# ------------------------------------------------------------------ structure
def test_kernels_and_dilations():
    w = rocket_kernels()
    assert w.shape == (84, 9) and w.dtype == torch.float64
    assert bool((w.sum(1) == 0).all())
    for k, sub in enumerate(itertools.combinations(range(9), 3)):
        assert [j for j in range(9) if w[k, j] == 2] == list(sub)
        assert int((w[k] == -1).sum()) == 6
    assert rocket_dilations(200) == [1, 2, 4, 8, 16]
    assert rocket_dilations(9) == [1] and rocket_dilations(16) == [1] and rocket_dilations(17) == [1, 2]
    with pytest.raises(ValueError):
        rocket_dilations(8)
    assert rocket_names(3) == ["RKT00000", "RKT00001", "RKT00002"]


@pytest.mark.parametrize("W", (9, 17))
def test_oracle_equals_a_naive_loop(W):
    A, q = 3, 2
    s = int_stream(2, W, W, A, lo=-5, hi=5)
    g = torch.Generator().manual_seed(W)
    n_dil = len(rocket_dilations(W))
    masks = torch.randint(1, 8, (n_dil, N_KERNELS), generator=g, dtype=torch.int32)
    b = torch.randint(-4, 4, (n_dil, N_KERNELS, q), generator=g).float() + 0.5
    p = RocketParams(W, A, masks, b)
    counts = rocket_counts_torch(s, p, W, W)
    feats = rocket_features_torch(s, p, W, W)
    combs = list(itertools.combinations(range(9), 3))
    for n in range(2):
        for e, d in enumerate(p.dilations):
            for k in range(N_KERNELS):
                w = [2 if j in combs[k] else -1 for j in range(9)]
                lo, hi = (4 * d, W - 4 * d) if (e + k) % 2 else (0, W)
                axes = [c for c in range(A) if (int(masks[e, k]) >> c) & 1]
                C = [sum(w[j] * float(s[n * W + t + (j - 4) * d, c]) for c in axes for j in range(9)
                         if 0 <= t + (j - 4) * d < W) for t in range(W)]
                for i in range(q):
                    cnt = sum(C[t] > float(b[e, k, i]) for t in range(lo, hi))
                    col = (e * N_KERNELS + k) * q + i
                    assert cnt == int(counts[n, col])
                    assert float(feats[n, col]) == float(np.float32(cnt) / np.float32(hi - lo))


def test_integer_streams_give_integer_counts_in_range():
    W, A = 65, 3
    s = int_stream(5, W, 32, A)
    p = hand_params(W, A)
    c = rocket_counts_torch(s, p, W, 32)
    L = p.range_lengths()
    d = torch.tensor(p.dilations).view(-1, 1)
    odd = (torch.arange(len(p.dilations)).view(-1, 1) + torch.arange(N_KERNELS).view(1, -1)) % 2 == 1
    assert torch.equal(L[odd], (W - 8 * d).expand(-1, N_KERNELS)[odd]) and bool((L[~odd] == W).all()) and int(L.min()) >= 1
    assert c.dtype == torch.int32 and c.shape == (5, p.n_features)
    assert bool((c >= 0).all()) and bool((c <= L.repeat_interleave(p.q, 1).reshape(1, -1)).all())
    # a bias below every value counts the whole range, one above none
    lo = RocketParams(W, A, p.masks, torch.full_like(p.biases, -1e6))
    hi = RocketParams(W, A, p.masks, torch.full_like(p.biases, 1e6))
    assert torch.equal(rocket_counts_torch(s, lo, W, 32), L.repeat_interleave(p.q, 1).reshape(1, -1).expand(5, -1).int())
    assert int(rocket_counts_torch(s, hi, W, 32).sum()) == 0
    assert bool((rocket_features_torch(s, lo, W, 32) == 1).all())
    # the valid-only range leaves the padded positions out: C of the chosen pairs, counted by hand
    C = rocket_conv_torch(s, p, W, 32, torch.tensor([2, 2]), torch.tensor([1, N_KERNELS + 1]))   # (e, k) = (0, 1), (1, 1)
    assert int((C[0, 4: W - 4] > float(p.biases[0, 1, 0])).sum()) == int(c[2, 1 * p.q])
    assert int((C[1] > float(p.biases[1, 1, 0])).sum()) == int(c[2, (N_KERNELS + 1) * p.q])


# ------------------------------------------------------------------ fit
@functools.lru_cache(maxsize=None)
def _fixture(n=4000):
    return generate_stream(n, StreamSpec())


def test_fit_is_reproducible_from_the_seed():
    s, _ = _fixture()
    s = s[: 300 * 200]
    a = RocketFeaturizer(seed=7).fit(s).rocket_params
    b = RocketFeaturizer(seed=7).fit(s).rocket_params
    c = RocketFeaturizer(seed=8).fit(s).rocket_params
    assert torch.equal(a.masks, b.masks) and torch.equal(a.biases, b.biases)
    assert not torch.equal(a.masks, c.masks) and not torch.equal(a.biases, c.biases)
    assert a.q == 4 and a.n_features == 1680 and a.biases.shape == (5, 84, 4) and a.biases.dtype == torch.float32
    assert int(a.masks.min()) >= 1 and int(a.masks.max()) <= 7 and bool(torch.isfinite(a.biases).all())
    assert set(a.masks.flatten().tolist()) == set(range(1, 8))             # every subset of three axes occurs
    assert bool((a.biases[..., 1:] >= a.biases[..., :-1]).all())            # quantiles ascend
    small = RocketFeaturizer(num_features=100).fit(s)                       # fewer than one bias each: q = 1
    assert small.num_features == 420 and small.names[-1] == "RKT00419"


def test_rows_do_not_depend_on_neighbouring_windows():
    s, _ = _fixture()
    s = s[: 40 * 200]
    m = RocketFeaturizer(overlap=0.5).fit(s)
    assert m.stride == 100 and m.halo() == 100
    X = m.transform(s)
    assert X.shape == (79, 1680) and X.dtype == torch.float32 and float(X.min()) >= 0 and float(X.max()) <= 1
    assert torch.equal(m.transform(s[700: 1600]), X[7: 15])
    out = torch.full((79, 1685), -7.0)
    m.transform_into(s, out, 5)
    assert torch.equal(out[:, 5:], X) and bool((out[:, :5] == -7).all())


def test_persist_round_trip(tmp_path):
    s, _ = _fixture()
    s = s[: 20 * 200]
    m = RocketFeaturizer(overlap=0.25, seed=3).fit(s)
    persist.save(m, str(tmp_path / "rocket"))
    r = persist.load(str(tmp_path / "rocket"))
    assert isinstance(r, RocketModel) and (r.hz, r.window, r.stride, r.seed) == (m.hz, m.window, m.stride, m.seed)
    assert torch.equal(r.rocket_params.masks, m.rocket_params.masks) and torch.equal(r.rocket_params.biases, m.rocket_params.biases)
    assert r.names == m.names and torch.equal(r.transform(s), m.transform(s))


# ------------------------------------------------------------------ raw-stream plumbing and command lines
def test_raw_table_columns_and_cli_end_to_end(tmp_path):
    import main
    import predict
    from har.data.split import split_ids
    from har.features.raw import WISDM43, raw_to_table, write_synthetic_raw

    p = str(tmp_path / "raw.csv")
    info = write_synthetic_raw(p, n_windows=160, users=5)
    plain = raw_to_table(p)
    t = raw_to_table(p, rocket=840)
    assert plain.columns == ["UID", "USER"] + WISDM43 + ["ACTIVITY"]          # switch off: the table as it was
    assert t.columns == plain.columns + rocket_names(840) and t.count() == 160
    assert t["RKT00000"].kind == "double" and t.rocket_model.num_features == 840
    for c in plain.columns:
        assert np.array_equal(np.asarray(t[c].data), np.asarray(plain[c].data))
    again = raw_to_table(p, rocket=t.rocket_model)                           # a fitted model is applied as is
    assert np.array_equal(again["RKT00839"].data, t["RKT00839"].data)

    with pytest.raises(SystemExit):
        main.config_from_args(["--rocket", "840"])                           # needs --raw
    out, mdir = tmp_path / "out", tmp_path / "models"
    s = main.run(main.config_from_args(["--raw", p, "--preset", "rocket", "--out-dir", str(out), "--device", "cpu",
                                        "--save-models", str(mdir)]))
    assert s["encoding"] == "rocket" and s["n_train"] + s["n_test"] == 160 and set(s["models"]) == {"lr"}
    assert s["models"]["lr"]["accuracy"] > 0.5
    assert (mdir / "rocket" / "metadata.json").exists()
    rec = predict.main(["--models", str(mdir), "--model", "lr", "--raw", p, "--device", "cpu", "--out",
                        str(tmp_path / "p.csv")])
    assert rec["rows"] == 160
    with open(tmp_path / "p.csv") as f:
        rows = list(csv.reader(f))[1:]
    pred = np.array([r[3] for r in rows])
    from har.features.raw import ACTIVITIES

    truth = np.array([ACTIVITIES[int(v)] for v in info["labels"]])
    test = split_ids(160, [0.7, 0.3], 2018) == 1
    assert int(test.sum()) == s["n_test"]
    assert float((pred[test] == truth[test]).mean()) == pytest.approx(s["models"]["lr"]["accuracy"], abs=1e-12)
    import shutil

    shutil.rmtree(mdir / "rocket")
    with pytest.raises(FileNotFoundError, match="rocket"):
        predict.main(["--models", str(mdir), "--model", "lr", "--raw", p, "--device", "cpu"])


# ------------------------------------------------------------------ accuracy against the 43 window features
def test_rocket_columns_beat_the_window_features():
    """StreamSpec() fixture, 2,000 training and the next 2,000 test windows, the project's LogisticRegression
    with identical parameters (its own standardisation included; the Wolfe line search, because the batched
    Armijo trials reject every step on the uncentred rocket columns) on both column sets.
    Measured: rocket 0.9275, window features 0.8795 (PARITY.md)."""
    from har.data.table import Column, Table
    from har.features.window import window_features_torch
    from har.models.logreg import LogisticRegression

    s, y = _fixture()
    W = 200
    y = torch.as_tensor(y).long()
    model = RocketFeaturizer().fit(s[: 2000 * W])                        # features of the training half only
    Xr = model.transform(s).double()
    Xw = torch.nan_to_num(window_features_torch(s, W, W, 20.0)[:, :43].double(), nan=-1.0)
    acc = {}
    for name, X in (("rocket", Xr), ("window43", Xw)):
        train = Table([Column("features", "vector", X[:2000].numpy()),
                       Column("label", "double", y[:2000].numpy().astype(np.float64))])
        m = LogisticRegression(maxIter=100, regParam=0.01, elasticNetParam=0.0, lineSearch="wolfe", device="cpu").fit(train)
        pred = m.predict_all(X[2000:].float())[2].long().cpu()
        acc[name] = float((pred == y[2000:]).double().mean())
    print(f"held-out accuracy, LogisticRegression(maxIter=100, regParam=0.01, lineSearch=wolfe): rocket {acc['rocket']:.4f}, "
          f"43 window features {acc['window43']:.4f}")
    assert acc["rocket"] > acc["window43"]


# ------------------------------------------------------------------ the near-tie condition of the GPU test's inputs
@pytest.mark.parametrize("n_windows,W,A", REAL_CASES)
def test_near_ties_are_rare_on_the_real_valued_inputs(n_windows, W, A):
    """On the exact inputs of tests/test_gpu_rocket.py::test_real_valued_within_ambiguity: the share of counted
    positions whose float64 C lies within gamma S of the bias is at most 1e-3 (on the oracle alone)."""
    s, p = real_case(n_windows, W, A)
    _, amb, counted = ambiguity(s, p, W, W)
    share = int(amb.sum()) / int(counted.sum())
    print(f"near ties ({n_windows}, {W}, {A}): {int(amb.sum())} of {int(counted.sum())} counted positions ({share:.3g})")
    assert share <= 1e-3
