"""KMeans / ClusteringEvaluator on the CPU: the PyTorch definitions of har/ops/kmeans.py (the oracle of the
kernels), the model, the initialisations, data parallelism on gloo, persistence and the commands."""
import csv
import json
import os
import re
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from _kmeans_util import ASSIGN_SHAPES, assign_case, blobs, gen, mixture, tie_rule
from har.evaluation.evaluators import ClusteringEvaluator
from har.models.kmeans import KMeans, KMeansModel
from har.ops import kmeans as KM


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ------------------------------------------------------------------ random init
def test_random_init_distinct_and_shard_independent():
    N, k = 1000, 16
    rows = KM.random_init_rows(7, k, N)
    assert len(set(rows.tolist())) == k and rows.min() >= 0 and rows.max() < N
    assert not np.array_equal(rows, KM.random_init_rows(8, k, N))
    keys = KM.random_init_keys(7, N)
    for cuts in ([0, 1000], [0, 333, 1000], [0, 1, 500, 999, 1000]):
        cand = np.concatenate([KM.random_init_rows(7, k, b - a, row_offset=a) for a, b in zip(cuts, cuts[1:])])
        merged = cand[np.argsort(keys[cand])][:k]
        assert np.array_equal(merged, rows)
    X, _, _ = blobs(300, 5, 3)
    m = KMeans(k=4, maxIter=0, initMode="random", seed=7).fit_tensors(X)
    assert torch.allclose(m.clusterCenters(), X[torch.from_numpy(KM.random_init_rows(7, 4, 300))], atol=1e-5)


# ------------------------------------------------------------------ fixed point
def test_fixed_point_round_trip():
    Xc, _ = mixture(700, 9, 3)
    Xc[:, 4] = 0.0                                              # an all-zero column: e = 0
    Xc[:, 5] *= 1e-6
    Xc[:, 6] *= 1e5
    K = 5
    a = torch.randint(0, K - 1, (700,), generator=gen(1)).to(torch.int32)   # cluster K - 1 stays empty
    scale = KM.feature_scales(Xc)
    amax = Xc.abs().amax(dim=0).double()
    assert float(scale[4]) == 1.0
    ok = amax > 0
    assert bool((amax[ok] * scale.double()[ok] < 2.0 ** 30).all()) and bool((amax[ok] * scale.double()[ok] * 2 >= 2.0 ** 30).all())
    nscale = KM.norm_scale(KM.row_norms(Xc))
    acc = KM.accumulate_torch(Xc, a, None, scale, nscale, K)
    q = torch.round(Xc.double() * scale.double())
    assert torch.equal((Xc * scale).double(), Xc.double() * scale.double())   # the scaling is exact: rint is the only rounding
    assert bool((q.abs() <= 2.0 ** 30).all())
    C0 = torch.full((K, 9), 77.0)
    Cn = KM.new_centers(acc, scale, C0)
    for k in range(K - 1):
        rows = a == k
        exact = (q[rows].sum(dim=0) / scale.double()) / rows.sum()          # fp64 mean of the quantized rows
        assert torch.equal(Cn[k], exact.float())
        raw = Xc[rows].double().mean(dim=0)
        assert bool(((Cn[k].double() - raw).abs() <= 2.0 ** -30 * amax + raw.abs() * 2.0 ** -24).all())
    assert torch.equal(Cn[K - 1], C0[K - 1])                   # the empty cluster keeps its centre


# ------------------------------------------------------------------ Lloyd invariants
@pytest.fixture(scope="module")
def blob_problem():
    return blobs()


def test_lloyd_invariants(blob_problem):
    X, y, _ = blob_problem
    for mode in ("k-means++", "random"):
        m = KMeans(k=6, maxIter=30, initMode=mode, seed=5).fit_tensors(X)
        s = m.summary
        h = s.costHistory
        assert len(h) == s.numIter and s.converged and s.numIter < 30
        assert all(b <= a * (1 + 1e-12) for a, b in zip(h, h[1:])) and s.trainingCost <= h[-1] * (1 + 1e-12)
        assert sum(s.clusterSizes) == X.shape[0]
        pred = m.predict(X)
        assert torch.equal(pred.to(torch.int32), s.predictions)
        assert m.computeCost(X) == pytest.approx(s.trainingCost, rel=1e-12)
        if mode == "k-means++":
            cm, maj, purity = m.label_map(pred, y, 6)
            assert purity >= 0.95 and int(cm.sum()) == X.shape[0] and cm.shape == (6, 6)
    # two fits are bitwise equal
    m2 = KMeans(k=6, maxIter=30, initMode="random", seed=5).fit_tensors(X)
    assert torch.equal(m2._Cw, m._Cw) and m2.summary.costHistory == m.summary.costHistory


def test_empty_cluster_keeps_its_centre(blob_problem):
    X, _, mu = blob_problem
    init = torch.cat([mu[:5], torch.full((1, X.shape[1]), 1e4)], 0)
    m = KMeans(k=6, maxIter=10)._fit_tensors(X, initial_centers=init)
    assert m.summary.clusterSizes[5] == 0
    assert torch.allclose(m.clusterCenters()[5], init[5], rtol=1e-6)


def test_weights_zero_rows_are_ignored(blob_problem):
    X, _, mu = blob_problem
    w = torch.ones(X.shape[0], dtype=torch.int32)
    w[::3] = 0
    est = KMeans(k=6, maxIter=8, seed=1)
    a = est._fit_tensors(X, w, initial_centers=mu)
    b = est._fit_tensors(X[w != 0], None, initial_centers=mu)
    # the same rows count; the column means differ (they are of all rows), so compare in original coordinates
    assert torch.allclose(a.clusterCenters(), b.clusterCenters(), atol=1e-5)
    assert a.summary.clusterSizes == b.summary.clusterSizes
    with pytest.raises(ValueError):
        est._fit_tensors(X, torch.full((X.shape[0],), 0.5))


# ------------------------------------------------------------------ silhouette
def _silhouette_brute(X, lab, K):
    Xd = X.double()
    d = torch.cdist(Xd, Xd) ** 2
    out = torch.zeros(X.shape[0], dtype=torch.float64)
    for i in range(X.shape[0]):
        own = lab == lab[i]
        n = int(own.sum())
        if n <= 1:
            continue
        a = d[i][own].sum() / (n - 1)
        b = min((d[i][lab == k].mean() for k in range(K) if k != int(lab[i]) and bool((lab == k).any())), default=None)
        if b is None:
            continue
        out[i] = (b - a) / max(a, b)
    return out


def test_silhouette_equals_brute_force():
    Xc, comp = mixture(300, 7, 9, comps=4)
    lab = comp.clone()
    lab[lab == 3] = 5            # cluster 3 and 4 empty (K = 6)
    lab[11] = 4                  # a singleton
    rows = KM.silhouette_rows_torch(Xc, lab, 6)
    ref = _silhouette_brute(Xc, lab, 6)
    assert float(rows[11]) == 0.0
    torch.testing.assert_close(rows, ref, rtol=1e-9, atol=1e-12)
    ev = ClusteringEvaluator()
    assert ev.evaluate_tensors(Xc + 3.0, lab, 6) == pytest.approx(float(ref.mean()), rel=1e-6)
    assert float(KM.silhouette(Xc, torch.zeros(300, dtype=torch.long), 1)) == 0.0     # one cluster: no neighbour
    with pytest.raises(ValueError):
        ClusteringEvaluator(metricName="other")


# ------------------------------------------------------------------ tie-rule guard of the GPU assignment test
@pytest.mark.parametrize("N,D,K", ASSIGN_SHAPES)
def test_tie_rule_excludes_few_rows(N, D, K):
    Xc, C, h = assign_case(N, D, K)
    a, clear, d2, atol = tie_rule(Xc, C, h)
    excluded = 1.0 - clear.double().mean().item()
    print(f"N={N} D={D} K={K}: excluded share {excluded:.6f}")
    assert excluded <= 0.01
    assert torch.equal(a, KM.assign_torch(Xc, C, h).assign)


# ------------------------------------------------------------------ data parallel
def _dp_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from har.data.table import Column, Table
    from har.models.base import data_parallel
    from har.parallel import dist as hd

    ctx = hd.init(device="cpu")
    X, _, _ = blobs(1001, 11, 5)
    t = Table([Column("features", "vector", X.double().numpy())])
    with data_parallel(ctx):
        m = KMeans(k=5, maxIter=15, seed=3, device="cpu").fit(t)
    if rank == 0:
        torch.save({"C": m._Cw, "pred": m.predict(X), "it": m.summary.numIter, "cost": m.summary.trainingCost,
                    "sizes": m.summary.clusterSizes, "hist": m.summary.costHistory}, os.path.join(out_dir, f"km_{world}.pt"))
    hd.shutdown(ctx)


@pytest.mark.parametrize("world", [2, 3])
def test_data_parallel_is_bitwise(world):
    d = tempfile.mkdtemp()
    mp.spawn(_dp_worker, args=(world, _free_port(), d), nprocs=world, join=True)
    got = torch.load(os.path.join(d, f"km_{world}.pt"), weights_only=True)
    X, _, _ = blobs(1001, 11, 5)
    m = KMeans(k=5, maxIter=15, seed=3, device="cpu").fit_tensors(X)
    assert torch.equal(got["C"], m._Cw) and torch.equal(got["pred"], m.predict(X))
    assert got["it"] == m.summary.numIter and got["sizes"] == m.summary.clusterSizes
    assert got["cost"] == pytest.approx(m.summary.trainingCost, rel=1e-12)
    assert got["hist"] == pytest.approx(m.summary.costHistory, rel=1e-12)


# ------------------------------------------------------------------ persistence and commands
def test_persist_round_trip(tmp_path, blob_problem):
    from har.utils import persist

    X, y, _ = blob_problem
    m = KMeans(k=6, seed=2).fit_tensors(X)
    m.label_map(m.predict(X), y, 6)
    persist.save(m, str(tmp_path / "km"), labels=list("abcdef"))
    r = persist.load(str(tmp_path / "km"), device="cpu")
    assert isinstance(r, KMeansModel) and r.k == 6
    assert torch.equal(r.predict(X), m.predict(X)) and torch.equal(r.clusterCenters(), m.clusterCenters())
    assert r.summary.as_dict() == m.summary.as_dict() and r.majority_labels == m.majority_labels


def test_cli_kmeans_then_predict_on_synthetic_raw(tmp_path):
    import main
    import predict
    from har.features.raw import raw_to_table, write_synthetic_raw

    p = str(tmp_path / "raw.csv")
    write_synthetic_raw(p, n_windows=120, users=4)
    mdir = tmp_path / "models"
    base = ["--raw", p, "--device", "cpu", "--preset", "lr-cpu"]
    s0 = main.run(main.config_from_args(base + ["--out-dir", str(tmp_path / "plain")]))
    s = main.run(main.config_from_args(base + ["--out-dir", str(tmp_path / "out"), "--kmeans", "6", "--kmeans-init",
                                               "random", "--kmeans-max-iter", "10", "--save-models", str(mdir)]))
    assert "kmeans" not in s0 and s["kmeans"]["k"] == 6 and sum(s["kmeans"]["cluster_sizes"]) == s["n_train"]
    assert 0.0 <= s["kmeans"]["purity"] <= 1.0 and -1.0 <= s["kmeans"]["silhouette"] <= 1.0
    txt = open(tmp_path / "out" / "result.txt").read()
    assert "Silhouette (test)" in txt and "Cluster x label" in txt
    with open(tmp_path / "out" / "metrics.jsonl") as f:
        assert "kmeans" in json.loads(f.readlines()[-1])
    # without the switch the text keeps its bytes: the run with it is the same text (up to the runs' own
    # timings and uids) followed by the KMeans block
    plain = open(tmp_path / "plain" / "result.txt").read()
    mask = lambda v: re.sub(r"[0-9a-f]{20}|\d+\.\d+(e-?\d+)?|\d+e-\d+", "#", v)
    assert "KMeans" not in plain and mask(txt.split("KMeans" + "-" * 60)[0]) == mask(plain)

    t = raw_to_table(p)
    tab = tmp_path / "windows.csv"
    with open(tab, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(t.columns)
        cols = [t[c].data for c in t.columns]
        for i in range(t.count()):
            w.writerow([c[i] for c in cols])
    out = tmp_path / "pred.csv"
    rec = predict.main(["--models", str(mdir), "--model", "kmeans", "--data", str(tab), "--device", "cpu", "--out",
                        str(out)])
    assert rec["rows"] == 120 and 1 <= rec["clusters_used"] <= 6 and "majority_label_accuracy" in rec
    with open(out) as f:
        rows = list(csv.reader(f))
    assert len(rows) == 121 and rows[0][-3:] == ["cluster", "majority_label", "label_name"]


# ------------------------------------------------------------------ range checks
def test_range_checks():
    X = torch.randn(20, 4)
    with pytest.raises(ValueError):
        KMeans(k=0).fit_tensors(X)
    with pytest.raises(ValueError):
        KMeans(k=21).fit_tensors(X)
    with pytest.raises(ValueError):
        KMeans(k=KM.MAX_K + 1).fit_tensors(torch.randn(KM.MAX_K + 2, 4))
    with pytest.raises(ValueError):
        KMeans(k=2).fit_tensors(torch.randn(20, KM.MAX_D + 1))
    with pytest.raises(ValueError):
        KMeans(k=2, initMode="other").fit_tensors(X)
    with pytest.raises(ValueError):
        KM.check_native_range(2, 0)
    assert KMeans(k=20, maxIter=2).fit_tensors(X).k == 20
