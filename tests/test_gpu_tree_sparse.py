"""One-hot-aware trees on the reference encoding.

The reference grows DecisionTree(depth 3) / RandomForest(100 x depth 4) on a 3,100-wide vector of
three one-hot blocks (934 + 1,401 + 755 binary columns) and 10 numeric columns (``Main/main.py:51-66,
297,478``).  The one-hot-aware path (``ops/tree.py`` find_thresholds_hybrid / bins_hybrid, tree.hip
SPARSE) takes the one-hot columns' 0 | 1 split from their entries instead of a sort, bins from the
hybrid parts and histograms a one-hot column over its nonzeros only (bin 0 = node totals - bin 1).
Every test pins it to the dense path of the same fit: thresholds, bins and whole forests bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _tree_sparse_util import arrays_hash as _arrays_hash
from _tree_sparse_util import dense_path as _dense_path
from _tree_sparse_util import same_arrays as _same_arrays
from _tree_sparse_util import synthetic_hybrid as _synthetic_hybrid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wisdm_ref(cuda, wisdm_csv):
    from har.suite import load_wisdm

    train, test, _ = load_wisdm(wisdm_csv, "reference", 2018, device=cuda)
    return train, test


@pytest.mark.parametrize("n,sample", [(3853, False), (24000, True)])
def test_hybrid_thresholds_and_bins_equal_dense(cuda, n, sample):
    from har.ops import tree as T
    from har.ops.stats import bin_features

    hm, _ = _synthetic_hybrid(cuda, N=n, seed=n)
    X = hm.to_dense()
    assert (T.threshold_sample_weights(n, 32) is not None) == sample
    for mb in (32, 2, 5):
        a = T.find_thresholds_hybrid(hm, mb, seed=7)
        b = T.ThresholdTable.from_any(T.find_thresholds_device(X, mb, seed=7))
        assert np.array_equal(a.counts, b.counts)
        w = max(a.mat.shape[1], b.mat.shape[1])
        assert np.array_equal(a.padded(w), b.padded(w))
        nb = torch.from_numpy((a.counts + 1).astype(np.int32)).to(cuda)
        thr = torch.from_numpy(a.padded(mb)).to(cuda)
        assert torch.equal(T.bins_hybrid(hm, thr, nb), bin_features(X, a))
        # the device-resident version (no host round trip): the same padded matrix and bin counts
        d = T.thresholds_hybrid_device(hm, mb, seed=7)
        assert d is not None
        assert torch.equal(d.nbins, nb) and torch.equal(d.thr_mat, thr)


def test_hybrid_all_ones_column_has_no_split(cuda):
    from har.ops import tree as T

    hm, _ = _synthetic_hybrid(cuda, N=3000, all_ones_block=True)
    tt = T.find_thresholds_hybrid(hm, 32)
    off, w = hm.blocks[-1]
    assert tt.counts[off] == 0  # every row holds it: one distinct value
    assert (tt.counts[off + w - 2:off + w] == 0).all()  # never set
    ref = T.ThresholdTable.from_any(T.find_thresholds_device(hm.to_dense(), 32))
    assert np.array_equal(tt.counts, ref.counts)


@pytest.mark.parametrize("kind", ["dt", "dt7", "rf", "rf_sub"])
def test_sparse_forest_equals_dense_synthetic(cuda, kind):
    from har.models.tree import DecisionTreeClassifier, RandomForestClassifier

    hm, y = _synthetic_hybrid(cuda, N=12000, seed=3)
    X = hm.to_dense()
    est = {"dt": lambda: DecisionTreeClassifier(maxDepth=3),
           "dt7": lambda: DecisionTreeClassifier(maxDepth=7, minInstancesPerNode=3),
           "rf": lambda: RandomForestClassifier(numTrees=20, maxDepth=5, seed=11),
           "rf_sub": lambda: RandomForestClassifier(numTrees=8, maxDepth=6, seed=2, subsamplingRate=0.6,
                                                    featureSubsetStrategy="onethird")}[kind]
    m = est().fit_tensors(X, y, 4, hybrid=hm)
    r = _dense_path(lambda: est().fit_tensors(X, y, 4))
    _same_arrays(m.arrs, r.arrs)


def test_sparse_reference_suite_fits_equal_dense(wisdm_ref):
    """The reference's DecisionTree(depth 3) and RandomForest(100 x depth 4) on WISDM: the
    one-hot-aware fits (eager, graph capture, graph replay) grow the dense path's forests."""
    from har.models import tree as tr
    from har.models.tree import DecisionTreeClassifier, RandomForestClassifier

    train, test = wisdm_ref
    tr._fit_graphs.clear()  # (a full graph cache would keep the capture from happening)
    tr._fit_graph_seen.clear()
    for make in (lambda: DecisionTreeClassifier(featuresCol="features", labelCol="label", maxDepth=3, maxBins=32),
                 lambda: RandomForestClassifier(featuresCol="features", labelCol="label", numTrees=100, maxDepth=4,
                                                maxBins=32, seed=2018)):
        ref = _dense_path(lambda: make().fit(train))
        est = make()
        assert est._hybrid(train, ref.device) is not None, "the reference encoding must take the sparse path"
        kinds = []
        for _ in range(3):  # eager, capture, replay
            m = est.fit(train)
            kinds.append(tr.LAST_FIT_KIND)
            _same_arrays(m.arrs, ref.arrs)
        assert kinds == ["eager", "capture", "replay"], kinds
        Xt = m.features_input(test)
        assert torch.equal(m.predict(Xt), ref.predict(Xt))


def test_sparse_tree_cross_validation_equals_dense(wisdm_ref):
    """DT-CV / RF-CV (fit_folds: every fold's trees in one build) on the reference encoding."""
    from har.evaluation.evaluators import MulticlassClassificationEvaluator
    from har.models.tree import DecisionTreeClassifier, RandomForestClassifier
    from har.tuning.crossval import CrossValidator, ParamGridBuilder

    train, _ = wisdm_ref
    for base, grid in ((DecisionTreeClassifier(maxDepth=3), ParamGridBuilder().addGrid("maxDepth", [2, 3]).build()),
                       (RandomForestClassifier(numTrees=10, maxDepth=3, seed=5),
                        ParamGridBuilder().addGrid("numTrees", [5, 10]).build())):
        def cv():
            return CrossValidator(estimator=base, estimatorParamMaps=grid,
                                  evaluator=MulticlassClassificationEvaluator(metricName="accuracy"),
                                  numFolds=3, seed=7).fit(train)

        a = cv()
        b = _dense_path(cv)
        assert a.avgMetrics == b.avgMetrics
        _same_arrays(a.bestModel.arrs, b.bestModel.arrs)


# --- what the level kernel's launcher refuses, the fit takes on the dense path -------------------------------
def _launcher_lds(F, max_bins, K, m=None):
    """``har_tree_hist_split_planned``'s dynamic LDS with the one-hot-aware kernel on (tree.hip), restated:
    fc * maxbins * K * 4 + fc * 4 + K * 4 + F * 2 + fc * 3, fc = min(m, 96 KB / (maxbins K 4)) features."""
    fc = max(1, min(F if m is None else m, 96 * 1024 // (max_bins * K * 4)))
    return fc * max_bins * K * 4 + fc * 4 + K * 4 + F * 2 + fc * 3


LDS_CAP = 150 * 1024  # the launcher's limit (contract code -3 above it)


def _sparse_calls(monkeypatch):
    """Counts the fits that take the one-hot-aware path (``ForestBuilder.prepare`` builds its kernel input)."""
    from har.ops import tree as T

    calls = []
    real = T.sparse_tree_input

    def spy(hm):
        calls.append(hm.n_features)
        return real(hm)

    monkeypatch.setattr(T, "sparse_tree_input", spy)
    return calls


def _wide_hybrid(cuda, width):
    hm, y = _synthetic_hybrid(cuda, N=512, widths=(width,), Fd=5, seed=9)
    assert hm.n_features == width + 5 and int(y.max()) == 3
    return hm, y


def test_hybrid_too_wide_for_the_sparse_kernels_lds_takes_the_dense_path(cuda, monkeypatch):
    """One one-hot block of 28,000 columns + 5 numeric ones, K = 4, maxBins = 32: the one-hot-aware kernel
    would need 192 * 32 * 4 * 4 + 192 * 4 + 4 * 4 + 28,005 * 2 + 192 * 3 = 155,674 bytes of LDS, above the
    launcher's 153,600.  The fit must not raise: ``hybrid_tree_ok`` refuses the matrix and the depth-3 tree
    is the dense path's."""
    from har.models.tree import DecisionTreeClassifier
    from har.ops import tree as T

    hm, y = _wide_hybrid(cuda, 28000)
    assert _launcher_lds(hm.n_features, 32, 4) == 155674 > LDS_CAP
    calls = _sparse_calls(monkeypatch)
    X = hm.to_dense()
    m = DecisionTreeClassifier(maxDepth=3).fit_tensors(X, y, 4, hybrid=hm)
    assert not calls
    r = _dense_path(lambda: DecisionTreeClassifier(maxDepth=3).fit_tensors(X, y, 4))
    _same_arrays(m.arrs, r.arrs)
    assert int(m.arrs.n_nodes[0]) > 1
    assert T.hybrid_tree_ok(hm, 32, 4) is False and T.hybrid_tree_ok(hm) is False
    assert T.sparse_hist_lds_bytes(hm.n_features, 32, 4) == 155674


def test_widest_hybrid_the_sparse_kernel_takes_equals_dense(cuda, monkeypatch):
    """The largest column count the launcher's LDS formula accepts at K = 4, maxBins = 32 (and one more is
    refused): ``hybrid_tree_ok`` agrees on both sides of the limit, the accepted matrix really takes the
    one-hot-aware kernel, and its tree is the dense path's bit for bit."""
    from har.models.tree import DecisionTreeClassifier
    from har.ops import tree as T

    F = max(f for f in range(6, 32768) if _launcher_lds(f, 32, 4) <= LDS_CAP)
    assert _launcher_lds(F + 1, 32, 4) > LDS_CAP and 20000 < F < 28005
    hm, y = _wide_hybrid(cuda, F - 5)
    over, _ = _wide_hybrid(cuda, F - 4)
    assert T.hybrid_tree_ok(hm, 32, 4) is True and T.hybrid_tree_ok(over, 32, 4) is False
    calls = _sparse_calls(monkeypatch)
    X = hm.to_dense()
    m = DecisionTreeClassifier(maxDepth=3).fit_tensors(X, y, 4, hybrid=hm)
    assert calls == [F]
    r = _dense_path(lambda: DecisionTreeClassifier(maxDepth=3).fit_tensors(X, y, 4))
    assert calls == [F]
    _same_arrays(m.arrs, r.arrs)
    assert int(m.arrs.n_nodes[0]) > 1


_FLOAT_ATOMICS_CHILD = """
import sys
sys.path.insert(0, "tests")
import torch
from _tree_sparse_util import arrays_hash, synthetic_hybrid
from har.models.tree import DecisionTreeClassifier
from har.ops import tree as T

cuda = torch.device("cuda:0")
hm, y = synthetic_hybrid(cuda, N=2000)
m = DecisionTreeClassifier(maxDepth=3).fit_tensors(hm.to_dense(), y, 4, hybrid=hm)
print("OK", int(T.hybrid_tree_ok(hm, 32, 4)), int(T.hybrid_tree_ok(hm)), arrays_hash(m.arrs))
"""


def test_float_atomics_switch_takes_the_dense_path(cuda):
    """``HAR_HIST_FLOAT_ATOMICS=1`` (read once per process by the library, hence a fresh child): the launcher
    refuses the one-hot-aware kernel (code -8), so ``hybrid_tree_ok`` must too and the fit must grow the dense
    path's tree — which, the float and the integer histograms being equal on integer weights, is this
    process's dense-path tree."""
    from har.models.tree import DecisionTreeClassifier
    from har.ops import tree as T

    assert os.environ.get("HAR_HIST_FLOAT_ATOMICS", "0")[:1] != "1"
    hm, y = _synthetic_hybrid(cuda, N=2000)
    assert T.hybrid_tree_ok(hm, 32, 4)
    X = hm.to_dense()
    want = _arrays_hash(_dense_path(lambda: DecisionTreeClassifier(maxDepth=3).fit_tensors(X, y, 4)).arrs)
    assert want == _arrays_hash(DecisionTreeClassifier(maxDepth=3).fit_tensors(X, y, 4, hybrid=hm).arrs)
    env = dict(os.environ, HAR_HIST_FLOAT_ATOMICS="1")
    env.pop("HAR_TREE_SPARSE", None)
    r = subprocess.run([sys.executable, "-c", _FLOAT_ATOMICS_CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("OK ")][-1].split()
    assert line[1:3] == ["0", "0"], line
    assert line[3] == want
