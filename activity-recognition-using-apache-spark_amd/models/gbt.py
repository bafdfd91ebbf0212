"""GBTClassifier — multiclass gradient-boosted trees (the estimator next to ``RandomForestClassifier``
in MLlib, which this project lacked).

Spark's ``GBTClassifier`` is binary only and fits variance-impurity regression trees to the
log-loss pseudo-residuals; this one boosts the multinomial softmax log-loss with Newton steps for any
K >= 2 (binary = the same path with K = 2): round m grows K regression trees in lock step, one per
class, on shared rows and bins, from second-order gains (``har/ops/gbt.py`` defines every piece).
Parameters carry Spark's names where Spark has them; ``regLambda`` (L2 on the leaf values) is new.

Engine: findSplits thresholds and the uint8 feature-major bins are the forest builder's
(``ops/tree.thresholds_for``, ``ops/stats.bin_features``).  On a GPU a round is enqueued as
``har_gbt_grad`` -> per level (``har_gbt_hist``, ``har_gbt_split``, ``har_gbt_partition``) ->
``har_gbt_update`` with no device -> host read; only the loss history and the node counts are read,
after the fit.  On a CPU the same loop runs the PyTorch definitions.  Derivatives are fixed point
(2^-20), so every sum is an exact integer sum and two fits with one seed are bitwise equal.

The model keeps its ``maxIter * K`` trees as one ``ForestArrays`` (tree t boosts class t % K; its leaf
statistics are zero except at that class), so prediction is the existing forest kernel:
``predict_raw = init + har_forest_predict(normalize=False)``, probability = softmax.
"""
from __future__ import annotations

import numpy as np
import torch

from ..data.table import Table
from ..ops import gbt as G
from ..ops import tree as T
from .base import ClassificationModel, ClassifierParams, Estimator, features_tensor, labels_tensor, new_uid, \
    num_label_classes, resolve_device
from .tree import ForestArrays, predict_forest

PRIOR_FLOOR = 1e-12  # a class absent from the training rows: its prior is clamped before the log


class GBTClassificationModel(ClassificationModel):
    def __init__(self, arrs: ForestArrays, init: torch.Tensor, num_features: int, num_classes: int,
                 loss_history=None, uid=None, device=None):
        super().__init__(uid or new_uid("GBTClassifier"))
        self.arrs = arrs
        self.device = device or arrs.feature.device
        self.init = init.to(device=self.device, dtype=torch.float32)
        self.num_features, self.num_classes = num_features, num_classes
        self.trainLossHistory = [float(v) for v in (loss_history if loss_history is not None else [])]

    @property
    def getNumTrees(self) -> int:
        return int(self.arrs.feature.shape[0])

    @property
    def totalNumNodes(self) -> int:
        return int(self.arrs.n_nodes.sum())

    @property
    def featureImportances(self) -> torch.Tensor:
        """Gain sums per feature over all trees, normalized to 1."""
        feat = self.arrs.feature.cpu()
        g = self.arrs.gain.cpu().double()
        m = feat >= 0
        imp = torch.zeros(self.num_features, dtype=torch.float64)
        imp.index_add_(0, feat[m].long(), g[m])
        s = imp.sum()
        return imp / s if s > 0 else imp

    def predict_raw(self, X):
        X = X.to(self.device)
        if self.getNumTrees == 0:
            return self.init.view(1, -1).expand(X.shape[0], -1).contiguous()
        return predict_forest(self.arrs, X, normalize=False) + self.init.view(1, -1)

    def raw_to_probability(self, raw: torch.Tensor) -> torch.Tensor:
        return torch.softmax(raw, dim=1)

    def __str__(self):
        return f"GBTClassificationModel (uid={self.uid}) with {self.getNumTrees} trees"

    def state(self):
        a = self.arrs
        return {"feature": a.feature.cpu(), "threshold": a.threshold.cpu(), "left": a.left.cpu(),
                "right": a.right.cpu(), "stats": a.stats.cpu(), "gain": a.gain.cpu(),
                "n_nodes": torch.as_tensor(a.n_nodes), "init": self.init.cpu(),
                "loss_history": torch.tensor(self.trainLossHistory, dtype=torch.float64), "max_depth": a.max_depth}


class GBTClassifier(Estimator, ClassifierParams):
    _param_names = ("maxIter", "stepSize", "maxDepth", "maxBins", "minInstancesPerNode", "minInfoGain",
                    "subsamplingRate", "regLambda", "seed", "featuresCol", "labelCol", "device")

    def __init__(self, featuresCol="features", labelCol="label", maxIter: int = 20, stepSize: float = 0.1,
                 maxDepth: int = 5, maxBins: int = 32, minInstancesPerNode: int = 1, minInfoGain: float = 0.0,
                 subsamplingRate: float = 1.0, regLambda: float = 1.0, seed: int = 0, device=None):
        super().__init__(new_uid("GBTClassifier"))
        self.featuresCol, self.labelCol = featuresCol, labelCol
        self.maxIter, self.stepSize, self.maxDepth, self.maxBins = maxIter, stepSize, maxDepth, maxBins
        self.minInstancesPerNode, self.minInfoGain = minInstancesPerNode, minInfoGain
        self.subsamplingRate, self.regLambda, self.seed, self.device = subsamplingRate, regLambda, seed, device

    def fit(self, table: Table) -> GBTClassificationModel:
        dev = resolve_device(self.device)
        X = features_tensor(table, self.featuresCol, dev)
        y = labels_tensor(table, self.labelCol, dev)
        K = num_label_classes(table, self.labelCol, dev)
        return self.fit_tensors(X, y, max(K, 2))

    def _check(self, K: int):
        G.check_native_range(self.maxDepth, self.maxBins, K)
        if int(self.maxIter) < 0:
            raise ValueError("maxIter must be >= 0")
        if int(self.minInstancesPerNode) < 1:
            raise ValueError("minInstancesPerNode must be >= 1")
        if not 0.0 < float(self.subsamplingRate) <= 1.0:
            raise ValueError("subsamplingRate must be in (0, 1]")
        if float(self.regLambda) < 0.0 or float(self.stepSize) <= 0.0:
            raise ValueError("regLambda must be >= 0 and stepSize > 0")

    def fit_tensors(self, X, y, K, thresholds=None) -> GBTClassificationModel:
        return self._fit_tensors(X, y, K, thresholds)

    def _fit_tensors(self, X, y, K, thresholds=None, native=None, q_hook=None) -> GBTClassificationModel:
        """The fit.  Private knobs of the probe and the tests: ``native=False`` runs the PyTorch definitions on
        GPU tensors (``tools/gbt_probe.py`` times them against the kernels; the public ``fit`` / ``fit_tensors``
        always take the kernels on a GPU), ``q_hook(round, qgh) -> qgh`` may replace a round's quantized
        derivatives."""
        self._check(K)
        dev = X.device
        N, F = X.shape
        if N < 1 or N > G.MAX_ROWS:
            raise ValueError(f"GBT takes 1..{G.MAX_ROWS} rows, got {N}")
        if int(y.min()) < 0 or int(y.max()) >= K:  # the fit's one read before the rounds
            raise ValueError("labels out of range")
        from ..ops.stats import bin_features

        if isinstance(thresholds, T.DeviceThresholds):
            thresholds = thresholds.to_table()
        if thresholds is None:
            thresholds = T.thresholds_for(X, self.maxBins, seed=self.seed)
        tt = T.ThresholdTable.from_any(thresholds)
        nbins = torch.from_numpy((tt.counts + 1).astype(np.int32)).to(dev)
        thr_mat = torch.from_numpy(tt.padded(self.maxBins)).to(dev)
        bins = bin_features(X, tt).to(dev).contiguous()
        y32 = y.to(torch.int32).contiguous()
        D, B, M = int(self.maxDepth), int(self.maxBins), int(self.maxIter)
        lam, step = float(self.regLambda), float(self.stepSize)
        min_inst, min_gain = int(self.minInstancesPerNode), float(self.minInfoGain)
        # initial margins: the log class priors (fp64 on the device, stored fp32)
        cnt = torch.bincount(y.long(), minlength=K).double()
        init = torch.log((cnt / N).clamp_min(PRIOR_FLOOR)).float()
        margins = init.view(1, K).repeat(N, 1).contiguous()
        arrs = G.GBTArrays.alloc(M * K, D, K, dev)
        native = X.is_cuda if native is None else bool(native)
        node_of = torch.empty(K, N, dtype=torch.int32, device=dev)
        hist_buf = None
        if native:
            nb = _n_loss_blocks(N, K)
            hist_buf = torch.empty(K * (1 << (D - 1)) * F * B * G.HCH, dtype=torch.int64, device=dev)
        else:
            nb = 1
        losses = torch.zeros(M + 1, nb, dtype=torch.float64, device=dev)
        for m in range(M):
            w = G.round_weights(self.seed, m, N, float(self.subsamplingRate), dev)
            if native:
                qgh, _ = G.grad_native(margins, y32, w, loss_out=losses[m])
            else:
                qgh, l = G.grad_torch(margins, y32, w)
                losses[m] = l
            if q_hook is not None:
                qgh = q_hook(m, qgh)
            node_of = G.grow_round(bins, nbins, thr_mat, qgh, w, arrs, m * K, D, B, lam, step, min_inst, min_gain,
                                   native=native, node_of=node_of, hist_buf=hist_buf)
            G.update(margins, node_of, arrs, m * K, native=native)
        if native:
            G.grad_native(margins, y32, None, want_q=False, loss_out=losses[M])
        else:
            losses[M] = G.grad_torch(margins, y32, None)[1]
        # the fit's reads: loss history and node counts
        hist = (losses.sum(dim=1) / N).cpu().tolist()
        n_nodes = ((arrs.feature >= 0).sum(dim=1) * 2 + 1).cpu().numpy().astype(np.int64)
        fa = ForestArrays(arrs.feature, arrs.thresh, arrs.left, arrs.right, arrs.stats, n_nodes, D, arrs.gains)
        return GBTClassificationModel(fa, init, F, K, hist, uid=self.uid, device=dev)


def _n_loss_blocks(N: int, K: int) -> int:
    from ..ops import _native

    return max(1, int(_native.kernels().gbt_grad_blocks(N, K)))


__all__ = ["GBTClassifier", "GBTClassificationModel"]
