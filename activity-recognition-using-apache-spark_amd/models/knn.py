"""KNNClassifier / KNNClassificationModel — exact (brute-force) k-nearest neighbours under the Euclidean
distance; ``har/ops/knn.py`` defines every operation.

Fitting keeps the training rows: it computes the column moments, stores the working rows ``Z = (X - mean) /
std`` (``standardize=False``: only the mean is removed) with their labels on the device and precomputes ``h =
||z||^2 / 2``.  A prediction is one ``knn_search`` (scores on the fp32 matrix cores fused with the running
top-k: the queries-by-references scores are never stored) and one ``knn_merge_vote``; nothing is read back
from the device in between.  The neighbours are the k smallest (score, index) pairs, so the lists do not
depend on the batching of the queries or on the split of the references.

The pair exclusion of the search (``qgroup[n] == rgroup[m] >= 0``) evaluates a whole protocol with ONE search
of a table against itself: ``leave_group_out`` (leave-one-out, leave-one-subject-out) and the CrossValidator's
folds (``cv_predictions``).  Both take the moments of the WHOLE table (features only, never labels) — the one
deviation from refitting per group, see PARITY.md.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from ..data.table import Table
from ..ops import knn as KN
from .base import ClassificationModel, ClassifierParams, Estimator, features_tensor, labels_tensor, new_uid, \
    num_label_classes, resolve_device


class KNNClassificationModel(ClassificationModel):
    _param_names = ("k", "weights", "standardize", "featuresCol", "labelCol")

    def __init__(self, Z: torch.Tensor, y: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, num_classes: int,
                 k: int = 5, weights: str = "uniform", standardize: bool = True, uid=None, device=None):
        super().__init__(uid or new_uid("KNNClassifier"))
        self.device = torch.device(device) if device is not None else Z.device
        self._Z = Z.to(device=self.device, dtype=torch.float32).contiguous()      # working rows, as fitted
        self._y = y.to(device=self.device, dtype=torch.int32).contiguous()
        self.mean = mean.to(device=self.device, dtype=torch.float32).contiguous()
        self.std = std.to(device=self.device, dtype=torch.float32).contiguous()
        self._h = KN.reference_h(self._Z)
        self.num_classes = int(num_classes)
        self.k, self.weights, self.standardize = int(k), weights, bool(standardize)
        KN.check_range(self.k, self.num_features, C=self.num_classes, M=self._Z.shape[0], weights=weights)

    @property
    def num_features(self) -> int:
        return int(self._Z.shape[1])

    @property
    def num_rows(self) -> int:
        return int(self._Z.shape[0])

    def _working_rows(self, X: torch.Tensor) -> torch.Tensor:
        X = X.to(device=self.device, dtype=torch.float32)
        if X.dim() != 2 or X.shape[1] != self.num_features:
            raise ValueError(f"KNNClassificationModel takes [N, {self.num_features}] rows, got {tuple(X.shape)}")
        return KN.working_rows(X, self.mean, self.std)

    @staticmethod
    def _groups(exclude, N, M, dev):
        if exclude is None:
            return None, None
        qg, rg = (torch.as_tensor(g).to(device=dev, dtype=torch.int32).contiguous() for g in exclude)
        if qg.numel() != N or rg.numel() != M:
            raise ValueError("exclude = (qgroup [N], rgroup [M])")
        return qg, rg

    def kneighbors(self, X: torch.Tensor, k: Optional[int] = None, exclude=None, native: Optional[bool] = None):
        """(idx int32 [N, k] into the training rows, d2 fp32 [N, k] in the working coordinates), ascending."""
        Q = self._working_rows(X)
        qg, rg = self._groups(exclude, Q.shape[0], self.num_rows, self.device)
        return KN.neighbors(Q, self._Z, self._h, self.k if k is None else int(k), qg, rg, native)

    def _search(self, Q, qg=None, rg=None, k=None, weights=None, native=None) -> KN.SearchResult:
        return KN.search(Q, self._Z, self._h, self.k if k is None else int(k), native, qgroup=qg, rgroup=rg,
                         y=self._y, C=self.num_classes, weights=self.weights if weights is None else weights)

    def predict_raw(self, X: torch.Tensor) -> torch.Tensor:
        return self._search(self._working_rows(X)).vote.raw

    def predict_all(self, X: torch.Tensor):
        v = self._search(self._working_rows(X)).vote
        pred = v.pred if self.thresholds is None else self._predict_from_probability(v.prob)
        return v.raw, v.prob, pred

    def state(self) -> Dict:
        return {"working_rows": self._Z.cpu(), "labels": self._y.cpu(), "mean": self.mean.cpu(), "std": self.std.cpu(),
                "k": self.k, "weights": self.weights, "standardize": self.standardize}

    @classmethod
    def from_state(cls, t, st, num_classes: int, uid=None, device=None) -> "KNNClassificationModel":
        return cls(t["working_rows"], t["labels"], t["mean"], t["std"], num_classes, int(st["k"]), st["weights"],
                   bool(st["standardize"]), uid=uid, device=device)

    def __str__(self):
        return (f"KNNClassificationModel (uid={self.uid}) with k={self.k}, {self.num_rows} rows, "
                f"{self.num_classes} classes")


class KNNClassifier(Estimator, ClassifierParams):
    _param_names = ("k", "weights", "standardize", "featuresCol", "labelCol", "device")

    def __init__(self, k: int = 5, weights: str = "uniform", standardize: bool = True, featuresCol="features",
                 labelCol="label", device=None):
        super().__init__(new_uid("KNNClassifier"))
        self.k, self.weights, self.standardize = k, weights, standardize
        self.featuresCol, self.labelCol, self.device = featuresCol, labelCol, device

    def _prep(self, table: Table):
        dev = resolve_device(self.device)
        return (features_tensor(table, self.featuresCol, dev), labels_tensor(table, self.labelCol, dev),
                num_label_classes(table, self.labelCol, dev))

    def fit_tensors(self, X: torch.Tensor, y: torch.Tensor, K: int) -> KNNClassificationModel:
        if X.dim() != 2 or X.shape[0] < 1:
            raise ValueError("KNNClassifier takes a non-empty [N, D] matrix")
        KN.check_range(int(self.k), X.shape[1], C=K, M=X.shape[0], weights=self.weights)
        Xf = X.float()
        mean, std = KN.standardizer(Xf, bool(self.standardize))
        m = KNNClassificationModel(KN.working_rows(Xf, mean, std), y, mean, std, K, int(self.k), self.weights,
                                   bool(self.standardize), uid=self.uid, device=X.device)
        m.featuresCol, m.labelCol = self.featuresCol, self.labelCol
        return m

    def fit(self, table: Table) -> KNNClassificationModel:
        return self.fit_tensors(*self._prep(table))

    # ------------------------------------------------------------------ grouped searches of a table against itself
    def leave_group_out(self, table: Table, groupCol: Optional[str] = None) -> torch.Tensor:
        """int64 [N]: the prediction of every row from the rows of the OTHER groups (``groupCol`` None: every row
        is its own group, leave-one-out), by one grouped search of the table against itself."""
        X, y, K = self._prep(table)
        N = X.shape[0]
        if groupCol is None:
            g = torch.arange(N, dtype=torch.int32, device=X.device)
        else:
            codes = np.unique(np.asarray(table[groupCol].data), return_inverse=True)[1]
            g = torch.as_tensor(codes.astype(np.int32)).to(X.device)
        m = self.fit_tensors(X, y, K)
        return m._search(m._Z, g, g).vote.pred

    def cv_predictions(self, table: Table, fold_ids: torch.Tensor, maps: List[Dict]):
        """The CrossValidator's branch: (labels [N], predictions int64 [maps, N], class weights fp64 [maps, N, K],
        K) with every row predicted from the rows of the other folds — ONE search at the largest k of the
        maps, one vote per map on the list prefixes."""
        X, y, K = self._prep(table)
        subs = [self.copy(pm) for pm in maps]
        kmax = max(int(s.k) for s in subs)
        m = self.copy({"k": kmax}).fit_tensors(X, y, K)
        g = fold_ids.to(device=X.device, dtype=torch.int32).contiguous()
        idx, d2 = KN.neighbors(m._Z, m._Z, m._h, kmax, g, g)
        votes = [KN.vote(idx, d2, m._y, K, s.weights, int(s.k)) for s in subs]
        return y, torch.stack([v.pred for v in votes]), torch.stack([v.raw for v in votes]), K


__all__ = ["KNNClassifier", "KNNClassificationModel"]
