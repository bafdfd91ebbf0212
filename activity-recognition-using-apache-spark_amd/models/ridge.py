"""RidgeClassifier / RidgeClassificationModel — one-vs-rest ridge regression on ±1 targets from Gram moments,
with the penalty chosen by one-pass k-fold cross-validation; ``har/ops/ridge.py`` defines every operation.

Fitting makes ONE pass over the rows (``ridge_gram``: the per-fold second moments on the fp32 matrix cores), then
solves ``(numFolds + 1) * len(alphas)`` bordered D x D systems by a batched blocked Cholesky in fp64: fold f's
training Gram is the total minus the fold's own, so the selection needs no second pass.  Every (fold, alpha)
model scores its own fold through one fp32 GEMM; counts and choice stay on the device and one host read ends
the fit.  The standardisation (the WHOLE table's column moments — features only, never labels, the same
deviation as kNN's, see PARITY.md) is folded into the weights, so serving is one product on the raw rows.
``probability`` is ``softmax(raw)``: uncalibrated, there so that HMMSmoother can consume it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from ..data.split import kfold_ids
from ..data.table import Table
from ..ops import ridge as RD
from .base import ClassificationModel, ClassifierParams, Estimator, features_tensor, labels_tensor, new_uid, \
    num_label_classes, resolve_device


@dataclass
class RidgeSummary:
    alpha: float
    alphas: List[float]
    cvCorrect: List[int]     # per alpha: correctly predicted held-out rows summed over the folds
    info: List[int]          # per system: 0, or 1 + the column whose pivot failed
    numFolds: int


class RidgeClassificationModel(ClassificationModel):
    _param_names = ("featuresCol", "labelCol")

    def __init__(self, Wx: torch.Tensor, bx: torch.Tensor, alpha: float = 0.0, summary: Optional[RidgeSummary] = None,
                 uid=None, device=None):
        super().__init__(uid or new_uid("RidgeClassifier"))
        self.device = torch.device(device) if device is not None else Wx.device
        self.Wx = Wx.to(device=self.device, dtype=torch.float32).contiguous()     # [K, D] on the raw rows
        self.bx = bx.to(device=self.device, dtype=torch.float32).contiguous()
        self.num_classes, self.num_features = int(self.Wx.shape[0]), int(self.Wx.shape[1])
        self.alpha = float(alpha)
        self.summary = summary

    def predict_raw(self, X: torch.Tensor) -> torch.Tensor:
        X = X.to(device=self.device, dtype=torch.float32)
        if X.dim() != 2 or X.shape[1] != self.num_features:
            raise ValueError(f"RidgeClassificationModel takes [N, {self.num_features}] rows, got {tuple(X.shape)}")
        return RD.predict_raw(X, self.Wx, self.bx)

    def raw_to_probability(self, raw):
        return torch.softmax(raw.double(), dim=1)

    def predict_all(self, X: torch.Tensor):
        raw = self.predict_raw(X)
        prob = self.raw_to_probability(raw)
        pred = RD.first_argmax(raw) if self.thresholds is None else self._predict_from_probability(prob)
        return raw, prob, pred

    def state(self) -> Dict:
        s = self.summary
        st = {"coefficients": self.Wx.cpu(), "intercepts": self.bx.cpu(), "alpha": self.alpha}
        if s is not None:
            st.update({"alphas": list(s.alphas), "cvCorrect": list(s.cvCorrect), "info": list(s.info),
                       "numFolds": s.numFolds})
        return st

    @classmethod
    def from_state(cls, t, st, uid=None, device=None) -> "RidgeClassificationModel":
        summ = None
        if "alphas" in st:
            summ = RidgeSummary(float(st["alpha"]), [float(v) for v in st["alphas"]], [int(v) for v in st["cvCorrect"]],
                                [int(v) for v in st["info"]], int(st["numFolds"]))
        return cls(t["coefficients"], t["intercepts"], float(st.get("alpha", 0.0)), summ, uid=uid, device=device)

    def __str__(self):
        return (f"RidgeClassificationModel (uid={self.uid}) with alpha={self.alpha:g}, {self.num_features} features, "
                f"{self.num_classes} classes")


class RidgeClassifier(Estimator, ClassifierParams):
    _param_names = ("alphas", "numFolds", "seed", "foldCol", "standardize", "featuresCol", "labelCol", "device")

    def __init__(self, alphas=None, numFolds: int = 5, seed: int = 0, foldCol: Optional[str] = None,
                 standardize: bool = True, featuresCol="features", labelCol="label", device=None):
        super().__init__(new_uid("RidgeClassifier"))
        self.alphas = RD.default_alphas() if alphas is None else [float(v) for v in alphas]
        self.numFolds, self.seed, self.foldCol, self.standardize = numFolds, seed, foldCol, standardize
        self.featuresCol, self.labelCol, self.device = featuresCol, labelCol, device

    def _folds(self, table: Optional[Table], N: int):
        """(host fold ids int64 [N], F): the distinct values of ``foldCol``, else ``kfold_ids``; one alpha or
        ``numFolds <= 1``: no folds."""
        alphas = [float(self.alphas)] if np.isscalar(self.alphas) else list(self.alphas)
        if self.foldCol is not None and table is not None and len(alphas) > 1:
            codes = np.unique(np.asarray(table[self.foldCol].data), return_inverse=True)[1].astype(np.int64)
            F = int(codes.max()) + 1 if codes.size else 1
            if F > RD.MAX_FOLDS:
                raise ValueError(f"RidgeClassifier: foldCol {self.foldCol!r} has {F} distinct values, at most "
                                 f"{RD.MAX_FOLDS} folds")
            return codes.reshape(-1), max(F, 1)
        if int(self.numFolds) <= 1 or len(alphas) == 1:
            return np.zeros(N, dtype=np.int64), 1
        return kfold_ids(N, int(self.numFolds), int(self.seed)).astype(np.int64), int(self.numFolds)

    def fit_tensors(self, X: torch.Tensor, y: torch.Tensor, K: int, fold=None, F: Optional[int] = None,
                    **kw) -> RidgeClassificationModel:
        if X.dim() != 2 or X.shape[0] < 1:
            raise ValueError("RidgeClassifier takes a non-empty [N, D] matrix")
        alphas = [float(self.alphas)] if np.isscalar(self.alphas) else [float(v) for v in self.alphas]
        if fold is None:
            fold, F = self._folds(None, X.shape[0])
        RD.check_range(X.shape[1], K, F, alphas, X.shape[0])
        Xf = X.float()
        mean, inv_std = RD.standardizer(Xf, bool(self.standardize))
        r = RD.fit(Xf, y, fold, int(F), alphas, mean, inv_std, int(K), **kw)
        m = RidgeClassificationModel(r.Wx, r.bx, r.alpha, RidgeSummary(r.alpha, alphas, r.cvCorrect, r.info, int(F)),
                                     uid=self.uid, device=X.device)
        m.featuresCol, m.labelCol = self.featuresCol, self.labelCol
        m.fit_result = r
        return m

    def fit(self, table: Table) -> RidgeClassificationModel:
        dev = resolve_device(self.device)
        X = features_tensor(table, self.featuresCol, dev)
        y = labels_tensor(table, self.labelCol, dev)
        K = num_label_classes(table, self.labelCol, dev)
        fold, F = self._folds(table, X.shape[0])
        return self.fit_tensors(X, y, K, fold, F)


__all__ = ["RidgeClassifier", "RidgeClassificationModel", "RidgeSummary"]
