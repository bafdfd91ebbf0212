"""DTWClassifier / DTWClassificationModel — k-nearest neighbours between RAW windows under banded dynamic
time warping; ``har/ops/dtw.py`` defines every operation.

A feature row is a flattened window, ``W`` samples of ``axes`` axes, time-major (the ``RAW*`` columns of
``raw_to_table(samples=True)``).  Fitting keeps the working windows (as given, or z-normalised per window and
axis) with their labels on the device.  A prediction is one ``dtw_search`` (the cost of every pair on one
lane, fused with the running top-k: the queries-by-references costs are never stored), one ``dtw_merge`` and
kNN's vote; nothing is read back from the device in between.  The band is ``radius`` samples, or ``band`` as a
fraction of the window (``radius = round(band * W)``).

The pair exclusion of the search evaluates a whole protocol with ONE search of a table against itself:
``leave_group_out`` (leave-one-out, leave-one-subject-out) and the CrossValidator's folds (``cv_predictions``,
maps over ``k`` / ``weights``).  Nothing is estimated from the table (the normalisation is per window), so
both equal refitting per group.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from ..data.table import Table
from ..ops import dtw as DT
from ..ops import knn as KN
from .base import ClassificationModel, ClassifierParams, Estimator, features_tensor, labels_tensor, new_uid, \
    num_label_classes, resolve_device


def resolve_radius(W: int, radius: Optional[int], band: Optional[float]) -> int:
    if radius is not None:
        return int(radius)
    return int(round(float(0.1 if band is None else band) * int(W)))


class DTWClassificationModel(ClassificationModel):
    _param_names = ("k", "radius", "weights", "axes", "normalize", "featuresCol", "labelCol")

    def __init__(self, Z: torch.Tensor, y: torch.Tensor, num_classes: int, k: int = 1, radius: int = 0,
                 weights: str = "uniform", normalize: str = "none", uid=None, device=None):
        super().__init__(uid or new_uid("DTWClassifier"))
        self.device = torch.device(device) if device is not None else Z.device
        if Z.dim() != 3:
            raise ValueError("DTWClassificationModel keeps its windows as [M, W, A]")
        self._Z = Z.to(device=self.device, dtype=torch.float32).contiguous()      # working windows, as fitted
        self._y = y.to(device=self.device, dtype=torch.int32).contiguous()
        self.num_classes = int(num_classes)
        self.k, self.radius, self.weights, self.normalize = int(k), int(radius), weights, normalize
        self.raw_settings: Optional[Dict] = None   # {"hz", "window_sec", "overlap"} of the raw stream (serving)
        if normalize not in DT.NORMALIZE:
            raise ValueError(f"DTW normalize must be one of {DT.NORMALIZE}, got {normalize!r}")
        DT.check_range(self.k, self.window, self.axes, self.radius, C=self.num_classes, M=self._Z.shape[0],
                       weights=weights)

    @property
    def window(self) -> int:
        return int(self._Z.shape[1])

    @property
    def axes(self) -> int:
        return int(self._Z.shape[2])

    @property
    def num_features(self) -> int:
        return self.window * self.axes

    @property
    def num_rows(self) -> int:
        return int(self._Z.shape[0])

    def _working_windows(self, X: torch.Tensor) -> torch.Tensor:
        X = X.to(device=self.device, dtype=torch.float32)
        if X.dim() == 2 and X.shape[1] == self.num_features:
            X = X.reshape(X.shape[0], self.window, self.axes)
        if X.dim() != 3 or tuple(X.shape[1:]) != (self.window, self.axes):
            raise ValueError(f"DTWClassificationModel takes [N, {self.num_features}] rows (windows of {self.window} "
                             f"samples, {self.axes} axes), got {tuple(X.shape)}")
        return DT.normalize(X, self.normalize)

    @staticmethod
    def _groups(exclude, N, M, dev):
        if exclude is None:
            return None, None
        qg, rg = (torch.as_tensor(g).to(device=dev, dtype=torch.int32).contiguous() for g in exclude)
        if qg.numel() != N or rg.numel() != M:
            raise ValueError("exclude = (qgroup [N], rgroup [M])")
        return qg, rg

    def kneighbors(self, X: torch.Tensor, k: Optional[int] = None, exclude=None, native: Optional[bool] = None):
        """(idx int32 [N, k] into the training windows, d2 fp32 [N, k] DTW costs), ascending."""
        Q = self._working_windows(X)
        qg, rg = self._groups(exclude, Q.shape[0], self.num_rows, self.device)
        return DT.neighbors(Q, self._Z, self.k if k is None else int(k), self.radius, qg, rg, native)

    def _search(self, Q, qg=None, rg=None, k=None, weights=None, native=None) -> KN.SearchResult:
        return DT.search(Q, self._Z, self.k if k is None else int(k), self.radius, native, qgroup=qg, rgroup=rg,
                         y=self._y, C=self.num_classes, weights=self.weights if weights is None else weights)

    def predict_raw(self, X: torch.Tensor) -> torch.Tensor:
        return self._search(self._working_windows(X)).vote.raw

    def predict_all(self, X: torch.Tensor):
        v = self._search(self._working_windows(X)).vote
        pred = v.pred if self.thresholds is None else self._predict_from_probability(v.prob)
        return v.raw, v.prob, pred

    def state(self) -> Dict:
        st = {"working_windows": self._Z.cpu(), "labels": self._y.cpu(), "k": self.k, "radius": self.radius,
              "weights": self.weights, "normalize": self.normalize}
        if self.raw_settings is not None:
            st["raw_settings"] = {k: float(v) for k, v in self.raw_settings.items()}
        return st

    @classmethod
    def from_state(cls, t, st, num_classes: int, uid=None, device=None) -> "DTWClassificationModel":
        m = cls(t["working_windows"], t["labels"], num_classes, int(st["k"]), int(st["radius"]), st["weights"],
                st["normalize"], uid=uid, device=device)
        m.raw_settings = st.get("raw_settings")
        return m

    def __str__(self):
        return (f"DTWClassificationModel (uid={self.uid}) with k={self.k}, radius={self.radius}, {self.num_rows} "
                f"windows of {self.window} x {self.axes}, {self.num_classes} classes")


class DTWClassifier(Estimator, ClassifierParams):
    _param_names = ("k", "radius", "band", "weights", "axes", "normalize", "featuresCol", "labelCol", "device")

    def __init__(self, k: int = 1, radius: Optional[int] = None, band: Optional[float] = 0.1, weights: str = "uniform",
                 axes: int = 3, normalize: str = "none", featuresCol="features", labelCol="label", device=None):
        super().__init__(new_uid("DTWClassifier"))
        self.k, self.radius, self.band, self.weights = k, radius, band, weights
        self.axes, self.normalize = axes, normalize
        self.featuresCol, self.labelCol, self.device = featuresCol, labelCol, device

    def _prep(self, table: Table):
        dev = resolve_device(self.device)
        return (features_tensor(table, self.featuresCol, dev), labels_tensor(table, self.labelCol, dev),
                num_label_classes(table, self.labelCol, dev))

    def fit_tensors(self, X: torch.Tensor, y: torch.Tensor, K: int) -> DTWClassificationModel:
        if X.dim() != 2 or X.shape[0] < 1:
            raise ValueError("DTWClassifier takes a non-empty [N, W * axes] matrix")
        DT.check_range(A=int(self.axes))
        Z = DT.as_windows(X.float(), int(self.axes))
        W = Z.shape[1]
        radius = resolve_radius(W, self.radius, self.band)
        DT.check_range(int(self.k), W, int(self.axes), radius, C=K, M=X.shape[0], weights=self.weights)
        m = DTWClassificationModel(DT.normalize(Z, self.normalize), y, K, int(self.k), radius, self.weights,
                                   self.normalize, uid=self.uid, device=X.device)
        m.featuresCol, m.labelCol = self.featuresCol, self.labelCol
        return m

    def fit(self, table: Table) -> DTWClassificationModel:
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
        idx, d2 = DT.neighbors(m._Z, m._Z, kmax, m.radius, g, g)
        votes = [KN.vote(idx, d2, m._y, K, s.weights, int(s.k)) for s in subs]
        return y, torch.stack([v.pred for v in votes]), torch.stack([v.raw for v in votes]), K


__all__ = ["DTWClassifier", "DTWClassificationModel"]
