"""KMeans / KMeansModel — MLlib's ``KMeans`` (Lloyd iterations, squared-Euclidean distance) with Spark's
parameter names; ``har/ops/kmeans.py`` defines every operation.

Engine: the rows are centred once (``Xc = X - mean``), then every iteration is ``kmeans_assign`` (scores on
the fp32 matrix cores, argmin, fixed-point cluster sums) followed by ``kmeans_update`` (new centres, ``h``,
the moved distance, the converged flag, the cost history and the zeroing of the accumulators, all on the
device).  On a GPU a fit of ``maxIter`` iterations is therefore enqueued without any device -> host read;
once the converged flag is set the remaining launches leave the state untouched.  The history, the
cluster sizes and ``numIter`` are read once after the fit.  The cluster sums are exact integers, so a fit
is bitwise reproducible and — under ``data_parallel(ctx)``, where each iteration all-reduces the flat
int64 accumulator buffer and the fp64 cost — centres, assignments and ``numIter`` are bitwise equal for
every world size (only the cost may differ in its last bits).

Initialisation: ``"random"`` takes the k rows with the smallest Philox keys of the row stream
``STREAM_KMEANS_INIT`` (identical on CPU and GPU and for any sharding); ``"k-means++"`` makes k
sequential D^2 draws — the running ``d2min`` comes from ``kmeans_assign`` against the newest centre, is
quantized to int64 so its cumulative sum is exact, and the draw is a Philox uniform located with
``searchsorted``; the chosen index never leaves the device.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from ..data.table import Column, Table
from ..ops import kmeans as KM
from ..ops import metrics as OM
from ..ops import rng
from .base import Estimator, Model, dp_allreduce, dp_rows, features_tensor, new_uid, resolve_device


@dataclass
class KMeansSummary:
    trainingCost: float = 0.0
    costHistory: List[float] = field(default_factory=list)
    clusterSizes: List[int] = field(default_factory=list)
    numIter: int = 0
    converged: bool = False
    k: int = 0
    predictions: Optional[torch.Tensor] = None   # int32 clusters of the (rank's) training rows

    def as_dict(self):
        return {"trainingCost": self.trainingCost, "costHistory": list(self.costHistory),
                "clusterSizes": list(self.clusterSizes), "numIter": self.numIter, "converged": self.converged,
                "k": self.k}


def cluster_label_map(k: int, device, pred: torch.Tensor, y: torch.Tensor, num_classes: int):
    """The cluster x label table, the majority label per cluster and the purity (``KMeansModel.label_map``;
    shared with ``GaussianMixtureModel``)."""
    n = max(int(k), int(num_classes))
    cm = OM.confusion_matrix(pred.to(device), y.to(device), n)[:int(k), :int(num_classes)]
    total = cm.sum()
    purity = float(cm.max(dim=1).values.sum().double() / total.double().clamp_min(1.0))
    return cm, cm.argmax(dim=1), purity


class KMeansModel(Model):
    _param_names = ("featuresCol", "predictionCol")
    featuresCol = "features"
    predictionCol = "prediction"

    def __init__(self, centers_centered: torch.Tensor, mean: torch.Tensor, summary: Optional[KMeansSummary] = None,
                 uid=None, device=None, label_map=None):
        super().__init__(uid or new_uid("KMeans"))
        self.device = torch.device(device) if device is not None else centers_centered.device
        self._Cw = centers_centered.to(device=self.device, dtype=torch.float32).contiguous()
        self.mean = mean.to(device=self.device, dtype=torch.float32).contiguous()
        self._h = KM.center_h(self._Cw)
        self.summary = summary or KMeansSummary(k=int(self._Cw.shape[0]))
        self.majority_labels = None if label_map is None else [int(v) for v in label_map]
        self.feature_cols = None   # the table columns the model was fitted on (None: the features column)

    @property
    def k(self) -> int:
        return int(self._Cw.shape[0])

    @property
    def num_features(self) -> int:
        return int(self._Cw.shape[1])

    def clusterCenters(self) -> torch.Tensor:
        """float32 [k, D] in the original coordinates."""
        return (self._Cw.double() + self.mean.double().view(1, -1)).float()

    def _working_rows(self, X: torch.Tensor) -> torch.Tensor:
        X = X.to(device=self.device, dtype=torch.float32)
        if X.dim() != 2 or X.shape[1] != self.num_features:
            raise ValueError(f"KMeansModel takes [N, {self.num_features}] rows, got {tuple(X.shape)}")
        return (X - self.mean.view(1, -1)).contiguous()

    def predict(self, X: torch.Tensor, native: Optional[bool] = None) -> torch.Tensor:
        """int64 cluster of every row (the lowest index among equally near centres)."""
        Xc = self._working_rows(X)
        if Xc.shape[0] == 0:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        return KM.assign(Xc, self._Cw, self._h, native, want_cost=False).assign.long()

    def computeCost(self, X: torch.Tensor) -> float:
        r = KM.assign(self._working_rows(X), self._Cw, self._h, None, want_cost=True)
        return float(KM.reduce_cost(r.part))

    def transform(self, table: Table) -> Table:
        pred = self.predict(features_tensor(table, self.featuresCol, self.device))
        return table.with_column(Column(self.predictionCol, "double", pred.double().cpu().numpy(),
                                        meta={"nullable": False}))

    def label_map(self, pred: torch.Tensor, y: torch.Tensor, num_classes: int):
        """(contingency int64 [k, num_classes] = rows of cluster c carrying label l, majority label per
        cluster [k], purity = the share of rows whose label is their cluster's majority label), taken
        through the confusion kernel of ``ops/metrics.py``."""
        cm, majority, purity = cluster_label_map(self.k, self.device, pred, y, num_classes)
        self.majority_labels = [int(v) for v in majority.tolist()]
        return cm, majority, purity

    def state(self):
        s = self.summary
        out = {"centers_centered": self._Cw.cpu(), "mean": self.mean.cpu(),
               "cost_history": torch.tensor(s.costHistory, dtype=torch.float64),
               "cluster_sizes": torch.tensor(s.clusterSizes, dtype=torch.int64),
               "training_cost": torch.tensor([s.trainingCost], dtype=torch.float64),
               "num_iter": torch.tensor([s.numIter, int(s.converged)], dtype=torch.int64)}
        if self.majority_labels is not None:
            out["majority_labels"] = torch.tensor(self.majority_labels, dtype=torch.int64)
        out["feature_cols"] = None if self.feature_cols is None else list(self.feature_cols)
        return out

    @classmethod
    def from_state(cls, st, uid=None, device=None) -> "KMeansModel":
        ni = st["num_iter"].tolist()
        summ = KMeansSummary(float(st["training_cost"][0]), [float(v) for v in st["cost_history"].tolist()],
                             [int(v) for v in st["cluster_sizes"].tolist()], int(ni[0]), bool(ni[1]),
                             int(st["centers_centered"].shape[0]))
        lm = st["majority_labels"].tolist() if "majority_labels" in st else None
        return cls(st["centers_centered"], st["mean"], summ, uid=uid, device=device, label_map=lm)

    def __str__(self):
        return f"KMeansModel (uid={self.uid}) with k={self.k}"


class KMeans(Estimator):
    _param_names = ("k", "maxIter", "tol", "initMode", "seed", "featuresCol", "predictionCol", "weightCol", "device")

    def __init__(self, k: int = 2, maxIter: int = 20, tol: float = 1e-4, initMode: str = "k-means++", seed: int = 0,
                 featuresCol="features", predictionCol="prediction", weightCol=None, device=None):
        super().__init__(new_uid("KMeans"))
        self.k, self.maxIter, self.tol, self.initMode, self.seed = k, maxIter, tol, initMode, seed
        self.featuresCol, self.predictionCol, self.weightCol, self.device = featuresCol, predictionCol, weightCol, device

    def fit(self, table: Table) -> KMeansModel:
        dev = resolve_device(self.device)
        X = features_tensor(table, self.featuresCol, dev)
        w = None
        if self.weightCol is not None:
            w = torch.as_tensor(np.asarray(table[self.weightCol].data)).to(dev)
        model = self._fit_tensors(X, w, row_range=dp_rows(X.shape[0]), allreduce=dp_allreduce())
        model.featuresCol, model.predictionCol = self.featuresCol, self.predictionCol
        return model

    def fit_tensors(self, X, weights=None) -> KMeansModel:
        return self._fit_tensors(X, weights)

    def fit_features(self, X: torch.Tensor, weights=None) -> KMeansModel:
        """``fit`` on a feature matrix every rank holds: row-sharded under ``data_parallel(ctx)``."""
        return self._fit_tensors(X.to(resolve_device(self.device)), weights, row_range=dp_rows(X.shape[0]),
                                 allreduce=dp_allreduce())

    # ------------------------------------------------------------------ checks
    def _check(self, N: int, D: int):
        k = int(self.k)
        if k < 1:
            raise ValueError(f"KMeans k must be >= 1, got {k}")
        KM.check_native_range(k, D, N)
        if k > N:
            raise ValueError(f"KMeans k = {k} exceeds the {N} rows")
        if int(self.maxIter) < 0 or float(self.tol) < 0.0:
            raise ValueError("maxIter and tol must be >= 0")
        if self.initMode not in ("k-means++", "random"):
            raise ValueError(f"initMode must be 'k-means++' or 'random', got {self.initMode!r}")

    @staticmethod
    def _weights(weights, N: int, dev) -> Optional[torch.Tensor]:
        if weights is None:
            return None
        w = torch.as_tensor(weights).to(dev)
        if w.numel() != N:
            raise ValueError("one weight per row")
        wl = w.long()
        # the fit's one read before its first kernel: integer weights >= 0 within the fixed-point budget
        lo, tot, frac = int(wl.min()), int(wl.sum()), bool((w.double() != wl.double()).any())
        if lo < 0 or frac or not 0 < tot <= KM.MAX_WEIGHT:
            raise ValueError(f"KMeans weights must be integers >= 0 with a total in 1..{KM.MAX_WEIGHT}")
        return wl.to(torch.int32).contiguous()

    # ------------------------------------------------------------------ initialisation (working coordinates)
    def _init_random(self, Xc: torch.Tensor) -> torch.Tensor:
        rows = KM.random_init_rows(int(self.seed), int(self.k), Xc.shape[0])
        return Xc.index_select(0, torch.from_numpy(rows).to(Xc.device)).contiguous()

    def _init_pp(self, Xc: torch.Tensor, nrm: torch.Tensor, nscale: torch.Tensor, w, native: bool) -> torch.Tensor:
        N, D = Xc.shape
        k, dev = int(self.k), Xc.device
        u = torch.from_numpy(rng.uniform(int(self.seed), rng.STREAM_KMEANS_PP, np.arange(k, dtype=np.uint64))).to(dev)
        wl = torch.ones(N, dtype=torch.int64, device=dev) if w is None else w.long()
        dscale = nscale.double() * 0.25          # d2 <= 4 max ||x||^2: the quantized sum stays below 2^36 * weight
        C = torch.zeros(k, D, dtype=torch.float32, device=dev)
        d2min = None
        for j in range(k):
            q = wl if d2min is None else torch.round(d2min.double() * dscale).long() * wl
            cum = q.cumsum(0)
            total = cum[-1]
            target = torch.minimum((u[j] * total.double()).floor().long(), total - 1).reshape(1)
            idx = torch.searchsorted(cum, target, right=True).clamp_(max=N - 1)
            c = Xc.index_select(0, idx).contiguous()                      # [1, D]
            C[j] = c[0]
            h = (0.5 * nrm.index_select(0, idx)).float()
            d2 = KM.assign(Xc, c, h, native, want_cost=False).d2
            d2min = d2 if d2min is None else torch.minimum(d2min, d2)
            d2min.index_fill_(0, idx, 0.0)                                 # a chosen row is never drawn again
        return C

    # ------------------------------------------------------------------ the fit
    def _fit_tensors(self, X, weights=None, native=None, initial_centers=None, row_range=None,
                     allreduce=None) -> KMeansModel:
        """The fit.  Private knobs of the probe and the tests: ``native=False`` runs the PyTorch definitions on
        GPU tensors, ``initial_centers`` [k, D] (original coordinates) replaces the initialisation.
        ``row_range`` / ``allreduce`` are the data-parallel form: ``X`` is the whole table on every rank (so
        the column means, the scales and the initialisation are the single-process ones), the rank iterates
        over rows [lo, hi) and the accumulators are summed over the ranks."""
        if X.dim() != 2:
            raise ValueError("KMeans takes a [N, D] matrix")
        N, D = X.shape
        self._check(N, D)
        dev = X.device
        native = X.is_cuda if native is None else bool(native)
        k, M = int(self.k), int(self.maxIter)
        w_all = self._weights(weights, N, dev)
        Xf = X.float()
        mean = KM.column_means(Xf)
        Xc_all = (Xf - mean.view(1, D)).contiguous()
        scale = KM.feature_scales(Xc_all)
        nrm = KM.row_norms(Xc_all)
        nscale = KM.norm_scale(nrm)
        if initial_centers is not None:
            C0 = torch.as_tensor(initial_centers).to(device=dev, dtype=torch.float32)
            if tuple(C0.shape) != (k, D):
                raise ValueError(f"initial_centers must be [{k}, {D}]")
            C0 = (C0 - mean.view(1, D)).contiguous()
        elif self.initMode == "random":
            C0 = self._init_random(Xc_all)
        else:
            C0 = self._init_pp(Xc_all, nrm, nscale, w_all, native)
        lo, hi = (0, N) if row_range is None else (int(row_range[0]), int(row_range[1]))
        Xc = Xc_all if (lo, hi) == (0, N) else Xc_all[lo:hi].contiguous()
        w = None if w_all is None else w_all[lo:hi].contiguous()
        n = hi - lo

        st = KM.FitState.alloc(C0, M)
        nb = max(1, -(-n // KM.rows_per_block())) if native else 1
        part = torch.zeros(nb, dtype=torch.float64, device=dev)
        tol2 = float(self.tol) ** 2

        def one_pass(want_assign: bool):
            if n > 0:
                r = KM.assign(Xc, st.C, st.h, native, w=w, scale=scale, nscale=nscale, acc=st.acc,
                              want_assign=want_assign, want_cost=True, part_out=part)
            else:
                r = KM.AssignResult(torch.zeros(0, dtype=torch.int32, device=dev),
                                    torch.zeros(0, dtype=torch.float32, device=dev), torch.zeros_like(part))
            cost = r.part
            if allreduce is not None:
                cost = KM.reduce_cost(cost).reshape(1).clone()
                allreduce(st.acc)
                allreduce(cost)
            return r, cost

        for _ in range(M):
            _, cost = one_pass(False)
            KM.update(st, scale, cost, tol2, M, native)
        # the final pass: the training rows' clusters, the sizes and the cost under the final centres
        r, cost = one_pass(True)
        # ---- the fit's reads ----
        it, conv = (int(v) for v in st.state.tolist())
        sizes = KM.acc_views(st.acc, k, D)[1].tolist()
        summ = KMeansSummary(float(KM.reduce_cost(cost)), [float(v) for v in st.cost_hist[:it].tolist()],
                             [int(v) for v in sizes], it, bool(conv), k, r.assign)
        return KMeansModel(st.C, mean, summ, uid=self.uid, device=dev)


def kmeans_feature_cols(encoding: str):
    """The dense numeric columns ``main.py --kmeans`` clusters: the whole features vector of the numeric
    encodings (None), the ten numeric columns next to the one-hot peaks of the reference encoding."""
    from ..features import wisdm

    return list(wisdm.NUMERIC_COLS) if encoding == "reference" else None


def table_features(table: Table, cols, device) -> torch.Tensor:
    if cols is None:
        return features_tensor(table, "features", device)
    return torch.as_tensor(np.ascontiguousarray(table.numeric_matrix(list(cols), dtype=np.float32))).to(device)


__all__ = ["KMeans", "KMeansModel", "KMeansSummary", "kmeans_feature_cols", "table_features"]
